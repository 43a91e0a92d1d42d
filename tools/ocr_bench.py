#!/usr/bin/env python
"""What reading a plate costs (yolo_amd.dense: OCRNet + PlateReader, LPDenseNet; csrc/dense.hip, csrc/ocr.hip).

  device   HIP-event time of one PlateReader.read_device call (OCRNet 32 / 12 / [6, 12, 24] at 160x384 + yolo_ocr_decode) at N = 1, 8, 32
           and of one LPDenseNet forward with licence_plate/v2/spec.yaml's body (64 / 16 / [6, 12, 24, 16], 3 classes) at 320x512 bs 1,
           for dtype bf16 and f32, with the launch count of each.  Xavier parameters (initialize), resident random inputs; the
           mean shader clock over each timed region is recorded beside it (bench.py's Telemetry).  Nobody has measured these nets
           before and no target is set.  The reference publishes one LPD figure (~50 FPS on a Xavier); it
           is named here only because it exists: another net version, another machine.
  host     the torch-CPU restatement (tests/dense_ref.py, float32) on the same inputs and parameters, wall clock: what there
           was to run before, not the code under test.

The parent process never opens the GPU: each step runs as one fresh child process under its own `timeout`, and the first step that
fails ends the run.  Writes profiles/ocr_bench.json (or --out).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LPD_V2 = {'num_init_features': 64, 'growth_rate': 16, 'block_config': [6, 12, 24, 16], 'LP_num_class': 3}
POINTS = (('ocr', 1), ('ocr', 8), ('ocr', 32), ('lpd_v2', 1))
SIZES = {'ocr': (160, 384), 'lpd_v2': (320, 512)}
STEPS = (('device', 420), ('host', 300))            # (step, seconds allowed)


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def _input(kind, n):
    import torch
    return torch.rand((n, 3) + SIZES[kind], generator=torch.Generator().manual_seed(n))


def step_device(args):
    import torch
    from bench import Telemetry
    from yolo_amd.dense import LPDenseNet, OCRNet, PlateReader
    if not torch.cuda.is_available():
        sys.exit('tools/ocr_bench.py --steps device needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    res = {'device_name': torch.cuda.get_device_name(0), 'clock': 'HIP events', 'warmup_calls': args.warmup, 'window_ms': args.window_ms}
    for dtype in ('bf16', 'f32'):
        ocr = PlateReader(OCRNet(dtype=dtype, device=dev).initialize(0))
        lpd = LPDenseNet(LPD_V2, dtype=dtype, device=dev).initialize(0)
        for kind, n in POINTS:
            x = _input(kind, n).to(dev)
            call = (lambda: ocr.read_device(x)) if kind == 'ocr' else (lambda: lpd(x))
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()                          # (sizes the timed window: untimed)
            for _ in range(args.iters):
                call()
            torch.cuda.synchronize()
            per_ms = (time.perf_counter() - t0) * 1e3 / args.iters
            calls = int(min(5000, max(args.iters, args.window_ms / per_ms)))
            tel = Telemetry(0).start()
            events = []
            for _ in range(calls):
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                e[0].record()
                call()
                e[1].record()
                events.append(e)
            torch.cuda.synchronize()
            r = {'net': kind, 'dtype': dtype, 'batch': n, 'size': list(SIZES[kind]), 'calls': calls,
                 'launches': ocr.launches if kind == 'ocr' else lpd.launches, 'call': _stat([a.elapsed_time(b) for a, b in events])}
            r['images_per_s'] = n * 1e3 / r['call']['median_ms']
            r.update(tel.stop())
            print(json.dumps(r), flush=True)
            res['%s_bs%d_%s' % (kind, n, dtype)] = r
    return res


def step_host(args):
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import dense_ref as R
    from yolo_amd import dense as D
    res = {'clock': 'time.perf_counter', 'route': 'tests/dense_ref.py, float32, torch on the CPU', 'torch_threads': torch.get_num_threads()}
    nets = {'ocr': (dict(F0=32, G=12, blocks=[6, 12, 24], bn_size=4), ('ocr', 10, 34), R.ocr_forward),
            'lpd_v2': (dict(F0=64, G=16, blocks=[6, 12, 24, 16], bn_size=4), ('lpd', 3), R.lpd_forward)}
    for kind, n in POINTS:
        net, head, fwd = nets[kind]
        P = R.random_params(D.dense_param_shapes(net['F0'], net['G'], net['blocks'], 4, head), 0)
        x, mode, ms = _input(kind, n), R.Mode('f32'), []
        for _ in range(args.host_iters + 1):
            t0 = time.perf_counter()
            fwd(net, P, x, mode)
            ms.append((time.perf_counter() - t0) * 1e3)
        r = {'net': kind, 'batch': n, 'call': _stat(ms[1:]), 'runs': args.host_iters}
        print(json.dumps(r), flush=True)
        res['%s_bs%d' % (kind, n)] = r
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--window-ms', type=float, default=1500.0, help='least length of a timed window of calls')
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--steps', default=','.join(s for s, _ in STEPS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ocr_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        got = {'device': step_device, 'host': step_host}[args.child](args)
        with open(args.child_out, 'w') as f:
            json.dump(got, f)
        return
    res = {'tool': 'tools/ocr_bench.py', 'reference_lpd_figure': 'about 50 FPS on a Xavier (SURVEY.md section 5): exists, not comparable'}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step, seconds in STEPS:
        if step not in args.steps.split(','):
            continue
        part = '%s.%s.part' % (args.out, step)
        cmd = ['timeout', '-k', '10', str(seconds), sys.executable, os.path.abspath(__file__), '--child', step, '--child-out', part,
               '--warmup', str(args.warmup), '--iters', str(args.iters), '--host-iters', str(args.host_iters), '--window-ms', str(args.window_ms)]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit('tools/ocr_bench.py: step %s ended with status %d; nothing further is started' % (step, rc))
        with open(part) as f:
            res[step] = json.load(f)
        os.remove(part)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
