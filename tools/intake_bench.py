#!/usr/bin/env python
"""What the frame intake costs, and what it replaces (yolo_amd.intake.FrameIntake, csrc/intake.hip).

  kernel    yolo_warp_u8_to_nchw alone on resident uint8 frames, by HIP events: 1920x1080 -> 416^2 bs 32, 1280x720 -> 608^2 bs 64,
            640x360 -> 416^2 bs 32.  Algorithmic bytes = the source bytes inside the footprint once (the whole frame: clip 1) plus
            the fp32 output; GB/s = those bytes over the median kernel time.  (A downscale reads a fraction of the source PIXELS,
            but every cache line of the footprint, so the whole frame is the honest denominator.)
  pipeline  D53 at 416^2 bs 32 (BASELINE configs[1]'s shape; --dtype, tune='auto'): forward -> predict on a resident fp32 tensor,
            next to FrameIntake -> forward -> predict from resident 1080p uint8 frames and from HOST 1080p frames (the pinned
            staging copy, the upload and the kernel inside the step).
  host      the route the intake replaces, on the same box: torch-CPU interpolate (bilinear, --threads threads, default 16) of
            the uint8 frames to fp32 416^2 / 255 plus the fp32 upload; wall clock around a device synchronise.  This is the
            comparison for "was it worth it", not the code under test.

The parent process never opens the GPU: every step runs as ONE fresh child process at a time under its own `timeout`, and the
first step that fails ends the run.  Writes profiles/intake_bench.json (or --out).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (((1080, 1920), (416, 416), 32), ((720, 1280), (608, 608), 64), ((360, 640), (416, 416), 32))
STEPS = (('kernel', 240), ('pipeline', 420), ('host', 300))          # (step, seconds allowed)


def algorithmic_bytes(src_hw, dst_hw, batch, C=3):
    return batch * (src_hw[0] * src_hw[1] * C + C * dst_hw[0] * dst_hw[1] * 4)


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def _frames(src_hw, batch, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (batch,) + tuple(src_hw) + (3,), generator=g, dtype=torch.uint8)


def step_kernel(args, dev):
    import torch
    from yolo_amd.intake import FrameIntake
    out = []
    for k, (src_hw, dst_hw, batch) in enumerate(CONFIGS):
        if args.config is not None and k != args.config:
            continue
        frames = _frames(src_hw, batch, k).to(dev)
        intake = FrameIntake(dst_hw, device=dev)
        events = []
        for i in range(args.warmup + args.iters):
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e[0].record()
            intake(frames)
            e[1].record()
            if i >= args.warmup:
                events.append(e)
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in events]
        nbytes = algorithmic_bytes(src_hw, dst_hw, batch)
        r = dict(_stat(ms), src=list(src_hw), dst=list(dst_hw), batch=batch, algorithmic_bytes=nbytes, iters=args.iters)
        r['gb_per_s'] = nbytes / (r['median_ms'] * 1e-3) / 1e9
        r['images_per_s'] = batch / (r['median_ms'] * 1e-3)
        out.append(r)
        print(json.dumps(r), flush=True)
        del frames, intake
        torch.cuda.empty_cache()
    return out


def step_pipeline(args, dev):
    import torch
    from oracle import graph as og, detect as od
    from yolo_amd.net import CarNet
    from yolo_amd.detect import Detector
    from yolo_amd.intake import FrameIntake
    src_hw, size, batch = CONFIGS[0]
    spec = og.spec_d53()
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    net = CarNet(spec, dtype=args.dtype, device=dev).initialize(seed=1234)
    det = Detector(spec, size, steps, device=dev)
    intake = FrameIntake(size, device=dev)
    host = _frames(src_hw, batch, 0)
    resident_u8 = host.to(dev)
    x = intake(resident_u8).clone()
    routes = {'forward_predict_resident_f32': lambda: det.predict_device(net(x)),
              'intake_forward_predict_resident_u8': lambda: det.predict_device(net(intake(resident_u8))),
              'intake_forward_predict_host_u8': lambda: det.predict_device(net(intake(host)))}
    out = {'net': 'D53', 'dtype': args.dtype, 'tune': 'auto', 'src': list(src_hw), 'size': list(size), 'batch': batch,
           'iters': args.iters, 'timed': 'HIP events around the whole step, no host wait inside the loop except the staging '
           "buffer's own event in the host route"}
    for name, fn in routes.items():
        events = []
        for i in range(args.warmup + args.iters):
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e[0].record()
            fn()
            e[1].record()
            if i >= args.warmup:
                events.append(e)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.iters):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.iters
        out[name] = dict(_stat([a.elapsed_time(b) for a, b in events]), wall_ms_per_step=wall * 1e3, images_per_s_wall=batch / wall)
        print(name, json.dumps(out[name]), flush=True)
    return out


def step_host(args, dev):
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(args.threads)
    out = []
    for k, (src_hw, dst_hw, batch) in enumerate(CONFIGS):
        host = _frames(src_hw, batch, k)
        ms, resize_ms = [], []
        for i in range(1 + args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = F.interpolate(host.permute(0, 3, 1, 2).float(), size=dst_hw, mode='bilinear', align_corners=False) / 255.0
            t1 = time.perf_counter()
            xd = x.to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i:
                ms.append((t2 - t0) * 1e3)
                resize_ms.append((t1 - t0) * 1e3)
        r = dict(_stat(ms), src=list(src_hw), dst=list(dst_hw), batch=batch, threads=args.threads, iters=args.host_iters,
                 resize_median_ms=_stat(resize_ms)['median_ms'])
        r['images_per_s'] = batch / (r['median_ms'] * 1e-3)
        out.append(r)
        print(json.dumps(r), flush=True)
        del xd
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/intake_bench.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    res = {'kernel': step_kernel, 'pipeline': step_pipeline, 'host': step_host}[args.child](args, dev)
    if args.child_out:
        with open(args.child_out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'result': res}, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dtype', default='bf16', help='arithmetic path of the net in the pipeline step')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-iters', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16, help='CPU threads of the host route')
    ap.add_argument('--steps', default=','.join(s for s, _ in STEPS))
    ap.add_argument('--config', type=int, default=None, help='kernel step: only CONFIGS[k] (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'intake_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {'tool': 'tools/intake_bench.py', 'warmup': args.warmup}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step, seconds in STEPS:
        if step not in args.steps.split(','):
            continue
        part = '%s.%s.part' % (args.out, step)
        cmd = ['timeout', '-k', '10', str(seconds), sys.executable, os.path.abspath(__file__), '--child', step, '--child-out', part,
               '--dtype', args.dtype, '--warmup', str(args.warmup), '--iters', str(args.iters), '--host-iters', str(args.host_iters),
               '--threads', str(args.threads)]
        if args.config is not None:
            cmd += ['--config', str(args.config)]
        rc = subprocess.call(cmd)
        if rc != 0:                                           # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.exit('intake_bench: step %r ended with status %d; stopping' % (step, rc))
        with open(part) as f:
            got = json.load(f)
        os.remove(part)
        res['device'] = got['device']
        res[step] = got['result']
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
