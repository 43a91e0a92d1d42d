#!/usr/bin/env python
"""What fitting anchors on the device costs (yolo_anchor_kmeans, csrc/anchors.hip), and the numpy route beside it.

Two points, on seeded synthetic box sizes (log-uniform area 0.02..0.6, log-normal aspect) and seeded starts:

  reference  the reference's own size: n = 1000, k = 9, one restart, max_iters = 10 (iou_kmeans.py:11 makes exactly 10 rounds)
  large      n = 100 000, k = 9, 32 restarts side by side, each to convergence (max_iters = 300)

  device  the one yolo_anchor_kmeans launch of each point, by HIP events on the device's own clock after `--warmup` untimed
          launches; medians and minima over at least `--iters` launches and at least `--window-ms` of back-to-back launches (a
          shorter window measures the clock's ramp as much as the kernel); the rounds each restart took are recorded, and the mean
          shader clock over the timed region (bench.py's Telemetry).  The inputs are resident: the upload and the init draw are not in the figure.
  host    fit_anchors' device=None route (numpy, one host thread) on the same rows and the same starts: wall clock of one run
          (`--host-iters` runs at the reference point).  The parent commit has no device route to compare with.

The GPU's clocks are whatever the machine runs at: the tool sets nothing.  The parent process never opens the GPU: each step runs
as ONE fresh child process under its own `timeout`, and the first step that fails ends the run.  Writes profiles/anchor_bench.json
(or --out).  The device step needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = (('reference', dict(n=1000, k=9, restarts=1, max_iters=10)), ('large', dict(n=100000, k=9, restarts=32, max_iters=300)))
STEPS = (('device', 240), ('host', 540))                  # (step, seconds allowed)


def synthetic_sizes(n, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    area = np.exp(rng.uniform(np.log(0.02), np.log(0.6), n))
    aspect = np.exp(rng.normal(0.0, 0.35, n))
    return np.stack([np.sqrt(area * aspect), np.sqrt(area / aspect)], axis=1).astype(np.float32)


def starts(rows, k, restarts, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    return np.stack([rows[rng.choice(len(rows), k, replace=False)] for _ in range(restarts)])


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def step_device(args):
    import torch
    from bench import Telemetry
    from yolo_amd import lib as L
    if not torch.cuda.is_available():
        sys.exit('tools/anchor_bench.py --steps device needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    lib = L.load()
    res = {'device_name': torch.cuda.get_device_name(0), 'clock': 'HIP events', 'warmup_launches': args.warmup,
           'sizing_launches_untimed': args.iters, 'window_ms': args.window_ms}
    for name, p in POINTS:
        n, k, R = p['n'], p['k'], p['restarts']
        rows = synthetic_sizes(n)
        d_rows, d_init = torch.from_numpy(rows).to(dev), torch.from_numpy(starts(rows, k, R)).to(dev)
        cent = torch.empty((R, k, 2), dtype=torch.float32, device=dev)
        counts = torch.empty((R, k), dtype=torch.int32, device=dev)
        mean = torch.empty((R,), dtype=torch.float64, device=dev)
        small = torch.empty((2 * R + 1,), dtype=torch.int32, device=dev)
        ws = torch.empty((lib.yolo_anchor_workspace_bytes(n, R, k),), dtype=torch.uint8, device=dev)

        def launch():
            L.check(lib.yolo_anchor_kmeans(L.ptr(d_rows), 2, n, L.ptr(d_init), R, k, p['max_iters'], L.ptr(cent), L.ptr(counts), L.ptr(mean),
                                           small.data_ptr(), small.data_ptr() + 4 * R, small.data_ptr() + 8 * R, L.ptr(ws), L.stream_ptr()),
                    'anchor_kmeans')
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()                              # (sizes the timed window: untimed, and warm-up as well)
        for _ in range(args.iters):
            launch()
        torch.cuda.synchronize()
        per_ms = (time.perf_counter() - t0) * 1e3 / args.iters
        launches = int(min(20000, max(args.iters, args.window_ms / per_ms)))
        tel = Telemetry(0).start()
        events = []
        for _ in range(launches):
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e[0].record()
            launch()
            e[1].record()
            events.append(e)
        torch.cuda.synchronize()
        r = dict(p, kmeans=_stat([a.elapsed_time(b) for a, b in events]), launches=launches)
        r.update(tel.stop())
        it = small[:R].cpu().numpy()
        r.update(rounds_min=int(it.min()), rounds_max=int(it.max()), rounds_total=int(it.sum()),
                 converged=int(small[R:2 * R].sum().item()), best_mean_iou=float(mean.max().item()))
        # one restart is one workgroup: its time is the slowest restart's rounds (+ 1 pass when max_iters cut it)
        r['us_per_round_of_the_slowest_restart'] = r['kmeans']['median_ms'] * 1e3 / max(1, int(it.max()))
        print(name, json.dumps(r), flush=True)
        res[name] = r
    return res


def step_host(args):
    from yolo_amd import anchors as am
    res = {'clock': 'time.perf_counter', 'host_threads': 1, 'route': 'yolo_amd.anchors._kmeans_host per restart (what fit_anchors(device=None) runs)'}
    for name, p in POINTS:
        rows = synthetic_sizes(p['n'])
        init = starts(rows, p['k'], p['restarts'])
        runs = args.host_iters if name == 'reference' else 1
        ms, rounds = [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            out = [am._kmeans_host(rows, init[r], p['max_iters']) for r in range(p['restarts'])]
            ms.append((time.perf_counter() - t0) * 1e3)
            rounds = [int(o[3]) for o in out]
        r = dict(p, kmeans=_stat(ms), runs=runs, rounds_max=max(rounds), rounds_total=sum(rounds), best_mean_iou=max(float(o[2]) for o in out))
        print(name, json.dumps(r), flush=True)
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--window-ms', type=float, default=1500.0, help='least length of a timed window of launches')
    ap.add_argument('--host-iters', type=int, default=5, help='runs of the numpy route at the reference point')
    ap.add_argument('--steps', default=','.join(s for s, _ in STEPS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'anchor_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        got = {'device': step_device, 'host': step_host}[args.child](args)
        with open(args.child_out, 'w') as f:
            json.dump(got, f)
        return
    res = {'tool': 'tools/anchor_bench.py'}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step, seconds in STEPS:
        if step not in args.steps.split(','):
            continue
        part = '%s.%s.part' % (args.out, step)
        cmd = ['timeout', '-k', '10', str(seconds), sys.executable, os.path.abspath(__file__), '--child', step, '--child-out', part,
               '--warmup', str(args.warmup), '--iters', str(args.iters), '--host-iters', str(args.host_iters), '--window-ms', str(args.window_ms)]
        rc = subprocess.call(cmd)
        if rc != 0:                                           # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.exit('anchor_bench: step %r ended with status %d; stopping' % (step, rc))
        with open(part) as f:
            res[step] = json.load(f)
        os.remove(part)
        with open(args.out, 'w') as f:                        # (rewritten after every step: a later step's failure keeps the earlier figures)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
