#!/usr/bin/env python
"""What the train-mode forward of the OCR DenseNet costs (yolo_amd.dense: OCRNet.forward(x, training=True); csrc/dense_train.hip).

  OCRNet 32 / 12 / [6, 12, 24] at 160x384, N = 1, 16 and 100 (the reference's OCR batch), dtype bf16 and f32, Xavier parameters, one
  resident random input per N.  Per point, by HIP events after warm-up, each in a timed window of its own:
    train      one forward(x, training=True): batch statistics, folds, running update, the inference kernels
    eval       one forward(x) of the same build: the yardstick; ratio = train / eval
    bn2_stats  the yolo_dense_bottleneck_stats calls of one training forward alone (the recomputed 1x1 and its reduction, on the
               buffers the training forward left): share = bn2_stats / train -- the input to a backward pass's decision whether to
               store the bottleneck instead of recomputing it
  train_launches stands next to launches.  No target is set: nobody has measured this before.  The mean shader clock over each
  timed window is recorded beside it (bench.py's Telemetry).

The parent process never opens the GPU: the measurement runs as one fresh child process under its own `timeout`.  Writes
profiles/ocr_train_fwd_bench.json (or --out).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = (160, 384)
BATCHES = (1, 16, 100)
SECONDS = 540


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def _timed(call, args):
    """Warm up, size a window of at least --window-ms, then time every call of it with a pair of events."""
    import torch
    from bench import Telemetry
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
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
    r = dict(_stat([a.elapsed_time(b) for a, b in events]), calls=calls)
    r.update(tel.stop())
    return r


def measure(args):
    import torch
    from yolo_amd import lib as L
    from yolo_amd.dense import OCRNet
    if not torch.cuda.is_available():
        sys.exit('tools/ocr_train_fwd_bench.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    res = {'device_name': torch.cuda.get_device_name(0), 'clock': 'HIP events', 'warmup_calls': args.warmup, 'window_ms': args.window_ms,
           'net': 'OCRNet 32 / 12 / [6, 12, 24]', 'size': list(SIZE)}
    for dtype in ('bf16', 'f32'):
        net = OCRNet(dtype=dtype, device=dev).initialize(0)
        for n in BATCHES:
            x = torch.rand((n, 3) + SIZE, generator=torch.Generator().manual_seed(n)).to(dev)
            train = _timed(lambda: net.forward(x, training=True), args)
            # (the plan's own launch list: the bottleneck-statistics entries of one training forward, on the buffers it left)
            stats_ops = [(name, fn, a) for name, fn, a in net._train_plan(x).ops if name.endswith('bn2.stats')]
            assert len(stats_ops) == sum(net.block_config)

            def bn2_stats():
                st = L.stream_ptr()
                for name, fn, a in stats_ops:
                    L.check(fn(*a, st), name)
            stats = _timed(bn2_stats, args)
            ev = _timed(lambda: net(x), args)                      # (its first warm-up call re-folds the running statistics)
            r = {'dtype': dtype, 'batch': n, 'launches': net.launches, 'train_launches': net.train_launches, 'train': train, 'eval': ev,
                 'bn2_stats': stats, 'bn2_stats_launches': 2 * len(stats_ops),
                 'ratio_train_over_eval': train['median_ms'] / ev['median_ms'],
                 'bn2_stats_share_of_train': stats['median_ms'] / train['median_ms'],
                 'train_images_per_s': n * 1e3 / train['median_ms']}
            print(json.dumps(r), flush=True)
            res['ocr_bs%d_%s' % (n, dtype)] = r
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--window-ms', type=float, default=1000.0, help='least length of a timed window of calls')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ocr_train_fwd_bench.json'))
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_out:
        with open(args.child_out, 'w') as f:
            json.dump(measure(args), f)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    part = args.out + '.part'
    cmd = ['timeout', '-k', '10', str(SECONDS), sys.executable, os.path.abspath(__file__), '--child-out', part, '--warmup', str(args.warmup),
           '--iters', str(args.iters), '--window-ms', str(args.window_ms)]
    rc = subprocess.call(cmd)
    if rc != 0:
        sys.exit('tools/ocr_train_fwd_bench.py: the measurement ended with status %d' % rc)
    with open(part) as f:
        res = {'tool': 'tools/ocr_train_fwd_bench.py', 'device': json.load(f)}
    os.remove(part)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
