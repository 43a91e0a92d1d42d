#!/usr/bin/env python
"""What drawing the licence plates of a training batch on the device costs, and what it replaces (LPGenerator.add_device,
csrc/plates.hip).

On seeded synthetic glyph images written to a temporary directory, colour augmenter on, r_max (45, 60, 45), at 416 x 416, batch 64:

  kernels  yolo_plate_compose, yolo_plate_stats and yolo_plate_render each alone, by HIP events, on one seeded batch of rows; the
           render pass also with the noise scale zeroed (what the Philox work costs).  Algorithmic bytes of the render pass =
           24 B per output pixel (12 read, 12 written); every kernel's GB/s = THOSE bytes over its median time.
  device   a whole add_device call: the host's draws (draw_params, also timed alone), the pinned upload, the three kernels; wall
           clock per call around a device synchronise.
  host     the route it replaces on the same batch: LPGenerator.add = add_host (PIL + numpy, one image at a time) + the fg / mask
           upload + yolo_composite_unit; wall clock per call around a device synchronise.
  train    a bf16 CarLPNet Trainer.train_step (D53, tune='auto') fed by each route, and on a resident batch: wall clock per step.

Timing: `--warmup` untimed calls, then `--iters` timed ones; medians (and minima) are reported; the kernels are timed by HIP
events on the device's own clock, whole calls by time.perf_counter around device synchronises.  The GPU's clocks are whatever
the machine runs at: the tool sets nothing.

The parent process never opens the GPU: every step runs as ONE fresh child process at a time under its own `timeout`, and the
first step that fails ends the run.  Writes profiles/plate_bench.json (or --out).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDE, BATCH = 416, 64
STEPS = (('kernels', 180), ('device', 180), ('host', 420), ('train', 600))          # (step, seconds allowed)
R_MAX = [45, 60, 45]
CAMERA = {'image_width': 640, 'image_height': 480,
          'projection_matrix': {'data': [610.0, 0.0, 322.5, 0.0, 0.0, 608.0, 241.25, 0.0, 0.0, 0.0, 1.0, 0.0]}}


def write_fonts(root, seed=0):
    """35 glyph images (0..33 and the dot, 34): a noise-coloured bar with an alpha ramp on a transparent ground."""
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root)
    for k in range(35):
        px = np.zeros((120, 60, 4), np.uint8)
        px[12:100 + k % 9, 8 + k % 5:50] = rng.integers(0, 256, 4, dtype=np.uint8)
        px[12:100 + k % 9, 8 + k % 5:50, 3] = np.linspace(255, 90, 88 + k % 9).astype(np.uint8)[:, None]
        Image.fromarray(px).save(os.path.join(root, '%d.png' % k))


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def _seed(s):
    import numpy as np
    np.random.seed(s)
    random.seed(s)


def _generator(root):
    from yolo_amd.render import LPGenerator
    return LPGenerator(SIDE, SIDE, root, CAMERA)


def _events(fn, warmup, iters):
    import torch
    events = []
    for i in range(warmup + iters):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        fn()
        e[1].record()
        if i >= warmup:
            events.append(e)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in events]


def _wall(fn, warmup, iters):
    import torch
    ms = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def step_kernels(args, dev, root):
    import torch
    from yolo_amd import lib as L
    lib = L.load()
    gen = _generator(root)
    _seed(1)
    _, rows = gen.draw_params(BATCH, SIDE, SIDE, R_MAX)
    quiet = rows.copy()
    quiet[:, 14] = 0
    atlas = torch.from_numpy(gen.glyph_atlas()).to(dev)
    rows_d, quiet_d = torch.from_numpy(rows).to(dev), torch.from_numpy(quiet).to(dev)
    bg = torch.rand((BATCH, 3, SIDE, SIDE), device=dev)
    y = torch.empty_like(bg)
    plates = torch.empty((BATCH, 160, 380, 4), dtype=torch.uint8, device=dev)
    work = torch.empty(lib.yolo_plate_workspace_bytes(BATCH, SIDE, SIDE), dtype=torch.uint8, device=dev)

    def compose():
        L.check(lib.yolo_plate_compose(L.ptr(atlas), L.ptr(rows_d), L.ptr(plates), BATCH, L.stream_ptr()), 'compose')

    def stats(r=rows_d):
        L.check(lib.yolo_plate_stats(L.ptr(plates), L.ptr(r), L.ptr(work), BATCH, SIDE, SIDE, L.stream_ptr()), 'stats')

    def rend(r=rows_d):
        L.check(lib.yolo_plate_render(L.ptr(bg), L.ptr(plates), L.ptr(r), L.ptr(work), L.ptr(y), BATCH, SIDE, SIDE, L.stream_ptr()), 'render')
    compose()
    stats()
    nbytes = 24 * BATCH * SIDE * SIDE
    window = float(((rows[:, 10] - rows[:, 8]) * (rows[:, 11] - rows[:, 9])).sum()) / (BATCH * SIDE * SIDE)
    r = {'size': SIDE, 'batch': BATCH, 'warmup': args.warmup, 'iters': args.iters, 'clock': 'HIP events', 'window_fraction_of_canvas': window,
         'algorithmic_bytes_24_per_pixel': nbytes, 'plate_bytes_written_by_compose': int(plates.numel())}
    for name, fn in (('plate_compose', compose), ('plate_stats', stats), ('plate_render', rend),
                     ('plate_stats_no_noise', lambda: stats(quiet_d)), ('plate_render_no_noise', lambda: rend(quiet_d))):
        if name == 'plate_render_no_noise':
            stats(quiet_d)
        st = _stat(_events(fn, args.warmup, args.iters))
        r[name] = {'median_us': st['median_ms'] * 1e3, 'min_us': st['min_ms'] * 1e3, 'gb_per_s_of_24_b_per_pixel': nbytes / (st['median_ms'] * 1e-3) / 1e9}
    # the integer work of the noise: 2 Philox4x32-10 calls per pixel, 10 rounds of 2 x (mul_hi + mul_lo) + 4 xor + 2 add each
    r['philox_calls_per_pass'] = 2 * BATCH * SIDE * SIDE
    print(json.dumps(r), flush=True)
    return r


def step_device(args, dev, root):
    import torch
    gen = _generator(root)
    bg = torch.rand((BATCH, 3, SIDE, SIDE), device=dev)
    y = torch.empty_like(bg)
    _seed(2)
    host = []
    for _ in range(args.warmup + args.iters):
        t0 = time.perf_counter()
        gen.draw_params(BATCH, SIDE, SIDE, R_MAX)
        host.append((time.perf_counter() - t0) * 1e3)
    r = {'size': SIDE, 'batch': BATCH, 'warmup': args.warmup, 'iters': args.iters, 'clock': 'time.perf_counter around device synchronises',
         'draw_params_host_only': _stat(host[args.warmup:]),
         'add_device_wall': _stat(_wall(lambda: gen.add_device(bg, R_MAX, out=y), args.warmup, args.iters))}
    r['images_per_s'] = BATCH / (r['add_device_wall']['median_ms'] * 1e-3)
    print(json.dumps(r), flush=True)
    return r


def step_host(args, dev, root):
    import torch
    gen = _generator(root)
    bg = torch.rand((BATCH, 3, SIDE, SIDE), device=dev)
    _seed(2)
    t0 = time.perf_counter()
    gen.add_host(BATCH, SIDE, SIDE, R_MAX)
    host_only = (time.perf_counter() - t0) * 1e3
    r = {'size': SIDE, 'batch': BATCH, 'warmup': 1, 'iters': args.host_iters, 'clock': 'time.perf_counter around device synchronises',
         'add_host_only_ms': host_only, 'add_wall': _stat(_wall(lambda: gen.add(bg, R_MAX), 1, args.host_iters))}
    r['images_per_s'] = BATCH / (r['add_wall']['median_ms'] * 1e-3)
    print(json.dumps(r), flush=True)
    return r


def step_train(args, dev, root):
    import torch
    from yolo_amd.net import CarLPNet
    from yolo_amd.spec import darknet53_spec
    from yolo_amd.train import Trainer
    gen = _generator(root)
    spec = dict(darknet53_spec(), LP_slice_point=[1, 3, 4, 7, 10], LP_r_max=R_MAX)
    net = CarLPNet(spec, dtype='bf16', device=dev, tune='auto').initialize(1)
    tr = Trainer(net, (SIDE, SIDE), lp_r_max=R_MAX)
    bg = torch.rand((BATCH, 3, SIDE, SIDE), device=dev)
    y = torch.empty_like(bg)
    lab = -torch.ones((BATCH, 1, 6 + 24), device=dev)                 # (no cars: the batch under test is the plates')
    _seed(3)
    x0, lp0 = gen.add_device(bg, R_MAX)
    x0, lp0 = x0.clone(), lp0.clone()

    def resident():
        tr.train_step(x0, lab, lp_labels=lp0)

    def device_route():
        x, lp = gen.add_device(bg, R_MAX, out=y)
        tr.train_step(x, lab, lp_labels=lp)

    def host_route():
        x, lp = gen.add(bg, R_MAX)
        tr.train_step(x, lab, lp_labels=lp)
    r = {'size': SIDE, 'batch': BATCH, 'net': 'D53 CarLPNet', 'dtype': 'bf16', 'tune': 'auto',
         'timed': 'wall clock (time.perf_counter) over a run of steps after 2 untimed ones, one device synchronise at its end'}
    for name, fn, iters in (('train_step_resident_batch', resident, args.train_iters), ('train_step_add_device', device_route, args.train_iters),
                            ('train_step_add_host', host_route, args.host_iters)):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / iters
        r[name] = {'ms_per_step': ms, 'images_per_s': BATCH / (ms * 1e-3), 'steps': iters}
        print(name, json.dumps(r[name]), flush=True)
    return r


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/plate_bench.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'fonts')
        write_fonts(root)
        res = {'kernels': step_kernels, 'device': step_device, 'host': step_host, 'train': step_train}[args.child](args, dev, root)
    if args.child_out:
        with open(args.child_out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'result': res}, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--host-iters', type=int, default=3, help='calls of the PIL route (seconds each)')
    ap.add_argument('--train-iters', type=int, default=10)
    ap.add_argument('--steps', default=','.join(s for s, _ in STEPS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plate_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {'tool': 'tools/plate_bench.py', 'warmup': args.warmup}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step, seconds in STEPS:
        if step not in args.steps.split(','):
            continue
        part = '%s.%s.part' % (args.out, step)
        cmd = ['timeout', '-k', '10', str(seconds), sys.executable, os.path.abspath(__file__), '--child', step, '--child-out', part,
               '--warmup', str(args.warmup), '--iters', str(args.iters), '--host-iters', str(args.host_iters),
               '--train-iters', str(args.train_iters)]
        rc = subprocess.call(cmd)
        if rc != 0:                                           # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.exit('plate_bench: step %r ended with status %d; stopping' % (step, rc))
        with open(part) as f:
            got = json.load(f)
        os.remove(part)
        res['device_name'] = got['device']                    # (not 'device': that is a step's name)
        res[step] = got['result']
        with open(args.out, 'w') as f:                        # (rewritten after every step: a later step's failure keeps the earlier figures)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
