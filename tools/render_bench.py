#!/usr/bin/env python
"""What drawing the training batch on the device costs, and what it replaces (RenderCar.render_device, csrc/render.hip).

On a seeded synthetic sprite set written to a temporary directory (16 textured ellipses of 400 x 260 on transparent canvases),
colour augmenter on, rotation 30 degrees and blur 0.3 as RenderCar defaults, at 416^2 and 608^2, batch 64:

  kernels  yolo_render_stats and yolo_render_cars each alone, by HIP events, on one seeded batch of rows.  Algorithmic bytes of the
           second pass = 24 B per output pixel (12 read, 12 written); GB/s = those over the median time.
  device   a whole render_device call: the host's draws (draw_params, also timed alone), the pinned upload, both kernels; wall
           clock per call around a device synchronise.
  host     the route it replaces: RenderCar.render = render_host (PIL + numpy, one image at a time) + the fg / mask upload +
           yolo_composite; wall clock per call around a device synchronise.
  train    a bf16 Trainer.train_step (D53, tune='auto') fed by each route, and on a resident batch: wall clock per step.

The parent process never opens the GPU: every step runs as ONE fresh child process at a time under its own `timeout`, and the
first step that fails ends the run.  Writes profiles/render_bench.json (or --out).  Needs the GPU: there is no fallback."""
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

CONFIGS = ((416, 64), (608, 64))                                     # (canvas side, batch)
STEPS = (('kernels', 180), ('device', 180), ('host', 420), ('train', 600))          # (step, seconds allowed)
CLASSES = [[15.0 * i, 0.0] for i in range(24)]


def write_sprites(root, seed=0, n=16, size=(260, 400)):
    """n textured ellipses (noise colour, opaque) on transparent canvases, named as the blender renders are."""
    import numpy as np
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    for mode in ('train', 'valid'):
        d = os.path.join(root, mode, 'cad')
        os.makedirs(d)
        for k in range(n):
            h, w = size
            alpha = Image.new('L', (w, h), 0)
            ImageDraw.Draw(alpha).ellipse((w // 10, h // 6, w - w // 12, h - h // 8), fill=255)
            px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            px[..., 3] = np.asarray(alpha)
            px[px[..., 3] == 0] = 0
            Image.fromarray(px).save(os.path.join(d, 'car%d_azi%d_ele%d.png' % (k, (36000 * k) // n, 1000 + 100 * (k % 5))))


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def _seed(s):
    import numpy as np
    np.random.seed(s)
    random.seed(s)


def _renderer(side, dev, root):
    from yolo_amd.render import RenderCar
    return RenderCar(side, side, CLASSES, root, device=dev)


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
    out = []
    for side, batch in CONFIGS:
        rc = _renderer(side, dev, root)
        _seed(1)
        _, rows = rc.draw_params(batch, 'train')
        atlas = torch.from_numpy(rc.atlas().data).to(dev)
        rows_d = torch.from_numpy(rows).to(dev)
        bg = torch.rand((batch, 3, side, side), device=dev) * 255
        y = torch.empty_like(bg)
        work = torch.empty(lib.yolo_render_workspace_bytes(batch, side, side), dtype=torch.uint8, device=dev)

        def stats():
            L.check(lib.yolo_render_stats(L.ptr(atlas), atlas.numel(), L.ptr(rows_d), L.ptr(work), batch, side, side, L.stream_ptr()), 'stats')

        def cars():
            L.check(lib.yolo_render_cars(L.ptr(bg), L.ptr(atlas), atlas.numel(), L.ptr(rows_d), L.ptr(work), L.ptr(y), batch, side, side,
                                         L.stream_ptr()), 'cars')
        stats()
        nbytes = 24 * batch * side * side
        window = float(((rows[:, 5] - rows[:, 3]) * (rows[:, 6] - rows[:, 4])).sum()) / (batch * side * side)
        r = {'size': side, 'batch': batch, 'iters': args.iters, 'atlas_bytes': int(atlas.numel()), 'window_fraction_of_canvas': window,
             'render_stats': _stat(_events(stats, args.warmup, args.iters)), 'render_cars': _stat(_events(cars, args.warmup, args.iters)),
             'render_cars_algorithmic_bytes': nbytes}
        r['render_cars_gb_per_s'] = nbytes / (r['render_cars']['median_ms'] * 1e-3) / 1e9
        out.append(r)
        print(json.dumps(r), flush=True)
        del bg, y
        torch.cuda.empty_cache()
    return out


def step_device(args, dev, root):
    import torch
    out = []
    for side, batch in CONFIGS:
        rc = _renderer(side, dev, root)
        bg = torch.rand((batch, 3, side, side), device=dev) * 255
        y = torch.empty_like(bg)
        _seed(2)
        host = []
        for _ in range(args.warmup + args.iters):
            t0 = time.perf_counter()
            rc.draw_params(batch, 'train')
            host.append((time.perf_counter() - t0) * 1e3)
        r = {'size': side, 'batch': batch, 'iters': args.iters, 'draw_params_host_only': _stat(host[args.warmup:]),
             'render_device_wall': _stat(_wall(lambda: rc.render_device(bg, 'train', out=y), args.warmup, args.iters))}
        r['images_per_s'] = batch / (r['render_device_wall']['median_ms'] * 1e-3)
        out.append(r)
        print(json.dumps(r), flush=True)
        del bg, y
        torch.cuda.empty_cache()
    return out


def step_host(args, dev, root):
    import torch
    out = []
    for side, batch in CONFIGS:
        rc = _renderer(side, dev, root)
        bg = torch.rand((batch, 3, side, side), device=dev) * 255
        _seed(2)
        t0 = time.perf_counter()
        rc.render_host(batch, 'train')
        host_only = (time.perf_counter() - t0) * 1e3
        r = {'size': side, 'batch': batch, 'iters': args.host_iters, 'render_host_only_ms': host_only,
             'render_wall': _stat(_wall(lambda: rc.render(bg, 'train'), 1, args.host_iters))}
        r['images_per_s'] = batch / (r['render_wall']['median_ms'] * 1e-3)
        out.append(r)
        print(json.dumps(r), flush=True)
        del bg
        torch.cuda.empty_cache()
    return out


def step_train(args, dev, root):
    import torch
    from yolo_amd.net import CarNet
    from yolo_amd.spec import darknet53_spec
    from yolo_amd.train import Trainer
    out = []
    for side, batch in CONFIGS:
        rc = _renderer(side, dev, root)
        net = CarNet(darknet53_spec(), dtype='bf16', device=dev, tune='auto').initialize(1)
        tr = Trainer(net, (side, side))
        bg = torch.rand((batch, 3, side, side), device=dev) * 255
        y = torch.empty_like(bg)
        _seed(3)
        x0, lab0 = rc.render_device(bg, 'train')
        x0, lab0 = x0.clone(), lab0.clone()

        def resident():
            tr.train_step(x0, lab0)

        def device_route():
            x, lab = rc.render_device(bg, 'train', out=y)
            tr.train_step(x, lab)

        def host_route():
            x, lab = rc.render(bg, 'train')
            tr.train_step(x, lab)
        r = {'size': side, 'batch': batch, 'net': 'D53', 'dtype': 'bf16', 'tune': 'auto',
             'timed': 'wall clock over a run of steps, one device synchronise at its end'}
        for name, fn, iters in (('train_step_resident_batch', resident, args.train_iters), ('train_step_render_device', device_route, args.train_iters),
                                ('train_step_render_host', host_route, args.host_iters)):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / iters
            r[name] = {'ms_per_step': ms, 'images_per_s': batch / (ms * 1e-3), 'steps': iters}
            print(name, json.dumps(r[name]), flush=True)
        out.append(r)
        del tr, net, bg, y, x0
        torch.cuda.empty_cache()
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/render_bench.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    with tempfile.TemporaryDirectory() as root:
        write_sprites(root)
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {'tool': 'tools/render_bench.py', 'warmup': args.warmup}
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
            sys.exit('render_bench: step %r ended with status %d; stopping' % (step, rc))
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
