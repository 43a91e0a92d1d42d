#!/usr/bin/env python
"""What making the background batch on the device costs, and what it replaces (BackgroundBank.next_batch, csrc/background.hip).

On a seeded synthetic bank of 200 noise-textured images of 480 x 640 (gradients plus noise; about 330 MB resident with the mip
levels), augmentation on, at 416^2, batch 64:

  kernels  yolo_bg_stats and yolo_bg_render each alone, by HIP events, on one seeded batch of rows.  Algorithmic bytes of the second
           pass = the 12 B written per output pixel plus the 4 B of every level pixel inside the batch's crops once (neighbouring
           outputs share taps, so that is the honest read side; 4 taps x 4 B per output are ASKED for); GB/s = those over the median
           time.  The mean shader clock over the timed region is recorded beside it (bench.py's Telemetry).
  intake   tools/intake_bench.py's kernel step in the same run on the same box: yolo_warp_u8_to_nchw is the same kind of kernel
           (uint8 gathers to fp32 planes), so its GB/s is the yardstick for yolo_bg_render's.
  device   a whole next_batch call: the host's draws (draw_params, also timed alone), the pinned upload, both kernels; wall clock
           per call around a device synchronise.
  host     the route it replaces, from images ALREADY DECODED in memory (mxnet's iterator also decodes a JPEG per image; that is
           left out, in the host route's favour): per image random_sized_crop, PIL crop + bilinear resize, mirror,
           ColorAugmenter.__call__ in numpy, then one upload of the (B,3,H,W) float32 batch; wall clock per call around a device
           synchronise, one host thread (as a Python loop runs).
  train    a bf16 Trainer.train_step (D53, tune='auto') on batches RenderCar.render_device draws over a background from each route,
           and over one resident background: wall clock per step.

Timing: `--warmup` untimed calls, then `--iters` timed ones; medians (and minima) are reported; the kernels are timed by HIP events
on the device's own clock, whole calls by time.perf_counter around device synchronises.  The GPU's clocks are whatever the machine
runs at: the tool sets nothing.

The parent process never opens the GPU: every step runs as ONE fresh child process at a time under its own `timeout`, and the first
step that fails ends the run.  Writes profiles/background_bench.json (or --out).  Needs the GPU: there is no fallback."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SIDE, BATCH = 416, 64
BANK_IMAGES, BANK_HW = 200, (480, 640)
STEPS = (('kernels', 240), ('intake', 240), ('device', 240), ('host', 420), ('train', 600))          # (step, seconds allowed)
CLASSES = [[15.0 * i, 0.0] for i in range(24)]


def synthetic_images(n=BANK_IMAGES, hw=BANK_HW, seed=0):
    """n (h, w, 3) uint8 images: a random colour gradient plus noise (photograph-like means, incompressible detail)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for _ in range(n):
        c0, cx, cy = rng.uniform(40, 200, 3), rng.uniform(-0.12, 0.12, 3), rng.uniform(-0.12, 0.12, 3)
        img = c0[None, None, :] + xx[..., None] * cx + yy[..., None] * cy + rng.integers(-40, 41, (h, w, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def _seed(s):
    import numpy as np
    np.random.seed(s)
    random.seed(s)


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


def _bank(dev):
    from yolo_amd.background import BackgroundBank
    return BackgroundBank(synthetic_images(), SIDE, SIDE, device=dev, mode='train')


def render_bytes(rows, side):
    """Algorithmic bytes of yolo_bg_render on these rows: the fp32 planes written plus every level pixel inside the rois once."""
    roi = rows[:, 3:7].astype('int64')
    read = int(((roi[:, 2] - roi[:, 0] + 1) * (roi[:, 3] - roi[:, 1] + 1) * 4).sum())
    return 12 * len(rows) * side * side + read, read


def host_batch(images, side, batch, aug, order):
    """The host route: -> (batch,3,side,side) float32 0..255 ndarray.  images: PIL images, decoded."""
    import numpy as np
    from PIL import Image
    from yolo_amd.background import random_sized_crop
    out = np.empty((batch, 3, side, side), np.float32)
    for i in range(batch):
        im = images[order[i % len(order)]]
        x0, y0, cw, ch, _ = random_sized_crop(im.size[1], im.size[0], (side, side))
        px = np.asarray(im.crop((x0, y0, x0 + cw, y0 + ch)).resize((side, side), Image.BILINEAR), np.float32)
        if random.random() < 0.5:
            px = px[:, ::-1]
        out[i] = aug(px).transpose(2, 0, 1)
    return out


def step_kernels(args, dev):
    import torch
    from bench import Telemetry
    from yolo_amd import lib as L
    lib = L.load()
    bank = _bank(dev)
    _seed(1)
    rows = bank.draw_params(BATCH)
    data = torch.from_numpy(bank.data).to(dev)
    rows_d = torch.from_numpy(rows).to(dev)
    y = torch.empty((BATCH, 3, SIDE, SIDE), device=dev)
    work = torch.empty(lib.yolo_bg_workspace_bytes(BATCH, SIDE, SIDE), dtype=torch.uint8, device=dev)

    def stats():
        L.check(lib.yolo_bg_stats(L.ptr(data), data.numel(), L.ptr(rows_d), L.ptr(work), BATCH, SIDE, SIDE, L.stream_ptr()), 'bg_stats')

    def rend():
        L.check(lib.yolo_bg_render(L.ptr(data), data.numel(), L.ptr(rows_d), L.ptr(work), L.ptr(y), BATCH, SIDE, SIDE, L.stream_ptr()), 'bg_render')
    stats()
    nbytes, read = render_bytes(rows, SIDE)
    torch.cuda.synchronize()
    tel = Telemetry(dev.index or 0).start()
    iters = 20 * args.iters                                   # (a second or so of back-to-back launches per kernel: a sustained figure)
    r = {'size': SIDE, 'batch': BATCH, 'warmup': args.warmup, 'iters': iters, 'clock': 'HIP events', 'bank_bytes': int(data.numel()),
         'bank_images': len(bank), 'bank_image_hw': list(BANK_HW), 'level_heights_used': sorted(set(int(v) for v in rows[:, 1])),
         'bg_stats': _stat(_events(stats, args.warmup, iters)), 'bg_render': _stat(_events(rend, args.warmup, iters)),
         'bg_render_algorithmic_bytes': nbytes, 'bg_render_roi_bytes_read_once': read, 'bg_render_tap_bytes_asked': 16 * BATCH * SIDE * SIDE}
    r.update(tel.stop())
    r['bg_render_gb_per_s'] = nbytes / (r['bg_render']['median_ms'] * 1e-3) / 1e9
    r['bg_stats_gb_per_s_of_roi_bytes'] = read / (r['bg_stats']['median_ms'] * 1e-3) / 1e9
    print(json.dumps(r), flush=True)
    return r


def step_intake(args, dev):
    import intake_bench
    ns = argparse.Namespace(warmup=args.warmup, iters=args.iters, config=None)
    return intake_bench.step_kernel(ns, dev)


def step_device(args, dev):
    import torch
    bank = _bank(dev)
    y = torch.empty((BATCH, 3, SIDE, SIDE), device=dev)
    _seed(2)
    host = []
    for _ in range(args.warmup + args.iters):
        t0 = time.perf_counter()
        bank.draw_params(BATCH)
        host.append((time.perf_counter() - t0) * 1e3)
    r = {'size': SIDE, 'batch': BATCH, 'warmup': args.warmup, 'iters': args.iters, 'clock': 'time.perf_counter around device synchronises',
         'draw_params_host_only': _stat(host[args.warmup:]),
         'next_batch_wall': _stat(_wall(lambda: bank.next_batch(BATCH, out=y), args.warmup, args.iters))}
    r['images_per_s'] = BATCH / (r['next_batch_wall']['median_ms'] * 1e-3)
    print(json.dumps(r), flush=True)
    return r


def step_host(args, dev):
    import torch
    from PIL import Image
    from yolo_amd.render import ColorAugmenter
    images = [Image.fromarray(im) for im in synthetic_images()]
    aug = ColorAugmenter(brightness=0.5, contrast=0.5, saturation=0.5, hue=1.0, pca_noise=0)
    order = list(range(len(images)))
    _seed(2)
    t0 = time.perf_counter()
    host_batch(images, SIDE, BATCH, aug, order)
    host_only = (time.perf_counter() - t0) * 1e3

    def route():
        random.shuffle(order)
        return torch.from_numpy(host_batch(images, SIDE, BATCH, aug, order)).to(dev)
    r = {'size': SIDE, 'batch': BATCH, 'warmup': 1, 'iters': args.host_iters, 'clock': 'time.perf_counter around device synchronises',
         'host_threads': 1, 'jpeg_decode': 'not included', 'host_batch_only_ms': host_only, 'host_route_wall': _stat(_wall(route, 1, args.host_iters))}
    r['images_per_s'] = BATCH / (r['host_route_wall']['median_ms'] * 1e-3)
    print(json.dumps(r), flush=True)
    return r


def step_train(args, dev):
    import torch
    from PIL import Image
    from render_bench import write_sprites
    from yolo_amd.net import CarNet
    from yolo_amd.render import ColorAugmenter, RenderCar
    from yolo_amd.spec import darknet53_spec
    from yolo_amd.train import Trainer
    bank = _bank(dev)
    images = [Image.fromarray(im) for im in synthetic_images()]
    aug = ColorAugmenter(brightness=0.5, contrast=0.5, saturation=0.5, hue=1.0, pca_noise=0)
    order = list(range(len(images)))
    with tempfile.TemporaryDirectory() as root:
        write_sprites(root)
        rc = RenderCar(SIDE, SIDE, CLASSES, root, device=dev)
        net = CarNet(darknet53_spec(), dtype='bf16', device=dev, tune='auto').initialize(1)
        tr = Trainer(net, (SIDE, SIDE))
        bg = torch.empty((BATCH, 3, SIDE, SIDE), device=dev)
        y = torch.empty_like(bg)
        _seed(3)
        bg0 = bank.next_batch(BATCH).clone()

        def resident():
            x, lab = rc.render_device(bg0, 'train', out=y)
            tr.train_step(x, lab)

        def device_route():
            x, lab = rc.render_device(bank.next_batch(BATCH, out=bg), 'train', out=y)
            tr.train_step(x, lab)

        def host_route():
            random.shuffle(order)
            x, lab = rc.render_device(torch.from_numpy(host_batch(images, SIDE, BATCH, aug, order)).to(dev), 'train', out=y)
            tr.train_step(x, lab)
        r = {'size': SIDE, 'batch': BATCH, 'net': 'D53', 'dtype': 'bf16', 'tune': 'auto',
             'timed': 'wall clock (time.perf_counter) over a run of steps after 2 untimed ones, one device synchronise at its end; every '
                      'route draws its cars with render_device'}
        for name, fn, iters in (('train_step_resident_background', resident, args.train_iters), ('train_step_background_bank', device_route, args.train_iters),
                                ('train_step_background_host', host_route, args.host_iters)):
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
        sys.exit('tools/background_bench.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    res = {'kernels': step_kernels, 'intake': step_intake, 'device': step_device, 'host': step_host, 'train': step_train}[args.child](args, dev)
    if args.child_out:
        with open(args.child_out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'result': res}, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-iters', type=int, default=3, help='calls of the host route (seconds each)')
    ap.add_argument('--train-iters', type=int, default=10)
    ap.add_argument('--steps', default=','.join(s for s, _ in STEPS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'background_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {'tool': 'tools/background_bench.py'}
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
            sys.exit('background_bench: step %r ended with status %d; stopping' % (step, rc))
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
