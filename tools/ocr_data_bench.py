#!/usr/bin/env python
"""What the OCR reader's labelled data costs on the device, and what it replaces (LPGenerator.render_device, yolo_amd/ocr.py,
csrc/ocr_data.hip).

On seeded synthetic glyph images written to a temporary directory, colour augmenter on, the reference's 160 x 384 canvas, at its
training batch of 100 and its validation batch of 16:

  kernels    yolo_plate_compose, yolo_ocr_plate_blur (also with every T forced to 0 and to 24, and with the noise scale zeroed),
             yolo_ocr_plate_render, yolo_ocr_targets, yolo_ocr_loss_fwd_bwd (with and without the gradient) and yolo_ocr_score,
             each alone, by HIP events, on one seeded batch of rows at batch 100.
  device     a whole render_device call: the host's draws (draw_ocr_params, also timed alone), the pinned upload, the three
             kernels; wall clock per call around a device synchronise.
  host       the route it replaces: LPGenerator.render = render_host (PIL + numpy, one image at a time) + the fg / mask upload
             + yolo_composite; wall clock per call around a device synchronise.
  validator  an OCRValidator.update step (net, decode, targets, losses, counts) on a resident batch and, beside it, the bf16
             OCRNet's forward alone at the same N: whether making the data would bound a later training step.

Timing: `--warmup` untimed calls, then `--iters` timed ones; medians (and minima) are reported; kernels by HIP events on the
device's own clock, whole calls by time.perf_counter around device synchronises.  The tool sets no clocks.

The parent process never opens the GPU: every step runs as ONE fresh child process at a time under its own `timeout`, and the
first step that fails ends the run.  Writes profiles/ocr_data_bench.json (or --out).  Needs the GPU: there is no fallback."""
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

H, W, WP, NCLS = 160, 384, 24, 34
BATCHES = (100, 16)
STEPS = (('kernels', 180), ('device', 180), ('host', 300), ('validator', 240))          # (step, seconds allowed)
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


def _stat(v, unit='ms'):
    import numpy as np
    scale = 1e3 if unit == 'us' else 1.0
    return {'median_' + unit: float(np.median(v)) * scale, 'min_' + unit: float(np.min(v)) * scale}


def _seed(s):
    import numpy as np
    np.random.seed(s)
    random.seed(s)


def _generator(root):
    from yolo_amd.render import LPGenerator
    return LPGenerator(H, W, root, CAMERA)


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
    import numpy as np
    import torch
    from yolo_amd import lib as L
    from yolo_amd import ocr
    lib = L.load()
    gen = _generator(root)
    B = BATCHES[0]
    _seed(1)
    labels, rows, taps, orders = gen.draw_ocr_params(B, H, W)
    quiet = rows.copy()
    quiet[:, 14] = 0
    t0, t24 = taps.copy(), taps.copy()
    t0[:, 0] = 0
    t24[:, 0] = 24                                            # (the weights past a row's own T are zeros: the work is what is timed)
    up = lambda a: torch.from_numpy(a).to(dev)
    atlas, rows_d, quiet_d, taps_d, t0_d, t24_d = up(gen.glyph_atlas()), up(rows), up(quiet), up(taps), up(t0), up(t24)
    labels_d, orders_d = up(labels), up(orders)
    bg = torch.rand((B, 3, H, W), device=dev) * 255
    y = torch.empty_like(bg)
    plates = torch.empty((B, 160, 380, 4), dtype=torch.uint8, device=dev)
    work = torch.empty(lib.yolo_ocr_plate_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    logits = torch.randn((B, WP, 1 + NCLS), device=dev) * 3
    st = L.stream_ptr

    def compose():
        L.check(lib.yolo_plate_compose(L.ptr(atlas), L.ptr(rows_d), L.ptr(plates), B, st()), 'compose')

    def blur(r=rows_d, t=taps_d):
        L.check(lib.yolo_ocr_plate_blur(L.ptr(plates), L.ptr(r), L.ptr(t), L.ptr(work), B, H, W, st()), 'blur')

    def rend():
        L.check(lib.yolo_ocr_plate_render(L.ptr(bg), L.ptr(rows_d), L.ptr(work), L.ptr(y), B, H, W, 0, st()), 'render')
    compose()
    blur()
    score_y, class_y = ocr.ocr_targets(labels_d, WP, orders_d)
    score = torch.empty((B, WP), dtype=torch.float32, device=dev)
    codes = torch.empty((B, WP), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    L.check(lib.yolo_ocr_decode(L.ptr(logits), None, L.ptr(score), L.ptr(codes), L.ptr(count), B, WP, NCLS, 0.2, st()), 'decode')
    window = float(((rows[:, 10] - rows[:, 8]) * (rows[:, 11] - rows[:, 9])).sum()) / (B * H * W)
    r = {'canvas': [H, W], 'batch': B, 'warmup': args.warmup, 'iters': args.iters, 'clock': 'HIP events', 'window_fraction_of_canvas': window,
         'taps_per_side': {'mean': float(taps[:, 0].mean()), 'min': int(taps[:, 0].min()), 'max': int(taps[:, 0].max())},
         'workspace_bytes': int(work.numel())}
    for name, fn in (('plate_compose', compose), ('ocr_plate_blur', blur), ('ocr_plate_blur_T0', lambda: blur(rows_d, t0_d)),
                     ('ocr_plate_blur_T24', lambda: blur(rows_d, t24_d)), ('ocr_plate_blur_no_noise', lambda: blur(quiet_d, taps_d)),
                     ('ocr_plate_render', rend), ('ocr_targets', lambda: ocr.ocr_targets(labels_d, WP, orders_d)),
                     ('ocr_loss', lambda: ocr.ocr_loss(logits, score_y, class_y)),
                     ('ocr_loss_with_gradient', lambda: ocr.ocr_loss(logits, score_y, class_y, grad=True)),
                     ('ocr_score', lambda: ocr.ocr_score(codes, count, labels_d, class_y, logits))):
        if name == 'ocr_plate_render':
            blur()
        r[name] = _stat(_events(fn, args.warmup, args.iters), 'us')
    # (targets, loss and score allocate their outputs through torch inside the timed call: the figure is the call's, not the bare kernel's)
    print(json.dumps(r), flush=True)
    return r


def step_device(args, dev, root):
    import torch
    gen = _generator(root)
    r = {'canvas': [H, W], 'warmup': args.warmup, 'iters': args.iters, 'clock': 'time.perf_counter around device synchronises'}
    for B in BATCHES:
        bg = torch.rand((B, 3, H, W), device=dev) * 255
        y = torch.empty_like(bg)
        _seed(2)
        host = []
        for _ in range(args.warmup + args.iters):
            t0 = time.perf_counter()
            gen.draw_ocr_params(B, H, W)
            host.append((time.perf_counter() - t0) * 1e3)
        wall = _stat(_wall(lambda: gen.render_device(bg, out=y), args.warmup, args.iters))
        r['batch_%d' % B] = {'draw_ocr_params_host_only': _stat(host[args.warmup:]), 'render_device_wall': wall,
                             'images_per_s': B / (wall['median_ms'] * 1e-3)}
    print(json.dumps(r), flush=True)
    return r


def step_host(args, dev, root):
    import torch
    gen = _generator(root)
    r = {'canvas': [H, W], 'warmup': 1, 'iters': args.host_iters, 'clock': 'time.perf_counter around device synchronises'}
    for B in BATCHES:
        bg = torch.rand((B, 3, H, W), device=dev) * 255
        _seed(2)
        t0 = time.perf_counter()
        gen.render_host(B, H, W)
        host_only = (time.perf_counter() - t0) * 1e3
        wall = _stat(_wall(lambda: gen.render(bg), 1, args.host_iters))
        r['batch_%d' % B] = {'render_host_only_ms': host_only, 'render_wall': wall, 'images_per_s': B / (wall['median_ms'] * 1e-3)}
    print(json.dumps(r), flush=True)
    return r


def step_validator(args, dev, root):
    import torch
    from yolo_amd.dense import OCRNet
    from yolo_amd.ocr import OCRValidator
    gen = _generator(root)
    net = OCRNet(dtype='bf16', device=dev)
    net.initialize(1)
    val = OCRValidator(net)
    r = {'canvas': [H, W], 'net': 'OCRNet(32, 12, [6, 12, 24], classes=34)', 'dtype': 'bf16', 'warmup': args.warmup, 'iters': args.iters,
         'clock': 'HIP events'}
    for B in BATCHES:
        _seed(3)
        x, labels = gen.render_device(torch.rand((B, 3, H, W), device=dev) * 255)
        x, labels = x.clone(), labels.clone()
        fwd = _stat(_events(lambda: net(x), args.warmup, args.iters))
        upd = _stat(_events(lambda: val.update(x, labels), args.warmup, args.iters))
        rd = _stat(_events(lambda: gen.render_device(x), args.warmup, args.iters))
        r['batch_%d' % B] = {'ocrnet_forward': fwd, 'validator_update': upd, 'render_device_stream_time': rd,
                             'update_less_forward_ms': upd['median_ms'] - fwd['median_ms']}
    r['result_after_the_timed_updates'] = val.result()
    print(json.dumps(r), flush=True)
    return r


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/ocr_data_bench.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'fonts')
        write_fonts(root)
        res = {'kernels': step_kernels, 'device': step_device, 'host': step_host, 'validator': step_validator}[args.child](args, dev, root)
    if args.child_out:
        with open(args.child_out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'result': res}, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--host-iters', type=int, default=3, help='calls of the PIL route (seconds each)')
    ap.add_argument('--steps', default=','.join(s for s, _ in STEPS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ocr_data_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {'tool': 'tools/ocr_data_bench.py', 'warmup': args.warmup}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step, seconds in STEPS:
        if step not in args.steps.split(','):
            continue
        part = '%s.%s.part' % (args.out, step)
        cmd = ['timeout', '-k', '10', str(seconds), sys.executable, os.path.abspath(__file__), '--child', step, '--child-out', part,
               '--warmup', str(args.warmup), '--iters', str(args.iters), '--host-iters', str(args.host_iters)]
        rc = subprocess.call(cmd)
        if rc != 0:                                           # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.exit('ocr_data_bench: step %r ended with status %d; stopping' % (step, rc))
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
