#!/usr/bin/env python
"""What the frame overlay costs, and what it replaces (yolo_amd.overlay.FrameOverlay, csrc/overlay.hip), at 1920x1080 bs 32.

  kernels  yolo_overlay_shapes and yolo_overlay_draw each alone, by HIP events, for two loads: 'top1_plate' (the car box and the plate
           of every frame, K = 2) and 'nms100' (100 NMS boxes a frame, K = 100); the plate's yolo_warp_u8_to_nchw beside them.  In the
           SAME run, alternating with the draw kernel, a device-to-device copy of the same frame batch (torch's copy_: 199 MB read and
           199 MB written) as the yardstick: the draw kernel reads no frame byte and writes only painted pixels, so the expectation to
           confirm or refute is draw < one copy of the frames.  The mean shader clock over the timed region is recorded beside it
           (bench.py's Telemetry).  Both loads also run with text labels (FrameOverlay(labels=True): class name, score and, on the
           car box, the azimuth of yolo_pose_top1, in the default 6 x 11 font): yolo_overlay_labels and yolo_overlay_text take their
           turns in the same alternation, so the expectation "at K = 2 the text kernel costs well below the draw kernel, because its
           grid follows the label area" is read off one run.
  host     the route the overlay replaces, on the same box: a blocking D2H of the rows, intake.plate_matrix per frame, PIL
           ImageDraw.line for the box and the plate edges on the host's frames (cv2 is not installed here; PIL's line is the
           nearest thing), the H2D of the matrices; wall clock around device synchronises.  The comparison for "was it worth it", not
           the code under test.
  video    D53 at 416^2 bs 32 (--dtype, tune='auto') from resident 1080p uint8 frames: FrameIntake -> net -> predict_device ->
           [pose_device ->] [FrameOverlay with the top-1 rows and resident plate rows] -> non-blocking D2H of the frames into pinned
           memory; wall clock per step without the overlay, with it, and with it and its labels, alternating blocks.  The plate rows are synthetic and resident (this net has
           no plate branch); everything else is the product's path.

The parent process never opens the GPU: every step runs as ONE fresh child process at a time under its own `timeout`, and the
first step that fails ends the run.  Writes profiles/overlay_bench.json (or --out).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRC_HW, BATCH, SIZE = (1080, 1920), 32, (416, 416)
CAMERA = {'image_width': 1920, 'image_height': 1080,
          'projection_matrix': {'data': [1230.0, 0.0, 967.5, 0.0, 0.0, 1246.5, 536.0, 0.0, 0.0, 0.0, 1.0, 0.0]}}
STEPS = (('kernels', 300), ('host', 300), ('video', 600))            # (step, seconds allowed)


def _stat(v):
    import numpy as np
    return {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}


def _frames(seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (BATCH,) + SRC_HW + (3,), generator=g, dtype=torch.uint8)


def _rows(seed):
    """-> (pred (B,8), lp (B,7), nms rows (B,400,8), kept (B,100), count (B,)) float32 / int32 ndarrays: boxes of 10..60 % of the
    frame, plates 1.5..6 m away, 100 kept boxes per frame."""
    import numpy as np
    g = np.random.default_rng(seed)
    pred = g.uniform(0.0, 1.0, (BATCH, 8))
    pred[:, 0] = g.uniform(0.6, 1.0, BATCH)
    pred[:, 1:3] = g.uniform(0.3, 0.7, (BATCH, 2))
    pred[:, 3:5] = g.uniform(0.1, 0.6, (BATCH, 2))
    lp = np.empty((BATCH, 7))
    lp[:, 0] = g.uniform(0.6, 1.0, BATCH)
    lp[:, 1], lp[:, 2], lp[:, 3] = g.uniform(-500, 500, BATCH), g.uniform(-300, 300, BATCH), g.uniform(1500, 6000, BATCH)
    lp[:, 4:] = g.uniform(-0.7, 0.7, (BATCH, 3))
    nbox = 400
    rows = g.uniform(0.0, 1.0, (BATCH, nbox, 8))
    cy, cx = g.uniform(0.0, 1.0, (BATCH, nbox)), g.uniform(0.0, 1.0, (BATCH, nbox))
    h, w = g.uniform(0.05, 0.5, (BATCH, nbox)), g.uniform(0.05, 0.5, (BATCH, nbox))
    rows[:, :, 1], rows[:, :, 2], rows[:, :, 3], rows[:, :, 4] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    kept = np.stack([g.permutation(nbox * 2)[:100] for _ in range(BATCH)]).astype(np.int32)
    return pred.astype(np.float32), lp.astype(np.float32), rows.astype(np.float32), kept, np.full(BATCH, 100, np.int32)


def _events(fn, warmup, iters):
    import torch
    ev = []
    for i in range(warmup + iters):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        fn()
        e[1].record()
        if i >= warmup:
            ev.append(e)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _events_alternating(fns, warmup, iters):
    """{name: fn}: one launch of each in turn, every one between its own pair of events -> {name: [ms]}."""
    import torch
    ev = {k: [] for k in fns}
    for i in range(warmup + iters):
        for k, fn in fns.items():
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e[0].record()
            fn()
            e[1].record()
            if i >= warmup:
                ev[k].append(e)
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def step_kernels(args, dev):
    import numpy as np
    import torch
    from bench import Telemetry
    from yolo_amd import lib as L
    from yolo_amd.overlay import FrameOverlay
    lib = L.load()
    frames = _frames(0).to(dev)
    spare = torch.empty_like(frames)
    pred, lp, rows, kept, count = [torch.from_numpy(a).to(dev) for a in _rows(1)]
    ov = FrameOverlay(camera=CAMERA, device=dev)
    ovl = FrameOverlay(camera=CAMERA, device=dev, labels=True, names=['car', 'truck'])
    font = ovl.font
    dirs = torch.tensor([[1.0, 0.0], [-1.0, 0.0]], dtype=torch.float32, device=dev)      # two classes: 0 and 180 degrees
    pose = torch.empty((BATCH, 4), dtype=torch.float32, device=dev)
    L.check(lib.yolo_pose_top1(L.ptr(pred), BATCH, 8, L.ptr(dirs), None, 0, 0, 0, None, L.ptr(pose), L.stream_ptr()), 'pose_top1')
    H, W = SRC_HW
    out = {'src': list(SRC_HW), 'batch': BATCH, 'warmup': args.warmup, 'iters': args.iters, 'clock': 'HIP events',
           'frame_batch_bytes': int(frames.numel())}
    torch.cuda.synchronize()
    tel = Telemetry(dev.index or 0).start()
    for name, kw in (('top1_plate', dict(pred=pred, lp=lp)), ('nms100', dict(nms=(rows, kept, count)))):
        work = frames.clone()
        ov(work, **kw)                                                  # builds the table (and the buffers) this load's kernels read
        table, K = ov.table, int(ov.table.shape[1])
        torch.cuda.synchronize()
        tab = table.cpu().numpy()
        s = L.stream_ptr()

        def draw():
            L.check(lib.yolo_overlay_draw(L.ptr(work), L.ptr(table), BATCH, H, W, 3, K, s), 'overlay_draw')

        def copy():
            spare.copy_(frames)

        def whole():
            ov(work, **kw)

        # the same load with labels: the label table FrameOverlay(labels=True) makes, then its two kernels through the ABI
        kwl = dict(kw, pose=pose) if name == 'top1_plate' else kw
        ovl(work, **kwl)
        labels = ovl.labels
        torch.cuda.synchronize()
        assert torch.equal(ovl.table, table)
        lab = labels.cpu().numpy()
        fnt = ovl._font

        def text():
            L.check(lib.yolo_overlay_text(L.ptr(work), L.ptr(labels), L.ptr(fnt), font.nglyph, font.first_code, font.cell_w, font.cell_h,
                                          font.advance, 1, 1, BATCH, H, W, 3, K, s), 'overlay_text')

        if name == 'top1_plate':
            def make_labels():
                L.check(lib.yolo_overlay_labels(L.ptr(table), None, None, None, None, 0, 0, 0, 1, L.ptr(pred), 8, L.ptr(pose), 1, L.ptr(lp),
                                                L.ptr(ovl._names), 2, font.cell_w, font.cell_h, font.advance, 1, 4, 1, 1, 0xff000000,
                                                BATCH, H, W, K, L.ptr(labels), s), 'overlay_labels')
        else:
            def make_labels():
                L.check(lib.yolo_overlay_labels(L.ptr(table), L.ptr(rows), L.ptr(kept), L.ptr(count), None, 400, 8, 100, 2, None, 0, None,
                                                1, None, L.ptr(ovl._names), 2, font.cell_w, font.cell_h, font.advance, 1, 4, 1, 1,
                                                0xff000000, BATCH, H, W, K, L.ptr(labels), s), 'overlay_labels')

        def whole_labels():
            ovl(work, **kwl)

        r = {'K': K, 'enabled_slots': int((tab[:, :, 10] != 0).sum()), 'enabled_labels': int((lab[:, :, 4] & 1).sum()),
             'label_chars': int(lab[:, :, 5].sum())}
        alt = _events_alternating({'draw': draw, 'd2d_copy': copy, 'labels': make_labels, 'text': text}, args.warmup, args.iters)
        assert np.array_equal(labels.cpu().numpy(), lab)                # the ABI call made the table FrameOverlay made
        r['overlay_draw'], r['d2d_copy_of_the_frames'] = _stat(alt['draw']), _stat(alt['d2d_copy'])
        r['overlay_labels'], r['overlay_text'] = _stat(alt['labels']), _stat(alt['text'])
        r['text_over_draw'] = r['overlay_text']['median_ms'] / r['overlay_draw']['median_ms']
        r['whole_call_with_labels'] = _stat(_events(whole_labels, args.warmup, args.iters))     # + yolo_overlay_labels + yolo_overlay_text
        r['draw_over_copy'] = r['overlay_draw']['median_ms'] / r['d2d_copy_of_the_frames']['median_ms']
        r['d2d_copy_gb_per_s'] = 2 * frames.numel() / (r['d2d_copy_of_the_frames']['median_ms'] * 1e-3) / 1e9
        r['whole_call'] = _stat(_events(whole, args.warmup, args.iters))           # shapes (+ warp) + draw as FrameOverlay launches them
        # the shapes kernel alone (and the plate's warp alone): through the ABI, on the buffers the call above made
        if name == 'top1_plate':
            cam = ov.camera
            mats, valid, verts = ov.matrices, torch.empty((BATCH,), dtype=torch.uint8, device=dev), ov.vertices
            clipped = torch.empty((BATCH, 3, 160, 380), dtype=torch.float32, device=dev)

            def shapes_abi():
                L.check(lib.yolo_overlay_shapes(None, None, None, 0, 0, 0, 1, None, 0, L.ptr(pred), 8, 0.5, 0, 0xff00ff00, L.ptr(lp),
                                                cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h, 0.5, 0xffff0000, 160, 380, BATCH, H, W,
                                                2, L.ptr(table), K, L.ptr(verts), L.ptr(mats), L.ptr(valid), s), 'overlay_shapes')

            def warp():
                L.check(lib.yolo_warp_u8_to_nchw(L.ptr(frames), L.ptr(clipped), L.ptr(mats), None, BATCH, H, W, 3, 160, 380, 0, 0, 0,
                                                 W - 1, H - 1, s), 'warp')
            r['plate_warp'] = _stat(_events(warp, args.warmup, args.iters))
        else:
            pal = ov._palette

            def shapes_abi():
                L.check(lib.yolo_overlay_shapes(L.ptr(rows), L.ptr(kept), L.ptr(count), 400, 8, 100, 2, L.ptr(pal), int(pal.shape[0]),
                                                None, 0, 0.5, 0, 0, None, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.5, 0, 160, 380, BATCH, H, W, 2,
                                                L.ptr(table), K, L.ptr(ov.vertices), None, None, s), 'overlay_shapes')
        before = table.clone()
        r['overlay_shapes'] = _stat(_events(shapes_abi, args.warmup, args.iters))
        assert torch.equal(before[:, :, :8], table[:, :, :8]) and torch.equal(before[:, :, 10], table[:, :, 10])
        out[name] = r
        print(name, json.dumps(r), flush=True)
        del work
    out.update(tel.stop())
    return out


def step_host(args, dev):
    import numpy as np
    import torch
    from PIL import Image, ImageDraw
    from yolo_amd import intake, render
    cam = render.PlateCamera(CAMERA)
    host = _frames(0).numpy()
    pred_d, lp_d = [torch.from_numpy(a).to(dev) for a in _rows(1)[:2]]
    H, W = SRC_HW
    ms, parts = [], {'d2h_rows': [], 'plate_matrix': [], 'pil_lines': [], 'h2d_matrices': []}
    for i in range(1 + args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred, lp = pred_d.cpu().numpy(), lp_d.cpu().numpy()             # the blocking D2H
        t1 = time.perf_counter()
        mats = np.stack([intake.plate_matrix(p[1:7].astype(np.float64), cam, SRC_HW) for p in lp])
        t2 = time.perf_counter()
        for n in range(BATCH):
            img = Image.fromarray(host[n])
            d = ImageDraw.Draw(img)
            b = pred[n]
            h, w = b[3] * H, b[4] * W
            box = [(b[2] * W + sx * w / 2, b[1] * H + sy * h / 2) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
            d.line(box + box[:1], fill=(0, 255, 0), width=2)
            c = cam.corners(lp[n, 1:7])
            pts = [(float(x), float(y)) for x, y in c]
            d.line(pts + pts[:1], fill=(0, 0, 255), width=2)
            host[n] = np.asarray(img)
        t3 = time.perf_counter()
        md = torch.from_numpy(mats.astype(np.float32)).to(dev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if i:
            ms.append((t4 - t0) * 1e3)
            for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                parts[k].append(v * 1e3)
    r = dict(_stat(ms), src=list(SRC_HW), batch=BATCH, iters=args.host_iters, clock='time.perf_counter around device synchronises',
             shapes='top-1 box + plate edges per frame', parts_median_ms={k: _stat(v)['median_ms'] for k, v in parts.items()})
    r['frames_per_s'] = BATCH / (r['median_ms'] * 1e-3)
    print(json.dumps(r), flush=True)
    del md
    return r


def step_video(args, dev):
    import torch
    from oracle import graph as og, detect as od
    from yolo_amd.net import CarNet
    from yolo_amd.detect import Detector
    from yolo_amd.intake import FrameIntake
    from yolo_amd.overlay import FrameOverlay
    spec = og.spec_d53()
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    net = CarNet(spec, dtype=args.dtype, device=dev).initialize(seed=1234)
    det = Detector(spec, SIZE, steps, device=dev)
    intake = FrameIntake(SIZE, device=dev)
    ov = FrameOverlay(camera=CAMERA, car_threshold=0.0, device=dev)     # (an untrained net: draw whatever it predicts)
    ovl = FrameOverlay(camera=CAMERA, car_threshold=0.0, device=dev, labels=True, names=['az%03d' % (15 * k) for k in range(det.C - 6)])
    resident = _frames(0).to(dev)
    lp = torch.from_numpy(_rows(1)[1]).to(dev)
    pinned = torch.empty(resident.shape, dtype=torch.uint8, pin_memory=True)
    annotated = torch.empty_like(resident)

    def plain():
        det.predict_device(net(intake(resident)))
        pinned.copy_(intake.frames, non_blocking=True)

    def with_overlay():
        pred, _ = det.predict_device(net(intake(resident)))
        out, _, _ = ov(intake.frames, pred=pred, lp=lp, out=annotated)
        pinned.copy_(out, non_blocking=True)

    def with_labels():
        pred, _ = det.predict_device(net(intake(resident)))
        pose, _ = det.pose_device(pred)
        out, _, _ = ovl(intake.frames, pred=pred, lp=lp, pose=pose, out=annotated)
        pinned.copy_(out, non_blocking=True)

    routes = {'without_overlay': plain, 'with_overlay': with_overlay, 'with_overlay_and_labels': with_labels}
    for fn in routes.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    wall = {k: [] for k in routes}
    block = max(1, args.iters // 5)
    for _ in range(5):                                                  # alternating blocks: both routes see the same box
        for k, fn in routes.items():
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) / block * 1e3)
    out = {'net': 'D53', 'dtype': args.dtype, 'tune': 'auto', 'src': list(SRC_HW), 'size': list(SIZE), 'batch': BATCH,
           'steps_per_block': block, 'blocks': 5, 'clock': 'time.perf_counter over a block of steps, one device synchronise at its end',
           'd2h_bytes_per_step': int(resident.numel()), 'overlay_draws_into': 'out= (a device copy of the frames is part of the overlay '
           'route: the intake\'s frames stay as they came)'}
    for k, v in wall.items():
        out[k] = dict(_stat(v), frames_per_s=BATCH / (float(sorted(v)[len(v) // 2]) * 1e-3))
    out['overlay_cost_ms_per_step'] = out['with_overlay']['median_ms'] - out['without_overlay']['median_ms']
    out['labels_cost_ms_per_step'] = out['with_overlay_and_labels']['median_ms'] - out['with_overlay']['median_ms']
    print(json.dumps(out), flush=True)
    return out


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/overlay_bench.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    res = {'kernels': step_kernels, 'host': step_host, 'video': step_video}[args.child](args, dev)
    if args.child_out:
        with open(args.child_out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'result': res}, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dtype', default='bf16', help='arithmetic path of the net in the video step')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-iters', type=int, default=5)
    ap.add_argument('--steps', default=','.join(s for s, _ in STEPS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'overlay_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-out', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {'tool': 'tools/overlay_bench.py', 'warmup': args.warmup}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step, seconds in STEPS:
        if step not in args.steps.split(','):
            continue
        part = '%s.%s.part' % (args.out, step)
        cmd = ['timeout', '-k', '10', str(seconds), sys.executable, os.path.abspath(__file__), '--child', step, '--child-out', part,
               '--dtype', args.dtype, '--warmup', str(args.warmup), '--iters', str(args.iters), '--host-iters', str(args.host_iters)]
        rc = subprocess.call(cmd)
        if rc != 0:                                           # a fault, an abort or a time limit: nothing more is started on the GPU
            sys.exit('overlay_bench: step %r ended with status %d; stopping' % (step, rc))
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
