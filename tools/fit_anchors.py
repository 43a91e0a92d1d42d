#!/usr/bin/env python
"""The reference's `kmean` mode (car/YOLO.py:599-638) with this package: sample box sizes from the renderer's labels
(RenderCar.draw_params -- no pixel is drawn), fit k anchors by IoU k-means on the device (fit_anchors, csrc/anchors.hip), and print

  each anchor as the reference does       [h, w] = [...], area = ...            (car/YOLO.py:630)
  the all_anchors block, ready for spec.yaml
  anchor_quality of the spec's CURRENT anchors on the same sample, for comparison

  tools/fit_anchors.py SPEC --sprites ROOT [--pascal ROOT] [--size H W] [--n 1000] [--k 9] [--restarts 16]

SPEC is a spec.yaml in the reference's schema (`all_anchors`, `classes`, `size`), or one of the built-in names `micro` (the test
suite's small net at 64 x 96) and `d53` (car/v1's anchors at 416 x 416).  ROOT holds the sprite set as the reference lays it out
(ROOT/{train,valid}/<cad>/*_azi*_ele*.png); --synthetic draws on tools/render_bench.py's synthetic ellipses instead.  Without
--pascal the PASCAL3D+ share of the reference's sample (pascal_rate 0.2) is left out.  --host runs the numpy route (device=None)."""
import argparse
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def load_spec(name):
    if name == 'micro':
        from oracle import graph
        return dict(graph.spec_micro(), size=[64, 96])
    if name == 'd53':
        from yolo_amd.spec import darknet53_spec
        return dict(darknet53_spec(), size=[416, 416])
    import yaml
    with open(name) as f:
        return yaml.safe_load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('spec')
    ap.add_argument('--sprites', default=None, help='the PNG sprite root')
    ap.add_argument('--pascal', default=None, help='the PASCAL3D+ root (enables the reference\'s pascal_rate 0.2)')
    ap.add_argument('--synthetic', action='store_true', help='synthetic sprites instead of --sprites')
    ap.add_argument('--size', type=int, nargs=2, default=None, metavar=('H', 'W'))
    ap.add_argument('--n', type=int, default=1000, help='images sampled (the reference: 1000)')
    ap.add_argument('--k', type=int, default=None, help='anchors (default: as many as the spec has)')
    ap.add_argument('--restarts', type=int, default=16)
    ap.add_argument('--max-iters', type=int, default=300)
    ap.add_argument('--mode', default='train')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--host', action='store_true', help='the numpy route (device=None)')
    args = ap.parse_args()
    import numpy as np
    from yolo_amd import anchors as am
    from yolo_amd.render import RenderCar
    spec = load_spec(args.spec)
    size = args.size or spec.get('size')
    if not size:
        sys.exit('fit_anchors: the spec has no size: give --size H W')
    if not args.synthetic and not args.sprites:
        sys.exit('fit_anchors: give --sprites ROOT (or --synthetic)')
    classes = spec.get('classes') or [[15.0 * i, 0.0] for i in range(24)]
    current = spec['all_anchors']
    scales = len(current)
    k = args.k or sum(len(a) for a in current)
    device = None if args.host else 'cuda:0'
    with tempfile.TemporaryDirectory() as tmp:
        root = args.sprites
        if args.synthetic:
            from render_bench import write_sprites
            write_sprites(tmp, size=(max(8, size[0] * 5 // 8), max(8, size[1] * 24 // 25)))          # (260 x 400 at 416 x 416)
            root = tmp
        rc = RenderCar(size[0], size[1], classes, root, augment=False, pascal_root=args.pascal)
        random.seed(args.seed)
        np.random.seed(args.seed)
        sizes = am.sample_sizes(rc, args.n, args.mode, pascal_rate=0.2 if args.pascal else 0.0, render_rate=1.0)
    print('%d box sizes from %d images at %d x %d (%s)' % (len(sizes), args.n, size[0], size[1], 'numpy' if args.host else 'device'))
    fit = am.fit_anchors(sizes, k=k, restarts=args.restarts, max_iters=args.max_iters, device=device)
    for (h, w), c in zip(fit.anchors, fit.counts):
        print('[h, w] = [%.4f, %.4f], area = %.2f    (%d boxes)' % (h, w, h * w, c))
    print('all_means_cent = %s' % [float(fit.anchors[:, 0].mean()), float(fit.anchors[:, 1].mean())])
    print('mean IoU %.4f: restart %d of %d, %d rounds, %s; restarts spread %.4f .. %.4f' % (
        fit.mean_iou, fit.restart, args.restarts, fit.iters, 'converged' if fit.converged else 'NOT converged',
        fit.runs['mean_iou'].min(), fit.runs['mean_iou'].max()))
    if k % scales == 0:
        rows = fit.all_anchors(scales)
        print('  all_anchors:\n    [')
        for s, row in enumerate(rows):
            print('      [%s]%s' % (', '.join('[%.4f, %.4f]' % (h, w) for h, w in row), ',' if s + 1 < scales else '],'))
    else:
        print('(%d anchors do not divide into the spec\'s %d scales: no all_anchors block)' % (k, scales))
    q = am.anchor_quality(sizes, current, device=device)
    print('the spec\'s current anchors on this sample: mean IoU %.4f, boxes per anchor %s' % (q['mean_iou'], list(int(c) for c in q['counts'])))


if __name__ == '__main__':
    main()
