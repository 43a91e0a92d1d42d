#!/usr/bin/env python
"""What the arithmetic paths cost in DETECTIONS, not in box error (VERDICT Weak 5), and what an evaluation step costs in time.

Quality.  D53 at 416x416, batch 32, the seeded random-BN net and inputs of tests/test_gpu_boxes.py (configs[1]).  Ground truth = what
the f32 path detects: the candidates its per-class NMS keeps (Detector.decode_nms, defaults) with score >= --gt-score, one label
each (ltrb -> yxhw, class from the candidate id).  Every path -- f32 itself, bf16, f16, bf16x3, f16x3 -- is then scored against
those labels by yolo_amd.evaluate.Evaluator: mAP (IoU > 0.5, all-point AP over the classes that have ground truth), the number of
detections, and mean_iou = the path's top-1 box against the f32 path's top-1 box.  The top-1 figures come from a SECOND Evaluator
(mode 'obj') whose one label per image holds that box: object 0 of the NMS ground truth is not the top-1 box, so one set of labels
cannot serve both, and the second update repeats a decode + NMS whose matching is not used (a tool, not a hot path).  The f32 row is
the tool's own sanity check -- the path scored against itself: mAP must be exactly 1 and mean_iou 1 to rounding, or the tool fails.

Time.  Device time by HIP events of one WHOLE Evaluator.update -- its own decode + NMS and predict_top1 launches plus the two
evaluation kernels and the log copies, not the evaluation kernels alone (their cost: a rocprofv3 kernel trace) -- next to the forward
pass and the separate Detector.decode_nms call it follows, same run, at 416x416 batch 32 and 608x608 batch 64 (--dtype, default bf16, tune='auto');
median and minimum over --iters timed iterations after --warmup untimed ones, mean shader clock over the timed region.

Writes profiles/eval_paths.json (or --out).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import graph as og, detect as od                # noqa: E402
from yolo_amd.net import CarNet                             # noqa: E402
from yolo_amd.detect import Detector                        # noqa: E402
from yolo_amd.evaluate import Evaluator                     # noqa: E402

PATHS = ('f32', 'bf16', 'f16', 'bf16x3', 'f16x3')


def labels_from_detections(rows, kept, ks, cnt, ncls, gt_score):
    """Kept detections with score >= gt_score -> labels (B, post_nms, 6 + ncls) on the device, training layout, cls -1 elsewhere."""
    B, post_nms = kept.shape
    ok = (torch.arange(post_nms, device=kept.device)[None, :] < cnt[:, None]) & (ks >= gt_score) & (kept >= 0)
    ids = kept.clamp(min=0).to(torch.int64)
    box = torch.gather(rows[..., 1:5], 1, (ids // ncls)[..., None].expand(B, post_nms, 4))
    l, t, r, b = box.unbind(-1)
    lab = torch.full((B, post_nms, 6 + ncls), -1.0, dtype=torch.float32, device=kept.device)
    yxhw = torch.stack([(ids % ncls).to(torch.float32), (t + b) / 2, (l + r) / 2, b - t, r - l], dim=-1)
    lab[..., :5] = torch.where(ok[..., None], yxhw, lab[..., :5])
    return lab


def top1_labels(pred, ncls):
    """predict_top1 rows [score, y, x, h, w, rot, cls...] -> labels (B, 1, 6 + ncls): that box, class = its most likely one."""
    lab = torch.full((pred.shape[0], 1, 6 + ncls), -1.0, dtype=torch.float32, device=pred.device)
    lab[:, 0, 0] = pred[:, 6:].argmax(dim=1).to(torch.float32)
    lab[:, 0, 1:5] = pred[:, 1:5]
    return lab


def quality(dev, gt_score, batch):
    spec, size = og.spec_d53(), (416, 416)
    ncls = spec['slice_point'][-1] - 6
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = torch.from_numpy(np.random.default_rng(7).random((batch, 3) + size, dtype=np.float32)).to(dev)
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    det = Detector(spec, size, steps, device=dev)
    out, gt, gt_top = {}, None, None
    for dtype in PATHS:
        net = CarNet(spec, dtype=dtype, device=dev).load_params(P)
        outs = net(x)
        if dtype == 'f32':
            rows, _, kept, ks, cnt = det.decode_nms(outs, 'class')
            gt = labels_from_detections(rows, kept, ks, cnt, ncls, gt_score)
            gt_top = top1_labels(det.predict_device(outs)[0], ncls)
        ev = Evaluator(det, mode='class', max_images=batch)
        ev.update(outs, gt)
        top = Evaluator(det, mode='obj', max_images=batch)
        top.update(outs, gt_top)
        r, t = ev.result(), top.result()
        out[dtype] = {'mAP': r['mAP'], 'n_det': int(r['n_det'].sum()), 'n_gt': int(r['n_gt'].sum()),
                      'classes_with_gt': int((r['n_gt'] > 0).sum()), 'true_positives': int((ev.logs()['det_tp'] == 1).sum()),
                      'mean_iou': t['mean_iou'], 'azimuth_rmse_deg': t['azimuth_rmse_deg'], 'azimuth_images': t['azimuth_images']}
        print('%-7s %s' % (dtype, json.dumps(out[dtype])), flush=True)
        if dtype == 'f32':                                    # the path against itself: anything short of perfect is a bug of this tool
            o = out[dtype]
            bad = [what for what, ok in (('no ground truth at this --gt-score', o['n_gt'] > 0), ('mAP != 1', o['mAP'] == 1.0),
                                         ('a ground truth without its true positive', o['true_positives'] == o['n_gt']),
                                         ('top-1 IoU against itself != 1 (NaN: a zero-area top-1 box)', abs(o['mean_iou'] - 1.0) < 1e-5),
                                         ('a top-1 box below IoU 0.5 against itself', o['azimuth_images'] == batch)) if not ok]
            if bad:
                sys.exit('eval_paths: the f32 path scored against its own detections is not perfect (%s): %s' % ('; '.join(bad), json.dumps(o)))
        del net, outs
        torch.cuda.empty_cache()
    return {'net': 'D53 random-BN seed 0', 'size': list(size), 'batch': batch, 'input_seed': 7, 'gt_score': gt_score,
            'ground_truth': 'f32 path: per-class NMS kept (valid_thresh 0.01, iou_thresh 0.45, topk 400, post_nms 100), score >= gt_score',
            'iou_thresh': 0.5, 'paths': out}


def timing(dev, dtype, size, batch, warmup, iters):
    from bench import Telemetry
    spec = og.spec_d53()
    ncls = spec['slice_point'][-1] - 6
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    net = CarNet(spec, dtype=dtype, device=dev).initialize(seed=1234)
    det = Detector(spec, size, steps, device=dev)
    x = torch.rand((batch, 3) + size, generator=torch.Generator().manual_seed(3)).to(dev)
    outs = net(x)
    rows, _, kept, ks, cnt = det.decode_nms(outs, 'class')
    labels = labels_from_detections(rows, kept, ks, cnt, ncls, 0.0)
    ev = Evaluator(det, mode='class', max_images=batch * (warmup + iters))
    mark = lambda: torch.cuda.Event(enable_timing=True)
    tel, events = None, []
    for i in range(warmup + iters):                          # (no host wait inside the loop: the queue stays fed, as in bench.py)
        if i == warmup:
            torch.cuda.synchronize()
            tel = Telemetry(dev.index or 0).start()
        e = [mark() for _ in range(4)]
        e[0].record()
        outs = net(x)
        e[1].record()
        det.decode_nms(outs, 'class')
        e[2].record()
        ev.update(outs, labels)
        e[3].record()
        if i >= warmup:
            events.append(e)
    torch.cuda.synchronize()
    t = tel.stop()
    fwd, dec, upd = [[e[k].elapsed_time(e[k + 1]) for e in events] for k in range(3)]
    r = ev.result()
    st = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(np.min(v))}
    return {'dtype': dtype, 'tune': 'auto', 'size': list(size), 'batch': batch, 'warmup': warmup, 'iters': iters,
            'forward': st(fwd), 'decode_nms': st(dec), 'update': st(upd),
            'update_is': 'one whole Evaluator.update: its own decode_nms and predict_top1, yolo_eval_match, yolo_eval_top1, log copies',
            'sclk_mhz': t['sclk_mhz'], 'telemetry_source': t['telemetry_source'], 'images_logged': r['images'], 'mAP_self': r['mAP']}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--gt-score', type=float, default=0.1, help='f32 detections at or above this score are ground truth')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dtype', default='bf16', help='path timed')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--skip-timing', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_paths.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/eval_paths.py needs a GPU: the HIP path has no CPU fallback')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'quality': quality(dev, args.gt_score, args.batch), 'timing': []}
    if not args.skip_timing:
        for size, batch in (((416, 416), 32), ((608, 608), 64)):
            res['timing'].append(timing(dev, args.dtype, size, batch, args.warmup, args.iters))
            print(json.dumps(res['timing'][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
