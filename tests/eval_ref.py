"""CPU restatement of the evaluation (test infrastructure only), written from its definition:

  match_image   PASCAL-VOC devkit matching of one image's ranked detections to its ground truth
  top1_image    the per-image arithmetic of _valid_iou (car/YOLO.py:514-526) + RadarProb.cls2ang (yolo_cv.py:85-95)
  ap_all_point  area under the monotone precision envelope (VOC 2010+), plain Python loops
  summarise     records -> the dict Evaluator.result() returns

IoUs are oracle.detect.box_iou_ltrb / get_iou: fp32, one rounding per operation."""
import math

import numpy as np

from oracle import detect as od

f32 = np.float32


def gt_ltrb(label):
    """[cls, y, x, h, w, ...] -> fp32 ltrb: l = x - w/2, t = y - h/2, r = x + w/2, b = y + h/2."""
    y, x, h, w = [f32(v) for v in label[1:5]]
    with np.errstate(all='ignore'):
        return np.asarray([x - w / f32(2), y - h / f32(2), x + w / f32(2), y + h / f32(2)], f32)


def match_image(rows, kept, kept_count, cand_per_box, labels, class_aware, iou_thresh):
    """rows (nbox, C); kept (post_nms,) candidate ids in score order; labels (nobj, >= 5).
    -> det_class, det_tp, det_gt (int32, post_nms), det_iou (float32, post_nms), gt_class (int32, nobj)."""
    post_nms, nobj, nbox = len(kept), labels.shape[0], rows.shape[0]
    det_class, det_tp, det_gt = [np.full(post_nms, -1, np.int32) for _ in range(3)]
    det_iou = np.zeros(post_nms, f32)
    gt_class = np.full(nobj, -1, np.int32)
    boxes = []
    for g in range(nobj):
        c = labels[g, 0]
        if c >= 0:                                            # (False for NaN)
            gt_class[g] = int(c) if class_aware else 0
        boxes.append(gt_ltrb(labels[g]))
    claimed = set()
    n = min(max(int(kept_count), 0), post_nms)
    for d in range(n):
        cid = int(kept[d])
        if cid < 0 or cid >= nbox * cand_per_box:
            continue                                          # a pad
        box = rows[cid // cand_per_box, 1:5].astype(f32)
        cls = cid % cand_per_box if class_aware else 0
        best, top = -1, -math.inf
        for g in range(nobj):
            if gt_class[g] < 0 or gt_class[g] != cls:
                continue
            with np.errstate(all='ignore'):
                v = float(od.box_iou_ltrb(box, boxes[g]))
            if v > top:
                best, top = g, v
        det_class[d], det_gt[d] = cls, best
        det_iou[d] = f32(top) if best >= 0 else f32(0)
        det_tp[d] = 0
        if best >= 0 and f32(top) > f32(iou_thresh):
            if best not in claimed:
                det_tp[d] = 1
            claimed.add(best)
    return det_class, det_tp, det_gt, det_iou, gt_class


def top1_image(pred_row, label0, class_dirs):
    """pred_row [score, y, x, h, w, rot, cls...], label0 [cls, y, x, h, w, ...] -> (iou, azimuth_rad, radius, valid)."""
    p = np.asarray(pred_row, f32)
    with np.errstate(all='ignore'):
        box = np.asarray([p[2] - p[4] / f32(2), p[1] - p[3] / f32(2), p[2] + p[4] / f32(2), p[1] + p[3] / f32(2)], f32)
        iou = float(od.get_iou(box, np.asarray(label0[:5], f32), mode=2)[0])
    prob = od.softmax(p[6:]).astype(np.float64)
    c = float(np.sum(np.asarray(class_dirs, np.float64)[:, 0] * prob))
    s = float(np.sum(np.asarray(class_dirs, np.float64)[:, 1] * prob))
    return iou, math.atan2(s, c), float(p[0]) * math.hypot(s, c), bool(label0[0] >= 0)


def ap_all_point(records, n_gt):
    """records: [(score, image, slot, tp)] of ONE class -> (AP, precision list, recall list).  Rank by score descending, ties by
    (image, slot) ascending."""
    recs = sorted(records, key=lambda r: (-float(r[0]), r[1], r[2]))
    tp = fp = 0
    prec, rec = [], []
    for r in recs:
        if r[3] == 1:
            tp += 1
        else:
            fp += 1
        prec.append(tp / float(tp + fp))
        rec.append(tp / float(n_gt) if n_gt else 0.0)
    ap, prev_r = 0.0, 0.0
    for i in range(len(recs)):
        if rec[i] != prev_r:
            ap += (rec[i] - prev_r) * max(prec[i:])           # the envelope: the best precision at this recall or beyond
            prev_r = rec[i]
    return ap, prec, rec


def summarise(det_class, det_tp, det_score, gt_class, top1, label_azimuth_deg, ncls):
    """Logs (images, post_nms) / (images, nobj) / (images, 4) / (images,) -> Evaluator.result()'s dict (without 'pr')."""
    images = len(top1)
    ap, n_gt, n_det = [float('nan')] * ncls, [0] * ncls, [0] * ncls
    for c in range(ncls):
        recs = [(det_score[i][k], i, k, int(det_tp[i][k])) for i in range(len(det_class)) for k in range(len(det_class[i]))
                if det_class[i][k] == c]
        n_gt[c] = int(sum(int(v == c) for row in gt_class for v in row))
        n_det[c] = len(recs)
        if n_gt[c]:
            ap[c] = ap_all_point(recs, n_gt[c])[0]
    with_gt = [ap[c] for c in range(ncls) if n_gt[c]]
    ious = [float(t[0]) for t in top1 if t[3] > 0]
    errs = []
    for t, az in zip(top1, label_azimuth_deg):
        if t[3] > 0 and f32(t[0]) >= f32(0.5):
            e = math.degrees(float(t[1])) - float(az)
            while e < -180:
                e += 360
            while e > 180:
                e -= 360
            errs.append(e * e)
    return {'images': images, 'mean_iou': sum(ious) / len(ious) if ious else float('nan'),
            'azimuth_rmse_deg': math.sqrt(sum(errs) / len(errs)) if errs else float('nan'), 'azimuth_images': len(errs),
            'ap': ap, 'mAP': sum(with_gt) / len(with_gt) if with_gt else float('nan'), 'n_gt': n_gt, 'n_det': n_det}
