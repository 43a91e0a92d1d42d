"""Detection quality on the device: the reference's two tracked figures and the mAP its headline metric names.

  Evaluator.update(outs, labels)   <- YOLO._valid_iou's loop body   car/YOLO.py:514-526 (predict, rebuilt box, get_iou mode 2)
  Evaluator.result()['mean_iou']   <- its mean                      car/YOLO.py:528
  ...['azimuth_rmse_deg']          <- the azimuth RMSE over IoU >= 0.5 frames   car/YOLO.py:806-832
  ...['mAP'], ['ap'], ['pr']       <- new: PASCAL-VOC matching of what the per-class NMS keeps, all-point AP

update() launches the HIP kernels of csrc/eval.hip behind one decode_nms and one predict_device call and writes into preallocated
device logs at offsets the host knows; nothing is copied to the host before result(), which finishes in numpy (finish())."""
import numpy as np

from . import lib as L


def average_precision(score, tp, n_gt):
    """One class: detections in (image, slot) order with their scores and TP flags (1 / 0) -> (AP, precision, recall, scores
    in rank order).  Rank = score descending, ties in the given order (stable sort).  precision = TP / (TP + FP), recall =
    TP / n_gt; AP = area under the monotone precision envelope (VOC 2010+, all points)."""
    score = np.asarray(score, np.float32).reshape(-1)
    tp = np.asarray(tp).reshape(-1)
    order = np.argsort(-score, kind='stable')
    hit = (tp[order] == 1)
    ctp = np.cumsum(hit, dtype=np.float64)
    cfp = np.cumsum(~hit, dtype=np.float64)
    recall = ctp / float(n_gt) if n_gt > 0 else np.zeros_like(ctp)
    precision = ctp / np.maximum(ctp + cfp, 1.0)
    mrec = np.concatenate([[0.0], recall, [1.0]])
    mpre = np.concatenate([[0.0], precision, [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    step = np.nonzero(mrec[1:] != mrec[:-1])[0]                # the recall steps; consecutive ones share an end point
    ap = 0.0
    if len(step):
        # One term per run of steps at the same envelope height: (recall at the run's end - recall at its start) x height.
        # Summing step by step would be the same area, but n float terms of 1/n do not add up to exactly 1.0: with the runs
        # merged a ranking of true positives only is ONE term, (1.0 - 0.0) x 1.0, and its AP is exactly 1.
        height = mpre[step + 1]
        first = np.concatenate([[0], np.nonzero(height[1:] != height[:-1])[0] + 1])
        last = np.concatenate([first[1:] - 1, [len(step) - 1]])
        ap = float(np.sum((mrec[step[last] + 1] - mrec[step[first]]) * height[first]))
    return ap, precision, recall, score[order]


def wrap_deg(err):
    """Angle difference wrapped into [-180, 180) degrees (car/YOLO.py:818-821)."""
    return (np.asarray(err, np.float64) + 180.0) % 360.0 - 180.0


def finish(det_class, det_tp, det_score, gt_class, top1, label_azimuth_deg, ncls):
    """The numpy end of Evaluator.result(): logs of `images` images -> the result dict.
    det_class / det_tp / det_score (images, post_nms): class -1 marks a pad slot; gt_class (images, nobj): -1 = no object;
    top1 (images, 4) [iou, azimuth_rad, radius, valid]; label_azimuth_deg (images,)."""
    det_class, det_tp = np.asarray(det_class).reshape(-1), np.asarray(det_tp).reshape(-1)
    det_score = np.asarray(det_score, np.float32).reshape(-1)
    gt_class = np.asarray(gt_class)
    top1 = np.asarray(top1, np.float32).reshape(-1, 4)
    images = int(top1.shape[0])
    ap = np.full(ncls, np.nan)
    n_gt, n_det, pr = np.zeros(ncls, np.int64), np.zeros(ncls, np.int64), []
    for c in range(ncls):
        sel = det_class == c                                  # (boolean selection keeps the (image, slot) order)
        n_gt[c], n_det[c] = int(np.sum(gt_class == c)), int(np.sum(sel))
        a, p, r, s = average_precision(det_score[sel], det_tp[sel], n_gt[c])
        if n_gt[c] > 0:
            ap[c] = a
        pr.append({'precision': p, 'recall': r, 'score': s})
    valid = top1[:, 3] > 0
    iou = top1[:, 0].astype(np.float64)
    good = valid & (top1[:, 0] >= np.float32(0.5))
    err = wrap_deg(np.degrees(top1[good, 1].astype(np.float64)) - np.asarray(label_azimuth_deg, np.float64).reshape(-1)[good])
    return {'images': images,
            'mean_iou': float(np.mean(iou[valid])) if valid.any() else float('nan'),
            'azimuth_rmse_deg': float(np.sqrt(np.mean(err * err))) if good.any() else float('nan'),
            'azimuth_images': int(np.sum(good)),
            'ap': ap, 'mAP': float(np.mean(ap[n_gt > 0])) if (n_gt > 0).any() else float('nan'),
            'n_gt': n_gt, 'n_det': n_det, 'pr': pr}


class Evaluator(object):
    """ev = Evaluator(detector); ev.update(net(x), labels) per batch; ev.result() -> dict (see finish()); ev.reset().

    mode 'class': detections are (box, class) candidates matched to ground truths of their class; 'obj': boxes, one class 0.
    labels: (B, nobj, 6 + ncls) float32 in the training layout [cls, y, x, h, w, rot, dist...], cls < 0 = no object; a device
    tensor or a numpy array.  The label azimuth of an image is azimuth_deg[i] when given, else class_azimuth_deg[int(cls)] of
    its object 0 (default k * 360 / ncls, as deploy.py)."""

    def __init__(self, detector, mode='class', iou_thresh=0.5, post_nms=100, max_images=4096, class_azimuth_deg=None):
        import torch
        if mode not in ('class', 'obj'):
            raise ValueError("mode should be 'class' or 'obj'")
        self.det, self.mode = detector, mode
        self.iou_thresh, self.post_nms, self.max_images = float(iou_thresh), int(post_nms), int(max_images)
        self.ncls_net = detector.C - 6
        if self.ncls_net < 1:
            raise ValueError('the evaluation needs class logits (C > 6)')
        self.ncls = self.ncls_net if mode == 'class' else 1
        self.cpb = self.ncls_net if mode == 'class' else 1
        self._lib = L.load()
        if self.post_nms < 1 or self.max_images < 1 or self._lib.yolo_eval_match_supported(1, self.post_nms) != 1:
            raise ValueError('post_nms should be in 1..1024 and max_images positive')
        if class_azimuth_deg is None:
            class_azimuth_deg = [k * 360.0 / self.ncls_net for k in range(self.ncls_net)]
        az = np.asarray(class_azimuth_deg, np.float64).reshape(-1)
        if az.shape[0] != self.ncls_net:
            raise ValueError('class_azimuth_deg should have one entry per class')
        dev = detector.device
        dirs = np.stack([np.cos(np.radians(az)), np.sin(np.radians(az))], axis=1).astype(np.float32)
        self._dirs = torch.from_numpy(dirs).to(dev)
        self._class_az = torch.from_numpy(az.astype(np.float32)).to(dev)
        n, k = self.max_images, self.post_nms
        self._det_class = torch.empty((n, k), dtype=torch.int32, device=dev)
        self._det_tp = torch.empty((n, k), dtype=torch.int32, device=dev)
        self._det_gt = torch.empty((n, k), dtype=torch.int32, device=dev)
        self._det_iou = torch.empty((n, k), dtype=torch.float32, device=dev)
        self._det_score = torch.empty((n, k), dtype=torch.float32, device=dev)
        self._top1 = torch.empty((n, 4), dtype=torch.float32, device=dev)
        self._label_az = torch.empty((n,), dtype=torch.float32, device=dev)
        self._gt_class = None                                 # (max_images, nobj): allocated by the first update
        self.images = 0

    def reset(self):
        self.images = 0
        self._gt_class = None                                 # (the next update may bring another number of labels per image)

    def _labels(self, labels, B):
        import torch
        if isinstance(labels, np.ndarray):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float32))
        labels = labels.to(self.det.device, torch.float32).contiguous()
        if labels.dim() != 3 or labels.shape[0] != B or labels.shape[2] < 5:
            raise ValueError('expected labels of shape (%d, nobj, >= 5)' % B)
        nobj = int(labels.shape[1])
        if self._gt_class is None:
            if self._lib.yolo_eval_match_supported(nobj, self.post_nms) != 1:
                raise L.YoloError('at most 512 labels per image')
            self._gt_class = torch.empty((self.max_images, nobj), dtype=torch.int32, device=self.det.device)
        elif self._gt_class.shape[1] != nobj:
            raise ValueError('labels per image changed from %d to %d: reset() starts a new log' % (self._gt_class.shape[1], nobj))
        if self.images + B > self.max_images:
            raise L.YoloError('Evaluator holds max_images = %d images, %d + %d do not fit' % (self.max_images, self.images, B))
        return labels

    def _match(self, rows, kept, kept_scores, kept_count, labels):
        B, nbox, Cc = rows.shape
        i0, i1 = self.images, self.images + B
        L.check(self._lib.yolo_eval_match(L.ptr(rows), L.ptr(kept), L.ptr(kept_count), L.ptr(labels), B, nbox, Cc, self.cpb,
                                          self.post_nms, labels.shape[1], labels.shape[2], 1 if self.mode == 'class' else 0,
                                          self.iou_thresh, L.ptr(self._det_class[i0:i1]), L.ptr(self._det_tp[i0:i1]),
                                          L.ptr(self._det_gt[i0:i1]), L.ptr(self._det_iou[i0:i1]), L.ptr(self._gt_class[i0:i1]),
                                          L.stream_ptr()), 'eval_match')
        self._det_score[i0:i1].copy_(kept_scores)

    def update_detections(self, rows, kept, kept_scores, kept_count, labels):
        """Matching only, for detections made elsewhere (Detector.nms / decode_nms outputs with this Evaluator's post_nms and
        mode); the images count as invalid for the top-1 figures."""
        L.require_current_device(self.det.device, 'this Evaluator')
        rows, kept, kept_scores, kept_count = rows.contiguous(), kept.contiguous(), kept_scores.contiguous(), kept_count.contiguous()
        B = rows.shape[0]
        if tuple(kept.shape) != (B, self.post_nms) or tuple(kept_scores.shape) != (B, self.post_nms) or tuple(kept_count.shape) != (B,):
            raise ValueError('expected kept ids / scores of shape (%d, %d) and %d counts' % (B, self.post_nms, B))
        if rows.shape[2] != self.det.C:
            raise ValueError('expected rows of %d values' % self.det.C)
        labels = self._labels(labels, B)
        self._match(rows, kept, kept_scores, kept_count, labels)
        self._top1[self.images:self.images + B].zero_()
        self._label_az[self.images:self.images + B].zero_()
        self.images += B

    def update(self, outs, labels, azimuth_deg=None, **nms_kwargs):
        """One batch: outs = net.forward's outputs.  nms_kwargs go to Detector.decode_nms (valid_thresh, iou_thresh, topk)."""
        import torch
        if 'post_nms' in nms_kwargs or 'mode' in nms_kwargs:
            raise ValueError('post_nms and mode are fixed by the Evaluator')
        B = int((outs[0] if isinstance(outs, (list, tuple)) else outs).shape[0])
        labels = self._labels(labels, B)                      # shape and capacity are checked before anything is launched
        rows, _, kept, ks, cnt = self.det.decode_nms(outs, self.mode, post_nms=self.post_nms, **nms_kwargs)
        pred, _ = self.det.predict_device(outs)
        self._match(rows, kept, ks, cnt, labels)
        i0, i1 = self.images, self.images + B
        L.check(self._lib.yolo_eval_top1(L.ptr(pred), L.ptr(labels), L.ptr(self._dirs), L.ptr(self._top1[i0:i1]), B, self.det.C,
                                         labels.shape[1], labels.shape[2], L.stream_ptr()), 'eval_top1')
        if azimuth_deg is None:
            cls = labels[:, 0, 0].nan_to_num(nan=0.0).clamp(0, self.ncls_net - 1).to(torch.int64)
            self._label_az[i0:i1] = self._class_az[cls]
        else:
            if not torch.is_tensor(azimuth_deg):
                azimuth_deg = torch.from_numpy(np.ascontiguousarray(azimuth_deg, dtype=np.float32))
            self._label_az[i0:i1] = azimuth_deg.to(self.det.device, torch.float32).reshape(B)
        self.images = i1

    def logs(self):
        """The device logs of the images seen so far, copied to the host: dict of numpy arrays."""
        n = self.images
        nobj = 0 if self._gt_class is None else self._gt_class.shape[1]
        gt = self._gt_class[:n].cpu().numpy() if nobj else np.zeros((0, 1), np.int32)
        return {'det_class': self._det_class[:n].cpu().numpy(), 'det_tp': self._det_tp[:n].cpu().numpy(),
                'det_gt': self._det_gt[:n].cpu().numpy(), 'det_iou': self._det_iou[:n].cpu().numpy(),
                'det_score': self._det_score[:n].cpu().numpy(), 'gt_class': gt, 'top1': self._top1[:n].cpu().numpy(),
                'label_azimuth_deg': self._label_az[:n].cpu().numpy()}

    def result(self):
        g = self.logs()
        return finish(g['det_class'], g['det_tp'], g['det_score'], g['gt_class'], g['top1'], g['label_azimuth_deg'], self.ncls)
