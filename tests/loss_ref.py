"""CPU restatement of the loss kernel's contract (test infrastructure only), plain numpy float64, written from its definition
(car/YOLO.py:482-498, LP_detection.py:354-360):

  logits  (B, nbox, C)               [score | Huber group 1 (g1) | group 2 (g2) | group 3 (nh - g1 - g2) | class (C - 1 - nh)]
  records (B, nobj, 2 + nh + ncls)   [valid, box index, Huber targets (nh), soft class label (ncls)]

  mask      a box is positive when a record with valid > 0 names it; the LAST such record supplies its targets (the reference's
            scatter loop overwrites)
  score     LogisticLoss(binary):  max(x, 0) - x y + log1p(exp(-|x|)),  y = mask,  weight where(mask, pos_w, neg_w) * s_score
  Huber     HuberLoss(rho = 1) per group, weight mask * s_group, mean over the group's width
  class     soft-label softmax cross-entropy  -sum_c y_c log softmax(x)_c,  weight mask * s_class;  gradient softmax * sum(y) - y
  every term is divided by nbox (the mean over the boxes); losses[q, b] sums loss q over the boxes of image b.

loss_ref returns, besides the losses and d(sum of the losses)/d(logits), what a tolerance is made of: W, the weight factor each
gradient element carries (0 on the Huber and class channels of a background box), abs_terms, sum |term| per loss and image, and ysum,
the label sum of each box's winning record."""
import collections

import numpy as np

LossRef = collections.namedtuple('LossRef', 'losses dlogits W abs_terms mask ysum')


def winning_records(records, nbox):
    """-> (B, nbox) int: the index of the last valid record that names the box, -1 for a background box."""
    records = np.asarray(records)
    B, nobj = records.shape[:2]
    win = -np.ones((B, nbox), np.int64)
    for b in range(B):
        for o in range(nobj):
            if records[b, o, 0] > 0:
                k = int(records[b, o, 1])
                if 0 <= k < nbox:
                    win[b, k] = o
    return win


def loss_ref(logits, records, scales5, pos_w, neg_w, nh, g1, g2):
    x = np.asarray(logits, np.float64)
    rec = np.asarray(records, np.float64)
    B, nbox, C = x.shape
    ncls = C - 1 - nh
    assert ncls >= 0 and rec.shape[2] == 2 + nh + ncls and g1 >= 1 and g2 >= 1 and g1 + g2 <= nh
    s_score, s_1, s_2, s_3, s_cls = [float(v) for v in scales5]
    win = winning_records(rec, nbox)
    mask = (win >= 0).astype(np.float64)
    tgt = np.zeros((B, nbox, nh + ncls))
    bb, kk = np.nonzero(win >= 0)
    tgt[bb, kk] = rec[bb, win[bb, kk], 2:]
    inv_n = 1.0 / nbox
    d, W, terms = np.zeros_like(x), np.zeros_like(x), np.zeros((5, B, nbox))

    # score
    xs = x[..., 0]
    W[..., 0] = np.where(mask > 0, float(pos_w), float(neg_w)) * s_score * inv_n
    e = np.exp(-np.abs(xs))
    sig = np.where(xs >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    terms[0] = (np.maximum(xs, 0.0) - xs * mask + np.log1p(e)) * W[..., 0]
    d[..., 0] = (sig - mask) * W[..., 0]

    # the three Huber groups
    lo = 0
    for q, (width, s) in enumerate(((g1, s_1), (g2, s_2), (nh - g1 - g2, s_3))):
        if width == 0:
            continue
        ch = slice(1 + lo, 1 + lo + width)
        df = x[..., ch] - tgt[..., lo:lo + width]
        ad = np.abs(df)
        w = (mask * s * inv_n / width)[..., None]
        W[..., ch] = w
        terms[1 + q] = (np.where(ad > 1.0, ad - 0.5, 0.5 * ad * ad) * w).sum(-1)
        d[..., ch] = np.where(ad > 1.0, np.sign(df), df) * w
        lo += width

    # class
    ysum = np.ones((B, nbox))
    if ncls:
        xc, y = x[..., 1 + nh:], tgt[..., nh:]
        z = xc - xc.max(-1, keepdims=True)
        lse = np.log(np.exp(z).sum(-1, keepdims=True))
        w = (mask * s_cls * inv_n)[..., None]
        W[..., 1 + nh:] = w
        ysum = np.where(mask > 0, y.sum(-1), 1.0)
        terms[4] = -(y * (z - lse)).sum(-1) * w[..., 0]
        d[..., 1 + nh:] = (np.exp(z - lse) * y.sum(-1, keepdims=True) - y) * w
    return LossRef(terms.sum(-1), d, W, np.abs(terms).sum(-1), mask, ysum)
