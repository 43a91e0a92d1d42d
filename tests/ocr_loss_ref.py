"""yolo_ocr_targets, yolo_ocr_loss_fwd_bwd and yolo_ocr_score restated on the CPU (include/yolo_amd.h is the definition): the targets
in numpy and the losses in torch, both in a precision the caller names -- float32 is the reference's arithmetic, float64 the
yardstick the tests measure both against --, the gradient from torch autograd; the counts and the peak rule in plain Python."""
import numpy as np
import torch


def round_half_away(v):
    return int(np.sign(v) * np.floor(np.abs(v) + 0.5))


def targets(labels, order=None, Wp=24, dtype=np.float64):
    """labels (B,nobj,3) float32 -> (score_y (B,Wp) `dtype`, class_y (B,Wp) int32).  The labels keep their float32 values; the
    arithmetic on them is done in `dtype`."""
    labels = np.asarray(labels, np.float32)
    B, nobj = labels.shape[:2]
    score_y, class_y = np.zeros((B, Wp), dtype), -np.ones((B, Wp), np.int32)
    wp = dtype(Wp)
    for b in range(B):
        for p in range(nobj):
            k = p if order is None else int(order[b][p])
            if not 0 <= k < nobj:
                continue
            c, L1, L2 = (dtype(v) for v in labels[b, k])
            if not c >= 0:
                continue
            left, right = max(round_half_away(L1 * wp), 0), min(round_half_away(L2 * wp), Wp)
            for i in range(left, right):
                box_cent = (dtype(i) + dtype(0.5)) / wp
                text_cent = (L1 + L2) / dtype(2)
                score_y[b, i] = dtype(1) - abs(box_cent - text_cent) / (L2 - L1)
                class_y[b, i] = int(c)
    return score_y, class_y


def losses(logits, score_y, class_y, score_w=0.1, class_w=1.0, dtype=torch.float64, grad=False):
    """logits (B,Wp,1+ncls), score_y (B,Wp), class_y (B,Wp) -> losses (2,B) `dtype` (grad: and d sum(losses) / d logits)."""
    x = torch.as_tensor(np.asarray(logits, np.float32)).to(dtype).requires_grad_(grad)
    y = torch.as_tensor(np.asarray(score_y, np.float32)).to(dtype)
    k = torch.as_tensor(np.asarray(class_y)).to(torch.int64).clamp(0, x.shape[2] - 2)
    z, c = x[..., 0], x[..., 1:]
    score = (torch.relu(z) - z * y + torch.log1p(torch.exp(-z.abs()))).mean(dim=1) * score_w
    cls = (y * (torch.logsumexp(c, dim=-1) - c.gather(-1, k[..., None])[..., 0])).mean(dim=1) * class_w
    out = torch.stack([score, cls])
    if not grad:
        return out.detach().numpy()
    out.sum().backward()
    return out.detach().numpy(), x.grad.numpy()


def peaks(score, thr):
    """OCR.predict's rule (OCR/OCR.py:188-194): the columns i with s[i] > thr, s[i] > s[i+1] and s[i] > s[i-1], s[-1] = s[Wp] = 0."""
    s = np.concatenate(([0], np.asarray(score, np.float64), [0]))
    return [i for i in range(len(s) - 2) if s[i + 1] > thr and s[i + 1] > s[i + 2] and s[i + 1] > s[i]]


def levenshtein(a, b):
    d = list(range(len(a) + 1))
    for j, cb in enumerate(b, 1):
        prev, d[0] = d[0], j
        for i, ca in enumerate(a, 1):
            prev, d[i] = d[i], min(d[i] + 1, d[i - 1] + 1, prev + (ca != cb))
    return d[len(a)]


def truth_text(label):
    """The classes of the labels with class >= 0 whose centre lies in [0, 1), left to right (float32 centres, ties in label order)."""
    rows = [(np.float32(np.float32(L[1] + L[2]) / np.float32(2)), n, int(L[0])) for n, L in enumerate(np.asarray(label, np.float32)) if L[0] >= 0]
    return [c for mid, _, c in sorted(r for r in rows if 0 <= r[0] < 1)]


def score_counts(codes, count, labels, class_y, logits):
    """-> (B,6) int: truth length, predicted length, Levenshtein distance, exact match, labelled columns, right ones among them."""
    out = []
    for b in range(len(codes)):
        truth = truth_text(labels[b])
        pred = [int(c) for c in codes[b] if c >= 0][:int(count[b])]
        dist = levenshtein(truth, pred)
        lab = [i for i in range(len(class_y[b])) if class_y[b][i] >= 0]
        right = sum(int(np.argmax(logits[b][i][1:])) == int(class_y[b][i]) for i in lab)
        out.append([len(truth), len(pred), dist, int(dist == 0), len(lab), right])
    return np.asarray(out, np.int64)
