"""yolo_loss_fwd_bwd / yolo_loss_lp_fwd_bwd straight through the C ABI against tests/loss_ref.py (float64), on records built BY HAND so
that every branch of the loss kernel is reached on its own: saturated and tiny score logits, Huber differences on and around the
|d| = 1 seam, class logits that need the max subtraction, soft labels whose sum is not 1, records that collide, are invalid or sit
on the last live thread of a partial block.  nbox in {1, 255, 257, 10647 (D53 at 416 x 416)}, C up to the real head's 30.

Bars, derived (every unweighted gradient term is O(1): sigma - y in [-1, 1], a Huber gradient in [-1, 1], softmax * sum(y) - y bounded
by max(sum(y), 1); each takes a handful of fp32 operations with expf / logf at a few ulp):
  |dlogits - ref| <= 2e-6 * W * max(1, sum(y))   element-wise, W the element's own weight factor (0 on a background box's Huber and
                                                 class channels: those are exactly 0)
  |loss - ref|    <= 1e-5 * sum |term|           per loss and image (an fp32 wave / block reduction plus at most 42 atomic adds)

What each planted value tells apart (image 0 carries the moderate values, so its loss sums stay sharp; the extremes live in images 1
and 2):
  score 0, +-1e-4, 2, -0.7 sigma(x) - y at the centre, log1p(exp(-|x|)) at its maximum; an odd number of plants, so that a missing
                           -x*y term does not cancel between +x and -x in the loss sum
  score +-30 .. +-1e4      expf overflow / underflow in both the loss form and 1 / (1 + expf(-x)); a naive log(1 + exp(x)) is inf
  masked and unmasked      pos_w against neg_w, and the -x*y term
  Huber +-1, nextafter     both arms meet at |d| = 1 (0.5 and +-1), so whichever arm a value on or next to the seam takes, loss and
                           gradient must come out continuous: a wrong constant in either arm shows here.  (Where the seam LIES is
                           visible only to a value between the true and the wrong seam; 3, -2.5 and 1e4 sit in the linear arm.)
  every group, distinct    a group boundary moved by one channel changes the scale (0.01 / 10 / 0.7) and the width divisor
  class +80 / -80          the max subtraction (expf(80 - lse) without it is inf); all-equal logits the uniform softmax
  label sums 0.5 / 2 / 0   the `* sum(y)` factor of the gradient; an all-zero row gives loss 0 and gradient 0
  box 0, box nbox - 1      the first thread and the last live thread of a partial block
  invalid / colliding      `valid > 0` and last-record-wins; a box valid in image 0 only must be background in images 1 and 2
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import train as ot
from loss_ref import loss_ref

f32 = np.float32
B = 3
SCALES = tuple(f32(v) for v in (0.1, 0.01, 10.0, 0.7, 0.3))
POS_W, NEG_W = f32(2.5), f32(0.1)
HEADS = {'car': (5, 2, 2, 'yolo_loss_fwd_bwd'), 'lp': (6, 2, 1, 'yolo_loss_lp_fwd_bwd')}
GUARD = 64

ONE = f32(1)
# (2 and -0.7, 3 and -2.5: values inside each arm, and an odd count, so that the +x and -x plants do not cancel in a loss sum)
SCORE_MODERATE = [2.0, 0.0, 1e-4, -1e-4, 30.0, -30.0, -0.7]
SCORE_ALL = SCORE_MODERATE + [100.0, -100.0, 1e4, -1e4]
HUBER_MODERATE = [f32(3), ONE, -ONE, np.nextafter(ONE, f32(2)), np.nextafter(ONE, f32(0)), np.nextafter(-ONE, f32(-2)),
                  np.nextafter(-ONE, f32(0)), f32(0), f32(-2.5)]
HUBER_ALL = [f32(1e4)] + HUBER_MODERATE
LABEL_KINDS = ('one_hot', 'dist', 'half', 'double', 'zero')


def _label(kind, ncls, i):
    y = np.zeros(ncls, f32)
    if ncls == 0 or kind == 'zero':
        return y
    if kind == 'one_hot':
        y[i % ncls] = 1
        return y
    d = ot.get_label_dist(0.0, 0.37 + i, [[360.0 / ncls * c, 0.0] for c in range(ncls)])[1]
    return {'dist': d, 'half': f32(0.5) * d, 'double': f32(2) * d}[kind]


def _class_logits(pattern, ncls, i, rng):
    if pattern == 'equal':
        return np.full(ncls, 3.0, f32)
    if pattern == 'hot':
        v = np.full(ncls, -80.0, f32)
        if ncls:
            v[(i + 1) % ncls] = 80.0
        return v
    return (1.5 * rng.standard_normal(ncls)).astype(f32)


def build_case(head, nbox, Cc, nobj=None, seed=0):
    """-> logits (B, nbox, C) f32, records (B, nobj, 2 + nh + ncls) f32, and the planted (image, box) lists."""
    nh, g1, g2, _ = HEADS[head]
    ncls = Cc - 1 - nh
    nobj = nobj or (3 if nbox < 64 else 12)
    rng = np.random.default_rng(seed + 1000 * nbox + Cc)
    logits = (1.5 * rng.standard_normal((B, nbox, Cc))).astype(f32)
    rec = np.zeros((B, nobj, 2 + nh + ncls), f32)
    rec[..., 1] = rng.integers(0, nbox, (B, nobj))                                   # every record names a box, valid or not
    rec[..., 2:2 + nh] = rng.standard_normal((B, nobj, nh))
    rec[..., 2 + nh:] = rng.random((B, nobj, ncls))
    last, mid = nbox - 1, min(9, nbox - 1)
    # image 0: box 0, the last box, and an INVALID record that names box 0 again with other targets
    rec[0, :3, 0], rec[0, :3, 1] = (1, 1, 0), (0, last, 0)
    # image 1: two valid records on one box (the later one's targets win), and the last box; box 0 is background here
    rec[1, :3, 0], rec[1, :3, 1] = (1, 1, 1), (mid, mid, last)
    # image 2: no valid record at all, though its records name boxes 0, 5 and the last one
    rec[2, :, 0] = 0
    rec[2, :3, 1] = (0, min(5, last), last)
    if nobj > 3:                                                                     # further positives on distinct boxes, block edges first
        taken = {0, min(5, last), mid, last}
        pool = [k for k in (255, 256, 254, 63, 64, 127, 128, nbox - 2, nbox // 2) if 0 < k < last and k not in taken]
        pool = list(dict.fromkeys(pool))
        rest = [k for k in rng.permutation(nbox).tolist() if k not in taken and k not in pool]
        n = nobj - 3
        rec[0, 3:, 0], rec[0, 3:, 1] = 1, (pool + rest)[:n]
        rec[1, 3:, 0], rec[1, 3:, 1] = 1, (rest[n:2 * n - 2] + pool[:2])[:n]
    # ---- plant ----
    masked, unmasked = [], []
    for b in range(B):
        score_v = SCORE_MODERATE if b == 0 else SCORE_ALL
        huber_v = HUBER_MODERATE if b == 0 else HUBER_ALL
        patterns = ('random', 'equal') if b == 0 else ('random', 'equal', 'hot')
        win = {}
        for o in range(nobj):
            if rec[b, o, 0] > 0:
                win[int(rec[b, o, 1])] = o
        for i, (k, o) in enumerate(sorted(win.items())):
            masked.append((b, k))
            logits[b, k, 0] = score_v[i % len(score_v)]
            for j in range(nh):
                d = huber_v[(i + j) % len(huber_v)]
                y = f32(-0.25) if d > 0 else f32(0.25)               # chosen so that y + d and (y + d) - y are exact in fp32
                rec[b, o, 2 + j] = y
                logits[b, k, 1 + j] = f32(y + d)
                assert f32(logits[b, k, 1 + j] - rec[b, o, 2 + j]) == d and float(y) + float(d) == float(logits[b, k, 1 + j])
            rec[b, o, 2 + nh:] = _label(LABEL_KINDS[(i + b + 2) % 5], ncls, i)     # (a lone box: sum 0.5 in image 0, sum 2 in image 1)
            logits[b, k, 1 + nh:] = _class_logits(patterns[i % len(patterns)], ncls, i, rng)
        free = [k for k in range(nbox) if k not in win][:12]
        for u, k in enumerate(free):
            unmasked.append((b, k))
            logits[b, k, 0] = score_v[u % len(score_v)]
            for j in range(nh):
                logits[b, k, 1 + j] = huber_v[(u + j) % len(huber_v)]          # target 0: the difference is the logit
            logits[b, k, 1 + nh:] = _class_logits(patterns[u % len(patterns)], ncls, u, rng)
    return logits, rec, masked, unmasked


def _guarded(n, fill, cuda):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=cuda)
    return buf, buf[GUARD:GUARD + n]


def _run_and_check(lib, cuda, head, nbox, Cc, nobj=None):
    nh, g1, g2, entry = HEADS[head]
    logits, rec, masked, unmasked = build_case(head, nbox, Cc, nobj)
    nobj = rec.shape[1]
    ref = loss_ref(logits, rec, SCALES, POS_W, NEG_W, nh, g1, g2)
    assert np.isfinite(ref.losses).all() and np.isfinite(ref.dlogits).all()
    assert ref.mask[0].sum() == len({k for b, k in masked if b == 0}) and ref.mask[2].sum() == 0
    assert ref.mask[0, 0] == 1 and ref.mask[1, 0] == (1 if nbox == 1 else 0)       # box 0: positive in image 0 only
    xd = torch.from_numpy(logits).to(cuda)
    rd = torch.from_numpy(rec).to(cuda)
    dbuf, dl = _guarded(B * nbox * Cc, float('nan'), cuda)
    lbuf, ls = _guarded(5 * B, -3.0e30, cuda)                                     # garbage: the call zeroes the losses itself
    s5 = (C.c_float * 5)(*[float(v) for v in SCALES])
    st = torch.cuda.current_stream().cuda_stream
    rc = getattr(lib, entry)(xd.data_ptr(), rd.data_ptr(), dl.data_ptr(), ls.data_ptr(), B, nbox, Cc, nobj, s5, float(POS_W),
                             float(NEG_W), st)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, n, what in ((dbuf, B * nbox * Cc, 'dlogits'), (lbuf, 5 * B, 'losses')):
        g = torch.cat([buf[:GUARD], buf[GUARD + n:]]).cpu().numpy()
        assert (np.isnan(g).all() if what == 'dlogits' else (g == f32(-3.0e30)).all()), 'the margin of %s was written' % what
    d = dl.cpu().numpy().reshape(B, nbox, Cc)
    losses = ls.cpu().numpy().reshape(5, B)
    assert np.isfinite(d).all() and np.isfinite(losses).all()                     # every element written, nothing saturated to inf / NaN
    # gradient, element-wise
    ysum = np.ones((B, nbox, Cc))
    ysum[..., 1 + nh:] = np.maximum(1.0, ref.ysum)[..., None]
    bar = 2e-6 * ref.W * ysum
    err = np.abs(d.astype(np.float64) - ref.dlogits)
    live = bar > 0
    ratio_d = float((err[live] / bar[live]).max())
    print('RATIO %s nbox=%d C=%d dlogits %.3f' % (head, nbox, Cc, ratio_d))
    assert (err <= bar).all(), 'dlogits: worst ratio %.3g to the bar at %s' % (ratio_d, np.unravel_index(np.argmax(err - bar), err.shape))
    # a background box: Huber and class gradients exactly zero, bit for bit (+0)
    bg = ref.mask == 0
    assert (d[bg][:, 1:].view(np.int32) == 0).all()
    # losses
    lbar = 1e-5 * ref.abs_terms
    lerr = np.abs(losses.astype(np.float64) - ref.losses)
    pos = lbar > 0
    ratio_l = float((lerr[pos] / lbar[pos]).max())
    print('RATIO %s nbox=%d C=%d losses %.3f' % (head, nbox, Cc, ratio_l))
    assert (lerr <= lbar).all(), 'losses: worst ratio %.3g, got %s ref %s' % (ratio_l, losses, ref.losses)
    assert (losses[1:, 2] == 0).all()                                             # the image without object: a score loss only
    if Cc == 1 + nh:
        assert (losses[4] == 0).all()                                             # no class channel: class loss exactly 0
    return ratio_d, ratio_l


def test_planted_content_reaches_every_branch():
    """(CPU) the cases hold what the docstring claims: every score value, every Huber difference in each of the three groups, every
    class pattern with every label kind, on positive boxes; the same values on background boxes."""
    for head, Cc in (('car', 30), ('lp', 11)):
        nh, g1, g2, _ = HEADS[head]
        logits, rec, masked, unmasked = build_case(head, 257, Cc)
        ref = loss_ref(logits, rec, SCALES, POS_W, NEG_W, nh, g1, g2)
        for boxes, on in ((masked, 1), (unmasked, 0)):
            bb, kk = np.array(boxes).T
            assert (ref.mask[bb, kk] == on).all()
            assert set(float(f32(v)) for v in SCORE_ALL) <= set(logits[bb, kk, 0].astype(np.float64).tolist())
        bb, kk = np.array(masked).T
        win = np.array([max(o for o in range(rec.shape[1]) if rec[b, o, 0] > 0 and int(rec[b, o, 1]) == k) for b, k in masked])
        diff = logits[bb, kk, 1:1 + nh] - rec[bb, win, 2:2 + nh]
        for lo, hi in ((0, g1), (g1, g1 + g2), (g1 + g2, nh)):
            assert set(float(v) for v in HUBER_ALL) <= set(diff[:, lo:hi].astype(np.float64).ravel().tolist())
        sums = rec[bb, win, 2 + nh:].astype(np.float64).sum(-1)
        for want in (0.0, 0.5, 1.0, 2.0):
            assert (np.abs(sums - want) < 1e-6).any()
        assert (logits[bb, kk, 1 + nh:].max(-1) == 80).any() and (logits[bb, kk, 1 + nh:].min(-1) == -80).any()
        assert (0, 0) in masked and (0, 256) in masked and (1, 256) in masked and (0, 9) not in masked and (1, 9) in masked


@pytest.mark.gpu
@pytest.mark.parametrize('Cc', [6, 7, 10, 30])
@pytest.mark.parametrize('nbox', [1, 255, 257, 10647])
def test_car_loss_every_branch(lib, cuda, nbox, Cc):
    _run_and_check(lib, cuda, 'car', nbox, Cc)


@pytest.mark.gpu
@pytest.mark.parametrize('Cc', [8, 11])
@pytest.mark.parametrize('nbox', [1, 255, 257, 10647])
def test_lp_loss_every_branch(lib, cuda, nbox, Cc):
    _run_and_check(lib, cuda, 'lp', nbox, Cc)


@pytest.mark.gpu
@pytest.mark.parametrize('head,Cc', [('car', 10), ('lp', 11)])
def test_loss_records_nobj3(lib, cuda, head, Cc):
    """Three records per image and nothing else: positive / positive / invalid-on-a-positive-box in image 0, two valid records on
    one box in image 1 (the later one's targets win), no valid record in image 2."""
    _run_and_check(lib, cuda, head, 257, Cc, nobj=3)


@pytest.mark.gpu
def test_loss_refusals(lib, cuda):
    buf = torch.zeros(4096, device=cuda)
    s5 = (C.c_float * 5)(0.1, 0.01, 10.0, 0.7, 0.3)
    p = buf.data_ptr()
    assert lib.yolo_loss_fwd_bwd(p, p, p, p, 1, 4, 5, 1, s5, 1.0, 0.1, None) == -1          # C < 6: not a car head
    assert lib.yolo_loss_lp_fwd_bwd(p, p, p, p, 1, 4, 7, 1, s5, 1.0, 0.1, None) == -1       # C < 8: not an LP head
    assert lib.yolo_loss_fwd_bwd(p, p, p, p, 1, 0, 10, 1, s5, 1.0, 0.1, None) == -1
    assert lib.yolo_loss_fwd_bwd(p, None, p, p, 1, 4, 10, 1, s5, 1.0, 0.1, None) == -1
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0
