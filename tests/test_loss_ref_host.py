"""tests/loss_ref.py (the float64 restatement the GPU loss tests compare with) against the oracle's own gluon losses
(oracle.train.logistic_loss / huber_loss / softmax_ce_loss) and torch autograd, on random logits with hand-built masks: the car head
(nh = 5, groups 2/2/1) and the LP head (nh = 6, groups 2/1/3), five distinct non-zero scales, a positive weight that is not 1 and
soft labels whose sums are not 1.  fp32 torch against float64: 1e-5 of the largest gradient, 1e-5 on the losses."""
import numpy as np
import pytest
import torch

from oracle import train as ot
from loss_ref import loss_ref

SCALES = (0.1, 0.01, 10.0, 0.7, 0.3)
POS_W, NEG_W = 2.5, 0.1
HEADS = {'car': (5, 2, 2), 'lp': (6, 2, 1)}


def _case(head, ncls, seed, B=3, nbox=50, nobj=4):
    nh, g1, g2 = HEADS[head]
    rng = np.random.default_rng(seed)
    C = 1 + nh + ncls
    logits = (1.5 * rng.standard_normal((B, nbox, C))).astype(np.float32)
    rec = np.zeros((B, nobj, 2 + nh + ncls), np.float32)
    rec[..., 2:2 + nh] = rng.standard_normal((B, nobj, nh))
    y = rng.random((B, nobj, ncls)) ** 3
    y = y / y.sum(-1, keepdims=True) * rng.choice([0.5, 1.0, 1.0, 2.0], (B, nobj, 1))    # soft labels; some rows do not sum to 1
    rec[..., 2 + nh:] = y
    for b in range(B):
        rec[b, :, 1] = rng.choice(nbox, nobj, replace=False)
        rec[b, :, 0] = 1
    rec[0, 1, 0] = 0                                   # an invalid record that names a box
    rec[1, 2, 1] = rec[1, 0, 1]                        # two valid records on one box: the later one's targets
    rec[2, :, 0] = 0                                   # an image without object
    return logits, rec, nh, g1, g2, ncls


def _dense(rec, B, nbox, nh, ncls):
    """The masks and targets by hand, as the reference's scatter loop writes them (car/YOLO.py:466-479): in order, overwriting."""
    mask = np.zeros((B, nbox, 1), np.float32)
    tgt = np.zeros((B, nbox, nh + ncls), np.float32)
    for b in range(B):
        for r in rec[b]:
            if r[0] > 0:
                mask[b, int(r[1])] = 1
                tgt[b, int(r[1])] = r[2:]
    return mask, tgt


def _oracle(logits, rec, nh, g1, g2, ncls, scales=SCALES, pos_w=POS_W, neg_w=NEG_W):
    B, nbox, C = logits.shape
    mask, tgt = _dense(rec, B, nbox, nh, ncls)
    x = torch.from_numpy(logits).requires_grad_(True)
    m, t = torch.from_numpy(mask), torch.from_numpy(tgt)
    sw = torch.from_numpy(ot.score_weight(mask, pos_w, neg_w))
    a, b_ = 1 + g1, 1 + g1 + g2
    losses = [ot.logistic_loss(x[..., :1], m, sw * scales[0]),
              ot.huber_loss(x[..., 1:a], t[..., :g1], m * scales[1]),
              ot.huber_loss(x[..., a:b_], t[..., g1:g1 + g2], m * scales[2]),
              ot.huber_loss(x[..., b_:1 + nh], t[..., g1 + g2:nh], m * scales[3]),
              ot.softmax_ce_loss(x[..., 1 + nh:], t[..., nh:], m * scales[4])]
    sum(l.sum() for l in losses).backward()
    return np.stack([l.detach().numpy() for l in losses]), x.grad.numpy(), (mask, tgt, sw)


@pytest.mark.parametrize('head,ncls', [('car', 4), ('car', 24), ('car', 1), ('lp', 1), ('lp', 4)])
def test_loss_ref_agrees_with_the_oracle_losses(head, ncls):
    logits, rec, nh, g1, g2, ncls = _case(head, ncls, seed=11 + ncls)
    ref_l, ref_g, _ = _oracle(logits, rec, nh, g1, g2, ncls)
    got = loss_ref(logits, rec, SCALES, POS_W, NEG_W, nh, g1, g2)
    live = ref_l[:4 if ncls == 1 else 5]                                   # (one class: softmax is 1 and the class loss 0)
    assert (live[:, :2] != 0).all() and (ref_l[1:, 2] == 0).all()          # every loss is live; the empty image has a score loss only
    np.testing.assert_allclose(got.losses, ref_l, rtol=1e-5, atol=0)
    assert np.abs(got.dlogits - ref_g).max() <= 1e-5 * np.abs(ref_g).max()
    # what the tolerances of the GPU tests are made of
    assert got.W.shape == logits.shape and (got.W[..., 0] > 0).all()
    assert ((got.W[..., 1:] > 0) == (got.mask[..., None] > 0)).all()
    assert (got.abs_terms >= np.abs(got.losses) * (1 - 1e-12)).all()


def test_loss_ref_agrees_with_get_loss_and_get_loss_lp():
    """The same through the oracle's own five-loss functions, with the car head's rotation term switched on."""
    logits, rec, nh, g1, g2, ncls = _case('car', 4, seed=5)
    mask, tgt = _dense(rec, 3, logits.shape[1], nh, ncls)
    scale = dict(zip(('score', 'box_yx', 'box_hw', 'rotate', 'class'), SCALES))
    x = torch.from_numpy(logits)
    cut = lambda a, pts: [a[..., i:j] for i, j in zip([0] + pts[:-1], pts)]
    sw = ot.score_weight(mask, POS_W, NEG_W)
    got = loss_ref(logits, rec, SCALES, POS_W, NEG_W, nh, g1, g2)
    ls = ot.get_loss(cut(x, [1, 3, 5, 6, 10]), [mask] + cut(tgt, [2, 4, 5, 9]), sw, mask, scale, car_rotate=True)
    np.testing.assert_allclose(got.losses, np.stack([l.numpy() for l in ls]), rtol=1e-5, atol=0)
    assert (got.losses[3, :2] > 0).all()
    ls = ot.get_loss(cut(x, [1, 3, 5, 6, 10]), [mask] + cut(tgt, [2, 4, 5, 9]), sw, mask, scale)          # car_rotate=False
    assert (np.stack([l.numpy() for l in ls])[3] == 0).all()
    logits, rec, nh, g1, g2, ncls = _case('lp', 4, seed=6)
    mask, tgt = _dense(rec, 3, logits.shape[1], nh, ncls)
    scale = dict(zip(('LP_score', 'LP_xy', 'LP_z', 'LP_r', 'LP_class'), SCALES))
    x = torch.from_numpy(logits)
    ls = ot.get_loss_LP(cut(x, [1, 3, 4, 7, 11]), [mask] + cut(tgt, [2, 3, 6, 10]), ot.score_weight(mask, POS_W, NEG_W), mask, scale)
    got = loss_ref(logits, rec, SCALES, POS_W, NEG_W, nh, g1, g2)
    np.testing.assert_allclose(got.losses, np.stack([l.numpy() for l in ls]), rtol=1e-5, atol=0)


def test_reference_step_keywords_reach_the_losses():
    """oracle.train.loss_and_grad_wrt_output(car_rotate=True, positive_weight, negative_weight): the rotation loss is live and equals
    loss_ref's third Huber group on the records the oracle's own assignment makes; the defaults leave it at zero."""
    from oracle import graph as og, detect as od
    spec, size = og.spec_micro(), (64, 96)
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    area = od.init_area(size, steps)
    ltrb = od.get_default_ltrb(size, steps, spec['all_anchors'])
    lab = ot.synthetic_labels(3, seed=9, render_rate=0.0, num_class=4)
    merged = (1.5 * np.random.default_rng(3).standard_normal((3, sum(area), 3, 10))).astype(np.float32)
    scale = dict(zip(('score', 'box_yx', 'box_hw', 'rotate', 'class'), SCALES))
    rl, rg, _ = ot.loss_and_grad_wrt_output(merged, lab, spec, size, scale, POS_W, NEG_W, car_rotate=True)
    rec = np.zeros((3, 1, 11), np.float32)
    for b in range(3):
        px, anc, box = ot.find_best(lab[b, 0], ltrb, spec['all_anchors'], size, steps, area)
        rec[b, 0] = np.concatenate([[1, px * 3 + anc], box, lab[b, 0, 5:]])
    got = loss_ref(merged.reshape(3, -1, 10), rec, SCALES, POS_W, NEG_W, 5, 2, 2)
    np.testing.assert_allclose(got.losses, np.stack(rl), rtol=1e-5, atol=0)
    assert (np.stack(rl)[3] > 0).all()
    assert np.abs(got.dlogits.reshape(rg.shape) - rg).max() <= 1e-5 * np.abs(rg).max()
    rl0, _, _ = ot.loss_and_grad_wrt_output(merged, lab, spec, size, scale, POS_W, NEG_W)
    assert (np.stack(rl0)[3] == 0).all()
