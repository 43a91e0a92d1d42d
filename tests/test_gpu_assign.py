"""yolo_assign_targets straight through the C ABI against oracle.train.find_best, row by row, on the Darknet-53 anchor grid at
416 x 416 (10 647 boxes) and at 256 x 512 (img_h != img_w; 8 064 boxes; dyadic cell centres), nobj = 4, B = 3, 24 classes:
the layer look-up in each of the three scales, both clamps of the inverse sigmoid, the all-zero tie, an exact non-zero tie,
IoU = 1, a `cls < 0` row between valid ones, NaN coordinates.  The box index is bit-exact, the four targets within
rtol 1e-5 / atol 1e-6 (the bar of test_gpu_train.py::test_assign_targets), rotation and class columns copied bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import graph as og, detect as od, train as ot
from yolo_amd.detect import make_grid

f32 = np.float32
NCLS, NOBJ, B, GUARD = 24, 4, 3, 64
SIZES = [(416, 416), (256, 512)]


class Grid(object):
    def __init__(self, size):
        self.spec, self.size = og.spec_d53(), size
        self.AA = self.spec['all_anchors']
        self.steps = od.init_steps(self.spec['layers'], self.AA)
        self.area = od.init_area(size, self.steps)
        self.ltrb = od.get_default_ltrb(size, self.steps, self.AA)
        self.cum = np.cumsum([0] + self.area)
        self.desc, self.nbox = make_grid(self.AA, size, self.steps)
        assert self.nbox == 3 * sum(self.area)

    def layer_of(self, px):
        return int(np.searchsorted(self.cum, px, side='right') - 1)

    def best(self, L):
        with np.errstate(all='ignore'):
            px, anc, box = ot.find_best(L, self.ltrb, self.AA, self.size, self.steps, self.area)
        return px * 3 + anc, box

    def ious(self, L):
        with np.errstate(all='ignore'):
            return od.get_iou(self.ltrb, np.asarray(L[:5], f32)).reshape(-1)

    def anchor_box(self, px, anc):
        """A label equal to anchor box (px, anc)."""
        b, lay = self.ltrb[px, anc], self.layer_of(px)
        return [0, (b[1] + b[3]) / f32(2), (b[0] + b[2]) / f32(2), self.AA[lay][anc][0], self.AA[lay][anc][1]]

    def tie(self, lay, anc, mode, i, j):
        """A box centred on the edge between two neighbouring cells of scale `lay` and small enough to lie inside anchor `anc` of
        both: the two intersections are the label itself, and at 256 x 512 every cell centre is dyadic, so the two IoUs come out
        bit-equal (asserted by the caller on the oracle's IoUs).  mode 'h': cells (i, j) and (i, j + 1); 'v': (i, j) and (i + 1, j).
        -> label, lower index, higher index."""
        ah, aw = self.AA[lay][anc]
        sy, sx = self.steps[lay] / self.size[0], self.steps[lay] / self.size[1]
        gw = self.size[1] // self.steps[lay]
        k1 = (self.cum[lay] + i * gw + j) * 3 + anc
        if mode == 'h':
            L = [0, (i + 0.5) * sy, (j + 1) * sx, np.floor((ah - 0.01) * 256) / 256, np.floor((aw - sx - 0.01) * 256) / 256]
            return L, int(k1), int(k1 + 3)
        L = [0, (i + 1) * sy, (j + 0.5) * sx, np.floor((ah - sy - 0.01) * 256) / 256, np.floor((aw - 0.01) * 256) / 256]
        return L, int(k1), int(k1 + 3 * gw)


def _labels(g, which):
    """-> labels (B, NOBJ, 6 + NCLS) f32 and, per (image, object), what the row is there for."""
    rng = np.random.default_rng(7)
    lab = np.zeros((B, NOBJ, 6 + NCLS), f32)
    lab[..., 0] = rng.integers(0, NCLS, (B, NOBJ))
    lab[..., 1:3] = rng.uniform(.15, .85, (B, NOBJ, 2))
    lab[..., 3:5] = rng.uniform(.2, .8, (B, NOBJ, 2))
    lab[..., 5] = rng.uniform(-.5, .5, (B, NOBJ))
    lab[..., 6:] = rng.random((B, NOBJ, NCLS))
    tag = {}

    def put(b, o, what, L):
        lab[b, o, 1:5] = L[1:5]
        tag[(b, o)] = what
    nan = float('nan')
    if which == 'nan':
        for o, col in enumerate((1, 2, 3, 4)):
            lab[0, o, col] = nan
            tag[(0, o)] = 'nan'
        lab[1, 1, 1:5] = nan
        tag[(1, 1)] = 'nan'
        lab[1, 2, 0] = -1
        lab[2, :, 0] = -1                                                    # an image without object
        return lab, tag
    put(0, 0, 'scale0', [0, .3, .4, .2216, .1552])
    lab[0, 1, 0] = -1                                                        # `no object` between two valid rows
    put(0, 2, 'scale1', [0, .5, .5, .40, .27])
    put(0, 3, 'scale2', [0, .45, .55, .6, .7])
    put(1, 0, 'clamp_lo_hi', [0, -0.03, 1.04, .3, .3])                       # centre above and right of the image: sty -> 0.0001, stx -> 0.9999
    put(1, 1, 'clamp_hi_lo', [0, 1.03, -0.02, .5, .5])
    put(1, 2, 'far', [0, 5, 5, .3, .3])                                      # every IoU is 0: the tie resolves to box 0
    put(1, 3, 'equal', g.anchor_box(1234, 1))
    put(2, 2, 'equal', g.anchor_box(g.cum[2] + 5, 0))
    lab[2, 3, 0] = -1
    if g.size == (256, 512):
        put(2, 0, 'tie', g.tie(1, 1, 'h', 7, 15)[0])                         # neighbouring lanes of one wave
        put(2, 1, 'tie', g.tie(0, 2, 'v', 13, 40)[0])                        # 192 boxes apart: other waves of the block
    else:
        put(2, 0, 'far', [0, -3, -3, .4, .4])
        put(2, 1, 'scale0', [0, .71, .22, .2, .2])
    return lab, tag


@pytest.mark.parametrize('which', ['main', 'nan'])
@pytest.mark.parametrize('size', SIZES)
def test_label_conditions_hold_on_the_oracle(size, which):
    """(CPU) the labels do to the ORACLE what they are there for -- conditions of the GPU test, not results of it."""
    g = Grid(size)
    lab, tag = _labels(g, which)
    layers = set()
    for (b, o), what in sorted(tag.items()):
        L = lab[b, o]
        k, box = g.best(L)
        iou = g.ious(L)
        if what.startswith('scale'):
            assert g.layer_of(k // 3) == int(what[-1])
            layers.add(g.layer_of(k // 3))
        elif what == 'clamp_lo_hi':
            assert abs(box[0] + 9.2102) < 1e-3 and abs(box[1] - 9.2102) < 1e-3
        elif what == 'clamp_hi_lo':
            assert abs(box[0] - 9.2102) < 1e-3 and abs(box[1] + 9.2102) < 1e-3
        elif what == 'far':
            assert (iou == 0).all() and k == 0
        elif what == 'equal':
            assert abs(iou.max() - 1) < 1e-6 and (iou == iou.max()).sum() == 1 and k == int(np.argmax(iou))
        elif what == 'nan':
            assert np.isnan(iou).all() and k == 0 and np.isnan(box).any()
        elif what == 'tie':
            top = np.nonzero(iou == iou.max())[0]
            assert iou.max() > 0.5 and len(top) == 2 and k == top[0]         # two bit-equal IoUs: the lower index is the answer
    if which == 'main':
        assert layers == {0, 1, 2}
        if size == (256, 512):
            (L1, a1, b1), (L2, a2, b2) = g.tie(1, 1, 'h', 7, 15), g.tie(0, 2, 'v', 13, 40)
            assert g.best(np.asarray(L1 + [0], f32))[0] == a1 and g.best(np.asarray(L2 + [0], f32))[0] == a2
            assert b1 - a1 == 3 and b2 - a2 == 192 and (a2 % 256) // 64 != (b2 % 256) // 64
            assert sum(1 for v in tag.values() if v == 'tie') == 2


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['main', 'nan'])
@pytest.mark.parametrize('size', SIZES)
def test_assign_targets_direct(lib, cuda, size, which):
    g = Grid(size)
    lab, tag = _labels(g, which)
    W = 7 + NCLS
    buf = torch.full((B * NOBJ * W + 2 * GUARD,), float('nan'), device=cuda)
    rec = buf[GUARD:GUARD + B * NOBJ * W]
    labd = torch.from_numpy(lab).to(cuda)
    anchors = torch.from_numpy(g.ltrb).to(cuda).contiguous()
    rc = lib.yolo_assign_targets(labd.data_ptr(), anchors.data_ptr(), rec.data_ptr(), B, NOBJ, NCLS, C.byref(g.desc),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
    got = rec.cpu().numpy().reshape(B, NOBJ, W)
    worst = 0.0
    for b in range(B):
        for o in range(NOBJ):
            L, R = lab[b, o], got[b, o]
            what = tag.get((b, o), 'random')
            if L[0] < 0:
                assert R[0] == 0 and np.isnan(R[1:]).all(), (b, o)                         # marked invalid, nothing else written
                continue
            k, box = g.best(L)
            assert R[0] == 1 and R[1] == k, (what, b, o, R[1], k)                          # bit-exact index
            np.testing.assert_allclose(R[2:6], box, rtol=1e-5, atol=1e-6, equal_nan=True, err_msg=str((what, b, o)))
            ok = np.isfinite(box)
            if ok.any():
                worst = max(worst, float((np.abs(R[2:6][ok] - box[ok]) / (1e-6 + 1e-5 * np.abs(box[ok]))).max()))
            assert np.array_equal(R[6:].view(np.int32), L[5:].view(np.int32)), (what, b, o)  # rotation and classes: copied
    print('RATIO assign %dx%d %s targets %.3f' % (size[0], size[1], which, worst))
