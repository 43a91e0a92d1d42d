"""The anchor kernels (csrc/anchors.hip: yolo_anchor_assign, yolo_anchor_kmeans) against the naive restatement of their definition
(tests/anchor_ref.py), and fit_anchors / anchor_quality on the device against the numpy route and the Detector's decode.

The shapes are the smallest at which the kernels can go wrong: n below a wave, one wave, ragged, one past the 1024-thread block and
three strides per thread plus one; k = 1, the k <= 9 and the k > 9 instantiations, and k = 32 (two walks of 16 clusters); dense
rows (8-byte loads) and a label-shaped tensor at an odd element offset (scalar loads, read in place)."""
import numpy as np
import pytest
import torch

import anchor_ref as ar
from yolo_amd import anchors as am
from yolo_amd import lib as L
from yolo_amd.detect import Detector

pytestmark = pytest.mark.gpu

NS, KS = (5, 64, 97, 1025, 3073), (1, 3, 9, 32)
_ROWS, _REF = {}, {}


def _rows(n):
    if n not in _ROWS:
        _ROWS[n] = ar.sizes(n, seed=n)
        _ROWS[n].setflags(write=False)
    return _ROWS[n]


def _cent(k):
    return ar.sizes(k, seed=1000 + k)


def _ref_assign(n, k):
    if (n, k) not in _REF:
        _REF[(n, k)] = ar.assign(_rows(n), _cent(k))
    return _REF[(n, k)]


def _ref_fit(n, k, seed):
    """The reference run of the (n, k) case: rows, init and ar.fit's result, made once."""
    key = ('fit', n, k, seed)
    if key not in _REF:
        rows = ar.sizes(n, seed=seed)
        init = rows[np.random.default_rng(100 + seed).choice(n, k, replace=False)]
        _REF[key] = (rows, init, ar.fit(rows, init, 300))
    return _REF[key]


FITS = ((97, 3, 3), (600, 9, 3))          # (n, k, seed): seeds whose reference run keeps every assignment margin >= 1e-5


def _up(a, cuda):
    return torch.from_numpy(np.array(a, order='C')).to(cuda)


def _label_tensor(rows, cuda, cols=30):
    """rows as columns 3:5 of a (n, 1, cols) label tensor that starts at an ODD element of its buffer: 4-byte aligned only."""
    n = len(rows)
    buf = torch.full((n * cols + 3,), -1.0, dtype=torch.float32, device=cuda)
    labels = buf[1:1 + n * cols].view(n, 1, cols)
    labels[:, 0, 3:5] = _up(rows, cuda)
    assert labels.data_ptr() % 8 == 4
    return labels


def _assign(lib, cuda, t, ptr, stride, n, cent, rows_out=True):
    k = len(cent)
    d_cent = _up(np.asarray(cent, np.float32), cuda)
    a = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    q = torch.full((n,), -7.0, dtype=torch.float32, device=cuda)
    counts = torch.full((k,), -7, dtype=torch.int32, device=cuda)
    mean = torch.full((1,), -7.0, dtype=torch.float64, device=cuda)
    nv = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    ws = torch.empty((lib.yolo_anchor_workspace_bytes(n, 1, k),), dtype=torch.uint8, device=cuda)
    rc = lib.yolo_anchor_assign(ptr, stride, n, L.ptr(d_cent), k, L.ptr(a) if rows_out else None, L.ptr(q) if rows_out else None,
                                L.ptr(counts), L.ptr(mean), L.ptr(nv), L.ptr(ws), L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    del t
    return dict(assign=a.cpu().numpy(), best_iou=q.cpu().numpy(), counts=counts.cpu().numpy(), mean_iou=float(mean.item()),
                n_valid=int(nv.item()))


def _assign_dense(lib, cuda, rows, cent, **kw):
    t = _up(rows, cuda)
    return _assign(lib, cuda, t, t.data_ptr(), 2, len(rows), cent, **kw)


def _kmeans(lib, cuda, rows, inits, max_iters=300):
    inits = np.asarray(inits, np.float32)
    R, k = inits.shape[:2]
    t, d_init = _up(rows, cuda), _up(inits, cuda)
    cent = torch.full((R, k, 2), -7.0, dtype=torch.float32, device=cuda)
    counts = torch.full((R, k), -7, dtype=torch.int32, device=cuda)
    mean = torch.full((R,), -7.0, dtype=torch.float64, device=cuda)
    iters, conv = (torch.full((R,), -7, dtype=torch.int32, device=cuda) for _ in range(2))
    nv = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    ws = torch.empty((lib.yolo_anchor_workspace_bytes(len(rows), R, k),), dtype=torch.uint8, device=cuda)
    rc = lib.yolo_anchor_kmeans(L.ptr(t), 2, len(rows), L.ptr(d_init), R, k, max_iters, L.ptr(cent), L.ptr(counts), L.ptr(mean),
                                L.ptr(iters), L.ptr(conv), L.ptr(nv), L.ptr(ws), L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return dict(centroids=cent.cpu().numpy(), counts=counts.cpu().numpy(), mean_iou=mean.cpu().numpy(), iters=iters.cpu().numpy(),
                converged=conv.cpu().numpy(), n_valid=int(nv.item()))


def _run_gap(rows, init):
    """The smallest best-to-second-best IoU margin along the numpy route's run from init (the precondition of a comparison between
    two routes whose double sums differ in their order), vectorised: the (600, 9) runs are too long for the row-by-row restatement
    to stay quick."""
    cent, gap = np.array(init, np.float32), np.inf
    for _ in range(300):
        h, w = rows[:, 0:1], rows[:, 1:2]
        inter = np.minimum(h, cent[None, :, 0]) * np.minimum(w, cent[None, :, 1])
        q = np.sort(inter / ((h * w + cent[None, :, 0] * cent[None, :, 1]) - inter), axis=1)
        gap = min(gap, float((q[:, -1] - q[:, -2]).min()))
        new = am._kmeans_host(rows, cent, 1)[0]
        if new.tobytes() == cent.tobytes():
            break
        cent = new
    return gap


def _same_assignment(got, ref):
    assert np.array_equal(got['assign'], ref['assign']) and np.array_equal(got['counts'], ref['counts'])
    assert np.array_equal(got['best_iou'].view(np.uint32), ref['best_iou'].view(np.uint32))
    assert got['n_valid'] == ref['n_valid']
    assert got['mean_iou'] == pytest.approx(ref['mean_iou'], rel=1e-12)


# ---- one assignment pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', NS)
def test_assign_equals_the_restatement(lib, cuda, n, k):
    rows, cent, ref = _rows(n), _cent(k), _ref_assign(n, k)
    _same_assignment(_assign_dense(lib, cuda, rows, cent), ref)
    # the same rows inside a label tensor, stride 30, from an odd element on
    labels = _label_tensor(rows, cuda)
    got = _assign(lib, cuda, labels, labels.data_ptr() + 12, 30, n, cent)
    _same_assignment(got, ref)
    # without the per-row outputs, and through the package on the tensor itself: the same sums, bit for bit
    bare = _assign(lib, cuda, labels, labels.data_ptr() + 12, 30, n, cent, rows_out=False)
    assert np.array_equal(bare['counts'], got['counts']) and bare['mean_iou'] == got['mean_iou'] and (bare['assign'] == -7).all()
    qual = am.anchor_quality(labels, cent.reshape(1, k, 2), device=cuda)
    assert qual['mean_iou'] == got['mean_iou'] and np.array_equal(qual['counts'], got['counts']) and qual['n_valid'] == n


def test_invalid_rows_are_assigned_nowhere(lib, cuda):
    rows = np.array(_rows(1025))
    bad = np.float32([[-1, -1], [0, 0.3], [0.3, 0], [np.nan, 0.2], [0.2, np.nan], [np.inf, 0.2], [0.2, np.inf], [-0.3, 0.3], [0.3, -np.inf]])
    at = np.arange(len(bad)) * 127 + 8                                      # interleaved; the last is row 1024, the one past the block
    rows[at] = bad
    cent = _cent(9)
    got, ref = _assign_dense(lib, cuda, rows, cent), ar.assign(rows, cent)
    _same_assignment(got, ref)
    assert (got['assign'][at] == -1).all() and (got['best_iou'][at] == 0).all()
    assert got['n_valid'] == 1025 - len(bad) == got['counts'].sum()
    none = _assign_dense(lib, cuda, np.tile(bad, (8, 1)), cent)
    assert none['n_valid'] == 0 and none['mean_iou'] == 0.0 and not none['counts'].any() and (none['assign'] == -1).all()
    assert not none['best_iou'].any()


def test_equal_centroids_give_the_rows_to_the_first(lib, cuda):
    rows = _rows(97)
    cent = np.float32([[0.3, 0.3], [0.5, 0.6], [0.3, 0.3], [0.5, 0.6]])
    got = _assign_dense(lib, cuda, rows, cent)
    _same_assignment(got, ar.assign(rows, cent))
    assert got['counts'][2] == 0 and got['counts'][3] == 0 and got['counts'][0] > 0 and got['counts'][1] > 0


# ---- the k-means ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,seed', FITS)
def test_kmeans_equals_the_restatement(lib, cuda, n, k, seed):
    rows, init, ref = _ref_fit(n, k, seed)
    # the precondition: along the reference's run no row's best and second-best IoU are closer than 1e-5, so a last-bit difference
    # in a double sum (2^-24 relative in a centroid, less in an IoU) cannot flip an assignment
    assert ref['gap'] >= 1e-5 and ref['converged'] and ref['iters'] > 3
    got = _kmeans(lib, cuda, rows, init[None])
    print('n %d k %d: iters %d / %d, centroid ulps %d, mean_iou %.17g / %.17g' % (
        n, k, got['iters'][0], ref['iters'], ar.ulp_diff(got['centroids'][0], ref['centroids']), got['mean_iou'][0], ref['mean_iou']))
    assert got['iters'][0] == ref['iters'] and got['converged'][0] == 1 and got['n_valid'] == n
    assert np.array_equal(got['counts'][0], ref['counts'])
    assert ar.ulp_diff(got['centroids'][0], ref['centroids']) <= 2
    assert got['mean_iou'][0] == pytest.approx(ref['mean_iou'], rel=1e-6)
    # a fixed point, with no margin needed: one reference step on what the device returned changes nothing
    assert ar.ulp_diff(ar.step(rows, got['centroids'][0]), got['centroids'][0]) <= 2
    # and the statistics are those of an assignment pass on the returned centroids
    again = _assign_dense(lib, cuda, rows, got['centroids'][0])
    assert np.array_equal(again['counts'], got['counts'][0]) and again['mean_iou'] == got['mean_iou'][0]


@pytest.mark.parametrize('k', (12, 32))
def test_fixed_point_with_more_than_nine_clusters(lib, cuda, k):
    """The 16-cluster walks (k = 12: one, k = 32: two): converged centroids stay put under one reference step, and the counts are
    the reference's on them."""
    rows = _rows(1025)
    init = rows[np.random.default_rng(k).choice(len(rows), k, replace=False)]
    got = _kmeans(lib, cuda, rows, init[None])
    assert got['converged'][0] == 1 and 1 < got['iters'][0] < 300
    assert ar.ulp_diff(ar.step(rows, got['centroids'][0]), got['centroids'][0]) <= 2
    ref = ar.assign(rows, got['centroids'][0])
    assert np.array_equal(got['counts'][0], ref['counts']) and got['mean_iou'][0] == pytest.approx(ref['mean_iou'], rel=1e-12)


def test_each_row_its_own_centroid_converges_at_once(lib, cuda):
    rows = _rows(5)
    got = _kmeans(lib, cuda, rows, rows[None])
    assert got['iters'][0] in (1, 2) and got['converged'][0] == 1 and got['mean_iou'][0] == 1.0
    assert np.array_equal(got['centroids'][0], rows) and list(got['counts'][0]) == [1] * 5


def test_an_empty_cluster_keeps_its_centroid(lib, cuda):
    rows = _rows(97)
    init = np.float32([[0.3, 0.3], [1e-3, 1e-3], [0.5, 0.6]])
    got, ref = _kmeans(lib, cuda, rows, init[None]), ar.fit(rows, init, 300)
    assert ref['gap'] >= 1e-5                                                # (the precondition of test_kmeans_equals_the_restatement)
    assert got['converged'][0] == 1 and got['counts'][0][1] == 0 and np.array_equal(got['centroids'][0][1], init[1])
    assert np.array_equal(got['counts'][0], ref['counts']) and got['counts'][0].sum() == 97
    assert ar.ulp_diff(got['centroids'][0], ref['centroids']) <= 2


def test_max_iters_stops_an_unfinished_run(lib, cuda):
    rows, init, ref = _ref_fit(*FITS[0])
    assert ref['iters'] > 1
    got = _kmeans(lib, cuda, rows, init[None], max_iters=1)
    assert got['iters'][0] == 1 and got['converged'][0] == 0
    want = ar.step(rows, init)
    assert ar.ulp_diff(got['centroids'][0], want) <= 2
    after = ar.assign(rows, got['centroids'][0])                              # the statistics: of the RETURNED centroids
    assert np.array_equal(got['counts'][0], after['counts']) and got['mean_iou'][0] == pytest.approx(after['mean_iou'], rel=1e-12)


def test_restarts_are_independent_and_repeatable(lib, cuda):
    rows = _rows(1025)
    rng = np.random.default_rng(7)
    inits = np.stack([rows[rng.choice(len(rows), 9, replace=False)] for _ in range(5)])
    all5, again = _kmeans(lib, cuda, rows, inits), _kmeans(lib, cuda, rows, inits)
    for key in ('centroids', 'counts', 'mean_iou', 'iters', 'converged'):
        assert all5[key].tobytes() == again[key].tobytes(), key
    assert len({c.tobytes() for c in all5['centroids']}) > 1                   # (different starts, different ends)
    for r in range(5):
        one = _kmeans(lib, cuda, rows, inits[r:r + 1])
        for key in ('centroids', 'counts', 'mean_iou', 'iters', 'converged'):
            assert one[key][0].tobytes() == all5[key][r].tobytes(), (key, r)


# ---- the package -------------------------------------------------------------------------------------------------------------
def test_fit_anchors_on_the_device_equals_the_numpy_route(lib, cuda):
    rows = _ref_fit(*FITS[1])[0]
    seed = 36                                                                # (a seed whose four runs keep the margin below)
    np.random.seed(seed)
    inits = [rows[np.random.choice(np.arange(len(rows)), 9, replace=False)] for _ in range(4)]
    assert min(_run_gap(rows, init) for init in inits) >= 1e-5               # the precondition, as in test_kmeans_equals_the_restatement
    np.random.seed(seed)
    host = am.fit_anchors(rows, k=9, restarts=4, device=None)
    fits = []
    for given in (rows, _up(rows, cuda), _label_tensor(rows, cuda)):           # numpy, dense tensor, label tensor read in place
        np.random.seed(seed)
        fits.append(am.fit_anchors(given, k=9, restarts=4, device=cuda))
    dev = fits[0]
    assert dev.restart == host.restart and dev.iters == host.iters and dev.converged and host.converged
    assert np.array_equal(dev.runs['iters'], host.runs['iters']) and np.array_equal(dev.counts, host.counts)
    assert ar.ulp_diff(dev.anchors, host.anchors) <= 2 and dev.mean_iou == pytest.approx(host.mean_iou, rel=1e-6)
    assert (np.diff(dev.anchors.prod(axis=1)) >= 0).all()
    for other in fits[1:]:                                                   # whichever way the rows arrive: the same bits
        assert np.array_equal(other.anchors, dev.anchors) and other.mean_iou == dev.mean_iou and other.restart == dev.restart
    with pytest.raises(ValueError):
        am.fit_anchors(rows[:5], k=9, device=cuda)


def test_the_device_route_refuses_the_shapes_the_numpy_route_refuses(lib, cuda):
    """No pointer is formed from a tensor of another shape: labels[:, :, 3:5] is (B, nobj, 2) with the labels' strides, and read as
    a label tensor it would give columns 6:8; (n, c != 2) would be read as its columns 0:2."""
    labels = _label_tensor(_rows(64), cuda, cols=7)
    wide = torch.ones((6, 3), dtype=torch.float32, device=cuda)
    for bad in (labels[:, :, 3:5], wide, wide[:, :1], torch.ones((2, 3, 4), dtype=torch.float32, device=cuda), wide[0]):
        for device in (cuda, None):
            with pytest.raises(ValueError):
                am.anchor_quality(bad, [[[0.3, 0.3]]], device=device)
            with pytest.raises(ValueError):
                am.fit_anchors(bad, k=1, device=device)
    # what the cut was meant to be: the two columns as dense rows, or the label tensor itself (7 floats a row: the last row's
    # h, w are the last floats read) -- the same bits either way, and the numpy route's figures
    cent = _cent(3).reshape(1, 3, 2)
    a = am.anchor_quality(labels, cent, device=cuda)
    b = am.anchor_quality(labels[:, 0, 3:5], cent, device=cuda)                # (n, 2) with stride 7: read in place
    c = am.anchor_quality(labels[:, 0, 3:5].contiguous(), cent, device=cuda)
    host = am.anchor_quality(labels.cpu().numpy(), cent, device=None)
    for got in (a, b, c):
        assert got['mean_iou'] == a['mean_iou'] and np.array_equal(got['counts'], host['counts']) and got['n_valid'] == 64
    assert a['mean_iou'] == pytest.approx(host['mean_iou'], rel=1e-12)
    empty = am.anchor_quality(torch.zeros((0, 2), dtype=torch.float32, device=cuda), cent, device=cuda)
    assert empty['n_valid'] == 0 and empty['mean_iou'] == 0.0 and not empty['counts'].any()


def test_fitted_anchors_are_what_the_detector_decodes(lib, cuda):
    """decode is exp(t) * anchor about the cell centre (csrc/detect.hip decode_axis): zero logits give boxes of the anchors' sizes.
    b - t = (c + a/2) - (c - a/2) with c < 1 and a < 1 (asserted): three roundings of numbers below 2, half an ulp (2^-24 * 2) each at most,
    so 2^-21 bounds the difference."""
    rows = _ref_fit(*FITS[1])[0]
    np.random.seed(22)
    fit = am.fit_anchors(rows, k=9, restarts=4, device=cuda)
    anchors = fit.all_anchors(3)
    assert fit.anchors.max() < 1
    assert am.anchor_quality(rows, anchors, device=cuda)['mean_iou'] == fit.mean_iou
    size, steps = (64, 96), [8, 16, 32]
    det = Detector({'all_anchors': anchors, 'slice_point': [1, 3, 5, 6, 8]}, size, steps, device=cuda)
    cells = [(size[0] // s) * (size[1] // s) for s in steps]
    dec = det.decode(torch.zeros((1, sum(cells), 3, 8), dtype=torch.float32, device=cuda)).cpu().numpy()[0]
    start = 0
    for i, ncell in enumerate(cells):
        boxes = dec[start:start + ncell * 3].reshape(ncell, 3, 8)
        start += ncell * 3
        hw = np.stack([boxes[:, :, 4] - boxes[:, :, 2], boxes[:, :, 3] - boxes[:, :, 1]], axis=-1)      # b - t, r - l
        assert np.abs(hw - fit.anchors[3 * i:3 * i + 3][None]).max() <= 2.0 ** -21, i
