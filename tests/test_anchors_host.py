"""CPU checks of the anchor fit's host side (yolo_amd/anchors.py: the numpy route, the result object, the sample) and of its C ABI
entries (declared, bound, revision still 5, bad arguments refused without a GPU); tests/anchor_ref.py is the naive restatement the
numpy route is held against."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import anchor_ref as ar
import render_ref as rr
from yolo_amd import anchors as am
from yolo_amd import lib as L
from yolo_amd import render

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = ('yolo_anchor_workspace_bytes', 'yolo_anchor_assign', 'yolo_anchor_kmeans')


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_anchor_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    for name, ret, nargs in zip(NAMES, ('long long', 'int', 'int'), (3, 12, 15)):
        assert name in L.SIGNATURES
        found = re.findall(r'^%s %s\(([^)]*)\);' % (ret, name), h, flags=re.M)                # the prototype, not a mention in a comment
        assert len(found) == 1
        proto = found[0]
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs
    assert (am.MAX_K, am.MAX_RESTARTS, am.MAX_ITERS) == (32, 65535, 10000)


def test_anchor_entries_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.yolo_anchor_workspace_bytes(1000, 16, 9) > 0
    for bad in ((0, 16, 9), (1000, 0, 9), (1000, 16, -1)):
        assert lib.yolo_anchor_workspace_bytes(*bad) == L.EINVAL
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    #         sizes stride n   cent k  assign best counts mean n_valid work stream
    assign = [p,    2,     64, p,   9, p,     p,   p,     p,   p,      p,   None]
    #         sizes stride n   init R  k  iters cent counts mean iters conv n_valid work stream
    kmeans = [p,    2,     64, p,   4, 9, 10,   p,   p,     p,   p,    p,   p,      p,   None]
    cases = ((lib.yolo_anchor_assign, assign, (0, 3, 7, 8, 9, 10), (2, 4), (8, 10), {4: 33}),
             (lib.yolo_anchor_kmeans, kmeans, (0, 3, 7, 8, 9, 10, 11, 12, 13), (2, 4, 5, 6), (9, 13), {5: 33, 4: 65536, 6: 10001}))
    for fn, ok, ptrs, sizes, doubles, beyond in cases:
        for k in ptrs:                                                      # a NULL required pointer
            a = list(ok); a[k] = None
            assert fn(*a) == L.EINVAL, k
        for k in sizes:                                                     # n, k, R, max_iters < 1
            for v in (0, -3):
                a = list(ok); a[k] = v
                assert fn(*a) == L.EINVAL, (k, v)
        for v in (1, 0, -2):                                                # stride < 2
            a = list(ok); a[1] = v
            assert fn(*a) == L.EINVAL, v
        for k in doubles:                                                   # a misaligned double* / workspace
            a = list(ok); a[k] = C.c_void_p(4100)
            assert fn(*a) == L.EINVAL, k
        for k, v in beyond.items():                                         # k > 32, R > 65535, max_iters > 10000
            a = list(ok); a[k] = v
            assert fn(*a) == L.EUNSUPPORTED, (k, v)
            a[k] = v - 1
            a[0] = None                                                     # (the limit itself passes that check: the NULL is found)
            assert fn(*a) == L.EINVAL, (k, v)
    # every YOLO_EINVAL condition comes before the YOLO_EUNSUPPORTED ones, whichever argument it is in
    for fn, ok, late, beyond in ((lib.yolo_anchor_assign, assign, (5, 6), {4: 33}),
                                 (lib.yolo_anchor_kmeans, kmeans, (7, 10, 11), {5: 33, 4: 65536, 6: 10001})):
        for k, v in beyond.items():
            for m in late:                                                  # a misaligned assign / best_iou; centroids / iters / converged
                a = list(ok); a[k] = v; a[m] = C.c_void_p(4098)
                assert fn(*a) == L.EINVAL, (k, m)
    a = list(assign); a[5] = a[6] = None                                    # assign / best_iou may be NULL: what is refused next is
    a[4] = 33                                                               # the k
    assert lib.yolo_anchor_assign(*a) == L.EUNSUPPORTED


def test_anchor_names_are_exported_lazily():
    """`import yolo_amd` alone loads neither the module nor torch (a fresh interpreter: this process has imported both); the first
    use of a name does."""
    code = ("import sys, yolo_amd; assert 'yolo_amd.anchors' not in sys.modules and 'torch' not in sys.modules; "
            "f = yolo_amd.fit_anchors; assert 'yolo_amd.anchors' in sys.modules and 'torch' not in sys.modules and f.__module__ == 'yolo_amd.anchors'")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, '-c', code], cwd=root, check=True, env=dict(os.environ, PYTHONPATH=root))
    import yolo_amd
    assert yolo_amd.fit_anchors is am.fit_anchors and yolo_amd.sample_sizes is am.sample_sizes
    assert yolo_amd.anchor_quality is am.anchor_quality and yolo_amd.AnchorFit is am.AnchorFit


# ---- the numpy route against the restatement ---------------------------------------------------------------------------------
def _inits(rows, k, restarts, seed):
    """fit_anchors' draw, restated: k distinct valid rows per restart from numpy's global generator."""
    valid = np.array([i for i in range(len(rows)) if ar.is_valid(rows[i, 0], rows[i, 1])])
    np.random.seed(seed)
    return [rows[np.random.choice(valid, k, replace=False)] for _ in range(restarts)]


def test_host_route_equals_the_restatement_from_the_same_seed():
    rows = ar.sizes(150, seed=2)
    rows[::7] = -1.0                                                        # 'no object' rows in between
    refs = [ar.fit(rows, init, 300) for init in _inits(rows, 4, 3, seed=9)]
    np.random.seed(9)
    fit = am.fit_anchors(rows, k=4, restarts=3, device=None)
    assert min(r['gap'] for r in refs) >= 1e-5                             # no assignment hangs on the last bit of a mean
    best = int(np.argmax([r['mean_iou'] for r in refs]))
    assert fit.restart == best and fit.iters == refs[best]['iters'] and fit.converged == bool(refs[best]['converged'])
    assert [r['iters'] for r in refs] == list(fit.runs['iters']) and all(fit.runs['converged'])
    np.testing.assert_allclose(fit.runs['mean_iou'], [r['mean_iou'] for r in refs], rtol=1e-12)
    order = np.argsort(refs[best]['centroids'].prod(axis=1), kind='stable')
    # the same assignments along the way and double sums of the same rows: the means differ by the order of the sum at most
    assert ar.ulp_diff(fit.anchors, refs[best]['centroids'][order]) <= 1
    assert np.array_equal(fit.counts, refs[best]['counts'][order]) and fit.counts.sum() == refs[best]['n_valid'] == 150 - 22
    assert fit.mean_iou == pytest.approx(refs[best]['mean_iou'], rel=1e-12)


def test_host_route_stops_at_max_iters_one_step_from_init():
    rows = ar.sizes(97, seed=1)
    init = _inits(rows, 3, 1, seed=4)[0]
    np.random.seed(4)
    fit = am.fit_anchors(rows, k=3, restarts=1, max_iters=1, device=None)
    assert fit.iters == 1 and not fit.converged
    want = ar.step(rows, init)
    assert ar.ulp_diff(fit.anchors, want[np.argsort(want.prod(axis=1), kind='stable')]) <= 1


def test_host_assignment_equals_the_restatement():
    rows = ar.sizes(200, seed=5)
    rows[[3, 50, 51, 120, 199]] = [[-1, -1], [0, 0.3], [np.nan, 0.2], [0.2, np.inf], [-0.3, 0.3]]
    cent = ar.sizes(9, seed=6)
    a, q, counts, mean_iou, n_valid = am._assign_host(rows, cent)
    ref = ar.assign(rows, cent)
    assert np.array_equal(a, ref['assign']) and np.array_equal(q.view(np.uint32), ref['best_iou'].view(np.uint32))
    assert np.array_equal(counts, ref['counts']) and n_valid == ref['n_valid'] == 195 and mean_iou == pytest.approx(ref['mean_iou'], rel=1e-12)
    qual = am.anchor_quality(rows, cent.reshape(3, 3, 2).tolist(), device=None)
    assert qual['n_valid'] == 195 and np.array_equal(qual['counts'], counts) and qual['mean_iou'] == mean_iou


def test_empty_cluster_keeps_its_centroid_and_ties_take_the_lowest_index():
    rows = ar.sizes(60, seed=8)
    cent = np.float32([[0.3, 0.3], [1e-3, 1e-3], [0.5, 0.6]])              # the second wins nothing: the reference would fail there
    new, counts, _, iters, converged = am._kmeans_host(rows, cent, 50)
    assert converged and counts[1] == 0 and counts[0] > 0 and counts[2] > 0 and counts.sum() == 60
    assert np.array_equal(new[1], cent[1]) and not np.array_equal(new[0], cent[0])
    assert np.array_equal(ar.fit(rows, cent, 50)['counts'], counts)
    a, _, counts, _, _ = am._assign_host(rows, np.float32([[0.3, 0.3], [0.5, 0.6], [0.3, 0.3]]))
    assert counts[2] == 0 and counts[0] > 0 and not (a == 2).any()          # of two equal centroids the first takes the rows


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def test_invalid_rows_are_dropped_and_too_few_valid_rows_are_refused():
    rows = ar.sizes(12, seed=3)
    rows[2:9] = [[-1, -1], [0, 0], [np.nan, 0.5], [0.5, np.inf], [-0.2, 0.2], [0.2, 0], [-np.inf, 1]]
    np.random.seed(0)
    fit = am.fit_anchors(rows, k=5, restarts=2, device=None)
    assert fit.counts.sum() == 5 and fit.mean_iou == 1.0                    # five valid rows, each its own anchor
    with pytest.raises(ValueError):
        am.fit_anchors(rows, k=6, restarts=2, device=None)
    with pytest.raises(ValueError):
        am.fit_anchors(rows[:, :1], k=1, device=None)
    # one shape rule for both calls: the sizes cut out of a label array are (B, nobj, 2), neither rows nor labels
    labels = -np.ones((4, 3, 30), np.float32)
    for bad in (labels[:, :, 3:5], rows[:, :1], np.ones((6, 3), np.float32), np.ones((2, 3, 4), np.float32), np.ones(6, np.float32)):
        with pytest.raises(ValueError):
            am.anchor_quality(bad, [[[0.3, 0.3]]], device=None)
        with pytest.raises(ValueError):
            am.fit_anchors(bad, k=1, device=None)
    empty = am.anchor_quality(np.zeros((0, 2), np.float32), [[[0.3, 0.3]]], device=None)
    assert empty['n_valid'] == 0 and empty['mean_iou'] == 0.0 and not empty['counts'].any()
    for bad in (dict(k=0), dict(k=33), dict(restarts=0), dict(max_iters=0), dict(max_iters=10001), dict(restarts=65536)):
        with pytest.raises(ValueError):
            am.fit_anchors(rows, device=None, **dict(dict(k=2), **bad))


def test_a_label_array_is_read_at_columns_three_and_four():
    rows = ar.sizes(24, seed=12)
    labels = -np.ones((8, 3, 30), np.float32)
    labels[:, :, 3:5] = rows.reshape(8, 3, 2)
    labels[5, 1] = -1.0                                                     # no object
    np.random.seed(1)
    a = am.fit_anchors(labels, k=3, restarts=2, device=None)
    np.random.seed(1)
    b = am.fit_anchors(np.delete(rows, 16, axis=0), k=3, restarts=2, device=None)
    assert np.array_equal(a.anchors, b.anchors) and np.array_equal(a.counts, b.counts) and a.counts.sum() == 23


# ---- the result object -------------------------------------------------------------------------------------------------------
def test_result_is_sorted_by_area_and_laid_out_like_the_spec():
    cent = np.float32([[[0.5, 0.5], [0.1, 0.2], [0.3, 0.1], [0.2, 0.2], [0.9, 0.1], [0.4, 0.4]],
                       [[0.5, 0.5], [0.1, 0.2], [0.3, 0.1], [0.2, 0.2], [0.9, 0.1], [0.4, 0.6]],
                       [[0.5, 0.5], [0.1, 0.2], [0.3, 0.1], [0.2, 0.2], [0.9, 0.1], [0.4, 0.7]]])
    counts = np.arange(18).reshape(3, 6)
    fit = am.AnchorFit(cent, counts, [0.5, 0.7, 0.7], [3, 4, 5], [1, 0, 1])
    assert fit.restart == 1 and fit.mean_iou == 0.7 and fit.iters == 4 and fit.converged is False      # the lowest index among equals
    assert np.array_equal(fit.anchors, np.float32([[0.1, 0.2], [0.3, 0.1], [0.2, 0.2], [0.9, 0.1], [0.4, 0.6], [0.5, 0.5]]))
    assert list(fit.counts) == [7, 8, 9, 10, 11, 6]
    assert list(fit.runs['iters']) == [3, 4, 5] and list(fit.runs['converged']) == [True, False, True]
    f = lambda v: float(np.float32(v))
    assert fit.all_anchors(3) == [[[f(0.1), f(0.2)], [f(0.3), f(0.1)]], [[f(0.2), f(0.2)], [f(0.9), f(0.1)]], [[f(0.4), f(0.6)], [f(0.5), f(0.5)]]]
    assert len(fit.all_anchors(2)) == 2 and len(fit.all_anchors(2)[0]) == 3 and len(fit.all_anchors(6)) == 6
    assert fit.all_anchors() == fit.all_anchors(3)
    for bad in (4, 5, 0):
        with pytest.raises(ValueError):
            fit.all_anchors(bad)


# ---- the sample --------------------------------------------------------------------------------------------------------------
def test_sample_sizes_are_draw_params_labels(tmp_path):
    rr.write_sprite_dir(str(tmp_path))
    rc = render.RenderCar(160, 256, rr.CLASSES, str(tmp_path), augment=False)
    random.seed(3); np.random.seed(3)
    got = am.sample_sizes(rc, 40, pascal_rate=0.0, render_rate=0.8, batch=16)
    random.seed(3); np.random.seed(3)
    labels = np.concatenate([rc.draw_params(b, 'train', 0.0, 0.8)[0] for b in (16, 16, 8)])
    has = labels[:, 0, 0] >= 0
    assert 0 < has.sum() < 40                                               # render_rate = 0.8 left some images empty
    assert got.dtype == np.float32 and np.array_equal(got, labels[has][:, 0, 3:5])
    # and the whole route: sample, fit, quality of the fit
    np.random.seed(5)
    fit = am.fit_anchors(got, k=3, restarts=4, device=None)
    assert am.anchor_quality(got, fit.all_anchors(3), device=None)['mean_iou'] == fit.mean_iou
    with pytest.raises(ValueError):                                         # the reference's pascal_rate needs the PASCAL3D+ crops
        am.sample_sizes(rc, 4)
