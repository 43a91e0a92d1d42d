"""Guard bands and poisoned surroundings for the entry points the tests drive through hand-rolled calls.

The large kernels address through maximum-range buffer resources: an out-of-range offset means "no access", so nothing but a
kernel's own offset arithmetic keeps a tile tail, a strip seam or a channel tail inside its tensor.  Here every operand lies in a
moat of NaN and every output and workspace between two 1 MiB bands of 0xFF (tests/util.py: guarded / moated) at EXACTLY the size
the header promises; each test also holds the result against the reference of the entry's own test, so a pass means the kernel ran
on real work.  A changed guard byte, or a NaN a moat put into a result, is a bug of the kernel or its dispatcher (the header
promises no readable memory beyond a tensor); a read beyond a tensor whose value is discarded passes by construction.  The
shapes are the smallest that still have the tails; yolo_conv_fwd's plain calls are covered through util.run_conv."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import (TDT, LDT, guarded, guards_intact, moated, run_conv, ref_conv, to_nhwc, from_nhwc, conv_variant, split_planes)
from test_gpu_conv import STATS_ALGOS
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu


class Guards(object):
    """The guarded outputs of one test: out() hands out a view, check() synchronizes and names the one whose guard changed."""

    def __init__(self, dev):
        self.dev, self.pairs = dev, []

    def out(self, name, shape, tdt, prior=None):
        buf, view = guarded(shape, tdt, self.dev, prior=prior)
        self.pairs.append((name, buf, view))
        return view

    def check(self):
        torch.cuda.synchronize()
        for name, buf, view in self.pairs:
            try:
                guards_intact(buf, view)
            except AssertionError as e:
                raise AssertionError('%s: %s' % (name, e))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _packed(lib, dev, w, ldt):
    """yolo_pack_conv_weights image of w (numpy OIHW) at exactly its size, guards checked, as a moated operand."""
    co, ci, k, _ = w.shape
    buf, wp = guarded((lib.yolo_packed_weight_bytes(co, ci, k, ldt),), torch.uint8, dev)
    L.check(lib.yolo_pack_conv_weights(moated(torch.from_numpy(w).to(dev)).data_ptr(), wp.data_ptr(), co, ci, k, ldt, _st()), 'pack')
    torch.cuda.synchronize()
    guards_intact(buf, wp)
    return wp


def _padded(lib, dev, v):
    """A per-channel vector padded with zeros to yolo_padded_channels, in a moat."""
    t = torch.zeros(lib.yolo_padded_channels(len(v)), device=dev)
    t[:len(v)] = torch.from_numpy(np.asarray(v, np.float32)).to(dev)
    return moated(t)


def _bars(dtype):
    """(rtol, atol) of one stored ulp of the 16-bit conv outputs, as test_gpu_conv.py's test_conv_bf16 / test_conv_f16 set them."""
    return (1.6e-2, 2e-2) if dtype == 'bf16' else (2e-3, 2e-3)


# ---- the harness itself, broken by hand: it must notice ---------------------------------------------------------------------------
def test_a_short_view_and_a_short_moat_are_noticed(lib, cuda):
    """A convolution that writes its full map through a guarded y ONE ROW short changes the guard right behind the view, and one
    that reads an x moated ONE ELEMENT short carries the moat's NaN into its last pixels; the full-size control does neither.
    (Both land inside the harness's own buffers: that is what the guard bands are for.)"""
    N, Cin, H, W, Cout, k = 2, 32, 13, 13, 64, 3
    rng = np.random.default_rng(1)
    xn = to_nhwc(rng.standard_normal((N, Cin, H, W)).astype(np.float32), 'bf16', cuda)
    wp = _packed(lib, cuda, (rng.standard_normal((Cout, Cin, k, k)) / 17).astype(np.float32), L.BF16)

    def conv(x, y):
        d = L.ConvDesc()
        d.x, d.w_packed, d.y = x.data_ptr(), wp.data_ptr(), y.data_ptr()
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope = N, H, W, Cin, Cout, k, 1, L.BF16, 1.0
        assert lib.yolo_conv_fwd(C.byref(d), _st()) == 0
        torch.cuda.synchronize()

    xm = moated(xn)
    ybuf, y = guarded((N * H * W, Cout), torch.bfloat16, cuda)
    conv(xm, y)
    assert guards_intact(ybuf, y) and not bool(torch.isnan(y.float()).any())
    sbuf, short = guarded((N * H * W - W, Cout), torch.bfloat16, cuda)
    conv(xm, short)
    assert torch.equal(short.view(torch.int16), y[:N * H * W - W].view(torch.int16))
    nb = 2 * short.numel()
    with pytest.raises(AssertionError, match=r'behind the %d-byte view .* offset %d from the view' % (nb, nb)):
        guards_intact(sbuf, short)
    assert int((sbuf[-(1 << 20):] != 0xFF).sum()) >= W * Cout * 2 - 16           # one row of bf16 (a value's byte may be 0xFF itself)
    ybuf, y2 = guarded((N * H * W, Cout), torch.bfloat16, cuda)
    conv(moated(xn.flatten()[:-1]), y2)
    assert guards_intact(ybuf, y2) and bool(torch.isnan(y2[-1].float()).all()) and not bool(torch.isnan(y2[:N * H * W - W - 2].float()).any())


# ---- the first-stage kernels: stem, stem + statistics, stem + down, residual block, all four convs -------------------------------
_FIRST = {}


def _first_stage(lib, dev, dtype):
    """Weights and folded-BN constants of the stem, the first down-sampling conv and the first residual block (numpy), and
    their device images (moated), once per element type."""
    if dtype in _FIRST:
        return _FIRST[dtype]
    rng = np.random.default_rng(41)
    p = {'w0': (rng.standard_normal((32, 3, 3, 3)) / 5).astype(np.float32), 'wd': (rng.standard_normal((64, 32, 3, 3)) / 17).astype(np.float32),
         'w1': (rng.standard_normal((32, 64, 1, 1)) / 8).astype(np.float32), 'w2': (rng.standard_normal((64, 32, 3, 3)) / 17).astype(np.float32)}
    for n, c in (('0', 32), ('d', 64), ('1', 32), ('2', 64)):
        p['s' + n], p['b' + n] = rng.uniform(0.5, 1.5, c).astype(np.float32), (0.3 * rng.standard_normal(c)).astype(np.float32)
    d = {'w0': moated(torch.from_numpy(p['w0']).to(dev))}
    for n in ('wd', 'w1', 'w2'):
        d[n] = _packed(lib, dev, p[n], LDT[dtype])
    for n in ('0', 'd', '1', '2'):
        d['s' + n], d['b' + n] = _padded(lib, dev, p['s' + n]), _padded(lib, dev, p['b' + n])
    _FIRST[dtype] = (p, d)
    return p, d


def _dp(d, *names):
    return tuple(d[n].data_ptr() for n in names)


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(1, 37, 61), (3, 8, 8), (1, 2, 2)])
def test_stem_kernels(lib, cuda, shape, dtype):
    """yolo_stem_conv_fwd, yolo_stem_conv_fwd_stats with its partial rows (bf16; refused in half, nothing written) and
    yolo_stem_down_fwd: the stem against the oracle, the statistics variant's map bit-identical to it and its partial rows
    summing to the stored map's sums, the fused pair bit-identical to stem + yolo_conv_fwd and against the oracle of the pair."""
    N, H, W = shape
    ldt, tdt, sim = LDT[dtype], TDT[dtype], (True if dtype == 'bf16' else 'f16')
    p, d = _first_stage(lib, cuda, dtype)
    x = np.random.default_rng(H * 100 + W).random((N, 3, H, W), dtype=np.float32)
    xd = moated(torch.from_numpy(x).to(cuda))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = Guards(cuda)
    mid = g.out('stem y', (N, H, W, 32), tdt)
    assert lib.yolo_stem_conv_fwd(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0'), mid.data_ptr(), N, H, W, 3, 32, ldt, 0.1, _st()) == 0
    rows = lib.yolo_stem_stats_rows(N, H, W, 32)
    assert rows > 0
    y1 = g.out('stem+stats y', (N, H, W, 32), tdt)
    part = g.out('stem partial rows', (rows, 2, 32), torch.float32)
    rc = lib.yolo_stem_conv_fwd_stats(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0'), y1.data_ptr(), N, H, W, 3, 32, ldt, 0.1, part.data_ptr(), _st())
    assert rc == (0 if dtype == 'bf16' else L.EUNSUPPORTED)
    two = g.out('stem, conv y', (N, Ho, Wo, 64), tdt)
    dd = L.ConvDesc()
    dd.x, dd.w_packed, dd.scale, dd.bias, dd.y = (mid.data_ptr(),) + _dp(d, 'wd', 'sd', 'bd') + (two.data_ptr(),)
    dd.N, dd.H, dd.W, dd.Cin, dd.Cout, dd.ksize, dd.stride, dd.dtype, dd.slope = N, H, W, 32, 64, 3, 2, ldt, 0.1
    assert lib.yolo_conv_fwd(C.byref(dd), _st()) == 0
    one = g.out('stem_down y', (N, Ho, Wo, 64), tdt)
    assert lib.yolo_stem_down_fwd(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0', 'wd', 'sd', 'bd'), one.data_ptr(), N, H, W, 32, 64, ldt, 0.1, _st()) == 0
    g.check()
    rtol, atol = _bars(dtype)
    r1 = ref_conv(x, p['w0'], p['s0'], p['b0'], 1, 0.1, bf16=sim)
    got = from_nhwc(mid)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, r1, rtol=rtol, atol=atol)
    if dtype == 'bf16':
        assert torch.equal(y1.view(torch.int16), mid.view(torch.int16))
        assert bool(torch.isfinite(part).all())
        # fp32 partial sums of at most N H W values each: n 2^-24 sum|v| bounds any summation order
        v = mid.double().reshape(-1, 32)
        eps = v.shape[0] * 2.0 ** -24
        s = part.double().sum(dim=0)
        assert bool(((s[0] - v.sum(dim=0)).abs() <= eps * v.abs().sum(dim=0) + 1e-30).all())
        assert bool(((s[1] - (v * v).sum(dim=0)).abs() <= 2 * eps * (v * v).sum(dim=0) + 1e-30).all())
    else:
        assert bool(torch.isnan(y1.float()).all()) and bool(torch.isnan(part).all())
    assert not torch.isnan(one.float()).any()
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))
    r2 = ref_conv(r1, p['wd'], p['sd'], p['bd'], 2, 0.1, bf16=sim)
    tol = 2e-2 if dtype == 'bf16' else 3e-3                       # (test_stem_down_fused_is_bit_identical's bar)
    np.testing.assert_allclose(from_nhwc(one), r2, rtol=tol, atol=tol * np.abs(r2).max())


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('case', [(3, 5, 62, 64), (1, 33, 63, 64), (1, 40, 8, 128), (1, 21, 66, 128)])
def test_res_block(lib, cuda, case, dtype):
    """yolo_res_block_fwd against the torch reference with the HIP path's rounding points (test_res_block_fused's bars)."""
    ldt, tdt, sim = LDT[dtype], TDT[dtype], (True if dtype == 'bf16' else 'f16')
    k16 = 1.0 if dtype == 'bf16' else 0.125
    N, H, W, Cc = case
    rng = np.random.default_rng(21)
    x = rng.standard_normal((N, Cc, H, W)).astype(np.float32)
    w1 = (rng.standard_normal((Cc // 2, Cc, 1, 1)) / np.sqrt(Cc)).astype(np.float32)
    w2 = (rng.standard_normal((Cc, Cc // 2, 3, 3)) / np.sqrt(Cc // 2 * 9)).astype(np.float32)
    s1, b1 = rng.uniform(.5, 1.5, Cc // 2).astype(np.float32), (.3 * rng.standard_normal(Cc // 2)).astype(np.float32)
    s2, b2 = rng.uniform(.5, 1.5, Cc).astype(np.float32), (.3 * rng.standard_normal(Cc)).astype(np.float32)
    mid = ref_conv(x, w1, s1, b1, 1, 0.1, bf16=sim)
    ref = ref_conv(mid, w2, s2, b2, 1, 0.1, residual=x, bf16=sim)
    wp1, wp2 = _packed(lib, cuda, w1, ldt), _packed(lib, cuda, w2, ldt)
    ts1, tb1, ts2, tb2 = (_padded(lib, cuda, v) for v in (s1, b1, s2, b2))
    xd = moated(to_nhwc(x, dtype, cuda))
    g = Guards(cuda)
    y = g.out('y', (N, H, W, Cc), tdt)
    assert lib.yolo_res_block_fwd(xd.data_ptr(), wp1.data_ptr(), ts1.data_ptr(), tb1.data_ptr(), wp2.data_ptr(), ts2.data_ptr(),
                                  tb2.data_ptr(), y.data_ptr(), N, H, W, Cc, ldt, 0.1, _st()) == 0
    g.check()
    got = from_nhwc(y)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=2e-2 * k16, atol=3e-2 * k16)
    assert np.abs(got - ref).mean() < (2e-3 if dtype == 'bf16' else 5e-4)


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', [(1, 16, 16), (2, 64, 124), (3, 34, 32)])
def test_stem_res(lib, cuda, shape, dtype):
    """yolo_stem_res_fwd byte-identical to yolo_stem_down_fwd + yolo_res_block_fwd (test_stem_res_is_byte_identical's reference)."""
    N, H, W = shape
    ldt, tdt = LDT[dtype], TDT[dtype]
    p, d = _first_stage(lib, cuda, dtype)
    xd = moated(torch.from_numpy(np.random.default_rng(N * 1000003 + H * 1009 + W).random((N, 3, H, W), dtype=np.float32)).to(cuda))
    Ho, Wo = H // 2, W // 2
    g = Guards(cuda)
    mid, two, one = (g.out(n, (N, Ho, Wo, 64), tdt) for n in ('stem_down y', 'res_block y', 'stem_res y'))
    assert lib.yolo_stem_down_fwd(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0', 'wd', 'sd', 'bd'), mid.data_ptr(), N, H, W, 32, 64, ldt, 0.1, _st()) == 0
    assert lib.yolo_res_block_fwd(mid.data_ptr(), *_dp(d, 'w1', 's1', 'b1', 'w2', 's2', 'b2'), two.data_ptr(), N, Ho, Wo, 64, ldt, 0.1, _st()) == 0
    assert lib.yolo_stem_res_fwd(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0', 'wd', 'sd', 'bd', 'w1', 's1', 'b1', 'w2', 's2', 'b2'),
                                 one.data_ptr(), N, H, W, 32, 64, ldt, 0.1, _st()) == 0
    g.check()
    assert not torch.isnan(two.float()).any()
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))


# ---- yolo_conv_fwd: statistics epilogue, fused tail, strided / up-sampled buffers -------------------------------------------------
BOUNDS_STATS_CASES = [(5, 32, 7, 9, 16, 1, 1), (2, 32, 16, 24, 24, 3, 1), (2, 64, 21, 37, 32, 1, 1)]


@pytest.mark.parametrize('case,algo,mode', [pytest.param(c, a, m, id='%s-a%d-m%d' % ('x'.join(map(str, c)), a, m))
                                            for c in BOUNDS_STATS_CASES for a in STATS_ALGOS for m in (1, 2)
                                            if conv_variant(c, 'bf16', a, stats_mode=m) is not None])
def test_conv_statistics_epilogue(lib, cuda, case, algo, mode):
    """The statistics epilogue with y guarded and the partial rows guarded at exactly yolo_conv_stats_rows() rows; as in
    test_gpu_conv.py, the BatchNorm fed by the partial rows must equal the one that reduces the stored tensor itself."""
    N, Cin, H, W, Cout, k, stride = case
    rng = np.random.default_rng(7)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    st = _st()
    xd = moated(to_nhwc(x, 'bf16', cuda))
    wp = _packed(lib, cuda, w, L.BF16)
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    npix = N * Ho * Wo
    cp = lib.yolo_padded_channels(Cout)
    gamma = moated(torch.from_numpy(rng.uniform(.5, 1.5, Cout).astype(np.float32)).to(cuda))
    beta = moated(torch.from_numpy((0.2 * rng.standard_normal(Cout)).astype(np.float32)).to(cuda))
    g = Guards(cuda)
    d = L.ConvDesc()
    d.x, d.w_packed = xd.data_ptr(), wp.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, Cin, Cout, k, stride, L.BF16, 1.0, algo
    ws = [torch.zeros(2 * Cout, dtype=torch.float64, device=cuda) for _ in range(4)]
    mk = lambda: (torch.empty(Cout, device=cuda), torch.empty(Cout, device=cuda))
    if mode == 1:
        y = g.out('y', (N, Ho, Wo, Cout), torch.bfloat16)
        d.y, d.stats, d.stats_mode = y.data_ptr(), 1, 1
        rows = lib.yolo_conv_stats_rows(C.byref(d))
        assert rows > 0
        part = g.out('partial rows', (rows, 2, cp), torch.float32)
        d.stats = part.data_ptr()
        assert lib.yolo_conv_fwd(C.byref(d), st) == 0
        g.check()
        assert bool(torch.isfinite(y.float()).all())
        (m1, i1), (m2, i2) = mk(), mk()
        z1, z2 = torch.empty_like(y), torch.empty_like(y)
        rm, rv = torch.zeros(Cout, device=cuda), torch.ones(Cout, device=cuda)
        assert lib.yolo_bn_train_fwd_partials(part.data_ptr(), rows, cp, y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None,
                                              z1.data_ptr(), m1.data_ptr(), i1.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                              ws[0].data_ptr(), ws[1].data_ptr(), 2 * Cout, npix, Cout, 1e-5, 0.9, 0.1, L.BF16, st) == 0
        assert lib.yolo_bn_train_fwd_pp(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, z2.data_ptr(), m2.data_ptr(),
                                        i2.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[2].data_ptr(), ws[3].data_ptr(), 2 * Cout,
                                        npix, Cout, 1e-5, 0.9, 0.1, L.BF16, st) == 0
        g.check()
        np.testing.assert_allclose(m1.cpu().numpy(), m2.cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(i1.cpu().numpy(), i2.cpu().numpy(), rtol=1e-5)
        assert float((z1.float() - z2.float()).abs().max()) <= 1e-2 * float(z2.float().abs().max())
        # ... and the stored map is the convolution (the bf16 bar of test_conv_bf16)
        ref = ref_conv(x, w, np.ones(Cout, np.float32), np.zeros(Cout, np.float32), stride, 1.0, bf16=True)
        np.testing.assert_allclose(from_nhwc(y), ref, rtol=1.6e-2, atol=2e-2)
        return
    yb = moated(torch.from_numpy(rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)).to(cuda).bfloat16())
    acc0 = torch.from_numpy((0.5 * rng.standard_normal((N, Ho, Wo, Cout))).astype(np.float32)).to(cuda).bfloat16()
    mean = moated(yb.float().mean(dim=(0, 1, 2)).contiguous())
    invstd = moated((1.0 / torch.sqrt(yb.float().var(dim=(0, 1, 2), unbiased=False) + 1e-5)).contiguous())
    y = g.out('y', (N, Ho, Wo, Cout), torch.bfloat16, prior=acc0)
    d.y = d.residual = y.data_ptr()
    d.stats, d.stats_mode, d.stats_y = 1, 2, yb.data_ptr()
    d.stats_mean, d.stats_invstd, d.stats_gamma, d.stats_beta, d.stats_slope = (mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                                                               beta.data_ptr(), 0.1)
    rows = lib.yolo_conv_stats_rows(C.byref(d))
    assert rows > 0
    part = g.out('partial rows', (rows, 2, cp), torch.float32)
    d.stats = part.data_ptr()
    assert lib.yolo_conv_fwd(C.byref(d), st) == 0
    g.check()
    assert bool(torch.isfinite(y.float()).all())
    dy1, dy2 = torch.empty_like(y), torch.empty_like(y)
    (g1, b1), (g2, b2) = mk(), mk()
    assert lib.yolo_bn_train_bwd_partials(part.data_ptr(), rows, cp, y.data_ptr(), yb.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                          gamma.data_ptr(), beta.data_ptr(), dy1.data_ptr(), g1.data_ptr(), b1.data_ptr(),
                                          ws[0].data_ptr(), ws[1].data_ptr(), 2 * Cout, npix, Cout, 0.1, L.BF16, st) == 0
    assert lib.yolo_bn_train_bwd_pp(y.data_ptr(), yb.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                    beta.data_ptr(), dy2.data_ptr(), g2.data_ptr(), b2.data_ptr(), ws[2].data_ptr(),
                                    ws[3].data_ptr(), 2 * Cout, npix, Cout, 0.1, L.BF16, st) == 0
    g.check()
    sc = float(g2.abs().max()) + float(b2.abs().max())
    np.testing.assert_allclose(g1.cpu().numpy(), g2.cpu().numpy(), rtol=1e-4, atol=1e-5 * sc)
    np.testing.assert_allclose(b1.cpu().numpy(), b2.cpu().numpy(), rtol=1e-4, atol=1e-5 * sc)
    assert float((dy1.float() - dy2.float()).abs().max()) <= 1e-2 * float(dy2.float().abs().max())
    ref = ref_conv(x, w, np.ones(Cout, np.float32), np.zeros(Cout, np.float32), stride, 1.0, residual=from_nhwc(acc0), bf16=True)
    np.testing.assert_allclose(from_nhwc(y), ref, rtol=1.6e-2, atol=2e-2)


BOUNDS_TAIL_CASES = [(5, 128, 13, 13, 256, 1, False, 90, True, False), (1, 256, 9, 70, 224, 1, True, 96, False, False)]


@pytest.mark.parametrize('case,algo', [(c, a) for c in BOUNDS_TAIL_CASES for a in (0, 2, 6)])
def test_conv_tail_1x1_fused(lib, cuda, case, algo):
    """The fused 1x1 tail with y and tail_y (the fp32 logits with their padded pitch) guarded: bit-identical to the two separate
    launches and the tail against torch on the rounded operands, as test_conv_tail_1x1_fused_is_bit_identical holds it."""
    N, Cin, H, W, Cout, stride, with_res, tcout, tf32, strided = case
    assert stride == 1 and not strided
    rng = np.random.default_rng(31)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    w1 = (rng.standard_normal((tcout, Cout, 1, 1)) / np.sqrt(Cout)).astype(np.float32)
    st, dt = _st(), L.BF16
    xd = moated(to_nhwc(x, 'bf16', cuda))
    rd = moated(to_nhwc(rng.standard_normal((N, Cout, H, W)).astype(np.float32), 'bf16', cuda)) if with_res else None
    wp, wp1 = _packed(lib, cuda, w, dt), _packed(lib, cuda, w1, dt)
    g1, g2 = np.random.default_rng(1), np.random.default_rng(2)
    s_, b_ = g1.uniform(.5, 1.5, Cout).astype(np.float32), (0.1 * g1.standard_normal(Cout)).astype(np.float32)
    s1_, b1_ = g2.uniform(.5, 1.5, tcout).astype(np.float32), (0.1 * g2.standard_normal(tcout)).astype(np.float32)
    sc, bi, sc1, bi1 = (_padded(lib, cuda, v) for v in (s_, b_, s1_, b1_))
    tpitch = tcout + 6 if tf32 else tcout                     # (fp32 logits: rows of a wider merged buffer)
    ttdt = torch.float32 if tf32 else torch.bfloat16
    outs = []
    for fused in (False, True):
        g = Guards(cuda)
        y = g.out('y', (N, H, W, Cout), torch.bfloat16)
        z = g.out('tail_y', (N, H, W, tpitch), ttdt)
        d = L.ConvDesc()
        d.x, d.w_packed, d.scale, d.bias, d.y = xd.data_ptr(), wp.data_ptr(), sc.data_ptr(), bi.data_ptr(), y.data_ptr()
        d.residual = rd.data_ptr() if with_res else None
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, Cin, Cout, 3, 1, dt, 0.1, algo
        d.y_pixel_stride, d.y_batch_stride = Cout, H * W * Cout
        if fused:
            d.tail_w_packed, d.tail_scale, d.tail_bias, d.tail_y = wp1.data_ptr(), sc1.data_ptr(), bi1.data_ptr(), z.data_ptr()
            d.tail_cout, d.tail_out_f32, d.tail_slope = tcout, int(tf32), (1.0 if tf32 else 0.1)
            d.tail_y_pixel_stride, d.tail_y_batch_stride = tpitch, H * W * tpitch
            assert lib.yolo_conv_fwd(C.byref(d), st) == 0
        else:
            for cand in ([algo] if algo else [6, 2]):         # the same tile variant as the fused call
                d.algo = cand
                if lib.yolo_conv_fwd(C.byref(d), st) == 0:
                    break
            else:
                raise AssertionError('no 256-cout variant takes the plain convolution')
            d1 = L.ConvDesc()
            d1.x, d1.w_packed, d1.scale, d1.bias, d1.y = y.data_ptr(), wp1.data_ptr(), sc1.data_ptr(), bi1.data_ptr(), z.data_ptr()
            d1.N, d1.H, d1.W, d1.Cin, d1.Cout, d1.ksize, d1.stride, d1.dtype = N, H, W, Cout, tcout, 1, 1, dt
            d1.out_f32, d1.slope = int(tf32), (1.0 if tf32 else 0.1)
            d1.x_pixel_stride = Cout
            d1.y_pixel_stride, d1.y_batch_stride = tpitch, H * W * tpitch
            assert lib.yolo_conv_fwd(C.byref(d1), st) == 0
        g.check()
        assert bool(torch.isnan(z[..., tcout:].float()).all()), 'the pad columns of a tail row were written'
        outs.append((y, z[..., :tcout].contiguous()))
    (y0, z0), (y1, z1) = outs
    assert not torch.isnan(y1.float()).any() and not torch.isnan(z1.float()).any()
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    it = torch.int32 if tf32 else torch.int16
    assert torch.equal(z0.view(it), z1.view(it))
    yin = y1.float().permute(0, 3, 1, 2).cpu()
    ref = F.conv2d(yin, torch.from_numpy(w1).to(torch.bfloat16).float())
    ref = ref * torch.from_numpy(s1_).view(1, -1, 1, 1) + torch.from_numpy(b1_).view(1, -1, 1, 1)
    if not tf32:
        ref = torch.where(ref > 0, ref, ref * 0.1).to(torch.bfloat16).float()
    np.testing.assert_allclose(z1.float().permute(0, 3, 1, 2).cpu().numpy(), ref.numpy(), rtol=1.6e-2, atol=2e-2)


@pytest.mark.parametrize('case', [(1, 128, 10, 14, 64, 1), (3, 32, 6, 5, 64, 3)])
def test_conv_strided_input_and_upsampled_output(lib, cuda, case):
    """x_pixel_stride / upsample2x / y_pixel_stride with the WIDE buffers in a moat and between guards: against the dense path on
    the same operands (test_gpu_conv.py's test of the same name), every tile variant that takes the shape."""
    N, Cin, H, W, Cout, k = case
    rng = np.random.default_rng(31)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    sc, bi = rng.uniform(.5, 1.5, Cout).astype(np.float32), (.2 * rng.standard_normal(Cout)).astype(np.float32)
    dense = run_conv(lib, cuda, x, w, sc, bi, 1, 0.1, 'bf16')
    st, tdt, dt = _st(), torch.bfloat16, L.BF16
    XC, x0, YC, y0 = Cin + 56, 40, Cout + 24, 8
    xw = torch.full((N, H, W, XC), float('nan'), dtype=tdt, device=cuda)
    xw[..., x0:x0 + Cin] = to_nhwc(x, 'bf16', cuda)
    xbuf = moated(xw)
    wp = _packed(lib, cuda, w, dt)
    scd, bid = _padded(lib, cuda, sc), _padded(lib, cuda, bi)
    ran = 0
    for algo in (0, 1, 2, 4, 8, 11, 22):
        g = Guards(cuda)
        ybuf = g.out('upsampled y', (N, 2 * H, 2 * W, YC), tdt, prior=torch.full((N, 2 * H, 2 * W, YC), -7.0, dtype=tdt, device=cuda))
        d = L.ConvDesc()
        d.x, d.w_packed, d.scale, d.bias = xbuf[..., x0:].data_ptr(), wp.data_ptr(), scd.data_ptr(), bid.data_ptr()
        d.y = ybuf[..., y0:].data_ptr()
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, Cin, Cout, k, 1, dt, 0.1, algo
        d.x_pixel_stride, d.upsample2x, d.y_pixel_stride, d.y_batch_stride = XC, 1, YC, 4 * H * W * YC
        rc = lib.yolo_conv_fwd(C.byref(d), st)
        g.check()
        if algo and rc == L.EUNSUPPORTED:
            continue
        assert rc == 0, (algo, rc)
        ran += 1
        got = ybuf.float().cpu().numpy()
        assert (got[..., :y0] == -7.0).all() and (got[..., y0 + Cout:] == -7.0).all(), algo
        up = np.repeat(np.repeat(dense, 2, axis=2), 2, axis=3)
        np.testing.assert_array_equal(got[..., y0:y0 + Cout].transpose(0, 3, 1, 2), up, err_msg='algo %d' % algo)
    assert ran >= 2
    # strided output with a dense residual
    res = rng.standard_normal((N, Cout, H, W)).astype(np.float32)
    ref = run_conv(lib, cuda, x, w, sc, bi, 1, 0.1, 'bf16', residual=res)
    rd = moated(to_nhwc(res, 'bf16', cuda))
    g = Guards(cuda)
    ybuf = g.out('strided y', (N, H, W, YC), tdt, prior=torch.full((N, H, W, YC), -7.0, dtype=tdt, device=cuda))
    d = L.ConvDesc()
    d.x, d.w_packed, d.scale, d.bias = xbuf[..., x0:].data_ptr(), wp.data_ptr(), scd.data_ptr(), bid.data_ptr()
    d.residual, d.y = rd.data_ptr(), ybuf[..., y0:].data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, Cin, Cout, k, 1, dt, 0.1, 0
    d.x_pixel_stride, d.y_pixel_stride, d.y_batch_stride = XC, YC, H * W * YC
    assert lib.yolo_conv_fwd(C.byref(d), st) == 0
    g.check()
    got = ybuf.float().cpu().numpy()
    assert (got[..., :y0] == -7.0).all() and (got[..., y0 + Cout:] == -7.0).all()
    np.testing.assert_array_equal(got[..., y0:y0 + Cout].transpose(0, 3, 1, 2), ref)


# ---- gradients: sub-pixel data gradient, weight gradients ------------------------------------------------------------------------
def _conv_grads(case, seed, round_to=None):
    """x, w, dy (numpy, NCHW) of conv case (N, Cin, H, W, Cout, k, stride) and the autograd dx, dw on the operands rounded to
    `round_to` (the gradient of the unrounded x / w: what the kernels accumulate in fp32)."""
    N, Cin, H, W, Cout, k, s = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    r = (lambda a: torch.from_numpy(a).to(round_to).float()) if round_to is not None else torch.from_numpy
    xt, wt = r(x).requires_grad_(True), r(w).requires_grad_(True)
    y = F.conv2d(xt, wt, None, stride=s, padding=k // 2)
    dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(r(dy))
    return x, w, dy, xt.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize('case', [(2, 8, 12, 20, 32), (2, 64, 2, 2, 32), (1, 40, 6, 10, 96)])
def test_dgrad_s2(lib, cuda, case):
    """yolo_conv_dgrad_s2, every variant that takes the shape, fresh and accumulating in place, dx between guards: against autograd
    on the bf16-rounded operands (test_dgrad_s2_subpixel's bars)."""
    N, Cin, H, W, Cout = case
    x, w, dy, ref, _ = _conv_grads((N, Cin, H, W, Cout, 3, 2), 5, torch.bfloat16)
    st = _st()
    wbuf, wd = guarded((lib.yolo_packed_weight_bytes(4 * Cin, Cout, 2, L.BF16),), torch.uint8, cuda)
    assert lib.yolo_pack_conv_weights_dgrad_s2(moated(torch.from_numpy(w).to(cuda)).data_ptr(), wd.data_ptr(), Cout, Cin, L.BF16, st) == 0
    dyd = moated(to_nhwc(dy, 'bf16', cuda))
    ones = _padded(lib, cuda, np.ones(4 * Cin, np.float32))
    zeros = _padded(lib, cuda, np.zeros(4 * Cin, np.float32))
    ran = 0
    for algo in (0, 2, 6, 10, 4):
        g = Guards(cuda)
        g.pairs.append(('packed image', wbuf, wd))
        out = g.out('dx', (N, H, W, Cin), torch.bfloat16)
        d = L.ConvDesc()
        d.x, d.w_packed, d.scale, d.bias, d.y = dyd.data_ptr(), wd.data_ptr(), ones.data_ptr(), zeros.data_ptr(), out.data_ptr()
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope = N, H // 2, W // 2, Cout, 4 * Cin, 2, 1, L.BF16, 1.0
        d.algo = algo
        rc = lib.yolo_conv_dgrad_s2(C.byref(d), st)
        g.check()
        if algo and rc == L.EUNSUPPORTED:
            assert bool(torch.isnan(out.float()).all())
            continue
        assert rc == 0, (algo, rc)
        ran += 1
        got = from_nhwc(out)
        assert np.isfinite(got).all(), algo
        np.testing.assert_allclose(got, ref, rtol=1e-2, atol=1e-2 * np.abs(ref).max(), err_msg='algo %d' % algo)
        d.residual = out.data_ptr()
        assert lib.yolo_conv_dgrad_s2(C.byref(d), st) == 0
        g.check()
        np.testing.assert_allclose(from_nhwc(out), 2 * ref, rtol=2e-2, atol=2e-2 * np.abs(ref).max(), err_msg='acc algo %d' % algo)
    assert ran >= 2


def _wgrad_case(lib, cuda, case, dtype, algo):
    """One weight-gradient call with dw (pre-filled with ones: the entry accumulates) and the workspace (exactly
    yolo_conv_wgrad_workspace_bytes(), zero on entry) between guards; -> rc, dw - 1, the workspace."""
    N, Cin, H, W, Cout, k, s = case
    x, w, dy, _, ref = _conv_grads(case, 3, torch.bfloat16 if dtype == 'bf16' else None)
    xd, dyd = moated(to_nhwc(x, dtype, cuda)), moated(to_nhwc(dy, dtype, cuda))
    g = Guards(cuda)
    dw = g.out('dw', (Cout, Cin, k, k), torch.float32, prior=torch.ones((Cout, Cin, k, k), device=cuda))
    nws = lib.yolo_conv_wgrad_workspace_bytes(Cin, Cout, k, LDT[dtype])
    assert nws >= 0
    ws = g.out('workspace', (nws,), torch.uint8, prior=torch.zeros(nws, dtype=torch.uint8, device=cuda))
    if algo is None:
        rc = lib.yolo_conv_wgrad(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, k, s, 0, LDT[dtype], _ptr(ws), _st())
    else:
        rc = lib.yolo_conv_wgrad_algo(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, k, s, 0, LDT[dtype], _ptr(ws), algo, _st())
    g.check()
    assert bool((ws == 0).all()), 'the workspace is left zeroed'
    return rc, dw.cpu().numpy() - 1.0, ref


WGRAD_GENERIC = [(1, 8, 20, 20, 16, 3, 1), (2, 96, 2, 3, 128, 3, 1), (1, 24, 41, 71, 40, 3, 2), (2, 64, 4, 6, 96, 1, 1)]


@pytest.mark.parametrize('dtype,algo', [('bf16', 0), ('bf16', 1), ('f32', None)])
@pytest.mark.parametrize('case', WGRAD_GENERIC)
def test_wgrad(lib, cuda, case, dtype, algo):
    """yolo_conv_wgrad_algo 0 / 1 in bf16 (test_wgrad_bf16_transposing_reads' bar) and yolo_conv_wgrad in f32 (test_wgrad's)."""
    rc, got, ref = _wgrad_case(lib, cuda, case, dtype, algo)
    assert rc == 0
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=(2e-3 if dtype == 'bf16' else 1e-3) * np.abs(ref).max())


@pytest.mark.parametrize('algo', [2, 3, 4])
@pytest.mark.parametrize('case', [(1, 64, 5, 4, 64), (1, 64, 2, 70, 64), (2, 64, 17, 19, 192)])
def test_wgrad_row_walk(lib, cuda, case, algo):
    N, Cin, H, W, Cout = case
    rc, got, ref = _wgrad_case(lib, cuda, (N, Cin, H, W, Cout, 3, 1), 'bf16', algo)
    assert rc == 0
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=2e-3 * np.abs(ref).max())


@pytest.mark.parametrize('algo', [5, 6])
@pytest.mark.parametrize('case', [(1, 128, 5, 13, 256), (4, 384, 9, 7, 256)])
def test_wgrad_1x1_gemm(lib, cuda, case, algo):
    N, Cin, H, W, Cout = case
    rc, got, ref = _wgrad_case(lib, cuda, (N, Cin, H, W, Cout, 1, 1), 'bf16', algo)
    assert rc == 0
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=2e-3 * np.abs(ref).max())


def _to_split(v, cuda):
    """(..., C) fp32 -> split storage (..., 2, round_up(C, 32)) bf16 on the device, zero pad channels."""
    v = torch.as_tensor(v, dtype=torch.float32)
    Cc = v.shape[-1]
    hi, lo = split_planes(v)
    out = torch.zeros(tuple(v.shape[:-1]) + (2, -(-Cc // 32) * 32), dtype=torch.bfloat16)
    out[..., 0, :Cc], out[..., 1, :Cc] = hi, lo
    return out.to(cuda)


# the two smallest WG_CASES of test_gpu_split_train.py with a channel count that is not a multiple of 32
@pytest.mark.parametrize('algo', [0, 1, 2])
@pytest.mark.parametrize('case', [(4, 96, 20, 24, 40, 3, 1), (2, 128, 26, 26, 90, 1, 1)])
def test_wgrad_split(lib, cuda, case, algo):
    """yolo_conv_wgrad_split against the float64 weight gradient of the split operands' values (test_split_wgrad's bar)."""
    N, Cin, H, W, Cout, k, s = case
    rng = np.random.default_rng(Cin * 7 + Cout)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    dy = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)
    xs, dys = _to_split(x, cuda), _to_split(dy, cuda)
    val = lambda t, c: (t.float()[..., 0, :c] + t.float()[..., 1, :c]).cpu().double().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(val(xs, Cin), (Cout, Cin, k, k), val(dys, Cout), stride=s, padding=k // 2)
    xd, dyd = moated(xs), moated(dys)
    g = Guards(cuda)
    dw = g.out('dw', (Cout, Cin, k, k), torch.float32, prior=torch.full((Cout, Cin, k, k), 0.5, device=cuda))
    nws = lib.yolo_conv_wgrad_split_workspace_bytes(Cin, Cout, k, L.BF16X3)
    ws = g.out('workspace', (nws,), torch.uint8, prior=torch.zeros(nws, dtype=torch.uint8, device=cuda))
    L.check(lib.yolo_conv_wgrad_split(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, k, s, 0, 0, L.BF16X3, _ptr(ws),
                                      algo, _st()), 'wgrad split')
    g.check()
    got = dw.cpu().double() - 0.5
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err < 2e-4, (algo, err)
    assert bool((ws == 0).all()), 'the workspace is left zeroed'


# ---- train-mode BatchNorm: the three-launch calls, the _pp pair, the _partials pair ----------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('variant', ['plain', 'pp', 'partials'])
@pytest.mark.parametrize('shape', [(1, 1, 1, 8), (1, 4, 6, 32), (2, 5, 7, 2112)])
def test_bn_train(lib, cuda, shape, variant, dtype):
    """yolo_bn_train_fwd / _bwd, the _pp pair and the _partials pair (bf16; refused in f32) with every output, both workspaces and
    zero_next (exactly zero_next_count doubles) between guards, against torch autograd on the stored operands (the bars of
    test_bn_train_fwd_bwd in f32, of test_bn_train_bf16 in bf16)."""
    N, H, W, Cc = shape
    npix = N * H * W
    rng = np.random.default_rng(3)
    tdt, ldt = TDT[dtype], LDT[dtype]
    rt = lambda a: torch.from_numpy(a.astype(np.float32)).to(tdt).float()
    y = rt(2 * rng.standard_normal((npix, Cc)) + 0.5).requires_grad_(True)
    gamma = torch.from_numpy(rng.uniform(.5, 1.5, Cc).astype(np.float32)).requires_grad_(True)
    beta = torch.from_numpy((.1 * rng.standard_normal(Cc)).astype(np.float32)).requires_grad_(True)
    res = rt(rng.standard_normal((npix, Cc)))
    dz = rt(rng.standard_normal((npix, Cc)))
    mean, var = y.mean(dim=0), y.var(dim=0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    a = (y - mean) * invstd * gamma + beta
    z = F.leaky_relu(a, 0.1) + res
    z.backward(dz)
    yd, resd, dzd = (moated(t.detach().to(cuda).to(tdt)) for t in (y, res, dz))
    g_, b_ = moated(gamma.detach().to(cuda)), moated(beta.detach().to(cuda))
    g = Guards(cuda)
    zd, dyd = g.out('z', (npix, Cc), tdt), g.out('dy', (npix, Cc), tdt)
    m_, is_, dg, db = (g.out(n, (Cc,), torch.float32) for n in ('mean', 'invstd', 'dgamma', 'dbeta'))
    rm = g.out('running_mean', (Cc,), torch.float32, prior=torch.zeros(Cc, device=cuda))
    rv = g.out('running_var', (Cc,), torch.float32, prior=torch.ones(Cc, device=cuda))
    zn = 2 * Cc                                                    # zero_next_count
    wa = g.out('workspace', (zn,), torch.float64, prior=torch.zeros(zn, dtype=torch.float64, device=cuda))
    wb = g.out('zero_next', (zn,), torch.float64, prior=torch.full((zn,), 123.0, dtype=torch.float64, device=cuda))
    p = lambda *ts: tuple(t.data_ptr() for t in ts)
    st = _st()
    if variant == 'plain':
        assert lib.yolo_bn_train_fwd(*p(yd, g_, b_, resd, zd, m_, is_, rm, rv, wa), npix, Cc, 1e-5, 0.9, 0.1, ldt, st) == 0
        assert lib.yolo_bn_train_bwd(*p(dzd, yd, m_, is_, g_, b_, dyd, dg, db, wa), npix, Cc, 0.1, ldt, st) == 0
        g.check()
        assert float(wa.abs().max()) == 0.0 and bool((wb == 123.0).all())          # left zeroed; the other buffer is not its business
    elif variant == 'pp':
        assert lib.yolo_bn_train_fwd_pp(*p(yd, g_, b_, resd, zd, m_, is_, rm, rv, wa, wb), zn, npix, Cc, 1e-5, 0.9, 0.1, ldt, st) == 0
        g.check()
        assert float(wb.abs().max()) == 0.0
        assert lib.yolo_bn_train_bwd_pp(*p(dzd, yd, m_, is_, g_, b_, dyd, dg, db, wb, wa), zn, npix, Cc, 0.1, ldt, st) == 0
        g.check()
        assert float(wa.abs().max()) == 0.0
    else:
        # the partial rows a convolution's statistics epilogue would have written, three of them over ragged pixel ranges:
        # forward sum(y), sum(y^2) of the stored map; backward sum(da), sum(da xhat), da = dz lrelu'(a)
        cp = lib.yolo_padded_channels(Cc)
        cuts = [0, npix // 3, npix // 2, npix]

        def partial_rows(u, v):
            t = torch.zeros((3, 2, cp), dtype=torch.float64)
            for i in range(3):
                t[i, 0, :Cc], t[i, 1, :Cc] = u[cuts[i]:cuts[i + 1]].sum(dim=0), v[cuts[i]:cuts[i + 1]].sum(dim=0)
            return moated(t.float().to(cuda))
        yv = y.detach().double()
        pf = partial_rows(yv, yv * yv)
        rc = lib.yolo_bn_train_fwd_partials(pf.data_ptr(), 3, cp, *p(yd, g_, b_, resd, zd, m_, is_, rm, rv, wa, wb), zn, npix, Cc, 1e-5,
                                            0.9, 0.1, ldt, st)
        g.check()
        if dtype == 'f32':
            assert rc == L.EUNSUPPORTED
            assert bool(torch.isnan(zd).all()) and bool((wb == 123.0).all())
            return
        assert rc == 0
        assert float(wb.abs().max()) == 0.0
        da = dz.double() * torch.where(a.detach() > 0, 1.0, 0.1).double()
        xhat = ((y - mean) * invstd).detach().double()
        pb = partial_rows(da, da * xhat)
        assert lib.yolo_bn_train_bwd_partials(pb.data_ptr(), 3, cp, *p(dzd, yd, m_, is_, g_, b_, dyd, dg, db, wb, wa), zn, npix, Cc, 0.1,
                                              ldt, st) == 0
        g.check()
        assert float(wa.abs().max()) == 0.0
    f = lambda t: t.float().cpu().numpy()
    zr, dyr = z.detach().numpy(), y.grad.numpy()
    for name, t in (('z', zd), ('dy', dyd), ('mean', m_), ('invstd', is_), ('dgamma', dg), ('dbeta', db), ('running_mean', rm), ('running_var', rv)):
        assert bool(torch.isfinite(t.float()).all()), name
    np.testing.assert_allclose(f(m_), mean.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(f(rv), 0.9 + 0.1 * var.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(f(rm), 0.1 * mean.detach().numpy(), rtol=1e-5, atol=1e-6)
    # dy is a difference of terms of size |gamma invstd dz|: with ONE pixel it is zero and only that size gives a scale
    scale = np.abs(dyr).max() if npix > 1 else float((gamma * invstd).abs().max() * dz.abs().max())
    if dtype == 'f32':
        np.testing.assert_allclose(f(zd), zr, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(f(dyd), dyr, rtol=1e-3, atol=1e-4 * scale)
    else:
        np.testing.assert_allclose(f(zd), zr, rtol=1e-2, atol=1e-2)
        np.testing.assert_allclose(f(dyd), dyr, rtol=1e-2, atol=1e-2 * scale)
    np.testing.assert_allclose(f(dg), gamma.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(f(db), beta.grad.numpy(), rtol=1e-4, atol=1e-4)


# ---- the weight packers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16', 'bf16x3', 'f16x3'])
@pytest.mark.parametrize('conv', [(30, 64, 1), (16, 8, 3), (90, 128, 1), (64, 32, 3), (72, 40, 3)], ids=lambda c: 'x'.join(map(str, c)))
def test_packers(lib, cuda, conv, dtype):
    """yolo_pack_conv_weights, _dgrad and _dgrad_s2 into an image of exactly yolo_packed_weight_bytes(), for every element type
    the call accepts.  An image is a rearrangement of the rounded weights (a split type's: hi parts twice, lo parts once) among
    zero padding: its non-zero values, sorted, are exactly theirs, and no byte of it is left unwritten."""
    Cout, Cin, k = conv
    ldt, tdt = LDT[dtype], TDT[dtype]
    w = torch.from_numpy(np.random.default_rng(Cout + Cin).standard_normal((Cout, Cin, k, k)).astype(np.float32))
    wd = moated(w.to(cuda))
    if dtype in ('bf16x3', 'f16x3'):                                # three K passes [w_hi | w_hi | w_lo] (include/yolo_amd.h)
        hi, lo = split_planes(w, tdt)
        want = torch.cat([t.float().flatten() for t in (hi, hi, lo)])
    else:
        want = w.to(tdt).float().flatten()
    want = np.sort(want[want != 0].numpy())
    st = _st()
    calls = [('fwd', (Cout, Cin, k), lambda p: lib.yolo_pack_conv_weights(wd.data_ptr(), p, Cout, Cin, k, ldt, st)),
             ('dgrad', (Cin, Cout, k), lambda p: lib.yolo_pack_conv_weights_dgrad(wd.data_ptr(), p, Cout, Cin, k, ldt, st))]
    if k == 3:
        calls.append(('dgrad_s2', (4 * Cin, Cout, 2), lambda p: lib.yolo_pack_conv_weights_dgrad_s2(wd.data_ptr(), p, Cout, Cin, ldt, st)))
    accepted = 0
    for name, dims, call in calls:
        nbytes = lib.yolo_packed_weight_bytes(*dims, ldt)
        if nbytes <= 0:
            assert call(wd.data_ptr()) != 0, name                  # no image of that kind in this type: the packer refuses, too
            continue
        buf, img = guarded((nbytes,), torch.uint8, cuda)
        rc = call(img.data_ptr())
        torch.cuda.synchronize()
        guards_intact(buf, img)
        if rc == L.EUNSUPPORTED:
            assert bool((img == 0xFF).all()), name + ': refused, yet wrote'
            continue
        assert rc == 0, (name, rc)
        accepted += 1
        vals = img.view(tdt).float().cpu()
        assert bool(torch.isfinite(vals).all()), name + ': bytes of the image were left unwritten'
        got = np.sort(vals[vals != 0].numpy())
        np.testing.assert_array_equal(got, want, err_msg=name)
    assert accepted >= 1 or dtype in ('bf16x3', 'f16x3')


# ---- decode + NMS as one call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [{}, dict(topk=50, post_nms=20)], ids=['defaults', 'topk50_post20'])
@pytest.mark.parametrize('B', [3, 1])
def test_decode_nms(lib, cuda, B, kw):
    """yolo_decode_nms at (160, 224) with rows, scores, kept ids / scores / counts and the selection workspace (exactly
    yolo_nms_select_workspace_bytes(B): the size the header requires of this call) between guards, bitwise against
    Detector.decode_nms."""
    from oracle import graph as og, detect as od
    from yolo_amd.detect import Detector
    spec, size = og.spec_d53(), (160, 224)
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    area = od.init_area(size, steps)
    rng = np.random.default_rng(11)
    Cc = spec['slice_point'][-1]
    outs = [torch.from_numpy((2.0 * rng.standard_normal((B, a, 3, Cc))).astype(np.float32)).to(cuda) for a in area]
    det = Detector(spec, size, steps, device=cuda)
    ref = det.decode_nms(outs, 'class', **kw)
    topk, post = kw.get('topk', 400), kw.get('post_nms', 100)
    m = moated(torch.cat(outs, dim=1).contiguous())
    g = Guards(cuda)
    rows = g.out('rows', (B, det.nbox, Cc), torch.float32)
    scores = g.out('scores', (B, det.nbox * (Cc - 6)), torch.float32)
    kept = g.out('kept', (B, post), torch.int32)
    ks = g.out('kept scores', (B, post), torch.float32)
    cnt = g.out('kept count', (B,), torch.int32)
    nws = lib.yolo_nms_select_workspace_bytes(B)
    assert 0 < nws <= lib.yolo_nms_workspace_bytes(B, det.nbox, Cc - 6, 1, topk)
    ws = g.out('select workspace', (nws,), torch.uint8)
    L.check(lib.yolo_decode_nms(m.data_ptr(), rows.data_ptr(), scores.data_ptr(), B, Cc, C.byref(det.grid), 1, 0.01, 0.45, topk, post,
                                kept.data_ptr(), ks.data_ptr(), cnt.data_ptr(), ws.data_ptr(), _st()), 'decode_nms')
    g.check()
    assert int(cnt.min()) > 0
    for name, a, b in zip(('rows', 'scores', 'kept', 'kept scores', 'kept count'), (rows, scores, kept, ks, cnt), ref):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
