"""The small kernels of the training step (csrc/train_ops.hip, csrc/elementwise.hip) straight through the C ABI in the single-plane
element types the training step runs them in: layout conversion, up-sample + concat and its backward, 2x dilation, the gradient
fan-in add, the strided row gather, the bias gradient and BatchNorm folding.  They move data or round once, so the references are
exact and the comparison is on BITS unless stated.  Every output is allocated at exactly its size between two 64-element margins,
pre-filled with NaN together with them: "every element written, nothing else touched" is part of each assertion."""
import numpy as np
import pytest
import torch

from yolo_amd import lib as L
from util import TDT, LDT

pytestmark = pytest.mark.gpu

GUARD = 64
PIXELS = [(1, 1, 1), (2, 5, 27), (3, 16, 16)]              # 1 and 270 pixels are no multiple of the 256-thread block, 768 is
IBITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
# round up into the next binade, bf16 ties (to even: down, then up), +-0, an fp32 subnormal, values that land on a bf16 / f16 subnormal
SPECIALS = [1.9999, -3.99999, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.0, -0.0, 1e-40, -3e-6, 2.0 ** -130, 0.1]


def st():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, tdt, dev, prior=None):
    """-> (whole buffer, view of `shape` in its middle); everything NaN, or `prior` (a CPU tensor) inside."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=tdt, device=dev)
    view = buf[GUARD:GUARD + n].view(shape)
    if prior is not None:
        view.copy_(prior.to(tdt))
    return buf, view


def margins_intact(buf):
    torch.cuda.synchronize()
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def untouched(buf):
    torch.cuda.synchronize()
    return bool(torch.isnan(buf).all())


def bits(t):
    return t.contiguous().view(IBITS[t.dtype]).cpu().numpy()


def same_bits(got, want):
    """got: device tensor; want: CPU tensor of the same dtype and shape."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    g, w = bits(got), bits(want)
    assert np.array_equal(g, w), '%d of %d elements differ, first at %s' % ((g != w).sum(), g.size, np.argwhere(g != w)[:1])


def randn(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    k = min(len(SPECIALS), flat.size)
    flat[:k] = np.asarray(SPECIALS, np.float32)[(np.arange(k) + int(np.prod(shape))) % len(SPECIALS)]
    return torch.from_numpy(x)


# ---- layout conversion --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', PIXELS)
@pytest.mark.parametrize('Cc', [1, 3, 8])
def test_nchw_to_nhwc(lib, cuda, Cc, shape, dtype):
    N, H, W = shape
    x = randn(np.random.default_rng(Cc + N), (N, Cc, H, W))
    want = torch.zeros((N, H, W, 8), dtype=TDT[dtype])
    want[..., :Cc] = x.permute(0, 2, 3, 1).to(TDT[dtype])                    # torch: round-to-nearest-even; channels C..7 exactly zero
    buf, y = guarded((N, H, W, 8), TDT[dtype], cuda)
    xd = x.to(cuda)
    assert lib.yolo_nchw_to_nhwc(xd.data_ptr(), y.data_ptr(), N, Cc, H, W, 8, LDT[dtype], st()) == 0
    assert margins_intact(buf)
    same_bits(y, want)


def test_nchw_to_nhwc_refusals(lib, cuda):
    x = torch.zeros((1, 9, 4, 4), device=cuda)
    buf, y = guarded((1, 4, 4, 16), torch.float32, cuda)
    assert lib.yolo_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), 1, 8, 4, 4, 16, L.F32, st()) == L.EUNSUPPORTED
    assert lib.yolo_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), 1, 9, 4, 4, 8, L.F32, st()) == L.EUNSUPPORTED
    assert lib.yolo_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), 1, 3, 4, 4, 8, 7, st()) == L.EINVAL            # no such dtype
    assert untouched(buf)


@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('shape', PIXELS)
@pytest.mark.parametrize('Cc', [1, 5, 64])
def test_nhwc_to_nchw(lib, cuda, Cc, shape, dtype):
    N, H, W = shape
    x = randn(np.random.default_rng(Cc + H), (N, H, W, Cc)).to(TDT[dtype])
    buf, y = guarded((N, Cc, H, W), torch.float32, cuda)
    xd = x.to(cuda)
    assert lib.yolo_nhwc_to_nchw(xd.data_ptr(), y.data_ptr(), N, Cc, H, W, LDT[dtype], st()) == 0
    assert margins_intact(buf)
    same_bits(y, x.float().permute(0, 3, 1, 2).contiguous())                  # exact widening of the stored values


def test_nhwc_to_nchw_refuses_split_types(lib, cuda):
    x = torch.zeros((1, 4, 4, 2, 32), dtype=torch.bfloat16, device=cuda)
    buf, y = guarded((1, 5, 4, 4), torch.float32, cuda)
    for dt in (L.BF16X3, L.F16X3):
        assert lib.yolo_nhwc_to_nchw(x.data_ptr(), y.data_ptr(), 1, 5, 4, 4, dt, st()) == L.EINVAL
    assert untouched(buf)


# ---- up-sample + concat and its backward ----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 2, 2), (3, 6, 10)])
@pytest.mark.parametrize('dtype,C1,C2', [('f32', 4, 12), ('f32', 12, 4), ('bf16', 8, 24), ('bf16', 40, 8), ('f16', 8, 24), ('f16', 40, 8)])
def test_upsample2x_concat(lib, cuda, dtype, C1, C2, shape):
    N, H, W = shape                                                           # of the OUTPUT; the up-sampled input is (N, H/2, W/2, C1)
    rng = np.random.default_rng(C1 + H)
    up = randn(rng, (N, H // 2, W // 2, C1)).to(TDT[dtype])
    route = randn(rng, (N, H, W, C2)).to(TDT[dtype])
    ib = IBITS[TDT[dtype]]
    u = np.repeat(np.repeat(up.view(ib).numpy(), 2, axis=2), 2, axis=1)
    want = torch.from_numpy(np.concatenate([u, route.view(ib).numpy()], axis=-1)).view(TDT[dtype])
    buf, y = guarded((N, H, W, C1 + C2), TDT[dtype], cuda)
    upd, routed = up.to(cuda), route.to(cuda)
    assert lib.yolo_upsample2x_concat(upd.data_ptr(), routed.data_ptr(), y.data_ptr(), N, H, W, C1, C2, LDT[dtype], st()) == 0
    assert margins_intact(buf)
    same_bits(y, want)


def test_upsample2x_concat_refusals(lib, cuda):
    src = torch.zeros(4096, dtype=torch.bfloat16, device=cuda)
    buf, y = guarded((1, 4, 4, 32), torch.bfloat16, cuda)
    p = src.data_ptr()
    assert lib.yolo_upsample2x_concat(p, p, y.data_ptr(), 1, 3, 4, 8, 24, L.BF16, st()) == L.EINVAL          # odd H
    assert lib.yolo_upsample2x_concat(p, p, y.data_ptr(), 1, 4, 3, 8, 24, L.BF16, st()) == L.EINVAL          # odd W
    assert lib.yolo_upsample2x_concat(p, p, y.data_ptr(), 1, 4, 4, 4, 24, L.BF16, st()) == L.EUNSUPPORTED    # C1 = 4: half a 16-byte unit
    assert lib.yolo_upsample2x_concat(p, p, y.data_ptr(), 1, 4, 4, 4, 24, L.F16, st()) == L.EUNSUPPORTED
    assert untouched(buf)


@pytest.mark.parametrize('acc_up,acc_route', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('C1,C2', [(3, 5), (8, 12)])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_upsample2x_concat_bwd(lib, cuda, dtype, C1, C2, acc_up, acc_route):
    """numpy fp32 in the kernel's own order: ((d00 + d01) + d10) + d11, then old + s when accumulating, then ONE round-to-nearest-even
    cast to the element type."""
    N, H, W = 2, 6, 10
    tdt = TDT[dtype]
    rng = np.random.default_rng(C1 + 2 * acc_up + acc_route)
    dcat = randn(rng, (N, H, W, C1 + C2)).to(tdt)
    up0 = randn(rng, (N, H // 2, W // 2, C1)).to(tdt)                         # prior contents: used or overwritten, never NaN-filled
    route0 = randn(rng, (N, H, W, C2)).to(tdt)
    d = dcat.float().numpy()
    s = ((d[:, 0::2, 0::2, :C1] + d[:, 0::2, 1::2, :C1]) + d[:, 1::2, 0::2, :C1]) + d[:, 1::2, 1::2, :C1]
    assert s.dtype == np.float32
    r = d[..., C1:]
    if acc_up:
        s = up0.float().numpy() + s
    if acc_route:
        r = route0.float().numpy() + r
    bu, dup = guarded(up0.shape, tdt, cuda, up0)
    br, droute = guarded(route0.shape, tdt, cuda, route0)
    dcatd = dcat.to(cuda)
    assert lib.yolo_upsample2x_concat_bwd(dcatd.data_ptr(), dup.data_ptr(), droute.data_ptr(), N, H, W, C1, C2, acc_up, acc_route,
                                          LDT[dtype], st()) == 0
    assert margins_intact(bu) and margins_intact(br)
    same_bits(dup, torch.from_numpy(np.ascontiguousarray(s)).to(tdt))
    same_bits(droute, torch.from_numpy(np.ascontiguousarray(r)).to(tdt))


# ---- 2x dilation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(8, 12, 4, 6), (7, 11, 4, 6), (2, 2, 1, 1)])   # the middle one: H = 2 Ho - 1, the odd map of the 608 family
@pytest.mark.parametrize('Cc', [8, 40])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_dilate2x(lib, cuda, dtype, Cc, hw):
    H, W, Ho, Wo = hw
    N, tdt = 2, TDT[dtype]
    dy = randn(np.random.default_rng(H + Cc), (N, Ho, Wo, Cc)).to(tdt)
    want = torch.zeros((N, H, W, Cc), dtype=tdt)
    want[:, ::2, ::2] = dy
    buf, d = guarded((N, H, W, Cc), tdt, cuda)                                # NaN: the zeros are written, not assumed
    dyd = dy.to(cuda)
    assert lib.yolo_dilate2x(dyd.data_ptr(), d.data_ptr(), N, H, W, Ho, Wo, Cc, LDT[dtype], st()) == 0
    assert margins_intact(buf)
    same_bits(d, want)


# ---- gradient fan-in add ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 255, 4099])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_add(lib, cuda, dtype, n):
    tdt = TDT[dtype]
    rng = np.random.default_rng(n)
    a, b = randn(rng, (n,)).to(tdt), (randn(rng, (n,)) * 1.7).to(tdt)
    want = (a.float() + b.float()).to(tdt)
    ad, bd = a.to(cuda), b.to(cuda)
    buf, y = guarded((n,), tdt, cuda)
    assert lib.yolo_add(ad.data_ptr(), bd.data_ptr(), y.data_ptr(), n, LDT[dtype], st()) == 0
    assert margins_intact(buf)
    same_bits(y, want)
    buf, y = guarded((n,), tdt, cuda, a)                                      # in place, y == a, as Trainer._add calls it
    assert lib.yolo_add(y.data_ptr(), bd.data_ptr(), y.data_ptr(), n, LDT[dtype], st()) == 0
    assert margins_intact(buf)
    same_bits(y, want)


# ---- strided row gather -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cc,Cpad', [(21, 24), (90, 96), (16, 16)])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_gather_rows(lib, cuda, dtype, Cc, Cpad):
    """The shape of the Trainer's slice of dlogits: rows of C floats inside wider rows, the batches further apart than their rows."""
    Bn, rows, tdt = 3, 7, TDT[dtype]
    rs = 2 * Cc + 5
    bs = (rows + 3) * rs
    src = randn(np.random.default_rng(Cc), (Bn * bs,))
    want = torch.zeros((Bn, rows, Cpad), dtype=tdt)
    want[..., :Cc] = src.view(Bn, rows + 3, rs)[:, :rows, :Cc].to(tdt)
    buf, dst = guarded((Bn * rows, Cpad), tdt, cuda)
    srcd = src.to(cuda)
    assert lib.yolo_gather_rows(srcd.data_ptr(), dst.data_ptr(), Bn, rows, Cc, Cpad, bs, rs, LDT[dtype], st()) == 0
    assert margins_intact(buf)
    same_bits(dst, want.view(Bn * rows, Cpad))


# ---- the entries above that take f32 and bf16 only ---------------------------------------------------------------------------
def test_f16_is_refused_with_nothing_launched(lib, cuda):
    src = torch.ones(4096, dtype=torch.float32, device=cuda)
    p = src.data_ptr()
    buf, y = guarded((2048,), torch.float32, cuda)
    buf2, y2 = guarded((2048,), torch.float32, cuda)
    o, o2 = y.data_ptr(), y2.data_ptr()
    for dt in (L.F16, L.BF16X3, L.F16X3):
        assert lib.yolo_add(p, p, o, 64, dt, st()) < 0
    assert lib.yolo_bias_grad(p, o, 16, 8, 0, L.F16, st()) < 0
    assert lib.yolo_gather_rows(p, o, 2, 4, 8, 8, 64, 16, L.F16, st()) < 0
    assert lib.yolo_dilate2x(p, o, 1, 4, 4, 2, 2, 8, L.F16, st()) < 0
    assert lib.yolo_upsample2x_concat_bwd(p, o, o2, 1, 4, 4, 8, 8, 0, 0, L.F16, st()) < 0
    assert untouched(buf) and untouched(buf2)


# ---- bias gradient (the one helper with atomics) -------------------------------------------------------------------------------
@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('Cc', [1, 21, 300])                                  # 300: each thread loops over two channels
@pytest.mark.parametrize('npix', [1, 64, 65, 1000])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_bias_grad(lib, cuda, dtype, npix, Cc, strided):
    """db[c] += sum_p dy[p, c] against a float64 column sum of the stored values plus the prior db.  The bar comes from the kernel:
    each block sums its 64 pixels serially in fp32 (<= 64 roundings on partial sums bounded by sum |dy|), then adds its partial sum
    to db with one atomic fp32 add (ceil(npix / 64) roundings on values bounded by |db0| + sum |dy|), so
        |err_c| <= (64 + ceil(npix / 64) + 1) * 2^-24 * (|db0_c| + sum_p |dy_pc|).
    Two calls: the bound as written for one call is no guarantee for two, so it is re-derived for what two calls compute.  Each
    block's serial sum s_k is the same in both calls (error <= 64 * 2^-24 * sum_block |dy| each time it is added), and db receives
    2 * ceil(npix / 64) atomic adds, each rounding a partial result bounded by |db0| + 2 sum |dy|.  Against db0 + 2 sum that gives
        |err_c| <= (64 + 2 ceil(npix / 64) + 1) * 2^-24 * (|db0_c| + 2 sum_p |dy_pc|),
    the one-call formula with the atomics and the summed magnitude of the two-call problem."""
    tdt = TDT[dtype]
    ps = Cc + 11 if strided else Cc
    rng = np.random.default_rng(npix + Cc)
    n = (npix - 1) * ps + Cc                                                  # exactly what the kernel may read
    host = torch.full((npix * ps,), float('nan'))                             # the gaps between the rows are poison
    host.view(npix, ps)[:, :Cc] = torch.from_numpy(rng.standard_normal((npix, Cc)).astype(np.float32))
    dy = host[:n].to(tdt)
    stored = dy.float().numpy().astype(np.float64)
    rows = np.stack([stored[p * ps:p * ps + Cc] for p in range(npix)])
    db0 = (3.0 * rng.standard_normal(Cc)).astype(np.float32)
    buf, db = guarded((Cc,), torch.float32, cuda, torch.from_numpy(db0))
    dyd = dy.to(cuda)
    nb = -(-npix // 64)
    mag = np.abs(rows).sum(0)
    for call in (1, 2):
        assert lib.yolo_bias_grad(dyd.data_ptr(), db.data_ptr(), npix, Cc, ps if strided else 0, LDT[dtype], st()) == 0
        assert margins_intact(buf)
        got = db.cpu().numpy().astype(np.float64)
        want = db0.astype(np.float64) + call * rows.sum(0)
        bar = (64 + call * nb + 1) * 2.0 ** -24 * (np.abs(db0) + call * mag)
        err = np.abs(got - want)
        print('RATIO bias_grad %s npix=%d C=%d strided=%d call=%d %.3f' % (dtype, npix, Cc, strided, call, (err / bar).max()))
        assert (err <= bar).all(), (call, float((err / bar).max()))


# ---- BatchNorm folding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['bn', 'beta_only', 'plain'])
@pytest.mark.parametrize('Cc', [1, 255, 257])
def test_fold_bn(lib, cuda, Cc, path):
    """scale = gamma / sqrt(var + eps), bias = beta - mean * scale against float64.  scale: rtol 1e-6 (an add, a square root and a
    divide in fp32, at the <= 2.5 ulp the HIP maths documentation gives for divide / sqrt); bias: 1e-6 * (|beta| + |mean * scale|),
    because the subtraction may cancel.  Without gamma: scale exactly 1 and bias exactly beta (or 0).  Pad entries exactly zero."""
    rng = np.random.default_rng(Cc)
    Cp = -(-Cc // 256) * 256
    eps = 1e-5
    gamma = rng.uniform(-2, 2, Cc).astype(np.float32)
    beta = rng.standard_normal(Cc).astype(np.float32)
    mean = (3 * rng.standard_normal(Cc)).astype(np.float32)
    var = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), Cc)).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(cuda)
    g_, b_, m_, v_ = dev(gamma), dev(beta), dev(mean), dev(var)
    bs, scale = guarded((Cp,), torch.float32, cuda)
    bb, bias = guarded((Cp,), torch.float32, cuda)
    args = {'bn': (g_.data_ptr(), b_.data_ptr(), m_.data_ptr(), v_.data_ptr()),
            'beta_only': (None, b_.data_ptr(), m_.data_ptr(), v_.data_ptr()),
            'plain': (None, None, None, None)}[path]
    assert lib.yolo_fold_bn(*args, eps, scale.data_ptr(), bias.data_ptr(), Cc, st()) == 0
    assert margins_intact(bs) and margins_intact(bb)
    s, b = scale.cpu().numpy(), bias.cpu().numpy()
    assert (s[Cc:].view(np.int32) == 0).all() and (b[Cc:].view(np.int32) == 0).all()
    if path == 'bn':
        rs = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + np.float64(np.float32(eps)))
        rb = beta.astype(np.float64) - mean.astype(np.float64) * rs
        es, eb = np.abs(s[:Cc] - rs), np.abs(b[:Cc] - rb)
        bar_s, bar_b = 1e-6 * np.abs(rs), 1e-6 * (np.abs(beta) + np.abs(mean * rs))
        print('RATIO fold_bn C=%d scale %.3f bias %.3f' % (Cc, (es / bar_s).max(), (eb / bar_b).max()))
        assert (es <= bar_s).all() and (eb <= bar_b).all()
    else:
        assert (s[:Cc] == 1).all()
        assert np.array_equal(b[:Cc].view(np.int32), (beta if path == 'beta_only' else np.zeros(Cc, np.float32)).view(np.int32))


def test_fold_bn_refuses_half_a_batchnorm(lib, cuda):
    g_ = torch.ones(8, device=cuda)
    buf, out = guarded((512,), torch.float32, cuda)
    assert lib.yolo_fold_bn(g_.data_ptr(), g_.data_ptr(), None, g_.data_ptr(), 1e-5, out.data_ptr(), out[256:].data_ptr(), 8, st()) == L.EINVAL
    assert lib.yolo_fold_bn(g_.data_ptr(), g_.data_ptr(), g_.data_ptr(), g_.data_ptr(), 1e-5, out.data_ptr(), None, 8, st()) == L.EINVAL
    assert untouched(buf)
