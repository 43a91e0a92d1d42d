"""Train-mode BatchNorm batch statistics on ill-conditioned channels (rho = mean^2 / var large), on every path that takes them for the
35 ms training step: the yolo_bn_train_* family, the convolution statistics epilogue, the stem's fused sums, and the Trainer's
rule that keeps small maps on the pivoted reduction.  Reference and channel classes: tests/bn_cond_ref.py (checked on the CPU by
tests/test_bn_cond_host.py, which also shows that the invstd bar separates a pivoted sum from a plain one).

Bars, the same on every path (DESIGN.md states them as the contract), against float64 two-pass statistics of the values AS STORED:
  mean         |mean - m64| <= 2^-23 |m64| + 1e-6 sqrt(v64)
  invstd       |invstd * sqrt(v64 + eps) - 1| <= 1e-3
  running_var  |rv - (0.9 * 1 + 0.1 v64)| <= 1e-4 v64 + 2^-23 |ref|
Everything behind the statistics (z, dy, dgamma, dbeta) is judged ONE HOP at a time: against the float64 restatement fed the
kernel's own float32 mean and invstd, at the bars the existing test of the dtype uses (test_bn_train_fwd_bwd, test_bn_train_bf16,
test_split_bn_train_fwd_bwd; the epilogue's backward at test_conv_statistics_epilogue's), with the scale taken per CHANNEL: a
constant channel's dy is 316 times a benign one's.

LeakyReLU's kink.  An element whose pre-activation a = gamma * xhat + beta lies within 2e-5 (1 + max|a|) of zero (tools/fuzz_bn.py's
window) may take either slope on the device.  Such elements are left out of the dy comparison, and their number is capped at 0.1 %
of the tensor (asserted).  Their channel is NOT left out: at 40 000 pixels a third of all channels holds such an element, so the
tolerance of that channel's dgamma / dbeta (and, through them, of its dy) is widened by exactly what the flagged elements can move
them, (1 - slope) |dz| each -- zero for a channel without one.  |beta| >= 0.05 keeps constant channels (xhat = 0) off the kink.

A true dy far below its own terms (two pixels normalise to +-1: dy is O(eps / var)) is compared at the scale of the terms: the scale
of a channel does not go below 1e-2 gamma invstd max|dz|, since the fp32 evaluation of da - mean(da) - xhat mean(da xhat) carries
2^-24 of those terms whatever is left of them.

For bf16 INPUTS plain fp32 sums are exact or nearly so (tests/test_bn_cond_host.py): the bf16 cases pin the bars, they do not
discriminate between a pivoted and a plain sum.  Every test prints its maxima per class (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_cond_ref as B
from test_gpu_split_train import _to_split, _val
from util import LDT
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu

EPS, MOM, SLOPE = B.EPS, B.MOMENTUM, B.SLOPE


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(v, kind, cuda):
    """(npix, C) float32 values that `kind` stores exactly -> the device tensor."""
    if kind == 'bf16x3':
        return _to_split(np.array(v, dtype=np.float32), cuda)                    # (a copy: the shared inputs are read-only)
    t = torch.tensor(np.asarray(v, dtype=np.float32)).to(cuda)               # (a copy: the shared inputs are read-only)
    return t.bfloat16() if kind == 'bf16' else t


def _host(t, kind, Cc):
    return (_val(t, Cc) if kind == 'bf16x3' else t.float().cpu()).double().numpy()


def _vec(v, cuda):
    return torch.from_numpy(np.asarray(v, dtype=np.float32)).to(cuda)


def _params(Cc, seed):
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.5, 1.5, Cc).astype(np.float32)
    beta = (rng.choice([-1.0, 1.0], Cc) * rng.uniform(0.05, 0.3, Cc)).astype(np.float32)
    return gamma, beta


def run_bn(lib, cuda, kind, y, dz, res, gamma, beta, pp):
    """One forward and one backward call of the three-launch (pp False) or the two-launch form -> float64 host arrays."""
    npix, Cc = y.shape
    yd, dzd = _dev(y, kind, cuda), _dev(dz, kind, cuda)
    rd = _dev(res, kind, cuda) if res is not None else None
    g_, b_ = _vec(gamma, cuda), _vec(beta, cuda)
    z, dy = torch.zeros_like(yd), torch.zeros_like(yd)
    mean, invstd, dg, db = (torch.full((Cc,), float('nan'), device=cuda) for _ in range(4))
    rm, rv = torch.zeros(Cc, device=cuda), torch.ones(Cc, device=cuda)
    ws = [torch.zeros(2 * Cc, dtype=torch.float64, device=cuda) for _ in range(2)]
    dt, st = LDT[kind], _st()
    if pp:
        L.check(lib.yolo_bn_train_fwd_pp(L.ptr(yd), L.ptr(g_), L.ptr(b_), L.ptr(rd), L.ptr(z), L.ptr(mean), L.ptr(invstd), L.ptr(rm),
                                         L.ptr(rv), L.ptr(ws[0]), L.ptr(ws[1]), 2 * Cc, npix, Cc, EPS, MOM, SLOPE, dt, st), 'bn fwd pp')
        L.check(lib.yolo_bn_train_bwd_pp(L.ptr(dzd), L.ptr(yd), L.ptr(mean), L.ptr(invstd), L.ptr(g_), L.ptr(b_), L.ptr(dy), L.ptr(dg),
                                         L.ptr(db), L.ptr(ws[1]), L.ptr(ws[0]), 2 * Cc, npix, Cc, SLOPE, dt, st), 'bn bwd pp')
    else:
        L.check(lib.yolo_bn_train_fwd(L.ptr(yd), L.ptr(g_), L.ptr(b_), L.ptr(rd), L.ptr(z), L.ptr(mean), L.ptr(invstd), L.ptr(rm),
                                      L.ptr(rv), L.ptr(ws[0]), npix, Cc, EPS, MOM, SLOPE, dt, st), 'bn fwd')
        L.check(lib.yolo_bn_train_bwd(L.ptr(dzd), L.ptr(yd), L.ptr(mean), L.ptr(invstd), L.ptr(g_), L.ptr(b_), L.ptr(dy), L.ptr(dg),
                                      L.ptr(db), L.ptr(ws[0]), npix, Cc, SLOPE, dt, st), 'bn bwd')
    torch.cuda.synchronize()
    f = lambda t: t.cpu().double().numpy()
    assert bool((_host(yd, kind, Cc) == y.astype(np.float64)).all()), 'the generator must hand out values the type stores exactly'
    return dict(z=_host(z, kind, Cc), dy=_host(dy, kind, Cc), mean=f(mean), invstd=f(invstd), rm=f(rm), rv=f(rv), dgamma=f(dg),
                dbeta=f(db))


def judge_stats(what, names, got, m64, v64):
    """The three bars per channel; prints the maxima per class first."""
    em, ei = B.mean_err_ulps(got['mean'], m64), B.invstd_err(got['invstd'], v64)
    for cls in sorted(set(names)):
        i = [c for c, n in enumerate(names) if n == cls]
        print('%s  %-16s mean %.2f ulp   invstd %.2e' % (what, cls, em[i].max(), ei[i].max()))
    bad = lambda ok: [(names[c], c) for c in np.nonzero(~ok)[0]]
    ok = np.abs(got['mean'] - m64) <= B.mean_bar(m64, v64)
    assert ok.all(), (what, 'mean', bad(ok), float(em.max()))
    ok = ei <= B.INVSTD_BAR
    assert ok.all(), (what, 'invstd', bad(ok), float(ei.max()))
    if 'rv' in got:
        ref = 0.9 + 0.1 * v64
        ok = np.abs(got['rv'] - ref) <= B.running_var_bar(v64, ref)
        assert ok.all(), (what, 'running_var', bad(ok))
        # (test_bn_train_fwd_bwd's bar: 1 - 0.9f is 0.1 (1 + 2^-22) in float32, so running_mean cannot be held to the mean's)
        ok = np.abs(got['rm'] - 0.1 * m64) <= 1e-5 * np.abs(0.1 * m64) + 1e-6
        assert ok.all(), (what, 'running_mean', bad(ok))


# (rtol, atol) of z; of dy, atol in units of the channel's scale; of dgamma / dbeta as a function of the two references
Z_BAR = {'f32': (1e-4, 1e-5), 'bf16': (1e-2, 1e-2)}
DY_BAR = {'f32': (1e-3, 1e-4), 'bf16': (1e-2, 1e-2), 'bf16x3': (0.0, 1e-4)}
PG_BAR = {'f32': lambda dg, db: (1e-4, 1e-4 + 0 * dg),                      # test_bn_train_fwd_bwd
          'bf16x3': lambda dg, db: (1e-4, 1e-4 + 0 * dg),                   # (the split path runs the same sums: f32's bar)
          'bf16': lambda dg, db: (1e-4, 1e-5 * (np.abs(dg) + np.abs(db))),  # test_conv_statistics_epilogue, mode 2, per channel
          'epilogue': lambda dg, db: (1e-4, 1e-5 * (np.abs(dg).max() + np.abs(db).max()) + 0 * dg)}


def judge_forward(what, kind, names, got, y, gamma, beta, res):
    zr = B.forward64(y, got['mean'], got['invstd'], gamma, beta, res)
    d = np.abs(got['z'] - zr)
    if kind == 'bf16x3':                                                    # test_split_bn_train_fwd_bwd: 3e-5 of |z| + 1e-3 max|z|
        ok = d < 3e-5 * (np.abs(zr) + 1e-3 * np.abs(zr).max(axis=0))
    else:
        rtol, atol = Z_BAR[kind]
        ok = d <= rtol * np.abs(zr) + atol
        print('%s  z: worst error %.2f of its bar' % (what, float((d / (rtol * np.abs(zr) + atol)).max())))
    assert ok.all(), (what, 'z', sorted({names[c] for c in np.nonzero(~ok)[1]}), float(d.max()))


def judge_backward(what, kind, names, got, y, dz, gamma, beta, mean=None, invstd=None, pg='', dy_bar=None, window_from=0):
    mean = got['mean'] if mean is None else mean
    invstd = got['invstd'] if invstd is None else invstd
    npix = y.shape[0]
    xhat, a = B.preact64(y, mean, invstd, gamma, beta)
    # (window_from = 1: max|a| is taken without pixel 0 -- a planted outlier there, itself 700 sigma from the kink, would widen the
    #  window of every other element of its channel by three orders of magnitude)
    flagged = np.abs(a) < 2e-5 * (1.0 + np.abs(a[window_from:]).max(axis=0))
    share = float(flagged.mean())
    print('%s  elements at the kink: %d of %d, in %d of %d channels' % (what, flagged.sum(), flagged.size, flagged.any(axis=0).sum(), y.shape[1]))
    assert share <= 1e-3, (what, 'too many elements near the kink', share)
    amb_b = (np.abs(dz) * flagged).sum(axis=0) * (1.0 - SLOPE)
    amb_g = (np.abs(dz * xhat) * flagged).sum(axis=0) * (1.0 - SLOPE)
    dyr, dgr, dbr = B.backward64(dz, y, mean, invstd, gamma, beta)
    rtol, atol = PG_BAR[pg or kind](dgr, dbr)
    for name, g, r, amb in (('dgamma', got['dgamma'], dgr, amb_g), ('dbeta', got['dbeta'], dbr, amb_b)):
        ok = np.abs(g - r) <= rtol * np.abs(r) + atol + amb
        clean = amb == 0
        if clean.any() and (rtol * np.abs(r) + atol)[clean].min() > 0:
            print('%s  %s: worst error %.3f of its bar (channels with no element at the kink)'
                  % (what, name, float((np.abs(g - r) / (rtol * np.abs(r) + atol))[clean].max())))
        assert ok.all(), (what, name, [(names[c], float(g[c]), float(r[c])) for c in np.nonzero(~ok)[0]])
    gi = np.abs(gamma.astype(np.float64) * invstd)
    scale = np.maximum(np.abs(dyr).max(axis=0), 1e-2 * gi * np.abs(dz).max(axis=0))
    rtol, atol = dy_bar or DY_BAR[kind]
    tol = rtol * np.abs(dyr) + atol * scale + gi * (amb_b + np.abs(xhat) * amb_g) / npix
    ok = (np.abs(got['dy'] - dyr) <= tol) | flagged
    if (tol > 0).all():
        print('%s  dy: worst error %.3f of its bar' % (what, float((np.abs(got['dy'] - dyr) / tol)[~flagged].max())))
    assert ok.all(), (what, 'dy', sorted({names[c] for c in np.nonzero(~ok)[1]}), float((np.abs(got['dy'] - dyr) / scale).max()))


# ---- (a) yolo_bn_train_fwd + _bwd and the two-launch forms ------------------------------------------------------------------------------
_CASES = {}


def _case(kind, npix, Cc):
    """Inputs and the float64 statistics of one (kind, shape), made once and left unchanged."""
    key = (kind, npix, Cc)
    if key not in _CASES:
        y, names, rho = B.channels(npix, Cc, kind, seed=100 + npix % 97 + Cc)
        rng = np.random.default_rng(npix + Cc)
        dz = B.store(rng.standard_normal((npix, Cc)), kind)
        res = B.store(rng.standard_normal((npix, Cc)), kind)
        # gamma / beta: the first draw that leaves the float64 reference a tenth of the kink cap -- a bf16 channel holds a handful of
        # distinct values, and one of them inside the window would put a fifth of the channel there (chosen on the reference alone)
        m64, v64 = B.stats64(y)
        for seed in range(npix, npix + 64):
            gamma, beta = _params(Cc, seed)
            _, a = B.preact64(y, m64, B.invstd64(v64), gamma, beta)
            if float((np.abs(a) < 4e-5 * (1.0 + np.abs(a).max(axis=0))).mean()) <= 1e-4:        # (twice the window: no value at its edge)
                break
        else:
            raise AssertionError('no gamma / beta keeps the channels off the kink')
        _CASES[key] = (y, names, rho, dz, res, gamma, beta, B.stats64(y))
        for a in (y, dz, res):
            a.setflags(write=False)
    return _CASES[key]


@pytest.mark.parametrize('with_res', [False, True], ids=['plain', 'residual'])
@pytest.mark.parametrize('pp', [False, True], ids=['three', 'pp'])
@pytest.mark.parametrize('npix,Cc', [(40000, 16), (4099, 264), (3, 8), (2, 8), (1, 8)])
@pytest.mark.parametrize('kind', ['f32', 'bf16x3', 'bf16'])
def test_bn_train_on_ill_conditioned_channels(lib, cuda, kind, npix, Cc, pp, with_res):
    y, names, rho, dz, res, gamma, beta, (m64, v64) = _case(kind, npix, Cc)
    what = '%s %dx%d %s' % (kind, npix, Cc, 'pp' if pp else 'three')
    got = run_bn(lib, cuda, kind, y, dz, res if with_res else None, gamma, beta, pp)
    judge_stats(what, names, got, m64, v64)
    if npix == 1:                                            # var 0: the mean IS the value; invstd = 1 / sqrt(eps) is in the bar above
        assert np.array_equal(got['mean'].astype(np.float32), y[0]) and (v64 == 0).all()
    const = [c for c, n in enumerate(names) if n in ('const', 'zero')]
    assert np.array_equal(got['mean'][const].astype(np.float32), y[0, const])        # (2^-23 |m| allows an ulp; a constant has none)
    judge_forward(what, kind, names, got, y, gamma, beta, res if with_res else None)
    judge_backward(what, kind, names, got, y, dz, gamma, beta)


# ---- (b) the pivot adversary at its sharpest --------------------------------------------------------------------------------------------
def test_bn_train_pivot_adversary_2_20(lib, cuda):
    """f32, 2^20 pixels, +-1000 + randn with pixel 0 = 0: sums around pixel 0 are sums around nothing, rho' = 1e6 / (1 + 1e6 / 2^20)
    = 5e5 -- the largest a pivot at pixel 0 can be made to see at this size."""
    npix, Cc = 1 << 20, 8
    rng = np.random.default_rng(20)
    y = (np.where(np.arange(Cc) % 2, -1000.0, 1000.0)[None, :] + rng.standard_normal((npix, Cc))).astype(np.float32)
    y[0] = 0.0
    dz = rng.standard_normal((npix, Cc)).astype(np.float32)
    gamma, beta = _params(Cc, 21)
    m64, v64 = B.stats64(y)
    rho = m64 * m64 / v64
    assert (rho > 4e5).all() and (rho < 6e5).all()
    names = ['adversary%s' % '+-'[c % 2] for c in range(Cc)]
    first = None
    for pp in (False, True):
        what = 'f32 2^20x8 %s' % ('pp' if pp else 'three')
        got = run_bn(lib, cuda, 'f32', y, dz, None, gamma, beta, pp)
        judge_stats(what, names, got, m64, v64)
        if first is None:
            first = got
            judge_forward(what, 'f32', names, got, y, gamma, beta, None)
            judge_backward(what, 'f32', names, got, y, dz, gamma, beta, window_from=1)
        else:                                               # the two forms are bit-identical (tests/test_gpu_train_ops.py): one reference
            for k in ('mean', 'invstd', 'z', 'dy', 'dgamma', 'dbeta'):
                assert np.array_equal(first[k], got[k]), k


# ---- (c) the convolution statistics epilogue, mode 1 -> yolo_bn_train_fwd_partials ------------------------------------------------------
C3, C1, C1W, CS2 = (2, 32, 48, 48, 64, 3, 1), (2, 64, 48, 48, 64, 1, 1), (2, 256, 48, 48, 128, 1, 1), (2, 32, 96, 96, 64, 3, 2)
# one variant per family (tests/util.py conv_variant(..., stats_mode=1) names them): a 256-cout and a 128-cout pipelined 3x3 tile,
# the tiled 1x1 the Trainer runs where the plan holds the flat kernel (39, on a shape the flat kernel takes), a 1x1 tile at the
# narrow shape, a stride-2 tile, the streaming kernel, the generic kernel, and the library's own choice for each shape
EPILOGUE = [(C3, 2), (C3, 7), (C1W, 39), (C1, 12), (CS2, 10), (C3, 13), (C3, 1), (C3, 0), (C1, 0), (CS2, 0)]
OFFSETS, SPREADS = [0.0, 4.0, 100.0, -100.0, 1000.0], [1.0, 0.25, 0.0]


def _planted_conv(lib, cuda, case, algo, stats_mode, extra=None):
    """A bf16 convolution whose output channel c is m_c + s_c * noise: input channel 0 is 1.0 and w[c, 0, centre] = m_c (bf16-exact,
    the centre tap never falls into the padding), the other weights of the channel are scaled by s_c, or zero for a constant channel.
    -> (descriptor, keep-alive list, y, partial rows, rows)."""
    N, Cin, H, W, Cout, k, stride = case
    rng = np.random.default_rng(Cout + k)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    x[..., 0] = 1.0
    m = np.array([OFFSETS[c % len(OFFSETS)] for c in range(Cout)])
    s = np.array([SPREADS[c % len(SPREADS)] for c in range(Cout)])
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32) * s[:, None, None, None].astype(np.float32)
    w[:, 0] = 0.0
    w[:, 0, k // 2, k // 2] = m
    xd = torch.from_numpy(x).to(cuda).bfloat16()
    wd = torch.from_numpy(w).to(cuda)
    wp = torch.empty(lib.yolo_packed_weight_bytes(Cout, Cin, k, L.BF16), dtype=torch.uint8, device=cuda)
    L.check(lib.yolo_pack_conv_weights(wd.data_ptr(), wp.data_ptr(), Cout, Cin, k, L.BF16, _st()), 'pack')
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.full((N, Ho, Wo, Cout), float('nan'), dtype=torch.bfloat16, device=cuda)
    d = L.ConvDesc()
    d.x, d.w_packed, d.y = xd.data_ptr(), wp.data_ptr(), y.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, Cin, Cout, k, stride, L.BF16, 1.0, algo
    d.stats, d.stats_mode = 1, stats_mode
    for f, v in (extra or {}).items():
        setattr(d, f, v)
    rows = lib.yolo_conv_stats_rows(C.byref(d))
    assert rows > 0, ('no statistics epilogue for', case, algo)
    part = torch.full((rows, 2, lib.yolo_padded_channels(Cout)), float('nan'), device=cuda)
    d.stats = part.data_ptr()
    return d, [xd, wd, wp], y, part, rows


def _fwd_from(lib, cuda, y, gamma, beta, part=None, rows=0, cp=0):
    """yolo_bn_train_fwd_partials (part given) or yolo_bn_train_fwd_pp over the stored bf16 map y (N, H, W, C)."""
    Cc = y.shape[-1]
    npix = y.numel() // Cc
    g_, b_ = _vec(gamma, cuda), _vec(beta, cuda)
    z = torch.empty_like(y)
    mean, invstd = torch.empty(Cc, device=cuda), torch.empty(Cc, device=cuda)
    rm, rv = torch.zeros(Cc, device=cuda), torch.ones(Cc, device=cuda)
    ws = [torch.zeros(2 * Cc, dtype=torch.float64, device=cuda) for _ in range(2)]
    if part is not None:
        L.check(lib.yolo_bn_train_fwd_partials(part.data_ptr(), rows, cp, y.data_ptr(), g_.data_ptr(), b_.data_ptr(), None, z.data_ptr(),
                                               mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[0].data_ptr(),
                                               ws[1].data_ptr(), 2 * Cc, npix, Cc, EPS, MOM, SLOPE, L.BF16, _st()), 'fwd partials')
    else:
        L.check(lib.yolo_bn_train_fwd_pp(y.data_ptr(), g_.data_ptr(), b_.data_ptr(), None, z.data_ptr(), mean.data_ptr(),
                                         invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), 2 * Cc,
                                         npix, Cc, EPS, MOM, SLOPE, L.BF16, _st()), 'fwd pp')
    torch.cuda.synchronize()
    f = lambda t: t.cpu().double().numpy()
    return dict(z=f(z.float()).reshape(npix, Cc), mean=f(mean), invstd=f(invstd), rm=f(rm), rv=f(rv))


def _rho_names(m64, v64):
    rho = np.where(v64 > 0, m64 * m64 / np.where(v64 > 0, v64, 1.0), np.where(m64 != 0, np.inf, 0.0))
    return rho, ['var0' if v == 0 else 'rho>=1e6' if r >= 1e6 else 'rho>=1e4' if r >= 1e4 else 'rho<1e4' for r, v in zip(rho, v64)]


@pytest.mark.parametrize('case,algo', [pytest.param(c, a, id='%s-a%d' % ('x'.join(map(str, c)), a)) for c, a in EPILOGUE])
def test_conv_epilogue_statistics_on_planted_offsets(lib, cuda, case, algo):
    """Both ways to the BatchNorm of a stored map -- the convolution's partial rows and the reduction over the map -- against the float64
    statistics of that map.  4608 output pixels: the first size the Trainer's rule lets take the epilogue's sums."""
    d, keep, y, part, rows = _planted_conv(lib, cuda, case, algo, 1)
    L.check(lib.yolo_conv_fwd(C.byref(d), _st()), 'conv')
    torch.cuda.synchronize()
    Cout = case[4]
    ys = y.float().cpu().double().numpy().reshape(-1, Cout)
    assert ys.shape[0] == 4608 and np.isfinite(ys).all()
    m64, v64 = B.stats64(ys)
    rho, names = _rho_names(m64, v64)
    assert (rho[np.isfinite(rho)] >= 1e4).any() and ((v64 == 0) & (m64 != 0)).any(), 'the planted offsets did not arrive'
    gamma, beta = _params(Cout, 31)
    what = '%s a%d' % ('x'.join(map(str, case)), algo)
    for way, got in (('partials', _fwd_from(lib, cuda, y, gamma, beta, part, rows, lib.yolo_padded_channels(Cout))),
                     ('reduce  ', _fwd_from(lib, cuda, y, gamma, beta))):
        judge_stats('%s %s' % (what, way), names, got, m64, v64)
        judge_forward('%s %s' % (what, way), 'bf16', names, got, ys, gamma, beta, None)


# ---- (d) mode 2 -> yolo_bn_train_bwd_partials -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,algo', [pytest.param(c, a, id='%s-a%d' % ('x'.join(map(str, c)), a)) for c, a in [(C3, 2), (C1, 0)]])
def test_conv_epilogue_backward_sums_on_ill_conditioned_y(lib, cuda, case, algo):
    """The data gradient's epilogue takes sum(da), sum(da * xhat) of the BatchNorm behind its output, xhat = (stats_y - mean) * invstd
    formed in fp32 from the fp32-rounded mean: stats_y drawn from the bf16 classes, the statistics float64 ones rounded to fp32,
    dgamma / dbeta / dy against backward64 at test_conv_statistics_epilogue's mode-2 bars."""
    N, Cin, H, W, Cout, k, stride = case
    npix = N * H * W
    yb_h, names, _ = B.channels(npix, Cout, 'bf16', seed=41)
    m64, v64 = B.stats64(yb_h)
    mean, invstd = m64.astype(np.float32), B.invstd64(v64).astype(np.float32)
    gamma, beta = _params(Cout, 42)
    rng = np.random.default_rng(43)
    yb = torch.from_numpy(yb_h).to(cuda).bfloat16().view(N, H, W, Cout)
    acc0 = torch.from_numpy((0.5 * rng.standard_normal((N, H, W, Cout))).astype(np.float32)).to(cuda).bfloat16()
    tm, ti, tg, tb = _vec(mean, cuda), _vec(invstd, cuda), _vec(gamma, cuda), _vec(beta, cuda)
    # an ordinary convolution (unit-variance output) accumulating into acc0: the gradient that reaches the BatchNorm
    x = torch.from_numpy(rng.standard_normal((N, H, W, Cin)).astype(np.float32)).to(cuda).bfloat16()
    w = torch.from_numpy((rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)).to(cuda)
    wp = torch.empty(lib.yolo_packed_weight_bytes(Cout, Cin, k, L.BF16), dtype=torch.uint8, device=cuda)
    L.check(lib.yolo_pack_conv_weights(w.data_ptr(), wp.data_ptr(), Cout, Cin, k, L.BF16, _st()), 'pack')
    y = acc0.clone()
    d = L.ConvDesc()
    d.x, d.w_packed, d.y, d.residual = x.data_ptr(), wp.data_ptr(), y.data_ptr(), y.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, Cin, Cout, k, stride, L.BF16, 1.0, algo
    d.stats, d.stats_mode, d.stats_y = 1, 2, yb.data_ptr()
    d.stats_mean, d.stats_invstd, d.stats_gamma, d.stats_beta, d.stats_slope = tm.data_ptr(), ti.data_ptr(), tg.data_ptr(), tb.data_ptr(), SLOPE
    rows = lib.yolo_conv_stats_rows(C.byref(d))
    assert rows > 0
    cp = lib.yolo_padded_channels(Cout)
    part = torch.full((rows, 2, cp), float('nan'), device=cuda)
    d.stats = part.data_ptr()
    L.check(lib.yolo_conv_fwd(C.byref(d), _st()), 'conv')
    dy = torch.empty_like(y)
    dg, db = torch.empty(Cout, device=cuda), torch.empty(Cout, device=cuda)
    ws = [torch.zeros(2 * Cout, dtype=torch.float64, device=cuda) for _ in range(2)]
    L.check(lib.yolo_bn_train_bwd_partials(part.data_ptr(), rows, cp, y.data_ptr(), yb.data_ptr(), tm.data_ptr(), ti.data_ptr(),
                                           tg.data_ptr(), tb.data_ptr(), dy.data_ptr(), dg.data_ptr(), db.data_ptr(), ws[0].data_ptr(),
                                           ws[1].data_ptr(), 2 * Cout, npix, Cout, SLOPE, L.BF16, _st()), 'bwd partials')
    torch.cuda.synchronize()
    f = lambda t: t.float().cpu().double().numpy()
    dz = f(y).reshape(npix, Cout)                            # the stored gradient: what the BatchNorm backward reads
    assert np.isfinite(dz).all() and float(np.abs(dz - f(acc0).reshape(npix, Cout)).max()) > 0.5
    got = dict(dy=f(dy).reshape(npix, Cout), dgamma=f(dg), dbeta=f(db))
    judge_backward('%s a%d mode 2' % ('x'.join(map(str, case)), algo), 'bf16', names, got, yb_h.astype(np.float64), dz, gamma, beta,
                   mean=mean.astype(np.float64), invstd=invstd.astype(np.float64), pg='epilogue', dy_bar=(0.0, 1e-2))


# ---- (e) yolo_stem_conv_fwd_stats ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('image', ['constant', 'noise'])
@pytest.mark.parametrize('shape', [(2, 64, 96, 32), (1, 37, 61, 32)])
def test_stem_statistics_on_flat_images(lib, cuda, shape, image):
    """The stem's own sums have the longest runs and no small-map rule: a flat image (exactly 0.5, or 0.5 + 0.002 noise) through weights
    whose taps sum to a few units per channel, almost all of it on the centre tap so that the padded border stays flat too."""
    N, H, W, Cout = shape
    rng = np.random.default_rng(H)
    x = np.full((N, 3, H, W), 0.5, dtype=np.float32)
    if image == 'noise':
        x += (0.002 * rng.standard_normal(x.shape)).astype(np.float32)
    w = (0.002 * rng.standard_normal((Cout, 3, 3, 3))).astype(np.float32)
    w[:, :, 1, 1] += (rng.choice([-1.0, 1.0], Cout) * rng.uniform(2.0, 6.0, Cout) / 3.0).astype(np.float32)[:, None]
    xd, wd = torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda)
    ones, zeros = torch.ones(Cout, device=cuda), torch.zeros(Cout, device=cuda)
    y = torch.full((N, H, W, Cout), float('nan'), dtype=torch.bfloat16, device=cuda)
    rows = lib.yolo_stem_stats_rows(N, H, W, Cout)
    assert rows > 0
    part = torch.full((rows, 2, Cout), float('nan'), device=cuda)
    L.check(lib.yolo_stem_conv_fwd_stats(xd.data_ptr(), wd.data_ptr(), ones.data_ptr(), zeros.data_ptr(), y.data_ptr(), N, H, W, 3, Cout,
                                         L.BF16, 1.0, part.data_ptr(), _st()), 'stem')
    torch.cuda.synchronize()
    ys = y.float().cpu().double().numpy().reshape(-1, Cout)
    assert np.isfinite(ys).all()
    m64, v64 = B.stats64(ys)
    rho, names = _rho_names(m64, v64)
    assert (rho >= 1e4).sum() >= Cout // 2, 'the stored map is not ill-conditioned'
    gamma, beta = _params(Cout, 51)
    what = 'stem %s %s' % ('x'.join(map(str, shape)), image)
    for way, got in (('partials', _fwd_from(lib, cuda, y, gamma, beta, part, rows, Cout)), ('reduce  ', _fwd_from(lib, cuda, y, gamma, beta))):
        judge_stats('%s %s' % (what, way), names, got, m64, v64)
        judge_forward('%s %s' % (what, way), 'bf16', names, got, ys, gamma, beta, None)


# ---- (f) the Trainer's rule ---------------------------------------------------------------------------------------------------------------
def test_trainer_keeps_small_maps_on_the_pivoted_reduction(lib, cuda):
    """bf16 fused forward on the micro net at 128 x 192, batch 2: maps from 49 152 pixels down to a few dozen.  Every conv_bn below 4096
    output pixels runs the reduction pass of its own (no statistics rows), and the epilogue is in use above the line."""
    from oracle import graph as og
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    spec, size = og.spec_micro(), (128, 192)
    P = og.init_params(og.build_graph(spec), seed=0, bn='random')
    net = CarNet(spec, dtype='bf16', device=cuda).load_params(P)
    tr = Trainer(net, size)
    assert tr._fuse_fwd
    x = torch.from_numpy(np.random.default_rng(2).random((2, 3) + size, dtype=np.float32)).to(cuda)
    outs = tr.forward(x)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    ops = [op for op in tr._plans[2].fwd if op['kind'] == 'conv_bn']
    pix = lambda op: int(np.prod(tuple(op['yraw'].shape)[:3]))
    small, large = [op for op in ops if pix(op) < 4096], [op for op in ops if pix(op) >= 4096]
    print('conv_bn ops: %d below 4096 pixels, %d from 4096 on, %d of those with statistics rows'
          % (len(small), len(large), sum(op['srows'] > 0 for op in large)))
    assert small and large
    assert all(op['srows'] == 0 and not op['desc'].stats for op in small), [(op['c'].name, pix(op), op['srows']) for op in small if op['srows']]
    assert any(op['srows'] > 0 for op in large)
    # the rule is what keeps them off the epilogue, not the kernels: the library would hand out rows for a small map's convolution
    willing = 0
    for op in small:
        d = op['desc']
        d.stats, d.stats_mode = 1, 1
        willing += lib.yolo_conv_stats_rows(C.byref(d)) > 0
        d.stats, d.stats_mode = None, 0
    assert willing > 0
