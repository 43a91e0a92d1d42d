"""The split types (dtype 'bf16x3' / 'f16x3') outside the storage's comfortable middle (tests/test_gpu_split.py covers every tile
variant there: N(0, 1) activations, 1 / sqrt(K) weights, channel counts in multiples of 32).

  * ragged channel slices as INPUT: Cin % 32 != 0 channels of a wider split buffer.  The kernels read each plane in whole
    32-channel K-chunks (include/yolo_amd.h, x_pixel_stride / x_lo_offset), so a chunk runs beyond the slice: into neighbouring
    channels (here the type's largest finite value: they may only ever meet zero weights), into pad channels (zero), and -- were a
    layout outside the contract -- into the next pixel and past the buffer, where the moat holds NaN;
  * ragged channel slices as OUTPUT, plain and up-sampled: nothing but the slice is written;
  * operands scaled by powers of two from half's subnormals to the top of its range, against the path's own arithmetic restated
    (tests/util.py ref_conv_split) and against float64 with a bound made of that restatement's own operand quantisation;
  * whole nets whose every activation buffer lies between two moats of NaN, one of them with pyramid levels of 16 and 48 channels:
    the down-sampling convolution behind such a level reads the ragged route half of a concat buffer.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graph as og, forward as of
from test_gpu_split import ALGOS, _check, _mk
from util import (guarded, guards_intact, moated, split_planes, run_conv, ref_conv, ref_conv_split, to_nhwc, from_nhwc,
                  eligible_pairs, conv_variant, LDT, TDT, SPLIT)
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu

MAPS = [(2, 7, 9), (2, 13, 13)]                      # tiles cross rows and images
CONVS = [(1, 1), (3, 1), (3, 2)]                     # (ksize, stride)


def _by_case(params):
    """eligible_pairs' (.., case, dtype, algo) params folded to one pytest item per (.., case, dtype) that takes every eligible variant
    in turn (the variants share operands and references; thousands of items became hundreds)."""
    groups = {}
    for p in params:
        groups.setdefault(p.values[:-1], (p.id.rsplit('-a', 1)[0], []))[1].append(p.values[-1])
    return [pytest.param(*key, tuple(algos), id=name) for key, (name, algos) in groups.items()]


def _each_variant(algos, run):
    """run(algo) for every variant; one assertion naming each variant that failed, so none hides behind another."""
    failed = []
    for algo in algos:
        try:
            run(algo)
        except AssertionError as e:
            failed.append('algo %d: %s' % (algo, str(e)[:600]))
    assert not failed, '%d of %d variants failed\n' % (len(failed), len(algos)) + '\n'.join(failed)


def _launch(lib, dev, dtype, xv, xshape, w, scale, bias, stride, yv, algo, up2=False):
    """yolo_conv_fwd (slope 0.1, no residual) on torch views of split tensors: xv (N, H, W, 2, Cin), yv (N, Ho', Wo', 2, Cout),
    either one possibly a channel slice of a wider buffer.  Weights, scale and bias as in util.run_conv: in moats / between guards."""
    N, H, W, Cin = xshape
    Cout, _, k, _ = w.shape
    st, dt = torch.cuda.current_stream().cuda_stream, LDT[dtype]
    wd = moated(torch.from_numpy(w).to(dev))
    wbuf, wp = guarded((lib.yolo_packed_weight_bytes(Cout, Cin, k, dt),), torch.uint8, dev)
    L.check(lib.yolo_pack_conv_weights(wd.data_ptr(), wp.data_ptr(), Cout, Cin, k, dt, st), 'pack')
    cp = lib.yolo_padded_channels(Cout)
    sc = torch.zeros(cp, device=dev); sc[:Cout] = torch.from_numpy(scale).to(dev)
    bi = torch.zeros(cp, device=dev); bi[:Cout] = torch.from_numpy(bias).to(dev)
    sc, bi = moated(sc), moated(bi)
    d = L.ConvDesc()
    d.x, d.w_packed, d.scale, d.bias, d.y = xv.data_ptr(), wp.data_ptr(), sc.data_ptr(), bi.data_ptr(), yv.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope, d.algo = N, H, W, Cin, Cout, k, stride, dt, 0.1, algo
    d.x_pixel_stride, d.x_lo_offset = xv.stride(2), xv.stride(3)
    d.y_pixel_stride, d.y_batch_stride, d.y_lo_offset, d.upsample2x = yv.stride(2), yv.stride(0), yv.stride(3), int(up2)
    rc = lib.yolo_conv_fwd(C.byref(d), st)
    assert rc == 0, 'yolo_conv_fwd rc=%d' % rc
    torch.cuda.synchronize()
    guards_intact(wbuf, wp)


# ---- A1: ragged input slices ---------------------------------------------------------------------------------------------------
# (Ctot, c0, Cin, Cp): x = channels [c0, c0 + Cin) of a split buffer of Ctot real channels with planes of Cp >= Ctot.  Middle:
# the chunk beyond the slice covers real channels; first; two tail slices, in planes wide enough for the chunk
# (Cp >= c0 + round_up(Cin, 32): the contract of include/yolo_amd.h -- what CarNet allocates for a concat buffer)
SLICES = [(128, 16, 40, 128), (64, 0, 24, 64), (32, 16, 16, 64), (96, 48, 48, 128)]


def _sliced_params():
    out = []
    for li, (Ctot, c0, Cin, Cp) in enumerate(SLICES):
        assert Cin % 8 == 0 and Cin % 32 and c0 + Cin <= Ctot <= Cp and Cp >= c0 + -(-Cin // 32) * 32
        cases = [(N, Cin, H, W, Cout, k, s, False) for (N, H, W) in MAPS for (k, s) in CONVS for Cout in (32, 64)]
        for p in eligible_pairs(cases, list(SPLIT), [0] + ALGOS, fields={'x_pixel_stride': 2 * Cp, 'x_lo_offset': Cp}):
            out.append(pytest.param(li, *p.values, id='c%dof%d-%s' % (c0, Ctot, p.id)))
    return _by_case(out)


@functools.lru_cache(maxsize=None)
def _conv_ref(case, dtype, seed):
    """(x, w, scale, bias, restated arithmetic, fp32 oracle) of one case: computed once, shared by the variants, never changed."""
    x, w, scale, bias, _ = _mk(case, seed)
    return (x, w, scale, bias, ref_conv_split(x, w, scale, bias, case[6], 0.1, rdt=TDT[dtype]), ref_conv(x, w, scale, bias, case[6], 0.1))


@pytest.mark.parametrize('li,case,dtype,algos', _sliced_params())
def test_split_ragged_input_slice(lib, cuda, li, case, dtype, algos):
    Ctot, c0, Cin, Cp = SLICES[li]
    N, _, H, W, Cout, k, stride, _ = case
    x, w, scale, bias, sim, ref = _conv_ref(case, dtype, 31)
    tdt = TDT[dtype]
    xbuf, full = guarded((N, H, W, 2, Cp), tdt, cuda)           # the last pixel's lo plane is followed directly by NaN
    full.zero_()                                                # pad channels: zero
    full[..., :Ctot] = torch.finfo(tdt).max                     # real channels outside the slice: finite, and large enough to show
    xv = full[..., c0:c0 + Cin]
    xv.copy_(to_nhwc(x, dtype, cuda)[..., :Cin])
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1

    def run(algo):
        ybuf, y = guarded((N, Ho, Wo, 2, Cout), tdt, cuda)
        _launch(lib, cuda, dtype, xv, (N, H, W, Cin), w, scale, bias, stride, y, algo)
        guards_intact(ybuf, y)
        guards_intact(xbuf, full)
        _check(from_nhwc(y), sim, ref, dtype)
    _each_variant(algos, run)


# ---- A2: ragged output slices --------------------------------------------------------------------------------------------------
# (Ctot, c0, Cout): y = channels [c0, c0 + Cout) of a split buffer with planes of round_up(Ctot, 32) channels, every element 7.0
OUT_SLICES = [(32, 24, 8), (64, 8, 24), (96, 56, 40), (40, 0, 40)]
OUT_CONVS = [(2, 64, 7, 9, 1, 1), (2, 32, 7, 9, 3, 1), (2, 32, 13, 13, 3, 2)]      # (N, Cin, H, W, ksize, stride)


def _out_params():
    out = []
    for li, (Ctot, c0, Cout) in enumerate(OUT_SLICES):
        Cp = -(-Ctot // 32) * 32
        for up2 in (0, 1):
            for (N, Cin, H, W, k, s) in OUT_CONVS:
                Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
                fields = {'y_pixel_stride': 2 * Cp, 'y_lo_offset': Cp, 'upsample2x': up2,
                          'y_batch_stride': Ho * Wo * 2 * Cp * (4 if up2 else 1)}
                for p in eligible_pairs([(N, Cin, H, W, Cout, k, s, False)], list(SPLIT), [0] + ALGOS, fields=fields):
                    out.append(pytest.param(li, up2, *p.values, id='c%dof%d-%s-%s' % (c0, Ctot, 'up2' if up2 else 'plain', p.id)))
    return _by_case(out)


@pytest.mark.parametrize('li,up2,case,dtype,algos', _out_params())
def test_split_ragged_output_slice(lib, cuda, li, up2, case, dtype, algos):
    Ctot, c0, Cout = OUT_SLICES[li]
    Cp = -(-Ctot // 32) * 32
    N, Cin, H, W, _, k, stride, _ = case
    x, w, scale, bias, sim, ref = _conv_ref(case, dtype, 32)
    tdt = TDT[dtype]
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    f = 2 if up2 else 1
    if up2:                                                     # gluoncv _upsample: repeat on W then H
        sim, ref = (np.repeat(np.repeat(a, 2, axis=2), 2, axis=3) for a in (sim, ref))
    xd = moated(to_nhwc(x, dtype, cuda))

    def run(algo):
        cbuf, cat = guarded((N, f * Ho, f * Wo, 2, Cp), tdt, cuda)
        cat.fill_(7.0)
        yv = cat[..., c0:c0 + Cout]
        _launch(lib, cuda, dtype, xd, (N, H, W, Cin), w, scale, bias, stride, yv, algo, up2=up2)
        guards_intact(cbuf, cat)
        _check(from_nhwc(yv), sim, ref, dtype)
        rest = cat.clone()
        rest[..., c0:c0 + Cout] = 7.0
        assert bool((rest == 7.0).all()), 'an element outside channels [%d, %d) of the output buffer was written' % (c0, c0 + Cout)
    _each_variant(algos, run)


# ---- A3: magnitudes ------------------------------------------------------------------------------------------------------------
# (x, w) scaled by exact powers of two (bias and residual by their product, so every term of the output scales alike).  f16x3: at
# x * 2^-10 the lo plane is all subnormal, at x * 2^-14 most of the hi plane too; (13, -3) puts max|x| = 4.28 * 2^13 = 35090 at half
# of half's range.
SCALES = [(0, 0), (-6, 0), (-10, 0), (-14, 0), (0, -8), (-8, -8), (13, -3)]
MAG_CASES = {'3x3': (2, 64, 13, 13, 64, 3, 1, True), '1x1': (2, 96, 16, 16, 64, 1, 1, False)}
MAG_ALGOS = {'3x3': [0, 1, 41, 4], '1x1': [0, 1, 40, 12]}       # heuristic, generic, the 64-cout split tile, a 128-cout tile
FLOOR = {'bf16x3': 0.0, 'f16x3': 2.0 ** -24}                     # one unit of the output pair's lo: half's subnormal spacing


def _mag_params():
    out = []
    for name, case in MAG_CASES.items():
        got = eligible_pairs([case], list(SPLIT), MAG_ALGOS[name])
        assert len(got) == 2 * len(MAG_ALGOS[name]), 'a pinned variant of the magnitude sweep is no longer eligible'
        out += [pytest.param(name, p.values[1], p.values[2], id='%s-%s-a%d' % (name, p.values[1], p.values[2])) for p in got]
    return out


@functools.lru_cache(maxsize=None)
def _mag_ref(name, dtype, sx, sw, zero_bias=False):
    """Scaled operands, the restated arithmetic, float64 truth and the bound on |kernel - truth|, all from the operands alone."""
    case = MAG_CASES[name]
    K, k, stride = case[1] * case[5] ** 2, case[5], case[6]
    x, w, scale, bias, r = _mk(case, 21)
    x, w, bias = np.ldexp(x, sx), np.ldexp(w, sw), np.ldexp(bias * (0 if zero_bias else 1), sx + sw)
    r = np.ldexp(r, sx + sw) if r is not None else None
    rdt = TDT[dtype]
    sim = ref_conv_split(x, w, scale, bias, stride, 0.1, residual=r, rdt=rdt)
    d64 = lambda a: torch.from_numpy(a).double()
    stored = lambda a: sum(p.double() for p in split_planes(torch.from_numpy(a), rdt))      # hi + lo as the path holds it
    conv = lambda a, b: F.conv2d(a, b, None, stride=stride, padding=k // 2)
    X, Wt, S, Bi = d64(x), d64(w), d64(scale).view(1, -1, 1, 1), d64(bias).view(1, -1, 1, 1)
    t = conv(X, Wt) * S + Bi
    truth = torch.where(t > 0, t, t * 0.1)
    # operand quantisation, first order, + fp32 accumulation of K products; LeakyReLU has slope <= 1: the epilogue scales by |scale|
    bound = (conv((stored(x) - X).abs(), Wt.abs()) + conv(X.abs(), (stored(w) - Wt).abs())
             + K * 2.0 ** -24 * conv(X.abs(), Wt.abs())) * S.abs()
    if r is not None:
        truth = truth + d64(r)
        bound = bound + (stored(r) - d64(r)).abs()              # (the residual is an operand too: read as a pair)
    bound = bound + FLOOR[dtype]                                # the output pair's quantisation
    return x, w, scale, bias, r, sim, truth.numpy(), bound.numpy()


@pytest.mark.parametrize('sx,sw', SCALES)
@pytest.mark.parametrize('name,dtype,algo', _mag_params())
def test_split_magnitude_sweep(lib, cuda, name, dtype, algo, sx, sw):
    """Kernel against the storage model away from O(1) data.  Measured kernel-to-model distances: NOTES.md."""
    x, w, scale, bias, r, sim, truth, bound = _mag_ref(name, dtype, sx, sw)
    assert np.abs(x).max() < 65504 and np.isfinite(sim).all()   # preconditions, on the reference alone
    y = run_conv(lib, cuda, x, w, scale, bias, MAG_CASES[name][6], 0.1, dtype, residual=r, algo=algo, expect_rc=0)
    assert np.isfinite(y).all()
    smax = np.abs(sim).max()
    d, e = np.abs(y - sim), np.abs(y - truth)
    print('\nmagnitude %s %s a%d x*2^%d w*2^%d: max|y-sim|/max|sim| = %.3g, max |y-sim| / bar = %.3g, max |y-truth| / bound = %.3g, '
          'max|y-truth|/max|truth| = %.3g' % (name, dtype, algo, sx, sw, d.max() / smax,
                                              (d / (3e-5 * (np.abs(sim) + smax) + FLOOR[dtype])).max(), (e / bound).max(),
                                              e.max() / np.abs(truth).max()))
    assert (d <= 3e-5 * (np.abs(sim) + smax) + FLOOR[dtype]).all()
    assert (e <= bound).all()


@pytest.mark.parametrize('name,algo', [(n, a) for n in MAG_CASES for a in MAG_ALGOS[n]])
def test_bf16x3_is_scale_invariant(lib, cuda, name, algo):
    """bf16 pairs have fp32's exponent range: with bias 0 nothing under- or overflows at these scales, and every operation of the
    path commutes with a power of two -- y(x * 2^a, w * 2^b) == 2^(a + b) * y(x, w), value for value."""
    run = lambda sx, sw: run_conv(lib, cuda, *_mag_ref(name, 'bf16x3', sx, sw, True)[:4], MAG_CASES[name][6], 0.1, 'bf16x3',
                                  residual=_mag_ref(name, 'bf16x3', sx, sw, True)[4], algo=algo, expect_rc=0)
    base = run(0, 0)
    assert np.isfinite(base).all() and np.abs(base).max() > 1
    for sx, sw in SCALES[1:]:
        assert np.array_equal(run(sx, sw), np.ldexp(base, sx + sw)), (sx, sw)


# ---- A4: whole nets between moats ----------------------------------------------------------------------------------------------
def spec_ragged():
    """Pyramid levels of 16, 48 and 96 channels: the concat buffers' route halves are channels [16, 32) and [48, 96) -- the two
    tail slices of SLICES -- read by the next stage's down-sampling convolution."""
    return dict(layers=[1, 1, 1, 1], channels=[8, 16, 16, 48, 96], slice_point=[1, 3, 5, 6, 10], all_anchors=og.CAR_ANCHORS)


def _moated_net(**kw):
    from yolo_amd.net import CarNet

    class Moated(CarNet):
        """Every activation buffer of the plan from util.guarded: zeros inside, NaN directly before and behind."""
        def _act(self, N, H, W, Cc, *a, **k):
            t = super()._act(N, H, W, Cc, *a, **k)
            shape = tuple(t.shape[:-1]) + ((t.stride(3),) if t.dim() == 5 else (Cc,))      # (split: the whole padded planes)
            buf, full = guarded(shape, t.dtype, t.device)
            full.zero_()
            self.__dict__.setdefault('moats', []).append((buf, full, Cc))
            return full[..., :Cc]
    return Moated(**kw)


@functools.lru_cache(maxsize=None)
def _net_ref(which):
    spec = {'micro': og.spec_micro, 'ragged': spec_ragged}[which]()
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(3).random((2, 3, 64, 96), dtype=np.float32)
    num = lambda outs: [o.numpy() for o in outs]
    return spec, P, x, {'f32': num(of.forward_torch(g, P, x)), 'bf16': num(of.forward_torch_bf16sim(g, P, x)),
                        'f16': num(of.forward_torch_f16sim(g, P, x))}


@pytest.mark.parametrize('dtype', ['bf16x3', 'f16x3', 'f32', 'bf16', 'f16'])
@pytest.mark.parametrize('which', ['micro', 'ragged'])
def test_nets_between_moats(cuda, which, dtype):
    spec, P, x, refs = _net_ref(which)
    net = _moated_net(spec=spec, dtype=dtype, device=cuda).load_params(P)
    outs = [o.cpu().numpy() for o in net(torch.from_numpy(x).to(cuda))]
    torch.cuda.synchronize()
    assert net.moats
    for o in outs:                                              # (fine -> coarse; a NaN read from a moat names its pixels)
        assert not np.isnan(o).any(), 'NaN logits at (image, pixel) %s of the %d-pixel scale' % (
            sorted({(int(b), int(p)) for b, p in zip(*np.nonzero(np.isnan(o))[:2])})[:8], o.shape[1])
    for buf, full, _ in net.moats:
        guards_intact(buf, full)
    if dtype in SPLIT:
        assert {b.data_ptr() for b in net._last_plan.buffers} == {full.data_ptr() for _, full, _ in net.moats}
        padded = [(full, Cc) for _, full, Cc in net.moats if full.shape[-1] != Cc]
        assert padded
        for full, Cc in padded:                                 # the caller zeroes once, the kernels never write them
            assert bool((full[..., Cc:] == 0).all()), 'pad channels of a %s buffer were written' % (tuple(full.shape),)
    ref = refs['f32']
    for i, (o, r) in enumerate(zip(outs, ref)):
        if dtype in SPLIT:                                      # tests/test_gpu_split.py test_split_net_narrow_specs
            np.testing.assert_allclose(o, r, rtol=0, atol=1e-3 if dtype == 'bf16x3' else 5e-4)
        elif dtype == 'f32':                                    # tests/test_gpu_net.py test_micro_f32 / _bf16 / _f16
            np.testing.assert_allclose(o, r, rtol=0, atol=1e-3)
        else:
            np.testing.assert_allclose(o, refs[dtype][i], rtol=0, atol=2e-2 if dtype == 'bf16' else 3e-3)
            assert np.abs(o - r).max() < (5e-2 if dtype == 'bf16' else 8e-3)


@pytest.mark.parametrize('dtype', SPLIT)
def test_net_refuses_a_route_slice_whose_chunks_leave_the_pixel(cuda, dtype):
    """A concat buffer with planes of round_up(up + route, 32) only (what CarNet allocated before it knew about the chunks): the
    down-sampling convolution behind a 16- or 48-channel level would read into the next pixel -- refused when the plan is built."""
    from yolo_amd.net import CarNet

    class Narrow(CarNet):
        def _act(self, N, H, W, Cc, *a, **k):
            return super()._act(N, H, W, Cc)

    spec, P, x, _ = _net_ref('ragged')
    net = Narrow(spec, dtype=dtype, device=cuda).load_params(P)
    with pytest.raises(L.YoloError, match='pixel'):
        net(torch.from_numpy(x).to(cuda))
