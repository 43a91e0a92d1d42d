"""The convolution and stem kernels across the 2 GiB and 4 GiB offset lines (audit table: NOTES.md, "Offsets past 2^31").

Every other GPU test keeps its tensors under a few hundred MB, where none of this arithmetic is reached:
  (a) conv_epilogue.h has two complete forms; the branching 64-bit one runs only when y, the residual or the tail output spans
      2^31 bytes.  Here y is four small images 1.5 GiB apart (yolo_conv_desc.y_batch_stride): image offsets 0, 1.5, 3.0 and
      4.5 GiB -- below 2^31, in [2^31, 2^32) and past 2^32 -- in a buffer that is allocated but never filled (tests/util.py Islands);
  (b) the statistics epilogues and the fused tail on the same layout, and the tail's refusal at its 32-bit limit;
  (c) input offsets in [2^31, 2^32) through x_pixel_stride: the pixels of one 8 x 8 map 48 MiB apart, and what the library does
      with a 5 GiB x;
  (d) the fixed-layout kernels (stem, stem + down, residual block, stem + down + block, the streaming kernel, the sub-pixel data
      gradient) on dense outputs past 2^31 and past 2^32 bytes: N copies of one small image.
All images of a call get the same input, so every image of the output must equal image 0 bit for bit, image 0 is held against the
CPU reference at the tolerances of the small-tensor tests, and the strided call is held bit for bit against the dense one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from util import (GUARD_BYTES, Islands, guarded, guards_intact, moated, to_nhwc, from_nhwc, ref_conv, ref_conv_split, conv_variant,
                  LDT, TDT, SPLIT)
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu

STEP = 3 << 29                      # bytes between the images of a strided y: 1.5 GiB
ALL, FEW = ('bf16', 'f16', 'f32', 'bf16x3', 'f16x3'), ('bf16', 'f32', 'bf16x3')


def _es(dtype, out_f32=False):
    return 4 if (out_f32 or dtype == 'f32') else 2


def _out_hw(case):
    N, Cin, H, W, Cout, k, stride = case
    pad = k // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=None)
def _host(case):
    """Operands of ONE image (every image of a call gets them): x (1,Cin,H,W), w, scale, bias, residual (1,Cout,Ho,Wo)."""
    N, Cin, H, W, Cout, k, stride = case
    rng = np.random.default_rng(1000 * Cin + 10 * H + k + stride + Cout)
    x = rng.standard_normal((1, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    bias = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    r = rng.standard_normal((1, Cout) + _out_hw(case)).astype(np.float32)
    return x, w, scale, bias, r


@functools.lru_cache(maxsize=None)
def _reference(case, dtype, res, ident, out_f32):
    """-> (restated split arithmetic or None, oracle) of one image, computed once and shared by the variants."""
    x, w, scale, bias, r = _host(case)
    stride, slope = case[6], (1.0 if ident else 0.1)
    if ident:
        scale, bias = np.ones_like(scale), np.zeros_like(bias)
    r = r if res else None
    if dtype in SPLIT:
        return (ref_conv_split(x, w, scale, bias, stride, slope, residual=r, rdt=TDT[dtype], out_f32=out_f32),
                ref_conv(x, w, scale, bias, stride, slope, residual=r))
    if dtype == 'f32':
        return None, ref_conv(x, w, scale, bias, stride, slope, residual=r)
    if out_f32:                                 # fp32 logits of 2-byte operands: only the operands are rounded
        rb = lambda a: torch.from_numpy(a).to(TDT[dtype]).float().numpy()
        return None, ref_conv(rb(x), rb(w), scale, bias, stride, slope)
    return None, ref_conv(x, w, scale, bias, stride, slope, residual=r, bf16=(True if dtype == 'bf16' else 'f16'))


def _check_image(y, dtype, out_f32, refs, what=''):
    """One image (NCHW fp32 values) against the reference at the tolerances of test_gpu_conv.py / test_gpu_split.py."""
    sim, ref = refs
    assert not np.isnan(y).any(), what
    if dtype in SPLIT:
        np.testing.assert_allclose(y, sim, rtol=3e-5, atol=3e-5, err_msg=what)
        tol = 2e-4 if dtype == 'bf16x3' else 3e-5
        np.testing.assert_allclose(y, ref, rtol=tol, atol=tol, err_msg=what)
    elif dtype == 'f32' or out_f32:
        np.testing.assert_allclose(y, ref, rtol=1e-4, atol=1e-4, err_msg=what)
    elif dtype == 'f16':
        np.testing.assert_allclose(y, ref, rtol=2e-3, atol=2e-3, err_msg=what)
        assert np.mean(np.abs(y - ref) > 2e-4 * (1 + np.abs(ref))) < 0.02, what
    else:
        np.testing.assert_allclose(y, ref, rtol=1.6e-2, atol=2e-2, err_msg=what)
        assert np.mean(np.abs(y - ref) > 1e-3 * (1 + np.abs(ref))) < 0.02, what


class _Ops:
    """The device operands of a conv case, every image the same: x and the residual dense in moats, the packed weights between
    guards."""

    def __init__(self, lib, dev, case, dtype, res=False, ident=False):
        N, Cin, H, W, Cout, k, stride = case
        x, w, scale, bias, r = _host(case)
        self.lib, self.dev, self.case, self.dtype = lib, dev, case, dtype
        self.st = torch.cuda.current_stream().cuda_stream
        dt = LDT[dtype]
        self.x = moated(to_nhwc(np.repeat(x, N, axis=0), dtype, dev))
        self.wbuf, self.wp = guarded((lib.yolo_packed_weight_bytes(Cout, Cin, k, dt),), torch.uint8, dev)
        L.check(lib.yolo_pack_conv_weights(moated(torch.from_numpy(w).to(dev)).data_ptr(), self.wp.data_ptr(), Cout, Cin, k, dt, self.st), 'pack')
        self.sc = self.bi = None
        if not ident:
            cp = lib.yolo_padded_channels(Cout)
            sc = torch.zeros(cp, device=dev); sc[:Cout] = torch.from_numpy(scale).to(dev)
            bi = torch.zeros(cp, device=dev); bi[:Cout] = torch.from_numpy(bias).to(dev)
            self.sc, self.bi = moated(sc), moated(bi)
        self.slope = 1.0 if ident else 0.1
        self.res = moated(to_nhwc(np.repeat(r, N, axis=0), dtype, dev)) if res else None

    def desc(self, algo, y_ptr, **fields):
        N, Cin, H, W, Cout, k, stride = self.case
        d = L.ConvDesc()
        d.x, d.w_packed, d.y = self.x.data_ptr(), self.wp.data_ptr(), y_ptr
        d.scale, d.bias = (self.sc.data_ptr(), self.bi.data_ptr()) if self.sc is not None else (None, None)
        d.residual = self.res.data_ptr() if self.res is not None else None
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = N, H, W, Cin, Cout, k, stride
        d.dtype, d.slope, d.algo = LDT[self.dtype], self.slope, algo
        for f, v in fields.items():
            setattr(d, f, v)
        return d

    def run(self, algo, y_ptr, expect=0, **fields):
        rc = self.lib.yolo_conv_fwd(C.byref(self.desc(algo, y_ptr, **fields)), self.st)
        assert rc == expect, 'yolo_conv_fwd rc=%d, expected %d' % (rc, expect)
        torch.cuda.synchronize()
        guards_intact(self.wbuf, self.wp)


def _img_shape(case, dtype, out_f32=False, up2=False):
    Cout, (Ho, Wo), m = case[4], _out_hw(case), (2 if up2 else 1)
    if dtype in SPLIT and not out_f32:
        return (m * Ho, m * Wo, 2, -(-Cout // 32) * 32)
    return (m * Ho, m * Wo, Cout)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _values(img, Cout, up2=False):
    """One NHWC image (split: (H, W, 2, Cp), its pad channels still the poison) -> NCHW fp32 values, a 2x2 up-sampled one reduced to its
    source pixels after checking that the four copies agree."""
    if img.dim() == 4:
        assert bool(torch.isnan(img[..., Cout:].float()).all()), 'the pad channels of a split plane were written'
        img = img[..., :Cout]
    if up2:
        for dy, dx in ((0, 1), (1, 0), (1, 1)):
            assert torch.equal(_bits(img[dy::2, dx::2].contiguous()), _bits(img[0::2, 0::2].contiguous())), 'the 2x2 patch differs'
        img = img[0::2, 0::2]
    return from_nhwc(img.unsqueeze(0))


# ---- (a) the branching form of the epilogue ---------------------------------------------------------------------------------------
FLAGS = {'plain': {}, 'res': dict(res=True), 'ident_res': dict(res=True, ident=True), 'ident': dict(ident=True),
         'up2': dict(up2=True), 'out_f32': dict(out_f32=True)}
K3, K3B, X8 = (4, 128, 13, 13, 256, 3, 1), (4, 64, 26, 26, 128, 3, 1), (4, 128, 8, 8, 256, 3, 1)      # (8 x 8: every tile crosses images)
K1, K1B, X8K1 = (4, 256, 13, 13, 128, 1, 1), (4, 128, 26, 26, 256, 1, 1), (4, 256, 8, 8, 256, 1, 1)
S2 = (4, 64, 26, 26, 128, 3, 2)
K3_90, K1_90 = K3[:4] + (90,) + K3[5:], K1[:4] + (90,) + K1[5:]                                         # (head logits: rows of 360 bytes)
# one variant per epilogue instantiation: the generic kernel, a 4-wave and an 8-wave 3x3 tile, a 1x1 tile of each group
# (2-12 | 19-21, 36-39 | 22-25), a stride-2 tile, a split-K tile
A3, A1, AS2 = (1, 4, 2), (1, 11, 19, 22, 30), (1, 9)


def _strided_fields(case, dtype, step, res=False, ident=False, up2=False, out_f32=False):
    f = dict(y_batch_stride=step // _es(dtype, out_f32))
    if up2:
        f['upsample2x'] = 1
    if out_f32:
        f['out_f32'] = 1
    return f


def _a_params(groups, step):
    out = []
    for case, dtypes, algos, flags in groups:
        for dtype in dtypes:
            for algo in algos:
                for flag in flags:
                    kw = FLAGS[flag]
                    if conv_variant(case, dtype, algo, residual=bool(kw.get('res')), fields=_strided_fields(case, dtype, step, **kw)) is not None:
                        out.append(pytest.param(case, dtype, algo, flag, id='%s-%s-a%d-%s' % ('x'.join(map(str, case)), dtype, algo, flag)))
    return out


A_GROUPS = [(K3, ALL, A3, ('res', 'up2')), (K3, FEW, A3, ('plain', 'ident_res')), (K3_90, FEW, (1, 2), ('out_f32',)),
            (K3B, FEW, A3, ('res',)), (X8, FEW, A3, ('res',)),
            (K1, ALL, A1, ('res', 'up2')), (K1, FEW, A1, ('ident_res',)), (K1_90, FEW, (1, 11), ('out_f32',)),
            (K1B, FEW, A1[1:], ('res',)), (X8K1, FEW, (1, 11, 30), ('res',)),
            (S2, ALL, AS2, ('plain',)), (S2, FEW, AS2, ('ident',))]


def _strided_against_dense(lib, dev, case, dtype, algo, flag, step):
    kw = FLAGS[flag]
    res, ident, up2, out_f32 = (bool(kw.get(k)) for k in ('res', 'ident', 'up2', 'out_f32'))
    N, Cout = case[0], case[4]
    ops = _Ops(lib, dev, case, dtype, res=res, ident=ident)
    shape, tdt = _img_shape(case, dtype, out_f32, up2), (torch.float32 if out_f32 else TDT[dtype])
    fields = _strided_fields(case, dtype, step, **kw)
    dbuf, dense = guarded((N,) + shape, tdt, dev)                         # the same call made densely
    ops.run(algo, dense.data_ptr(), **{k: v for k, v in fields.items() if k != 'y_batch_stride'})
    guards_intact(dbuf, dense)
    isl = Islands(N, dense[0].numel() * dense.element_size(), step, dev)
    y = isl.view(shape, tdt)
    ops.run(algo, isl.data_ptr(), **fields)
    isl.intact()
    for i in range(1, N):
        assert torch.equal(_bits(y[i]), _bits(y[0])), 'image %d (at %.2f GiB) differs from image 0' % (i, i * step / 2.0 ** 30)
    differ = sum(int((_bits(y[i]) != _bits(dense[i])).sum()) for i in range(N))
    print('%s %s algo %d %s: %d of %d stored elements differ from the dense call' % (case, dtype, algo, flag, differ, dense.numel()))
    _check_image(_values(y[0], Cout, up2), dtype, out_f32, _reference(case, dtype, res, ident, out_f32), 'image 0')
    assert differ == 0, '%d stored elements differ from the dense call' % differ
    del isl, y, dense, dbuf, ops


@pytest.mark.parametrize('case,dtype,algo,flag', _a_params(A_GROUPS, STEP))
def test_epilogue_branching_form(lib, cuda, case, dtype, algo, flag):
    """y spans 6 GiB (buf32 == 0): the branching 64-bit epilogue with its own residual, lo-plane, up-sampling and fp32 stores.  The
    four images equal each other, image 0 the reference, every band around every image is intact, and the whole equals the dense call
    (the buffer form) bit for bit.  (Measured on an MI355X: 0 differing elements in every case -- the two forms compile the same
    arithmetic; nothing had to be allowed for FMA contraction.)"""
    _strided_against_dense(lib, cuda, case, dtype, algo, flag, STEP)


UNDER = ((1 << 31) - 256) // 4      # four images whose extent stays 256 bytes under 2^31: the last byte offsets of the buffer form
U_GROUPS = [(K3, FEW, (1, 2), ('res',)), (K1, FEW, (11,), ('up2',)), (K1_90, ('bf16',), (1,), ('out_f32',))]


@pytest.mark.parametrize('case,dtype,algo,flag', _a_params(U_GROUPS, UNDER))
def test_epilogue_buffer_form_just_under_2gib(lib, cuda, case, dtype, algo, flag):
    """The other side of the threshold in conv_dispatch: an extent of 2^31 - 256 bytes still takes the buffer form, whose int byte
    offsets then reach their largest values."""
    assert 4 * UNDER < 0x7fffffff and UNDER % 16 == 0
    _strided_against_dense(lib, cuda, case, dtype, algo, flag, UNDER)


# ---- (b) statistics and the fused tail under the branching form -------------------------------------------------------------------
B3, B1, BS2 = (2, 64, 13, 13, 128, 3, 1), (2, 256, 26, 26, 256, 1, 1), (2, 64, 26, 26, 128, 3, 2)
B_PARAMS = [pytest.param(c, a, m, id='%s-a%d-m%d' % ('x'.join(map(str, c)), a, m))
            for c, algos in ((B3, (1, 2, 4, 6)), (B1, (1, 11, 19, 22)), (BS2, (1, 9))) for a in algos for m in (1, 2)
            if conv_variant(c, 'bf16', a, stats_mode=m, fields=dict(y_batch_stride=STEP // 2)) is not None]


@pytest.mark.parametrize('case,algo,mode', B_PARAMS)
def test_statistics_branching_form(lib, cuda, case, algo, mode):
    """The checks of test_conv_statistics_epilogue with y (and, mode 2, stats_y, which shares y's offsets) as two images 1.5 GiB
    apart: 3 GiB, the branching form.  The BatchNorm fed by the partial rows equals the one that reduces the stored tensor, and the
    stored tensor equals the dense call's."""
    N, Cin, H, W, Cout, k, stride = case
    (Ho, Wo), dev = _out_hw(case), cuda
    ops = _Ops(lib, dev, case, 'bf16', ident=True)
    st, cp, npix = ops.st, lib.yolo_padded_channels(Cout), N * Ho * Wo
    rng = np.random.default_rng(7)
    gamma = torch.from_numpy(rng.uniform(.5, 1.5, Cout).astype(np.float32)).to(dev)
    beta = torch.from_numpy((0.2 * rng.standard_normal(Cout)).astype(np.float32)).to(dev)
    shape = (Ho, Wo, Cout)
    isl = Islands(N, Ho * Wo * Cout * 2, STEP, dev)
    y = isl.view(shape, torch.bfloat16)
    dbuf, dense = guarded((N,) + shape, torch.bfloat16, dev)
    ws = [torch.zeros(2 * Cout, dtype=torch.float64, device=dev) for _ in range(4)]
    mk = lambda: (torch.empty(Cout, device=dev), torch.empty(Cout, device=dev))
    fields = dict(stats=1, stats_mode=mode)
    isl_s = None
    if mode == 2:
        yb1 = torch.from_numpy(rng.standard_normal((1,) + shape).astype(np.float32)).to(dev).bfloat16()
        yb = yb1.expand(N, -1, -1, -1).contiguous()
        acc0 = torch.from_numpy((0.5 * rng.standard_normal((1,) + shape)).astype(np.float32)).to(dev).bfloat16()
        ops.res = moated(acc0.expand(N, -1, -1, -1).contiguous())         # the existing gradient: dense, y strided
        mean = yb.float().mean(dim=(0, 1, 2)).contiguous()
        invstd = (1.0 / torch.sqrt(yb.float().var(dim=(0, 1, 2), unbiased=False) + 1e-5)).contiguous()
        isl_s = Islands(N, Ho * Wo * Cout * 2, STEP, dev)
        isl_s.view(shape, torch.bfloat16).copy_(yb)
        fields.update(stats_mean=mean.data_ptr(), stats_invstd=invstd.data_ptr(), stats_gamma=gamma.data_ptr(),
                      stats_beta=beta.data_ptr(), stats_slope=0.1)
    rows = lib.yolo_conv_stats_rows(C.byref(ops.desc(algo, isl.data_ptr(), y_batch_stride=STEP // 2, stats_y=(isl_s.data_ptr() if isl_s else None), **fields)))
    assert rows > 0
    part = torch.full((rows, 2, cp), float('nan'), device=dev)
    part_d = torch.full((rows, 2, cp), float('nan'), device=dev)
    fields['stats'] = part_d.data_ptr()
    ops.run(algo, dense.data_ptr(), stats_y=(yb.data_ptr() if mode == 2 else None), **fields)
    guards_intact(dbuf, dense)
    fields['stats'] = part.data_ptr()
    ops.run(algo, isl.data_ptr(), y_batch_stride=STEP // 2, stats_y=(isl_s.data_ptr() if isl_s else None), **fields)
    isl.intact()
    yc = y.contiguous()
    assert bool(torch.isfinite(yc.float()).all())
    assert torch.equal(_bits(yc), _bits(dense)), 'the stored tensor differs from the dense call'
    for i in range(1, N):
        assert torch.equal(_bits(yc[i]), _bits(yc[0]))
    if mode == 1:
        (m1, i1), (m2, i2) = mk(), mk()
        z1, z2 = torch.empty_like(yc), torch.empty_like(yc)
        rm, rv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
        assert lib.yolo_bn_train_fwd_partials(part.data_ptr(), rows, cp, yc.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None,
                                              z1.data_ptr(), m1.data_ptr(), i1.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                              ws[0].data_ptr(), ws[1].data_ptr(), 2 * Cout, npix, Cout, 1e-5, 0.9, 0.1, L.BF16, st) == 0
        assert lib.yolo_bn_train_fwd_pp(yc.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, z2.data_ptr(), m2.data_ptr(),
                                        i2.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[2].data_ptr(), ws[3].data_ptr(), 2 * Cout,
                                        npix, Cout, 1e-5, 0.9, 0.1, L.BF16, st) == 0
        torch.cuda.synchronize()
        np.testing.assert_allclose(m1.cpu().numpy(), m2.cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(i1.cpu().numpy(), i2.cpu().numpy(), rtol=1e-5)
        assert float((z1.float() - z2.float()).abs().max()) <= 1e-2 * float(z2.float().abs().max())
    else:
        isl_s.intact()
        dy1, dy2 = torch.empty_like(yc), torch.empty_like(yc)
        (g1, b1), (g2, b2) = mk(), mk()
        assert lib.yolo_bn_train_bwd_partials(part.data_ptr(), rows, cp, yc.data_ptr(), yb.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                              gamma.data_ptr(), beta.data_ptr(), dy1.data_ptr(), g1.data_ptr(), b1.data_ptr(),
                                              ws[0].data_ptr(), ws[1].data_ptr(), 2 * Cout, npix, Cout, 0.1, L.BF16, st) == 0
        assert lib.yolo_bn_train_bwd_pp(yc.data_ptr(), yb.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                        beta.data_ptr(), dy2.data_ptr(), g2.data_ptr(), b2.data_ptr(), ws[2].data_ptr(),
                                        ws[3].data_ptr(), 2 * Cout, npix, Cout, 0.1, L.BF16, st) == 0
        torch.cuda.synchronize()
        sc = float(g2.abs().max()) + float(b2.abs().max())
        np.testing.assert_allclose(g1.cpu().numpy(), g2.cpu().numpy(), rtol=1e-4, atol=1e-5 * sc)
        np.testing.assert_allclose(b1.cpu().numpy(), b2.cpu().numpy(), rtol=1e-4, atol=1e-5 * sc)
        assert float((dy1.float() - dy2.float()).abs().max()) <= 1e-2 * float(dy2.float().abs().max())
    del isl, isl_s, y, ops


# (N, Cin, H, W, Cout, stride, residual, tail_cout, tail fp32)
T_CASES = [((2, 128, 26, 26, 256, 1, True, 128, False), (0, 2, 6)), ((2, 64, 26, 26, 128, 2, False, 64, False), (9, 17)),
           ((2, 128, 13, 13, 256, 1, False, 90, True), (2,)), ((2, 64, 8, 8, 128, 1, True, 64, False), (7,))]


class _Tail:
    """Operands of a 3x3 convolution with a fused tail 1x1 (as test_conv_tail_1x1_fused_is_bit_identical builds them)."""

    def __init__(self, lib, dev, tcase):
        N, Cin, H, W, Cout, stride, with_res, tcout, tf32 = tcase
        self.case = (N, Cin, H, W, Cout, 3, stride)
        self.ops = _Ops(lib, dev, self.case, 'bf16', res=with_res)
        rng = np.random.default_rng(31)
        self.w1 = (rng.standard_normal((tcout, Cout, 1, 1)) / np.sqrt(Cout)).astype(np.float32)
        self.wp1 = torch.empty(lib.yolo_packed_weight_bytes(tcout, Cout, 1, L.BF16), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_pack_conv_weights(torch.from_numpy(self.w1).to(dev).data_ptr(), self.wp1.data_ptr(), tcout, Cout, 1, L.BF16, self.ops.st), 'pack')
        cp = lib.yolo_padded_channels(tcout)
        self.sc1, self.bi1 = torch.zeros(cp, device=dev), torch.zeros(cp, device=dev)
        self.sc1[:tcout] = torch.from_numpy(rng.uniform(.5, 1.5, tcout).astype(np.float32)).to(dev)
        self.bi1[:tcout] = torch.from_numpy((0.1 * rng.standard_normal(tcout)).astype(np.float32)).to(dev)
        self.tcout, self.tf32, self.tslope = tcout, tf32, (1.0 if tf32 else 0.1)

    def fields(self, z_ptr, **more):
        return dict(tail_w_packed=self.wp1.data_ptr(), tail_scale=self.sc1.data_ptr(), tail_bias=self.bi1.data_ptr(), tail_y=z_ptr,
                    tail_cout=self.tcout, tail_out_f32=int(self.tf32), tail_slope=self.tslope, **more)


@pytest.mark.parametrize('tcase,algo', [pytest.param(c, a, id='%s-a%d' % ('x'.join(str(int(v)) for v in c), a)) for c, algos in T_CASES for a in algos])
def test_tail_branching_form(lib, cuda, tcase, algo):
    """The checks of test_conv_tail_1x1_fused_is_bit_identical with y and tail_y as two images 1.5 GiB apart: the main output and
    the tail of the fused call equal, bit for bit, the two separate dense launches; the tail reads y back through 32-bit offsets that
    reach 1.5 GiB here."""
    dev = cuda
    t = _Tail(lib, dev, tcase)
    N, Cout, (Ho, Wo), ops = tcase[0], tcase[4], _out_hw(t.case), t.ops
    zdt = torch.float32 if t.tf32 else torch.bfloat16
    zes = 4 if t.tf32 else 2
    # the two separate launches, dense (the same tile variant: kernel families differ in their K order)
    y0 = torch.full((N, Ho, Wo, Cout), float('nan'), dtype=torch.bfloat16, device=dev)
    z0 = torch.full((N, Ho, Wo, t.tcout), float('nan'), dtype=zdt, device=dev)
    stride = tcase[5]
    for cand in ([algo] if algo else (([17, 9] if Cout <= 128 else []) + [18, 16, 10] if stride == 2 else ([7] if Cout <= 128 else []) + [6, 2])):
        if lib.yolo_conv_fwd(C.byref(ops.desc(cand, y0.data_ptr())), ops.st) == 0:
            break
    else:
        raise AssertionError('no 256-cout variant takes the plain convolution')
    d1 = L.ConvDesc()
    d1.x, d1.w_packed, d1.scale, d1.bias, d1.y = y0.data_ptr(), t.wp1.data_ptr(), t.sc1.data_ptr(), t.bi1.data_ptr(), z0.data_ptr()
    d1.N, d1.H, d1.W, d1.Cin, d1.Cout, d1.ksize, d1.stride, d1.dtype = N, Ho, Wo, Cout, t.tcout, 1, 1, L.BF16
    d1.out_f32, d1.slope = int(t.tf32), t.tslope
    assert lib.yolo_conv_fwd(C.byref(d1), ops.st) == 0
    # the fused call on the strided layout
    isl_y, isl_z = Islands(N, Ho * Wo * Cout * 2, STEP, dev), Islands(N, Ho * Wo * t.tcout * zes, STEP, dev)
    ops.run(algo, isl_y.data_ptr(), **t.fields(isl_z.data_ptr(), y_batch_stride=STEP // 2, tail_y_batch_stride=STEP // zes))
    isl_y.intact()
    isl_z.intact()
    y1, z1 = isl_y.view((Ho, Wo, Cout), torch.bfloat16).contiguous(), isl_z.view((Ho, Wo, t.tcout), zdt).contiguous()
    assert not torch.isnan(y1.float()).any() and not torch.isnan(z1.float()).any()
    assert torch.equal(_bits(y0), _bits(y1)) and torch.equal(_bits(z0), _bits(z1))
    for i in range(1, N):
        assert torch.equal(_bits(z1[i]), _bits(z1[0]))
    yin = y1.float().permute(0, 3, 1, 2).cpu()
    ref = torch.nn.functional.conv2d(yin, torch.from_numpy(t.w1).to(torch.bfloat16).float())
    ref = ref * t.sc1[:t.tcout].cpu().view(1, -1, 1, 1) + t.bi1[:t.tcout].cpu().view(1, -1, 1, 1)
    if not t.tf32:
        ref = torch.where(ref > 0, ref, ref * 0.1).to(torch.bfloat16).float()
    np.testing.assert_allclose(z1.float().permute(0, 3, 1, 2).cpu().numpy(), ref.numpy(), rtol=1.6e-2, atol=2e-2)
    del isl_y, isl_z, t, ops


@pytest.mark.parametrize('algo', [2, 6, 0])
def test_tail_refused_at_its_32bit_limit(lib, cuda, algo):
    """N * y_batch_stride * 2 == 0xffffff00: the tail's read-back offsets would reach the marker of a padding slot.  Refused with
    YOLO_EUNSUPPORTED and nothing written; eight elements of stride less are taken (tests/test_host.py), which is 3 GiB below
    what test_tail_branching_form runs."""
    t = _Tail(lib, cuda, (2, 128, 13, 13, 256, 1, False, 128, False))
    step = 0xffffff00 // 2
    isl_y = Islands(2, 13 * 13 * 256 * 2, step, cuda)
    zbuf, z = guarded((2, 13, 13, 128), torch.bfloat16, cuda)
    t.ops.run(algo, isl_y.data_ptr(), expect=L.EUNSUPPORTED, **t.fields(z.data_ptr(), y_batch_stride=step // 2))
    isl_y.intact()
    guards_intact(zbuf, z)
    assert bool((isl_y.region(0) == 0xFF).all()) and bool((isl_y.region(1) == 0xFF).all()) and bool(torch.isnan(z.float()).all())
    del isl_y


# ---- (c) input offsets through x_pixel_stride -----------------------------------------------------------------------------------
PITCH, PITCH5 = 48 << 20, 80 << 20            # 64 pixels: 3 GiB (pixels 43.. lie in [2^31, 2^32)) and 5 GiB
C_CASES = [(1, 64, 8, 8, 128, 3, 1), (1, 128, 8, 8, 128, 3, 1), (1, 64, 8, 8, 128, 1, 1), (1, 128, 8, 8, 128, 1, 1)]
C_ALGOS = (1, 4, 11, 30, 32)                  # generic, a 3x3 tile, a 1x1 tile, split-K
C_PARAMS = [pytest.param(c, dt, a, id='%s-%s-a%d' % ('x'.join(map(str, c)), dt, a)) for c in C_CASES for dt in ('bf16', 'f32') for a in C_ALGOS
            if conv_variant(c, dt, a, fields=dict(x_pixel_stride=PITCH // _es(dt))) is not None]


def _pixels_apart(ops, pitch):
    """The case's one input image with its pixels `pitch` bytes apart, NaN in GUARD_BYTES before and behind each pixel's channels."""
    Cin, tdt = ops.case[1], TDT[ops.dtype]
    isl = Islands(ops.x[0].numel() // Cin, Cin * ops.x.element_size(), pitch, ops.dev)
    isl.view((Cin,), tdt).copy_(ops.x.reshape(-1, Cin))
    return isl


@pytest.mark.parametrize('case,dtype,algo', C_PARAMS)
def test_input_pixels_48mib_apart(lib, cuda, case, dtype, algo):
    """x_pixel_stride = 48 MiB: the input offsets of pixels 43 .. 63 lie in [2^31, 2^32), where conv_pipe / conv_sk keep them as
    unsigned and a sign extension would show.  Bit for bit the dense call, and the reference."""
    ops = _Ops(lib, cuda, case, dtype)
    shape = _img_shape(case, dtype)
    dbuf, dense = guarded((1,) + shape, TDT[dtype], cuda)
    ops.run(algo, dense.data_ptr())
    guards_intact(dbuf, dense)
    xin = _pixels_apart(ops, PITCH)
    assert 43 * PITCH >= 1 << 31 > 42 * PITCH and 64 * PITCH < 0xffffff00
    ybuf, y = guarded((1,) + shape, TDT[dtype], cuda)
    ops.x = xin.view((case[1],), TDT[dtype])            # (desc() takes its data_ptr)
    ops.run(algo, y.data_ptr(), x_pixel_stride=PITCH // _es(dtype))
    guards_intact(ybuf, y)
    xin.intact()
    _check_image(_values(y[0], case[4]), dtype, False, _reference(case, dtype, False, False, False))
    assert torch.equal(_bits(y), _bits(dense))
    del xin, ops


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('case', C_CASES)
def test_input_extent_of_5gib(lib, cuda, case, dtype):
    """x_pixel_stride = 80 MiB, an extent of 5 GiB: conv_pipe and conv_sk refuse (32-bit offsets) and write nothing; algo 0 falls
    through to the generic kernel, whose offsets are 64-bit, and computes what it computes on the dense input."""
    ops = _Ops(lib, cuda, case, dtype)
    shape = _img_shape(case, dtype)
    dbuf, dense = guarded((1,) + shape, TDT[dtype], cuda)
    ops.run(1, dense.data_ptr())
    xin = _pixels_apart(ops, PITCH5)
    ops.x = xin.view((case[1],), TDT[dtype])
    ps = PITCH5 // _es(dtype)
    ybuf, y = guarded((1,) + shape, TDT[dtype], cuda)
    refused = 0
    for algo in (2, 4, 6, 11, 19, 22, 30, 32):
        if conv_variant(case, dtype, algo, fields=dict(x_pixel_stride=PITCH // _es(dtype))) is None:
            continue                                    # (not a variant for this shape at any pitch)
        assert conv_variant(case, dtype, algo, fields=dict(x_pixel_stride=ps)) is None
        ops.run(algo, y.data_ptr(), expect=L.EUNSUPPORTED, x_pixel_stride=ps)
        refused += 1
    assert refused >= 2 and bool(torch.isnan(y.float()).all())
    name = conv_variant(case, dtype, 0, fields=dict(x_pixel_stride=ps))
    assert name is not None and 'conv_igemm_kernel' in name, name
    ops.run(0, y.data_ptr(), x_pixel_stride=ps)
    guards_intact(ybuf, y)
    xin.intact()
    _check_image(_values(y[0], case[4]), dtype, False, _reference(case, dtype, False, False, False))
    assert torch.equal(_bits(y), _bits(dense))
    del xin, ops


# ---- (d) the fixed-layout kernels on dense outputs past 2^31 and 2^32 bytes -------------------------------------------------------
# N copies of one small image, the smallest N whose OUTPUT crosses the line.  These kernels address through a 64-bit base per row
# or tile plus offsets of at most a few rows (the audit table), so nothing here is refused; their host checks cap grids only.
LINES = [31, 32]


def _copies_past(line, image_bytes):
    return (1 << line) // image_bytes + 1


def _copies(one, N):
    """(1, ...) -> N dense copies."""
    return one.expand(N, *one.shape[1:]).contiguous()


def _every_image_equals_the_first(y, what):
    N = y.shape[0]
    flat = _bits(y.view(N, -1))
    per = max(1, (256 << 20) // (flat.shape[1] * flat.element_size()))
    for i in range(0, N, per):
        same = (flat[i:i + per] == flat[0:1]).all(dim=1)
        if not bool(same.all()):
            n = i + int((~same).nonzero()[0])
            raise AssertionError('%s: image %d of %d (byte offset %d) differs from image 0' % (what, n, N, n * flat.shape[1] * flat.element_size()))


def _first_stage(lib, dev, dtype='bf16'):
    from test_gpu_bounds import _first_stage as fs
    return fs(lib, dev, dtype)


def _dp(d, *names):
    return tuple(d[n].data_ptr() for n in names)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _image(H, W, dev, seed):
    x = np.random.default_rng(seed).random((1, 3, H, W), dtype=np.float32)
    return x, torch.from_numpy(x).to(dev)


@pytest.mark.parametrize('dtype,line', [('bf16', 31), ('bf16', 32), ('bf16x3', 31)])
def test_stem_past_the_line(lib, cuda, dtype, line):
    """yolo_stem_conv_fwd on copies of one 37 x 61 image (ragged tiles on both sides) whose output passes 2^31 / 2^32 bytes."""
    H, W = 37, 61
    p, d = _first_stage(lib, cuda)
    x, x1 = _image(H, W, cuda, 5)
    shape = (H, W, 32) if dtype == 'bf16' else (H, W, 2, 32)
    N = _copies_past(line, int(np.prod(shape)) * 2)
    xd = _copies(x1, N)
    ybuf, y = guarded((N,) + shape, TDT[dtype], cuda)
    assert y.numel() * 2 > 1 << line
    assert lib.yolo_stem_conv_fwd(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0'), y.data_ptr(), N, H, W, 3, 32, LDT[dtype], 0.1, _st()) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    _every_image_equals_the_first(y, 'stem')
    got = from_nhwc(y[:1])
    if dtype == 'bf16':
        np.testing.assert_allclose(got, ref_conv(x, p['w0'], p['s0'], p['b0'], 1, 0.1, bf16=True), rtol=1.6e-2, atol=2e-2)
    else:
        np.testing.assert_allclose(got, ref_conv(x, p['w0'], p['s0'], p['b0'], 1, 0.1), rtol=2e-5, atol=2e-5)
    del xd, y, ybuf


@pytest.mark.parametrize('line', LINES)
def test_stem_statistics_past_the_line(lib, cuda, line):
    """yolo_stem_conv_fwd_stats likewise: the stored map is yolo_stem_conv_fwd's, every image's partial rows are image 0's, those sum
    to the stored image's sums, and (2^31: three such tensors fit the budget) the BatchNorm fed by the rows equals the one that
    reduces the tensor, as in test_stem_statistics."""
    H, W, Cout = 37, 61, 32
    p, d = _first_stage(lib, cuda)
    x, x1 = _image(H, W, cuda, 6)
    N = _copies_past(line, H * W * Cout * 2)
    xd = _copies(x1, N)
    rows = lib.yolo_stem_stats_rows(N, H, W, Cout)
    assert rows > 0 and rows % N == 0
    ybuf, y = guarded((N, H, W, Cout), torch.bfloat16, cuda)
    pbuf, part = guarded((rows, 2, Cout), torch.float32, cuda)
    st = _st()
    assert lib.yolo_stem_conv_fwd_stats(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0'), y.data_ptr(), N, H, W, 3, Cout, L.BF16, 0.1, part.data_ptr(), st) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    guards_intact(pbuf, part)
    _every_image_equals_the_first(y, 'stem + statistics')
    one = torch.empty((1, H, W, Cout), dtype=torch.bfloat16, device=cuda)
    assert lib.yolo_stem_conv_fwd(x1.data_ptr(), *_dp(d, 'w0', 's0', 'b0'), one.data_ptr(), 1, H, W, 3, Cout, L.BF16, 0.1, st) == 0
    assert torch.equal(_bits(one), _bits(y[:1]))
    np.testing.assert_allclose(from_nhwc(one), ref_conv(x, p['w0'], p['s0'], p['b0'], 1, 0.1, bf16=True), rtol=1.6e-2, atol=2e-2)
    assert bool(torch.isfinite(part).all())
    _every_image_equals_the_first(part.view(N, -1), 'partial rows')
    # fp32 partial sums of at most H W values each: n 2^-24 sum|v| bounds any summation order (test_gpu_bounds.py test_stem_kernels)
    v = one.double().reshape(-1, Cout)
    eps = v.shape[0] * 2.0 ** -24
    s = part.view(N, -1, 2, Cout)[0].double().sum(dim=0)
    assert bool(((s[0] - v.sum(dim=0)).abs() <= eps * v.abs().sum(dim=0) + 1e-30).all())
    assert bool(((s[1] - (v * v).sum(dim=0)).abs() <= 2 * eps * (v * v).sum(dim=0) + 1e-30).all())
    if line == 31:
        gamma, beta = torch.rand(Cout, device=cuda) + .5, torch.randn(Cout, device=cuda) * .1
        ws = [torch.zeros(2 * Cout, dtype=torch.float64, device=cuda) for _ in range(4)]
        m1, i1, m2, i2 = (torch.empty(Cout, device=cuda) for _ in range(4))
        z1, z2 = torch.empty_like(y), torch.empty_like(y)
        rm, rv = torch.zeros(Cout, device=cuda), torch.ones(Cout, device=cuda)
        npix = N * H * W
        assert lib.yolo_bn_train_fwd_partials(part.data_ptr(), rows, Cout, y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None,
                                              z1.data_ptr(), m1.data_ptr(), i1.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[0].data_ptr(),
                                              ws[1].data_ptr(), 2 * Cout, npix, Cout, 1e-5, 0.9, 0.1, L.BF16, st) == 0
        assert lib.yolo_bn_train_fwd_pp(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, z2.data_ptr(), m2.data_ptr(),
                                        i2.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[2].data_ptr(), ws[3].data_ptr(), 2 * Cout, npix,
                                        Cout, 1e-5, 0.9, 0.1, L.BF16, st) == 0
        torch.cuda.synchronize()
        np.testing.assert_allclose(m1.cpu().numpy(), m2.cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(i1.cpu().numpy(), i2.cpu().numpy(), rtol=1e-5)
        z1 -= z2                                                          # (in place: no fourth tensor of this size)
        assert float(z1.abs().max()) <= 1e-2 * float(z2[:1].abs().max())      # (every image of z2 is the same)
        del z1, z2
    del xd, y, ybuf


@pytest.mark.parametrize('line', LINES)
def test_stem_down_past_the_line(lib, cuda, line):
    """yolo_stem_down_fwd on copies of one 200 x 250 image (three strips, several row slices): image 0 is the two-kernel path's bit
    for bit and the oracle's within test_stem_down_fused_is_bit_identical's bar."""
    H, W = 200, 250
    Ho, Wo = 100, 125
    p, d = _first_stage(lib, cuda)
    x, x1 = _image(H, W, cuda, 7)
    N = _copies_past(line, Ho * Wo * 64 * 2)
    xd = _copies(x1, N)
    ybuf, y = guarded((N, Ho, Wo, 64), torch.bfloat16, cuda)
    st = _st()
    assert lib.yolo_stem_down_fwd(xd.data_ptr(), *_dp(d, 'w0', 's0', 'b0', 'wd', 'sd', 'bd'), y.data_ptr(), N, H, W, 32, 64, L.BF16, 0.1, st) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    _every_image_equals_the_first(y, 'stem_down')
    mid = torch.empty((1, H, W, 32), dtype=torch.bfloat16, device=cuda)
    two = torch.full((1, Ho, Wo, 64), float('nan'), dtype=torch.bfloat16, device=cuda)
    assert lib.yolo_stem_conv_fwd(x1.data_ptr(), *_dp(d, 'w0', 's0', 'b0'), mid.data_ptr(), 1, H, W, 3, 32, L.BF16, 0.1, st) == 0
    dd = L.ConvDesc()
    dd.x, dd.w_packed, dd.scale, dd.bias, dd.y = (mid.data_ptr(),) + _dp(d, 'wd', 'sd', 'bd') + (two.data_ptr(),)
    dd.N, dd.H, dd.W, dd.Cin, dd.Cout, dd.ksize, dd.stride, dd.dtype, dd.slope = 1, H, W, 32, 64, 3, 2, L.BF16, 0.1
    assert lib.yolo_conv_fwd(C.byref(dd), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(y[:1]), _bits(two))
    r1 = ref_conv(x, p['w0'], p['s0'], p['b0'], 1, 0.1, bf16=True)
    r2 = ref_conv(r1, p['wd'], p['sd'], p['bd'], 2, 0.1, bf16=True)
    np.testing.assert_allclose(from_nhwc(y[:1]), r2, rtol=2e-2, atol=2e-2 * np.abs(r2).max())
    del xd, y, ybuf


@pytest.mark.parametrize('line', LINES)
def test_res_block_past_the_line(lib, cuda, line):
    """yolo_res_block_fwd, 64 channels, on copies of one 37 x 70 image (two strips, the second ragged): x and y both pass the line;
    image 0 within test_res_block_fused's bars."""
    H, W, Cc = 37, 70, 64
    p, d = _first_stage(lib, cuda)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((1, Cc, H, W)).astype(np.float32)
    N = _copies_past(line, H * W * Cc * 2)
    xd = _copies(to_nhwc(x, 'bf16', cuda), N)
    ybuf, y = guarded((N, H, W, Cc), torch.bfloat16, cuda)
    assert lib.yolo_res_block_fwd(xd.data_ptr(), *_dp(d, 'w1', 's1', 'b1', 'w2', 's2', 'b2'), y.data_ptr(), N, H, W, Cc, L.BF16, 0.1, _st()) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    _every_image_equals_the_first(y, 'res_block')
    mid = ref_conv(x, p['w1'], p['s1'], p['b1'], 1, 0.1, bf16=True)
    ref = ref_conv(mid, p['w2'], p['s2'], p['b2'], 1, 0.1, residual=x, bf16=True)
    got = from_nhwc(y[:1])
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=2e-2, atol=3e-2)
    assert np.abs(got - ref).mean() < 2e-3
    del xd, y, ybuf


@pytest.mark.parametrize('line', LINES)
def test_stem_res_past_the_line(lib, cuda, line):
    """yolo_stem_res_fwd on copies of one 48 x 208 image (two strips): image 0 is byte for byte what yolo_stem_down_fwd followed by
    yolo_res_block_fwd give for that image (test_stem_res_is_byte_identical's check; those two are held against the oracle above)."""
    H, W = 48, 208
    Ho, Wo = H // 2, W // 2
    p, d = _first_stage(lib, cuda)
    x, x1 = _image(H, W, cuda, 9)
    N = _copies_past(line, Ho * Wo * 64 * 2)
    xd = _copies(x1, N)
    ybuf, y = guarded((N, Ho, Wo, 64), torch.bfloat16, cuda)
    st = _st()
    names = ('w0', 's0', 'b0', 'wd', 'sd', 'bd', 'w1', 's1', 'b1', 'w2', 's2', 'b2')
    assert lib.yolo_stem_res_fwd(xd.data_ptr(), *_dp(d, *names), y.data_ptr(), N, H, W, 32, 64, L.BF16, 0.1, st) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    _every_image_equals_the_first(y, 'stem_res')
    mid = torch.full((1, Ho, Wo, 64), float('nan'), dtype=torch.bfloat16, device=cuda)
    two = torch.full((1, Ho, Wo, 64), float('nan'), dtype=torch.bfloat16, device=cuda)
    assert lib.yolo_stem_down_fwd(x1.data_ptr(), *_dp(d, *names[:6]), mid.data_ptr(), 1, H, W, 32, 64, L.BF16, 0.1, st) == 0
    assert lib.yolo_res_block_fwd(mid.data_ptr(), *_dp(d, *names[6:]), two.data_ptr(), 1, Ho, Wo, 64, L.BF16, 0.1, st) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(two.float()).any()
    assert torch.equal(_bits(y[:1]), _bits(two))
    del xd, y, ybuf


S_CASE = (32, 40, 75, 64)           # Cin, H, W, Cout: 3x3 stride 1, several balanced strips, the last ragged, row slices (STREAM_CASES)


@pytest.mark.parametrize('algo,line', [(13, 31), (14, 31), (13, 32), (14, 32)])
def test_conv_stream_past_the_line(lib, cuda, algo, line):
    """conv_stream (algo 13 / 14) needs a dense y, so only a really large one reaches its offsets: copies of one 40 x 75 image, with
    the residual at 2^31 (x, the residual and y together stay within the memory budget) and without it at 2^32."""
    Cin, H, W, Cout = S_CASE
    res = line == 31
    case = (1, Cin, H, W, Cout, 3, 1)
    x, w, scale, bias, r = _host(case)
    N = _copies_past(line, H * W * Cout * 2)
    full = (N,) + case[1:]
    name = conv_variant(full, 'bf16', algo, residual=res)
    assert name is not None and 'conv_stream_kernel' in name, name
    ops = _Ops(lib, cuda, case, 'bf16', res=res)
    ops.case = full
    ops.x = _copies(ops.x, N)
    if res:
        ops.res = _copies(ops.res, N)
    ybuf, y = guarded((N, H, W, Cout), torch.bfloat16, cuda)
    ops.run(algo, y.data_ptr())
    guards_intact(ybuf, y)
    _every_image_equals_the_first(y, 'conv_stream')
    got = from_nhwc(y[:1])
    ref = ref_conv(x, w, scale, bias, 1, 0.1, residual=(r if res else None), bf16=True)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, ref, rtol=1.6e-2, atol=2e-2)
    assert np.mean(np.abs(got - ref) > 1e-3 * (1 + np.abs(ref))) < 0.02
    del ops, y, ybuf


@pytest.mark.parametrize('line', LINES)
def test_dgrad_s2_past_the_line(lib, cuda, line):
    """yolo_conv_dgrad_s2 writes dx depth-to-space into a dense tensor: copies of one 48 x 80 x 64 gradient, dx past the line (dy stays
    under the 4 GiB its input offsets allow).  conv_igemm.hip derives buf32 from dx's extent, so this is the branching form with
    a.d2s; fresh and accumulating in place (the residual is dx itself), against autograd as test_dgrad_s2_subpixel does."""
    Cin, H, W, Cout = 64, 48, 80, 128                           # forward conv: (Cin,H,W) -> (Cout,H/2,W/2)
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    dy = rng.standard_normal((1, Cout, H // 2, W // 2)).astype(np.float32)
    rb = lambda a: torch.from_numpy(a).to(torch.bfloat16).float()
    xt = torch.zeros((1, Cin, H, W)).requires_grad_(True)
    torch.nn.functional.conv2d(xt, rb(w), None, stride=2, padding=1).backward(rb(dy))
    ref = xt.grad.numpy()
    st = _st()
    wd = torch.empty(lib.yolo_packed_weight_bytes(4 * Cin, Cout, 2, L.BF16), dtype=torch.uint8, device=cuda)
    assert lib.yolo_pack_conv_weights_dgrad_s2(torch.from_numpy(w).to(cuda).data_ptr(), wd.data_ptr(), Cout, Cin, L.BF16, st) == 0
    N = _copies_past(line, H * W * Cin * 2)
    dyd = _copies(to_nhwc(dy, 'bf16', cuda), N)
    assert dyd.numel() * 2 < 0xffffff00
    cp = lib.yolo_padded_channels(4 * Cin)
    ones, zeros = torch.ones(cp, device=cuda), torch.zeros(cp, device=cuda)
    ybuf, out = guarded((N, H, W, Cin), torch.bfloat16, cuda)
    d = L.ConvDesc()
    d.x, d.w_packed, d.scale, d.bias, d.y = dyd.data_ptr(), wd.data_ptr(), ones.data_ptr(), zeros.data_ptr(), out.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope = N, H // 2, W // 2, Cout, 4 * Cin, 2, 1, L.BF16, 1.0
    assert lib.yolo_conv_dgrad_s2(C.byref(d), st) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, out)
    _every_image_equals_the_first(out, 'dgrad_s2')
    got = from_nhwc(out[:1])
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-2, atol=1e-2 * np.abs(ref).max())
    d.residual = out.data_ptr()                                  # accumulate in place
    assert lib.yolo_conv_dgrad_s2(C.byref(d), st) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, out)
    _every_image_equals_the_first(out, 'dgrad_s2, accumulating')
    np.testing.assert_allclose(from_nhwc(out[:1]), 2 * ref, rtol=2e-2, atol=2e-2 * np.abs(ref).max())
    del dyd, out, ybuf
