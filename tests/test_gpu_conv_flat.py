"""The flat streaming 1x1 (csrc/conv_flat.hip, algo lib.CONV_FLAT_ALGO) through the C ABI: byte for byte the tiled 1x1 (algo 39)
on the same buffers and inside the 1x1 tolerance of tests/test_gpu_conv.py against the CPU oracle -- less than one tile, a ragged
last tile with tiles crossing rows and images, and per channel pair a map on which every persistent block walks at least four
tiles with a partial last round; its refusals (host only); its surroundings (guard bands around the output, NaN behind the
input's last pixel); and a D53 net whose eligible layers all run it."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import TDT, LDT, conv_variant, guarded, guards_intact, moated, to_nhwc, from_nhwc, ref_conv, bits_of
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu

FLAT, TILED = L.CONV_FLAT_ALGO, 39
PAIRS = [(256, 128), (512, 256)]
SMALL = [(1, 3, 3, 256, 128), (3, 7, 9, 256, 128), (2, 13, 13, 512, 256)]        # (N, H, W, Cin, Cout)


def _walk_shape(cin, cout):
    """(N, 13, 13, cin, cout) on which every block of the persistent grid walks >= 4 tiles and the last round is partial."""
    tp, bpc = L.conv_flat_geometry(cin, cout)
    grid = torch.cuda.get_device_properties(0).multi_processor_count * bpc
    n = -(-(grid * 4 + grid // 2) * tp // 169)
    tiles = -(-n * 169 // tp)
    assert tiles // grid >= 4 and tiles % grid != 0 and (n * 169) % tp != 0, (n, tiles, grid)
    return (n, 13, 13, cin, cout)


def _operands(shape, dtype, res, affine, seed=3):
    N, H, W, Cin, Cout = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Cin, H, W), dtype=np.float32)
    w = (rng.standard_normal((Cout, Cin, 1, 1)) / np.sqrt(Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32) if affine else None
    bias = (0.1 * rng.standard_normal(Cout)).astype(np.float32) if affine else None
    r = rng.standard_normal((N, Cout, H, W), dtype=np.float32) if res else None
    return x, w, scale, bias, r


class _Conv(object):
    """One 1x1 on device buffers that stay put between launches: y(algo) -> the output tensor (N, H, W, Cout), freshly poisoned,
    between guard bands that are checked after the launch."""

    def __init__(self, lib, dev, shape, dtype, x, w, scale, bias, r, slope=0.1, xd=None):
        N, H, W, Cin, Cout = shape
        self.lib, self.dev, self.shape, self.dtype = lib, dev, shape, dtype
        self.st = torch.cuda.current_stream().cuda_stream
        dt = LDT[dtype]
        self.xd = moated(to_nhwc(x, dtype, dev)) if xd is None else xd
        wd = moated(torch.from_numpy(w).to(dev))
        self.wbuf, self.wp = guarded((lib.yolo_packed_weight_bytes(Cout, Cin, 1, dt),), torch.uint8, dev)
        L.check(lib.yolo_pack_conv_weights(wd.data_ptr(), self.wp.data_ptr(), Cout, Cin, 1, dt, self.st), 'pack')
        self.sc = self.bi = None
        if scale is not None:
            cp = lib.yolo_padded_channels(Cout)
            sc = torch.zeros(cp, device=dev); sc[:Cout] = torch.from_numpy(scale).to(dev)
            bi = torch.zeros(cp, device=dev); bi[:Cout] = torch.from_numpy(bias).to(dev)
            self.sc, self.bi = moated(sc), moated(bi)
        self.rd = moated(to_nhwc(r, dtype, dev)) if r is not None else None
        self.slope = slope

    def desc(self, y, algo):
        N, H, W, Cin, Cout = self.shape
        d = L.ConvDesc()
        d.x, d.w_packed, d.y = self.xd.data_ptr(), self.wp.data_ptr(), y.data_ptr()
        d.scale, d.bias = L.ptr(self.sc), L.ptr(self.bi)
        d.residual = L.ptr(self.rd)
        d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = N, H, W, Cin, Cout, 1, 1
        d.dtype, d.slope, d.algo = LDT[self.dtype], self.slope, algo
        return d

    def y(self, algo):
        N, H, W, Cin, Cout = self.shape
        ybuf, y = guarded((N, H, W, Cout), TDT[self.dtype], self.dev)
        d = self.desc(y, algo)
        buf = C.create_string_buffer(256)
        assert self.lib.yolo_conv_kernel_name(C.byref(d), buf, 256) == 0, 'algo %d refuses the shape' % algo
        assert ('conv_flat_kernel' in buf.value.decode()) == (algo == FLAT), buf.value
        assert self.lib.yolo_conv_fwd(C.byref(d), self.st) == 0
        torch.cuda.synchronize()
        guards_intact(ybuf, y)
        guards_intact(self.wbuf, self.wp)
        return y


def _check(lib, cuda, shape, dtype, res, affine):
    x, w, scale, bias, r = _operands(shape, dtype, res, affine)
    cv = _Conv(lib, cuda, shape, dtype, x, w, scale, bias, r)
    yf, yt = cv.y(FLAT), cv.y(TILED)
    assert not bool(torch.isnan(yf).any())
    assert torch.equal(bits_of(yf), bits_of(yt)), '%d values differ from the tiled kernel' % int((bits_of(yf) != bits_of(yt)).sum())
    one = np.ones(shape[4], np.float32)
    ref = (ref_conv(x, w, scale, bias, 1, 0.1, residual=r, bf16=(True if dtype == 'bf16' else 'f16')) if affine else
           ref_conv(x, w, one, 0 * one, 1, 1.0, residual=r, bf16=(True if dtype == 'bf16' else 'f16')))     # (identity epilogue)
    y = from_nhwc(yf)
    if dtype == 'f16':
        np.testing.assert_allclose(y, ref, rtol=2e-3, atol=2e-3)
        assert np.mean(np.abs(y - ref) > 2e-4 * (1 + np.abs(ref))) < 0.02
    else:
        np.testing.assert_allclose(y, ref, rtol=1.6e-2, atol=2e-2)
        assert np.mean(np.abs(y - ref) > 1e-3 * (1 + np.abs(ref))) < 0.02


@pytest.mark.parametrize('affine', [True, False], ids=['bn', 'identity'])
@pytest.mark.parametrize('res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_flat_equals_the_tiled_kernel_and_the_oracle(lib, cuda, shape, dtype, res, affine):
    _check(lib, cuda, shape, dtype, res, affine)


@pytest.mark.parametrize('affine', [True, False], ids=['bn', 'identity'])
@pytest.mark.parametrize('res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: '%dto%d' % p)
def test_flat_persistent_walk(lib, cuda, pair, dtype, res, affine):
    """ring reuse and the persistent loop: >= 4 tiles per block, a partial last round, a ragged last tile"""
    _check(lib, cuda, _walk_shape(*pair), dtype, res, affine)


def test_flat_refusals_and_names():
    ok = {(256, 128): 'void conv_flat_kernel<256, 128, %s>(FlatArgs)', (512, 256): 'void conv_flat_kernel<512, 256, %s>(FlatArgs)'}
    for (cin, cout), name in ok.items():
        case = (2, cin, 13, 13, cout, 1, 1)
        for dtype in ('bf16', 'f16'):
            assert conv_variant(case, dtype, FLAT) == name % (dtype + '_t')
            assert conv_variant(case, dtype, FLAT, residual=True) == name % (dtype + '_t')
            # strided views, up-sampled stores, fp32 logits, a statistics epilogue, a fused tail
            for fields in ({'x_pixel_stride': 2 * cin}, {'y_pixel_stride': 2 * cout}, {'y_batch_stride': 13 * 13 * cout + 64},
                           {'upsample2x': 1}, {'out_f32': 1},
                           {'tail_w_packed': True, 'tail_y': True, 'tail_cout': 64, 'tail_slope': 0.1}):
                assert conv_variant(case, dtype, FLAT, fields=fields) is None, fields
            assert conv_variant(case, dtype, FLAT, stats_mode=1) is None
            assert conv_variant(case, dtype, FLAT, stats_mode=2) is None
        for dtype in ('f32', 'bf16x3', 'f16x3'):
            assert conv_variant(case, dtype, FLAT) is None, dtype
        assert conv_variant((2, cin, 13, 13, cout, 3, 1), 'bf16', FLAT) is None
        assert L.conv_flat_geometry(cin, cout) is not None
    for cin, cout in ((256, 256), (512, 128), (1024, 512), (128, 64), (256, 64), (512, 192)):
        assert conv_variant((2, cin, 13, 13, cout, 1, 1), 'bf16', FLAT) is None, (cin, cout)
        assert L.conv_flat_geometry(cin, cout) is None


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('shape', SMALL[:2], ids=lambda s: 'x'.join(map(str, s)))
def test_flat_surroundings(lib, cuda, shape, dtype):
    """The output sits between poisoned guard bands and comes back untouched outside the map (checked by _Conv.y); the bytes
    behind the input's last pixel are NaN in one run and zeros in the other, and the outputs are the same."""
    x, w, scale, bias, r = _operands(shape, dtype, True, True, seed=5)
    y_nan = _Conv(lib, cuda, shape, dtype, x, w, scale, bias, r).y(FLAT)
    xt = to_nhwc(x, dtype, cuda)
    pool = torch.zeros(xt.numel() + (1 << 19), dtype=xt.dtype, device=cuda)          # 1 MiB of zeros behind the last pixel
    xz = pool[:xt.numel()].view(xt.shape)
    xz.copy_(xt)
    y_zero = _Conv(lib, cuda, shape, dtype, x, w, scale, bias, r, xd=xz).y(FLAT)
    assert not bool(torch.isnan(y_nan).any())
    assert torch.equal(bits_of(y_nan), bits_of(y_zero))


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_flat_in_a_net_equals_the_tiled_kernels(cuda, dtype):
    """A D53 CarNet at 2 x 3 x 64 x 64 with the flat kernel forced on every eligible layer: the logits of the same net with those
    layers on algo 39, byte for byte."""
    import oracle.graph as og
    from yolo_amd.net import CarNet
    from yolo_amd.tuner import conv_key
    spec = og.spec_d53()
    P = og.init_params(og.build_graph(spec), seed=0, bn='random')
    x = torch.from_numpy(np.random.default_rng(7).random((2, 3, 64, 64), dtype=np.float32)).to(cuda)

    def net():
        return CarNet(spec, dtype=dtype, device=cuda, tune='plan', fuse_tail=False).load_params(P)
    probe = net()
    probe(x)
    keys = [conv_key(d) for kind, d, _ in probe._plan_for(2, 64, 64).ops
            if kind == 'conv' and d.ksize == 1 and (d.Cin, d.Cout) in PAIRS and not (d.x_pixel_stride or d.y_pixel_stride or d.upsample2x)]
    assert len(set(keys)) >= 2 and len(keys) >= 16, keys
    outs = {}
    for algo in (FLAT, TILED):
        n = net()
        n.load_tuning_state({'algo': {k: algo for k in keys}})
        outs[algo] = [o.clone() for o in n(x)]
        flat = sum('conv_flat_kernel' in k for _, k, _ in n.plan_kernels(2, 64, 64))
        assert flat == (len(keys) if algo == FLAT else 0) and n.stale_choices == 0
    torch.cuda.synchronize()
    assert all(not bool(torch.isnan(a.float()).any()) and torch.equal(bits_of(a), bits_of(b)) for a, b in zip(outs[FLAT], outs[TILED]))
