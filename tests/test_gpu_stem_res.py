"""yolo_stem_res_fwd (stem + first down-sampling conv + first residual block as ONE kernel, csrc/stem_res.hip) against the two
kernels it replaces, yolo_stem_down_fwd followed by yolo_res_block_fwd: same operand, K and accumulation order and the same
rounding points, so the output BYTES must be equal -- through the C ABI on random images and random-BN parameters, and once
through CarNet."""
import ctypes as C

import numpy as np
import pytest

import torch
from util import TDT, LDT
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu

_PARAMS = {}


def _params(lib, dev, dtype):
    """Random weights and folded-BN constants of the four convs on the device, packed once per element type."""
    if dtype in _PARAMS:
        return _PARAMS[dtype]
    ldt = LDT[dtype]
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(31)

    def pack(w):
        co, ci, k, _ = w.shape
        wp = torch.empty(lib.yolo_packed_weight_bytes(co, ci, k, ldt), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_pack_conv_weights(torch.from_numpy(w).to(dev).data_ptr(), wp.data_ptr(), co, ci, k, ldt, st), 'pack')
        return wp

    def bn(n, spread):
        out = []
        for v in (rng.uniform(0.5, 1.5, n), spread * rng.standard_normal(n)):
            t = torch.zeros(lib.yolo_padded_channels(n), device=dev)
            t[:n] = torch.from_numpy(v.astype(np.float32)).to(dev)
            out.append(t)
        return out
    p = {'w0': torch.from_numpy((rng.standard_normal((32, 3, 3, 3)) / 5).astype(np.float32)).to(dev),
         'wd': pack((rng.standard_normal((64, 32, 3, 3)) / 17).astype(np.float32)),
         'w1': pack((rng.standard_normal((32, 64, 1, 1)) / 8).astype(np.float32)),
         'w2': pack((rng.standard_normal((64, 32, 3, 3)) / 17).astype(np.float32))}
    (p['s0'], p['b0']), (p['sd'], p['bd']) = bn(32, 0.3), bn(64, 0.3)
    (p['s1'], p['b1']), (p['s2'], p['b2']) = bn(32, 0.3), bn(64, 0.3)
    torch.cuda.synchronize()
    _PARAMS[dtype] = p
    return p


def _ptr(p, *names):
    return tuple(p[n].data_ptr() for n in names)


def _geometry(lib, N, H, W):
    v = [C.c_int() for _ in range(4)]
    assert lib.yolo_stem_res_geometry(N, H, W, *[C.addressof(c) for c in v]) == 0
    return dict(zip(('nstrips', 'strip_w', 'rows_per_slice', 'slices'), (c.value for c in v)))


def _both(lib, dev, dtype, N, H, W):
    """-> (fused output, output of the two existing calls), each (N, H/2, W/2, 64)."""
    p, ldt, tdt = _params(lib, dev, dtype), LDT[dtype], TDT[dtype]
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(np.random.default_rng(N * 1000003 + H * 1009 + W).random((N, 3, H, W), dtype=np.float32)).to(dev)
    Ho, Wo = H // 2, W // 2
    mid = torch.full((N, Ho, Wo, 64), float('nan'), dtype=tdt, device=dev)
    two = torch.full((N, Ho, Wo, 64), float('nan'), dtype=tdt, device=dev)
    one = torch.full((N, Ho, Wo, 64), float('nan'), dtype=tdt, device=dev)
    assert lib.yolo_stem_down_fwd(x.data_ptr(), *_ptr(p, 'w0', 's0', 'b0', 'wd', 'sd', 'bd'), mid.data_ptr(), N, H, W, 32, 64, ldt, 0.1, st) == 0
    assert lib.yolo_res_block_fwd(mid.data_ptr(), *_ptr(p, 'w1', 's1', 'b1', 'w2', 's2', 'b2'), two.data_ptr(), N, Ho, Wo, 64, ldt, 0.1, st) == 0
    assert lib.yolo_stem_res_fwd(x.data_ptr(), *_ptr(p, 'w0', 's0', 'b0', 'wd', 'sd', 'bd', 'w1', 's1', 'b1', 'w2', 's2', 'b2'),
                                 one.data_ptr(), N, H, W, 32, 64, ldt, 0.1, st) == 0
    torch.cuda.synchronize()
    return one, two


# (N, H, W, strips per image, least row slices)
CASES = [
    pytest.param(1, 16, 16, 1, 1, id='one_strip_one_slice'),              # the smallest the walkers take
    pytest.param(2, 64, 120, 1, 1, id='one_strip_60_columns'),
    pytest.param(2, 64, 124, 2, 1, id='two_strips_second_2_wide'),        # halo columns at a strip seam
    pytest.param(1, 48, 208, 2, 1, id='strips_wo_104'),                   # a width that is not a multiple of the strip
    pytest.param(1, 416, 32, 1, 3, id='three_or_more_row_slices'),        # slice seams with the producer's extra rows
    pytest.param(3, 34, 32, 1, 1, id='odd_output_height'),                # ... and a batch that is not a power of two
]


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('N,H,W,nstrips,min_slices', CASES)
def test_stem_res_is_byte_identical(lib, cuda, N, H, W, nstrips, min_slices, dtype):
    g = _geometry(lib, N, H, W)
    assert g['nstrips'] == nstrips and g['strip_w'] == 60 and g['slices'] >= min_slices
    assert (g['slices'] - 1) * g['rows_per_slice'] < H // 2 <= g['slices'] * g['rows_per_slice']
    one, two = _both(lib, cuda, dtype, N, H, W)
    assert not torch.isnan(two.float()).any()
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))


def test_stem_res_rejects_and_writes_nothing(lib, cuda):
    p = _params(lib, cuda, 'bf16')
    ptrs = _ptr(p, 'w0', 's0', 'b0', 'wd', 'sd', 'bd', 'w1', 's1', 'b1', 'w2', 's2', 'b2')
    x = torch.rand((1, 3, 18, 18), device=cuda)
    y = torch.full((1, 9, 9, 64), float('nan'), dtype=torch.float32, device=cuda)       # (large enough for every case below)
    call = lambda H, W, c1, c2, dt, slope=0.1: lib.yolo_stem_res_fwd(x.data_ptr(), *ptrs, y.data_ptr(), 1, H, W, c1, c2, dt, slope, None)
    assert call(17, 16, 32, 64, L.BF16) == L.EUNSUPPORTED                              # odd H
    assert call(16, 17, 32, 64, L.BF16) == L.EUNSUPPORTED                              # odd W
    assert call(16, 16, 16, 64, L.BF16) == L.EUNSUPPORTED                              # channel counts
    assert call(16, 16, 32, 128, L.BF16) == L.EUNSUPPORTED
    assert call(16, 16, 32, 64, L.F32) == L.EUNSUPPORTED                               # element types
    assert call(16, 16, 32, 64, L.BF16X3) == L.EUNSUPPORTED
    assert call(16, 16, 32, 64, L.BF16, 1.5) == L.EINVAL
    assert lib.yolo_stem_res_fwd(None, *ptrs, y.data_ptr(), 1, 16, 16, 32, 64, L.BF16, 0.1, None) == L.EINVAL
    v = [C.c_int(-7) for _ in range(4)]
    assert lib.yolo_stem_res_geometry(1, 17, 16, *[C.addressof(c) for c in v]) == L.EUNSUPPORTED
    assert [c.value for c in v] == [-7] * 4
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


def test_net_stem_res_forced_matches_two_launches(cuda):
    """CarNet on the D53 spec with the one launch forced against today's plan (stem_down + res_block): byte-identical logits; the
    block's output keeps its parity tap, the down conv's map is no longer materialised; FLOPs = the four convs."""
    from yolo_amd.net import CarNet
    from yolo_amd.spec import darknet53_spec
    x = torch.rand((2, 3, 64, 64), device=cuda)
    nets, outs = [], []
    for fuse in ('force', True):
        net = CarNet(darknet53_spec(), dtype='bf16', device=cuda, fuse_stem=fuse, fuse_res=True).initialize(5)
        outs.append([t.clone() for t in net(x)])
        nets.append(net)
    kinds = [[op[0] for op in n._last_plan.ops] for n in nets]
    assert kinds[0][0] == 'stem_res' and 'stem_down' not in kinds[0] and kinds[1][:2] == ['stem_down', 'res_block']
    assert kinds[0][1:] == kinds[1][2:]
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert 'stages.0.down' not in nets[0]._last_plan.act and 'stages.0.down' in nets[1]._last_plan.act
    tap = [n.activation_nchw('stages.0.res.0.c2') for n in nets]
    assert torch.equal(tap[0], tap[1])
    k = [n.plan_kernels(2, 64, 64) for n in nets]
    assert k[0][0][:2] == ('stages.0.res.0.c2', 'stem_res_kernel') and k[0][0][2] == k[1][0][2] + k[1][1][2]
    # the split types, fuse_res=False and fuse_stem=False never take it
    for kw in (dict(dtype='bf16x3', fuse_stem='force'), dict(dtype='bf16', fuse_stem='force', fuse_res=False), dict(dtype='bf16', fuse_stem=False)):
        n = CarNet(darknet53_spec(), device=cuda, **kw).initialize(5)
        n(x)
        assert 'stem_res' not in [op[0] for op in n._last_plan.ops]
