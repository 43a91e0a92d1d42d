"""The split-bf16 training path (Trainer on CarNet(dtype='bf16x3'), include/yolo_amd.h YOLO_BF16X3): its building blocks
against float64 and a split simulation restated here, then whole steps against the oracle's fp32 autograd restatement of
_train_batch (car/YOLO.py:350-399).  Split storage: per pixel a hi plane of Cp = round_up(C, 32) values, then the lo plane."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graph as og, train as ot
from util import split_planes, ab_counts, ab_tensor
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu

DT = L.BF16X3


def _cp(C):
    return -(-C // 32) * 32


def _to_split(v, cuda, fill=0.0):
    """(..., C) fp32 -> split storage (..., 2, Cp) bf16 on the device; the pad channels hold `fill`."""
    v = torch.as_tensor(v, dtype=torch.float32)
    C = v.shape[-1]
    hi, lo = split_planes(v)
    out = torch.full(tuple(v.shape[:-1]) + (2, _cp(C)), fill, dtype=torch.bfloat16)
    out[..., 0, :C], out[..., 1, :C] = hi, lo
    return out.to(cuda)


def _val(t, C):
    """split storage -> (..., C) fp32 value hi + lo (exact in fp32)."""
    t = t.float().cpu()
    return t[..., 0, :C] + t[..., 1, :C]


def _store(v):
    """A value as the split path stores it: hi = bf16(v), lo = bf16(v - hi)."""
    hi, lo = split_planes(torch.as_tensor(v, dtype=torch.float32))
    return hi.float() + lo.float()


def _pads_zero(t, C):
    return C == t.shape[-1] or bool((t[..., C:] == 0).all())


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---- BatchNorm train forward / backward ---------------------------------------------------------------------------------
@pytest.mark.parametrize('C,npix,residual', [(32, 3000, False), (48, 2000, True), (1024, 169, True), (48, 1, False)])
def test_split_bn_train_fwd_bwd(lib, cuda, C, npix, residual):
    rng = np.random.default_rng(C + npix)
    y = (rng.standard_normal((npix, C)) * 2 + 3).astype(np.float32)
    dz = rng.standard_normal((npix, C)).astype(np.float32)
    res = rng.standard_normal((npix, C)).astype(np.float32) if residual else None
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.2).astype(np.float32)
    eps, mom, slope = 1e-5, 0.9, 0.1
    yd, dzd = _to_split(y, cuda), _to_split(dz, cuda)
    rd = _to_split(res, cuda) if residual else None
    yv, dzv = _val(yd, C).double(), _val(dzd, C).double()
    g_t, b_t = torch.from_numpy(gamma).to(cuda), torch.from_numpy(beta).to(cuda)
    for pp in (False, True):
        z = torch.zeros_like(yd)
        dy = torch.zeros_like(yd)
        mean, invstd = torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
        rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        dgam, dbet = torch.zeros(C, device=cuda), torch.zeros(C, device=cuda)
        ws = [torch.zeros(2 * C, dtype=torch.float64, device=cuda) for _ in range(2)]
        if pp:
            L.check(lib.yolo_bn_train_fwd_pp(yd.data_ptr(), g_t.data_ptr(), b_t.data_ptr(), L.ptr(rd), z.data_ptr(), mean.data_ptr(),
                                             invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), 2 * C,
                                             npix, C, eps, mom, slope, DT, _st()), 'bn fwd pp')
            L.check(lib.yolo_bn_train_bwd_pp(dzd.data_ptr(), yd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g_t.data_ptr(),
                                             b_t.data_ptr(), dy.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), ws[1].data_ptr(),
                                             ws[0].data_ptr(), 2 * C, npix, C, slope, DT, _st()), 'bn bwd pp')
        else:
            L.check(lib.yolo_bn_train_fwd(yd.data_ptr(), g_t.data_ptr(), b_t.data_ptr(), L.ptr(rd), z.data_ptr(), mean.data_ptr(),
                                          invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), ws[0].data_ptr(), npix, C, eps, mom, slope,
                                          DT, _st()), 'bn fwd')
            L.check(lib.yolo_bn_train_bwd(dzd.data_ptr(), yd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g_t.data_ptr(),
                                          b_t.data_ptr(), dy.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), ws[0].data_ptr(), npix, C,
                                          slope, DT, _st()), 'bn bwd')
        torch.cuda.synchronize()
        # float64 reference on the values the kernels read (hi + lo)
        mu = yv.mean(0)
        var = ((yv - mu) ** 2).mean(0)
        ist = 1.0 / torch.sqrt(var + eps)
        np.testing.assert_allclose(mean.cpu().double().numpy(), mu.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(invstd.cpu().double().numpy(), ist.numpy(), rtol=1e-5)
        xh = (yv - mu) * ist
        a = torch.from_numpy(gamma).double() * xh + torch.from_numpy(beta).double()
        zr = torch.where(a > 0, a, a * slope)
        if residual:
            zr = zr + _val(rd, C).double()
        da = dzv * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
        db_r, dg_r = da.sum(0), (da * xh).sum(0)
        dyr = torch.from_numpy(gamma).double() * ist * (da - db_r / npix - xh * dg_r / npix)
        # one unit of the split storage: 2^-16 of the value (plus the fp32 arithmetic in front of the rounding)
        zs = _val(z, C).double()
        assert float(((zs - zr).abs() / (zr.abs() + 1e-3 * zr.abs().max())).max()) < 3e-5, 'z'
        np.testing.assert_allclose(dbet.cpu().double().numpy(), db_r.numpy(), rtol=1e-4, atol=1e-4 * float(db_r.abs().max()))
        np.testing.assert_allclose(dgam.cpu().double().numpy(), dg_r.numpy(), rtol=1e-4, atol=1e-4 * float(dg_r.abs().max()))
        dys = _val(dy, C).double()
        scale = float(dyr.abs().max())
        if npix > 1:
            assert float((dys - dyr).abs().max()) < 1e-4 * scale, 'dy'
        else:
            assert float(dys.abs().max()) < 1e-4, 'dy of a one-pixel map'        # (xhat = 0 and da - mean(da) = 0)
        for t in (z, dy):
            assert _pads_zero(t, C)
        np.testing.assert_allclose(rm.cpu().numpy(), (0.1 * mu).float().numpy(), rtol=1e-5, atol=1e-6)
        assert all(bool((w == 0).all()) for w in (ws[0],)) or pp


# ---- split weight gradient ----------------------------------------------------------------------------------------------
WG_CASES = [
    # N, Cin, H, W, Cout, k, stride
    (1, 8, 416, 416, 32, 3, 1),         # the 416^2 stem on the 8-channel split image copy
    (1, 32, 208, 208, 64, 3, 2),        # 208^2 stride 2 (64 -> 32 channels into 104^2)
    (2, 1024, 13, 13, 512, 1, 1),       # 13^2 x 1024
    (2, 512, 13, 13, 1024, 3, 1),
    (2, 64, 26, 26, 128, 3, 2),
    (4, 96, 20, 24, 40, 3, 1),          # Cout % 32 != 0
    (2, 128, 26, 26, 90, 1, 1),         # an output conv's Cout
    (8, 64, 104, 104, 64, 1, 1),        # 86 k pixels: the range is split over many blocks
]


def _wgrad_ref(x, dy, k, stride):
    """float64 dw of the split arithmetic's operands (hi + lo values): the conv's autograd weight gradient."""
    xd = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    dyd = torch.from_numpy(dy).double().permute(0, 3, 1, 2)
    return torch.nn.grad.conv2d_weight(xd, (dy.shape[3], x.shape[3], k, k), dyd, stride=stride, padding=k // 2)


@pytest.mark.parametrize('case', WG_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_split_wgrad(lib, cuda, case):
    N, Cin, H, W, Cout, k, s = case
    rng = np.random.default_rng(Cin * 7 + Cout)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    dy = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)
    xd, dyd = _to_split(x, cuda), _to_split(dy, cuda)
    xv, dyv = _val(xd, Cin).numpy(), _val(dyd, Cout).numpy()
    ref = _wgrad_ref(xv, dyv, k, s)
    ws = torch.zeros(lib.yolo_conv_wgrad_split_workspace_bytes(Cin, Cout, k, DT), dtype=torch.uint8, device=cuda)
    for algo in (0, 1, 2):
        dw = torch.full((Cout, Cin, k, k), 0.5, dtype=torch.float32, device=cuda)       # (the entry ADDS into dw)
        L.check(lib.yolo_conv_wgrad_split(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, k, s, 0, 0, DT,
                                          ws.data_ptr(), algo, _st()), 'wgrad split')
        torch.cuda.synchronize()
        got = dw.cpu().double() - 0.5
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < 2e-4, (algo, err)
        assert bool((ws == 0).all()), 'the workspace is left zeroed'
    # the split product drops dy_lo x_lo only: against the plain fp32 gradient of the UNROUNDED operands it is within 2e-4 too
    ref32 = _wgrad_ref(x, dy, k, s)
    assert float((got - ref32).abs().max() / ref32.abs().max()) < 2e-4


def test_split_wgrad_padded_rows_and_refusals(lib, cuda):
    """An output conv's gradient rows: Cout = 30 logical channels in rows of cpad = 32 (plane 32, pixel stride 64) and a wider
    row (pixel stride 160, lo offset 80)."""
    N, Cin, H, W, Cout = 2, 64, 13, 13, 30
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    dy = rng.standard_normal((N, H, W, Cout)).astype(np.float32)
    xd = _to_split(x, cuda)
    hi, lo = split_planes(torch.from_numpy(dy))
    wide = torch.full((N, H, W, 160), 3.0, dtype=torch.bfloat16)
    wide[..., :Cout], wide[..., 80:80 + Cout] = hi, lo
    wide = wide.to(cuda)
    ref = _wgrad_ref(_val(xd, Cin).numpy(), (hi.float() + lo.float()).numpy(), 1, 1)
    ws = torch.zeros(lib.yolo_conv_wgrad_split_workspace_bytes(Cin, Cout, 1, DT), dtype=torch.uint8, device=cuda)
    dw = torch.zeros((Cout, Cin, 1, 1), device=cuda)
    # (the 8-channel units read past channel 30 land on 3.0 here: their products belong to rows >= Cout, never stored)
    L.check(lib.yolo_conv_wgrad_split(wide.data_ptr(), xd.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, 1, 1, 160, 80, DT,
                                      ws.data_ptr(), 0, _st()), 'wgrad split strided')
    torch.cuda.synchronize()
    assert float((dw.cpu().double() - ref).abs().max() / ref.abs().max()) < 2e-4
    p = dw.data_ptr()
    assert lib.yolo_conv_wgrad_split(wide.data_ptr(), xd.data_ptr(), p, N, H, W, 12, Cout, 1, 1, 0, 0, DT, ws.data_ptr(), 0, _st()) == L.EUNSUPPORTED
    assert lib.yolo_conv_wgrad_split(wide.data_ptr(), xd.data_ptr(), p, N, H, W, Cin, Cout, 1, 1, 0, 0, L.BF16, ws.data_ptr(), 0, _st()) == L.EINVAL
    assert lib.yolo_conv_wgrad_split(wide.data_ptr(), xd.data_ptr(), p, N, H, W, Cin, Cout, 1, 1, 0, 0, DT, ws.data_ptr(), 3, _st()) == L.EINVAL
    assert lib.yolo_conv_wgrad_split(wide.data_ptr(), xd.data_ptr(), p, N, H, W, Cin, Cout, 1, 1, 40, 20, DT, ws.data_ptr(), 0, _st()) == L.EINVAL
    assert lib.yolo_conv_wgrad_split_workspace_bytes(64, 64, 3, L.BF16) == L.EINVAL
    # the pinned answers of the bf16 entries stay
    assert lib.yolo_conv_wgrad_workspace_bytes(64, 64, 3, DT) == L.EINVAL
    assert lib.yolo_pack_batch_blocks(64, 64, 3, DT) == L.EUNSUPPORTED
    assert bool((ws == 0).all())


def test_split_wgrad_batch_past_4gib(lib, cuda):
    """A batch whose split x reaches 4 GiB (the kernel's offsets are 32-bit) runs as launches over slices of whole images.  The
    batch is two different 416^2 8-channel images (tests/util.py ab_counts): the 193 copies that lie wholly below 2^32 bytes are A,
    the 65 from the one that touches the line onward are B (5.7 GB of x, likewise of dy), and an image's 22 MB do not divide 2^32 --
    so a slice that started at the wrong image, or an offset that wrapped, would change the sum: dw / N is
    (nA dw(A) + nB dw(B)) / N."""
    Cin, H, W, Cout = 8, 416, 416, 32
    rng = np.random.default_rng(21)
    x2 = _to_split(rng.standard_normal((2, H, W, Cin)).astype(np.float32), cuda)
    d2 = _to_split(rng.standard_normal((2, H, W, Cout)).astype(np.float32), cuda)
    nA, nB = ab_counts(32, x2[0].numel() * 2)
    N = nA + nB
    ref = sum(n * _wgrad_ref(_val(x2[i:i + 1], Cin).numpy(), _val(d2[i:i + 1], Cout).numpy(), 3, 1) for i, n in ((0, nA), (1, nB))) / N
    assert nA * x2[0].numel() * 2 < 1 << 32 < (nA + 1) * x2[0].numel() * 2 and nB * 4 >= N
    xs, ds = ab_tensor(x2[0], x2[1], nA, nB, cuda)[1], ab_tensor(d2[0], d2[1], nA, nB, cuda)[1]
    ws = torch.zeros(lib.yolo_conv_wgrad_split_workspace_bytes(Cin, Cout, 3, DT), dtype=torch.uint8, device=cuda)
    for algo in (0, 2):
        dw = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float32, device=cuda)
        L.check(lib.yolo_conv_wgrad_split(ds.data_ptr(), xs.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, 3, 1, 0, 0, DT,
                                          ws.data_ptr(), algo, _st()), 'wgrad split, sliced batch')
        torch.cuda.synchronize()
        err = float((dw.cpu().double() / N - ref).abs().max() / ref.abs().max())
        assert err < 2e-4, (algo, err)
        assert bool((ws == 0).all())
    del xs, ds


@pytest.mark.parametrize('case', [(2, 72, 13, 13, 136, 1, 1),        # P = 338: a ragged second cout tile, a cin tail
                                  (3, 96, 15, 17, 40, 3, 2)],        # Ho x Wo = 8 x 9, P = 216: border taps, Cout % 32 != 0
                         ids=lambda c: 'x'.join(map(str, c)))
def test_split_wgrad_with_zero_lo_planes_is_the_bf16_kernel_bitwise(lib, cuda, case):
    """The split per-tap kernel is the bf16 one on (hi, lo) planes.  On operands that are exactly bf16 the lo planes are all zero,
    so the two extra MFMAs of a fragment pair (hi x lo, lo x hi) add exact zeros, and with the same 128 x 128 tile (split algo 2;
    the bf16 entry's algo 1 lands on the per-tap kernel: both cases are outside the strip and row-group domains) and the same
    ascending 16-pixel K steps dw comes out bit for bit the same.  That needs one slice per launch, so that neither adds partial
    sums atomically in an order of its own: P <= 960 keeps the bf16 launch below 16 chunks of 64 pixels and the split one below 32
    chunks of 32."""
    N, Cin, H, W, Cout, k, s = case
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    assert N * Ho * Wo <= 960
    rng = np.random.default_rng(Cin + Cout)
    x = torch.from_numpy(rng.standard_normal((N, H, W, Cin)).astype(np.float32)).bfloat16()
    dy = torch.from_numpy(rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)).bfloat16()
    xs, dys = _to_split(x.float(), cuda), _to_split(dy.float(), cuda)
    assert bool((xs[..., 1, :] == 0).all()) and bool((dys[..., 1, :] == 0).all()), 'lo planes of bf16 values are zero'
    xb, dyb = x.to(cuda), dy.to(cuda)
    ws = torch.zeros(lib.yolo_conv_wgrad_split_workspace_bytes(Cin, Cout, k, DT), dtype=torch.uint8, device=cuda)
    dw_s = torch.zeros((Cout, Cin, k, k), dtype=torch.float32, device=cuda)
    dw_b = torch.zeros_like(dw_s)
    L.check(lib.yolo_conv_wgrad_split(dys.data_ptr(), xs.data_ptr(), dw_s.data_ptr(), N, H, W, Cin, Cout, k, s, 0, 0, DT,
                                      ws.data_ptr(), 2, _st()), 'wgrad split')
    L.check(lib.yolo_conv_wgrad_algo(dyb.data_ptr(), xb.data_ptr(), dw_b.data_ptr(), N, H, W, Cin, Cout, k, s, 0, L.BF16,
                                     ws.data_ptr(), 1, _st()), 'wgrad bf16')
    torch.cuda.synchronize()
    assert float(dw_b.abs().max()) > 1.0
    assert torch.equal(dw_s, dw_b)


# ---- data-gradient weight image -----------------------------------------------------------------------------------------
def _host_dgrad_image(w, Cout_f, Cin_f, k):
    """The split data-gradient image built on the host: rows = forward input channels (padded to 256), K = forward output
    channels in three passes [w'_hi | w'_hi | w'_lo] of 32-channel chunks; [chunk][tap][row][64 B] with the 16-byte units of a
    row XOR-swizzled by (row >> 2) & 3 (pack_one, csrc/conv_igemm.hip)."""
    rows, K = Cin_f, Cout_f
    rows_p, n = -(-rows // 256) * 256, -(-K // 32)
    wt = torch.from_numpy(w).permute(1, 0, 2, 3).flip(2, 3).reshape(rows, K, k * k)        # W'[ci][co][tap]
    hi, lo = split_planes(wt)
    img = torch.zeros((3 * n, k * k, rows_p, 32), dtype=torch.bfloat16)
    for pas, src in enumerate((hi, hi, lo)):
        for ch in range(n):
            for tap in range(k * k):
                blk = torch.zeros((rows_p, 32), dtype=torch.bfloat16)
                c1 = min(K, ch * 32 + 32)
                blk[:rows, :c1 - ch * 32] = src[:, ch * 32:c1, tap]
                # physical unit p of row r holds logical unit p ^ ((r >> 2) & 3)
                perm = torch.arange(rows_p)[:, None].__rshift__(2).__and__(3) ^ torch.arange(4)[None, :]
                units = blk.view(rows_p, 4, 8)
                img[pas * n + ch, tap] = torch.gather(units, 1, perm[:, :, None].expand(rows_p, 4, 8)).view(rows_p, 32)
    return img


@pytest.mark.parametrize('Cout_f,Cin_f,k', [(64, 32, 3), (48, 96, 1), (32, 8, 3)])
def test_split_dgrad_weight_image(lib, cuda, Cout_f, Cin_f, k):
    rng = np.random.default_rng(Cout_f + Cin_f)
    w = (rng.standard_normal((Cout_f, Cin_f, k, k)) / 8).astype(np.float32)
    nbytes = lib.yolo_packed_weight_bytes(Cin_f, Cout_f, k, DT)
    img = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    L.check(lib.yolo_pack_conv_weights_dgrad(torch.from_numpy(w).to(cuda).data_ptr(), img.data_ptr(), Cout_f, Cin_f, k, DT, _st()),
            'pack dgrad')
    torch.cuda.synchronize()
    host = _host_dgrad_image(w, Cout_f, Cin_f, k)
    assert img.numel() == host.numel() * 2
    assert torch.equal(img.cpu().view(torch.bfloat16).view(host.shape).view(torch.int16), host.view(torch.int16)), 'bit for bit'
    # through yolo_conv_fwd: dx = conv_stride1(dy, W') against the fp64 data gradient (stride 1)
    N, H, W = 2, 11, 13
    dy = rng.standard_normal((N, H, W, Cout_f)).astype(np.float32)
    dyd = _to_split(dy, cuda)
    dx = torch.zeros((N, H, W, 2, _cp(Cin_f)), dtype=torch.bfloat16, device=cuda)
    d = L.ConvDesc()
    d.x, d.w_packed, d.scale, d.bias, d.residual, d.y = dyd.data_ptr(), img.data_ptr(), None, None, None, dx.data_ptr()
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.dtype, d.slope = N, H, W, Cout_f, Cin_f, k, 1, DT, 1.0
    L.check(lib.yolo_conv_fwd(d, _st()), 'dgrad conv')
    torch.cuda.synchronize()
    dyv = _val(dyd, Cout_f).double().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_input((N, Cin_f, H, W), torch.from_numpy(w).double(), dyv, stride=1, padding=k // 2)
    got = _val(dx, Cin_f).double().permute(0, 3, 1, 2)
    assert float((got - ref).abs().max() / ref.abs().max()) < 2e-4
    assert _pads_zero(dx, Cin_f)
    # the sub-pixel image has no split form
    assert lib.yolo_pack_conv_weights_dgrad_s2(torch.from_numpy(w).to(cuda).data_ptr(), img.data_ptr(), Cout_f, Cin_f, DT, _st()) \
        in (L.EUNSUPPORTED, L.EINVAL)


# ---- helpers ------------------------------------------------------------------------------------------------------------
def test_split_helpers_exact(lib, cuda):
    rng = np.random.default_rng(11)
    st = _st()
    N, H, W, C1, C2 = 2, 6, 8, 24, 40
    # yolo_upsample2x_concat / _bwd
    up = rng.standard_normal((N, H // 2, W // 2, C1)).astype(np.float32)
    route = rng.standard_normal((N, H, W, C2)).astype(np.float32)
    upd, rd = _to_split(up, cuda), _to_split(route, cuda)
    cat = torch.zeros((N, H, W, 2, _cp(C1 + C2)), dtype=torch.bfloat16, device=cuda)
    L.check(lib.yolo_upsample2x_concat(upd.data_ptr(), rd.data_ptr(), cat.data_ptr(), N, H, W, C1, C2, DT, st), 'upcat')
    torch.cuda.synchronize()
    upv = _val(upd, C1)
    exp = torch.cat([upv.repeat_interleave(2, 1).repeat_interleave(2, 2), _val(rd, C2)], -1)
    assert torch.equal(_val(cat, C1 + C2), exp) and _pads_zero(cat, C1 + C2)
    hi_planes = cat.cpu()[..., 0, :C1 + C2]
    assert torch.equal(hi_planes[..., C1:], rd.cpu()[..., 0, :C2])                               # planes copied, not re-split
    dcat = rng.standard_normal((N, H, W, C1 + C2)).astype(np.float32)
    dcd = _to_split(dcat, cuda)
    dcv = _val(dcd, C1 + C2)
    for acc in (0, 1):
        dup = _to_split(np.ones((N, H // 2, W // 2, C1), np.float32), cuda)
        dro = _to_split(np.ones((N, H, W, C2), np.float32), cuda)
        L.check(lib.yolo_upsample2x_concat_bwd(dcd.data_ptr(), dup.data_ptr(), dro.data_ptr(), N, H, W, C1, C2, acc, acc, DT, st), 'upcat bwd')
        torch.cuda.synchronize()
        s = dcv[..., :C1].view(N, H // 2, 2, W // 2, 2, C1)
        s = ((s[:, :, 0, :, 0] + s[:, :, 0, :, 1]) + s[:, :, 1, :, 0]) + s[:, :, 1, :, 1]
        assert torch.equal(_val(dup, C1), _store(s + acc))
        assert torch.equal(_val(dro, C2), _store(dcv[..., C1:] + acc))
        assert _pads_zero(dup, C1) and _pads_zero(dro, C2)
    # yolo_dilate2x
    Ho, Wo, C = 3, 4, 48
    dy = rng.standard_normal((N, Ho, Wo, C)).astype(np.float32)
    dyd = _to_split(dy, cuda)
    dil = torch.zeros((N, 2 * Ho, 2 * Wo, 2, _cp(C)), dtype=torch.bfloat16, device=cuda)
    dil[..., :C] = 9.0
    L.check(lib.yolo_dilate2x(dyd.data_ptr(), dil.data_ptr(), N, 2 * Ho, 2 * Wo, Ho, Wo, C, DT, st), 'dilate')
    torch.cuda.synchronize()
    exp = torch.zeros((N, 2 * Ho, 2 * Wo, 2, C), dtype=torch.bfloat16)
    exp[:, ::2, ::2] = dyd.cpu()[..., :C]
    assert torch.equal(dil.cpu()[..., :C], exp) and _pads_zero(dil, C)
    # yolo_add_split (and yolo_add's refusal: its element count cannot locate a lo plane)
    a, b = rng.standard_normal((N, 5, 7, C)).astype(np.float32), rng.standard_normal((N, 5, 7, C)).astype(np.float32)
    ad, bd = _to_split(a, cuda), _to_split(b, cuda)
    y = torch.zeros_like(ad)
    L.check(lib.yolo_add_split(ad.data_ptr(), bd.data_ptr(), y.data_ptr(), N * 35, C, DT, st), 'add split')
    torch.cuda.synchronize()
    assert torch.equal(_val(y, C), _store(_val(ad, C) + _val(bd, C))) and _pads_zero(y, C)
    assert lib.yolo_add(ad.data_ptr(), bd.data_ptr(), y.data_ptr(), ad.numel(), DT, st) == L.EINVAL
    # yolo_gather_rows (fp32 strided rows -> split rows of Cpad channels) and yolo_bias_grad
    B, rows, Cg, Cpad = 2, 37, 30, 32
    src = rng.standard_normal((B, rows + 3, 45)).astype(np.float32)
    dst = torch.zeros((B * rows, 2, _cp(Cpad)), dtype=torch.bfloat16, device=cuda)
    srct = torch.from_numpy(src).to(cuda)
    L.check(lib.yolo_gather_rows(srct.data_ptr(), dst.data_ptr(), B, rows, Cg, Cpad, (rows + 3) * 45, 45, DT, st), 'gather')
    torch.cuda.synchronize()
    exp = torch.zeros((B * rows, Cpad))
    exp[:, :Cg] = torch.from_numpy(src[:, :rows, :Cg].reshape(B * rows, Cg))
    assert torch.equal(_val(dst, Cpad), _store(exp))
    db = torch.full((Cg,), 0.25, device=cuda)
    L.check(lib.yolo_bias_grad(dst.data_ptr(), db.data_ptr(), B * rows, Cg, 0, DT, st), 'bias grad')
    torch.cuda.synchronize()
    np.testing.assert_allclose(db.cpu().numpy(), (_val(dst, Cg).double().sum(0) + 0.25).numpy(), rtol=1e-5, atol=1e-5)
    # yolo_nchw_to_nhwc: the 8-channel split copy of the image
    img = rng.random((N, 3, 5, 6), dtype=np.float32)
    x8 = torch.zeros((N, 5, 6, 2, 32), dtype=torch.bfloat16, device=cuda)
    L.check(lib.yolo_nchw_to_nhwc(torch.from_numpy(img).to(cuda).data_ptr(), x8.data_ptr(), N, 3, 5, 6, 8, DT, st), 'nchw')
    torch.cuda.synchronize()
    exp = torch.zeros((N, 5, 6, 8))
    exp[..., :3] = torch.from_numpy(img).permute(0, 2, 3, 1)
    assert torch.equal(_val(x8, 8), _store(exp)) and _pads_zero(x8, 8)


# ---- whole training steps -----------------------------------------------------------------------------------------------
def _setup(cuda, dtype='bf16x3', B=2, seed_lab=1, tune='auto'):
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    spec, size = og.spec_micro(), (64, 96)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((B, 3) + size, dtype=np.float32)
    lab = ot.synthetic_labels(B, seed=seed_lab, render_rate=0.0, num_class=4)
    net = CarNet(spec, dtype=dtype, device=cuda, tune=tune).load_params(P)
    return spec, size, g, P, x, lab, net, Trainer(net, size)


def _loss_errors(losses, rl):
    """Per loss row (score, box_yx, box_hw, rotate, class[, the five LP losses]): max |HIP - oracle| over the batch, relative to
    the row's largest value.  (A loss of a few boxes near their targets, box_hw, is a small difference of nearly equal numbers:
    element-wise relative errors there measure the cancellation, not the step.)"""
    a, b = losses.cpu().numpy().astype(np.float64), np.stack(rl).astype(np.float64)
    return [float(np.abs(a[i] - b[i]).max() / (np.abs(b[i]).max() + 1e-30)) for i in range(a.shape[0])]


def _rel(grads, rg):
    return {n: float(np.linalg.norm(grads[n].cpu().numpy().astype(np.float64) - rg[n]) / (np.linalg.norm(rg[n]) + 1e-30)) for n in rg}


def test_trainer_split_micro_step_vs_oracle(cuda):
    """The point of the feature: the reference's fp32 arithmetic at the bf16 MFMA rate.  Against the oracle's fp32 step the split
    step's gradients are at least 10x closer (median L2) than the bf16 trainer's on the same net and inputs."""
    spec, size, g, P, x, lab, net, tr = _setup(cuda)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    losses = tr.train_step(xt, lt, update=False)
    torch.cuda.synchronize()
    rl, rg, rmerged = ot.train_step_reference(g, P, x, lab, spec, size)
    merged = tr.merged_logits().cpu().numpy()
    assert np.abs(merged - rmerged).max() / np.abs(rmerged).max() < 5e-4
    np.testing.assert_allclose(losses.cpu().numpy(), np.stack(rl), rtol=1e-3, atol=1e-7)
    rel = _rel(tr.grads(), rg)
    assert set(tr.grads()) == set(rg)
    outs_ = [n for n in rel if '.out.' in n]
    assert outs_ and max(rel[n] for n in outs_) < 1e-3, max((rel[n], n) for n in outs_)
    *_, net16, tr16 = _setup(cuda, dtype='bf16')
    tr16.train_step(xt, lt, update=False)
    rel16 = _rel(tr16.grads(), rg)
    m3, m16 = np.median(list(rel.values())), np.median(list(rel16.values()))
    print('median gradient L2 error against the fp32 oracle: bf16x3 %.3g, bf16 %.3g (worst bf16x3 %.3g)' % (m3, m16, max(rel.values())))
    assert m3 * 10 < m16, (m3, m16)
    first = float(tr.train_step(xt, lt).sum())
    for _ in range(30):
        last = float(tr.train_step(xt, lt).sum())
    assert last < 0.7 * first, (first, last)


def _split_buffers(tr):
    """(storage, logical channels) of every split buffer the trainer's plans own."""
    out = []
    for P in tr._plans.values():
        seen = set()
        for op in P.fwd:
            for k in ('x', 'yraw', 'z', 'res', 'up', 'route', 'cat'):
                t = op.get(k)
                if t is not None and id(t) not in seen:
                    seen.add(id(t))
                    out += [(b, t.shape[3]) for b in (t.val, t.gbuf) if b is not None]
            if 'dil' in op:
                out.append((op['dil'], op['c'].cout))
            if 'dyp' in op:
                out.append((op['dyp'], op['cpad']))
    return out


def test_trainer_split_pads_stay_zero_and_inference_after_training(cuda):
    from yolo_amd.net import CarNet
    spec, size, g, P, x, lab, net, tr = _setup(cuda, B=3, seed_lab=3)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    for _ in range(4):
        losses = tr.train_step(xt, lt)
    outs = tr.forward(xt)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(o).all()) for o in outs)
    bufs = _split_buffers(tr)
    assert len(bufs) > 50
    for t, C in bufs:
        assert t.dim() >= 3 and t.shape[-2] == 2 and _pads_zero(t, C), (tuple(t.shape), C)
    # inference after training = a fresh split net loaded with the trained weights and running statistics
    trained = {k: v.detach().cpu().numpy().copy() for k, v in net.params.items()}
    o1 = [o.clone() for o in net(xt)]
    fresh = CarNet(spec, dtype='bf16x3', device=cuda).load_params(trained)
    o2 = fresh(xt)
    torch.cuda.synchronize()
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', ['bf16x3', 'f32'])
def test_trainer_ignores_the_plans_bf16_gradient_choices(cuda, dtype):
    """tune='plan': a plan's data- and weight-gradient keys carry no dtype and hold bf16 choices.  A plan holding an entry for
    EVERY gradient shape of this micro step -- the keys a bf16 trainer measures, each given an id no split or fp32 kernel takes --
    must not reach the split / fp32 descriptors: the step runs and matches the heuristic's losses."""
    from yolo_amd.train import Trainer
    spec, size, g, P, x, lab, net, tr = _setup(cuda, tune='plan', dtype=dtype)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    *_, tr16 = _setup(cuda, dtype='bf16', tune='measure')
    state = tr16.tune(xt, lt)
    assert state['dgrad'] and state['wgrad']
    tr.load_tuning_state({'algo': {}, 'dgrad': {k: 99 for k in state['dgrad']}, 'wgrad': {k: 99 for k in state['wgrad']}})
    tr = Trainer(net, size)
    held = tr.tuning_state()
    assert set(state['dgrad']) <= set(held['dgrad']) and set(state['wgrad']) <= set(held['wgrad'])     # the foreign entries are there ...
    lp = tr.train_step(xt, lt, update=False)                             # ... and never applied (99 is refused)
    *_, tra = _setup(cuda, dtype=dtype)
    la = tra.train_step(xt, lt, update=False)
    np.testing.assert_allclose(lp.cpu().numpy(), la.cpu().numpy(), rtol=1e-4, atol=1e-7)
    tr.train_step(xt, lt)
    assert tr.t == 1


def test_trainer_split_measured_variants(cuda):
    spec, size, g, P, x, lab, net, tr = _setup(cuda, tune='measure')
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    state = tr.tune(xt, lt)
    assert state['wgrad'] and all(k[0] == 'bf16x3' for k in state['wgrad'])
    assert all(k[0] == 'bf16x3' for k in state['dgrad'])
    losses = tr.train_step(xt, lt, update=False)
    rl, _, _ = ot.train_step_reference(g, P, x, lab, spec, size)
    np.testing.assert_allclose(losses.cpu().numpy(), np.stack(rl), rtol=1e-3, atol=1e-7)


def test_trainer_refuses_f16x3(cuda):
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    net = CarNet(og.spec_micro(), dtype='f16x3', device=cuda)
    with pytest.raises(L.YoloError):
        Trainer(net, (64, 96))


def test_carlpnet_train_step_split(cuda):
    from yolo_amd.net import CarLPNet
    from yolo_amd.train import Trainer
    spec = dict(og.spec_micro(), LP_slice_point=[1, 3, 4, 7, 10], LP_r_max=[45, 60, 45])
    size = (64, 96)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    B = 4
    x = np.random.default_rng(2).random((B, 3) + size, dtype=np.float32)
    lab = ot.synthetic_labels(B, seed=1, render_rate=0.25, num_class=4)
    lpl = ot.synthetic_lp_labels(B, size, seed=2, add_rate=0.75)
    lpl[0, 0, 7:9] = [size[1] + 40.0, -3.0]
    lpl[0, 0, 0] = 1
    net = CarLPNet(spec, dtype='bf16x3', device=cuda).load_params(P)
    tr = Trainer(net, size, lp_r_max=spec['LP_r_max'])
    xt, lt, lpt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda), torch.from_numpy(lpl).to(cuda)
    cap = {}
    losses = tr.train_step(xt, lt, lp_labels=lpt, update=False, capture=cap)
    torch.cuda.synchronize()
    # every layer one hop from its reference on the step's own saved values (LP branch included): bar 1e-3
    from test_gpu_configs import _one_hop_check
    print('CarLPNet one-hop worst (bf16x3):', _one_hop_check(tr, _plain_plan(tr._last[0]), cap, net.params, 1e-3, 1e-3, _store))
    rl, rg, rmerged, rlp = ot.train_step_reference_lp(g, P, x, lab, lpl, spec, size)
    assert losses.shape == (10, B)
    lerr = _loss_errors(losses, rl)
    rel = _rel(tr.grads(), rg)
    worst = max(rel, key=rel.get)
    tight = [n for n in rel if n.startswith(('lp.out.', 'lp.4.tip.weight', 'heads.2.'))]
    car = [n for n in tight if n.startswith('heads.2.')]
    lp_tight = [n for n in tight if not n.startswith('heads.2.')]
    el = np.abs(losses.cpu().numpy() - np.stack(rl)) / (np.abs(np.stack(rl)) + 1e-30)
    print('CarLPNet split step: loss errors (of each loss row\'s scale) %s; element-wise worst car %.3g, LP %.3g; gradient L2 errors '
          'median %.3g, worst %.3g (%s); heads.2.* worst %.3g (%s); lp.out / lp.4.tip worst %.3g (%s)'
          % (np.round(lerr, 6).tolist(), el[:5].max(), el[5:].max(), np.median(list(rel.values())), rel[worst], worst,
             max(rel[n] for n in car), max(car, key=rel.get), max(rel[n] for n in lp_tight), max(lp_tight, key=rel.get)))
    assert len(car) >= 15 and len(lp_tight) >= 3
    # The finest car head carries only car-loss gradient, outside the LP branch, but its inputs come through the shared trunk: end to
    # end it measures 4.3e-3 (heads.2.b3.beta, a cancelling sum) against the fp32 path's 2e-3 bar, every layer one hop from its
    # reference within 1e-3 (above) -- the LeakyReLU flips of a forward ~1e-4 off fp32, as in the D53 test.  Bar 1e-2.
    assert max(rel[n] for n in car) < 1e-2, max((rel[n], n) for n in car)
    # Behind the LP branch the bars are measured ones, looser than the fp32 path's: that branch amplifies any difference of the
    # forward (the fp32 test: 1e-6 on the input moves the oracle's own LP output by 2e-3), and the split forward differs from
    # fp32 by ~1e-4 -- the gradients of the LP output conv and last tip, the LP losses and the shared early layers move with it.
    assert max(lerr[:5]) < 2e-3 and max(lerr[5:]) < 1e-2, lerr
    assert rel[worst] < 0.5, (worst, rel[worst])
    assert max(rel[n] for n in lp_tight) < 0.05, max((rel[n], n) for n in lp_tight)
    grads = tr.grads()
    cos = {}
    for name in rg:
        a, b = grads[name].cpu().numpy().astype(np.float64).ravel(), rg[name].astype(np.float64).ravel()
        cos[name] = a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30)
    print('CarLPNet split step: lowest gradient cosine %.4f (%s)' % (min(cos.values()), min(cos, key=cos.get)))
    assert min(cos.values()) > 0.9, min(cos, key=cos.get)
    first = float(tr.train_step(xt, lt, lp_labels=lpt).sum())
    for _ in range(30):
        last = float(tr.train_step(xt, lt, lp_labels=lpt).sum())
    assert last < 0.7 * first, (first, last)


class _PlainT(object):
    __slots__ = ('val', 'shape', 'grad')


def _plain_plan(P):
    """The trainer's plan with every split buffer replaced by its values hi + lo as fp32 (N, H, W, C): the form
    tests/test_gpu_configs.py:_one_hop_check reads (same tensor identities, so its consumer map holds)."""
    memo = {}

    def conv(t):
        if t is None:
            return None
        if id(t) not in memo:
            o = _PlainT()
            o.shape = t.shape
            o.val = _val(t.val, t.shape[3])
            o.grad = _val(t.grad, t.shape[3]) if t.grad is not None else None
            memo[id(t)] = o
        return memo[id(t)]
    Q = type('Plan', (), {})()
    Q.fwd = []
    for op in P.fwd:
        q = dict(op)
        for k in ('x', 'yraw', 'z', 'res', 'up', 'route', 'cat'):
            if k in op:
                q[k] = conv(op[k])
        if 'dyp' in op:
            q['dyp'] = _val(op['dyp'], op['cpad'])
        Q.fwd.append(q)
    return Q


def test_d53_train_step_split_vs_oracle(cuda):
    """BASELINE configs[2] geometry (Darknet-53, 416^2) at B = 2 on the split path.  First every forward value and every gradient
    of the step one hop from its reference, computed from the step's own saved inputs (the values hi + lo): bar 1e-3 for stored
    values and parameter gradients alike -- this is what holds each layer.  Then against the oracle's fp32 step: the five losses
    (each within 1e-3 of its row's largest value: the box_hw loss of a few boxes near their targets is a difference of nearly
    equal numbers, element-wise 2e-3 on one image), the six output convolutions' gradients (< 1e-3, the fp32 path's bar) and the
    end-to-end gradient errors, printed and bounded.  Those are looser than the fp32 path's (median < 2e-2): a forward ~1e-4
    off fp32 flips LeakyReLU' for more elements, which the one-hop check above shows to be the only difference."""
    from test_gpu_configs import _one_hop_check
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    spec, SIZE = og.spec_d53(), (416, 416)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((2, 3) + SIZE, dtype=np.float32)
    lab = ot.synthetic_labels(2, seed=3, render_rate=0.0, num_class=24)
    net = CarNet(spec, dtype='bf16x3', device=cuda).load_params(P)
    tr = Trainer(net, SIZE)
    cap = {}
    losses = tr.train_step(torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda), update=False, capture=cap)
    torch.cuda.synchronize()
    worst = _one_hop_check(tr, _plain_plan(tr._last[0]), cap, net.params, 1e-3, 1e-3, _store)
    print('one-hop worst (bf16x3):', worst)
    rl, rg, rmerged = ot.train_step_reference(g, P, x, lab, spec, SIZE)
    merged = tr.merged_logits().cpu().numpy()
    lerr = np.abs(merged - rmerged).max() / np.abs(rmerged).max()
    loss_err = _loss_errors(losses, rl)
    rel = _rel(tr.grads(), rg)
    outs_ = [n for n in rel if '.out.' in n]
    print('D53 split step: logits %.3g of scale; loss errors %s; gradient L2 errors median %.3g, worst %.3g (%s); output convs '
          'worst %.3g' % (lerr, np.round(loss_err, 6).tolist(), np.median(list(rel.values())), max(rel.values()),
                          max(rel, key=rel.get), max(rel[n] for n in outs_)))
    assert lerr < 1e-3 and max(loss_err) < 1e-3, (lerr, loss_err)
    assert len(outs_) == 6 and max(rel[n] for n in outs_) < 1e-3, max((rel[n], n) for n in outs_)
    # (end to end, past the output convs, a forward that differs from fp32 by ~1e-4 relative flips LeakyReLU' for ~1e-4 of the
    # elements: ~1e-2 of a gradient's L2 norm per layer, compounding over 75 layers -- measured median 6.1e-2, worst 8.0e-2)
    assert max(rel.values()) < 0.15 and np.median(list(rel.values())) < 0.1
