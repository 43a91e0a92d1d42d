"""The training-step kernels across the 2 GiB and 4 GiB offset lines (audit table: NOTES.md, "Offsets past 2^31 and 2^32 bytes: the
training step").

BatchNorm, the weight gradients, the movers and the adders reduce over, or rewrite, the WHOLE tensor, so the tensors here are really
filled -- N copies of two small images (tests/util.py ab_counts): image A wherever an image lies wholly below the line under test,
image B from the image that touches the line onward, at least a quarter of them B.  An image is 20 x 28 or 20 x 13 pixels (2004 x
44 and 510 x 91 for the column-strip kernel, see HS), so its byte size does not divide 2^31: an offset that wraps by 2^31 or 2^32 reads (or writes) the wrong image at the wrong phase and the
result changes.  The tensors are expanded on the device; the references are CPU float64 on A and B alone, combined by the counts.
Outputs lie between guard bands, pre-filled with 0xFF: an unwritten element is a NaN, a write beyond the tensor changes a band."""
import functools

import numpy as np
import pytest
import torch

from util import guarded, guards_intact, split_planes, ab_counts, ab_tensor, ab_images_equal, bits_of, TDT, LDT
from yolo_amd import lib as L

pytestmark = pytest.mark.gpu

H0, W0 = 20, 28
# The column-strip weight-gradient kernel adds one fp32 partial sum per (image, strip) to every gradient element, and n fp32
# additions of EQUAL terms err by up to n 2^-24 of the sum, all the same way.  Hundreds of thousands of 20 x 28 images would put
# that above the bar of 1e-3; tall images (two strips, the second ragged) keep n below 10^4: n 2^-24 < 5e-4.
HS, WS = 2004, 44
EPS, MOM, SLOPE = 1e-5, 0.9, 0.1


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cp(C):
    return -(-C // 32) * 32


def _es(dtype):
    return 4 if dtype == 'f32' else 2


def _store(v, dtype):
    """fp32 (..., C) CPU tensor -> (the tensor as `dtype` stores it -- split: (..., 2, Cp), zero pads --, the float64 values the
    kernels read from that storage)."""
    v = torch.as_tensor(v, dtype=torch.float32)
    if dtype == 'f32':
        return v.clone(), v.double()
    if dtype == 'bf16':
        s = v.bfloat16()
        return s, s.double()
    C = v.shape[-1]
    hi, lo = split_planes(v)
    s = torch.zeros(tuple(v.shape[:-1]) + (2, _cp(C)), dtype=torch.bfloat16)
    s[..., 0, :C], s[..., 1, :C] = hi, lo
    return s, hi.double() + lo.double()


def _values(t, dtype, C, poisoned_pads=False):
    """Storage (one image, device or host) -> float64 values on the host; poisoned_pads: the pad channels of a split OUTPUT still
    hold the 0xFF it was pre-filled with."""
    t = t.cpu()
    if dtype != 'bf16x3':
        return t.double()
    if poisoned_pads and t.shape[-1] != C:
        assert bool((bits_of(t[..., C:].contiguous()) == -1).all()), 'the pad channels of a split plane were written'
    return t[..., 0, :C].double() + t[..., 1, :C].double()


def _image_bytes(s):
    return s.numel() * s.element_size()


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _exact(t, nA, wantA, wantB, what, C=None):
    """Image 0 (an A) and image nA (the B that touches the line) equal the expected storage bit for bit; C: split storage whose pad
    channels are not written (they still hold 0xFF)."""
    for i, want in ((0, wantA), (nA, wantB)):
        got = t[i].cpu()
        if C is not None and got.shape[-1] != C:
            assert bool((bits_of(got[..., C:].contiguous()) == -1).all()), '%s: the pad channels of image %d were written' % (what, i)
            got, want = got[..., :C], want[..., :C]
        g, w = bits_of(got.contiguous()), bits_of(want.contiguous())
        assert g.shape == w.shape and torch.equal(g, w), '%s: image %d: %d of %d elements differ' % (what, i, int((g != w).sum()), g.numel())


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------
BN_C = {'f32': 32, 'bf16': 32, 'bf16x3': 40}          # (split: 40 channels in planes of 64, so pad channels exist)


class _Case(object):
    pass


@functools.lru_cache(maxsize=None)
def _bn_case(dtype, line):
    """Images A and B of y, the residual and dz, and the float64 BatchNorm of nA copies of A and nB of B."""
    C = BN_C[dtype]
    rng = np.random.default_rng(100 * C + line)
    c = _Case()
    c.C, c.dtype = C, dtype
    c.gamma = torch.from_numpy(rng.uniform(.5, 1.5, C).astype(np.float32))
    c.beta = torch.from_numpy((.2 * rng.standard_normal(C)).astype(np.float32))
    g, b = c.gamma.double(), c.beta.double()
    c.k = {}
    for kind, shift in (('A', .5), ('B', -1.)):
        k = c.k[kind] = _Case()
        k.ys, k.yv = _store((2 * rng.standard_normal((H0, W0, C)) + shift).astype(np.float32), dtype)
        k.rs, k.rv = _store(rng.standard_normal((H0, W0, C)).astype(np.float32), dtype)
        k.ds, k.dv = _store(rng.standard_normal((H0, W0, C)).astype(np.float32), dtype)
    c.nA, c.nB = ab_counts(line, _image_bytes(c.k['A'].ys))
    w = {'A': c.nA, 'B': c.nB}
    c.npix = (c.nA + c.nB) * H0 * W0
    c.s1 = sum(w[n] * c.k[n].yv.sum((0, 1)) for n in w)
    c.s2 = sum(w[n] * (c.k[n].yv ** 2).sum((0, 1)) for n in w)
    c.mean = c.s1 / c.npix
    c.var = sum(w[n] * ((c.k[n].yv - c.mean) ** 2).sum((0, 1)) for n in w) / c.npix
    c.ist = 1.0 / torch.sqrt(c.var + EPS)
    # The bars of the statistics.  The reduction sums (y - k) and (y - k)^2 around the pivot k = pixel 0 of the tensor, n = _bn_chain()
    # fp32 terms per thread and in double from there on: n fp32 additions in any order stay within n 2^-24 sum|v| (8 more for
    # the fp32 operations in front of them), and the results are rounded to fp32 once.  var = q / N - d^2 with d = mean - k.
    # (test_bn_train_fwd_bwd's rtol of 1e-5 is for threads that add 8 terms; here they add hundreds.)
    piv = c.k['A'].yv[0, 0]
    e1 = sum(w[n] * (c.k[n].yv - piv).abs().sum((0, 1)) for n in w) / c.npix
    e2 = sum(w[n] * ((c.k[n].yv - piv) ** 2).sum((0, 1)) for n in w) / c.npix
    u = (_bn_chain(c.npix, C, dtype) + 8) * 2.0 ** -24
    c.mean_bar = u * e1 + 2.0 ** -23 * c.mean.abs()
    c.var_bar = u * (e2 + 2 * (c.mean - piv).abs() * e1) + 2.0 ** -23 * c.var
    c.ist_bar = c.ist * (0.5 * c.var_bar / (c.var + EPS) + 2.0 ** -23)
    for n in w:
        k = c.k[n]
        k.xh = (k.yv - c.mean) * c.ist
        a = g * k.xh + b
        k.z = torch.where(a > 0, a, a * SLOPE)
        # where a is within 1e-3 of zero, fp32 arithmetic may take the other branch of the LeakyReLU: such elements get dz = 0, so
        # that da = 0 on either branch (z differs by less than 1e-3 * |a| there, far below its tolerance)
        near = a.abs() < 1e-3
        if dtype == 'bf16x3':
            k.ds[..., 0, :C][near] = 0
            k.ds[..., 1, :C][near] = 0
        else:
            k.ds[near] = 0
        k.dv = torch.where(near, torch.zeros_like(k.dv), k.dv)
        k.da = k.dv * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))
    c.db = sum(w[n] * c.k[n].da.sum((0, 1)) for n in w)
    c.dg = sum(w[n] * (c.k[n].da * c.k[n].xh).sum((0, 1)) for n in w)
    c.mag_b = sum(w[n] * c.k[n].da.abs().sum((0, 1)) for n in w)
    c.mag_g = sum(w[n] * (c.k[n].da * c.k[n].xh).abs().sum((0, 1)) for n in w)
    for n in w:
        k = c.k[n]
        k.dy = g * c.ist * (k.da - c.db / c.npix - k.xh * c.dg / c.npix)
    return c


def _bn_image(got, ref, dtype, what, backward):
    """One image against float64 at the bars of test_bn_train_fwd_bwd (f32), test_bn_train_bf16 and test_split_bn_train_fwd_bwd."""
    got, ref = got.numpy(), ref.numpy()
    assert not np.isnan(got).any(), what + ': unwritten elements'
    top = np.abs(ref).max()
    err = np.abs(got - ref)
    print('%s %s: worst error %.3g (largest value %.3g)' % (what, dtype, err.max(), top))
    if dtype == 'f32':
        np.testing.assert_allclose(got, ref, err_msg=what, **(dict(rtol=1e-3, atol=1e-4 * top) if backward else dict(rtol=1e-4, atol=1e-5)))
    elif dtype == 'bf16':
        np.testing.assert_allclose(got, ref, err_msg=what, **(dict(rtol=1e-2, atol=1e-2 * top) if backward else dict(rtol=1e-2, atol=1e-2)))
    elif backward:
        assert err.max() < 1e-4 * top, what
    else:
        print('%s: worst |error| / (|z| + 1e-3 max|z|) %.3g (bar 3e-5)' % (what, (err / (np.abs(ref) + 1e-3 * top)).max()))
        assert (err / (np.abs(ref) + 1e-3 * top)).max() < 3e-5, what


def _bn_params(with_res):
    out = []
    for form, dtypes in (('plain', ('f32', 'bf16', 'bf16x3')), ('pp', ('f32', 'bf16', 'bf16x3')), ('partials', ('bf16',))):
        for dtype in dtypes:
            for res in ((False, True) if with_res else (False,)):
                out.append((form, dtype, res, 31))
    out += [('plain', 'f32', False, 32), ('pp', 'bf16', with_res, 32), ('partials', 'bf16', False, 32), ('pp', 'bf16x3', False, 32)]
    return [pytest.param(*p, id='%s-%s-%s2^%d' % (p[0], p[1], 'res-' if p[2] else '', p[3])) for p in out]


def _bn_chain(npix, C, dtype):
    """The most fp32 terms one thread of the BatchNorm reduction adds before the sums go on in double: the pixels of a block's range
    (bn_partition in csrc/bn_train.hip: 64 KB of the tensor, or npix over at most 2048 ranges; C <= 256 here) over its pixel lanes."""
    elem = 2 if dtype == 'bf16' else 4
    ranges = min(max(131072 // C, 64), 2048)
    ppb = max(65536 // (C * elem), 16)
    if -(-npix // ppb) > ranges:
        ppb = -(-npix // ranges)
    return -(-ppb // (256 // (C // 8)))


PART_ROWS = 8


def _partial_rows(q0, q1, cuda):
    """(C,) float64 sums -> PART_ROWS partial rows [rows][2][C] float32 that add up to them (to one fp32 rounding per row)."""
    part = torch.empty((PART_ROWS, 2, q0.numel()), dtype=torch.float32)
    part[:, 0], part[:, 1] = (q0 / PART_ROWS).float(), (q1 / PART_ROWS).float()
    return part.to(cuda)


@pytest.mark.parametrize('form,dtype,res,line', _bn_params(True))
def test_bn_forward_across_the_line(lib, cuda, form, dtype, res, line):
    """yolo_bn_train_fwd / _pp / _partials on y (and the residual, and z) just past 2^31 / 2^32 bytes: mean, invstd and the running
    statistics against the count-weighted float64 mixture of the two images' moments, every A image of z equal to the first and every
    B image to the first B, one of each against float64, no NaN left in z, the bands intact, the workspace (plain) or zero_next
    (the two-launch forms) zero afterwards.  _partials: the rows come from the CPU sums -- the apply pass is what crosses the line.
    (bf16x3: before bn_reduce_kernel summed a step's values on their own first, the mean of these tensors was off by 9e-7 and z of
    image A stood at 5.4e-5, 3.1e-5 with the residual and 7.1e-5 at 2^32 against the bar of 3e-5; now, image A / image B: 7.6e-6 / 7.5e-6, with the residual 9.8e-6 / 1.9e-5, at 2^32 7.5e-6 / 8.9e-6.)"""
    c = _bn_case(dtype, line)
    C, nA, nB, A, B = c.C, c.nA, c.nB, c.k['A'], c.k['B']
    y = ab_tensor(A.ys, B.ys, nA, nB, cuda)[1]
    assert y.numel() * y.element_size() > 1 << line and nB * 4 >= nA + nB
    r = ab_tensor(A.rs, B.rs, nA, nB, cuda)[1] if res else None
    zbuf, z = guarded(y.shape, y.dtype, cuda)
    gam, bet = c.gamma.to(cuda), c.beta.to(cuda)
    mean, invstd = torch.full((C,), float('nan'), device=cuda), torch.full((C,), float('nan'), device=cuda)
    rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    ws, nxt = torch.zeros(2 * C, dtype=torch.float64, device=cuda), torch.full((2 * C,), 7.0, dtype=torch.float64, device=cuda)
    head = (y.data_ptr(), gam.data_ptr(), bet.data_ptr(), L.ptr(r), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(),
            rv.data_ptr(), ws.data_ptr())
    tail = (c.npix, C, EPS, MOM, SLOPE, LDT[dtype], _st())
    if form == 'plain':
        rc = lib.yolo_bn_train_fwd(*(head + tail))
    elif form == 'pp':
        rc = lib.yolo_bn_train_fwd_pp(*(head + (nxt.data_ptr(), 2 * C) + tail))
    else:
        part = _partial_rows(c.s1, c.s2, cuda)
        rc = lib.yolo_bn_train_fwd_partials(*((part.data_ptr(), PART_ROWS, C) + head + (nxt.data_ptr(), 2 * C) + tail))
    assert rc == 0, rc
    torch.cuda.synchronize()
    guards_intact(zbuf, z)
    for name, got, ref, bar in (('mean', mean, c.mean, c.mean_bar), ('invstd', invstd, c.ist, c.ist_bar),
                                ('running_mean', rm, (1 - MOM) * c.mean, (1 - MOM) * c.mean_bar + 2.0 ** -23 * c.mean.abs()),
                                ('running_var', rv, MOM + (1 - MOM) * c.var, (1 - MOM) * c.var_bar + 2.0 ** -23 * (1 + c.var))):
        err = (got.cpu().double() - ref).abs()
        print('%s: worst error / bar %.3g, worst relative error %.3g' % (name, float((err / bar).max()), float((err / ref.abs()).max())))
        assert bool((err <= bar).all()), name
    ab_images_equal(z, nA, 'z')
    if dtype == 'bf16x3':           # (a figure, not a check: the same comparison with the device's own fp32 mean and invstd in the reference)
        xh = (A.yv - mean.cpu().double()) * invstd.cpu().double()
        a = c.gamma.double() * xh + c.beta.double()
        zr = torch.where(a > 0, a, a * SLOPE) + (A.rv if res else 0)
        d = (_values(z[0], dtype, C) - zr).abs() / (zr.abs() + 1e-3 * zr.abs().max())
        print('z of image A with the returned statistics in the reference: worst %.3g (bar 3e-5)' % float(d.max()))
    for i, k, name in ((0, A, 'A'), (nA, B, 'B')):
        _bn_image(_values(z[i], dtype, C, True), k.z + (k.rv if res else 0), dtype, 'z of image %s' % name, False)
    assert bool((ws == 0).all()) if form == 'plain' else bool((nxt == 0).all())
    del y, r, z, zbuf
    _free()


@pytest.mark.parametrize('form,dtype,res,line', _bn_params(False))
def test_bn_backward_across_the_line(lib, cuda, form, dtype, res, line):
    """yolo_bn_train_bwd / _pp / _partials likewise (mean and invstd are the float64 mixture's): dgamma and dbeta against nA times the
    A image's sums plus nB times the B image's, dy equal per kind and one image of each kind against float64.
    The bar of the sums: a thread of the reduction adds n = _bn_chain() fp32 terms (a few hundred here) before the sums go on in
    double, each term a few fp32 operations from its float64 value (8 more), and n fp32 additions in any order stay within
    n 2^-24 sum|v|."""
    c = _bn_case(dtype, line)
    C, nA, nB, A, B = c.C, c.nA, c.nB, c.k['A'], c.k['B']
    y = ab_tensor(A.ys, B.ys, nA, nB, cuda)[1]
    dz = ab_tensor(A.ds, B.ds, nA, nB, cuda)[1]
    assert y.numel() * y.element_size() > 1 << line
    dbuf, dy = guarded(y.shape, y.dtype, cuda)
    gam, bet = c.gamma.to(cuda), c.beta.to(cuda)
    mean, invstd = c.mean.float().to(cuda), c.ist.float().to(cuda)
    dgam, dbet = torch.full((C,), float('nan'), device=cuda), torch.full((C,), float('nan'), device=cuda)
    ws, nxt = torch.zeros(2 * C, dtype=torch.float64, device=cuda), torch.full((2 * C,), 7.0, dtype=torch.float64, device=cuda)
    head = (dz.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gam.data_ptr(), bet.data_ptr(), dy.data_ptr(),
            dgam.data_ptr(), dbet.data_ptr(), ws.data_ptr())
    tail = (c.npix, C, SLOPE, LDT[dtype], _st())
    if form == 'plain':
        rc = lib.yolo_bn_train_bwd(*(head + tail))
    elif form == 'pp':
        rc = lib.yolo_bn_train_bwd_pp(*(head + (nxt.data_ptr(), 2 * C) + tail))
    else:
        part = _partial_rows(c.db, c.dg, cuda)
        rc = lib.yolo_bn_train_bwd_partials(*((part.data_ptr(), PART_ROWS, C) + head + (nxt.data_ptr(), 2 * C) + tail))
    assert rc == 0, rc
    torch.cuda.synchronize()
    guards_intact(dbuf, dy)
    for got, ref, mag, name in ((dbet, c.db, c.mag_b, 'dbeta'), (dgam, c.dg, c.mag_g, 'dgamma')):
        err = (got.cpu().double() - ref).abs()
        bar = (_bn_chain(c.npix, C, dtype) + 8) * 2.0 ** -24 * mag + 2.0 ** -23 * ref.abs()
        print('%s: worst error / bar %.3g' % (name, float((err / bar).max())))
        assert bool((err <= bar).all()), name
    ab_images_equal(dy, nA, 'dy')
    for i, k, name in ((0, A, 'A'), (nA, B, 'B')):
        _bn_image(_values(dy[i], dtype, C, True), k.dy, dtype, 'dy of image %s' % name, True)
    assert bool((ws == 0).all()) if form == 'plain' else bool((nxt == 0).all())
    del y, dz, dy, dbuf
    _free()


# ---- weight gradients -----------------------------------------------------------------------------------------------------------
def _out_hw(H, W, k, s):
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def _dw_ref(xv, dv, k, s):
    """float64 weight gradient of a batch: xv (n, H, W, Cin), dv (n, Ho, Wo, Cout) -> (Cout, Cin, k, k)."""
    return torch.nn.grad.conv2d_weight(xv.permute(0, 3, 1, 2), (dv.shape[3], xv.shape[3], k, k), dv.permute(0, 3, 1, 2), stride=s,
                                       padding=k // 2)


@functools.lru_cache(maxsize=None)
def _wg_images(dtype, Cin, H, W, Cout, k, s):
    """Images A and B of x and dy as `dtype` stores them, and each one's float64 weight gradient."""
    rng = np.random.default_rng(1000 * Cin + 10 * W + Cout + k + s)
    Ho, Wo = _out_hw(H, W, k, s)
    out = {}
    for kind in 'AB':
        im = out[kind] = _Case()
        im.xs, im.xv = _store(rng.standard_normal((H, W, Cin)).astype(np.float32), dtype)
        im.ds, im.dv = _store(rng.standard_normal((Ho, Wo, Cout)).astype(np.float32), dtype)
        im.dw = _dw_ref(im.xv[None], im.dv[None], k, s)
    return out


def _wgrad(lib, dtype, dy, x, dw, N, shape, ws, algo, ps=0, lo=0):
    Cin, H, W, Cout, k, s = shape
    if dtype == 'bf16x3':
        return lib.yolo_conv_wgrad_split(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, k, s, ps, lo, L.BF16X3,
                                         ws.data_ptr(), algo, _st())
    return lib.yolo_conv_wgrad_algo(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), N, H, W, Cin, Cout, k, s, ps, LDT[dtype], L.ptr(ws),
                                    algo, _st())


def _workspace(lib, dtype, shape, cuda):
    Cin, H, W, Cout, k, s = shape
    if dtype == 'f32':
        return None
    fn = lib.yolo_conv_wgrad_split_workspace_bytes if dtype == 'bf16x3' else lib.yolo_conv_wgrad_workspace_bytes
    return torch.zeros(fn(Cin, Cout, k, LDT[dtype]), dtype=torch.uint8, device=cuda)


def _dw_close(got, ref, dtype, what):
    """got, ref float64 (normalised by N): the bar of the entry's small-tensor test."""
    got, ref = got.numpy(), ref.numpy()
    top = np.abs(ref).max()
    print('%s %s: worst error %.3g of the largest gradient' % (what, dtype, np.abs(got - ref).max() / top))
    assert np.isfinite(got).all(), what
    if dtype == 'bf16x3':
        assert np.abs(got - ref).max() / top < 2e-4, what
    elif dtype == 'f32':
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-3 * top, err_msg=what)
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=2e-3 * top, err_msg=what)


DW0 = 0.5                               # the entries ADD into dw


def _refused(lib, dtype, dy, x, dwbuf, dw, N, shape, ws, algo, what, ps=0, lo=0):
    """The call answers YOLO_EUNSUPPORTED and changes no byte of dw, its bands or the workspace."""
    before = dw.clone()
    rc = _wgrad(lib, dtype, dy, x, dw, N, shape, ws, algo, ps, lo)
    torch.cuda.synchronize()
    assert rc == L.EUNSUPPORTED, '%s: rc = %d' % (what, rc)
    guards_intact(dwbuf, dw)
    assert torch.equal(bits_of(dw), bits_of(before)), what + ': a refused call wrote dw'
    assert ws is None or bool((ws == 0).all()), what + ': a refused call wrote the workspace'


def _wgrad_ab(lib, cuda, dtype, shape, nA, nB, algos, wrong=(), refused=()):
    """x and dy as nA images A and nB images B; every algo of `algos` gives (nA dw(A) + nB dw(B)), held after division by N; the
    algos of `wrong` and `refused` answer YOLO_EUNSUPPORTED and write nothing."""
    Cin, H, W, Cout, k, s = shape
    im = _wg_images(dtype, *shape)
    N = nA + nB
    x = ab_tensor(im['A'].xs, im['B'].xs, nA, nB, cuda)[1]
    dy = ab_tensor(im['A'].ds, im['B'].ds, nA, nB, cuda)[1]
    ref = (nA * im['A'].dw + nB * im['B'].dw) / N
    ws = _workspace(lib, dtype, shape, cuda)
    dwbuf, dw = guarded((Cout, Cin, k, k), torch.float32, cuda)
    for algo in algos:
        dw.fill_(DW0)
        rc = _wgrad(lib, dtype, dy, x, dw, N, shape, ws, algo)
        torch.cuda.synchronize()
        assert rc == 0, 'algo %d: rc = %d' % (algo, rc)
        guards_intact(dwbuf, dw)
        _dw_close((dw.cpu().double() - DW0) / N, ref, dtype, 'algo %d' % algo)
        assert ws is None or bool((ws == 0).all()), 'the workspace is left zeroed'
    dw.fill_(DW0)
    for algo in tuple(wrong) + tuple(refused):
        _refused(lib, dtype, dy, x, dwbuf, dw, N, shape, ws, algo, 'algo %d' % algo)
    nbytes = x.numel() * x.element_size()
    del x, dy
    _free()
    return nbytes


# (id: the kernel the case lands in) dtype, algo, (Cin, H, W, Cout, k, stride), line, algos that must refuse the shape
WG = [
    ('f32-k3s1', 'f32', 0, (16, H0, W0, 8, 3, 1), 31, ()), ('f32-k3s2', 'f32', 0, (16, H0, W0, 8, 3, 2), 31, ()),
    ('f32-k1', 'f32', 0, (16, H0, W0, 8, 1, 1), 31, ()),
    ('f32-k3s1', 'f32', 0, (16, H0, W0, 8, 3, 1), 32, ()), ('f32-k3s2', 'f32', 0, (16, H0, W0, 8, 3, 2), 32, ()),
    ('f32-k1', 'f32', 0, (16, H0, W0, 8, 1, 1), 32, ()),
    # the per-tap kernel (wgrad_bf16_kernel): x in [2^31, 2^32), its unsigned 32-bit offsets above the sign bit
    ('general-k1-cin64', 'bf16', 1, (64, H0, W0, 8, 1, 1), 31, (2, 5)), ('general-k3s2-cin64', 'bf16', 1, (64, H0, W0, 8, 3, 2), 31, (2, 5)),
    # the column-strip kernel (3x3, Cin <= 64): 64-bit bases, so past 2^32 too
    ('strip-s1', 'bf16', 1, (8, HS, WS, 8, 3, 1), 31, (2, 5)), ('strip-s2', 'bf16', 1, (8, HS, WS, 8, 3, 2), 31, (2, 5)),
    ('strip-s1', 'bf16', 1, (8, HS, WS, 8, 3, 1), 32, (2, 5)), ('strip-s2', 'bf16', 1, (8, HS, WS, 8, 3, 2), 32, (2, 5)),
    # the row-group kernel (3x3 stride 1, W <= 40, Cin > 64): 13 columns are the (TH, K-steps) = (6, 5) variant, 20 rows leave a ragged group
    ('rows', 'bf16', 1, (72, H0, 13, 8, 3, 1), 31, (2, 5)), ('rows', 'bf16', 1, (72, H0, 13, 8, 3, 1), 32, (2, 5)),
    ('walk-2', 'bf16', 2, (64, H0, W0, 64, 3, 1), 31, (5,)), ('walk-3', 'bf16', 3, (64, H0, W0, 64, 3, 1), 31, (5,)),
    ('walk-4', 'bf16', 4, (64, H0, W0, 64, 3, 1), 31, (5,)),
    ('gemm-5', 'bf16', 5, (128, H0, W0, 128, 1, 1), 31, (2,)), ('gemm-6', 'bf16', 6, (256, H0, W0, 256, 1, 1), 31, (2,)),
    # the split kernel in ONE launch (below the slicing threshold of 0xffffff00 bytes)
    ('split-64x64', 'bf16x3', 1, (8, H0, W0, 8, 3, 1), 31, ()), ('split-128x128', 'bf16x3', 2, (8, H0, W0, 8, 3, 1), 31, ()),
    ('split-64x64-k1', 'bf16x3', 1, (8, H0, W0, 8, 1, 1), 31, ()),
]


@pytest.mark.parametrize('dtype,algo,shape,line,wrong', [pytest.param(*c[1:], id='%s-2^%d' % (c[0], c[4])) for c in WG])
def test_wgrad_across_the_line(lib, cuda, dtype, algo, shape, line, wrong):
    """x just past the line (dy with it wherever Cout and the stride leave it as large): dw / N against
    (nA dw(A, dA) + nB dw(B, dB)) / N at the bar of the entry's small-tensor test; dw starts at 0.5 between guard bands, the
    workspace is zero afterwards, and an algo outside whose domain the shape lies is refused with nothing written."""
    im = _wg_images(dtype, *shape)
    nA, nB = ab_counts(line, _image_bytes(im['A'].xs))
    nbytes = _wgrad_ab(lib, cuda, dtype, shape, nA, nB, (algo,), wrong=(wrong if dtype == 'bf16' else ()))
    assert nbytes > 1 << line
    if line == 31:
        assert nbytes < 0xffffff00


PAST = (1 << 32) + (1 << 20)            # the extent a wide dy pitch spans


# (id: the kernel) dtype, algo, (Cin, H, W, Cout, k, stride)
DY = [('f32', 'f32', 0, (16, H0, W0, 8, 3, 1)), ('general', 'bf16', 1, (64, H0, W0, 8, 1, 1)), ('strip-s1', 'bf16', 1, (8, H0, W0, 8, 3, 1)),
      ('strip-s2', 'bf16', 1, (8, H0, W0, 8, 3, 2)), ('rows', 'bf16', 1, (72, H0, 13, 8, 3, 1)), ('split-64x64', 'bf16x3', 1, (8, H0, W0, 8, 3, 1)),
      ('split-128x128', 'bf16x3', 2, (8, H0, W0, 8, 1, 1))]


@pytest.mark.parametrize('dtype,algo,shape', [pytest.param(*c[1:], id=c[0]) for c in DY])
def test_wgrad_dy_pitch_spans_4gib(lib, cuda, dtype, algo, shape):
    """dy_pixel_stride (and dy_lo_offset) so wide that the few thousand pixels of dy span more than 2^32 bytes, x a few MB: dy is a
    torch.empty of the full extent in which only the Cout (and lo) channels of each pixel are written.  Against float64 at the
    small-tensor bar, as the dense call is."""
    Cin, H, W, Cout, k, s = shape
    N, (Ho, Wo) = 4, _out_hw(H, W, k, s)
    rng = np.random.default_rng(Cin + k + s)
    xs, xv = _store(rng.standard_normal((N, H, W, Cin)).astype(np.float32), dtype)
    ds, dv = _store(rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32), dtype)
    ref = _dw_ref(xv, dv, k, s)
    P, es = N * Ho * Wo, _es(dtype)
    ps = -(-PAST // (es * P * 16)) * 16
    assert P * ps * es > 1 << 32 and ps % 16 == 0
    lo = ps // 2 if dtype == 'bf16x3' else 0
    x, dense = xs.to(cuda), ds.to(cuda)
    wide = torch.empty(P * ps, dtype=TDT[dtype], device=cuda).view(P, ps)
    if dtype == 'bf16x3':
        wide[:, :Cout], wide[:, lo:lo + Cout] = dense.view(P, 2, -1)[:, 0, :Cout], dense.view(P, 2, -1)[:, 1, :Cout]
    else:
        wide[:, :Cout] = dense.view(P, Cout)
    ws = _workspace(lib, dtype, shape, cuda)
    dwbuf, dw = guarded((Cout, Cin, k, k), torch.float32, cuda)
    for what, dyt, p, l in (('dense', dense, 0, 0), ('wide', wide, ps, lo)):
        dw.fill_(DW0)
        rc = _wgrad(lib, dtype, dyt, x, dw, N, shape, ws, algo, p, l)
        torch.cuda.synchronize()
        assert rc == 0, (what, rc)
        guards_intact(dwbuf, dw)
        _dw_close(dw.cpu().double() - DW0, ref, dtype, what)
        assert ws is None or bool((ws == 0).all())
    del wide
    _free()


def _first_past(span):
    """The first pitch (a multiple of 16 elements) that dy_lanes_fit(span, .) of csrc/wgrad.hip does not take."""
    return (0x7fffffff - 4096) // (2 * span) // 16 * 16 + 16


def _past(elements):
    return elements // 16 * 16 + 16


# (id) dtype, (Cin, H, W, Cout, k, stride), [(dy_pixel_stride, the call runs)]
PITCH = [('per-tap', 'bf16', (64, 4, 4, 8, 1, 1), [(_first_past(64), False), (_first_past(64) - 16, True)]),
         ('split', 'bf16x3', (8, 4, 4, 8, 1, 1), [(_first_past(33), False), (_first_past(33) - 16, True)]),
         # the strip kernel's farthest live lane is pixel Wo + 31 = 71 of the step: at the first pitch with 71 * ps * 2 >= 2^31 its
         # `int d_off` would wrap (and read zeros), so the right result there needs the hand-over to the per-tap kernel
         ('strip-then-per-tap', 'bf16', (8, 4, 40, 8, 3, 1), [(_past((1 << 31) // (2 * 71)), True), (_first_past(40 + 32), True),
                                                               (_first_past(40 + 32) - 16, True)]),
         # the row-group kernel's `int d_goff` counts ELEMENTS and its farthest live lane is pixel TH * W - 1 = 77 of the group: at
         # the first pitch with 77 * ps >= 2^31 it would wrap.  The per-tap kernel does not take that pitch either: refused
         ('rows-then-per-tap', 'bf16', (72, 6, 13, 8, 3, 1), [(_first_past(112), True), (_first_past(112) - 16, True),
                                                               (_past((1 << 31) // 77), False)])]


@pytest.mark.parametrize('dtype,shape,pitches', [pytest.param(*c[1:], id=c[0]) for c in PITCH])
def test_wgrad_dy_pitch_past_the_lane_offsets(lib, cuda, dtype, shape, pitches):
    """The bf16 and split kernels reach some pixels of dy through 32-bit lane offsets behind a 64-bit base.  At the first pitch (a
    multiple of 16 elements) that the host's bound for 64 / 33 pixels does not take, the per-tap and the split kernel refuse, nothing
    written; 16 elements less and they run and are right.  The strip and row-group paths hand a pitch past THEIR bound on to the
    per-tap kernel, whose chunk of 64 pixels still fits: the result is right -- also at the pitch at which the strip kernel's own
    farthest lane offset would really pass 2^31 bytes -- and a pitch at which the row-group kernel's would wrap is refused by the
    per-tap kernel as well.  Every pointer covers the extent the arguments describe."""
    Cin, H, W, Cout, k, s = shape
    N, P = 1, H * W
    rng = np.random.default_rng(Cin + W)
    xs, xv = _store(rng.standard_normal((N, H, W, Cin)).astype(np.float32), dtype)
    ds, dv = _store(rng.standard_normal((N, H, W, Cout)).astype(np.float32), dtype)
    x, dense = xs.to(cuda), ds.to(cuda)
    ref = _dw_ref(xv, dv, k, s)
    ws = _workspace(lib, dtype, shape, cuda)
    dwbuf, dw = guarded((Cout, Cin, k, k), torch.float32, cuda)
    for ps, runs in pitches:
        wide = torch.empty(P * ps, dtype=torch.bfloat16, device=cuda).view(P, ps)
        lo = ps // 2 if dtype == 'bf16x3' else 0
        if dtype == 'bf16x3':
            wide[:, :Cout], wide[:, lo:lo + Cout] = dense.view(P, 2, -1)[:, 0, :Cout], dense.view(P, 2, -1)[:, 1, :Cout]
        else:
            wide[:, :Cout] = dense.view(P, Cout)
        dw.fill_(DW0)
        if not runs:
            _refused(lib, dtype, wide, x, dwbuf, dw, N, shape, ws, 1, '%s pitch %d' % (dtype, ps), ps, lo)
        else:
            rc = _wgrad(lib, dtype, wide, x, dw, N, shape, ws, 1, ps, lo)
            torch.cuda.synchronize()
            assert rc == 0, (dtype, ps, rc)
            guards_intact(dwbuf, dw)
            _dw_close(dw.cpu().double() - DW0, ref, dtype, 'pitch %d' % ps)
            assert bool((ws == 0).all())
        del wide
        _free()


# (id) (Cin, H, W, Cout, k, stride), the family's explicit algos, its limit on the extent of dy (as of x) in bytes
DYLIM = [('walk', (64, H0, W0, 64, 3, 1), (2, 3, 4), 0xffffff00), ('gemm', (128, H0, W0, 128, 1, 1), (5,), 0xfffffe00),
         ('gemm-256', (128, H0, W0, 256, 1, 1), (5, 6), 0xfffffe00)]


@pytest.mark.parametrize('shape,algos,limit', [pytest.param(*c[1:], id=c[0]) for c in DYLIM])
def test_wgrad_walk_and_gemm_dy_at_their_limits(lib, cuda, shape, algos, limit):
    """The row walk and the 1x1 GEMM take dy_pixel_stride too and bound the extent of dy on its own (wgrad_walk_dispatch,
    wgrad_gemm_dispatch).  x is a few MB; dy is a torch.empty of the full extent with only the Cout channels of each pixel written.
    At the first pitch (a multiple of 8 elements) at which N * Ho * Wo * pitch * 2 reaches the limit, the family's algos refuse,
    nothing written, and algo 0 goes on -- the walk to the column-strip kernel (Cin <= 64), the GEMM to the per-tap kernel -- and
    is right.  One pitch step below, dy spans [2^31, 2^32) and every explicit algo runs and is right."""
    Cin, H, W, Cout, k, s = shape
    N, P = 4, 4 * H * W
    rng = np.random.default_rng(Cin + Cout + k)
    xs, xv = _store(rng.standard_normal((N, H, W, Cin)).astype(np.float32), 'bf16')
    ds, dv = _store(rng.standard_normal((N, H, W, Cout)).astype(np.float32), 'bf16')
    x, dense = xs.to(cuda), ds.to(cuda)
    ref = _dw_ref(xv, dv, k, s)
    at = -(-limit // (2 * P * 8)) * 8
    assert P * at * 2 >= limit > P * (at - 8) * 2 > 1 << 31
    ws = _workspace(lib, 'bf16', shape, cuda)
    dwbuf, dw = guarded((Cout, Cin, k, k), torch.float32, cuda)

    def run(algo, dyt, ps, what):
        dw.fill_(DW0)
        rc = _wgrad(lib, 'bf16', dyt, x, dw, N, shape, ws, algo, ps)
        torch.cuda.synchronize()
        assert rc == 0, '%s: rc = %d' % (what, rc)
        guards_intact(dwbuf, dw)
        _dw_close(dw.cpu().double() - DW0, ref, 'bf16', what)
        assert bool((ws == 0).all()), what

    for algo in algos + (0,):
        run(algo, dense, 0, 'dense, algo %d' % algo)
    for ps, refused in ((at, True), (at - 8, False)):
        wide = torch.empty(P * ps, dtype=torch.bfloat16, device=cuda).view(P, ps)
        wide[:, :Cout] = dense.view(P, Cout)
        dw.fill_(DW0)
        for algo in algos:
            if refused:
                _refused(lib, 'bf16', wide, x, dwbuf, dw, N, shape, ws, algo, 'pitch %d, algo %d' % (ps, algo), ps)
            else:
                run(algo, wide, ps, 'pitch %d, algo %d' % (ps, algo))
        run(0, wide, ps, 'pitch %d, algo 0' % ps)
        del wide
        _free()


# ---- refusals at the 32-bit limits, and what algo = 0 does after them ------------------------------------------------------------
# 0xffffff00 = 2^8 * 3^2 * 5 * 7 * 13 * 17 * 241: 75915 images of 17 x 26 pixels of 128 bytes are exactly that many bytes
LIM_N = 75915


def _limit_counts(image_bytes, N):
    nA = (1 << 31) // image_bytes
    assert (1 << 31) % image_bytes and (N - nA) * 4 >= N
    return nA, N - nA


def test_wgrad_per_tap_kernel_at_its_limit(lib, cuda):
    """x of exactly 0xffffff00 bytes, a 1x1 with Cin = 64: the per-tap kernel (algo 1) refuses, and so does algo 0 -- the GEMM does
    not take Cin % 128, nothing else takes a 1x1 (the final refusal).  One 16-byte step of a pixel less (Cin = 56) and it runs."""
    shape = (64, 17, 26, 8, 1, 1)
    assert LIM_N * 17 * 26 * 64 * 2 == 0xffffff00
    nA, nB = _limit_counts(17 * 26 * 64 * 2, LIM_N)
    _wgrad_ab(lib, cuda, 'bf16', shape, nA, nB, (), refused=(1, 0, 5, 2))
    shape = (56, 17, 26, 8, 1, 1)
    nA, nB = _limit_counts(17 * 26 * 56 * 2, LIM_N)
    _wgrad_ab(lib, cuda, 'bf16', shape, nA, nB, (1, 0))


def test_wgrad_walk_at_its_limit(lib, cuda):
    """x (and dy) of exactly 0xffffff00 bytes, 3x3 stride 1, 64 -> 64 channels: the row walk (algos 2, 3, 4) refuses; algo 0 goes on
    to the column-strip kernel (Cin <= 64), whose bases are 64-bit, and is right.  One image less and the walk runs.  (723 images of
    510 x 91 pixels: few enough partial sums per element for the strip kernel, see HS.)"""
    shape = (64, 510, 91, 64, 3, 1)
    assert 723 * 510 * 91 * 64 * 2 == 0xffffff00
    nA, nB = _limit_counts(510 * 91 * 64 * 2, 723)
    _wgrad_ab(lib, cuda, 'bf16', shape, nA, nB, (0, 1), refused=(2, 3, 4))
    _wgrad_ab(lib, cuda, 'bf16', shape, nA, nB - 1, (2, 3, 4))


def test_wgrad_walk_at_its_limit_falls_to_the_row_groups(lib, cuda):
    """The same with 128 input channels on 17 x 13 maps: after the walk's refusal algo 0 lands in the row-group kernel (W <= 40)."""
    shape = (128, 17, 13, 64, 3, 1)
    assert LIM_N * 17 * 13 * 128 * 2 == 0xffffff00
    nA, nB = _limit_counts(17 * 13 * 128 * 2, LIM_N)
    _wgrad_ab(lib, cuda, 'bf16', shape, nA, nB, (0,), refused=(2, 3))


def test_wgrad_gemm_at_its_limit(lib, cuda):
    """The 1x1 GEMM refuses at 0xfffffe00 bytes of x (= 2^9 * 47 * 178481: that many images of 2 x 47 pixels of 256 bytes); algo 0
    goes on to the per-tap kernel, which takes an x below 0xffffff00, and is right.  One image less and the GEMM runs."""
    shape, N = (128, 2, 47, 128, 1, 1), 178481
    assert N * 2 * 47 * 128 * 2 == 0x7fffff00 * 2
    nA, nB = _limit_counts(2 * 47 * 128 * 2, N)
    _wgrad_ab(lib, cuda, 'bf16', shape, nA, nB, (0, 1), refused=(5, 6))
    _wgrad_ab(lib, cuda, 'bf16', shape, nA, nB - 1, (5,))


# ---- the movers and the adders --------------------------------------------------------------------------------------------------
MOVE = [('f32', 31), ('bf16', 31), ('bf16x3', 31), ('bf16', 32)]
MOVE_IDS = ['%s-2^%d' % m for m in MOVE]


def _rand(rng, shape, dtype):
    return _store(rng.standard_normal(shape).astype(np.float32), dtype)


def _restore(v, dtype):
    """fp32 result -> the storage the kernel writes (one rounding; split: hi = bf16(v), lo = bf16(v - hi))."""
    return _store(v, dtype)[0]


def _f32(s, dtype, C):
    """Storage -> the fp32 value a kernel computes with (split: hi + lo in fp32)."""
    return s.float() if dtype != 'bf16x3' else s[..., 0, :C].float() + s[..., 1, :C].float()


@pytest.mark.parametrize('dtype,line', MOVE, ids=MOVE_IDS)
def test_add_across_the_line(lib, cuda, dtype, line):
    """yolo_add (f32, bf16: flat) and yolo_add_split (40 channels in planes of 64): one fp32 add, exact."""
    C = 40 if dtype == 'bf16x3' else 8
    rng = np.random.default_rng(line)
    (aA, _), (aB, _), (bA, _), (bB, _) = (_rand(rng, (H0, W0, C), dtype) for _ in range(4))
    nA, nB = ab_counts(line, _image_bytes(aA))
    a, b = ab_tensor(aA, aB, nA, nB, cuda)[1], ab_tensor(bA, bB, nA, nB, cuda)[1]
    ybuf, y = guarded(a.shape, a.dtype, cuda)
    assert y.numel() * y.element_size() > 1 << line
    if dtype == 'bf16x3':
        rc = lib.yolo_add_split(a.data_ptr(), b.data_ptr(), y.data_ptr(), (nA + nB) * H0 * W0, C, L.BF16X3, _st())
    else:
        rc = lib.yolo_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), y.numel(), LDT[dtype], _st())
    assert rc == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    ab_images_equal(y, nA, 'a + b')
    want = [_restore(_f32(p, dtype, C) + _f32(q, dtype, C), dtype) for p, q in ((aA, bA), (aB, bB))]
    _exact(y, nA, want[0], want[1], 'a + b', C if dtype == 'bf16x3' else None)
    del a, b, y, ybuf
    _free()


@pytest.mark.parametrize('dtype,line', MOVE, ids=MOVE_IDS)
def test_dilate2x_across_the_line(lib, cuda, dtype, line):
    """yolo_dilate2x: the dilated tensor past the line, zeros written and values moved as stored."""
    C, (Ho, Wo) = 8, (H0 // 2, W0 // 2)
    rng = np.random.default_rng(line + 1)
    (sA, _), (sB, _) = _rand(rng, (Ho, Wo, C), dtype), _rand(rng, (Ho, Wo, C), dtype)
    want = []
    for s in (sA, sB):
        w = torch.zeros((H0, W0) + tuple(s.shape[2:]), dtype=s.dtype)
        w[::2, ::2] = s
        want.append(w)
    nA, nB = ab_counts(line, _image_bytes(want[0]))
    src = ab_tensor(sA, sB, nA, nB, cuda)[1]
    dbuf, d = guarded((nA + nB,) + tuple(want[0].shape), want[0].dtype, cuda)
    assert d.numel() * d.element_size() > 1 << line
    assert lib.yolo_dilate2x(src.data_ptr(), d.data_ptr(), nA + nB, H0, W0, Ho, Wo, C, LDT[dtype], _st()) == 0
    torch.cuda.synchronize()
    guards_intact(dbuf, d)
    ab_images_equal(d, nA, 'dilated')
    _exact(d, nA, want[0], want[1], 'dilated', C if dtype == 'bf16x3' else None)
    del src, d, dbuf
    _free()


@pytest.mark.parametrize('dtype,line', MOVE, ids=MOVE_IDS)
def test_upsample2x_concat_across_the_line(lib, cuda, dtype, line):
    """yolo_upsample2x_concat: 8 + 8 channels, the concatenated tensor past the line; 16-byte units copied as they are."""
    C1 = C2 = 8
    rng = np.random.default_rng(line + 2)
    ups = [_rand(rng, (H0 // 2, W0 // 2, C1), dtype)[0] for _ in 'AB']
    routes = [_rand(rng, (H0, W0, C2), dtype)[0] for _ in 'AB']
    want = []
    for u, r in zip(ups, routes):
        u2 = u.repeat_interleave(2, 0).repeat_interleave(2, 1)
        if dtype == 'bf16x3':
            w = torch.zeros((H0, W0, 2, _cp(C1 + C2)), dtype=u.dtype)
            w[..., :C1], w[..., C1:C1 + C2] = u2[..., :C1], r[..., :C2]
        else:
            w = torch.cat([u2, r], -1)
        want.append(w)
    nA, nB = ab_counts(line, _image_bytes(want[0]))
    up, route = ab_tensor(ups[0], ups[1], nA, nB, cuda)[1], ab_tensor(routes[0], routes[1], nA, nB, cuda)[1]
    ybuf, y = guarded((nA + nB,) + tuple(want[0].shape), want[0].dtype, cuda)
    assert y.numel() * y.element_size() > 1 << line
    assert lib.yolo_upsample2x_concat(up.data_ptr(), route.data_ptr(), y.data_ptr(), nA + nB, H0, W0, C1, C2, LDT[dtype], _st()) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    ab_images_equal(y, nA, 'concatenated')
    _exact(y, nA, want[0], want[1], 'concatenated', C1 + C2 if dtype == 'bf16x3' else None)
    del up, route, y, ybuf
    _free()


@pytest.mark.parametrize('dtype,line,acc', [pytest.param(d, l, a, id='%s-2^%d-%s' % (d, l, 'accumulating' if a else 'fresh'))
                                            for d, l in MOVE for a in (0, 1) if not (l == 32 and a)])
def test_upsample2x_concat_bwd_across_the_line(lib, cuda, dtype, line, acc):
    """yolo_upsample2x_concat_bwd: dcat past the line (2^32: fresh only); ((d00 + d01) + d10) + d11 in fp32, then old + s when
    accumulating, one rounding."""
    C1 = C2 = 8
    rng = np.random.default_rng(line + 3 + acc)
    cats = [_rand(rng, (H0, W0, C1 + C2), dtype)[0] for _ in 'AB']
    up0 = [_rand(rng, (H0 // 2, W0 // 2, C1), dtype)[0] for _ in 'AB']
    ro0 = [_rand(rng, (H0, W0, C2), dtype)[0] for _ in 'AB']
    wu, wr = [], []
    for cs, u0, r0 in zip(cats, up0, ro0):
        d = _f32(cs, dtype, C1 + C2)
        s = ((d[0::2, 0::2, :C1] + d[0::2, 1::2, :C1]) + d[1::2, 0::2, :C1]) + d[1::2, 1::2, :C1]
        r = d[..., C1:]
        if acc:
            s, r = _f32(u0, dtype, C1) + s, _f32(r0, dtype, C2) + r
        wu.append(_restore(s, dtype))
        wr.append(_restore(r.contiguous(), dtype))
    nA, nB = ab_counts(line, _image_bytes(cats[0]))
    dcat = ab_tensor(cats[0], cats[1], nA, nB, cuda)[1]
    assert dcat.numel() * dcat.element_size() > 1 << line
    ubuf, dup = guarded((nA + nB,) + tuple(up0[0].shape), up0[0].dtype, cuda)
    rbuf, dro = guarded((nA + nB,) + tuple(ro0[0].shape), ro0[0].dtype, cuda)
    if acc:
        dup[:nA], dup[nA:] = up0[0].to(cuda), up0[1].to(cuda)
        dro[:nA], dro[nA:] = ro0[0].to(cuda), ro0[1].to(cuda)
        if dtype == 'bf16x3':                            # (the pads of an accumulated-into tensor are not read or written: poison them again)
            bits_of(dup)[..., C1:] = -1
            bits_of(dro)[..., C2:] = -1
    assert lib.yolo_upsample2x_concat_bwd(dcat.data_ptr(), dup.data_ptr(), dro.data_ptr(), nA + nB, H0, W0, C1, C2, acc, acc,
                                          LDT[dtype], _st()) == 0
    torch.cuda.synchronize()
    guards_intact(ubuf, dup)
    guards_intact(rbuf, dro)
    ab_images_equal(dup, nA, 'dup')
    ab_images_equal(dro, nA, 'droute')
    _exact(dup, nA, wu[0], wu[1], 'dup', C1 if dtype == 'bf16x3' else None)
    _exact(dro, nA, wr[0], wr[1], 'droute', C2 if dtype == 'bf16x3' else None)
    del dcat, dup, dro, ubuf, rbuf
    _free()


@pytest.mark.parametrize('dtype,line', MOVE, ids=MOVE_IDS)
def test_gather_rows_across_the_line(lib, cuda, dtype, line):
    """yolo_gather_rows: the strided fp32 source (37 of 40 rows of 45 floats per batch, 30 of them gathered) past the line."""
    rows, extra, rs, C, Cpad = 37, 3, 45, 30, 32
    rng = np.random.default_rng(line + 4)
    srcs = [torch.from_numpy(rng.standard_normal((rows + extra, rs)).astype(np.float32)) for _ in 'AB']
    want = []
    for s in srcs:
        v = torch.zeros((rows, Cpad))
        v[:, :C] = s[:rows, :C]
        want.append(_restore(v, dtype))
    nA, nB = ab_counts(line, _image_bytes(srcs[0]))
    src = ab_tensor(srcs[0], srcs[1], nA, nB, cuda)[1]
    assert src.numel() * 4 > 1 << line
    dbuf, dst = guarded((nA + nB,) + tuple(want[0].shape), want[0].dtype, cuda)
    assert lib.yolo_gather_rows(src.data_ptr(), dst.data_ptr(), nA + nB, rows, C, Cpad, (rows + extra) * rs, rs, LDT[dtype], _st()) == 0
    torch.cuda.synchronize()
    guards_intact(dbuf, dst)
    ab_images_equal(dst, nA, 'gathered rows')
    _exact(dst, nA, want[0], want[1], 'gathered rows', Cpad if dtype == 'bf16x3' else None)
    del src, dst, dbuf
    _free()


@pytest.mark.parametrize('dtype,line', MOVE, ids=MOVE_IDS)
def test_bias_grad_across_the_line(lib, cuda, dtype, line):
    """yolo_bias_grad: column sums of dy past the line, added to an existing db, against float64 at the bar of test_bias_grad -- the
    blocks of 64 pixels add their fp32 partial sums with one fp32 atomic each.  A is positive and B negative, so a sum over the
    wrong images is off by a large part of sum|v|."""
    C = 64
    rng = np.random.default_rng(line + 5)
    (sA, vA), (sB, vB) = (_store((sign * rng.uniform(.5, 1.5, (H0, W0, C))).astype(np.float32), dtype) for sign in (1, -1))
    nA, nB = ab_counts(line, _image_bytes(sA))
    dy = ab_tensor(sA, sB, nA, nB, cuda)[1]
    assert dy.numel() * dy.element_size() > 1 << line
    npix = (nA + nB) * H0 * W0
    db0 = rng.standard_normal(C).astype(np.float32)
    dbuf, db = guarded((C,), torch.float32, cuda, prior=torch.from_numpy(db0).to(cuda))
    assert lib.yolo_bias_grad(dy.data_ptr(), db.data_ptr(), npix, C, 0, LDT[dtype], _st()) == 0
    torch.cuda.synchronize()
    guards_intact(dbuf, db)
    want = db0.astype(np.float64) + (nA * vA.sum((0, 1)) + nB * vB.sum((0, 1))).numpy()
    mag = (nA * vA.abs().sum((0, 1)) + nB * vB.abs().sum((0, 1))).numpy()
    bar = (64 + -(-npix // 64) + 1) * 2.0 ** -24 * (np.abs(db0) + mag)
    err = np.abs(db.cpu().numpy().astype(np.float64) - want)
    print('bias_grad %s: worst error / bar %.3g, bar / sum|v| %.3g' % (dtype, (err / bar).max(), (bar / mag).max()))
    assert (err <= bar).all()
    assert (bar < 0.1 * mag).all()                       # (a sum that took B for A, or A for B, is off by more than that)
    del dy
    _free()


@pytest.mark.parametrize('dtype,line', MOVE, ids=MOVE_IDS)
def test_nchw_to_nhwc_across_the_line(lib, cuda, dtype, line):
    """yolo_nchw_to_nhwc: 3 planes of fp32 -> 8-channel pixels of `dtype`; the output passes the line."""
    C = 3
    rng = np.random.default_rng(line + 6)
    xs = [torch.from_numpy(rng.standard_normal((C, H0, W0)).astype(np.float32)) for _ in 'AB']
    want = []
    for x in xs:
        v = torch.zeros((H0, W0, 8))
        v[..., :C] = x.permute(1, 2, 0)
        want.append(_restore(v, dtype))
    nA, nB = ab_counts(line, _image_bytes(want[0]))
    x = ab_tensor(xs[0], xs[1], nA, nB, cuda)[1]
    ybuf, y = guarded((nA + nB,) + tuple(want[0].shape), want[0].dtype, cuda)
    assert y.numel() * y.element_size() > 1 << line
    assert lib.yolo_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), nA + nB, C, H0, W0, 8, LDT[dtype], _st()) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    ab_images_equal(y, nA, 'nhwc')
    _exact(y, nA, want[0], want[1], 'nhwc', 8 if dtype == 'bf16x3' else None)
    del x, y, ybuf
    _free()


@pytest.mark.parametrize('dtype,line', [m for m in MOVE if m[0] != 'bf16x3'], ids=[i for i in MOVE_IDS if 'x3' not in i])
def test_nhwc_to_nchw_across_the_line(lib, cuda, dtype, line):
    """yolo_nhwc_to_nchw (f32, bf16: it refuses the split types): the fp32 planes pass the line; exact widening."""
    C = 8
    rng = np.random.default_rng(line + 7)
    xs = [_rand(rng, (H0, W0, C), dtype)[0] for _ in 'AB']
    want = [x.float().permute(2, 0, 1).contiguous() for x in xs]
    nA, nB = ab_counts(line, _image_bytes(want[0]))
    x = ab_tensor(xs[0], xs[1], nA, nB, cuda)[1]
    ybuf, y = guarded((nA + nB,) + tuple(want[0].shape), torch.float32, cuda)
    assert y.numel() * 4 > 1 << line
    assert lib.yolo_nhwc_to_nchw(x.data_ptr(), y.data_ptr(), nA + nB, C, H0, W0, LDT[dtype], _st()) == 0
    torch.cuda.synchronize()
    guards_intact(ybuf, y)
    ab_images_equal(y, nA, 'nchw')
    _exact(y, nA, want[0], want[1], 'nchw')
    del x, y, ybuf
    _free()
