"""The DenseNet kernels (csrc/dense.hip), the OCR reading rule (csrc/ocr.hip) and the nets built on them against tests/dense_ref.py.

Tolerances are MEASURED, not fixed: e(a, b) = max|a - b| / max|b|;
  f32 path   e(kernel, ref64) <= 8 x e(ref32, ref64)     both sides are float32 roundings summed in another order; a wrong border,
                                                         channel or offset is wrong by the activations' own size
  bf16 path  e(kernel, ref32) <= 2 x e(bf16-emulated, ref32)
For a single entry the emulation rounds where the kernel rounds (dense_ref.Mode(kernel_points=True)).  Every test prints what it
measured (pytest -s).  Buffers are surrounded by NaN guard bands and pre-filled with NaN wherever the entry must not read or write.
"""
import numpy as np
import pytest
import torch

import dense_ref as R
from yolo_amd import dense as D
from yolo_amd import lib as L
from yolo_amd.dense import LPDenseNet, OCRNet, PlateReader

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'f32': torch.float32}
LDT = {'bf16': L.BF16, 'f32': L.F32}
GUARD = 4096


def guarded(shape, tdt, dev):
    """A NaN-filled tensor of `shape` inside a NaN guard band: (whole flat buffer, view)."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), float('nan'), dtype=tdt, device=dev)
    return flat, flat[GUARD:GUARD + n].view(shape)


def guards_intact(flat):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())


def folded(lib, P, name, c, dev):
    cp = lib.yolo_padded_channels(c)
    s, t = torch.empty(cp, device=dev), torch.empty(cp, device=dev)
    g, b, m, v = (P['%s.%s' % (name, f)].to(dev).contiguous() for f in R.BN_FIELDS)
    assert lib.yolo_fold_bn(L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), 1e-5, L.ptr(s), L.ptr(t), c, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    return s, t


def check(kernel, dtype, ref64, ref32, emu, what):
    """The tolerance rule of the module docstring; kernel and references as CPU tensors of one shape."""
    kernel = kernel.double().cpu()
    assert bool(torch.isfinite(kernel).all()), what
    if dtype == 'f32':
        got, base = R.rel_err(kernel, ref64), R.rel_err(ref32, ref64)
        print('%s f32: e(kernel, ref64) %.3e   e(ref32, ref64) %.3e' % (what, got, base))
        assert got <= 8 * base, (what, got, base)
    else:
        got, base = R.rel_err(kernel, ref32), R.rel_err(emu, ref32)
        print('%s bf16: e(kernel, ref32) %.3e   e(emulated, ref32) %.3e' % (what, got, base))
        assert got <= 2 * base, (what, got, base)
    return got


def stored(t, dtype):
    """t as the buffer's element type holds it, back in float32."""
    return t.to(TDT[dtype]).float()


# ---- yolo_dense_layer_fwd ----------------------------------------------------------------------------------------------------------
LAYERS = [(32, 48, 12), (44, 48, 12), (386 - 12, 48, 12), (72, 64, 16), (504, 64, 16),
          (45, 48, 12),            # odd Cin (a transition's C // 2 can be odd): element-wise stores
          (98, 48, 12),            # Cin % 4 == 2, OCRNet's third block: 4-byte stores on bf16
          (40, 128, 32)]           # the largest bottleneck and two tiles of new channels


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('hw', [(5, 7), (11, 13)])            # smaller than a tile and odd; two tiles wide and high
@pytest.mark.parametrize('cin,cm,g', LAYERS)
def test_dense_layer(lib, cuda, cin, cm, g, hw, dtype):
    N, (H, W) = 2, hw
    Cs = D.round_up(cin + g, 32) + 32                         # channels beyond Cin + G exist and must stay untouched
    shapes = {}
    pre = 'stage1.layer0.'
    for f in R.BN_FIELDS:
        shapes[pre + 'bn1.' + f], shapes[pre + 'bn2.' + f] = (cin,), (cm,)
    shapes[pre + 'conv1.weight'], shapes[pre + 'conv2.weight'] = (cm, cin, 1, 1), (g, cm, 3, 3)
    P = R.random_params(shapes, cin + 7 * cm)
    t2_positive = (cin, hw) == (44, (5, 7))                    # the case where padding m instead of b is wrong by the activations
    if t2_positive:
        P[pre + 'bn2.beta'] = P[pre + 'bn2.beta'].abs() + 2.0 + (P[pre + 'bn2.running_mean'] / torch.sqrt(P[pre + 'bn2.running_var'])).abs() * 1.5
        assert float(R.fold(P, pre + 'bn2', R.Mode('f32'))[1].min()) > 0
    x = stored(torch.randn((N, cin, H, W), generator=torch.Generator().manual_seed(cin)), dtype)
    flat, buf = guarded((N, H, W, Cs), TDT[dtype], cuda)
    buf[..., :cin] = x.permute(0, 2, 3, 1).to(cuda).to(TDT[dtype])
    before = buf[..., :cin].clone()
    s1, t1 = folded(lib, P, pre + 'bn1', cin, cuda)
    s2, t2 = folded(lib, P, pre + 'bn2', cm, cuda)
    w1 = D.pack_operand(P[pre + 'conv1.weight'].reshape(cm, cin).to(cuda), TDT[dtype])
    w2 = D.pack_operand(D.conv3_matrix(P[pre + 'conv2.weight'].to(cuda)), TDT[dtype])
    assert w1.numel() * w1.element_size() == lib.yolo_dense_operand_bytes(cm, cin, LDT[dtype])
    assert w2.numel() * w2.element_size() == lib.yolo_dense_operand_bytes(g, 9 * D.round_up(cm, 32), LDT[dtype])
    rc = lib.yolo_dense_layer_fwd(L.ptr(buf), L.ptr(w1), L.ptr(s1), L.ptr(t1), L.ptr(w2), L.ptr(s2), L.ptr(t2), N, H, W, Cs, cin, cm, g,
                                  LDT[dtype], L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(flat)
    assert torch.equal(buf[..., :cin].view(torch.int16 if dtype == 'bf16' else torch.int32), before.view(torch.int16 if dtype == 'bf16' else torch.int32))
    assert bool(torch.isnan(buf[..., cin + g:]).all())
    got = buf[..., cin:cin + g].float().cpu().permute(0, 3, 1, 2)
    new = lambda mode: R.dense_layer(x.to(mode.dtype), P, pre, mode)[:, cin:]
    check(got, dtype, new(R.Mode('f64')), new(R.Mode('f32')), new(R.Mode('bf16', True)),
          'dense_layer Cin %d Cm %d G %d %dx%d%s' % (cin, cm, g, H, W, ' t2>0' if t2_positive else ''))


# ---- yolo_dense_transition_fwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('c,hw', [(104, (6, 8)), (196, (7, 9)), (98, (5, 12)), (520, (4, 7))])
def test_transition(lib, cuda, c, hw, dtype):
    N, (H, W) = 2, hw
    shapes = {'trans1.conv.weight': (c // 2, c, 1, 1)}
    for f in R.BN_FIELDS:
        shapes['trans1.bn.' + f] = (c,)
    P = R.random_params(shapes, c)
    x = stored(torch.randn((N, c, H, W), generator=torch.Generator().manual_seed(c + 1)), dtype)
    Cs_in, Cs_out = D.round_up(c, 32), D.round_up(c // 2 + 24, 32)
    fin, bin_ = guarded((N, H, W, Cs_in), TDT[dtype], cuda)
    bin_[..., :c] = x.permute(0, 2, 3, 1).to(cuda).to(TDT[dtype])
    fout, bout = guarded((N, H // 2, W // 2, Cs_out), TDT[dtype], cuda)
    s, t = folded(lib, P, 'trans1.bn', c, cuda)
    w = D.pack_operand(P['trans1.conv.weight'].reshape(c // 2, c).to(cuda), TDT[dtype])
    rc = lib.yolo_dense_transition_fwd(L.ptr(bin_), L.ptr(w), L.ptr(s), L.ptr(t), L.ptr(bout), N, H, W, c, Cs_in, Cs_out, LDT[dtype],
                                       L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(fin) and guards_intact(fout)
    assert bool(torch.isnan(bout[..., c // 2:]).all())
    got = bout[..., :c // 2].float().cpu().permute(0, 3, 1, 2)
    ref = lambda mode: R.transition(x.to(mode.dtype), P, 'trans1', mode)
    assert tuple(got.shape) == tuple(ref(R.Mode('f32')).shape) == (N, c // 2, H // 2, W // 2)
    check(got, dtype, ref(R.Mode('f64')), ref(R.Mode('f32')), ref(R.Mode('bf16', True)), 'transition C %d %dx%d' % (c, H, W))


# ---- yolo_dense_stem_fwd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('f0,hw', [(16, (21, 37)), (32, (70, 44)), (64, (22, 19))])      # odd conv maps: the pool's last window hangs over
def test_stem(lib, cuda, f0, hw, dtype):
    N, (H, W) = 2, hw
    shapes = {'stem.weight': (f0, 3, 7, 7)}
    for f in R.BN_FIELDS:
        shapes['stem.' + f] = (f0,)
    P = R.random_params(shapes, f0)
    x = torch.rand((N, 3, H, W), generator=torch.Generator().manual_seed(f0 + 2))
    Hp, Wp = D.stem_out_hw(H, W)
    assert ((H - 1) // 2 + 1) % 2 == 1 or ((W - 1) // 2 + 1) % 2 == 1
    Cs = D.round_up(f0 + 8, 32)
    flat, buf = guarded((N, Hp, Wp, Cs), TDT[dtype], cuda)
    s, t = folded(lib, P, 'stem', f0, cuda)
    xd, wd = x.to(cuda), P['stem.weight'].to(cuda).contiguous()
    rc = lib.yolo_dense_stem_fwd(L.ptr(xd), L.ptr(wd), L.ptr(s), L.ptr(t), L.ptr(buf), N, H, W, f0, Cs, LDT[dtype], L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(flat) and bool(torch.isnan(buf[..., f0:]).all())
    got = buf[..., :f0].float().cpu().permute(0, 3, 1, 2)
    ref = lambda mode: R.stem(x.to(mode.dtype), P, mode)
    assert tuple(got.shape) == tuple(ref(R.Mode('f32')).shape)
    check(got, dtype, ref(R.Mode('f64')), ref(R.Mode('f32')), ref(R.Mode('bf16', True)), 'stem F0 %d %dx%d' % (f0, H, W))


# ---- yolo_dense_bn_relu ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('columns', [0, 1])
def test_bn_relu_layouts(lib, cuda, columns, dtype):
    N, H, W, Cc, Cs, Cp = 2, 3, 9, 50, 96, 64
    shapes = {'final.bn.' + f: (Cc,) for f in R.BN_FIELDS}
    P = R.random_params(shapes, 11)
    x = stored(torch.randn((N, Cc, H, W), generator=torch.Generator().manual_seed(12)), dtype)
    fin, bin_ = guarded((N, H, W, Cs), TDT[dtype], cuda)
    bin_[..., :Cc] = x.permute(0, 2, 3, 1).to(cuda).to(TDT[dtype])
    fout, out = guarded((N, 1, W, H * Cp) if columns else (N, H, W, Cp), TDT[dtype], cuda)
    s, t = folded(lib, P, 'final.bn', Cc, cuda)
    rc = lib.yolo_dense_bn_relu(L.ptr(bin_), L.ptr(s), L.ptr(t), L.ptr(out), N, H, W, Cc, Cs, Cp, columns, LDT[dtype], L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(fin) and guards_intact(fout)
    got = out.float().cpu()
    if columns:
        got = got.view(N, W, H, Cp).permute(0, 2, 1, 3)       # [n][0][w][h * Cp + c] -> (N, H, W, Cp)
    assert bool((got[..., Cc:] == 0).all())                    # the pad channels are zeros, not NaN
    got = got[..., :Cc].permute(0, 3, 1, 2)
    ref = lambda mode: R.bn_relu(x.to(mode.dtype), P, 'final.bn', mode)
    check(got, dtype, ref(R.Mode('f64')), ref(R.Mode('f32')), ref(R.Mode('bf16', True)), 'bn_relu columns %d' % columns)


# ---- yolo_ocr_decode ---------------------------------------------------------------------------------------------------------------
def _z(p):
    return float(np.log(p / (1 - p)))


def _crafted():
    """(N, W', 1 + ncls) logits; every sigmoid at least 1e-3 from the thresholds 0.6 / 0.2 and from its neighbours unless equal on purpose."""
    ncls = 6
    rows = [
        [0.90, 0.30, 0.70, 0.70, 0.10, 0.65, 0.61, 0.30, 0.50, 0.80],       # peaks at 0 and W' - 1; equal neighbours 2, 3: neither
        [0.10, 0.75, 0.75, 0.75, 0.15, 0.25, 0.21, 0.19, 0.30, 0.05],       # a plateau 1..3: no peak; 5 and 8 only under thr 0.2
        [0.95, 0.94, 0.93, 0.92, 0.91, 0.90, 0.89, 0.88, 0.87, 0.86],       # monotone: only column 0
        [0.55, 0.59, 0.58, 0.62, 0.61, 0.15, 0.18, 0.17, 0.22, 0.21],
    ]
    lg = np.zeros((len(rows), 10, 1 + ncls), np.float32)
    rng = np.random.default_rng(5)
    lg[:, :, 1:] = rng.permutation(ncls * 40).reshape(4, 10, ncls)[:, :, :] * 0.25       # distinct class logits
    for n, r in enumerate(rows):
        lg[n, :, 0] = [_z(p) for p in r]
    lg[0, 0, 1:] = [1.0, 3.0, 3.0, -1.0, 3.0, 0.0]            # class ties: the first index wins
    lg[0, 9, 1:] = 2.0                                        # all equal: class 0
    return lg, ncls


@pytest.mark.parametrize('thr', [0.6, 0.2])
def test_ocr_decode_crafted(lib, cuda, thr):
    lg, ncls = _crafted()
    N, Wp = lg.shape[:2]
    d = torch.from_numpy(lg).to(cuda)
    valid = torch.tensor([1, 1, 0, 1], dtype=torch.uint8, device=cuda)
    for v in (None, valid):
        score = torch.full((N, Wp), -1.0, device=cuda)
        codes = torch.full((N, Wp), -7, dtype=torch.int32, device=cuda)
        count = torch.full((N,), -7, dtype=torch.int32, device=cuda)
        assert lib.yolo_ocr_decode(L.ptr(d), L.ptr(v), L.ptr(score), L.ptr(codes), L.ptr(count), N, Wp, ncls, thr, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        for n in range(N):
            s, c = R.read_columns(lg[n], thr)
            if v is not None and int(valid[n]) == 0:
                c = np.full_like(c, -1)
            assert np.abs(score[n].cpu().numpy() - s).max() <= 1e-6
            assert codes[n].cpu().tolist() == c.tolist(), (n, thr)
            assert int(count[n]) == int((c >= 0).sum())
    s0, c0 = R.read_columns(lg[0], thr)
    assert c0[0] == 1 and c0[9] == 0 and c0[2] == c0[3] == -1                # the crafted properties themselves
    assert (R.read_columns(lg[1], thr)[1][1:4] == -1).all()
    assert (R.read_columns(lg[1], 0.2)[1] >= 0).sum() > (R.read_columns(lg[1], 0.6)[1] >= 0).sum()


def test_ocr_decode_many_columns(lib, cuda):
    """More columns than one pass of the block's threads."""
    rng = np.random.default_rng(9)
    N, Wp, ncls = 3, 700, 5
    lg = np.round(rng.standard_normal((N, Wp, 1 + ncls)) * 8).astype(np.float32) / 4       # coarse values: exact ties do occur
    d = torch.from_numpy(lg).to(cuda)
    score = torch.empty((N, Wp), device=cuda)
    codes = torch.empty((N, Wp), dtype=torch.int32, device=cuda)
    count = torch.empty((N,), dtype=torch.int32, device=cuda)
    assert lib.yolo_ocr_decode(L.ptr(d), None, L.ptr(score), L.ptr(codes), L.ptr(count), N, Wp, ncls, 0.6, L.stream_ptr()) == 0
    for n in range(N):
        # (equal neighbours are equal float32 sigmoids too: the same logit; the 0.6 threshold lies between two grid values)
        s, c = R.read_columns(lg[n], 0.6)
        assert codes[n].cpu().tolist() == c.tolist() and int(count[n]) == int((c >= 0).sum())


# ---- whole nets ----------------------------------------------------------------------------------------------------------------------
def band_image(N, size, seed, band=16):
    """High-contrast vertical bands, one per score column, plus a little noise: the columns of a random net then differ."""
    g = torch.Generator().manual_seed(seed)
    low = (torch.rand((N, 3, 1, -(-size[1] // band)), generator=g) > 0.5).float()
    x = low.repeat_interleave(band, dim=3)[..., :size[1]].expand(N, 3, size[0], size[1])
    return (0.9 * x + 0.1 * torch.rand((N, 3) + tuple(size), generator=g)).clamp(0, 1).contiguous()


def level_image(N, size, seed, band=16):
    """Grey vertical bands, one per score column, of four levels with no two neighbours alike, plus a little noise.
    -> (image (N, 3, H, W), level (N, bands) in 0..3)."""
    g = torch.Generator().manual_seed(seed)
    nb = -(-size[1] // band)
    level = torch.zeros((N, nb), dtype=torch.long)
    for n in range(N):
        prev = -1
        for i in range(nb):
            k = int(torch.randint(0, 4, (1,), generator=g))
            while k == prev:
                k = int(torch.randint(0, 4, (1,), generator=g))
            level[n, i] = prev = k
    low = torch.tensor([0.0, 0.3, 0.7, 1.0])[level].view(N, 1, 1, nb).expand(N, 3, 1, nb)
    x = low.repeat_interleave(band, dim=3)[..., :size[1]].expand(N, 3, size[0], size[1])
    return (0.9 * x + 0.1 * torch.rand((N, 3) + tuple(size), generator=g)).clamp(0, 1).contiguous(), level


_CASES = {}


def ocr_case(name):
    """Parameters, input and the three references of a net, computed once on the CPU and shared.  The nets are random up to their
    last convolution, which dense_ref.craft_reading fits on the CPU to the grey levels of the input's bands (see there).  The seeds
    were chosen on the CPU such that the float32 reference's logits are neither constant nor saturated (the checks below state it)
    and that its reading is decided by margins well above the bf16 EMULATION's error: with margins > 2 e max|logit| the full net
    leaves 1 of 48 columns out at e = that error and at twice it, 2 at four times; the micro net 2, 2 and 6 of 74."""
    if name not in _CASES:
        if name == 'ocr':
            net, head, size, seed = dict(F0=32, G=12, blocks=[6, 12, 24], bn_size=4), ('ocr', 10, 34), (160, 384), 6
        else:       # OCR-shaped, odd maps 13 x 151, 6 x 75, 3 x 37
            net, head, size, seed = dict(F0=16, G=8, blocks=[2, 3, 2], bn_size=4), ('ocr', 3, 34), (52, 602), MICRO_SEED
        shapes = D.dense_param_shapes(net['F0'], net['G'], net['blocks'], 4, head)
        P = R.random_params(shapes, seed)
        x, level = level_image(2, size, seed + 100)
        R.craft_reading(net, P, x, level, seed, head[2])
        refs = {m: R.ocr_forward(net, P, x, R.Mode(m)) for m in ('f64', 'f32', 'bf16')}
        lg = refs['f32']
        score = torch.sigmoid(lg[..., 0])
        print('%s: std of the score logits %.2f, of the class logits %.2f' % (name, float(lg[..., 0].std()), float(lg[..., 1:].std())))
        assert float(lg[..., 0].std()) > 0.5 and float(lg[..., 1:].std()) > 0.3            # not constant
        assert 0.02 < float(score.min()) and float(score.max()) < 0.98 and float(lg.abs().max()) < 30     # not saturated
        _CASES[name] = (net, head, size, P, x, refs)
    return _CASES[name]


MICRO_SEED = 6


def build_ocr(name, dtype, cuda):
    net, head, size, P, x, refs = ocr_case(name)
    m = OCRNet(classes=head[2], num_init_features=net['F0'], growth_rate=net['G'], block_config=net['blocks'], size=size, dtype=dtype,
               device=cuda).load_params(P)
    return m, x.to(cuda), refs


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('name', ['ocr', 'micro'])
def test_ocr_net(cuda, name, dtype):
    m, x, refs = build_ocr(name, dtype, cuda)
    score_x, class_x = m(x)
    torch.cuda.synchronize()
    W_ = refs['f32'].shape[2]
    assert tuple(score_x.shape) == (2, 1, W_, 1) and tuple(class_x.shape) == (2, 1, W_, 34) and score_x.dtype == torch.float32
    got = torch.cat([score_x, class_x], -1).cpu()
    check(got, dtype, refs['f64'], refs['f32'], refs['bf16'], 'OCRNet %s' % name)
    assert m.launches <= sum(m.block_config) + len(m.block_config) - 1 + 8 - 1
    with pytest.raises(ValueError):
        m(x.permute(0, 1, 3, 2))                                 # not contiguous: refused, not copied
    # nothing is allocated after the first call with a shape, and a second call gives the same bits
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = torch.cat(m(x), -1)
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), got)
    del again
    assert torch.cuda.memory_allocated() <= before


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_lpd_net(cuda, dtype):
    spec = dict(num_init_features=16, growth_rate=8, block_config=[2, 3, 2, 2], LP_num_class=3)
    net = dict(F0=16, G=8, blocks=[2, 3, 2, 2], bn_size=4)
    P = R.random_params(D.dense_param_shapes(16, 8, [2, 3, 2, 2], 4, ('lpd', 3)), 21)
    x = band_image(2, (64, 96), 22, band=8)
    refs = {m: R.lpd_forward(net, P, x, R.Mode(m)) for m in ('f64', 'f32', 'bf16')}
    assert float(refs['f32'].std()) > 0.05
    m = LPDenseNet(spec, dtype=dtype, device=cuda).load_params(P)
    out = m(x.to(cuda))
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(refs['f32'].shape) == (2, 10, 2, 3) and out.dtype == torch.float32
    check(out.cpu(), dtype, refs['f64'], refs['f32'], refs['bf16'], 'LPDenseNet micro')


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_plate_reader_is_the_rule_on_its_own_logits(cuda, dtype):
    m, x, _ = build_ocr('ocr', dtype, cuda)
    for thr in (0.6, 0.2):
        reader = PlateReader(m, threshold=thr)
        texts = reader.read(x)
        lg = m.logits(x).cpu().numpy()
        want = [R.text_of(R.read_columns(lg[n], thr)[1], D.OCR_NAMES) for n in range(lg.shape[0])]
        assert texts == want
        score, codes, count = reader.read_device(x, valid=torch.tensor([0, 1], dtype=torch.uint8, device=cuda))
        assert int(count[0]) == 0 and int(count[1]) == len(want[1]) and bool((codes[0] == -1).all())
    assert any(len(t) > 0 for t in want)
    assert reader.launches <= 42 + 2 + 8


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('name', ['micro', 'ocr'])
def test_decoded_text(cuda, name, dtype):
    """Codes agree with the float32 reference's at every column whose margins (score to threshold, score to both neighbours, top-2
    class gap, all in logits) exceed the measured error of this dtype scaled to logits, and at most 10 % of the columns may be
    left out, on both dtypes.  (The error that sets the margin is the kernel's own, which test_ocr_net holds to twice the
    emulation's: a kernel with more error cannot buy itself a shorter comparison.)"""
    m, x, refs = build_ocr(name, dtype, cuda)
    ref = refs['f32'][:, 0].numpy()
    reader = PlateReader(m, threshold=0.6)
    lg = m.logits(x).cpu().numpy()
    e = R.rel_err(lg, ref)
    _, codes, _ = reader.read_device(x)
    codes = codes.cpu().numpy()
    left_out = 0
    for n in range(ref.shape[0]):
        _, want = R.read_columns(ref[n], 0.6)
        clear = R.column_margins(ref[n], 0.6) > 2 * e * np.abs(ref).max()      # (x 2: both the score and its neighbour move)
        assert (codes[n][clear] == want[clear]).all()
        left_out += int((~clear).sum())
    print('decoded text %s %s: e %.3e, %d of %d columns left out' % (name, dtype, e, left_out, ref.shape[0] * ref.shape[1]))
    assert left_out <= 0.1 * ref.shape[0] * ref.shape[1]
    assert sum(len(R.text_of(R.read_columns(ref[n], 0.6)[1], D.OCR_NAMES)) for n in range(ref.shape[0])) >= 8      # there is a text to read


def test_gluon_params_file_round_trip(cuda, tmp_path):
    m, x, _ = build_ocr('micro', 'bf16', cuda)
    want = torch.cat(m(x), -1).clone()
    path = str(tmp_path / 'micro.params')
    m.save_gluon_params(path)
    m2 = OCRNet(classes=34, num_init_features=16, growth_rate=8, block_config=[2, 3, 2], size=(52, 602), device=cuda).load_gluon_params(path)
    assert torch.equal(torch.cat(m2(x), -1), want)
    m2.initialize(5)                                           # new parameters are re-folded and re-packed before the next call
    assert not torch.equal(torch.cat(m2(x), -1), want)


def test_frame_overlay_feeds_the_reader(cuda):
    import overlay_ref
    from yolo_amd.overlay import FrameOverlay
    N, H, W = 2, 48, 64
    frames = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (N, H, W, 3), dtype=np.uint8)).to(cuda)
    lp = overlay_ref.plate_rows(12, N)
    lp[:, 1:4] = [[30, -20, 900], [-60, 25, 1200]]
    lp[1, 0] = 0.0                                               # the second plate is below the overlay's threshold
    ov = FrameOverlay(camera=overlay_ref.CAMERA, LP_size=(160, 384), device=cuda)
    _, clipped, lp_valid = ov(frames, lp=torch.from_numpy(lp).to(cuda))
    assert tuple(clipped.shape) == (N, 3, 160, 384) and lp_valid.cpu().tolist() == [1, 0]
    m, _, _ = build_ocr('ocr', 'bf16', cuda)
    reader = PlateReader(m)
    texts = reader.read(clipped, lp_valid)
    lg = m.logits(clipped).cpu().numpy()
    assert texts == [R.text_of(R.read_columns(lg[0], 0.6)[1], D.OCR_NAMES), '']
