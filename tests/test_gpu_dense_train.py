"""The train-mode DenseNet forward (csrc/dense_train.hip, DenseNet.forward(training=True)) against tests/dense_train_ref.py.

Tolerances are those of tests/test_gpu_dense.py (its `check`), e(a, b) = max|a - b| / max|b|:
  f32 path   e(kernel, ref64) <= 8 x e(ref32, ref64)
  bf16 path  e(kernel, ref32) <= 2 x e(bf16-emulated with the kernels' rounding points, ref32)
For STATISTICS the rule is applied per array with a floor of 16 * 2^-24 on the f32 bound: the restatement's pairwise two-pass sums can
be closer to float64 than any blocked reduction rounded to float32 needs to be.  The statistics of channels AS STORED are a reduction
of given numbers whatever the buffer's type (the emulation and the float32 restatement of them coincide), so they are judged by the
f32 rule against the float64 statistics of the same stored values on both dtypes.
bf16 is judged hop by hop (one dense layer end to end; every stage of a whole net fed the device's own buffer for the stage before):
a random ReLU net with batch statistics amplifies rounding, as tests/test_gpu_train.py says of the Darknet body, so bf16 is not held
end to end.  Every test prints what it measured (pytest -s).  Outputs sit in NaN guard bands; inputs must keep their bits.

Seeds of the whole-net cases: the 'ocr' and 'micro' cases of test_gpu_dense.py (seed 6 both) and 21 / 22 for the micro LPDenseNet,
for which the float32 restatement of the TRAINING forward lies 1.0e-6 (micro), 1.2e-6 (LPD) and 2.6e-6 (OCRNet) from the float64 one
in the logits, and at most 2.2e-6 in any array of statistics (measured on the CPU, printed by the tests): not erratic.
"""
import pytest
import torch

import dense_ref as R
import dense_train_ref as TR
from test_gpu_dense import LAYERS, LDT, TDT, band_image, check, folded, guarded, guards_intact, ocr_case, stored
from yolo_amd import dense as D
from yolo_amd import lib as L
from yolo_amd.dense import LPDenseNet, OCRNet

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
DTYPES = ['bf16', 'f32']
MAPS = [(1, 1), (5, 7), (11, 13)]       # the smallest population (N = 2); smaller than a tile and odd; two tiles each way, ragged


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_stats(got, ref64, ref32, what):
    """The f32 rule with the floor, for one array of statistics."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    e, base = R.rel_err(got, ref64), R.rel_err(ref32, ref64)
    print('%s: e(kernel, ref64) %.3e   e(ref32, ref64) %.3e' % (what, e, base))
    assert e <= max(8 * base, FLOOR), (what, e, base)


def check_pair(got, dtype, refs, what):
    """(mean, var) from the device against {mode: (mean, var)}: test_gpu_dense.check per array, the floor on the f32 bound."""
    for i, f in enumerate(('mean', 'var')):
        if dtype == 'f32':
            check_stats(got[i], refs['f64'][i], refs['f32'][i], '%s %s f32' % (what, f))
        else:
            check(got[i].cpu(), dtype, refs['f64'][i], refs['f32'][i], refs['bf16'][i], '%s %s' % (what, f))


def workspace(lib, channels, dev):
    n = lib.yolo_dense_stats_workspace_bytes(channels)
    assert n > 0 and n % 8 == 0
    return guarded((n // 8,), torch.float64, dev)


def nan_vec(n, dev):
    return guarded((n,), torch.float32, dev)


class Fold(object):
    """A yolo_bn_batch_fold over fresh device arrays for BatchNorm `name` of P."""

    def __init__(self, lib, P, name, c, dev, momentum=0.9):
        cp = lib.yolo_padded_channels(c)
        self.c = c
        self.gamma, self.beta = P[name + '.gamma'].to(dev).contiguous(), P[name + '.beta'].to(dev).contiguous()
        self.rm, self.rv = P[name + '.running_mean'].to(dev).clone(), P[name + '.running_var'].to(dev).clone()
        self.fs, self.scale = guarded((cp,), torch.float32, dev)
        self.fb, self.bias = guarded((cp,), torch.float32, dev)
        d = self.d = L.BnBatchFold()
        d.gamma, d.beta, d.running_mean, d.running_var = L.ptr(self.gamma), L.ptr(self.beta), L.ptr(self.rm), L.ptr(self.rv)
        d.scale, d.bias, d.C, d.eps, d.momentum = L.ptr(self.scale), L.ptr(self.bias), c, 1e-5, momentum

    def ref(self):
        import ctypes
        return ctypes.byref(self.d)

    def check(self, P, name, mean, var, what, momentum=0.9):
        """scale, bias and the running update against the definition in float64 / float32 on the DEVICE's own mean and var."""
        assert guards_intact(self.fs) and guards_intact(self.fb)
        assert bool((self.scale[self.c:] == 0).all()) and bool((self.bias[self.c:] == 0).all())
        def definition(dt):
            m, v = mean.cpu().to(dt), var.cpu().to(dt)
            s = P[name + '.gamma'].to(dt) / torch.sqrt(v + 1e-5)
            return dict(scale=s, bias=P[name + '.beta'].to(dt) - m * s,
                        rm=momentum * P[name + '.running_mean'].to(dt) + (1.0 - momentum) * m,
                        rv=momentum * P[name + '.running_var'].to(dt) + (1.0 - momentum) * v)
        r64, r32 = definition(torch.float64), definition(torch.float32)
        got = dict(scale=self.scale[:self.c], bias=self.bias[:self.c], rm=self.rm, rv=self.rv)
        for k in ('scale', 'bias', 'rm', 'rv'):
            check_stats(got[k], r64[k], r32[k], '%s fold %s' % (what, k))


def layer_params(cin, cm, g):
    shapes, pre = {}, 'stage1.layer0.'
    for f in R.BN_FIELDS:
        shapes[pre + 'bn1.' + f], shapes[pre + 'bn2.' + f] = (cin,), (cm,)
    shapes[pre + 'conv1.weight'], shapes[pre + 'conv2.weight'] = (cm, cin, 1, 1), (g, cm, 3, 3)
    return R.random_params(shapes, cin + 7 * cm), pre


MODES = {'f64': R.Mode('f64'), 'f32': R.Mode('f32'), 'bf16': R.Mode('bf16', True)}


# ---- yolo_dense_bottleneck_stats -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', MAPS)
@pytest.mark.parametrize('cin,cm,g', LAYERS)
def test_bottleneck_stats(lib, cuda, cin, cm, g, hw, dtype):
    N, (H, W) = 2, hw
    Cs = D.round_up(cin + g, 32) + 32
    P, pre = layer_params(cin, cm, g)
    x = stored(torch.randn((N, cin, H, W), generator=torch.Generator().manual_seed(cin)), dtype)
    flat, buf = guarded((N, H, W, Cs), TDT[dtype], cuda)                  # channels >= Cin stay NaN: they must not reach the sums
    buf[..., :cin] = x.permute(0, 2, 3, 1).to(cuda).to(TDT[dtype])
    before = bits(flat).clone()
    s1, t1 = folded(lib, P, pre + 'bn1', cin, cuda)
    w1 = D.pack_operand(P[pre + 'conv1.weight'].reshape(cm, cin).to(cuda), TDT[dtype])
    fm, mean = nan_vec(cm, cuda)
    fv, var = nan_vec(cm, cuda)
    fw, ws = workspace(lib, cm, cuda)
    rc = lib.yolo_dense_bottleneck_stats(L.ptr(buf), L.ptr(w1), L.ptr(s1), L.ptr(t1), L.ptr(mean), L.ptr(var), L.ptr(ws), None, N, H, W, Cs,
                                         cin, cm, LDT[dtype], L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(fm) and guards_intact(fv) and guards_intact(fw)
    assert torch.equal(bits(flat), before)                                 # no byte of the buffer is written

    def ref(mode):
        s, t = R.fold(P, pre + 'bn1', mode)
        a = mode.r(R.affine_relu(x.to(mode.dtype), s, t))
        return TR.stats(torch.nn.functional.conv2d(a, mode.r(mode.p(P, pre + 'conv1.weight'))))
    check_pair((mean, var), dtype, {k: ref(m) for k, m in MODES.items()}, 'bottleneck Cin %d Cm %d %dx%d' % (cin, cm, H, W))


# ---- yolo_dense_channel_stats ----------------------------------------------------------------------------------------------------
SLICES = [(0, 32), (32, 12), (45, 12), (98, 12), (374, 12), (0, 260)]


def run_channel_stats(lib, cuda, values, c0, dtype):
    """values (N, n, H, W) float32 -> the device's (mean, var) of the slice [c0, c0 + n) of a buffer that is NaN everywhere else."""
    N, n, H, W = values.shape
    Cs = D.round_up(c0 + n, 32) + 32
    flat, buf = guarded((N, H, W, Cs), TDT[dtype], cuda)
    buf[..., c0:c0 + n] = values.permute(0, 2, 3, 1).to(cuda).to(TDT[dtype])
    before = bits(flat).clone()
    fm, mean = nan_vec(Cs, cuda)
    fv, var = nan_vec(Cs, cuda)
    fw, ws = workspace(lib, n, cuda)
    rc = lib.yolo_dense_channel_stats(L.ptr(buf), L.ptr(mean), L.ptr(var), L.ptr(ws), None, N, H, W, Cs, c0, n, LDT[dtype], L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(fm) and guards_intact(fv) and guards_intact(fw) and torch.equal(bits(flat), before)
    for out in (mean, var):                                                # nothing outside [c0, c0 + n) is written
        assert bool(torch.isnan(out[:c0]).all()) and bool(torch.isnan(out[c0 + n:]).all())
    return mean[c0:c0 + n], var[c0:c0 + n]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c0,n,hw', [(c0, n, hw) for c0, n in SLICES for hw in MAPS]
                         + [(45, 12, (100, 200))])                        # 40 000 pixels: many partial rows per channel
def test_channel_stats(lib, cuda, c0, n, hw, dtype):
    N, (H, W) = 2, hw
    g = torch.Generator().manual_seed(c0 + n)
    x = stored(torch.randn((N, n, H, W), generator=g) * (0.5 + torch.rand((1, n, 1, 1), generator=g)) + torch.randn((1, n, 1, 1), generator=g),
               dtype)
    got = run_channel_stats(lib, cuda, x, c0, dtype)
    for i, f in enumerate(('mean', 'var')):
        check_stats(got[i], TR.stats(x.double())[i], TR.stats(x)[i], 'channel stats [%d, %d) %dx%d %s %s' % (c0, c0 + n, H, W, dtype, f))


def test_channel_stats_cancellation(lib, cuda):
    """One channel 50 + 0.1 randn over 40 000 pixels: sums kept in double are good to ~1e-7; a plain float32 E[x^2] - mean^2 would be
    off by mean^2 * 2^-24 / var = 1.5e-2 and more.  The bound 1e-3 separates the two."""
    x = (50.0 + 0.1 * torch.randn((2, 1, 100, 200), generator=torch.Generator().manual_seed(77))).float()
    mean, var = run_channel_stats(lib, cuda, x, 5, 'f32')
    m64, v64 = TR.stats(x.double())
    em, ev = R.rel_err(mean.cpu(), m64), R.rel_err(var.cpu(), v64)
    print('cancellation: mean %.6f var %.6e   relative errors %.3e %.3e' % (float(mean), float(var), em, ev))
    assert ev <= 1e-3 and em <= 1e-6


def _cancellation(what, mean, var, y64):
    """The bars of test_channel_stats_cancellation, per channel, against the float64 statistics of y64 (N, C, H, W); prints what it saw."""
    m64, v64 = TR.stats(y64)
    rho = float((m64 * m64 / v64).min())
    em = float(((mean.double().cpu() - m64).abs() / m64.abs()).max())
    ev = float(((var.double().cpu() - v64).abs() / v64).max())
    print('%s cancellation: rho >= %.2e   relative errors mean %.3e var %.3e' % (what, rho, em, ev))
    assert rho >= 1e5, 'the case is not ill-conditioned'
    assert ev <= 1e-3 and em <= 1e-6


def test_bottleneck_stats_cancellation(lib, cuda):
    """The bottleneck's output 50 + 0.07 noise per channel (rho about 5e5) over 40 000 pixels: input channel 0 is 1 behind an identity
    BN1, its weights are 50, the other weights are small."""
    N, H, W, cin, cm, g = 2, 100, 200, 32, 48, 12
    Cs = D.round_up(cin + g, 32) + 32
    gen = torch.Generator().manual_seed(78)
    x = torch.randn((N, cin, H, W), generator=gen)
    x[:, 0] = 1.0
    w = 0.1 * torch.randn((cm, cin), generator=gen) / cin ** 0.5
    w[:, 0] = 50.0
    flat, buf = guarded((N, H, W, Cs), torch.float32, cuda)
    buf[..., :cin] = x.permute(0, 2, 3, 1).to(cuda)
    cp = lib.yolo_padded_channels(cin)
    s1, t1 = torch.ones(cp, device=cuda), torch.zeros(cp, device=cuda)
    w1 = D.pack_operand(w.to(cuda), torch.float32)
    fm, mean = nan_vec(cm, cuda)
    fv, var = nan_vec(cm, cuda)
    fw, ws = workspace(lib, cm, cuda)
    assert lib.yolo_dense_bottleneck_stats(L.ptr(buf), L.ptr(w1), L.ptr(s1), L.ptr(t1), L.ptr(mean), L.ptr(var), L.ptr(ws), None, N, H, W, Cs,
                                           cin, cm, L.F32, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert guards_intact(fm) and guards_intact(fv) and guards_intact(fw)
    y64 = torch.nn.functional.conv2d(torch.relu(x.double()), w.double().view(cm, cin, 1, 1))
    _cancellation('bottleneck', mean, var, y64)


def test_stem_stats_cancellation(lib, cuda):
    """A flat image 0.5 + 0.002 noise through a stem whose weight sits on the centre tap (taps summing to 2..6 per channel, the rest
    5e-4 noise, so that the padded border stays flat too): rho of the raw output about 1e6."""
    N, H, W, f0 = 2, 100, 200, 16
    gen = torch.Generator().manual_seed(79)
    x = 0.5 + 0.002 * (torch.rand((N, 3, H, W), generator=gen) - 0.5)
    w = 5e-4 * torch.randn((f0, 3, 7, 7), generator=gen)
    w[:, :, 3, 3] += ((2.0 + 4.0 * torch.rand(f0, generator=gen)) / 3.0)[:, None]
    xd, wd = x.to(cuda), w.to(cuda).contiguous()
    fm, mean = nan_vec(f0, cuda)
    fv, var = nan_vec(f0, cuda)
    fw, ws = workspace(lib, f0, cuda)
    assert lib.yolo_dense_stem_stats(L.ptr(xd), L.ptr(wd), L.ptr(mean), L.ptr(var), L.ptr(ws), None, N, H, W, f0, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert guards_intact(fm) and guards_intact(fv) and guards_intact(fw)
    _cancellation('stem', mean, var, torch.nn.functional.conv2d(x.double(), w.double(), stride=2, padding=3))


# ---- yolo_dense_stem_stats -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f0,hw', [(16, (21, 37)), (32, (70, 44)), (64, (22, 19))])
def test_stem_stats(lib, cuda, f0, hw):
    N, (H, W) = 2, hw
    shapes = {'stem.weight': (f0, 3, 7, 7)}
    for f in R.BN_FIELDS:
        shapes['stem.' + f] = (f0,)
    P = R.random_params(shapes, f0)
    x = torch.rand((N, 3, H, W), generator=torch.Generator().manual_seed(f0 + 2))
    xd, wd = x.to(cuda), P['stem.weight'].to(cuda).contiguous()
    xb, wb = bits(xd).clone(), bits(wd).clone()
    fm, mean = nan_vec(f0, cuda)
    fv, var = nan_vec(f0, cuda)
    fw, ws = workspace(lib, f0, cuda)
    fold = Fold(lib, P, 'stem', f0, cuda, momentum=0.75)
    rc = lib.yolo_dense_stem_stats(L.ptr(xd), L.ptr(wd), L.ptr(mean), L.ptr(var), L.ptr(ws), fold.ref(), N, H, W, f0, L.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(fm) and guards_intact(fv) and guards_intact(fw)
    assert torch.equal(bits(xd), xb) and torch.equal(bits(wd), wb)
    raw = lambda dt: TR.stats(torch.nn.functional.conv2d(x.to(dt), P['stem.weight'].to(dt), stride=2, padding=3))
    for i, f in enumerate(('mean', 'var')):
        check_stats((mean, var)[i], raw(torch.float64)[i], raw(torch.float32)[i], 'stem stats F0 %d %dx%d %s' % (f0, H, W, f))
    fold.check(P, 'stem', mean, var, 'stem F0 %d' % f0, momentum=0.75)


# ---- one hop: a train-mode dense layer end to end ------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', [(5, 7), (11, 13)])
@pytest.mark.parametrize('cin,cm,g', LAYERS)
def test_train_layer_hop(lib, cuda, cin, cm, g, hw, dtype):
    """Channel statistics + fold of BN1, bottleneck statistics + fold of BN2, the UNCHANGED yolo_dense_layer_fwd, the statistics of
    the G channels it appended."""
    N, (H, W) = 2, hw
    Cs = D.round_up(cin + g, 32) + 32
    P, pre = layer_params(cin, cm, g)
    x = stored(torch.randn((N, cin, H, W), generator=torch.Generator().manual_seed(cin)) + 0.3, dtype)
    flat, buf = guarded((N, H, W, Cs), TDT[dtype], cuda)
    buf[..., :cin] = x.permute(0, 2, 3, 1).to(cuda).to(TDT[dtype])
    before = bits(buf[..., :cin]).clone()
    w1 = D.pack_operand(P[pre + 'conv1.weight'].reshape(cm, cin).to(cuda), TDT[dtype])
    w2 = D.pack_operand(D.conv3_matrix(P[pre + 'conv2.weight'].to(cuda)), TDT[dtype])
    fbm, bmean = nan_vec(Cs, cuda)
    fbv, bvar = nan_vec(Cs, cuda)
    f2m, mean2 = nan_vec(cm, cuda)
    f2v, var2 = nan_vec(cm, cuda)
    fw, ws = workspace(lib, max(cm, cin), cuda)
    f1, f2 = Fold(lib, P, pre + 'bn1', cin, cuda), Fold(lib, P, pre + 'bn2', cm, cuda)
    st, dt = L.stream_ptr(), LDT[dtype]
    assert lib.yolo_dense_channel_stats(L.ptr(buf), L.ptr(bmean), L.ptr(bvar), L.ptr(ws), f1.ref(), N, H, W, Cs, 0, cin, dt, st) == 0
    assert lib.yolo_dense_bottleneck_stats(L.ptr(buf), L.ptr(w1), L.ptr(f1.scale), L.ptr(f1.bias), L.ptr(mean2), L.ptr(var2), L.ptr(ws),
                                           f2.ref(), N, H, W, Cs, cin, cm, dt, st) == 0
    assert lib.yolo_dense_layer_fwd(L.ptr(buf), L.ptr(w1), L.ptr(f1.scale), L.ptr(f1.bias), L.ptr(w2), L.ptr(f2.scale), L.ptr(f2.bias), N, H,
                                    W, Cs, cin, cm, g, dt, st) == 0
    assert lib.yolo_dense_channel_stats(L.ptr(buf), L.ptr(bmean), L.ptr(bvar), L.ptr(ws), None, N, H, W, Cs, cin, g, dt, st) == 0
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f in (flat, fbm, fbv, f2m, f2v, fw))
    assert torch.equal(bits(buf[..., :cin]), before) and bool(torch.isnan(buf[..., cin + g:]).all())
    assert bool(torch.isnan(bmean[cin + g:]).all()) and bool(torch.isnan(bvar[cin + g:]).all())
    what = 'hop Cin %d Cm %d G %d %dx%d' % (cin, cm, g, H, W)
    refs = {}
    for k, mode in MODES.items():
        tape = TR.Tape(0.9)
        y, (m, v) = TR.dense_layer(x.to(mode.dtype), P, pre, mode, tape)
        refs[k] = dict(new=y[:, cin:], bn2=tape.stats[pre + 'bn2'], tail=(m[cin:], v[cin:]), tape=tape)
    got = buf[..., cin:cin + g].float().cpu().permute(0, 3, 1, 2)
    check(got, dtype, refs['f64']['new'], refs['f32']['new'], refs['bf16']['new'], what + ' new channels')
    check_pair((mean2, var2), dtype, {k: r['bn2'] for k, r in refs.items()}, what + ' BN2')
    check_pair((bmean[cin:cin + g], bvar[cin:cin + g]), dtype, {k: r['tail'] for k, r in refs.items()}, what + ' new statistics')
    # the statistics of the input channels, as stored: a reduction of given numbers on both dtypes
    for i, f in enumerate(('mean', 'var')):
        check_stats((bmean, bvar)[i][:cin], TR.stats(x.double())[i], TR.stats(x)[i], what + ' input ' + f)
    f1.check(P, pre + 'bn1', bmean[:cin], bvar[:cin], what + ' BN1')
    f2.check(P, pre + 'bn2', mean2, var2, what + ' BN2')


# ---- whole nets --------------------------------------------------------------------------------------------------------------------
_TRAIN = {}
NETS = ['micro', 'lpd', 'ocr']


def train_case(name):
    """(kind, net, head, size, P, x, {mode: (output, Tape)} for f64 and f32), computed once on the CPU and shared."""
    if name not in _TRAIN:
        if name == 'lpd':
            net, head, size = dict(F0=16, G=8, blocks=[2, 3, 2, 2], bn_size=4), ('lpd', 3), (64, 96)
            P = R.random_params(D.dense_param_shapes(16, 8, [2, 3, 2, 2], 4, head), 21)
            x, fwd = band_image(2, size, 22, band=8), TR.lpd_forward
        else:
            net, head, size, P, x, _ = ocr_case(name)
            fwd = TR.ocr_forward
        refs = {m: fwd(net, P, x, R.Mode(m)) for m in ('f64', 'f32')}
        print('%s: e(ref32, ref64) of the training logits %.3e' % (name, R.rel_err(refs['f32'][0], refs['f64'][0])))
        ev = (R.lpd_forward if name == 'lpd' else R.ocr_forward)(net, P, x, R.Mode('f64'))
        assert R.rel_err(ev, refs['f64'][0]) > 1e-2                       # an eval-mode answer is visibly wrong
        _TRAIN[name] = (fwd, net, head, size, P, x, refs)
    return _TRAIN[name]


def build(name, dtype, cuda):
    fwd, net, head, size, P, x, refs = train_case(name)
    if name == 'lpd':
        m = LPDenseNet(dict(num_init_features=16, growth_rate=8, block_config=[2, 3, 2, 2], LP_num_class=3), dtype=dtype, device=cuda)
    else:
        m = OCRNet(classes=head[2], num_init_features=net['F0'], growth_rate=net['G'], block_config=net['blocks'], size=size, dtype=dtype,
                   device=cuda)
    return m.load_params(P), x.to(cuda)


def output(m, out):
    return (torch.cat(out, -1) if isinstance(out, list) else out).clone()


@pytest.mark.parametrize('name', NETS)
def test_train_forward_f32(cuda, name):
    fwd, net, head, size, P, x, refs = train_case(name)
    m, xd = build(name, 'f32', cuda)
    xb = bits(xd).clone()
    ev0 = output(m, m(xd))
    static = {k: v.clone() for k, v in m.params.items() if 'running' not in k}
    torch.cuda.synchronize()
    got = output(m, m.forward(xd, training=True))
    torch.cuda.synchronize()
    assert torch.equal(bits(xd), xb)
    assert tuple(got.shape) == tuple(refs['f32'][0].shape) and got.dtype == torch.float32
    check(got.cpu(), 'f32', refs['f64'][0], refs['f32'][0], None, '%s training logits' % name)
    t64, t32 = refs['f64'][1], refs['f32'][1]
    assert sorted(m.batch_stats) == sorted(t64.stats) == sorted(n for n, _ in m.bn_names())
    worst = 0.0
    for bn, c in m.bn_names():
        mean, var = m.batch_stats[bn]
        assert tuple(mean.shape) == tuple(var.shape) == (c,) and mean.dtype == var.dtype == torch.float32
        for i, f in enumerate(('mean', 'var')):
            check_stats((mean, var)[i], t64.stats[bn][i], t32.stats[bn][i], '%s %s batch %s' % (name, bn, f))
        for f in ('running_mean', 'running_var'):
            k = '%s.%s' % (bn, f)
            check_stats(m.params[k], t64.running[k], t32.running[k], '%s %s' % (name, k))
            worst = max(worst, R.rel_err(m.params[k].cpu(), t64.running[k]))
    print('%s: largest running-statistic distance %.3e' % (name, worst))
    for k, v in static.items():                                             # weights, gamma, beta keep their bits
        assert torch.equal(bits(m.params[k]), bits(v)), k
    assert m.train_launches == 5 + 5 * sum(m.block_config) + 3 * (len(m.block_config) - 1) + m._head_launches + 5
    # an inference call re-folds: it differs from the one before and matches the restatement's eval forward with the updated statistics
    ev1 = output(m, m(xd))
    torch.cuda.synchronize()
    assert not torch.equal(ev1, ev0)
    eval_fwd = R.lpd_forward if name == 'lpd' else R.ocr_forward
    check(ev1.cpu(), 'f32', eval_fwd(net, t64.updated(P), x, R.Mode('f64')), eval_fwd(net, t32.updated(P), x, R.Mode('f32')), None,
          '%s inference after the update' % name)
    with pytest.raises(ValueError):
        m.forward(xd.permute(0, 1, 3, 2), training=True)                   # not contiguous: refused in training mode too


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['micro', 'lpd'])
def test_train_forward_is_reproducible_and_allocates_nothing(cuda, name, dtype):
    fwd, net, head, size, P, x, refs = train_case(name)
    m, xd = build(name, dtype, cuda)
    first = output(m, m.forward(xd, training=True))
    stats1 = {k: (a.clone(), b.clone()) for k, (a, b) in m.batch_stats.items()}
    run1 = {k: v.clone() for k, v in m.params.items() if 'running' in k}
    for k in run1:                                                          # the same starting statistics, in place
        m.params[k].copy_(P[k])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = m.forward(xd, training=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= before
    second = output(m, out)
    assert torch.equal(bits(second), bits(first))
    for k, (a, b) in m.batch_stats.items():
        assert torch.equal(bits(a), bits(stats1[k][0])) and torch.equal(bits(b), bits(stats1[k][1])), k
    for k, v in run1.items():
        assert torch.equal(bits(m.params[k]), bits(v)), k
    assert m.forward(xd, training=True) is out and m(xd) is out                # the same output objects as inference


def hop_refs(fn):
    return {k: fn(mode) for k, mode in MODES.items()}


@pytest.mark.parametrize('name', NETS)
def test_train_forward_bf16_hop_by_hop(cuda, name):
    """bf16: finite, the right shapes, and every stage of the restatement fed the DEVICE's own buffer for the stage before."""
    fwd, net, head, size, P, x, refs = train_case(name)
    m, xd = build(name, 'bf16', cuda)
    got = output(m, m.forward(xd, training=True))
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(refs['f32'][0].shape) and bool(torch.isfinite(got).all())
    for bn, c in m.bn_names():
        assert all(tuple(t.shape) == (c,) and bool(torch.isfinite(t).all()) for t in m.batch_stats[bn])
    tb = m.training_buffers(xd)
    nchw = lambda t, c: t[..., :c].float().cpu().permute(0, 3, 1, 2).contiguous()
    F0, G = net['F0'], net['G']
    chans = D.block_channels(F0, G, net['blocks'])
    # the stem: the image is the input
    r = hop_refs(lambda mode: TR.stem(x.to(mode.dtype), P, mode, TR.Tape(0.9)))
    check(nchw(tb['blocks'][0], F0), 'bf16', r['f64'], r['f32'], r['bf16'], '%s stem' % name)
    for s, n in enumerate(net['blocks']):
        buf, cin = tb['blocks'][s], chans[s][0]
        for k in range(n):
            pre = 'stage%d.layer%d.' % (s + 1, k)
            xin = nchw(buf, cin)

            def layer(mode):
                tape = TR.Tape(0.9)
                y, _ = TR.dense_layer(xin.to(mode.dtype), P, pre, mode, tape)
                return y[:, cin:], tape.stats[pre + 'bn2']
            r = hop_refs(layer)
            check(nchw(buf, cin + G)[:, cin:], 'bf16', r['f64'][0], r['f32'][0], r['bf16'][0], '%s %snew channels' % (name, pre))
            check_pair(m.batch_stats[pre + 'bn2'], 'bf16', {q: v[1] for q, v in r.items()}, '%s %sbn2' % (name, pre))
            for i, f in enumerate(('mean', 'var')):                          # BN1: the stored channels' statistics
                check_stats(m.batch_stats[pre + 'bn1'][i], TR.stats(xin.double())[i], TR.stats(xin)[i], '%s %sbn1 %s' % (name, pre, f))
            cin += G
        xin = nchw(buf, cin)
        if s != len(net['blocks']) - 1:
            r = hop_refs(lambda mode: TR.transition(xin.to(mode.dtype), P, 'trans%d' % (s + 1), mode, TR.Tape(0.9)))
            check(nchw(tb['blocks'][s + 1], cin // 2), 'bf16', r['f64'], r['f32'], r['bf16'], '%s trans%d' % (name, s + 1))
    pad = (1, 1) if name == 'lpd' else 0

    def tail(mode):
        tape = TR.Tape(0.9)
        out = TR.head(TR.bn_relu(xin.to(mode.dtype), P, 'final.bn', mode, tape), P, mode, pad, tape)
        return out if name == 'lpd' else out.permute(0, 2, 3, 1)
    r = hop_refs(tail)
    check(got.cpu(), 'bf16', r['f64'], r['f32'], r['bf16'], '%s final BN and head' % name)


# ---- recalibrate_bn ------------------------------------------------------------------------------------------------------------------
def test_recalibrate_one_batch_makes_inference_the_training_forward(cuda):
    fwd, net, head, size, P, x, refs = train_case('micro')
    m, xd = build('micro', 'f32', cuda)
    static = {k: v.clone() for k, v in m.params.items() if 'running' not in k}
    train = m.logits(xd, training=True).clone()
    m.load_params(P)
    assert m.recalibrate_bn([xd]) == 1
    ev = m.logits(xd).clone()
    torch.cuda.synchronize()
    ref = {}
    for k in ('f64', 'f32'):
        Q, _ = TR.recalibrate(TR.ocr_forward, net, P, [x], R.Mode(k))
        ref[k] = R.ocr_forward(net, Q, x, R.Mode(k))[:, 0]
    check(ev.cpu(), 'f32', ref['f64'], ref['f32'], None, 'inference after recalibrate_bn([x])')
    check(ev.cpu(), 'f32', refs['f64'][0][:, 0], refs['f32'][0][:, 0], None, 'the same against the training forward')
    print('inference after recalibrate vs the device training logits: %.3e' % R.rel_err(ev.cpu(), train.cpu()))
    for k, v in static.items():
        assert torch.equal(bits(m.params[k]), bits(v)), k
    with pytest.raises(ValueError):
        m.recalibrate_bn([])


def test_recalibrate_three_batches_is_their_mean(cuda):
    fwd, net, head, size, P, x, refs = train_case('micro')
    m, xd = build('micro', 'f32', cuda)
    g = torch.Generator().manual_seed(31)
    batches = [x] + [(x + 0.2 * torch.rand(x.shape, generator=g)).clamp(0, 1).contiguous() for _ in range(2)]
    kept = []
    # the batch statistics of each batch alone (train mode reads no running statistic)
    for b in batches:
        m.forward(b.to(cuda), training=True)
        kept.append({k: (a.clone(), v.clone()) for k, (a, v) in m.batch_stats.items()})
    m.load_params(P)
    assert m.recalibrate_bn(b.to(cuda) for b in batches) == 3                  # any iterable
    torch.cuda.synchronize()
    Q64, _ = TR.recalibrate(TR.ocr_forward, net, P, batches, R.Mode('f64'))
    Q32, _ = TR.recalibrate(TR.ocr_forward, net, P, batches, R.Mode('f32'))
    worst = 0.0
    for bn, _ in m.bn_names():
        for i, f in enumerate(('running_mean', 'running_var')):
            k = '%s.%s' % (bn, f)
            check_stats(m.params[k], Q64[k], Q32[k], 'recalibrate %s' % k)
            own = sum(s[bn][i].double().cpu() for s in kept) / 3.0
            worst = max(worst, R.rel_err(m.params[k].cpu(), own))
    print('recalibrate: largest distance from the mean of the device\'s own three batch statistics %.3e' % worst)
    assert worst <= FLOOR


# ---- unchanged paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_inference_is_untouched_by_training_elsewhere(cuda, dtype):
    fwd, net, head, size, P, x, refs = train_case('micro')
    a, xd = build('micro', dtype, cuda)
    b, _ = build('micro', dtype, cuda)
    first = output(a, a(xd))
    b.forward(xd, training=True)
    second = output(a, a(xd))
    torch.cuda.synchronize()
    assert torch.equal(bits(first), bits(second))
    assert a.launches == 1 + sum(a.block_config) + len(a.block_config) - 1 + 3 == 13
    assert not a._folds_stale and b._folds_stale
