"""CPU checks of the train-mode DenseNet forward: the restatement (tests/dense_train_ref.py) against an independent composition of
torch.nn modules in .train(), recalibrate as the mean of the batches' statistics, and the C ABI entries of csrc/dense_train.hip
(declared, bound, built, bad arguments refused without a GPU)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import dense_ref as R
import dense_train_ref as TR
from yolo_amd import dense as D
from yolo_amd import lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = {'yolo_dense_stats_workspace_bytes': 1, 'yolo_dense_bn_batch_fold': 4, 'yolo_dense_bottleneck_stats': 16,
         'yolo_dense_channel_stats': 13, 'yolo_dense_stem_stats': 11}
NET = dict(F0=16, G=8, blocks=[2, 2], bn_size=4)
HEAD = ('ocr', 3, 5)
SIZE = (26, 70)            # maps 7 x 18 and 3 x 9: the head's kernel is 3 rows high


def params(seed):
    return R.random_params(D.dense_param_shapes(NET['F0'], NET['G'], NET['blocks'], NET['bn_size'], HEAD), seed)


def images(seed, n=3):
    return torch.rand((n, 3) + SIZE, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- the restatement against torch.nn ----------------------------------------------------------------------------------------------
class _Layer(nn.Module):
    def __init__(self, cin, cm, g):
        super().__init__()
        self.bn1, self.conv1 = nn.BatchNorm2d(cin, momentum=0.1), nn.Conv2d(cin, cm, 1, bias=False)
        self.bn2, self.conv2 = nn.BatchNorm2d(cm, momentum=0.1), nn.Conv2d(cm, g, 3, padding=1, bias=False)

    def forward(self, x):
        return torch.cat([x, self.conv2(torch.relu(self.bn2(self.conv1(torch.relu(self.bn1(x))))))], 1)


def _modules(P):
    """{parameter prefix: module} and the forward function of the two-block OCR-shaped net; torch's momentum 0.1 is Gluon's 0.9."""
    F0, G, Cm = NET['F0'], NET['G'], NET['bn_size'] * NET['G']
    M = {'stem': (nn.Conv2d(3, F0, 7, 2, 3, bias=False), nn.BatchNorm2d(F0, momentum=0.1))}
    chans = D.block_channels(F0, G, NET['blocks'])
    for s, n in enumerate(NET['blocks']):
        for k in range(n):
            M['stage%d.layer%d' % (s + 1, k)] = _Layer(chans[s][0] + k * G, Cm, G)
    c1 = chans[0][1]
    M['trans1'] = (nn.BatchNorm2d(c1, momentum=0.1), nn.Conv2d(c1, c1 // 2, 1, bias=False))
    cf = chans[1][1]
    M['final'] = nn.BatchNorm2d(cf, momentum=0.1)
    M['head'] = (nn.Conv2d(cf, D.HEAD_WIDTH, (HEAD[1], 1)), nn.BatchNorm2d(D.HEAD_WIDTH, momentum=0.1), nn.Conv2d(D.HEAD_WIDTH, HEAD[2] + 1, 1))

    def load_bn(bn, name):
        bn.weight.data, bn.bias.data = P[name + '.gamma'].double(), P[name + '.beta'].double()
        bn.running_mean.data, bn.running_var.data = P[name + '.running_mean'].double(), P[name + '.running_var'].double()

    bns = {}
    M['stem'][0].weight.data = P['stem.weight'].double()
    bns['stem'] = M['stem'][1]
    for s, n in enumerate(NET['blocks']):
        for k in range(n):
            pre, m = 'stage%d.layer%d.' % (s + 1, k), M['stage%d.layer%d' % (s + 1, k)]
            m.conv1.weight.data, m.conv2.weight.data = P[pre + 'conv1.weight'].double(), P[pre + 'conv2.weight'].double()
            bns[pre + 'bn1'], bns[pre + 'bn2'] = m.bn1, m.bn2
    M['trans1'][1].weight.data = P['trans1.conv.weight'].double()
    bns['trans1.bn'], bns['final.bn'], bns['head.bn'] = M['trans1'][0], M['final'], M['head'][1]
    M['head'][0].weight.data, M['head'][0].bias.data = P['head.conv1.weight'].double(), P['head.conv1.bias'].double()
    M['head'][2].weight.data, M['head'][2].bias.data = P['head.conv2.weight'].double(), P['head.conv2.bias'].double()
    for name, bn in bns.items():
        bn.double()
        load_bn(bn, name)
        bn.train()

    def forward(x):
        f = nn.functional.max_pool2d(torch.relu(M['stem'][1](M['stem'][0](x))), 3, 2, 1)
        for s, n in enumerate(NET['blocks']):
            for k in range(n):
                f = M['stage%d.layer%d' % (s + 1, k)](f)
            if s == 0:
                f = nn.functional.avg_pool2d(M['trans1'][1](torch.relu(M['trans1'][0](f))), 2, 2)
        f = torch.relu(M['final'](f))
        return M['head'][2](torch.relu(M['head'][1](M['head'][0](f)))).permute(0, 2, 3, 1)
    return bns, forward


def test_restatement_equals_torch_modules_in_train_mode():
    P, x = params(3), images(4)
    bns, forward = _modules(P)
    with torch.no_grad():
        want = forward(x)
    got, tape = TR.ocr_forward(NET, P, x, R.Mode('f64'), momentum=0.9)
    assert tuple(got.shape) == tuple(want.shape) == (3, 1, 9, 6)
    assert R.rel_err(got, want) < 1e-10
    assert sorted(tape.stats) == sorted(bns) == sorted(n for n, _ in _bn_names())
    # an eval-mode answer is visibly different: the running statistics of random_params are not the batch's
    assert R.rel_err(R.ocr_forward(NET, P, x, R.Mode('f64')), want) > 1e-2
    for name, bn in bns.items():
        c = bn.num_features
        assert tuple(tape.stats[name][0].shape) == (c,)
        assert R.rel_err(tape.running[name + '.running_mean'], bn.running_mean) < 1e-10
        # torch keeps the UNBIASED variance in running_var, Gluon (and this library) the biased one: unbiased = biased * n / (n - 1),
        # n = the BatchNorm's population N * H * W, read off the update itself
        rv0 = P[name + '.running_var'].double()
        unbiased = (bn.running_var - 0.9 * rv0) / 0.1
        biased = tape.stats[name][1]
        n = float((unbiased / biased).mean())
        n = round(n / (n - 1.0)) if abs(n - 1.0) > 1e-12 else 0          # n / (n - 1) -> n
        assert n > 1 and n % 3 == 0                                       # a multiple of the batch size
        assert R.rel_err(tape.running[name + '.running_var'], 0.9 * rv0 + 0.1 * unbiased * (n - 1.0) / n) < 1e-9


def _bn_names():
    shapes = D.dense_param_shapes(NET['F0'], NET['G'], NET['blocks'], NET['bn_size'], HEAD)
    return [(k[:-len('.gamma')], v[0]) for k, v in shapes.items() if k.endswith('.gamma')]


def test_recalibrate_is_the_mean_of_the_batches_statistics():
    P = params(5)
    batches = [images(10 + k, 2) for k in range(3)]
    mode = R.Mode('f64')
    Q, tapes = TR.recalibrate(TR.ocr_forward, NET, P, batches, mode)
    assert len(tapes) == 3
    # the batch statistics of batch k depend only on the weights, gamma and beta (train mode reads no running statistic)
    alone = [TR.ocr_forward(NET, P, x, mode)[1] for x in batches]
    for name, _ in _bn_names():
        for i, f in enumerate(('running_mean', 'running_var')):
            mean3 = sum(t.stats[name][i] for t in alone) / 3.0
            assert R.rel_err(Q['%s.%s' % (name, f)], mean3) < 1e-12, name
    for k in P:
        if 'running' not in k:
            assert Q[k] is P[k]
    with pytest.raises(ValueError):
        TR.recalibrate(TR.ocr_forward, NET, P, [], mode)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_train_entries_declared_bound_and_built(lib):
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == lib.yolo_version()
    for name, nargs in NAMES.items():
        assert name in L.SIGNATURES and hasattr(lib, name)
        proto = re.search(r'^(?:int|long long) %s\(([^)]*)\)' % name, h, re.M | re.S).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs, name
    assert 'typedef struct yolo_bn_batch_fold' in h
    assert [f for f, _ in L.BnBatchFold._fields_] == ['gamma', 'beta', 'running_mean', 'running_var', 'scale', 'bias', 'C', 'eps', 'momentum']
    assert C.sizeof(L.BnBatchFold) == 6 * 8 + 4 + 4 + 4 + 4              # six pointers, an int, two floats, padding to 8
    rows = int(re.search(r'#define YOLO_DENSE_STATS_ROWS (\d+)', h).group(1))
    assert lib.yolo_dense_stats_workspace_bytes(48) == rows * 2 * 48 * 8
    assert lib.yolo_dense_stats_workspace_bytes(0) == L.EINVAL and lib.yolo_dense_stats_workspace_bytes(-4) == L.EINVAL


def _fold(**kw):
    p = 4096
    d = L.BnBatchFold()
    d.gamma, d.beta, d.running_mean, d.running_var, d.scale, d.bias, d.C, d.eps, d.momentum = p, p, p, p, p, p, 48, 1e-5, 0.9
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refusals(fn, ok, ptrs, sizes, nullable=()):
    for k in ptrs:
        if k not in nullable:
            a = list(ok); a[k] = None
            assert fn(*a) == L.EINVAL, (fn.__name__, k)
    for k in sizes:
        for v in (0, -3):
            a = list(ok); a[k] = v
            assert fn(*a) == L.EINVAL, (fn.__name__, k, v)


def test_train_entries_refuse_bad_arguments_without_a_gpu(lib):
    """Validation comes before any launch: none of these pointers is ever dereferenced, and no GPU is needed to be refused."""
    p = C.c_void_p(4096)
    f48, f32_ = _fold(), _fold(C=32)
    #      buf w1 s1 t1 mean var ws fold            N  H  W  Cs  Cin Cm  dtype  stream
    bott = [p, p, p, p, p,   p,  p, C.byref(f48),   2, 5, 7, 96, 44, 48, L.BF16, None]
    #      buf mean var ws fold          N  H  W  Cs  c0  n   dtype  stream
    chan = [p, p,   p,  p, C.byref(f48), 2, 5, 7, 96, 45, 12, L.F32, None]
    #      x  w  mean var ws fold           N  H   W   F0  stream
    stem = [p, p, p,   p,  p, C.byref(f32_), 2, 21, 37, 32, None]
    _refusals(lib.yolo_dense_bottleneck_stats, bott, (0, 1, 2, 3, 4, 5, 6), (8, 9, 10, 11, 12, 13))
    _refusals(lib.yolo_dense_channel_stats, chan, (0, 1, 2, 3), (5, 6, 7, 8, 10))
    _refusals(lib.yolo_dense_stem_stats, stem, (0, 1, 2, 3, 4), (6, 7, 8, 9))
    a = list(chan); a[9] = -1                                                   # c0 may be 0, not negative
    assert lib.yolo_dense_channel_stats(*a) == L.EINVAL
    for fn, ok, k in ((lib.yolo_dense_bottleneck_stats, bott, 14), (lib.yolo_dense_channel_stats, chan, 11)):
        a = list(ok); a[k] = 17                                                 # an unknown dtype
        assert fn(*a) == L.EINVAL
        for dt in (L.F16, L.BF16X3, L.F16X3):                                   # valid, not taken here
            a = list(ok); a[k] = dt
            assert fn(*a) == L.EUNSUPPORTED
    # a malformed fold, through every entry that takes one
    for bad in (dict(gamma=None), dict(beta=None), dict(scale=None), dict(bias=None), dict(C=0), dict(running_mean=None),
                dict(running_var=None), dict(eps=0.0), dict(momentum=-0.1), dict(momentum=1.5)):
        assert lib.yolo_dense_bn_batch_fold(p, p, C.byref(_fold(**bad)), None) == L.EINVAL, bad
        a = list(chan); a[4] = C.byref(_fold(**bad))
        assert lib.yolo_dense_channel_stats(*a) == L.EINVAL, bad
        a = list(bott); a[7] = C.byref(_fold(**bad))
        assert lib.yolo_dense_bottleneck_stats(*a) == L.EINVAL, bad
        a = list(stem); a[5] = C.byref(_fold(C=32, **bad) if 'C' not in bad else _fold(**bad))
        assert lib.yolo_dense_stem_stats(*a) == L.EINVAL, bad
    for k in (0, 1, 2):
        a = [p, p, C.byref(f48), None]; a[k] = None
        assert lib.yolo_dense_bn_batch_fold(*a) == L.EINVAL
    # the limits of yolo_dense_layer_fwd
    for k, v in ((13, 40), (13, 144), (12, 7), (11, 80), (12, 100)):            # Cm % 16, Cm <= 128, Cin >= 8, Cs % 32, Cin <= Cs
        a = list(bott); a[k] = v
        assert lib.yolo_dense_bottleneck_stats(*a) == L.EUNSUPPORTED, (k, v)
    a = list(bott); a[7] = C.byref(f32_)                                        # the fold is BN2: C == Cm
    assert lib.yolo_dense_bottleneck_stats(*a) == L.EUNSUPPORTED
    a = list(chan); a[9], a[10] = 90, 12                                        # c0 + n <= Cs
    assert lib.yolo_dense_channel_stats(*a) == L.EUNSUPPORTED
    for k, v in ((9, 12), (9, 72)):                                             # F0 % 8, F0 <= 64
        a = list(stem); a[k] = v
        assert lib.yolo_dense_stem_stats(*a) == L.EUNSUPPORTED
    a = list(stem); a[5] = C.byref(f48)                                         # the fold is the stem's BN: C == F0
    assert lib.yolo_dense_stem_stats(*a) == L.EUNSUPPORTED
    # buffers of 2^31 bytes
    a = list(bott); a[8], a[9], a[10], a[11] = 2 ** 8, 2 ** 8, 2 ** 8, 64       # 2^24 pixels x 64 channels x 2 bytes
    assert lib.yolo_dense_bottleneck_stats(*a) == L.EUNSUPPORTED
    a = list(chan); a[5], a[6], a[7], a[8] = 2 ** 8, 2 ** 8, 2 ** 7, 64         # 2^23 pixels x 64 channels x 4 bytes
    assert lib.yolo_dense_channel_stats(*a) == L.EUNSUPPORTED
    a = list(stem); a[6], a[7], a[8] = 2 ** 9, 2 ** 10, 2 ** 10 // 3 + 1        # N x 3 x H x W x 4 bytes
    assert lib.yolo_dense_stem_stats(*a) == L.EUNSUPPORTED


def test_no_trainer_is_offered_yet():
    import yolo_amd
    with pytest.raises(AttributeError):
        yolo_amd.OCRTrainer
    assert callable(D.DenseNet.recalibrate_bn) and callable(D.DenseNet.training_buffers)
    assert 'training' in D.OCRNet.logits.__code__.co_varnames and 'training' in D.DenseNet.forward.__code__.co_varnames
