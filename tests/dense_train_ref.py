"""Torch-CPU restatement of the DenseNet bodies' TRAIN-MODE forward: BatchNorm with the batch's statistics, the statistics kept per
BatchNorm, the running statistics updated as Gluon does (running = momentum * running + (1 - momentum) * batch, the BIASED variance).
Written from the definition, sharing no code with the package; the arithmetic modes are those of tests/dense_ref.py ('f64', 'f32',
'bf16' emulated, kernel_points=True: rounded where the kernels round).

Statistics are taken where the kernels take them:
  a block's channels   of the values AS STORED (rounded to the buffer's type), once, when the channel is written
  BN2 of a dense layer of the fp32 bottleneck m = W1 a, before any rounding
  the stem's BN        of the raw 7x7 convolution
  the head's BN        of the first convolution + bias as stored
A statistic is the mean and the biased variance over (N, H, W), in the mode's float type (two passes; the kernels add in double).
"""
import torch
import torch.nn.functional as F

import dense_ref as R

EPS = R.EPS


def stats(t):
    """(N, C, H, W) -> (mean (C), biased variance (C))."""
    m = t.mean(dim=(0, 2, 3))
    return m, ((t - m.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))


class Tape(object):
    """What a training forward leaves: stats {bn name: (mean, var)} and running {'<bn>.running_mean' / '_var': updated value}."""

    def __init__(self, momentum):
        self.momentum, self.stats, self.running = momentum, {}, {}

    def note(self, P, name, mode, m, v):
        self.stats[name] = (m, v)
        for f, b in (('running_mean', m), ('running_var', v)):
            self.running['%s.%s' % (name, f)] = self.momentum * mode.p(P, '%s.%s' % (name, f)) + (1.0 - self.momentum) * b

    def updated(self, P):
        """P with the running statistics replaced by the updated ones (in the mode's float type)."""
        Q = dict(P)
        Q.update(self.running)
        return Q


def fold_batch(P, name, mode, tape, m, v):
    tape.note(P, name, mode, m, v)
    s = mode.p(P, name + '.gamma') / torch.sqrt(v + EPS)
    return s, mode.p(P, name + '.beta') - m * s


def stem(x, P, mode, tape):
    w = mode.p(P, 'stem.weight')
    if mode.emu and not mode.kernel_points:
        x, w = R.rbf(x), R.rbf(w)
    raw = F.conv2d(x, w, stride=2, padding=3)
    s, t = fold_batch(P, 'stem', mode, tape, *stats(raw))
    return mode.r(F.max_pool2d(R.affine_relu(raw, s, t), 3, 2, 1))


def dense_layer(x, P, pre, mode, tape, xstats=None):
    """x (N, Cin, H, W) as stored -> ((N, Cin + G, H, W), (mean, var) of all Cin + G channels)."""
    m1, v1 = xstats if xstats is not None else stats(x)
    s1, t1 = fold_batch(P, pre + 'bn1', mode, tape, m1, v1)
    a = mode.r(R.affine_relu(x, s1, t1))
    m = F.conv2d(a, mode.r(mode.p(P, pre + 'conv1.weight')))
    s2, t2 = fold_batch(P, pre + 'bn2', mode, tape, *stats(m))
    b = mode.r(R.affine_relu(m, s2, t2))
    y = mode.r(F.conv2d(b, mode.r(mode.p(P, pre + 'conv2.weight')), padding=1))
    ym, yv = stats(y)
    return torch.cat([x, y], 1), (torch.cat([m1, ym]), torch.cat([v1, yv]))


def transition(x, P, name, mode, tape, xstats=None):
    s, t = fold_batch(P, name + '.bn', mode, tape, *(xstats if xstats is not None else stats(x)))
    w = mode.r(mode.p(P, name + '.conv.weight'))
    a = R.affine_relu(x, s, t)
    if mode.kernel_points:
        return mode.r(F.conv2d(mode.r(F.avg_pool2d(a, 2, 2)), w))
    return mode.r(F.avg_pool2d(F.conv2d(mode.r(a), w), 2, 2))


def bn_relu(x, P, name, mode, tape, xstats=None):
    s, t = fold_batch(P, name, mode, tape, *(xstats if xstats is not None else stats(x)))
    return mode.r(R.affine_relu(x, s, t))


def head_hidden(f, P, mode, padding, tape):
    """Conv + bias STORED, then the BatchNorm of its batch statistics as yolo_bn_train_fwd states it, ReLU."""
    h = mode.r(F.conv2d(f, mode.r(mode.p(P, 'head.conv1.weight')), mode.p(P, 'head.conv1.bias'), padding=padding))
    m, v = stats(h)
    tape.note(P, 'head.bn', mode, m, v)
    g, b = mode.p(P, 'head.bn.gamma'), mode.p(P, 'head.bn.beta')
    c = lambda u: u.view(1, -1, 1, 1)
    return mode.r(torch.relu(c(g) * (h - c(m)) * c(1.0 / torch.sqrt(v + EPS)) + c(b)))


def head(f, P, mode, padding, tape):
    return F.conv2d(head_hidden(f, P, mode, padding, tape), mode.r(mode.p(P, 'head.conv2.weight')), mode.p(P, 'head.conv2.bias'))


def body(net, P, x, mode, tape):
    x = torch.as_tensor(x).detach().cpu().to(mode.dtype)
    f = stem(x, P, mode, tape)
    st = None
    for s, n in enumerate(net['blocks']):
        for k in range(n):
            f, st = dense_layer(f, P, 'stage%d.layer%d.' % (s + 1, k), mode, tape, st)
        if s != len(net['blocks']) - 1:
            f, st = transition(f, P, 'trans%d' % (s + 1), mode, tape, st), None
    return bn_relu(f, P, 'final.bn', mode, tape, st)


def ocr_forward(net, P, x, mode, momentum=0.9):
    """-> ((B, 1, W', 1 + classes) logits, Tape)."""
    tape = Tape(momentum)
    return head(body(net, P, x, mode, tape), P, mode, 0, tape).permute(0, 2, 3, 1).contiguous(), tape


def lpd_forward(net, P, x, mode, momentum=0.9):
    tape = Tape(momentum)
    return head(body(net, P, x, mode, tape), P, mode, (1, 1), tape), tape


def recalibrate(forward, net, P, batches, mode):
    """The k-th batch at momentum 1 - 1 / k: the running statistics end as the plain average of the batches' statistics.
    -> (P with the new running statistics, [Tape per batch])."""
    tapes = []
    for k, x in enumerate(batches, 1):
        _, tape = forward(net, P, x, mode, 1.0 - 1.0 / k)
        P = tape.updated(P)
        tapes.append(tape)
    if not tapes:
        raise ValueError('no batch')
    return P, tapes
