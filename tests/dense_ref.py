"""Torch-CPU restatement of the DenseNet bodies (yolo_amd/dense.py states the network; gluoncv's builder is not available and is
restated from recall there) and a numpy restatement of OCR.predict's reading rule (OCR/OCR.py:180-201).  Written from the
definition, sharing no code with the package.

Three arithmetic modes:
  'f64'   everything in float64
  'f32'   everything in float32
  'bf16'  bf16-EMULATED: weights and every convolution input rounded to bf16, sums in float32, appended / stored features rounded to
          bf16.  BatchNorm is folded in float32 (scale = gamma / sqrt(var + eps), bias = beta - mean * scale) in every mode but f64.
kernel_points=True moves the roundings to where the kernels round (include/yolo_amd.h): the stem convolves the unrounded image
with unrounded weights and rounds its output only; a transition pools first, rounds, then convolves.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
BN_FIELDS = ('gamma', 'beta', 'running_mean', 'running_var')


def rbf(t):
    return t.to(torch.bfloat16).to(t.dtype)


class Mode(object):
    def __init__(self, name, kernel_points=False):
        assert name in ('f64', 'f32', 'bf16')
        self.name, self.kernel_points = name, kernel_points
        self.dtype = torch.float64 if name == 'f64' else torch.float32
        self.emu = name == 'bf16'

    def r(self, t):
        return rbf(t) if self.emu else t

    def p(self, P, name):
        v = P[name]
        v = torch.from_numpy(np.asarray(v)) if not isinstance(v, torch.Tensor) else v
        return v.detach().cpu().to(self.dtype)


def fold(P, name, mode):
    g, b, m, v = (mode.p(P, '%s.%s' % (name, f)) for f in BN_FIELDS)
    s = g / torch.sqrt(v + EPS)
    return s, b - m * s


def affine_relu(x, s, t):
    return torch.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1))


def bn_act(x, P, name, mode):
    """ReLU(BatchNorm(x)), inference mode."""
    s, t = fold(P, name, mode)
    return affine_relu(x, s, t)


def stem(x, P, mode):
    w = mode.p(P, 'stem.weight')
    if mode.emu and not mode.kernel_points:
        x, w = rbf(x), rbf(w)
    y = bn_act(F.conv2d(x, w, stride=2, padding=3), P, 'stem', mode)
    return mode.r(F.max_pool2d(y, 3, 2, 1))


def dense_layer(x, P, pre, mode):
    """x (N, Cin, H, W) -> (N, Cin + G, H, W): identity first, the new channels raw."""
    a = mode.r(bn_act(x, P, pre + 'bn1', mode))
    m = F.conv2d(a, mode.r(mode.p(P, pre + 'conv1.weight')))
    b = mode.r(bn_act(m, P, pre + 'bn2', mode))
    y = F.conv2d(b, mode.r(mode.p(P, pre + 'conv2.weight')), padding=1)       # zero padding of b
    return torch.cat([x, mode.r(y)], 1)


def transition(x, P, name, mode):
    w = mode.r(mode.p(P, name + '.conv.weight'))
    a = bn_act(x, P, name + '.bn', mode)
    if mode.kernel_points:
        return mode.r(F.conv2d(mode.r(F.avg_pool2d(a, 2, 2)), w))
    return mode.r(F.avg_pool2d(F.conv2d(mode.r(a), w), 2, 2))


def bn_relu(x, P, name, mode):
    return mode.r(bn_act(x, P, name, mode))


def body(net, P, x, mode, taps=None):
    """net: dict(F0, G, blocks, bn_size).  Returns the map after the final BN + ReLU; taps (a list) receives every block's output."""
    x = torch.as_tensor(x).detach().cpu().to(mode.dtype)
    f = stem(x, P, mode)
    for s, n in enumerate(net['blocks']):
        for k in range(n):
            f = dense_layer(f, P, 'stage%d.layer%d.' % (s + 1, k), mode)
        if taps is not None:
            taps.append(f)
        if s != len(net['blocks']) - 1:
            f = transition(f, P, 'trans%d' % (s + 1), mode)
    return bn_relu(f, P, 'final.bn', mode)


def head_hidden(f, P, mode, padding):
    """The head up to the input of its last convolution: Conv + bias, BN, ReLU."""
    h = F.conv2d(f, mode.r(mode.p(P, 'head.conv1.weight')), mode.p(P, 'head.conv1.bias'), padding=padding)
    return mode.r(bn_act(h, P, 'head.bn', mode))


def head(f, P, mode, padding):
    h = head_hidden(f, P, mode, padding)
    return F.conv2d(h, mode.r(mode.p(P, 'head.conv2.weight')), mode.p(P, 'head.conv2.bias'))


def ocr_forward(net, P, x, mode):
    """(B, 1, W', 1 + classes): the NHWC logits OCRDenseNet.hybrid_forward slices into score_x and class_x."""
    return head(body(net, P, x, mode), P, mode, 0).permute(0, 2, 3, 1).contiguous()


def lpd_forward(net, P, x, mode):
    """(B, 7 + classes, h, w)."""
    return head(body(net, P, x, mode), P, mode, (1, 1))


def random_params(shapes, seed, head_gain=1.0):
    """Xavier-uniform weights and NON-TRIVIAL BatchNorm: gamma around 1, beta / mean / var such that the folded biases are clearly
    non-zero and often positive (otherwise the rule 'the 3x3 pads the activated map' is invisible)."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for name, shp in shapes.items():
        if name.endswith('.weight'):
            fan = (shp[0] + shp[1]) * shp[2] * shp[3] / 2.0
            P[name] = (torch.rand(shp, generator=g) * 2 - 1) * (3.0 / fan) ** 0.5
            if name == 'head.conv2.weight':
                P[name] = P[name] * head_gain
        elif name.endswith('.gamma'):
            P[name] = 0.8 + 0.4 * torch.rand(shp, generator=g)
        elif name.endswith('.beta'):
            P[name] = -0.2 + 0.7 * torch.rand(shp, generator=g)
        elif name.endswith('.running_mean'):
            P[name] = 0.3 * torch.randn(shp, generator=g)
        elif name.endswith('.running_var'):
            P[name] = 0.5 + torch.rand(shp, generator=g)
        else:                                   # conv bias
            P[name] = 0.2 * torch.randn(shp, generator=g)
    return P


def craft_reading(net, P, x, level, seed, classes, ridge=2.0):
    """Chooses the LAST head convolution of an OCR net on the CPU so that the float32 reference reads a definite text off x.
    A net that is random to its last layer tells its score columns apart by a few times the bf16 error (its outputs are dominated
    by constants), so nothing could be said about its reading on bf16; a trained net's last layer looks at what separates its
    columns.  The hidden columns h (512 values each) of the float64 reference differ from their mean along a few directions only
    (singular values 10, 9, 2.2, then < 0.6 on the full net), while the bf16 error is spread over all 512.  So head.conv2 is the
    RIDGE fit W = T' H (H'H + ridge I)^-1 of targets T to the centred columns H, which keeps to the strong directions: level
    (B, W') in 0..3 is the grey level of the input band over each column; the score target is 0.405 (the logit of 0.6) plus
    -2, -0.9, 0.9, 2 by level, the class targets are 3 at one seeded class per level and within +-0.5 elsewhere.  The fit is
    loose (that is the price of the ridge); the margins are whatever the float32 reference then has, and the tests measure them.
    Everything before that layer stays random.  P is changed in place."""
    g = torch.Generator().manual_seed(seed)
    mode = Mode('f64')
    h = head_hidden(body(net, P, x, mode), P, mode, 0)                 # (B, 512, 1, W')
    B, K, _, Wc = h.shape
    H = h.permute(0, 3, 1, 2).reshape(B * Wc, K)
    mean = H.mean(0, keepdim=True)
    Hc = H - mean
    lv = torch.as_tensor(level)[:, :Wc].reshape(-1)
    T = torch.rand((B * Wc, 1 + classes), generator=g, dtype=torch.float64) - 0.5
    T[:, 0] = torch.tensor([-2.0, -0.9, 0.9, 2.0], dtype=torch.float64)[lv]
    cls = torch.randint(0, classes, (4,), generator=g)
    T[torch.arange(B * Wc), 1 + cls[lv]] = 3.0
    Tm = T.mean(0)
    W = torch.linalg.solve(Hc.t() @ Hc + ridge * torch.eye(K, dtype=torch.float64), Hc.t() @ (T - Tm)).t()
    b = Tm.clone()
    b[0] += 0.405
    P['head.conv2.weight'] = W.reshape(1 + classes, K, 1, 1).float().contiguous()
    P['head.conv2.bias'] = (b - W @ mean[0]).float().contiguous()
    return P


def rel_err(a, b):
    """e(a, b) = max|a - b| / max|b|."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


# ---- OCR.predict's reading rule -----------------------------------------------------------------------------------------------
def read_columns(logits, thr):
    """logits (W', 1 + ncls) -> (score (W') float64, codes (W') int: the class at a peak, -1 elsewhere)."""
    logits = np.asarray(logits, dtype=np.float64)
    score = 1.0 / (1.0 + np.exp(-logits[:, 0]))
    e = np.exp(logits[:, 1:] - logits[:, 1:].max(axis=-1, keepdims=True))
    soft = e / e.sum(axis=-1, keepdims=True)
    s2 = np.concatenate(([0], score, [0]))
    codes = np.full(len(score), -1, dtype=np.int64)
    for i in range(len(score)):
        if s2[i + 1] > thr and s2[i + 1] > s2[i + 2] and s2[i + 1] > s2[i]:
            codes[i] = int(np.argmax(logits[i, 1:]))     # (the softmax is monotone: its argmax is the logits')
            assert soft[i, codes[i]] == soft[i].max()
    return score, codes


def text_of(codes, names):
    return ''.join(names[c] for c in codes if c >= 0)


def column_margins(logits, thr):
    """Per column, the smallest distance IN LOGITS that could change the reading: score logit to the threshold's logit, to both
    neighbours' score logits (the sigmoid is monotone), and the gap between the two largest class logits."""
    logits = np.asarray(logits, dtype=np.float64)
    z = logits[:, 0]
    zt = np.log(thr / (1.0 - thr))
    big = 1e30
    left = np.concatenate(([big], np.abs(z[1:] - z[:-1])))
    right = np.concatenate((np.abs(z[:-1] - z[1:]), [big]))
    cls = np.sort(logits[:, 1:], axis=-1)
    return np.minimum(np.minimum(np.abs(z - zt), np.minimum(left, right)), cls[:, -1] - cls[:, -2])
