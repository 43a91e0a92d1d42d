"""Reference and channel generators for train-mode BatchNorm on ill-conditioned channels (plain numpy / torch on the CPU).

Restatement.  Gluon BatchNorm in training mode + LeakyReLU (+ residual) and its backward, two-pass in float64 (SURVEY App. A.3;
include/yolo_amd.h yolo_bn_train_fwd / _bwd).  forward64 / backward64 TAKE the mean and invstd they are given, so a kernel is
checked one hop at a time: its statistics against stats64, everything behind them against the restatement fed the kernel's own
float32 statistics.

Generator.  channels(npix, C, kind, seed) -> an (npix, C) float32 array whose channels cycle through named classes.  The condition
of a channel for a one-pass variance is rho = mean^2 / var: fp32 sums of y and y^2 carry about rho * 2^-24 relative error into
the variance.  `kind` is how the values are stored: 'f32' as drawn, 'bf16x3' as hi + lo of two bf16 planes, 'bf16' as one bf16
value -- the array holds exactly what the device tensor will hold, and the realised rho of THAT is returned with it.

Emulator.  naive_one_pass_f32 restates the weakness the tests pin: sequential fp32 sums of y and y^2 over short runs, combined in
double, var = max(Q/n - d^2, 0)."""
from math import gcd

import numpy as np
import torch

EPS, MOMENTUM, SLOPE = 1e-5, 0.9, 0.1

# the classes in the order the channels cycle through them (the worst conditioned first: a narrow tensor holds a prefix);
# value = the rho the name stands for (None: no finite nominal value; the pivot adversaries' outlier at pixel 0 IS their variance:
# rho is about npix, and that is also what sums around pixel 0 see)
EXACT_CLASSES = [('rho1e8+', 1e8), ('rho1e8-', 1e8), ('const', None), ('pivot-adversary', None), ('rho1e6+', 1e6), ('rho1e6-', 1e6),
                 ('benign', 0.0625), ('spike', None), ('zero', None), ('two-valued', None), ('rho1e4+', 1e4), ('rho1e4-', 1e4)]
# one bf16 value per element: 100 +- 0.3 lands on the 0.5 grid of [64, 128) -- var 0.09 + 0.25 / 12, rho about 1e5
BF16_CLASSES = [('bf_rho+', 1e5), ('bf_rho-', 1e5), ('const', None), ('bf_pivot', None), ('bf_two', None), ('benign', 0.0625),
                ('spike', None), ('zero', None)]
EXACT_CONSTS = [65.3, 19.99, 37.3, -3.7, 1000.1, 0.1]
BF16_CONSTS = [65.5, 20.0, 37.25, -3.75, 1000.0, 0.1015625]          # eight significant bits each


def class_table(kind):
    return BF16_CLASSES if kind == 'bf16' else EXACT_CLASSES


def class_of_channel(c, ncls):
    """Channel c -> class index.  Octet o starts k further along the cycle than 8 channels would, k the smallest shift that makes
    the step per octet coprime with the number of classes: position e of the octets then meets every class within ncls octets,
    so every class lands in every octet position (and, from 8 * ncls channels on, in every 256-channel group)."""
    k = 0
    while gcd(8 + k, ncls) != 1:
        k += 1
    return (c + k * (c // 8)) % ncls


def store(v, kind):
    """float32 values as a tensor of `kind` holds them."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    if kind == 'bf16':
        t = t.bfloat16().float()
    elif kind == 'bf16x3':
        hi = t.bfloat16().float()
        t = hi + (t - hi).bfloat16().float()
    else:
        assert kind == 'f32', kind
    return t.numpy()


def _column(name, npix, rng, kind, nth_const):
    n = rng.standard_normal(npix)
    sign = -1.0 if name.endswith('-') else 1.0
    if name == 'benign':
        v = 0.5 + 2.0 * n
    elif name.startswith('rho1e4'):
        v = sign * 100.0 + n
    elif name.startswith('rho1e6'):
        v = sign * 100.0 + 0.1 * n
    elif name.startswith('rho1e8'):
        v = sign * 1000.0 + 0.1 * n
    elif name.startswith('bf_rho'):
        v = sign * 100.0 + 0.3 * n
    elif name == 'const':
        consts = BF16_CONSTS if kind == 'bf16' else EXACT_CONSTS
        v = np.full(npix, consts[nth_const % len(consts)])
    elif name == 'zero':
        v = np.zeros(npix)
    elif name == 'spike':
        v = np.zeros(npix)
        if npix > 1:
            v[1 + int(rng.integers(npix - 1))] = 1e4                 # never pixel 0
    elif name == 'two-valued':
        m = np.float32(100.0)
        v = np.where(rng.random(npix) < 0.5, m, np.nextafter(m, np.float32(np.inf))).astype(np.float64)
    elif name == 'bf_two':
        v = np.where(rng.random(npix) < 0.5, 100.0, 100.5)
    elif name == 'pivot-adversary':
        v = 1000.0 + 0.1 * n
        v[0] = 0.0
    elif name == 'bf_pivot':
        v = 100.0 + 0.3 * n
        v[0] = 0.0
    else:
        raise ValueError(name)
    return v


def rho_of(col):
    """mean^2 / var of one stored channel in float64: inf for a non-zero constant, 0 for the zero channel."""
    m, v = stats64(np.asarray(col, dtype=np.float64).reshape(-1, 1))
    m, v = float(m[0]), float(v[0])
    if v == 0.0:
        return np.inf if m != 0.0 else 0.0
    return m * m / v


def channels(npix, C, kind, seed, only=None):
    """-> (y, names, rho): y (npix, C) float32 holding exactly what a tensor of `kind` stores, the class name of every channel, the
    realised rho of every stored channel.  only: a list of class names to cycle through instead of the kind's whole table."""
    table = [n for n, _ in class_table(kind)]
    if only is not None:
        assert all(n in table for n in only)
        table = list(only)
    rng = np.random.default_rng(seed)
    y = np.empty((npix, C), dtype=np.float32)
    names, nconst = [], 0
    for c in range(C):
        name = table[class_of_channel(c, len(table))]
        y[:, c] = store(_column(name, npix, rng, kind, nconst), kind)
        nconst += name == 'const'
        names.append(name)
    return y, names, np.array([rho_of(y[:, c]) for c in range(C)])


def nominal_rho(name, kind):
    return dict(class_table(kind))[name]


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------
def stats64(y):
    """(npix, C) -> mean, biased variance in float64, two passes around pixel 0: the differences of float32 values are exact in
    float64, so a constant channel has variance exactly 0 and its own value as the mean."""
    y = np.asarray(y, dtype=np.float64)
    d = y - y[:1]
    dm = d.mean(axis=0)
    return y[0] + dm, ((d - dm) ** 2).mean(axis=0)


def invstd64(var, eps=EPS):
    return 1.0 / np.sqrt(np.asarray(var, dtype=np.float64) + eps)


def running64(mean, var, running_mean, running_var, momentum=MOMENTUM):
    """Gluon's update: r = momentum * r + (1 - momentum) * batch; running_var takes the BIASED variance."""
    return momentum * running_mean + (1.0 - momentum) * mean, momentum * running_var + (1.0 - momentum) * var


def preact64(y, mean, invstd, gamma, beta):
    f = lambda a: np.asarray(a, dtype=np.float64)
    xhat = (f(y) - f(mean)) * f(invstd)
    return xhat, f(gamma) * xhat + f(beta)


def forward64(y, mean, invstd, gamma, beta, res=None, slope=SLOPE):
    _, a = preact64(y, mean, invstd, gamma, beta)
    z = np.where(a > 0, a, a * slope)
    return z if res is None else z + np.asarray(res, dtype=np.float64)


def backward64(dz, y, mean, invstd, gamma, beta, slope=SLOPE):
    """-> dy, dgamma, dbeta.  The residual branch receives dz unchanged and is not part of this."""
    xhat, a = preact64(y, mean, invstd, gamma, beta)
    da = np.asarray(dz, dtype=np.float64) * np.where(a > 0, 1.0, slope)
    n = da.shape[0]
    dbeta, dgamma = da.sum(axis=0), (da * xhat).sum(axis=0)
    dy = np.asarray(gamma, dtype=np.float64) * np.asarray(invstd, dtype=np.float64) * (da - dbeta / n - xhat * dgamma / n)
    return dy, dgamma, dbeta


# ---- the weakness ---------------------------------------------------------------------------------------------------------------------
def naive_one_pass_f32(y, run, pivot=None):
    """One-pass statistics as a kernel takes them when nothing guards the sums: every lane adds `run` consecutive terms of y and of
    y^2 one after the other in float32, the lanes' sums are combined in double, var = max(Q/n - d^2, 0).  pivot (C,) float32: the
    sums are taken of (y - pivot) instead, the subtraction in float32, and the mean gets the pivot back in double.
    -> mean, var (float64)."""
    y = np.asarray(y, dtype=np.float32)
    n, C = y.shape
    if pivot is not None:
        y = (y - np.asarray(pivot, dtype=np.float32)[None, :]).astype(np.float32)
    lanes = -(-n // run)
    pad = np.zeros((lanes * run, C), dtype=np.float32)
    pad[:n] = y
    pad = pad.reshape(lanes, run, C)
    s = np.zeros((lanes, C), dtype=np.float32)
    q = np.zeros((lanes, C), dtype=np.float32)
    for j in range(run):
        v = pad[:, j]
        s = (s + v).astype(np.float32)
        q = (q + (v * v).astype(np.float32)).astype(np.float32)
    d = s.astype(np.float64).sum(axis=0) / n
    var = np.maximum(q.astype(np.float64).sum(axis=0) / n - d * d, 0.0)
    return d + (0.0 if pivot is None else np.asarray(pivot, dtype=np.float64)), var


# ---- the bars (training's BatchNorm) ---------------------------------------------------------------------------------------
def mean_bar(m64, v64):
    """One float32 ulp of a value rounded from double, plus float32 noise of terms of size sigma."""
    return 2.0 ** -23 * np.abs(m64) + 1e-6 * np.sqrt(v64)


def mean_err_ulps(mean, m64):
    """|mean - m64| in float32 ulps of m64 (for the printed tables; the zero channel counts in units of 2^-149)."""
    ulp = np.spacing(np.abs(np.asarray(m64, dtype=np.float64)).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(mean, dtype=np.float64) - m64) / ulp


def invstd_err(invstd, v64, eps=EPS):
    return np.abs(np.asarray(invstd, dtype=np.float64) * np.sqrt(v64 + eps) - 1.0)


INVSTD_BAR = 1e-3


def running_var_bar(v64, ref):
    return 1e-4 * v64 + 2.0 ** -23 * np.abs(ref)
