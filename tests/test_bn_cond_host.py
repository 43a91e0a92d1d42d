"""tests/bn_cond_ref.py checked on the CPU: the float64 restatement against torch, the generator's classes against their names, and
the invstd bar of tests/test_gpu_bn_cond.py against the weakness it is there to catch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cond_ref as B

KINDS = ['f32', 'bf16x3', 'bf16']


def _ncls(kind):
    return len(B.class_table(kind))


@pytest.mark.parametrize('kind', KINDS)
def test_every_class_lands_in_every_octet_position(kind):
    n = _ncls(kind)
    seen = {(B.class_of_channel(c, n), c % 8) for c in range(8 * n)}
    assert len(seen) == 8 * n
    # 264 channels (the GPU test's two channel groups): every class is there, the ragged second group starts a fresh octet
    assert {B.class_of_channel(c, n) for c in range(264)} == set(range(n))


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('kind', KINDS)
def test_restatement_equals_torch_autograd(kind, with_res):
    """stats64 / forward64 / backward64 / running64 against torch.nn.functional.batch_norm(training=True) + leaky_relu and its
    autograd in float64, on every class: z, the running statistics, dy, dgamma, dbeta."""
    npix, C = 257, 2 * _ncls(kind)
    y, names, _ = B.channels(npix, C, kind, seed=11)
    rng = np.random.default_rng(12)
    gamma = rng.uniform(0.5, 1.5, C)
    beta = rng.choice([-1.0, 1.0], C) * rng.uniform(0.05, 0.3, C)
    dz = rng.standard_normal((npix, C))
    res = rng.standard_normal((npix, C)) if with_res else None
    m, v = B.stats64(y)
    ist = B.invstd64(v)
    z = B.forward64(y, m, ist, gamma, beta, res)
    dy, dg, db = B.backward64(dz, y, m, ist, gamma, beta)
    rm, rv = B.running64(m, v, np.zeros(C), np.ones(C))

    yt = torch.from_numpy(y).double().requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    trm, trv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    zt = F.leaky_relu(F.batch_norm(yt, trm, trv, gt, bt, training=True, momentum=1.0 - B.MOMENTUM, eps=B.EPS), B.SLOPE)
    if with_res:
        zt = zt + torch.from_numpy(res)
    zt.backward(torch.from_numpy(dz))
    # (a constant channel: torch's mean of n equal values need not be the value itself, so its variance is ~1e-28 where
    #  stats64 gives exactly 0 -- far below eps either way; everything is compared per channel, relative to the channel's scale)
    def close(a, b, what, tol=1e-9):
        a, b = np.asarray(a), np.asarray(b)
        scale = np.abs(b).reshape(-1, C).max(axis=0) + 1e-300
        err = (np.abs(a - b).reshape(-1, C) / scale).max(axis=0)
        assert (err <= tol).all(), (what, [(names[c], float(err[c])) for c in np.nonzero(err > tol)[0]])
    close(z, zt.detach().numpy(), 'z')
    close(dy, yt.grad.numpy(), 'dy')
    close(dg, gt.grad.numpy(), 'dgamma', 1e-9 * npix)
    close(db, bt.grad.numpy(), 'dbeta', 1e-9 * npix)
    np.testing.assert_allclose(rm, trm.numpy(), rtol=1e-12, atol=1e-300)
    # torch's running_var takes the UNBIASED variance, Gluon's the biased one
    np.testing.assert_allclose(rv, 0.9 + (trv.numpy() - 0.9) * (npix - 1) / npix, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize('npix', [4096, 40000])
@pytest.mark.parametrize('kind', KINDS)
def test_classes_realise_what_they_name(kind, npix):
    """After the storage type's rounding: rho within a factor 2 of the name, `const` has variance exactly 0 and its value as the mean,
    the bf16 rho channels keep at least 3 distinct values, the adversaries' pixel 0 is 0 and the spike is not at pixel 0."""
    C = 3 * _ncls(kind)
    y, names, rho = B.channels(npix, C, kind, seed=5)
    assert np.array_equal(y, B.store(y, kind))                           # the array holds what the tensor will hold
    m, v = B.stats64(y)
    assert set(names) == {n for n, _ in B.class_table(kind)}
    for c, name in enumerate(names):
        nom = B.nominal_rho(name, kind)
        if nom is not None:
            assert nom / 2 <= rho[c] <= nom * 2, (name, rho[c])
        if name == 'const':
            assert v[c] == 0.0 and m[c] == y[0, c] and np.isinf(rho[c]) and y[0, c] != 0
        if name == 'zero':
            assert not y[:, c].any() and rho[c] == 0.0
        if name == 'spike':
            assert y[0, c] == 0 and np.count_nonzero(y[:, c]) == 1 and abs(y[:, c].max() - 1e4) <= 1e4 / 256
        if name.startswith('bf_rho'):
            assert len(np.unique(y[:, c])) >= 3
        if name in ('two-valued', 'bf_two'):
            assert len(np.unique(y[:, c])) == 2 and rho[c] > 1e4
        if name in ('pivot-adversary', 'bf_pivot'):
            assert y[0, c] == 0.0 and abs(m[c]) > 99 and min(npix, 1e4) / 4 <= rho[c] <= npix
    assert len({float(y[0, c]) for c in range(C) if names[c] == 'const'}) >= 3


@pytest.mark.parametrize('npix', [4096, 40000])
def test_the_invstd_bar_discriminates(npix):
    """The bar |invstd * sqrt(var64 + eps) - 1| <= 1e-3 must separate the kernels from the weakness: with plain fp32 sums over runs of
    8 terms (the shortest run the reduction's partition gives a lane) the emulation misses it by at least 10x on rho1e8+- and on
    the constants 65.3 and 19.99, while the same sums taken around pixel 0 stay inside it by orders of magnitude.

    For bf16 INPUTS the plain sums are exact or nearly so (squares of 8-bit significands need 16 bits, the runs are short): the bf16
    cases of tests/test_gpu_bn_cond.py therefore pin the bar on the paths that take plain sums (the convolution epilogue, the stem)
    and do NOT discriminate between a pivoted and a plain sum.  The last lines show that."""
    only = ['rho1e8+', 'rho1e8-', 'const']
    y, names, _ = B.channels(npix, 16 * len(only), 'f32', seed=3, only=only)
    _, v64 = B.stats64(y)
    _, vn = B.naive_one_pass_f32(y, 8)
    _, vp = B.naive_one_pass_f32(y, 8, pivot=y[0])
    en, ep = B.invstd_err(B.invstd64(vn), v64), B.invstd_err(B.invstd64(vp), v64)
    print('pivot  invstd error on every channel: <= %.2e' % ep.max())
    # The error of ONE rho1e8 channel is the mean of npix signed roundings: its size falls as 1 / sqrt(npix) and a single channel can
    # land near zero by chance (1 in 7 below 1e-2 at 40000 pixels).  A class is judged as the GPU tests judge it, by the maximum
    # over its channels -- and, so that one unlucky channel cannot carry the claim, by the median over 16 channels as well.
    for cls in ('rho1e8+', 'rho1e8-'):
        e = en[[c for c, n in enumerate(names) if n == cls]]
        print('naive  %-8s invstd error: median %.2e  max %.2e' % (cls, np.median(e), e.max()))
        assert len(e) == 16 and e.max() >= 10 * B.INVSTD_BAR and np.median(e) >= 10 * B.INVSTD_BAR, (cls, e)
    for k in (65.3, 19.99):                                              # (deterministic: every channel of a constant is the same)
        e = en[[c for c, n in enumerate(names) if n == 'const' and y[0, c] == np.float32(k)]]
        print('naive  const %-6s invstd error: %.2e' % (k, e.min()))
        assert len(e) and e.min() >= 10 * B.INVSTD_BAR, (k, e)
    assert (ep <= 1e-2 * B.INVSTD_BAR).all(), float(ep.max())
    yb, nb, _ = B.channels(npix, 16, 'bf16', seed=3)
    _, vb64 = B.stats64(yb)
    eb = B.invstd_err(B.invstd64(B.naive_one_pass_f32(yb, 8)[1]), vb64)
    print('bf16 inputs, naive: <= %.2e' % eb.max())
    assert (eb <= B.INVSTD_BAR).all()
