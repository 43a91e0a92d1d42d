"""GPU parity at the BASELINE.json configurations themselves (round-1 verdict: the Darknet-53 training step, the
608x608 forward and the batch-32 measured-tuning plan were benched but never compared with the oracle).

  configs[1]  D53 spec forward 416x416 bs 32, tune='measure' (bench.py's plan)      test_config1_bs32_measured_plan
  configs[2]  car/YOLO.py training step (car/YOLO.py:350-399), D53 spec 416x416       test_d53_train_step_*  (B=2 fp32 and
              bf16 against the oracle; bs 64 bf16 as a replicated-batch property)
  configs[4]  D53 spec forward 608x608 + decode + NMS (car/utils.py:68-95 at N=7581)  test_d53_608_forward

The one-hop tests re-derive EVERY gradient of the step from values the HIP path saved one layer away (oracle.train.
bn_act_backward / conv_backward): chaos cannot accumulate, so the bars are tight at the real layer shapes -- the
strip / row-group / per-tap weight gradients, the sub-pixel stride-2 data gradient and the channel-group BatchNorm
reductions all run at the shapes they were written for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graph as og, forward as of, train as ot, detect as od
from util import KERNEL_SETS, pin_kernels, assert_plan_held

pytestmark = pytest.mark.gpu

SIZE = (416, 416)


def _nchw(t, c=None):
    """NHWC device tensor (f32 / bf16) -> float32 NCHW CPU tensor (first c channels)."""
    t = t.float()
    if c is not None:
        t = t[..., :c]
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _kink_flips(dy, dy_ref, a_ref, tol, a_impl=None, frac=2e-5):
    """Elements where the implementation took the other LeakyReLU branch than the float64 reference: their dy is off by
    the kink's factor.  Legitimate only for elements whose BatchNorm output is within rounding of zero -- checked -- and
    only for a handful of them.

    a_impl: the BatchNorm output as the implementation's fp32 arithmetic evaluates it (bn_train.hip: xh = (y - mean) * invstd;
    a = gamma * xh + beta, no contraction) -- the branch decisions are then read off it directly.  Without it only the
    elements whose dy is off by more than `tol` are found: a flipped element with a smaller dz stayed in the reference's
    sums (round 4: one such element, 1.9 % of the largest dy, put dbeta of stages.2.res.7.c1 -- a sum that cancels to
    4e-5 out of 2e-2 of summands -- 0.7 % off its reference after a change of kernel variants moved the data by an ulp)."""
    err = (dy.double() - dy_ref).abs() / (dy_ref.abs().max() + 1e-30)
    bad = err > tol
    if a_impl is not None:
        flipped = (a_impl > 0) != (a_ref > 0)
        assert not bool((bad & ~flipped).any()), 'an element whose branch decision agrees with the reference is off'
        # (bf16: the elements of a channel that share ONE stored value of y flip together when that value's BatchNorm output is
        #  the one within rounding of zero -- 58 of 1.4 M seen.  So the flips are counted per distinct (channel, value of a): at
        #  most two values per channel -- the bf16 neighbours either side of the kink -- and the same global fraction as without
        #  a_impl; what makes a flip legitimate is the distance check below)
        bad = flipped
        if bool(bad.any()):
            idx = bad.nonzero()
            keys = {}
            for c_, v_ in zip(idx[:, 1].tolist(), a_impl[bad].tolist()):
                keys.setdefault(c_, set()).add(v_)
            assert max(len(v_) for v_ in keys.values()) <= 2, 'a channel flips at more than two stored values: %s' % {c_: len(v_) for c_, v_ in keys.items() if len(v_) > 2}
            assert sum(len(v_) for v_ in keys.values()) <= max(1.0, frac * bad.numel()), 'too many distinct flipped values: %d' % sum(len(v_) for v_ in keys.values())
    if bool(bad.any()):
        if a_impl is None:
            assert float(bad.double().mean()) <= frac, 'too many elements off: %d of %d' % (int(bad.sum()), bad.numel())
        far = float(a_ref[bad].abs().max()) > 2e-5 * float(a_ref.abs().max())
        if far:
            print('off elements (n, c, y, x) -> got / want:',
                  [(i, float(dy[tuple(i)]), float(dy_ref[tuple(i)])) for i in bad.nonzero()[:24].tolist()])
        assert not far, 'an element far from the kink is off'
    return bad


def _one_hop_check(tr, P, cap, params, tol, tol_w, rb, exact_kink=True):
    """Every forward value and every gradient of the step against its one-hop reference.  rb: the rounding the HIP path
    applies when it stores an activation (identity for fp32, bf16 round for bf16).  exact_kink: resolve LeakyReLU
    branch decisions at the kink element by element (fp32); in bf16 the stored rounding hides them below the bar."""
    grads = tr.grads()
    nflip = [0]
    consumers = {}
    for op in P.fwd:
        for k in ('x', 'res', 'up', 'route'):
            t = op.get(k)
            if t is not None:
                consumers.setdefault(id(t), []).append((k, op))
    worst = {}

    def note(kind, name, err, bar):
        if err > worst.get(kind, (0, ''))[0]:
            worst[kind] = (err, name)
        assert err < bar, '%s %s: relative error %.3g (bar %.1g)' % (kind, name, err, bar)

    def grad_ref(t):
        """Sum of the contributions of t's consumers, each from the consumer's own captured dy."""
        tot = None
        for k, op in consumers[id(t)]:
            if op['kind'] == 'conv_bn':
                c = op['c']
                if k == 'res':
                    g = _nchw(cap[c.name]['dz'])
                else:
                    w = params[c.name + '.weight'].detach().float().cpu()
                    if w.shape[1] != t.shape[3]:
                        continue                                            # (the image: channel-padded, no gradient wanted)
                    g = torch.nn.grad.conv2d_input((t.shape[0], t.shape[3], t.shape[1], t.shape[2]), rb(w),
                                                   _nchw(cap[c.name]['dy']), stride=c.stride, padding=c.k // 2)
            elif op['kind'] == 'out':
                c = op['c']
                w = params[c.name + '.weight'].detach().float().cpu()
                dyp = op['dyp'].float()[:, :c.cout].view(t.shape[0], t.shape[1], t.shape[2], c.cout)
                g = torch.nn.grad.conv2d_input((t.shape[0], t.shape[3], t.shape[1], t.shape[2]), rb(w), _nchw(dyp), stride=1, padding=0)
            else:
                dcat = _nchw(op['cat'].grad)
                cu = op['up'].shape[3]
                if k == 'up':
                    g = F.avg_pool2d(dcat[:, :cu], 2) * 4.0                 # backward of the nearest 2x up-sampling
                else:
                    g = dcat[:, cu:]
            tot = g if tot is None else tot + g
        return tot

    for op in P.fwd:
        if op['kind'] == 'conv_bn':
            c, xin, y, z = op['c'], op['x'], op['yraw'], op['z']
            w = params[c.name + '.weight'].detach().float().cpu()
            x = _nchw(xin.val, c.cin)
            yraw = _nchw(y.val)
            # forward, one hop: the raw convolution of the saved input, BN + LeakyReLU (+ residual) of the saved raw output
            note('conv fwd', c.name, _rel(yraw, rb(F.conv2d(x, rb(w), None, stride=c.stride, padding=c.k // 2))), tol)
            dz = _nchw(cap[c.name]['dz'])
            gam, bet = params[c.name + '.gamma'].cpu(), params[c.name + '.beta'].cpu()
            zref, dy_ref, dg_ref, db_ref, aref = ot.bn_act_backward(yraw, gam, bet, dz)
            if op['res'] is not None:
                zref = zref + _nchw(op['res'].val).double()
            note('bn fwd', c.name, _rel(_nchw(z.val), rb(zref.float())), tol)
            np.testing.assert_allclose(op['mean'].cpu().numpy(), yraw.double().mean(dim=(0, 2, 3)).numpy(), rtol=1e-4, atol=1e-5)
            # backward, one hop (for the branch decisions the implementation took at the kink of LeakyReLU)
            dy = _nchw(cap[c.name]['dy'])
            assert bool(torch.isfinite(dy).all()), 'dy of %s has elements its BatchNorm backward did not write' % c.name
            if exact_kink:
                try:
                    # the implementation's own evaluation of the BatchNorm output (fp32, its saved mean / invstd)
                    v4 = lambda t: t.detach().float().cpu().view(1, -1, 1, 1)
                    a_impl = v4(gam) * ((yraw - v4(op['mean'])) * v4(op['invstd'])) + v4(bet)
                    flips = _kink_flips(dy, dy_ref, aref, tol, a_impl=a_impl)
                except AssertionError as e:
                    raise AssertionError('bn bwd dy %s: %s' % (c.name, str(e).splitlines()[0]))
                if bool(flips.any()):
                    nflip[0] += int(flips.sum())
                    _, dy_ref, dg_ref, db_ref, _ = ot.bn_act_backward(yraw, gam, bet, dz, flip=flips)
            note('bn bwd dy', c.name, _rel(dy, rb(dy_ref.float())), tol)
            note('dgamma', c.name, _rel(grads[c.name + '.gamma'].cpu(), dg_ref), tol_w)
            note('dbeta', c.name, _rel(grads[c.name + '.beta'].cpu(), db_ref), tol_w)
            dw_ref = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride=c.stride, padding=c.k // 2)
            note('wgrad', c.name, _rel(grads[c.name + '.weight'].cpu(), dw_ref), tol_w)
            if id(z) in consumers:
                note('dgrad (d/dz)', c.name, _rel(dz, rb(grad_ref(z))), tol)
        elif op['kind'] == 'out':
            c, xin = op['c'], op['x']
            x = _nchw(xin.val)
            dyp = op['dyp'].float()[:, :c.cout].view(xin.shape[0], xin.shape[1], xin.shape[2], c.cout)
            w = params[c.name + '.weight'].detach().float().cpu()
            dw_ref = torch.nn.grad.conv2d_weight(x, w.shape, _nchw(dyp), stride=1, padding=0)
            note('wgrad', c.name, _rel(grads[c.name + '.weight'].cpu(), dw_ref), tol_w)
            note('dbias', c.name, _rel(grads[c.name + '.bias'].cpu(), dyp.sum(dim=(0, 1, 2)).cpu()), tol_w)
        else:
            note('dgrad (d/dcat)', 'upcat', _rel(_nchw(op['cat'].grad), rb(grad_ref(op['cat']))), tol)
    worst['kink flips'] = (nflip[0], '')
    return worst


def _d53(cuda, dtype, B, tune='auto', seed_lab=3, render_rate=0.0):
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    spec = og.spec_d53()
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((B, 3) + SIZE, dtype=np.float32)
    lab = ot.synthetic_labels(B, seed=seed_lab, render_rate=render_rate, num_class=24)
    net = CarNet(spec, dtype=dtype, device=cuda, tune=tune).load_params(P)
    return spec, g, P, x, lab, net, Trainer(net, SIZE)


def test_d53_train_step_f32_vs_oracle(cuda):
    """BASELINE configs[2] geometry at B=2, fp32 path: train-mode logits, the five losses and the gradients against the
    oracle's autograd restatement of _train_batch; then every value of the step one hop from its reference (<= 1e-4)."""
    spec, g, P, x, lab, net, tr = _d53(cuda, 'f32', 2)
    cap = {}
    losses = tr.train_step(torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda), update=False, capture=cap)
    torch.cuda.synchronize()
    worst = _one_hop_check(tr, tr._last[0], cap, net.params, 1e-4, 1e-4, lambda t: t)
    print('one-hop worst (fp32):', worst)
    rl, rg, rmerged = ot.train_step_reference(g, P, x, lab, spec, SIZE)
    merged = tr.merged_logits().cpu().numpy()
    assert np.abs(merged - rmerged).max() / np.abs(rmerged).max() < 1e-4
    np.testing.assert_allclose(losses.cpu().numpy(), np.stack(rl), rtol=1e-3, atol=1e-7)
    grads = tr.grads()
    assert set(grads) == set(rg)
    rel = {n: float(np.linalg.norm(grads[n].cpu().numpy().astype(np.float64) - rg[n]) / (np.linalg.norm(rg[n]) + 1e-30)) for n in rg}
    # End to end only the output convolutions (no activation between them and the loss) can be tight: a forward that
    # differs by 1e-5 relative flips LeakyReLU' for ~1e-5 of the elements, each flip changes that element's gradient
    # tenfold, i.e. ~sqrt(1e-5) = 3e-3 of the L2 norm PER LAYER.  Everything else is held by the one-hop check above.
    outs_ = [n for n in rel if '.out.' in n]
    assert len(outs_) == 6 and max(rel[n] for n in outs_) < 1e-3, max((rel[n], n) for n in outs_)
    print('end-to-end gradient L2 errors: median %.3g, worst %.3g (%s)' % (np.median(list(rel.values())), max(rel.values()), max(rel, key=rel.get)))
    assert max(rel.values()) < 0.15 and np.median(list(rel.values())) < 2e-2, (max(rel.values()), np.median(list(rel.values())))


def test_d53_train_step_bf16_one_hop(cuda):
    """The bench configuration's arithmetic (bf16 activations and activation gradients, MFMA bf16 convolutions,
    transposing-read weight gradients, sub-pixel stride-2 data gradients) at the D53 layer shapes: one hop from the
    reference on the bf16-rounded saved operands.  An activation is stored with ONE bf16 rounding (2^-9 relative);
    the weight gradients accumulate in fp32.  Bar for a stored activation: 2.5 bf16 ulps of the largest element (the HIP
    fp32 value and the float64 reference can round to neighbouring bf16 values: one ulp = 2^-7 relative)."""
    spec, g, P, x, lab, net, tr = _d53(cuda, 'bf16', 4, tune='measure')
    cap = {}
    losses = tr.train_step(torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda), update=False, capture=cap)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all())
    rb = lambda t: t.to(torch.bfloat16).float()
    worst = _one_hop_check(tr, tr._last[0], cap, net.params, 2e-2, 2e-3, rb)
    print('one-hop worst (bf16):', worst)
    rl, _, _ = ot.train_step_reference(g, P, x, lab, spec, SIZE, sim_bf16=True)
    np.testing.assert_allclose(losses.cpu().numpy(), np.stack(rl), rtol=5e-2, atol=5e-3)


def test_d53_train_bs64_bf16_replicated_batch(cuda):
    """BASELINE configs[2] at its own size (bs 64, bf16, measured kernel variants).  The oracle cannot run 64 images
    (70 GB of autograd state), so the batch is 32 copies of a 2-image batch: batch statistics over the copies equal the
    2-image statistics, hence every copy's losses must equal the oracle's B=2 losses and all copies must agree.  Then the
    loss must fall over 10 updates."""
    spec, g, P, x2, lab2, net, tr = _d53(cuda, 'bf16', 2, tune='measure')
    x = torch.from_numpy(np.tile(x2, (32, 1, 1, 1))).to(cuda)
    lab = torch.from_numpy(np.tile(lab2, (32, 1, 1))).to(cuda)
    losses = tr.train_step(x, lab, update=False)
    torch.cuda.synchronize()
    L = losses.cpu().numpy()
    assert L.shape == (5, 64) and np.isfinite(L).all()
    rl, _, _ = ot.train_step_reference(g, P, x2, lab2, spec, SIZE, sim_bf16=True)
    np.testing.assert_allclose(L[:, :2], np.stack(rl), rtol=5e-2, atol=5e-3)
    for k in range(1, 32):
        np.testing.assert_allclose(L[:, 2 * k:2 * k + 2], L[:, :2], rtol=1e-5, atol=1e-7)
    # (the gradients of this configuration are held one hop at a time, on the device, by
    #  test_d53_train_bs64_bf16_device_one_hop below -- the loose whole-step cosine bars this test used to carry are gone)
    first = float(tr.train_step(x, lab).sum())
    for _ in range(9):
        last = float(tr.train_step(x, lab).sum())
    assert np.isfinite(last) and last < first, (first, last)


def _taps_conv(x, w, stride):
    """Raw convolution (pad k//2) of NHWC fp32 x (N,H,W,Cin) with OIHW fp32 w as one fp32 matmul per tap (rocBLAS; no MIOpen)."""
    N, H, W, Cin = x.shape
    Cout, _, k, _ = w.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p))
    y = torch.zeros((N * Ho * Wo, Cout), dtype=torch.float32, device=x.device)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :].reshape(-1, Cin)
            y += xs @ w[:, :, kh, kw].t()
    return y.view(N, Ho, Wo, Cout)


def _taps_dgrad(dy, w, stride, H, W):
    """d/dx of the same convolution: scatter of dy @ w[:, :, kh, kw] per tap into the padded input grid."""
    N, Ho, Wo, Cout = dy.shape
    _, Cin, k, _ = w.shape
    p = k // 2
    dxp = torch.zeros((N, H + 2 * p, W + 2 * p, Cin), dtype=torch.float32, device=dy.device)
    d2 = dy.reshape(-1, Cout)
    for kh in range(k):
        for kw in range(k):
            dxp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :] += (d2 @ w[:, :, kh, kw]).view(N, Ho, Wo, Cin)
    return dxp[:, p:p + H, p:p + W, :]


def _taps_wgrad(x, dy, k, stride):
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    p = k // 2
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p))
    dw = torch.empty((Cout, Cin, k, k), dtype=torch.float32, device=x.device)
    d2 = dy.reshape(-1, Cout)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :].reshape(-1, Cin)
            dw[:, :, kh, kw] = d2.t() @ xs
    return dw


@pytest.mark.parametrize('kernels', KERNEL_SETS)
def test_d53_train_bs64_bf16_device_one_hop(cuda, kernels):
    """BASELINE configs[2] at its own size and arithmetic -- bs 64, bf16, measured kernel variants, 64 DIFFERENT images, half
    of them without an object -- held one hop at a time ON THE DEVICE (the CPU oracle cannot hold 64 images): for a spread of
    layers that covers every kernel family at its full-size launch (the fused-statistics forward convolutions, the split-pixel
    atomics of the strip / row-walk / per-tap / GEMM weight gradients, the sub-pixel stride-2 data gradient, the channel-group
    BatchNorm reductions) the raw convolution, BatchNorm forward + backward, the weight gradient and the data gradient are
    re-derived with plain fp32 torch-ROCm matmuls from the operands the kernels themselves read.  Same bars as the B=4
    one-hop test: 2.5 bf16 ulps of the largest element for stored activations, 2e-3 for fp32 weight gradients."""
    from yolo_amd.spec import LEAKY_SLOPE
    spec, g, P, _, _, net, tr = _d53(cuda, 'bf16', 2, tune='measure')
    pinned = pin_kernels(tr, kernels)              # ('plan': profiles/plan.json's forward / data-gradient / weight-gradient choices)
    B = 64
    x = torch.rand((B, 3) + SIZE, generator=torch.Generator().manual_seed(11)).to(cuda)
    lab = torch.from_numpy(ot.synthetic_labels(B, seed=5, render_rate=0.5, num_class=24)).to(cuda)
    tr.train_step(x, lab, update=False)                                        # (measures the variants at this batch size)
    net.load_params(P)
    cap = {}
    losses = tr.train_step(x, lab, update=False, capture=cap)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all())
    plan = tr._last[0]
    ops = {op['c'].name: op for op in plan.fwd if op['kind'] == 'conv_bn'}
    rb = lambda t: t.to(torch.bfloat16).float()
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))
    tol, tol_w = 2e-2, 2e-3
    layers = ['stem', 'stages.0.down', 'stages.0.res.0.c1', 'stages.0.res.0.c2', 'stages.1.down', 'stages.1.res.1.c2',
              'stages.2.down', 'stages.2.res.0.c1', 'stages.2.res.0.c2', 'stages.3.res.7.c2', 'stages.4.res.3.c2',
              'heads.0.b1', 'heads.0.b2', 'heads.1.b3', 'heads.2.b0', 'heads.2.tip', 'transitions.1']
    worst = {}

    def note(kind, name, err, bar):
        worst[kind] = max(worst.get(kind, (0, '')), (err, name))
        assert err < bar, '%s %s: relative error %.3g (bar %.1g)' % (kind, name, err, bar)

    grads = tr.grads()
    for name in layers:
        op = ops[name]
        c = op['c']
        w = rb(net.params[name + '.weight'].detach().float())
        xin = op['x'].val.float()[..., :c.cin]
        yraw = op['yraw'].val.float()
        # forward: raw convolution of the saved input; BatchNorm + LeakyReLU (+ residual) of the saved raw output
        note('conv fwd', name, rel(yraw, rb(_taps_conv(xin, w, c.stride))), tol)
        gam, bet = net.params[name + '.gamma'].float(), net.params[name + '.beta'].float()
        n = yraw.shape[0] * yraw.shape[1] * yraw.shape[2]
        mean = yraw.double().mean(dim=(0, 1, 2))
        var = (yraw.double() - mean).pow(2).mean(dim=(0, 1, 2))
        assert rel(op['mean'], mean.float()) < 1e-4 and rel(op['invstd'], (1.0 / torch.sqrt(var + 1e-5)).float()) < 1e-4
        xh = (yraw - op['mean']) * op['invstd']
        a = gam * xh + bet
        z = torch.where(a > 0, a, a * LEAKY_SLOPE)
        if op['res'] is not None:
            z = z + op['res'].val.float()
        note('bn fwd', name, rel(op['z'].val.float(), rb(z)), tol)
        # backward: dy, dgamma, dbeta from the captured dz
        dz, dy = cap[name]['dz'].float(), cap[name]['dy'].float()
        assert bool(torch.isfinite(dy).all())
        da = dz * torch.where(a > 0, 1.0, LEAKY_SLOPE)
        s1, s2 = da.double().sum(dim=(0, 1, 2)), (da * xh).double().sum(dim=(0, 1, 2))
        ref = gam * op['invstd'] * (da - (s1 / n).float() - xh * (s2 / n).float())
        off = ((dy - rb(ref)).abs() > tol * ref.abs().max()) & (a.abs() > 1e-3)          # (near the kink either branch is right)
        assert not bool(off.any()), 'bn bwd dy %s: %d elements off, %d of them exact zeros' % (name, int(off.sum()), int((dy[off] == 0).sum()))
        note('dgamma', name, rel(grads[name + '.gamma'], s2.float()), tol_w)
        note('dbeta', name, rel(grads[name + '.beta'], s1.float()), tol_w)
        # weight gradient of the convolution from the dy the kernel read (fp32 accumulation of the bf16 operands)
        note('wgrad', name, rel(grads[name + '.weight'], _taps_wgrad(xin, dy, c.k, c.stride)), tol_w)
        del xin, yraw, xh, a, z, dz, dy, da, ref, off
    # data gradients: a producer whose ONLY consumer is one convolution receives exactly that convolution's data gradient
    pairs = [('stem', 'stages.0.down'), ('stages.0.res.0.c2', 'stages.1.down'), ('stages.0.res.0.c1', 'stages.0.res.0.c2'),
             ('stages.1.res.1.c1', 'stages.1.res.1.c2'), ('stages.2.res.0.c1', 'stages.2.res.0.c2'),
             ('stages.3.res.7.c1', 'stages.3.res.7.c2'), ('stages.4.res.3.c1', 'stages.4.res.3.c2'),
             ('heads.0.b1', 'heads.0.b2'), ('heads.1.b0', 'heads.1.b1'), ('heads.2.b3', 'heads.2.b4')]
    nuse = {}
    for op in plan.fwd:
        for k_ in ('x', 'res', 'up', 'route'):
            t = op.get(k_)
            if t is not None:
                nuse[id(t)] = nuse.get(id(t), 0) + 1
    for prod, cons in pairs:
        po, co = ops[prod], ops[cons]
        assert co['x'] is po['z'] and nuse[id(po['z'])] == 1, (prod, cons)
        c = co['c']
        w = rb(net.params[cons + '.weight'].detach().float())
        N_, H_, W_, _ = po['z'].shape
        ref = _taps_dgrad(cap[cons]['dy'].float(), w, c.stride, H_, W_)
        note('dgrad s%d k%d' % (c.stride, c.k), cons, rel(cap[prod]['dz'].float(), rb(ref)), tol)
        del ref
    print('bs-64 device one-hop worst:', worst)
    assert_plan_held(tr, pinned, 'train_416_bs64_bf16_one_hop')


def test_d53_608_forward(cuda):
    """BASELINE configs[4] geometry: D53 spec at 608x608 (N = 7581 cells, 22 743 boxes), B=1: fp32 logits within 1e-3 of
    the oracle, bf16 as good as the rounding-aware oracle; decode + top-1 + NMS on the real logits."""
    from yolo_amd.net import CarNet
    from yolo_amd.detect import Detector
    spec, size = og.spec_d53(), (608, 608)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((1, 3) + size, dtype=np.float32)
    ref = [r.numpy() for r in of.forward_torch(g, P, x)]
    assert [r.shape for r in ref] == [(1, 5776, 3, 30), (1, 1444, 3, 30), (1, 361, 3, 30)]
    xt = torch.from_numpy(x).to(cuda)
    net = CarNet(spec, dtype='f32', device=cuda, tune='measure').load_params(P)
    outs = net(xt)
    for o, r in zip(outs, ref):
        np.testing.assert_allclose(o.cpu().numpy(), r, rtol=0, atol=1e-3)
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    syxhw = od.init_syxhw(size, steps, spec['all_anchors'])
    det = Detector(spec, size, steps, device=cuda)
    pred, idx = det.predict_device(outs)
    hip_logits = [o.cpu().numpy() for o in outs]
    rpred, ridx = od.predict(hip_logits, spec['slice_point'], size, syxhw)
    assert idx.cpu().tolist() == ridx.tolist()                                          # bit-exact index
    np.testing.assert_allclose(pred.cpu().numpy(), rpred, rtol=1e-5, atol=1e-6)
    rows = det.decode(outs)
    ref_rows = od.decode_all(ref, spec['slice_point'], size, syxhw)
    err = np.abs(rows.cpu().numpy()[..., :5] - ref_rows[..., :5]) / (1.0 + np.abs(ref_rows[..., :5]))
    assert err.max() < 1e-3
    scores = det.nms_scores(rows, 'class')
    kept, ks, cnt = det.nms(rows, 'class', scores=scores)
    rk, rs = od.nms(rows.cpu().numpy()[0], mode='class', scores=scores.cpu().numpy()[0])    # (bit-identical inputs)
    n = int(cnt[0])
    assert n == len(rk) and kept[0, :n].cpu().tolist() == list(rk)                     # kept ids bit-exact
    # bf16, measured variants
    net16 = CarNet(spec, dtype='bf16', device=cuda, tune='measure').load_params(P)
    outs16 = [o.cpu().numpy() for o in net16(xt)]
    sim = [s.numpy() for s in of.forward_torch_bf16sim(g, P, x)]
    rms = lambda a: float(np.sqrt(np.mean(a * a)))
    for o, s, r in zip(outs16, sim, ref):
        e_hip, e_sim = rms(o - r) / r.std(), rms(s - r) / r.std()
        assert e_hip < 1.5 * e_sim + 1e-3 and e_hip < 0.015, (e_hip, e_sim)


@pytest.mark.parametrize('kernels', KERNEL_SETS)
def test_config4_608_bs64_measured_plan_replicated(cuda, kernels):
    """The north-star shape as bench.py runs it (BASELINE configs[4] per GPU: D53 spec, 608x608, bs 64, bf16, measured kernel
    variants).  A size-independent property at the full size: eval-mode images are independent, so a batch that repeats two
    images must return each of them bit-identically wherever it sits in the batch (pixel tiles cross image boundaries at
    other offsets for every copy: 32 different tile alignments per layer) -- and both against the rounding-aware oracle."""
    from yolo_amd.net import CarNet
    spec, size = og.spec_d53(), (608, 608)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    two = np.random.default_rng(5).random((2, 3) + size, dtype=np.float32)
    x = torch.from_numpy(two).to(cuda).repeat(32, 1, 1, 1)                 # a, b, a, b, ...
    net = CarNet(spec, dtype='bf16', device=cuda, tune='measure').load_params(P)
    pinned = pin_kernels(net, kernels)
    outs = [o.clone() for o in net(x)]
    assert_plan_held(net, pinned, 'configs4_608_bs64_bf16')
    assert len({op[1].algo for op in net._last_plan.ops if op[0] == 'conv'}) > 3
    for o in outs:
        assert o.shape[0] == 64 and bool(torch.isfinite(o).all())
        assert bool((o[0::2] == o[0:1]).all()) and bool((o[1::2] == o[1:2]).all())
        assert not bool((o[0] == o[1]).all())
    ref = [r.numpy() for r in of.forward_torch(g, P, two)]
    sim = [s_.numpy() for s_ in of.forward_torch_bf16sim(g, P, two)]
    rms = lambda a: float(np.sqrt(np.mean(a * a)))
    for o, s_, r in zip(outs, sim, ref):
        got = o[:2].cpu().numpy()
        e_hip, e_sim = rms(got - r) / r.std(), rms(s_ - r) / r.std()
        assert e_hip < 1.5 * e_sim + 1e-3 and e_hip < 0.015, (e_hip, e_sim)


@pytest.mark.parametrize('kernels', KERNEL_SETS)
@pytest.mark.parametrize('dtype', ['f32', 'bf16x3', 'bf16', 'f16'])
def test_config1_bs32_measured_plan(cuda, dtype, kernels):
    """BASELINE configs[1] as bench.py runs it: D53 spec, 416x416, bs 32, per-layer kernel variants pinned by
    measurement (tile quantisation is batch dependent: the bs-32 plan picks other variants than a B=2 plan).  Images
    0, 1 and 31 of the batch against the oracle (eval-mode BN: images are independent)."""
    from yolo_amd.net import CarNet
    spec = og.spec_d53()
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(7).random((32, 3) + SIZE, dtype=np.float32)
    net = CarNet(spec, dtype=dtype, device=cuda, tune='measure').load_params(P)
    pinned = pin_kernels(net, kernels)
    outs = [o.cpu().numpy() for o in net(torch.from_numpy(x).to(cuda))]
    assert_plan_held(net, pinned, 'configs1_416_bs32_%s' % dtype)
    assert len({op[1].algo for op in net._last_plan.ops if op[0] == 'conv'}) > 3       # a mix of pinned variants
    sel = [0, 1, 31]
    ref = [r.numpy() for r in of.forward_torch(g, P, x[sel])]
    if dtype in ('f32', 'bf16x3'):            # the two paths held to the north-star tolerance: exact fp32 and split bf16 (three MFMAs per product)
        for o, r in zip(outs, ref):
            np.testing.assert_allclose(o[sel], r, rtol=0, atol=1e-3)
        return
    # (f16 = the reference's use_fp16, car/YOLO.py:98-100: the rounding-aware oracle rounds to IEEE half; its error is ~8x smaller
    #  than bf16's, and so are the bars)
    sim_fn, bar, slack = (of.forward_torch_bf16sim, 0.015, 1e-3) if dtype == 'bf16' else (of.forward_torch_f16sim, 0.002, 2e-4)
    sim = [s.numpy() for s in sim_fn(g, P, x[sel])]
    rms = lambda a: float(np.sqrt(np.mean(a * a)))
    for o, s, r in zip(outs, sim, ref):
        e_hip, e_sim = rms(o[sel] - r) / r.std(), rms(s - r) / r.std()
        assert e_hip < 1.5 * e_sim + slack and e_hip < bar, (e_hip, e_sim)
        for k in range(3):                                                              # every image on its own, too
            assert rms(o[sel[k]] - r[k]) / r.std() < bar * 4 / 3


def test_tune_plan_is_the_benched_and_tested_kernel_set(cuda):
    """`CarNet(spec, tune='plan')` -- what INTEGRATION.md section 2 tells a maintainer to write -- launches, for BASELINE configs[1],
    exactly the kernel instantiations bench.py launches (tune='measure' + the plan file loaded) and the `kernels='plan'` parity
    tests above compare with the oracle: same launch list, bit-identical logits; nothing is timed, a shape the plan does not
    hold gets the heuristic's variant (and the Trainer of such a net adopts the plan's gradient-kernel choices)."""
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    from yolo_amd import plans
    spec = og.spec_d53()
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = torch.from_numpy(np.random.default_rng(7).random((32, 3) + SIZE, dtype=np.float32)).to(cuda)
    state, meta = plans.load(plans.DEFAULT)
    for dtype in ('bf16', 'bf16x3'):
        a = CarNet(spec, dtype=dtype, device=cuda, tune='plan').load_params(P)
        b = CarNet(spec, dtype=dtype, device=cuda, tune='measure').load_params(P)
        b.load_tuning_state(state)
        oa = [o.clone() for o in a(x)]
        ob = b(x)
        assert a.plan_signature(32, *SIZE) == b.plan_signature(32, *SIZE)
        assert all(bool((p_ == q_).all()) for p_, q_ in zip(oa, ob))
        assert plans.new_keys(a.tuning_state(), state) == 0 and a.stale_choices == 0
    small = CarNet(spec, dtype='bf16', device=cuda, tune='plan').load_params(P)        # B = 2: not in the plan -> heuristic, no timing
    outs = small(x[:2])
    assert plans.new_keys(small.tuning_state(), state) == 0
    ref = CarNet(spec, dtype='bf16', device=cuda, tune='auto').load_params(P)(x[:2])
    for o, r in zip(outs, ref):
        assert float((o - r).abs().max()) <= 0.05 * float(r.abs().max())
    tr = Trainer(CarNet(spec, dtype='bf16', device=cuda, tune='plan').load_params(P), SIZE)
    held = tr.tuning_state()
    assert len(held['wgrad']) == len(state['wgrad']) and len(held['dgrad']) == len(state['dgrad'])
