"""GPU parity of the training step (yolo_amd.train.Trainer, fp32 path) against the oracle's torch-autograd
restatement of _train_batch (car/YOLO.py:350-399): train-mode BN forward, target assignment, the five
losses, every parameter gradient, and the MXNet-formula Adam update."""
import numpy as np
import pytest
import torch

from oracle import graph as og, train as ot, detect as od

pytestmark = pytest.mark.gpu


def _setup(cuda, B=2, seed_lab=1, render_rate=0.0, dtype='f32'):
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    spec, size = og.spec_micro(), (64, 96)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((B, 3) + size, dtype=np.float32)
    lab = ot.synthetic_labels(B, seed=seed_lab, render_rate=render_rate, num_class=4)
    net = CarNet(spec, dtype=dtype, device=cuda).load_params(P)
    tr = Trainer(net, size)
    return spec, size, g, P, x, lab, net, tr


def _close(a, b, rtol, name):
    scale = np.abs(b).max() + 1e-12
    err = np.abs(a - b).max() / scale
    assert err < rtol, '%s: max err %.3g of scale %.3g' % (name, err * scale, scale)


def test_assign_targets(cuda):
    spec, size, g, P, x, lab, net, tr = _setup(cuda, B=6, seed_lab=5)
    lab[3] = -1                                                   # an image without object
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    area = od.init_area(size, steps)
    ltrb = od.get_default_ltrb(size, steps, spec['all_anchors'])
    np.testing.assert_array_equal(tr.anchors_ltrb.cpu().numpy(), ltrb)      # bit-identical anchor boxes
    tr.train_step(torch.from_numpy(x[:1].repeat(6, 0)).to(cuda), torch.from_numpy(lab).to(cuda), update=False)
    rec = tr._last[1].cpu().numpy()
    for b in range(6):
        if lab[b, 0, 0] < 0:
            assert rec[b, 0, 0] == 0
            continue
        px, anc, box = ot.find_best(lab[b, 0], ltrb, spec['all_anchors'], size, steps, area)
        assert rec[b, 0, 0] == 1 and int(rec[b, 0, 1]) == px * 3 + anc       # bit-exact index
        np.testing.assert_allclose(rec[b, 0, 2:6], box, rtol=1e-5, atol=1e-6)
        np.testing.assert_array_equal(rec[b, 0, 6:], lab[b, 0, 5:])


def test_train_step_losses_and_grads(cuda):
    spec, size, g, P, x, lab, net, tr = _setup(cuda)
    losses = tr.train_step(torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda), update=False)
    rl, rg, rmerged = ot.train_step_reference(g, P, x, lab, spec, size)
    _close(tr.merged_logits().cpu().numpy(), rmerged, 1e-4, 'train-mode logits')
    np.testing.assert_allclose(losses.cpu().numpy(), np.stack(rl), rtol=1e-3, atol=1e-7)
    grads = tr.grads()
    assert set(grads) == set(rg)
    # LeakyReLU' is discontinuous: the two forwards differ by ~1e-5 relative (fp32 accumulation order), which
    # flips the sign of a handful of near-zero pre-activations and moves individual gradient entries by
    # percents (measured: feeding the oracle's own backward with the HIP forward's activations reproduces
    # the HIP gradients to 1e-6).  So the whole-step bar is an L2 one; the strict element-wise parity of
    # every backward building block is in tests/test_gpu_train_ops.py.
    rel = {}
    for name in sorted(rg):
        a, b = grads[name].cpu().numpy().astype(np.float64), rg[name].astype(np.float64)
        rel[name] = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
    worst = max(rel, key=rel.get)
    assert rel[worst] < 0.1, (worst, rel[worst])
    assert np.median(list(rel.values())) < 2e-3, np.median(list(rel.values()))
    assert np.mean([v < 1e-2 for v in rel.values()]) > 0.8


def test_train_step_with_rotation_loss_and_score_weights(cuda):
    """_train_batch(..., car_rotate=True) (car/YOLO.py:350, 491-496) with a non-zero rotation scale and score weights that are not
    the defaults: the third Huber group end to end, against the oracle switched the same way."""
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    spec, size = og.spec_micro(), (64, 96)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((2, 3) + size, dtype=np.float32)
    lab = ot.synthetic_labels(2, seed=1, render_rate=0.0, num_class=4)
    assert (lab[:, 0, 0] >= 0).all() and (lab[:, 0, 5] != 0).all()           # every image has an object with a non-zero rotation
    scale = dict(ot.DEFAULT_SCALE, rotate=0.5)
    kw = dict(scale=scale, car_rotate=True, positive_weight=2.0, negative_weight=0.2)
    net = CarNet(spec, dtype='f32', device=cuda).load_params(P)
    tr = Trainer(net, size, **kw)
    losses = tr.train_step(torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda), update=False).cpu().numpy()
    rl, rg, rmerged = ot.train_step_reference(g, P, x, lab, spec, size, **kw)
    np.testing.assert_allclose(losses, np.stack(rl), rtol=1e-3, atol=1e-7)
    assert (losses[3] != 0).all() and (np.stack(rl)[3] != 0).all()
    grads = tr.grads()
    assert set(grads) == set(rg)
    rel = {}
    for name in sorted(rg):                                                  # the three L2 conditions of test_train_step_losses_and_grads
        a, b = grads[name].cpu().numpy().astype(np.float64), rg[name].astype(np.float64)
        rel[name] = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
    worst = max(rel, key=rel.get)
    assert rel[worst] < 0.1, (worst, rel[worst])
    assert np.median(list(rel.values())) < 2e-3, np.median(list(rel.values()))
    assert np.mean([v < 1e-2 for v in rel.values()]) > 0.8
    # the rotation channel of d(losses)/d(logits), at the step's own logits (no forward difference in the way)
    merged = tr.merged_logits().cpu().numpy()
    _, gout, _ = ot.loss_and_grad_wrt_output(merged, lab, spec, size, scale, 2.0, 0.2, car_rotate=True)
    dm = tr._last[0].dmerged.cpu().numpy().reshape(gout.shape)
    top = np.abs(gout[..., 5]).max()
    assert top > 0 and np.abs(dm[..., 5] - gout[..., 5]).max() <= 1e-4 * top


def test_loss_grad_wrt_logits(cuda):
    """d(sum of losses)/d(logits) alone, on random logits (isolates loss.hip from the network)."""
    from yolo_amd import lib as L
    import ctypes as C
    spec, size, g, P, x, lab, net, tr = _setup(cuda, B=3, seed_lab=9)
    merged = (1.5 * np.random.default_rng(3).standard_normal((3, tr.nbox // 3, 3, 10))).astype(np.float32)
    rl, gout, _ = ot.loss_and_grad_wrt_output(merged, lab, spec, size)
    lib = tr.lib
    logits = torch.from_numpy(merged).to(cuda).contiguous()
    labels = torch.from_numpy(lab).to(cuda)
    rec = torch.empty((3, 1, 7 + 4), device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.yolo_assign_targets(labels.data_ptr(), tr.anchors_ltrb.data_ptr(), rec.data_ptr(), 3, 1, 4, C.byref(tr.grid), st) == 0
    dl = torch.empty_like(logits); ls = torch.empty((5, 3), device=cuda)
    s5 = (C.c_float * 5)(0.1, 0.01, 10.0, 0.0, 0.3)
    assert lib.yolo_loss_fwd_bwd(logits.data_ptr(), rec.data_ptr(), dl.data_ptr(), ls.data_ptr(), 3, tr.nbox, 10, 1, s5, 1.0, 0.1, st) == 0
    np.testing.assert_allclose(ls.cpu().numpy(), np.stack(rl), rtol=1e-4, atol=1e-8)
    _close(dl.cpu().numpy().reshape(gout.shape), gout, 1e-4, 'dlogits')


@pytest.mark.parametrize('n,offset', [(4099, 0), (4099, 1), (3, 0), (8, 3)])
def test_adam_c_abi_vector_and_unaligned(cuda, n, offset):
    """yolo_adam_step / yolo_adam_step_dev straight through the C ABI, on arrays of any length and alignment: the host-scalar and
    the device-slot rescale give the same bits, nothing outside the n elements is touched, and the values are the oracle's."""
    import ctypes as C
    from yolo_amd import lib as L
    lib = L.load()
    rng = np.random.default_rng(n + offset)
    host = [rng.standard_normal(n).astype(np.float32) for _ in range(3)] + [np.abs(rng.standard_normal(n)).astype(np.float32)]
    def run(off, dev_slot):
        bufs = [torch.zeros(n + 8, device=cuda) for _ in range(4)]
        views = [b[off:off + n] for b in bufs]
        for vw, h in zip(views, host):
            vw.copy_(torch.from_numpy(h))
        w, g, m, v = views
        st = torch.cuda.current_stream().cuda_stream
        if dev_slot:
            gb = torch.full((1,), 4.0, device=cuda)
            rc = lib.yolo_adam_step_dev(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 3, C.c_float(1e-3), C.c_float(0.9),
                                        C.c_float(0.999), C.c_float(1e-8), gb.data_ptr(), st)
        else:
            rc = lib.yolo_adam_step(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 3, C.c_float(1e-3), C.c_float(0.9),
                                    C.c_float(0.999), C.c_float(1e-8), C.c_float(0.25), st)
        assert rc == 0
        torch.cuda.synchronize()
        for b, vw in zip(bufs, views):                     # nothing outside the n elements is touched
            assert float(b[:off].abs().sum()) == 0 and float(b[off + n:].abs().sum()) == 0
        return [x.cpu().numpy().copy() for x in (w, m, v)]
    ref = run(0, False)
    for got in (run(offset, False), run(offset, True)):
        for a_, b_ in zip(got, ref):
            assert np.array_equal(a_.view(np.int32), b_.view(np.int32))
    w, g, m, v = (h.copy() for h in host)
    ot.adam_step(w, g, m, v, 3, lr=1e-3, rescale=0.25)
    np.testing.assert_allclose(ref[0], w, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(ref[1], m, rtol=1e-5, atol=1e-7)     # (1.f - beta in fp32 on the device, in double in the oracle)
    np.testing.assert_allclose(ref[2], v, rtol=1e-5, atol=1e-8)


def test_train_step_rejects_malformed_labels(cuda):
    """Label tensors of the wrong rank, batch or row width raise ValueError before anything is launched (their rows would be
    read with the wrong stride); CPU / float64 labels are converted."""
    spec, size, g, P, x, lab, net, tr = _setup(cuda)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    w = tr.wflat.clone()
    for bad in (lt[..., :-1], lt[:, 0], lt[:1], torch.cat([lt, lt], dim=0), lt[:, :0]):
        with pytest.raises(ValueError):
            tr.train_step(xt, bad)
    with pytest.raises(ValueError):
        tr.train_step(torch.rand((2, 3, size[0] + 32, size[1]), device=cuda), lt)
    assert torch.equal(w, tr.wflat) and tr.t == 0
    a = tr.train_step(xt, lt, update=False)
    b = tr.train_step(xt, lt.cpu().double(), update=False)
    assert torch.equal(a, b)


def test_trainer_for_another_size_keeps_the_optimiser_state(cuda):
    """net.trainer(size) for a new image size: new grid and plan, the same hyper-parameters, Adam moments and update count."""
    from yolo_amd.train import Trainer
    spec, size, g, P, x, lab, net, tr = _setup(cuda)
    tr = Trainer(net, size, learning_rate=3e-4, negative_weight=0.2)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    tr.train_step(xt, lt)
    m, v, w = tr.mflat.clone(), tr.vflat.clone(), tr.wflat.clone()
    other = (size[0] + 32, size[1])
    tr2 = net.trainer(other)
    assert tr2 is not tr and tr2.size == other and net.trainer() is tr2
    assert tr2.t == 1 and tr2.lr == 3e-4 and tr2.neg_w == 0.2
    assert torch.equal(tr2.mflat, m) and torch.equal(tr2.vflat, v) and torch.equal(tr2.wflat, w)
    x2 = torch.rand((2, 3) + other, device=cuda)
    assert torch.isfinite(tr2.train_step(x2, lt)).all() and tr2.t == 2
    assert net.trainer(other) is tr2                                   # same size again: the same object


def test_save_state_writes_the_path_it_is_given(cuda, tmp_path):
    spec, size, g, P, x, lab, net, tr = _setup(cuda)
    path = str(tmp_path / 'weights.pt')
    net.save_state(path)
    import os
    assert os.path.exists(path) and not os.path.exists(path + '.npz')
    from yolo_amd.net import CarNet
    n2 = CarNet(spec, dtype='f32', device=cuda)
    n2.load_state(path)
    for k, v in net.params.items():
        assert torch.equal(v, n2.params[k]), k


def test_adam_update_and_second_step(cuda):
    spec, size, g, P, x, lab, net, tr = _setup(cuda)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    tr.train_step(xt, lt)                                           # step 1 with the update (global batch 2)
    # Adam in isolation: the oracle's MXNet-formula step applied to the gradients this very step produced
    # (they stay in the flat bucket until the next backward) must give the weights now in the net.
    for name, gr in tr.grads().items():
        w = P[name].copy(); m = np.zeros_like(w); v = np.zeros_like(w)
        ot.adam_step(w, gr.cpu().numpy(), m, v, 1, lr=1e-3, rescale=1.0 / 2)
        np.testing.assert_allclose(net.params[name].cpu().numpy(), w, rtol=1e-5, atol=2e-7, err_msg=name)
    # running statistics: 0.9*r + 0.1*batch (biased variance)
    st = {}
    from oracle import forward as of
    of.forward_torch(g, P, x, training=True, bn_stats=st)
    for cname, (mean, var) in list(st.items())[:6]:
        np.testing.assert_allclose(net.params[cname + '.running_mean'].cpu().numpy(),
                                   0.9 * P[cname + '.running_mean'] + 0.1 * mean.numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(net.params[cname + '.running_var'].cpu().numpy(),
                                   0.9 * P[cname + '.running_var'] + 0.1 * var.numpy(), rtol=1e-4, atol=1e-6)
    l2 = tr.train_step(xt, lt)                                      # the re-packed weights are in use
    assert torch.isfinite(l2).all() and tr.t == 2


def test_inference_after_training_uses_the_updated_weights(cuda):
    """train -> validate -> train -> validate on ONE net (the reference's _valid_iou every valid_step,
    car/YOLO.py:501-534): every inference forward must see the weights and running statistics of the step before it
    (the folded scale/bias and the packed weight images are re-made), and load_params on a net that has a Trainer
    must reach the trainer's flat buffer."""
    from oracle import forward as of
    spec, size, g, P, x, lab, net, tr = _setup(cuda)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)

    def check(tag):
        Pn = {k: v.detach().cpu().numpy().copy() for k, v in net.params.items()}
        ref = of.forward_torch(g, Pn, x)
        outs = net(xt)
        torch.cuda.synchronize()
        for o, r in zip(outs, ref):
            err = float(np.abs(o.cpu().numpy() - r.numpy()).max())
            assert err < 1e-3, (tag, err)
        return [o.clone() for o in outs]

    o0 = check('before training')
    for _ in range(3):
        tr.train_step(xt, lt)
    o1 = check('after 3 steps')
    assert max(float((a - b).abs().max()) for a, b in zip(o0, o1)) > 1e-3          # the update was visible
    for _ in range(2):
        tr.train_step(xt, lt)
    o2 = check('after 5 steps')
    assert max(float((a - b).abs().max()) for a, b in zip(o1, o2)) > 1e-4
    tr.train_step(xt, lt, update=False)                  # no weight update, but the running statistics moved
    check('after a step without update')
    # load_params after the Trainer was built: in place, so the trainer trains the loaded weights
    net.load_params(P)
    o3 = check('after load_params')
    assert all(torch.equal(a, b) for a, b in zip(o0, o3))
    assert all(net.params[n].data_ptr() == v.data_ptr() for n, v in tr.pview.items())
    l_a = tr.train_step(xt, lt, update=False)
    spec2, size2, g2, P2, x2, lab2, net2, tr2 = _setup(cuda)
    l_b = tr2.train_step(xt, lt, update=False)
    np.testing.assert_allclose(l_a.cpu().numpy(), l_b.cpu().numpy(), rtol=1e-5, atol=1e-8)    # = a fresh trainer's losses


def test_training_reduces_loss(cuda):
    spec, size, g, P, x, lab, net, tr = _setup(cuda, B=4, seed_lab=3)
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    first = float(tr.train_step(xt, lt).sum())
    for _ in range(30):
        last = float(tr.train_step(xt, lt).sum())
    assert last < 0.7 * first, (first, last)


def test_train_step_bf16(cuda):
    """bf16 activations / activation gradients (MFMA bf16 convolutions + transposing-read weight gradient), fp32
    master weights, statistics and optimiser.  A randomly initialised net in train mode is chaotic in bf16: the
    ORACLE's own bf16-rounding simulation differs from its fp32 run by ~0.7 on the logits and 60-90 % on the
    early-layer gradients (measured), so the whole-step bar is directional agreement with that simulation; the
    strict element-wise parity of each bf16 building block is in tests/test_gpu_train_ops.py."""
    spec, size, g, P, x, lab, net, tr = _setup(cuda, B=4, seed_lab=3, dtype='bf16')
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda)
    losses = tr.train_step(xt, lt, update=False)
    rl, rg, _ = ot.train_step_reference(g, P, x, lab, spec, size, sim_bf16=True)
    np.testing.assert_allclose(losses.cpu().numpy(), np.stack(rl), rtol=5e-2, atol=5e-3)
    np.testing.assert_allclose(losses.cpu().numpy()[0], np.stack(rl)[0], rtol=1e-2)
    cos = {}
    for name in rg:
        a, b = tr.grads()[name].cpu().numpy().astype(np.float64).ravel(), rg[name].astype(np.float64).ravel()
        cos[name] = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
    assert np.median(list(cos.values())) > 0.85, np.median(list(cos.values()))
    assert min(cos.values()) > 0.3, min(cos, key=cos.get)
    first = float(tr.train_step(xt, lt).sum())
    for _ in range(30):
        last = float(tr.train_step(xt, lt).sum())
    assert last < 0.7 * first, (first, last)


def test_multiple_objects_per_image_with_collision(cuda):
    """labels (B, nobj=3, 6+C): the reference's scatter loop (car/YOLO.py:466-478) lets the LAST object that maps
    to a box overwrite the earlier one; rows with cls < 0 are skipped.  Assignment records, losses and d/d(logits)
    against the oracle."""
    import ctypes as C
    spec, size, g, P, x, lab1, net, tr = _setup(cuda, B=3, seed_lab=11)
    rng = np.random.default_rng(12)
    lab = -np.ones((3, 3, 6 + 4), np.float32)
    for b in range(3):
        for o in range(3):
            d = rng.random(4).astype(np.float32); d /= d.sum()
            lab[b, o, :6] = [int(np.argmax(d)), rng.uniform(.2, .8), rng.uniform(.2, .8), rng.uniform(.2, .9), rng.uniform(.2, .9), 0.1]
            lab[b, o, 6:] = d
    lab[0, 2, :5] = lab[0, 0, :5]            # image 0: objects 0 and 2 land on the same box (different class rows)
    lab[1, 1] = -1                           # image 1: a hole in the middle of the object list
    lab[2] = -1                              # image 2: no object at all
    merged = (1.5 * rng.standard_normal((3, tr.nbox // 3, 3, 10))).astype(np.float32)
    rl, gout, (y, mask, sw) = ot.loss_and_grad_wrt_output(merged, lab, spec, size)
    assert mask[0].sum() == 2 and mask[1].sum() == 2 and mask[2].sum() == 0
    lib = tr.lib
    logits = torch.from_numpy(merged).to(cuda).contiguous()
    labels = torch.from_numpy(lab).to(cuda)
    rec = torch.empty((3, 3, 7 + 4), device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.yolo_assign_targets(labels.data_ptr(), tr.anchors_ltrb.data_ptr(), rec.data_ptr(), 3, 3, 4, C.byref(tr.grid), st) == 0
    r = rec.cpu().numpy()
    assert r[0, 0, 1] == r[0, 2, 1] and r[1, 1, 0] == 0 and (r[2, :, 0] == 0).all()
    dl = torch.empty_like(logits); ls = torch.empty((5, 3), device=cuda)
    s5 = (C.c_float * 5)(0.1, 0.01, 10.0, 0.0, 0.3)
    assert lib.yolo_loss_fwd_bwd(logits.data_ptr(), rec.data_ptr(), dl.data_ptr(), ls.data_ptr(), 3, tr.nbox, 10, 3, s5, 1.0, 0.1, st) == 0
    np.testing.assert_allclose(ls.cpu().numpy(), np.stack(rl), rtol=1e-4, atol=1e-8)
    _close(dl.cpu().numpy().reshape(gout.shape), gout, 1e-4, 'dlogits')
    # and through the whole step (3 objects per image)
    losses = tr.train_step(torch.from_numpy(x[:1].repeat(3, 0)).to(cuda), labels, update=False)
    assert losses.shape == (5, 3) and bool(torch.isfinite(losses).all()) and float(losses[2, 2]) == 0.0


# ---- CarLPNet: joint car + licence-plate training step (car_and_LP/YOLO.py:262-300) ------------------------------
def _lp_setup(cuda, B=4, dtype='f32'):
    from yolo_amd.net import CarLPNet
    from yolo_amd.train import Trainer
    spec = dict(og.spec_micro(), LP_slice_point=[1, 3, 4, 7, 10], LP_r_max=[45, 60, 45])
    size = (64, 96)
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((B, 3) + size, dtype=np.float32)
    lab = ot.synthetic_labels(B, seed=1, render_rate=0.25, num_class=4)
    lpl = ot.synthetic_lp_labels(B, size, seed=2, add_rate=0.75)
    lpl[0, 0, 7:9] = [size[1] + 40.0, -3.0]                      # a plate centre outside the image: clipped to the edge cell
    lpl[0, 0, 0] = 1
    net = CarLPNet(spec, dtype=dtype, device=cuda).load_params(P)
    tr = Trainer(net, size, lp_r_max=spec['LP_r_max'])
    return spec, size, g, P, x, lab, lpl, net, tr


def test_lp_assignment_and_losses(cuda):
    import ctypes as C
    spec, size, g, P, x, lab, lpl, net, tr = _lp_setup(cuda)
    B = x.shape[0]
    step = od.init_steps(spec['layers'], spec['all_anchors'])[0]
    fh, fw = size[0] // step, size[1] // step
    lp_out = (1.5 * np.random.default_rng(5).standard_normal((B, fh, fw, 10))).astype(np.float32)
    scale = {'LP_score': 0.1, 'LP_xy': 10.0, 'LP_z': 1.0, 'LP_r': 0.1, 'LP_class': 0.3}     # (class term switched on)
    rl, gout, (y, mask) = ot.lp_loss_and_grad_wrt_output(lp_out, lpl, size, step, spec['LP_r_max'], spec['LP_slice_point'], scale)
    lib = tr.lib
    st = torch.cuda.current_stream().cuda_stream
    labels = torch.from_numpy(lpl).to(cuda)
    rec = torch.empty((B, 1, 8 + 3), device=cuda)
    assert lib.yolo_assign_targets_lp(labels.data_ptr(), rec.data_ptr(), B, 1, 10, 3, size[0], size[1], step, 45.0, 60.0, 45.0, st) == 0
    r = rec.cpu().numpy()
    for b in range(B):
        if lpl[b, 0, 0] < 0:
            assert r[b, 0, 0] == 0
            continue
        (hf, wf), p = ot.find_best_LP(lpl[b, 0], size, step, spec['LP_r_max'])
        assert r[b, 0, 0] == 1 and int(r[b, 0, 1]) == hf * fw + wf               # bit-exact cell
        np.testing.assert_allclose(r[b, 0, 2:8], p, rtol=1e-5, atol=1e-6)
        assert r[b, 0, 8:].tolist() == [1.0 if c == int(lpl[b, 0, -1]) else 0.0 for c in range(3)]
    assert int(r[0, 0, 1]) == 0 * fw + (fw - 1)                                    # clipped to row 0, last column
    logits = torch.from_numpy(lp_out.reshape(B, fh * fw, 10)).to(cuda).contiguous()
    dl = torch.empty_like(logits); ls = torch.empty((5, B), device=cuda)
    s5 = (C.c_float * 5)(0.1, 10.0, 1.0, 0.1, 0.3)
    assert lib.yolo_loss_lp_fwd_bwd(logits.data_ptr(), rec.data_ptr(), dl.data_ptr(), ls.data_ptr(), B, fh * fw, 10, 1, s5, 1.0, 0.1, st) == 0
    np.testing.assert_allclose(ls.cpu().numpy(), np.stack(rl), rtol=1e-4, atol=1e-8)
    _close(dl.cpu().numpy().reshape(gout.shape), gout, 1e-4, 'd lp logits')


def test_carlpnet_train_step(cuda):
    spec, size, g, P, x, lab, lpl, net, tr = _lp_setup(cuda)
    xt, lt, lpt = torch.from_numpy(x).to(cuda), torch.from_numpy(lab).to(cuda), torch.from_numpy(lpl).to(cuda)
    losses = tr.train_step(xt, lt, lp_labels=lpt, update=False)
    rl, rg, rmerged, rlp = ot.train_step_reference_lp(g, P, x, lab, lpl, spec, size)
    assert losses.shape == (10, x.shape[0])
    np.testing.assert_allclose(losses.cpu().numpy(), np.stack(rl), rtol=2e-3, atol=1e-7)
    grads = tr.grads()
    assert set(grads) == set(rg)
    rel = {}
    for name in sorted(rg):
        a, b = grads[name].cpu().numpy().astype(np.float64), rg[name].astype(np.float64)
        rel[name] = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
    # The LP path of this randomly initialised net is chaotic in train mode (30 more layers, BatchNorm statistics over
    # 384 samples): perturbing the ORACLE's input by 1e-6 relative moves its own LP output by 2e-3 and its gradients
    # by 3 % (median).  So: parameters whose gradient does not pass through the chaotic part must match tightly --
    # the LP output conv and last tip (fed by the strictly tested LP loss kernel), and the finest car head (car
    # gradient only) -- and everything else must agree in direction.
    worst = max(rel, key=rel.get)
    assert rel[worst] < 0.3, (worst, rel[worst])
    tight = [n for n in rel if n.startswith(('lp.out.', 'lp.4.tip.weight', 'heads.2.'))]
    assert len(tight) >= 20 and max(rel[n] for n in tight) < 2e-3, max((rel[n], n) for n in tight)
    lp_names = [n for n in rel if n.startswith('lp.')]
    assert len(lp_names) == 30 * 3 + 2
    for name in rg:
        a, b = grads[name].cpu().numpy().astype(np.float64).ravel(), rg[name].astype(np.float64).ravel()
        assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30) > 0.95, name
    with pytest.raises(ValueError):
        tr.train_step(xt, lt, update=False)                                        # LP labels are required
    first = float(tr.train_step(xt, lt, lp_labels=lpt).sum())
    for _ in range(30):
        last = float(tr.train_step(xt, lt, lp_labels=lpt).sum())
    assert last < 0.7 * first, (first, last)


def test_two_stream_step_every_bn_backward_consistent(cuda):
    """The weight gradients run on a side stream beside the BatchNorm backward and the data gradients.  Every dy the
    BatchNorm backward stored is re-derived on the GPU from exactly what the kernel read (the captured dz, the saved raw
    output and statistics): built with packed fp32 operations (v_pk_mul_f32 / v_pk_add_f32) the apply pass stored wrong
    values -- the low element of a pair in lanes 48-63, exact zeros mostly, 1-3 times per step at batch 4 -- whenever MFMA
    kernels of the other stream shared its CUs (csrc/Makefile: -packed-fp32-ops).  D53 spec, 416x416, six steps."""
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    from yolo_amd.spec import darknet53_spec, LEAKY_SLOPE
    net = CarNet(darknet53_spec(), dtype='bf16', device=cuda).initialize(seed=1234)
    tr = Trainer(net, (416, 416))
    B = 4
    x = torch.rand((B, 3, 416, 416), generator=torch.Generator().manual_seed(1)).to(cuda)
    lab = -torch.ones((B, 1, 30)); lab[:, 0, 0] = 3.0; lab[:, 0, 1:5] = torch.tensor([.5, .5, .4, .3]); lab[:, 0, 5] = 0.1
    lab[:, 0, 6:] = 1.0 / 24
    lab = lab.to(cuda)
    bad = []
    for it in range(6):
        cap = {}
        tr.train_step(x, lab, update=False, capture=cap)
        torch.cuda.synchronize()
        for op in tr._last[0].fwd:
            if op['kind'] != 'conv_bn':
                continue
            c = op['c']
            dz, dy, y = cap[c.name]['dz'].float(), cap[c.name]['dy'].float(), op['yraw'].val.float()
            g, b = net.params[c.name + '.gamma'].float(), net.params[c.name + '.beta'].float()
            xh = (y - op['mean']) * op['invstd']
            a = g * xh + b
            da = dz * torch.where(a > 0, 1.0, LEAKY_SLOPE)
            n = y.shape[0] * y.shape[1] * y.shape[2]
            k1 = (da.double().sum(dim=(0, 1, 2)) / n).float()
            k2 = ((da * xh).double().sum(dim=(0, 1, 2)) / n).float()
            ref = g * op['invstd'] * (da - k1 - xh * k2)
            off = ((dy - ref).abs() > 0.02 * ref.abs().max()) & (a.abs() > 1e-3)
            if bool(off.any()):
                bad.append((it, c.name, int(off.sum()), int((dy[off] == 0).sum())))
    assert not bad, bad


@pytest.fixture(scope='module')
def tuned(cuda):
    """One tune='measure' bf16 net + Trainer of the micro spec, shared by the cases below and released with the module: the choices
    of its inference plan and of one training step, its launch list, inference logits and training losses under them."""
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    spec, size = og.spec_micro(), (64, 96)
    P = og.init_params(og.build_graph(spec), seed=0, bn='random')
    x = torch.from_numpy(np.random.default_rng(2).random((2, 3) + size, dtype=np.float32)).to(cuda)
    lab = torch.from_numpy(ot.synthetic_labels(2, seed=1, render_rate=0.0, num_class=4)).to(cuda)
    net = CarNet(spec, dtype='bf16', device=cuda, tune='measure').load_params(P)
    tr = Trainer(net, size)
    net(x)                                                # (the inference plan's shapes are measured before the state is taken)
    state = tr.tune(x, lab)
    logits = [o.clone() for o in net(x)]
    losses = tr.train_step(x, lab, update=False).clone()
    return dict(spec=spec, size=size, P=P, x=x, lab=lab, state=state, logits=logits, losses=losses,
                signature=net.plan_signature(2, *size), train_logits=tr.merged_logits().clone())


@pytest.mark.parametrize('mode', ['measure', 'plan'])
def test_tuning_state_pins_a_fresh_net_and_trainer(cuda, tmp_path, tuned, mode):
    """The choices one net + Trainer measured, handed to a fresh pair -- tune='measure' + load_tuning_state, or tune='plan' on a
    plan file written from them --: nothing is measured again, nothing is stale, the same launch list, bit-identical inference
    logits, training-mode logits and losses."""
    from yolo_amd.net import CarNet
    from yolo_amd.train import Trainer
    from yolo_amd import plans
    t = tuned
    state = t['state']
    assert all(state[s] for s in plans.SECTIONS)
    if mode == 'plan':
        path = str(tmp_path / 'plan.json')
        plans.save(path, state)
        fresh = CarNet(t['spec'], dtype='bf16', device=cuda, tune='plan', tune_cache=path).load_params(t['P'])
        ftr = Trainer(fresh, t['size'])
        assert fresh.plan_meta['md5'] == plans.md5(state)
    else:
        fresh = CarNet(t['spec'], dtype='bf16', device=cuda, tune='measure').load_params(t['P'])
        ftr = Trainer(fresh, t['size'])
        assert ftr.tuning_state() == {s: {} for s in plans.SECTIONS}
        ftr.load_tuning_state(state)
    assert fresh.tune == mode
    logits = [o.clone() for o in fresh(t['x'])]
    losses = ftr.train_step(t['x'], t['lab'], update=False)
    torch.cuda.synchronize()
    assert plans.new_keys(ftr.tuning_state(), state) == 0 and plans.new_keys(fresh.tuning_state(), state) == 0
    assert fresh.stale_choices == 0
    assert fresh.plan_signature(2, *t['size']) == t['signature']
    assert all(torch.equal(a, b) for a, b in zip(logits, t['logits']))
    assert torch.equal(ftr.merged_logits(), t['train_logits'])
    assert torch.equal(losses, t['losses'])
