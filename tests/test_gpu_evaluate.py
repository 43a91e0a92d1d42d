"""GPU checks of the evaluation (csrc/eval.hip through the C ABI and yolo_amd.evaluate.Evaluator) against tests/eval_ref.py:
matching on fuzzed inputs (indices exact, IoUs bit-equal), a self-labelling known answer (AP = 1), the top-1 IoU / azimuth
against the oracle and the reference's own azimuth vectors, and the whole path on the micro net."""
import os

import numpy as np
import pytest
import torch

import eval_ref as er
from oracle import graph as og, forward as of, detect as od

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _ltrb_of(lab):
    y, x, h, w = lab[..., 1], lab[..., 2], lab[..., 3], lab[..., 4]
    return np.stack([x - w / f32(2), y - h / f32(2), x + w / f32(2), y + h / f32(2)], axis=-1).astype(f32)


def _fuzz(seed, nobj, mode, B=6, nbox=160, ncls=4, post_nms=48):
    """Rows, kept ids and labels with: detections that duplicate one ground truth (exactly and jittered), identical ground
    truths (the tie rule), cls < 0 rows, an image with kept_count 0 (1), an image without labels (2), a NaN box (3),
    out-of-range ids (4)."""
    rng = np.random.default_rng(seed)
    C, cpb = 6 + ncls, (ncls if mode == 'class' else 1)
    labels = -np.ones((B, nobj, 6 + ncls), f32)
    rows = rng.standard_normal((B, nbox, C)).astype(f32)
    cyx, hw = rng.uniform(.1, .9, (B, nbox, 2)), rng.uniform(.05, .4, (B, nbox, 2))
    rows[..., 1] = cyx[..., 1] - hw[..., 1] / 2; rows[..., 2] = cyx[..., 0] - hw[..., 0] / 2
    rows[..., 3] = cyx[..., 1] + hw[..., 1] / 2; rows[..., 4] = cyx[..., 0] + hw[..., 0] / 2
    kept = -np.ones((B, post_nms), np.int32)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        nvalid = int(rng.integers(1, min(nobj, 12) + 1))
        where = rng.choice(nobj, nvalid, replace=False)
        for g in where:
            labels[b, g, 0] = rng.integers(0, ncls)
            labels[b, g, 1:3] = rng.uniform(.2, .8, 2)
            labels[b, g, 3:5] = rng.uniform(.05, .4, 2)
            labels[b, g, 5:] = rng.random(1 + ncls)
        if nobj >= 2:                                         # two identical ground truths: the lower index is chosen
            src = int(where[0])
            dst = (src + 1) % nobj
            labels[b, dst] = labels[b, src]
            where = np.unique(np.append(where, dst))
        ids = []
        n = int(rng.integers(8, post_nms - 4))
        for k in range(n):
            box = int(rng.integers(0, nbox))
            cls = int(rng.integers(0, ncls))
            kind = rng.integers(0, 4)
            if kind:                                          # near a ground truth: exact copy (IoU 1, ties) or jittered
                g = int(rng.choice(where))
                jit = 0.0 if kind == 1 else (0.02 if kind == 2 else 0.12)
                rows[b, box, 1:5] = _ltrb_of(labels[b, g]) + (jit * rng.uniform(-1, 1, 4)).astype(f32)
                cls = int(labels[b, g, 0])
            ids.append(box * cpb + (cls if mode == 'class' else 0))
        kept[b, :n] = ids
        cnt[b] = n
    cnt[1] = 0                                                # its ids stay in place: nothing at or beyond the count is read
    labels[2, :, 0] = -1
    rows[3, kept[3, 0] // cpb, 2] = np.nan
    kept[4, 2] = nbox * cpb + 3
    kept[4, 5] = -7
    kept[4, 7] = 0x7fffffff
    return rows, kept, cnt, labels, cpb


@pytest.mark.parametrize('mode', ['class', 'obj'])
@pytest.mark.parametrize('nobj', [1, 7, 512])
def test_match_equals_the_restatement_on_fuzzed_inputs(cuda, lib, mode, nobj):
    rows, kept, cnt, labels, cpb = _fuzz(100 + nobj, nobj, mode)
    B, nbox, C = rows.shape
    post_nms = kept.shape[1]
    d = lambda a: torch.from_numpy(a).to(cuda)
    drows, dkept, dcnt, dlab = d(rows), d(kept), d(cnt), d(labels)
    oi = [torch.full((B, post_nms), -99, dtype=torch.int32, device=cuda) for _ in range(3)]
    oiou = torch.full((B, post_nms), -99., dtype=torch.float32, device=cuda)
    ogt = torch.full((B, nobj), -99, dtype=torch.int32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    import ctypes as C_
    rc = lib.yolo_eval_match(drows.data_ptr(), dkept.data_ptr(), dcnt.data_ptr(), dlab.data_ptr(), B, nbox, C, cpb, post_nms, nobj,
                             labels.shape[2], 1 if mode == 'class' else 0, C_.c_float(0.5), oi[0].data_ptr(), oi[1].data_ptr(),
                             oi[2].data_ptr(), oiou.data_ptr(), ogt.data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in oi] + [oiou.cpu().numpy(), ogt.cpu().numpy()]
    ntp = ndup = 0
    for b in range(B):
        want = er.match_image(rows[b], kept[b], cnt[b], cpb, labels[b], mode == 'class', 0.5)
        for name, g, w in zip(('det_class', 'det_tp', 'det_gt'), got[:3], want[:3]):
            assert np.array_equal(g[b], w), (name, b, g[b], w)
        assert np.array_equal(got[3][b].view(np.uint32), want[3].view(np.uint32)), (b, got[3][b], want[3])     # bit-equal IoUs
        assert np.array_equal(got[4][b], want[4]), b
        ntp += int(np.sum(want[1] == 1))
        ndup += int(np.sum((want[1] == 0) & (want[3] > 0.5)))
    assert (got[0][1] == -1).all() and (got[1][1] == -1).all() and (got[3][1] == 0).all()      # kept_count 0: pads only
    assert (got[4][2] == -1).all() and not (got[1][2] == 1).any()                               # no labels: no TP
    assert got[0][4, 2] == -1 and got[0][4, 5] == -1 and got[0][4, 7] == -1                     # out-of-range ids are pads
    assert got[3][3, 0] == 0 and got[1][3, 0] == 0                                              # the NaN box matches nothing
    assert ntp > 0 and ndup > 0, 'the fuzz holds no true positive / no duplicate detection of a claimed ground truth'


def test_match_rejects_more_than_512_labels(cuda, lib):
    import ctypes as C_
    p = torch.zeros(1 << 16, device=cuda).data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.yolo_eval_match(p, p, p, p, 1, 100, 10, 4, 48, 513, 10, 1, C_.c_float(0.5), p, p, p, p, p, st) == -2
    assert lib.yolo_eval_match(p, p, p, p, 1, 100, 10, 4, 1025, 4, 10, 1, C_.c_float(0.5), p, p, p, p, p, st) == -2
    assert lib.yolo_eval_match(p, p, p, p, 1, 100, 10, 4, 48, 4, 10, 1, C_.c_float(0.5), p, p, p, p, None, st) == -1


@pytest.mark.parametrize('mode', ['class', 'obj'])
def test_self_labelling_known_answer(cuda, mode):
    """Every detection the NMS keeps becomes a label (ltrb -> yxhw, class from the candidate id): every detection is a true
    positive matched to its own label, AP = mAP = 1 exactly, recall reaches 1."""
    from yolo_amd.detect import Detector
    from yolo_amd.evaluate import Evaluator
    spec = og.spec_d53()
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    det = Detector(spec, (416, 416), steps, device=cuda)
    rng = np.random.default_rng(5)
    B, nbox, C, post_nms = 4, 300, 30, 100
    rows = rng.standard_normal((B, nbox, C)).astype(f32)
    rows[..., 0] = rng.uniform(0.05, 1, (B, nbox))
    cyx, hw = rng.uniform(.1, .9, (B, nbox, 2)), rng.uniform(.05, .5, (B, nbox, 2))
    rows[..., 1] = cyx[..., 1] - hw[..., 1] / 2; rows[..., 2] = cyx[..., 0] - hw[..., 0] / 2
    rows[..., 3] = cyx[..., 1] + hw[..., 1] / 2; rows[..., 4] = cyx[..., 0] + hw[..., 0] / 2
    drows = torch.from_numpy(rows).to(cuda)
    kept, ks, cnt = det.nms(drows, mode, post_nms=post_nms)
    kh, ch = kept.cpu().numpy(), cnt.cpu().numpy()
    cpb = 24 if mode == 'class' else 1
    labels = -np.ones((B, post_nms, 30), f32)
    for b in range(B):
        assert ch[b] > 10
        for d in range(int(ch[b])):
            l, t, r, bt = rows[b, kh[b, d] // cpb, 1:5]
            labels[b, d, :5] = [kh[b, d] % cpb, (t + bt) / f32(2), (l + r) / f32(2), bt - t, r - l]
    ev = Evaluator(det, mode=mode, post_nms=post_nms, max_images=8)
    ev.update_detections(drows, kept, ks, cnt, labels)
    g = ev.logs()
    for b in range(B):
        n = int(ch[b])
        assert (g['det_tp'][b, :n] == 1).all() and (g['det_tp'][b, n:] == -1).all()
        assert np.array_equal(g['det_gt'][b, :n], np.arange(n))
        assert (g['det_iou'][b, :n] > 0.9999).all()
    r = ev.result()
    with_gt = r['n_gt'] > 0
    assert with_gt.any() and (r['ap'][with_gt] == 1.0).all() and r['mAP'] == 1.0
    assert int(r['n_gt'].sum()) == int(r['n_det'].sum()) == int(ch.sum())
    for c in np.nonzero(with_gt)[0]:
        assert r['pr'][c]['recall'][-1] == 1.0 and (r['pr'][c]['precision'] == 1.0).all()
    assert r['images'] == B and np.isnan(r['mean_iou'])             # (matching only: no top-1 figures)


def _dirs(ncls):
    az = np.radians(np.arange(ncls) * 360.0 / ncls)
    return np.stack([np.cos(az), np.sin(az)], axis=1).astype(f32)


def test_top1_iou_and_valid_against_the_oracle(cuda, lib):
    from yolo_amd.detect import Detector
    spec, size, B = og.spec_d53(), (416, 416), 6
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    area = od.init_area(size, steps)
    rng = np.random.default_rng(17)
    outs = [rng.standard_normal((B, a, 3, 30)).astype(f32) for a in area]
    syxhw = od.init_syxhw(size, steps, spec['all_anchors'])
    det = Detector(spec, size, steps, device=cuda)
    pred, _ = det.predict_device([torch.from_numpy(o).to(cuda) for o in outs])
    rpred, _ = od.predict(outs, spec['slice_point'], size, syxhw)
    labels = -np.ones((B, 2, 30), f32)
    for b in range(B):
        labels[b, 0, :5] = [b % 24, rpred[b, 1] + rng.uniform(-.05, .05), rpred[b, 2] + rng.uniform(-.05, .05),
                            rpred[b, 3] * rng.uniform(.7, 1.3), rpred[b, 4] * rng.uniform(.7, 1.3)]
        labels[b, 1, :5] = [3, .5, .5, .9, .9]               # object 1 is never read
    labels[2, 0, 0] = -1                                      # an image without an object: invalid, still evaluated
    labels[4, 0, :5] = [1, .9, .9, .01, .01]                  # a small box in a corner
    out = torch.full((B, 4), -99., dtype=torch.float32, device=cuda)
    dl, dd = torch.from_numpy(labels).to(cuda), torch.from_numpy(_dirs(24)).to(cuda)
    assert lib.yolo_eval_top1(pred.data_ptr(), dl.data_ptr(), dd.data_ptr(), out.data_ptr(), B, 30, 2, 30,
                              torch.cuda.current_stream().cuda_stream) == 0
    got = out.cpu().numpy()
    want = np.zeros(B, f32)
    for b in range(B):
        p = rpred[b]
        box = np.asarray([p[2] - p[4] / f32(2), p[1] - p[3] / f32(2), p[2] + p[4] / f32(2), p[1] + p[3] / f32(2)], f32)
        want[b] = od.get_iou(box, labels[b, 0, :5], mode=2)[0]
    print('top-1 IoU', got[:, 0], want)
    np.testing.assert_allclose(got[:, 0], want, rtol=1e-5, atol=1e-6)
    assert got[:, 3].tolist() == [1, 1, 0, 1, 1, 1]
    for b in range(B):                                        # azimuth / radius against the restatement
        _, az, rad, _ = er.top1_image(rpred[b], labels[b, 0], _dirs(24))
        e = abs(az - float(got[b, 1]))
        assert abs(rad - got[b, 2]) < 1e-5 and (min(e, abs(e - 2 * np.pi)) < 1e-4 or rad < 1e-3)


def test_top1_azimuth_against_the_reference_vectors(cuda, lib):
    """RadarProb.cls2ang run from the reference (tests/golden/reference_vectors.npz: azi_logits -> azi_angle): the device
    azimuth, modulo 2 pi, within 2e-6 rad -- the bar tests/test_reference_vectors.py holds the host code to.  Row 0 has
    all-zero logits: radius 0, the angle is undefined, and it is the only row left out."""
    G = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_vectors.npz'))
    logits, angle = G['azi_logits'].astype(f32), G['azi_angle']
    n = logits.shape[0]
    assert n == 16
    pred = np.zeros((n, 30), f32)
    pred[:, 0] = 1.0
    pred[:, 1:5] = [.5, .5, .2, .2]
    pred[:, 6:] = logits
    labels = np.zeros((n, 1, 30), f32)
    labels[:, 0, 1:5] = [.5, .5, .2, .2]
    out = torch.full((n, 4), -99., dtype=torch.float32, device=cuda)
    dp, dl, dd = torch.from_numpy(pred).to(cuda), torch.from_numpy(labels).to(cuda), torch.from_numpy(_dirs(24)).to(cuda)
    assert lib.yolo_eval_top1(dp.data_ptr(), dl.data_ptr(), dd.data_ptr(), out.data_ptr(), n, 30, 1, 30,
                              torch.cuda.current_stream().cuda_stream) == 0
    got = out.cpu().numpy()
    left_out = [k for k in range(n) if not np.any(logits[k] != logits[k, 0])]          # uniform classes: no direction
    assert left_out == [0]
    assert got[0, 2] < 1e-6
    for k in range(1, n):
        e = abs(float(got[k, 1]) - float(angle[k]))
        print('azimuth row %d: device %.9f reference %.9f' % (k, got[k, 1], angle[k]))
        assert min(e, abs(e - 2 * np.pi)) < 2e-6, (k, got[k, 1], angle[k])
    assert (got[:, 3] == 1).all() and np.allclose(got[:, 0], 1.0, atol=1e-6)


def test_evaluator_end_to_end_on_the_micro_net(cuda):
    """Two update() calls of different batch sizes on the f32 micro net, then result(), against tests/eval_ref.py applied to the
    oracle-side pipeline (torch-CPU forward, the oracle's decode, NMS and predict), as tests/test_gpu_boxes.py builds it."""
    from yolo_amd.net import CarNet
    from yolo_amd.detect import Detector
    from yolo_amd.evaluate import Evaluator
    from yolo_amd import lib as L
    spec, size, B, post_nms, nobj = og.spec_micro(), (64, 96), 5, 40, 6
    ncls = spec['slice_point'][-1] - 6
    g = og.build_graph(spec)
    P = og.init_params(g, seed=0, bn='random')
    x = np.random.default_rng(2).random((B, 3) + size, dtype=np.float32)
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    syxhw = od.init_syxhw(size, steps, spec['all_anchors'])
    ref = [r.numpy() for r in of.forward_torch(g, P, x)]
    ref_rows = od.decode_all(ref, spec['slice_point'], size, syxhw)
    ref_pred, _ = od.predict(ref, spec['slice_point'], size, syxhw)
    rk = [od.nms(ref_rows[i], mode='class', post_nms=post_nms) for i in range(B)]
    # labels from the oracle's own detections: object 0 near the top-1 box with its most likely class, three near kept
    # detections of their class, one random box, one empty row; image 3 has no object at all
    rng = np.random.default_rng(9)
    labels = -np.ones((B, nobj, 6 + ncls), f32)
    for i in range(B):
        p = ref_pred[i]
        labels[i, 0, :5] = [int(np.argmax(p[6:])), p[1] + rng.uniform(-.02, .02), p[2] + rng.uniform(-.02, .02),
                            p[3] * rng.uniform(.85, 1.15), p[4] * rng.uniform(.85, 1.15)]
        ids = rk[i][0]
        for j, d in enumerate(ids[[0, len(ids) // 3, len(ids) // 2]]):
            l, t, r, b = ref_rows[i, d // ncls, 1:5]
            labels[i, 1 + j, :5] = [d % ncls, (t + b) / 2 + rng.uniform(-.02, .02), (l + r) / 2 + rng.uniform(-.02, .02),
                                    (b - t) * rng.uniform(.8, 1.2), (r - l) * rng.uniform(.8, 1.2)]
        labels[i, 4, :5] = [rng.integers(0, ncls), rng.uniform(.3, .7), rng.uniform(.3, .7), rng.uniform(.1, .4), rng.uniform(.1, .4)]
    labels[3, :, 0] = -1
    az = np.arange(ncls) * 360.0 / ncls
    dirs = _dirs(ncls)
    exp = {k: [] for k in ('det_class', 'det_tp', 'det_score', 'gt_class', 'top1', 'az')}
    for i in range(B):
        ids, sc = rk[i]
        kept = -np.ones(post_nms, np.int32)
        kept[:len(ids)] = ids
        score = np.zeros(post_nms, f32)
        score[:len(ids)] = sc
        dc, tp, _, _, gc = er.match_image(ref_rows[i], kept, len(ids), ncls, labels[i], True, 0.5)
        exp['det_class'].append(dc); exp['det_tp'].append(tp); exp['det_score'].append(score); exp['gt_class'].append(gc)
        exp['top1'].append(er.top1_image(ref_pred[i], labels[i, 0], dirs))
        exp['az'].append(az[int(labels[i, 0, 0])] if labels[i, 0, 0] >= 0 else 0.0)
    want = er.summarise(exp['det_class'], exp['det_tp'], exp['det_score'], exp['gt_class'], exp['top1'], exp['az'], ncls)

    net = CarNet(spec, dtype='f32', device=cuda).load_params(P)
    det = Detector(spec, size, steps, device=cuda)
    ev = Evaluator(det, mode='class', post_nms=post_nms, max_images=B)
    xd = torch.from_numpy(x).to(cuda)
    ev.update(net(xd[:3]), labels[:3])                                        # numpy labels
    ev.update(net(xd[3:]), torch.from_numpy(labels[3:]).to(cuda))             # device labels
    got = ev.result()
    logs = ev.logs()
    print('end to end: got', {k: got[k] for k in ('images', 'mean_iou', 'azimuth_rmse_deg', 'azimuth_images', 'mAP', 'ap', 'n_gt', 'n_det')})
    print('end to end: want', want)
    assert got['images'] == want['images'] == B
    assert got['n_gt'].tolist() == want['n_gt'] and got['n_det'].tolist() == want['n_det']
    assert np.array_equal(logs['det_tp'], np.stack(exp['det_tp']))            # slot by slot: the two pipelines rank alike
    assert np.array_equal(logs['det_class'], np.stack(exp['det_class']))
    assert np.array_equal(logs['gt_class'], np.stack(exp['gt_class']))
    assert sum(want['n_det']) > 20 and 0 < int(np.sum(np.stack(exp['det_tp']) == 1)) < sum(want['n_det'])
    assert abs(got['mAP'] - want['mAP']) <= 1e-6 and abs(got['mean_iou'] - want['mean_iou']) <= 1e-6
    np.testing.assert_allclose(got['ap'], want['ap'], rtol=0, atol=1e-6, equal_nan=True)
    assert got['azimuth_images'] == want['azimuth_images'] and want['azimuth_images'] >= 2
    assert abs(got['azimuth_rmse_deg'] - want['azimuth_rmse_deg']) < 1e-2
    assert logs['top1'][:, 3].tolist() == [1, 1, 1, 0, 1]
    # a full log refuses another batch; reset() returns to empty
    with pytest.raises(L.YoloError):
        ev.update(net(xd[:1]), labels[:1])
    assert ev.result()['images'] == B
    ev.reset()
    r0 = ev.result()
    assert r0['images'] == 0 and int(r0['n_det'].sum()) == 0 and int(r0['n_gt'].sum()) == 0 and np.isnan(r0['mAP'])
    ev.update(net(xd[:2]), labels[:2, :3])                                    # (another number of labels per image after a reset)
    assert ev.result()['images'] == 2
