"""The overlay's text and the published row on the device against tests/overlay_text_ref.py: yolo_overlay_text bit for bit from
hand-made label tables, yolo_overlay_labels in exact integer equality, yolo_pose_top1 (azimuth and radius bit-equal to
yolo_eval_top1's, the azimuth against the reference's own vectors, class and depth exact), and FrameOverlay(labels=True) end to end."""
import math
import os

import numpy as np
import pytest
import torch

import overlay_ref as R
import overlay_text_ref as T
from yolo_amd import lib as L
from yolo_amd.overlay import BitmapFont, FrameOverlay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SENTINEL = 0xA5
# csrc/overlay.hip: a block of yolo_overlay_text owns OV_TEXT_TILE_W x OV_TEXT_TILE_H pixels, counted from the top-left corner of its
# label's paint rectangle clipped to the frame
OV_TEXT_TILE_W, OV_TEXT_TILE_H = 256, 16
FONT = T.synthetic_font(4)                              # 12 glyphs of 5 x 7 for the bytes 'A'..'L': 'A' all ink, 'B' empty
FIRST, CELL_W, ADVANCE = 65, 5, 6


def _text(lib, dev, frames, labels, scale, pad, offset=0, font=FONT, cell_w=CELL_W, advance=ADVANCE, first=FIRST):
    """frames (N,H,W,C) uint8 ndarray, labels (N,K,16) int32 -> the painted frames; the device frames start
    `offset` bytes into a larger buffer whose other bytes must come back untouched."""
    N, H, W, Cc = frames.shape
    guard = 64
    buf = torch.full((offset + frames.size + guard,), SENTINEL, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + frames.size].view(N, H, W, Cc)
    view.copy_(torch.from_numpy(frames).to(dev))
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    fnt = torch.from_numpy(np.ascontiguousarray(font).view(np.int32)).to(dev)
    rc = lib.yolo_overlay_text(L.ptr(view), L.ptr(lab), L.ptr(fnt), font.shape[0], first, cell_w, font.shape[1], advance, scale, pad,
                               N, H, W, Cc, labels.shape[1], L.stream_ptr())
    assert rc == L.OK
    host = buf.cpu().numpy()
    assert (host[:offset] == SENTINEL).all() and (host[offset + frames.size:] == SENTINEL).all()
    return host[offset:offset + frames.size].reshape(frames.shape)


def _frames(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _hand_made(scale):
    """the labels of the raster test for a 53 x 37 frame: (x, y, text, ink, ground, flags[, nchar])."""
    s = scale
    return [(-7, -3, 'ACDEF', (10, 20, 30, 40), (1, 2, 3, 4), 3),                      # leaves the left and the top edge
            (53 - 9 * s, 9, 'GHAIJ', (50, 60, 70, 80), (5, 6, 7, 8), 3),               # leaves the right edge
            (6, 37 - 4 * s, 'KLCA', (90, 100, 110, 120), (9, 10, 11, 12), 3),          # leaves the bottom edge
            (12, 14, 'AEGIK', (200, 201, 202, 203), (130, 131, 132, 133), 3),          # overlapping: with a ground ...
            (15, 14 + 3 * s, 'FAHJ', (210, 211, 212, 213), (0, 0, 0, 0), 1),           # ... and without, over it
            (17, 13, 'CAB', (220, 221, 222, 223), (140, 141, 142, 143), 3),            # ... and a third with a ground over both
            (20, 20, '', (1, 1, 1, 1), (2, 2, 2, 2), 3),                               # nchar 0: not even its ground
            (2, 2, 'AAAAA', (3, 3, 3, 3), (4, 4, 4, 4), 2),                            # disabled (bit 0 clear)
            (-30 * s, 26, 'ABCDEFGHIJKL' * 3 + 'ABCD', (230, 231, 232, 233), (150, 151, 152, 153), 3),     # nchar 40
            (30, 3, 'Az@A', (240, 241, 242, 243), (160, 161, 162, 163), 3),            # bytes outside the font ink nothing
            (200, 200, 'AAAA', (5, 5, 5, 5), (6, 6, 6, 6), 3),                         # wholly outside the frame ...
            (-900, -300, 'AAAA', (5, 5, 5, 5), (6, 6, 6, 6), 3),                       # ... on the other side
            (4, 4, 'A' * 40, (7, 7, 7, 7), (8, 8, 8, 8), 3, 41)]                       # nchar 41: disabled, nothing written


@pytest.mark.parametrize('scale', [1, 3])
@pytest.mark.parametrize('Cc', [1, 3, 4])
def test_text_equals_the_restatement(lib, cuda, Cc, scale):
    frames = _frames(1, (2, 37, 53, Cc))
    table = T.as_int32([T.pack_label(*lab) for lab in _hand_made(scale)])
    labels = np.stack([table, table[::-1]])                                   # the painter's order both ways
    pad = 1
    want = T.draw_text(frames, labels, FONT, FIRST, CELL_W, ADVANCE, scale, pad)
    got = _text(lib, cuda, frames, labels, scale, pad, offset=3)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, frames) and not np.array_equal(want[0], want[1])
    # run twice: the same bytes
    assert np.array_equal(_text(lib, cuda, frames, labels, scale, pad, offset=1), got)
    # the empty, the disabled, the outside and the 41-character labels alone write nothing
    quiet = np.stack([table[[6, 7, 10, 11, 12]]] * 2)
    assert np.array_equal(_text(lib, cuda, frames, quiet, scale, pad, offset=1), frames)


def test_text_crosses_tile_borders_both_ways(lib, cuda):
    """600 x 70 px at scale 2: a 40-character label is (39 x 6 + 5) x 2 = 478 px wide and 14 + 2 x 3 = 20 px high with its ground: two
    tiles across and two down, the borders 256 px and 16 px from the rectangle's corner.  One label starts left of the frame (its
    tiles count from column 0), one lies over the corner where four tiles meet, without a ground."""
    frames = _frames(3, (1, 70, 600, 3))
    scale, pad = 2, 3
    long_text = 'ACDEFGHIJKLA' * 3 + 'CDEF'
    assert (len(long_text) - 1) * ADVANCE * scale + CELL_W * scale + 2 * pad > OV_TEXT_TILE_W and 7 * scale + 2 * pad > OV_TEXT_TILE_H
    labs = [(40, 10, long_text, (10, 20, 30), (1, 2, 3), 3), (-100, 40, long_text[::-1], (40, 50, 60), (4, 5, 6), 3),
            (40 - pad + OV_TEXT_TILE_W - 20, 10 - pad + OV_TEXT_TILE_H - 9, 'AEAK', (70, 80, 90), (0, 0, 0), 1),
            (100, 34, 'AAL', (100, 110, 120), (7, 8, 9), 3)]
    labels = T.as_int32([[T.pack_label(*lab) for lab in labs]])
    got = _text(lib, cuda, frames, labels, scale, pad, offset=1)
    assert np.array_equal(got, T.draw_text(frames, labels, FONT, FIRST, CELL_W, ADVANCE, scale, pad))
    # an advance wider than the cell, a pad of a tile's width: the ground box covers whole tiles
    got = _text(lib, cuda, frames, labels[:, :2], 1, 300, offset=2, advance=9)
    assert np.array_equal(got, T.draw_text(frames, labels[:, :2], FONT, FIRST, CELL_W, 9, 1, 300))


def test_no_enabled_label_leaves_the_buffer_alone(lib, cuda):
    frames = np.full((2, 37, 53, 3), SENTINEL, np.uint8)
    table = T.as_int32([T.pack_label(x, y, t, i, g, fl & ~1) for (x, y, t, i, g, fl, *_) in _hand_made(1)])
    assert np.array_equal(_text(lib, cuda, frames, np.stack([table, table]), 1, 1, offset=1), frames)


# ---- labels ----------------------------------------------------------------------------------------------------------------
H0, W0 = 120, 160
NAMES = ['', 'sixteen_bytes_xx', 'car']


def _label_cases():
    """rows, kept ids, scores, top-1 rows, poses and plates with the special values put in, and the reference's shape tables."""
    B, nbox, Cc, post = 4, 6, 9, 4
    rows, kept, count = R.nms_case(5, B, nbox, Cc, post)
    count[:] = [2, 4, 4, 3]                                                 # kept_count < post_nms
    kept[0] = [7, 2, 9, 9]                                                  # (ids beyond the count are never looked at)
    kept[1] = [0, -1, nbox * 3 + 1, 17]                                     # a pad and an id beyond nbox * cand_per_box inside the count
    kept[2] = [1, 5, 8, 15]
    kept[3] = [3, 6, 16, 0]
    rows[:, :, 0] = np.random.default_rng(1).uniform(0, 1, (B, nbox))
    rows[2, 0, 0], rows[2, 1, 0], rows[2, 2, 0] = np.nan, -0.5, 0.0625
    scores = np.random.default_rng(2).uniform(0, 1, (B, post)).astype(f32)
    scores[3, 0], scores[3, 1], scores[3, 2] = np.nextafter(f32(1), f32(2)), np.inf, 0.3125
    pred = R.top1_rows(3, B, Cc)
    pred[:, 0] = [np.nan, -0.25, 0.0625, np.nextafter(f32(1), f32(2))]
    pred[0, 1:5] = [0.08, 0.5, 0.14, 0.3]                                   # at the frame's top: the label moves inside
    pred[1, 1:5] = [0.5, 0.93, 0.3, 0.12]                                   # at its right edge: the label moves left
    pred[2, 1:5] = [0.5, 0.02, 0.3, 0.2]                                    # over its left edge: the label moves right
    pose = np.array([[-0.4, 0.5, -1, 2], [math.pi, 0.5, 3.5, 1], [np.nan, 0.1, 2, 0], [1.0, 0.9, 7, 3]], f32)      # class 3: beyond nname
    lp = R.plate_rows(7, B)
    lp[:, 1:4] = [[30, -20, 900], [-60, 25, 1200], [10, 10, 1500], [0, 0, 1000]]
    lp[1, 0] = 0.25                                                         # a disabled plate slot
    tabs = {cpb: R.shapes(B, H0, W0, nms=(rows, kept, count), cand_per_box=cpb, pred=pred, car_threshold=-1.0, lp=lp,
                          camera=R.CAMERA)['table'] for cpb in (3, 1)}
    for cpb in tabs:
        tabs[cpb][:, post, 10] = 1                                          # (a NaN score is not above any threshold: the text is wanted here)
    tabs[3][3, post, 10] = 0                                                # ... and a disabled top-1 slot
    return dict(B=B, nbox=nbox, C=Cc, post=post, rows=rows, kept=kept, count=count, scores=scores, pred=pred, pose=pose, lp=lp, tabs=tabs)


@pytest.fixture(scope='module')
def label_cases():
    return _label_cases()


def _labels(lib, dev, c, cpb, scores, pose, show_deg, names, m, ground):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    table, rows, kept, count, pred, lp = [t(c[k]) for k in ('t', 'rows', 'kept', 'count', 'pred', 'lp')]
    sc, po = t(scores), t(pose)
    nm = None
    if names:
        raw = np.zeros((len(names), 16), np.uint8)
        for k, s in enumerate(names):
            raw[k, :len(s)] = np.frombuffer(s.encode(), np.uint8)
        nm = t(raw)
    K = c['post'] + 2
    out = torch.full((c['B'], K, 16), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    rc = lib.yolo_overlay_labels(L.ptr(table), L.ptr(rows), L.ptr(kept), L.ptr(count), L.ptr(sc), c['nbox'], c['C'], c['post'], cpb,
                                 L.ptr(pred), c['C'], L.ptr(po), int(show_deg), L.ptr(lp), L.ptr(nm), len(names) if names else 0,
                                 m['cell_w'], m['cell_h'], m['advance'], m['scale'], m['gap'], m['pad'], 0 if ground is None else 1,
                                 0 if ground is None else R.pack_colour(ground), c['B'], H0, W0, K, L.ptr(out), L.stream_ptr())
    assert rc == L.OK
    return out.cpu().numpy()


M1 = dict(cell_w=6, cell_h=11, advance=6, scale=1, gap=4, pad=1)
M2 = dict(cell_w=5, cell_h=7, advance=7, scale=2, gap=0, pad=3)


@pytest.mark.parametrize('case', ['class_scores_pose', 'class_rows_nopose', 'obj_nodeg', 'class_two_names'])
def test_labels_equal_the_restatement(lib, cuda, label_cases, case):
    c = dict(label_cases)
    cpb, scores, pose, show_deg, names, m, ground = {
        'class_scores_pose': (3, c['scores'], c['pose'], True, NAMES, M1, (0, 0, 0)),
        'class_rows_nopose': (3, None, None, True, NAMES, M1, (9, 8, 7)),
        'obj_nodeg': (1, c['scores'], c['pose'], False, NAMES, M2, None),
        'class_two_names': (3, None, c['pose'], True, NAMES[:2], M2, (1, 2, 3))}[case]        # class 2: beyond nname
    c['t'] = c['tabs'][cpb]
    got = _labels(lib, cuda, c, cpb, scores, pose, show_deg, names, m, ground)
    want = T.labels(c['t'], W0, nms=(c['rows'], c['kept'], c['count']), kept_scores=scores, cand_per_box=cpb, pred=c['pred'], pose=pose,
                    show_deg=show_deg, lp=c['lp'], names=names, ground=ground, **m)
    texts = [[T.label_text(w).decode() for w in img] for img in want]
    print(case, texts)
    assert np.array_equal(got, want)
    post = c['post']
    # what the cases were made for, read off the restatement
    assert want[0, 2:post, 4].tolist() == [0, 0] and want[1, 1:3, 4].tolist() == [0, 0] and not want[1, 1].any()
    assert want[1, post + 1, 4] == 0                                                      # the plate below its threshold
    if case == 'class_scores_pose':
        assert want[3, post, 4] == 0                                                      # the disabled top-1 slot
        assert texts[0][post] == 'car -.--- -23' and texts[1][post] == 'sixteen_bytes_xx -.--- 180' and texts[2][post] == '0.062'
        assert texts[3][0] == '1.000' and texts[3][1] == '-.---' and texts[3][2] == 'sixteen_bytes_xx 0.312'      # ids 3, 6, 16: classes 0, 0, 1
        assert want[0, post, 1] == 1 + M1['gap']                                          # the box's top is row 1: moved under the top edge
        assert want[1, post, 0] == W0 - (len(texts[1][post]) * 6) - 1                     # moved left
        assert want[2, post, 0] == 1                                                      # moved right to pad
    if case == 'class_rows_nopose':
        assert texts[2][:3] == ['sixteen_bytes_xx -.---', 'car -.---', 'car 0.062'] and texts[2][post] == '0.062'
    if case == 'obj_nodeg':
        assert texts[0][post] == 'car -.---' and all(' ' not in t for t in texts[2][:post]) and (want[:, :, 4] != 3).all()
    if case == 'class_two_names':
        assert texts[0][post] == '-.--- -23' and texts[2][1] == '-.---' and texts[2][2] == '0.062'


# ---- the published row -----------------------------------------------------------------------------------------------------
def _dirs(ncls):
    az = np.radians(np.arange(ncls) * 360.0 / ncls)
    return np.stack([np.cos(az), np.sin(az)], axis=1).astype(f32)


def _pose(lib, dev, pred, depth, row5, in_place=False, ncls=None):
    B, Cc = pred.shape
    dp = torch.from_numpy(pred).to(dev)
    dd = torch.from_numpy(_dirs(Cc - 6)).to(dev)
    de = None if depth is None else torch.from_numpy(depth).to(dev)
    rows = dp if in_place else torch.full((B, Cc), -99., dtype=torch.float32, device=dev)
    pose = torch.full((B, 4), -99., dtype=torch.float32, device=dev)
    Hd, Wd = (0, 0) if depth is None else depth.shape[1:]
    assert lib.yolo_pose_top1(L.ptr(dp), B, Cc, L.ptr(dd), L.ptr(de), Hd, Wd, row5, L.ptr(rows), L.ptr(pose), L.stream_ptr()) == L.OK
    return pose.cpu().numpy(), rows.cpu().numpy()


def _pose_rows():
    """(B,30) rows: random logits, tied logits, NaN logits, and the centres the depth lookup is about."""
    g = np.random.default_rng(21)
    B = 70                                                                  # more than one block of 64 threads
    pred = g.uniform(0, 1, (B, 30)).astype(f32)
    pred[:, 6:] = g.standard_normal((B, 24)).astype(f32) * 3
    pred[1, 6:] = 0.5; pred[1, [9, 17]] = 2.0                               # two equal largest logits: the lower index
    pred[2, 6:] = np.nan; pred[2, 11] = -1.0                                # a NaN never wins
    pred[3, 6:] = np.nan                                                    # all NaN: class 0
    pred[4, 2] = 1.0                                                        # x = 1.0: index = Wd
    pred[5, 1] = 1.0
    pred[6, 2] = -0.5                                                       # a negative centre
    pred[7, 1] = np.nan
    pred[8, 2] = np.inf
    pred[9, 1:3] = [0.5, 0.5]                                               # ... where the depth image holds a NaN
    pred[10, 2] = -0.001                                                    # (int)(-0.032) = 0: inside
    return pred


def test_pose_equals_eval_top1_bit_for_bit_and_the_depth_lookup(lib, cuda):
    pred = _pose_rows()
    B = pred.shape[0]
    Hd, Wd = 24, 32
    depth = np.random.default_rng(22).uniform(0.3, 20.0, (B, Hd, Wd)).astype(f32)
    depth[9, 12, 16] = np.nan
    pose, rows = _pose(lib, cuda, pred, depth, 0)
    labels = np.zeros((B, 1, 30), f32)
    out = torch.full((B, 4), -99., dtype=torch.float32, device=cuda)
    dp, dl, dd = torch.from_numpy(pred).to(cuda), torch.from_numpy(labels).to(cuda), torch.from_numpy(_dirs(24)).to(cuda)
    assert lib.yolo_eval_top1(L.ptr(dp), L.ptr(dl), L.ptr(dd), L.ptr(out), B, 30, 1, 30, L.stream_ptr()) == L.OK
    ev = out.cpu().numpy()
    fin = [0, 1] + list(range(4, B))                                        # (rows 2 and 3 hold NaN logits: a NaN has no bits to compare)
    assert np.isfinite(ev[fin, 1:3]).all() and np.isnan(pose[2:4, :2]).all() and np.isnan(ev[2:4, 1:3]).all()
    assert np.array_equal(pose[fin, :2].view(np.uint32), ev[fin, 1:3].view(np.uint32))  # azimuth and radius: the same bits
    assert pose[:, 3].tolist() == [float(T.top_class(p[6:])) for p in pred] and pose[1:4, 3].tolist() == [3.0, 5.0, 0.0]
    want = np.array([T.depth_at(pred[b], depth[b]) for b in range(B)], f32)
    assert np.array_equal(pose[:, 2].view(np.uint32), want.view(np.uint32))             # exact, the NaN included
    assert want[4:9].tolist() == [-1, -1, -1, -1, -1] and np.isnan(want[9]) and want[10] == depth[10, int(Hd * pred[10, 1]), 0]
    assert (want[11:] > 0).all()
    assert np.array_equal(rows.view(np.uint32), pred.view(np.uint32))                   # row5 = 0: a copy
    # row5 = 1 / 2, into another tensor and in place; depth NULL
    for row5, col in ((1, 0), (2, 2)):
        for in_place in (False, True):
            p2, r2 = _pose(lib, cuda, pred, depth, row5, in_place=in_place)
            assert np.array_equal(p2.view(np.uint32), pose.view(np.uint32))
            keep = [j for j in range(30) if j != 5]
            assert np.array_equal(r2[:, keep].view(np.uint32), pred[:, keep].view(np.uint32))
            assert np.array_equal(r2[:, 5].view(np.uint32), pose[:, col].view(np.uint32))
    p3, r3 = _pose(lib, cuda, pred, None, 2)
    assert (p3[:, 2] == -1).all() and (r3[:, 5] == -1).all() and np.array_equal(p3[:, [0, 1, 3]].view(np.uint32), pose[:, [0, 1, 3]].view(np.uint32))


def test_pose_azimuth_against_the_reference_vectors(lib, cuda):
    """RadarProb.cls2ang run from the reference (tests/golden/reference_vectors.npz: azi_logits -> azi_angle): within 2e-6 rad modulo
    2 pi, the bar tests/test_gpu_evaluate.py holds yolo_eval_top1 to.  Row 0 (all-zero logits: no direction) is left out as there."""
    G = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_vectors.npz'))
    logits, angle = G['azi_logits'].astype(f32), G['azi_angle']
    n = logits.shape[0]
    pred = np.zeros((n, 30), f32)
    pred[:, 0] = 1.0
    pred[:, 1:5] = [.5, .5, .2, .2]
    pred[:, 6:] = logits
    pose, _ = _pose(lib, cuda, pred, None, 0)
    assert [k for k in range(n) if not np.any(logits[k] != logits[k, 0])] == [0] and pose[0, 1] < 1e-6
    for k in range(1, n):
        e = abs(float(pose[k, 0]) - float(angle[k]))
        print('azimuth row %d: device %.9f reference %.9f' % (k, pose[k, 0], angle[k]))
        assert min(e, abs(e - 2 * np.pi)) < 2e-6, (k, pose[k, 0], angle[k])


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_pose_device(cuda, lib):
    from oracle import graph as og, detect as od
    from yolo_amd.detect import Detector
    spec, size = og.spec_d53(), (416, 416)
    det = Detector(spec, size, od.init_steps(spec['layers'], spec['all_anchors']), device=cuda)
    pred_h = _pose_rows()[:12]
    depth_h = np.random.default_rng(23).uniform(0.3, 20.0, (12, 24, 32)).astype(f32)
    want, _ = _pose(lib, cuda, pred_h, depth_h, 0)
    pred, depth = torch.from_numpy(pred_h).to(cuda), torch.from_numpy(depth_h).to(cuda)
    pose, rows = det.pose_device(pred, depth=depth)
    assert np.array_equal(pose.cpu().numpy().view(np.uint32), want.view(np.uint32)) and torch.equal(rows.view(torch.int32), pred.view(torch.int32))
    assert rows is not pred
    pose2, rows2 = det.pose_device(pred, depth=depth, row5='depth')
    assert torch.equal(_bits(rows2[:, 5]), _bits(pose[:, 2]))
    pose3, rows3 = det.pose_device(pred, row5='azimuth', out=pred)
    assert rows3 is pred and torch.equal(_bits(pred[:, 5]), _bits(pose[:, 0])) and (pose3[:, 2] == -1).all()
    # the class azimuths given: the default's 15-degree steps turned by 90 degrees turn every azimuth by pi / 2
    pose4, _ = det.pose_device(torch.from_numpy(pred_h).to(cuda), class_azimuth_deg=[k * 15.0 + 90.0 for k in range(24)])
    d = (pose4[:, 0] - pose[:, 0]).cpu().numpy()[[0, 1] + list(range(4, 12))]
    assert np.abs(np.mod(d - math.pi / 2 + math.pi, 2 * math.pi) - math.pi).max() < 1e-5
    with pytest.raises(ValueError):
        det.pose_device(pred, row5='radius')
    with pytest.raises(ValueError):
        det.pose_device(pred, depth=depth[:3])


# ---- FrameOverlay ----------------------------------------------------------------------------------------------------------
class _Counting(object):
    """the library with every call recorded by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def test_frame_overlay_with_labels_end_to_end(cuda, lib):
    N, H, W = 2, 120, 160
    frames_h = _frames(8, (N, H, W, 3))
    pred, lp = R.top1_rows(11, N, 9), R.plate_rows(12, N)
    lp[:, 1:4] = [[30, -20, 900], [-60, 25, 1200]]
    pred[0, 1:5] = [0.1, 0.5, 0.18, 0.3]                                    # a box at the top: its label moves inside
    rows, kept, count = R.nms_case(13, N, 10, 9, 4)
    scores = np.random.default_rng(14).uniform(0, 1, (N, 4)).astype(f32)
    names = ['sedan', 'van', b'truck']
    t = lambda a: torch.from_numpy(a).to(cuda)
    pose_h, _ = _pose(lib, cuda, pred, None, 0)
    ov = FrameOverlay(camera=R.CAMERA, device=cuda, labels=True, names=names)
    ov._lib = _Counting(ov._lib)
    font = ov.font
    m = dict(cell_w=font.cell_w, cell_h=font.cell_h, advance=font.advance, scale=1, gap=4, pad=1)
    # pred + pose + lp
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=cuda)
    got, clipped, valid = ov(t(frames_h), pred=t(pred), lp=t(lp), pose=t(pose_h), out=out)
    assert ov._lib.calls == ['yolo_overlay_shapes', 'yolo_overlay_labels', 'yolo_warp_u8_to_nchw', 'yolo_overlay_draw', 'yolo_overlay_text']
    table, labels = ov.table.cpu().numpy(), ov.labels.cpu().numpy()
    assert labels.shape == (N, 2, 16) and (table[:, :, 10] == 1).all() and valid.cpu().tolist() == [1, 1]
    want_labels = T.labels(table, W, pred=pred, pose=pose_h, lp=lp, names=names, **m)
    assert np.array_equal(labels, want_labels)
    assert T.label_text(labels[0, 0]).decode().split(' ')[0] in ('sedan', 'van', 'truck') and labels[0, 0, 1] == table[0, 0, 1:8:2].min() + 4
    lined = R.draw(frames_h, table)
    want = T.draw_text(lined, labels, font.masks, 32, font.cell_w, font.advance, 1, 1)
    assert np.array_equal(got.cpu().numpy(), want) and not np.array_equal(want, lined)
    # the clipped plate was read before anything was drawn
    import intake_ref
    mats = ov.matrices.cpu().numpy()
    assert np.array_equal(clipped.cpu().numpy(), intake_ref.warp_u8(frames_h, mats.reshape(N, 3, 3), (160, 380), border=0))
    # nms, with and without the kept scores, in place; a second call with the size allocates nothing
    for sc in (scores, None):
        frames = t(frames_h)
        got, _, _ = ov(frames, nms=(t(rows), t(kept), t(count)), nms_scores=None if sc is None else t(sc))
        assert got is frames
        table, labels = ov.table.cpu().numpy(), ov.labels.cpu().numpy()
        assert np.array_equal(labels, T.labels(table, W, nms=(rows, kept, count), kept_scores=sc, cand_per_box=3, names=names, **m))
        want = T.draw_text(R.draw(frames_h, table), labels, font.masks, 32, font.cell_w, font.advance, 1, 1)
        assert np.array_equal(frames.cpu().numpy(), want) and (labels[:, :, 4] == 3).sum() == int(count.sum())
    args = (t(rows), t(kept), t(count))
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(cuda)['allocation.all.allocated']
    ov(frames, nms=args)
    assert torch.cuda.memory_stats(cuda)['allocation.all.allocated'] == before
    # a font of the caller's, enlarged, without a ground box
    ov2 = FrameOverlay(device=cuda, labels=True, font=BitmapFont(FONT, CELL_W, advance=ADVANCE, first_code=46), font_scale=2,
                       label_ground=None, label_gap=2, label_pad=0)
    frames = t(frames_h)
    ov2(frames, pred=t(pred))
    labels = ov2.labels.cpu().numpy()
    m2 = dict(cell_w=CELL_W, cell_h=7, advance=ADVANCE, scale=2, gap=2, pad=0)
    assert np.array_equal(labels, T.labels(ov2.table.cpu().numpy(), W, pred=pred, ground=None, **m2)) and (labels[:, 0, 4] == 1).all()
    want = T.draw_text(R.draw(frames_h, ov2.table.cpu().numpy()), labels, FONT, 46, CELL_W, ADVANCE, 2, 0)
    assert np.array_equal(frames.cpu().numpy(), want)
    with pytest.raises(ValueError):
        ov(t(frames_h), lp=t(lp), pose=t(pose_h))                           # pose without pred
    with pytest.raises(ValueError):
        FrameOverlay(device=cuda, labels=True, names=['a name of seventeen'])


def test_frame_overlay_defaults_are_unchanged(cuda):
    """labels=False (the default): the launches FrameOverlay made before it could write text, and the same bytes."""
    N, H, W = 2, 120, 160
    frames_h = _frames(9, (N, H, W, 3))
    pred, lp = R.top1_rows(11, N), R.plate_rows(12, N)
    lp[:, 1:4] = [[30, -20, 900], [-60, 25, 1200]]
    rows, kept, count = R.nms_case(13, N, 10, 8, 4)
    t = lambda a: torch.from_numpy(a).to(cuda)
    ov = FrameOverlay(camera=R.CAMERA, device=cuda)
    ov._lib = _Counting(ov._lib)
    frames = t(frames_h)
    ov(frames, pred=t(pred), lp=t(lp), nms=(t(rows), t(kept), t(count)))
    assert ov._lib.calls == ['yolo_overlay_shapes', 'yolo_warp_u8_to_nchw', 'yolo_overlay_draw'] and ov.labels is None
    assert np.array_equal(frames.cpu().numpy(), R.draw(frames_h, ov.table.cpu().numpy()))
    frames = t(frames_h)
    ov(frames, pred=t(pred))
    assert ov._lib.calls[3:] == ['yolo_overlay_shapes', 'yolo_overlay_draw']
    assert np.array_equal(frames.cpu().numpy(), R.draw(frames_h, ov.table.cpu().numpy()))
    with pytest.raises(ValueError):
        ov(frames, pred=t(pred), pose=torch.zeros((N, 4), device=cuda))     # pose is for the labels
    assert not hasattr(ov, 'font')
