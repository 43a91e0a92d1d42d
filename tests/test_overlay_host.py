"""CPU checks of the frame overlay: its C ABI entries (declared, bound, exported, revision still 5, bad arguments refused without a
GPU), the package's seams, and the numpy restatement (tests/overlay_ref.py) against independent formulations -- the rasteriser
against a float64 distance test, the box against cv2_add_bbox's formula, the plate against PlateCamera.corners and plate_matrix."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np

import overlay_ref as R
from yolo_amd import intake
from yolo_amd import lib as L
from yolo_amd import render

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = ('yolo_overlay_table_bytes', 'yolo_overlay_shapes', 'yolo_overlay_draw')


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_overlay_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    assert int(re.search(r'#define YOLO_OVERLAY_SLOT_WORDS (\d+)', h).group(1)) == R.SLOT_WORDS
    from yolo_amd import overlay
    assert overlay.SLOT_WORDS == R.SLOT_WORDS
    assert int(re.search(r'#define YOLO_OVERLAY_MAX_SLOTS (\d+)', h).group(1)) == overlay.MAX_SLOTS == 128
    for name, nargs in zip(NAMES, (2, 35, 8)):
        assert name in L.SIGNATURES
        proto = re.search(r'^(?:int|long long) %s\(([^)]*)\);' % name, h, flags=re.M).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs, name


def _shapes_args():
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    #       rows kept count nbox C  post cpb palette npal pred C  thr  use_r colour lp fx   fy   cx   cy   cw   ch   thr  colour lh   lw
    return [p,   p,   p,    10,  8, 3,   2,  p,      8,   p,   8, 0.5, 0,    255,   p, 4e2, 4e2, 3e2, 2e2, 640, 480, 0.5, 255,   160, 380,
            # B H   W   t  table K  vertices matrices lp_valid stream
            2,  32, 48, 2, p,    5, p,       p,       p,       None]


def test_overlay_entries_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.yolo_overlay_table_bytes(2, 5) == 2 * 5 * R.SLOT_WORDS * 4
    for bad in ((0, 5), (2, 0), (-1, 5)):
        assert lib.yolo_overlay_table_bytes(*bad) == L.EINVAL
    assert lib.yolo_overlay_table_bytes(2, 129) == L.EUNSUPPORTED
    ok = _shapes_args()
    for k in (29, 1, 2, 7, 32, 33):                                        # NULL table / kept / count / palette / matrices / lp_valid
        a = list(ok); a[k] = None
        assert lib.yolo_overlay_shapes(*a) == L.EINVAL, k
    for k in (3, 5, 6, 8, 19, 20, 23, 24, 25, 26, 27, 28, 30):              # non-positive sizes
        for v in (0, -3):
            a = list(ok); a[k] = v
            assert lib.yolo_overlay_shapes(*a) == L.EINVAL, (k, v)
    a = list(ok); a[0] = a[9] = a[14] = None; a[30] = 1
    assert lib.yolo_overlay_shapes(*a) == L.EINVAL                         # no source at all
    a = list(ok); a[30] = 4
    assert lib.yolo_overlay_shapes(*a) == L.EINVAL                         # K is not post_nms + 1 + 1
    a = list(ok); a[29] = C.c_void_p(4100)
    assert lib.yolo_overlay_shapes(*a) == L.EINVAL                         # a table not 16-byte aligned
    for k, v in ((26, 16385), (27, 16385), (28, 256)):
        a = list(ok); a[k] = v
        assert lib.yolo_overlay_shapes(*a) == L.EUNSUPPORTED, k
    a = list(ok); a[5], a[30] = 127, 129
    assert lib.yolo_overlay_shapes(*a) == L.EUNSUPPORTED
    p = C.c_void_p(4096)
    #       frames table N  H   W   C  K  stream
    draw = [p,     p,    2, 32, 48, 3, 5, None]
    for k in (0, 1):
        a = list(draw); a[k] = None
        assert lib.yolo_overlay_draw(*a) == L.EINVAL
    for k in (2, 3, 4, 5, 6):
        for v in (0, -3):
            a = list(draw); a[k] = v
            assert lib.yolo_overlay_draw(*a) == L.EINVAL, (k, v)
    a = list(draw); a[1] = C.c_void_p(4104)
    assert lib.yolo_overlay_draw(*a) == L.EINVAL
    for k, v in ((6, 129), (5, 5), (3, 16385), (4, 16385)):
        a = list(draw); a[k] = v
        assert lib.yolo_overlay_draw(*a) == L.EUNSUPPORTED, (k, v)


def test_frame_overlay_is_exported_lazily():
    import yolo_amd
    from yolo_amd import FrameOverlay, overlay
    assert FrameOverlay is overlay.FrameOverlay is yolo_amd.FrameOverlay
    assert [tuple(c) for c in R.PALETTE[:, :3].tolist()] == list(overlay.PALETTE)


def test_predict_LP_batch_delegates_to_the_device_rows():
    """predict_LP_batch's contract is unchanged: it is predict_LP_rows (the kernel call it used to make) plus the D2H."""
    from yolo_amd import detect
    import yolo_amd
    assert yolo_amd.predict_LP_rows is detect.predict_LP_rows
    body = inspect.getsource(detect.predict_LP_batch).split('"""')[2]
    assert body.strip() == 'return predict_LP_rows(LP_batch_out, LP_slice_point, r_max).cpu().numpy()'
    rows_src = inspect.getsource(detect.predict_LP_rows)
    assert 'yolo_predict_lp_nhwc' in rows_src and '.cpu()' not in rows_src and 'synchronize' not in rows_src
    assert inspect.signature(detect.predict_LP_rows) == inspect.signature(detect.predict_LP_batch)


def test_frame_intake_keeps_the_frames_attribute():
    assert isinstance(intake.FrameIntake.frames, property)
    src = inspect.getsource(intake.FrameIntake.__call__)
    assert 'self._read = ' in src and 'weakref.ref(given)' in src          # the caller's tensor is not kept alive


# ---- the rasteriser --------------------------------------------------------------------------------------------------------
def _dist(ax, ay, bx, by, x, y):
    """float64 distance from (x, y) to the closed segment, the textbook way (projection clamped to [0, 1])."""
    dx, dy = float(bx - ax), float(by - ay)
    dd = dx * dx + dy * dy
    s = 0.0 if dd == 0.0 else min(1.0, max(0.0, ((x - ax) * dx + (y - ay) * dy) / dd))
    return math.hypot(x - (ax + s * dx), y - (ay + s * dy))


SEGMENTS = [(5, 7, 40, 7), (12, 3, 12, 50), (3, 4, 55, 47), (50, 10, 8, 33), (20, 20, 20, 20), (-9, 12, 30, -6), (60, 60, 70, 90),
            (0, 0, 63, 63), (31, 2, 33, 61), (10, 40, 11, 40)]


def test_integer_rule_equals_a_float64_distance_test():
    decided = 0
    for (ax, ay, bx, by) in SEGMENTS:
        for t in (1, 2, 3, 5):
            for y in range(64):
                for x in range(64):
                    d = _dist(ax, ay, bx, by, x, y)
                    if abs(d - t / 2.0) <= 1e-9:                                # on the rim: only the integer rule is exact
                        continue
                    decided += 1
                    assert R.segment_paints(ax, ay, bx, by, t, x, y) == (d < t / 2.0), (ax, ay, bx, by, t, x, y)
    assert decided > 150000
    # on the rim itself the rule includes the point: an axis-aligned edge at t = 2 is 3 px wide
    assert [R.segment_paints(5, 7, 40, 7, 2, 20, y) for y in (5, 6, 7, 8, 9)] == [False, True, True, True, False]


def test_draw_equals_the_rule_on_every_pixel_with_painters_order():
    """draw() visits only each segment's grown box: the whole canvas by the rule gives the same picture."""
    frames = np.random.default_rng(0).integers(0, 256, (1, 40, 64, 3), dtype=np.uint8)
    slots = [([(5, 5), (50, 8), (48, 30), (7, 33)], (10, 20, 30), 2, 1), ([(20, -5), (70, 10), (30, 45), (-4, 20)], (200, 0, 0), 5, 1),
             ([(30, 30), (30, 30), (30, 30), (30, 30)], (1, 2, 3), 5, 1), ([(0, 0), (63, 0), (63, 39), (0, 39)], (9, 9, 9), 1, 0),
             ([(10, 10), (40, 10), (40, 25), (10, 25)], (0, 255, 0), 1, 1)]
    table = R.make_table(slots)[None]
    want = frames.copy()
    for (v, colour, t, en) in slots:
        if not en:
            continue
        for y in range(40):
            for x in range(64):
                if any(R.segment_paints(v[e][0], v[e][1], v[(e + 1) % 4][0], v[(e + 1) % 4][1], t, x, y) for e in range(4)):
                    want[0, y, x] = colour
    got = R.draw(frames, table)
    assert np.array_equal(got, want) and not np.array_equal(got, frames)
    assert np.array_equal(R.draw(frames, R.make_table([slots[3]])[None]), frames)      # nothing enabled: untouched
    # a slot beyond the limits counts as disabled
    bad = [([(5, 5), (2 ** 20 + 1, 8), (48, 30), (7, 33)], (1, 1, 1), 2, 1), ([(5, 5), (50, 8), (48, 30), (7, 33)], (1, 1, 1), 256, 1)]
    assert np.array_equal(R.draw(frames, R.make_table(bad)[None]), frames)


# ---- the shapes ------------------------------------------------------------------------------------------------------------
def _cv2_add_bbox_corners(b, im_h, im_w, use_r):
    """yolo_cv.cv2_add_bbox (yolo_cv.py:253-266) with its array and its astype(int), on float64 inputs."""
    b = [float(v) for v in b]
    r = 0 if not use_r else -b[5]
    h = b[3] * im_h
    w = b[4] * im_w
    a = np.array([[
        [w * math.cos(r) / 2 - h * math.sin(r) / 2, w * math.sin(r) / 2 + h * math.cos(r) / 2],
        [-w * math.cos(r) / 2 - h * math.sin(r) / 2, -w * math.sin(r) / 2 + h * math.cos(r) / 2],
        [-w * math.cos(r) / 2 + h * math.sin(r) / 2, -w * math.sin(r) / 2 - h * math.cos(r) / 2],
        [w * math.cos(r) / 2 + h * math.sin(r) / 2, w * math.sin(r) / 2 - h * math.cos(r) / 2]]])
    s = np.array([b[2], b[1]]) * [im_w, im_h]
    return (a + s)[0], (a + s).astype(int)[0]


def test_box_corners_equal_cv2_add_bbox():
    pred = R.top1_rows(3, 16)
    for (H, W) in ((48, 64), (1080, 1920)):
        for use_r in (False, True):
            out = R.shapes(len(pred), H, W, pred=pred, use_r=use_r)
            for n, p in enumerate(pred):
                v, vi = _cv2_add_bbox_corners(p, H, W, use_r)
                assert np.array_equal(out['v64'][n, 0], v)
                assert np.array_equal(out['table'][n, 0, :8].reshape(4, 2), vi) and out['table'][n, 0, 10] == 1
    # strictly above the threshold (car/video_node.py:316); a NaN row is disabled
    pred[0, 0], pred[1, 0], pred[2, 3] = 0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nan
    out = R.shapes(len(pred), 48, 64, pred=pred)
    assert out['table'][:3, 0, 10].tolist() == [0, 1, 0] and not out['table'][2, 0, :8].any()


def test_nms_slots_follow_the_kept_list():
    rows, kept, count = R.nms_case(5, 2, 12, 9, 6)
    kept[0, 0], count[1] = 12 * 3 + 1, 6                                    # an id out of range; a full row
    kept[1] = [0, 4, 35, -1, 7, 8]                                          # a pad inside the count
    out = R.shapes(2, 48, 64, nms=(rows, kept, count), cand_per_box=3)
    for b in range(2):
        for j in range(6):
            idx = kept[b, j]
            on = j < count[b] and 0 <= idx < 36
            assert out['table'][b, j, 10] == int(on), (b, j)
            if on:
                l, t, r, bo = rows[b, idx // 3, 1:5].astype(np.float64)
                assert np.array_equal(out['v64'][b, j], [[l * 64, t * 48], [r * 64, t * 48], [r * 64, bo * 48], [l * 64, bo * 48]])
                assert out['table'][b, j, 8] == np.int64(R.pack_colour(R.PALETTE[idx % 3])).astype(np.int32)


# Differences between the restatement's matrix (the header's fp64 elimination on the float32 corners) and intake.plate_matrix (LAPACK's
# solve on the same corners), as max |m - ref| / |ref| over the entries, over the 64 poses of plate_rows(7, 64) at three frame sizes.
# MEASURED here on the CPU: 1.43e-13 (conditioning varies with the pose: the worst entries belong to the most tilted plates).
# The bound is 8 x that maximum.
MATRIX_MEASURED = 1.43e-13
MATRIX_BOUND = 8 * MATRIX_MEASURED


def test_plate_corners_and_matrix_equal_the_packages():
    cam, cd = render.PlateCamera(R.CAMERA), R.camera_dict(R.CAMERA)
    assert (cd['fx'], cd['fy'], cd['cx'], cd['cy'], cd['w'], cd['h']) == (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)
    rows = R.plate_rows(7, 64)
    worst = 0.0
    for (H, W) in ((48, 64), (480, 640), (1080, 1920)):
        for r in rows:
            pose = r[1:7].astype(np.float64)
            pts, divides = R.plate_corners(pose, cd)
            want = cam.corners(pose)
            # two fp64 routes to the same corner (closed form / matrix products), each rounded to float32: one float32 step at the most
            assert divides and np.all(np.abs(pts - want) <= np.spacing(np.abs(want)))
            spts, wanted, M, valid = R.plate_entry(r, cd, W, H, 0.5)
            assert wanted and valid == 1 and M.dtype == np.float32 and M[8] == 1
            # the same float32 scaling as plate_matrix's
            scaled = want.copy()
            scaled[:, 0] = scaled[:, 0] * (W / float(cam.w))
            scaled[:, 1] = scaled[:, 1] * (H / float(cam.h))
            assert scaled.dtype == np.float32 and np.all(np.abs(spts - scaled) <= np.spacing(np.abs(scaled)))
            src = [(380, 160), (0, 160), (0, 0), (380, 0)]
            m = np.append(R.solve_homography(src, scaled.astype(np.float64)), 1.0).reshape(3, 3)
            ref = intake.plate_matrix(pose, cam, (H, W))
            diff = float((np.abs(m - ref) / np.abs(ref)).max())
            worst = max(worst, diff)
            # and the map does what it is for: the plate image's corners land on the frame's
            for (x, y), (u, v) in zip(src, scaled.astype(np.float64)):
                q = m @ [x, y, 1.0]
                assert abs(q[0] / q[2] - u) < 1e-8 and abs(q[1] / q[2] - v) < 1e-8
    print('max |m - plate_matrix| / |plate_matrix| = %.3g (bound %.3g)' % (worst, MATRIX_BOUND))
    assert worst <= MATRIX_BOUND


def test_degenerate_plates_give_the_outside_matrix():
    cd = R.camera_dict(R.CAMERA)
    cases = {'on the image plane': [0.9, 0, 0, 0, 0, 0, 0],                  # Z = 0 and no tilt: w = 0 at every corner
             'edge on': [0.9, 0, 0, 3000, 0, math.pi / 2, 0],               # turned 90 degrees: the float32 corners on one line
             'far away': [0.9, 0, 0, 1e30, 0, 0, 0],                        # the four float32 corners coincide
             'NaN': [0.9, np.nan, 0, 3000, 0, 0, 0], 'inf': [0.9, 0, 0, np.inf, 0, 0, 0],
             'below the threshold': [0.5, 10, 20, 3000, 0.1, 0.2, 0.3]}
    for name, row in cases.items():
        pts, wanted, M, valid = R.plate_entry(np.float32(row), cd, 64, 48, 0.5)
        assert wanted == (name != 'below the threshold')
        assert valid == 0 and np.array_equal(M, R.OUTSIDE), name
    assert R.solve_homography([(0, 0)] * 4, np.ones((4, 2))) is None
