"""The frame overlay restated in numpy / plain Python (the role tests/intake_ref.py plays for the intake): include/yolo_amd.h's
definitions of yolo_overlay_shapes -- the shapes in float64 in the written order, the elimination in the header's order -- and of
yolo_overlay_draw, the rasteriser in Python integers (exact at any size)."""
import math

import numpy as np

f32 = np.float32
SLOT_WORDS = 12
MAX_COORD = 2 ** 20
MAX_T = 255
OUTSIDE = np.array([0, 0, -4, 0, 0, -4, 0, 0, 1], f32)
# the reference's palette (yolo_modules/yolo_cv.py:11-20) padded to four bytes
PALETTE = np.array([(255, 255, 0, 255), (255, 0, 255, 255), (0, 255, 255, 255), (0, 0, 255, 255), (0, 255, 0, 255), (255, 0, 0, 255),
                    (255, 255, 255, 255), (0, 0, 0, 255)], np.uint8)
CAMERA = {'image_width': 640, 'image_height': 480,
          'projection_matrix': {'data': [410.0, 0.0, 322.5, 0.0, 0.0, 415.5, 238.25, 0.0, 0.0, 0.0, 1.0, 0.0]}}


def pack_colour(c):
    c = [int(v) for v in c]
    c = c + [255] * (4 - len(c))
    return c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24)


# ---- shapes --------------------------------------------------------------------------------------------------------------------
def box_vertices(row, W, H):
    """NMS slot: [score, l, t, r, b, ...] -> float64 (4,2)."""
    l, t, r, b = [float(v) for v in row[1:5]]
    return np.array([[l * W, t * H], [r * W, t * H], [r * W, b * H], [l * W, b * H]], np.float64)


def top1_vertices(p, W, H, use_r):
    """cv2_add_bbox's corners in the header's operation order, float64."""
    r = -float(p[5]) if use_r else 0.0
    h, w = float(p[3]) * H, float(p[4]) * W
    cr, sr = math.cos(r), math.sin(r)
    wc, hs, ws, hc = (w * cr) / 2.0, (h * sr) / 2.0, (w * sr) / 2.0, (h * cr) / 2.0
    sx, sy = float(p[2]) * W, float(p[1]) * H
    return np.array([[(wc - hs) + sx, (ws + hc) + sy], [(-wc - hs) + sx, (-ws + hc) + sy],
                     [(-wc + hs) + sx, (-ws - hc) + sy], [(wc + hs) + sx, (ws - hc) + sy]], np.float64)


def plate_corners(pose, cam):
    """projection_matrix's closed form + __call__'s divide -> (float32 (4,2) [NaN / inf where w = 0], all four w non-zero)."""
    X, Y, Z, r1, r2, r3 = [float(v) for v in pose]
    fx, fy, cx, cy = cam['fx'], cam['fy'], cam['cx'], cam['cy']
    sin, cos = math.sin, math.cos
    a = sin(r1) * cos(r2) * 84.0
    b = sin(r1) * sin(r2) * cos(r3) * 84.0
    c = sin(r2) * 199.5
    d = sin(r3) * cos(r1) * 84.0
    e = cos(r2) * cos(r3) * 199.5
    f = sin(r1) * sin(r2) * sin(r3) * 84.0
    g = sin(r3) * cos(r2) * 199.5
    h = cos(r1) * cos(r3) * 84.0
    with np.errstate(all='ignore'):
        ans = np.array([[cx * (Z + a - c) + fx * (X + b - d + e), cx * (Z + a + c) + fx * (X + b - d - e),
                         cx * (Z - a + c) + fx * (X - b + d - e), cx * (Z - a - c) + fx * (X - b + d + e)],
                        [cy * (Z + a - c) + fy * (Y + f + g + h), cy * (Z + a + c) + fy * (Y + f - g + h),
                         cy * (Z - a + c) + fy * (Y - f - g - h), cy * (Z - a - c) + fy * (Y - f + g - h)],
                        [Z + a - c, Z + a + c, Z - a + c, Z - a - c]], np.float64)
        pts = np.stack([ans[0] / ans[2], ans[1] / ans[2]], axis=1).astype(f32)
    return pts, bool(np.all(ans[2] != 0.0))


def camera_dict(camera):
    """a render.PlateCamera-style calibration dict -> the six numbers the entry takes."""
    P = camera['projection_matrix']['data']
    return dict(fx=float(P[0]), fy=float(P[5]), cx=float(P[2]), cy=float(P[6]), w=int(camera['image_width']), h=int(camera['image_height']))


def scaled_plate_corners(pose, cam, W, H):
    pts, divides = plate_corners(pose, cam)
    with np.errstate(all='ignore'):
        pts[:, 0] = pts[:, 0] * f32(W / float(cam['w']))
        pts[:, 1] = pts[:, 1] * f32(H / float(cam['h']))
    return pts, divides


def solve_homography(src, dst):
    """The header's elimination, float64 -> (m0..m7 or None when a pivot is zero / not finite or a solution entry is not finite)."""
    A = np.zeros((8, 9), np.float64)
    for i in range(4):
        x, y, u, v = float(src[i][0]), float(src[i][1]), float(dst[i][0]), float(dst[i][1])
        A[i] = [x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u, u]
        A[i + 4] = [0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v, v]
    with np.errstate(all='ignore'):
        for k in range(8):
            p, best = k, abs(A[k, k])
            for r in range(k + 1, 8):
                if abs(A[r, k]) > best:
                    p, best = r, abs(A[r, k])
            if p != k:
                A[[k, p]] = A[[p, k]]
            piv = A[k, k]
            if not (abs(piv) > 0.0) or not math.isfinite(piv):
                return None
            for r in range(k + 1, 8):
                fct = A[r, k] / piv
                for c in range(k, 9):
                    A[r, c] = A[r, c] - fct * A[k, c]
        m = np.zeros(8, np.float64)
        for k in range(7, -1, -1):
            s = A[k, 8]
            for c in range(k + 1, 8):
                s = s - A[k, c] * m[c]
            m[k] = s / A[k, k]
    return m if np.all(np.isfinite(m)) else None


def plate_entry(lp_row, cam, W, H, lp_threshold, LP_size=(160, 380)):
    """-> (float32 (4,2) scaled corners, wanted, float32 (9,) matrix, lp_valid)."""
    pts, divides = scaled_plate_corners(lp_row[1:7], cam, W, H)
    wanted = bool(f32(lp_row[0]) > f32(lp_threshold))
    m = None
    if wanted and divides and np.all(np.isfinite(pts)):
        src = [(LP_size[1], LP_size[0]), (0, LP_size[0]), (0, 0), (LP_size[1], 0)]
        m = solve_homography(src, pts.astype(np.float64))
    if m is None:
        return pts, wanted, OUTSIDE.copy(), 0
    return pts, wanted, np.append(m, 1.0).astype(f32), 1


def _slot(v64, colour, t, enabled):
    """float64 (4,2) vertices -> the 12 words."""
    ok = bool(np.all(np.isfinite(v64)) and np.all(np.abs(v64) <= MAX_COORD))
    words = np.zeros(SLOT_WORDS, np.int64)
    if ok:
        words[:8] = np.trunc(v64).astype(np.int64).reshape(8)
    words[8], words[9], words[10] = colour, t, int(enabled and ok)
    return words


def shapes(B, H, W, thickness=2, nms=None, cand_per_box=1, palette=PALETTE, pred=None, car_threshold=0.5, use_r=False,
           car_color=(0, 255, 0), lp=None, camera=None, lp_threshold=0.5, lp_color=(0, 0, 255), LP_size=(160, 380)):
    """yolo_overlay_shapes -> dict(table int32 (B,K,12) [colour as the int32 the device holds], v64 float64 (B,K,4,2) [the vertices
    before rounding: the plate's are its float32 corners], vertices float32, matrices (B,9) / None, lp_valid (B,) uint8 / None)."""
    post = nms[1].shape[1] if nms is not None else 0
    K = post + (pred is not None) + (lp is not None)
    table = np.zeros((B, K, SLOT_WORDS), np.int64)
    v64 = np.zeros((B, K, 4, 2), np.float64)
    mats = np.zeros((B, 9), f32) if lp is not None else None
    valid = np.zeros(B, np.uint8) if lp is not None else None
    cam = camera_dict(camera) if lp is not None else None
    with np.errstate(all='ignore'):
        for b in range(B):
            s = 0
            if nms is not None:
                rows, kept, count = nms
                nbox = rows.shape[1]
                for j in range(post):
                    idx = int(kept[b, j]) if j < min(int(count[b]), post) else -1
                    box = idx // cand_per_box if idx >= 0 else -1
                    if 0 <= box < nbox:
                        v64[b, s] = box_vertices(rows[b, box], W, H)
                        colour = pack_colour(palette[(idx % cand_per_box) % len(palette)])
                        table[b, s] = _slot(v64[b, s], colour, thickness, True)
                    else:
                        table[b, s] = _slot(v64[b, s], 0, thickness, False)
                    s += 1
            if pred is not None:
                v64[b, s] = top1_vertices(pred[b], W, H, use_r)
                table[b, s] = _slot(v64[b, s], pack_colour(car_color), thickness, bool(f32(pred[b, 0]) > f32(car_threshold)))
                s += 1
            if lp is not None:
                pts, wanted, mats[b], valid[b] = plate_entry(lp[b], cam, W, H, lp_threshold, LP_size)
                v64[b, s] = pts.astype(np.float64)
                table[b, s] = _slot(v64[b, s], pack_colour(lp_color), thickness, wanted)
    table = (table & 0xffffffff).astype(np.uint32).view(np.int32)
    return dict(table=table, v64=v64, vertices=v64.astype(f32), matrices=mats, lp_valid=valid)


# ---- draw ----------------------------------------------------------------------------------------------------------------------
def segment_paints(ax, ay, bx, by, t, x, y):
    """4 dist^2 <= t^2 for the integer point (x, y) and the closed segment A -> B, in Python integers (no overflow at any size)."""
    dx, dy, px, py = bx - ax, by - ay, x - ax, y - ay
    u, dd = px * dx + py * dy, dx * dx + dy * dy
    if u <= 0:
        return 4 * (px * px + py * py) <= t * t
    if u >= dd:
        return 4 * ((px - dx) ** 2 + (py - dy) ** 2) <= t * t
    cr = px * dy - py * dx
    return 4 * cr * cr <= t * t * dd


def slot_enabled(words):
    return bool(words[10] != 0 and 1 <= words[9] <= MAX_T and all(-MAX_COORD <= int(v) <= MAX_COORD for v in words[:8]))


def draw(frames, table):
    """yolo_overlay_draw: frames (N,H,W,C) uint8, table (N,K,12) int32 -> a painted copy."""
    out = np.array(frames, copy=True)
    N, H, W, C = out.shape
    table = np.asarray(table)
    for n in range(N):
        for words in table[n]:                                  # ascending: a later slot paints over an earlier one
            if not slot_enabled(words):
                continue
            w = [int(v) for v in words]
            t, grow = w[9], (w[9] + 1) // 2
            colour = [(w[8] >> (8 * c)) & 0xff for c in range(C)]
            for e in range(4):
                ax, ay, bx, by = w[2 * e], w[2 * e + 1], w[2 * ((e + 1) % 4)], w[2 * ((e + 1) % 4) + 1]
                # only the pixels of the segment's grown box can be within t / 2 (an exact test follows for each of them)
                for y in range(max(0, min(ay, by) - grow), min(H - 1, max(ay, by) + grow) + 1):
                    for x in range(max(0, min(ax, bx) - grow), min(W - 1, max(ax, bx) + grow) + 1):
                        if segment_paints(ax, ay, bx, by, t, x, y):
                            out[n, y, x] = colour
    return out


def make_table(slots):
    """[(vertices [(x, y)] * 4, colour tuple, t, enabled)] -> int32 (K,12)."""
    tab = np.zeros((len(slots), SLOT_WORDS), np.int64)
    for k, (v, colour, t, en) in enumerate(slots):
        tab[k, :8] = np.asarray(v, np.int64).reshape(8)
        tab[k, 8], tab[k, 9], tab[k, 10] = pack_colour(colour), t, en
    return (tab & 0xffffffff).astype(np.uint32).view(np.int32)


# ---- shared cases of tests/test_overlay_host.py and tests/test_gpu_overlay.py ---------------------------------------------------
def plate_rows(seed, n):
    """float32 (n,7) rows [score, X, Y, Z mm, r1, r2, r3 rad]: plates 1.5 .. 6 m in front of the camera, turned by up to 0.7 rad."""
    g = np.random.default_rng(seed)
    rows = np.empty((n, 7), np.float64)
    rows[:, 0] = g.uniform(0.6, 1.0, n)
    rows[:, 1] = g.uniform(-500, 500, n)
    rows[:, 2] = g.uniform(-300, 300, n)
    rows[:, 3] = g.uniform(1500, 6000, n)
    rows[:, 4:7] = g.uniform(-0.7, 0.7, (n, 3))
    return rows.astype(f32)


def top1_rows(seed, n, C=8):
    """float32 (n,C) rows [score, y, x, h, w, rot, cls...]."""
    g = np.random.default_rng(seed)
    rows = g.uniform(0.0, 1.0, (n, C))
    rows[:, 0] = g.uniform(0.6, 1.0, n)
    rows[:, 3:5] = g.uniform(0.1, 0.6, (n, 2))
    rows[:, 5] = g.uniform(-1.5, 1.5, n)
    return rows.astype(f32)


def nms_case(seed, B, nbox, C, post):
    """decoded rows (B,nbox,C) [score, l, t, r, b, rot, cls...] with some boxes leaving the frame, kept ids ('class' mode:
    id = box * (C - 6) + class) padded with -1, kept counts."""
    g = np.random.default_rng(seed)
    rows = g.uniform(0.0, 1.0, (B, nbox, C))
    cy, cx = g.uniform(-0.1, 1.1, (B, nbox)), g.uniform(-0.1, 1.1, (B, nbox))
    h, w = g.uniform(0.05, 0.5, (B, nbox)), g.uniform(0.05, 0.5, (B, nbox))
    rows[:, :, 1], rows[:, :, 2], rows[:, :, 3], rows[:, :, 4] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    count = g.integers(1, post + 1, B).astype(np.int32)
    kept = np.full((B, post), -1, np.int32)
    for b in range(B):
        kept[b, :count[b]] = g.integers(0, nbox * (C - 6), count[b])
    return rows.astype(f32), kept, count


def far_from_integers(v64, margin=1e-6):
    """every finite vertex coordinate lies at least `margin` from an integer (so a last-bit difference cannot move a truncation);
    slots whose eight coordinates are all exactly 0 -- an NMS slot without a box: nothing was computed -- are left out."""
    v = np.asarray(v64, np.float64).reshape(-1, 8)
    v = v[np.any(v != 0.0, axis=1)]
    v = v[np.isfinite(v)]
    return bool(np.all(np.abs(v - np.rint(v)) >= margin))
