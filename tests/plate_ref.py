"""The device plate renderer restated in numpy (the role tests/render_ref.py plays for the cars): yolo_plate_compose,
yolo_plate_stats and yolo_plate_render as include/yolo_amd.h defines them, every operation in float32 and in the header's order,
the noise in integers, so an IEEE device reproduces it bit for bit -- except the canvas mean, which is taken here from ONE float64
sum (the device adds 16 partial sums: the float32 it rounds to can differ by an ulp).  Also Philox4x32-10, the row packer and
unpacker, and the glyph images and camera the two test files share."""
import math

import numpy as np

f32 = np.float32
u32 = np.uint32
IDX_LIMIT = f32(2.0 ** 30)
ROW_WORDS = 48
PLATE_H, PLATE_W = 160, 380
GLYPH_H, GLYPH_W, GLYPH_TOP = 90, 45, 35
DOT_H, DOT_W, DOT_TOP, DOT_LEFT = 70, 10, 45, 158
CELL_X = (7, 56, 106, 175, 225, 274, 324)
GLYPH_BYTES = 34 * GLYPH_H * GLYPH_W * 4 + DOT_H * DOT_W * 4
NOISE_UNIT = math.sqrt(8 * 65535 / 12.0)                 # the standard deviation of a sum of 8 uniform bytes
CAMERA = {'image_width': 640, 'image_height': 480,
          'projection_matrix': {'data': [610.0, 0.0, 322.5, 0.0, 0.0, 608.0, 241.25, 0.0, 0.0, 0.0, 1.0, 0.0]}}


# ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11; Random123's constants) ------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays of one shape (or scalars), key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & np.uint64(0xffffffff) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    m0, m1, lo32, sh = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                    # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return [v.astype(u32) for v in c]


def _byte_sum(a, b):
    a, b = a.astype(np.int64), b.astype(np.int64)
    return sum(((w >> s) & 255) for w in (a, b) for s in (0, 8, 16, 24))


def noise_z(key, H, W):
    """z (H, W, 4) float32: per pixel (column j, row i) and channel R, G, B, A the sum of 8 Philox bytes less 1020."""
    j = np.broadcast_to(np.arange(W, dtype=np.uint64)[None, :], (H, W))
    i = np.broadcast_to(np.arange(H, dtype=np.uint64)[:, None], (H, W))
    z = np.zeros((H, W, 4), f32)
    for h in (0, 1):
        w = philox4x32_10([j, i, np.uint64(h), np.uint64(0)], key)
        z[..., 2 * h] = (_byte_sum(w[0], w[1]) - 1020).astype(f32)
        z[..., 2 * h + 1] = (_byte_sum(w[2], w[3]) - 1020).astype(f32)
    return z


def noise_scale(sigma):
    return f32(sigma / NOISE_UNIT)


# ---- rows --------------------------------------------------------------------------------------------------------------------
def unpack(row):
    """One int32 row -> dict of its fields (the layout of include/yolo_amd.h, yolo_plate_render)."""
    row = np.ascontiguousarray(row, np.int32)
    fl = row.view(f32)
    return dict(has=int(row[0]), ids=[int(v) for v in row[1:8]], win=[int(v) for v in row[8:12]],
                key=(int(row[12:14].view(u32)[0]), int(row[12:14].view(u32)[1])), s=f32(fl[14]), m=fl[16:25].copy(),
                w0=f32(fl[25]), w1=f32(fl[26]), A=fl[27:36].reshape(3, 3).copy(), D=fl[36:45].reshape(3, 3).copy(), e=fl[45:48].copy())


def make_row(ids, m, win, key=(0, 0), s=0.0, w0=1.0, w1=0.0, A=None, D=None, e=None, has=1):
    """The other way round, for tests that write rows by hand (m: 9 numbers, canvas index -> texel index)."""
    row = np.zeros(ROW_WORDS, np.int32)
    fl = row.view(f32)
    row[0] = has
    row[1:8] = ids
    row[8:12] = win
    row[12:14] = np.asarray(key, u32).view(np.int32)
    fl[14] = f32(s)
    fl[16:25] = np.asarray(m, np.float64).reshape(9).astype(f32)
    fl[25], fl[26] = f32(w0), f32(w1)
    fl[27:36] = (np.eye(3) if A is None else np.asarray(A, np.float64)).reshape(9).astype(f32)
    fl[36:45] = (np.zeros((3, 3)) if D is None else np.asarray(D, np.float64)).reshape(9).astype(f32)
    fl[45:48] = (np.zeros(3) if e is None else np.asarray(e, np.float64)).astype(f32)
    return row


def has_plate(r):
    return r['has'] != 0 and all(0 <= g < 34 for g in r['ids'])


# ---- compose -----------------------------------------------------------------------------------------------------------------
def split_atlas(glyphs):
    """The atlas bytes -> (34 glyph arrays (90,45,4), the dot (70,10,4))."""
    glyphs = np.asarray(glyphs, np.uint8).reshape(-1)
    assert glyphs.size == GLYPH_BYTES
    n = GLYPH_H * GLYPH_W * 4
    return [glyphs[k * n:(k + 1) * n].reshape(GLYPH_H, GLYPH_W, 4) for k in range(34)], glyphs[34 * n:].reshape(DOT_H, DOT_W, 4)


def compose(glyphs, rows, fill=0):
    """-> plates (N,160,380,4) uint8; the plate of a no-plate row keeps `fill` (the device does not write it)."""
    glyph, dot = split_atlas(glyphs)
    plates = np.full((len(rows), PLATE_H, PLATE_W, 4), fill, np.uint8)
    for n, row in enumerate(rows):
        r = unpack(row)
        if not has_plate(r):
            continue
        plates[n] = 255
        for k, g in enumerate(r['ids']):
            plates[n, GLYPH_TOP:GLYPH_TOP + GLYPH_H, CELL_X[k]:CELL_X[k] + GLYPH_W] = glyph[g]
        plates[n, DOT_TOP:DOT_TOP + DOT_H, DOT_LEFT:DOT_LEFT + DOT_W] = dot
    return plates


# ---- the pixels --------------------------------------------------------------------------------------------------------------
def tap(level, sx, sy):
    """yolo_render_cars' bilinear tap of an (h, w, 4) uint8 image at float32 positions (sx, sy) -> (..., 4) float32."""
    h, w = level.shape[:2]
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f)[..., None], (sy - y0f)[..., None]
    assert fx.dtype == f32 and fy.dtype == f32
    x0 = np.fmin(np.fmax(x0f, -IDX_LIMIT), IDX_LIMIT).astype(np.int64)
    y0 = np.fmin(np.fmax(y0f, -IDX_LIMIT), IDX_LIMIT).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1, cy0, cy1 = np.clip(x0, 0, w - 1), np.clip(x1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)
    inx0, inx1, iny0, iny1 = cx0 == x0, cx1 == x1, cy0 == y0, cy1 == y1
    lv, zero = level.astype(f32), f32(0)
    ta = np.where((inx0 & iny0)[..., None], lv[cy0, cx0], zero)
    tb = np.where((inx1 & iny0)[..., None], lv[cy0, cx1], zero)
    tc = np.where((inx0 & iny1)[..., None], lv[cy1, cx0], zero)
    td = np.where((inx1 & iny1)[..., None], lv[cy1, cx1], zero)
    top = ta + fx * (tb - ta)
    bot = tc + fx * (td - tc)
    val = top + fy * (bot - top)
    assert val.dtype == f32
    return val


def sample(plate, m, x, y):
    """S(x, y) for float32 arrays x, y of one shape -> (..., 4) float32: 0 where !(den > 0) or den is not finite."""
    with np.errstate(all='ignore'):
        nx = (m[0] * x + m[1] * y) + m[2]
        ny = (m[3] * x + m[4] * y) + m[5]
        den = (m[6] * x + m[7] * y) + m[8]
        assert den.dtype == f32
        front = (den > 0) & np.isfinite(den)
        val = tap(plate, nx / den, ny / den)
    return np.where(front[..., None], val, f32(0))


def window_of(r, H, W):
    return max(r['win'][0], 0), max(r['win'][1], 0), min(r['win'][2], W), min(r['win'][3], H)


def quad(plate, r, H, W):
    """Q for every pixel of an (H, W) canvas -> (H, W, 4) float32."""
    j = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
    i = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W))
    m, w0, w1 = r['m'], r['w0'], r['w1']
    with np.errstate(all='ignore'):
        if w1 == 0:
            P = sample(plate, m, j, i)
        else:
            one, rows = f32(1), []
            for dy in (-1, 0, 1):
                y = i + f32(dy)
                rows.append((w1 * sample(plate, m, j - one, y) + w0 * sample(plate, m, j, y)) + w1 * sample(plate, m, j + one, y))
            P = (w1 * rows[0] + w0 * rows[1]) + w1 * rows[2]
        assert P.dtype == f32
        l, t, rr, b = window_of(r, H, W)
        Q = np.zeros((H, W, 4), f32)
        if rr > l and b > t:
            Q[t:b, l:rr] = P[t:b, l:rr]
        if r['s'] != 0:
            Q = np.fmin(np.fmax(Q + noise_z(r['key'], H, W) * r['s'], f32(0)), f32(255))
        assert Q.dtype == f32
    return Q


def render(bg, plates, rows, return_parts=False):
    """bg (N,3,H,W) float32 0..1, plates (N,160,380,4) uint8, rows (N, ROW_WORDS) int32 -> out (N,3,H,W) float32 0..1
    (return_parts: also the per-image mean colour float32 (N,3) and mask (N,H,W))."""
    bg = np.asarray(bg, f32)
    N, _, H, W = bg.shape
    out = np.fmin(np.fmax(bg, f32(0)), f32(1))
    mus, masks = np.zeros((N, 3), f32), np.zeros((N, H, W), f32)
    for n in range(N):
        r = unpack(rows[n])
        if not has_plate(r):
            continue
        Q = quad(plates[n], r, H, W)
        l, t, rr, b = window_of(r, H, W)
        drawn = np.zeros((H, W), bool)
        if r['s'] != 0:
            drawn[:] = True
        elif rr > l and b > t:
            drawn[t:b, l:rr] = True
        with np.errstate(all='ignore'):
            mu = (Q[..., :3].astype(np.float64).sum(axis=(0, 1)) / float(H * W)).astype(f32)
            k = ((r['D'][:, 0] * mu[0] + r['D'][:, 1] * mu[1]) + r['D'][:, 2] * mu[2]) + r['e']
            mask = Q[..., 3] / f32(255)
            for c in range(3):
                A = r['A'][c]
                fg = (((A[0] * Q[..., 0] + A[1] * Q[..., 1]) + A[2] * Q[..., 2]) + k[c]) / f32(255)
                v = bg[n, c] * (f32(1) - mask) + fg * mask
                assert v.dtype == f32
                out[n, c] = np.where(drawn, np.fmin(np.fmax(v, f32(0)), f32(1)), out[n, c])
        mus[n], masks[n] = mu, np.where(drawn, mask, f32(0))
    return (out, mus, masks) if return_parts else out


# ---- what tests/test_plate_device_host.py and tests/test_gpu_plates.py share -------------------------------------------------
def write_fonts(root, size=(60, 30)):
    """Glyph images named as licence_plate_render/fonts (0..33 = digits then letters, 34 = the dot): a coloured bar per glyph on
    a transparent ground with an alpha RAMP down the bar (soft alpha, so that a paste of all four bytes differs from an
    alpha-blended one), each glyph its own colour and extent."""
    import os
    from PIL import Image
    os.makedirs(root)
    h, w = size
    for k in range(35):
        px = np.zeros((h, w, 4), np.uint8)
        top, bot, left, right = 6, 50 + k % 7, 4 + k % 5, 24
        px[top:bot, left:right, 0], px[top:bot, left:right, 1], px[top:bot, left:right, 2] = 10 + 6 * k, 240 - 5 * k, (37 * k) % 255
        px[top:bot, left:right, 3] = np.linspace(255, 40 + 3 * k, bot - top).astype(np.uint8)[:, None]
        Image.fromarray(px).save(os.path.join(root, '%d.png' % k))


def quad_map(quad_xy, H, W, homography, corners):
    """The row's map for a plate whose corners (bottom-right, bottom-left, top-left, top-right, as LP_CORNERS orders them) land on
    the CONTINUOUS canvas points quad_xy: canvas index -> (+0.5) -> plate through homography(quad, LP_CORNERS) -> (-0.5)."""
    half = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
    return np.linalg.inv(half) @ homography(np.float64(quad_xy), corners) @ half


def window(m, H, W, slack=1.01):
    """The conservative window of a map: samples are non-zero only for texel indices in (-1, 380) x (-1, 160); their pre-image's
    bound, rounded outwards, plus `slack` (1 px of blur, 0.01 for float32), clipped to the canvas."""
    F = np.linalg.inv(np.asarray(m, np.float64).reshape(3, 3))
    xs, ys = np.float64([-1, PLATE_W, PLATE_W, -1]), np.float64([-1, -1, PLATE_H, PLATE_H])
    den = F[2, 0] * xs + F[2, 1] * ys + F[2, 2]
    px, py = (F[0, 0] * xs + F[0, 1] * ys + F[0, 2]) / den, (F[1, 0] * xs + F[1, 1] * ys + F[1, 2]) / den
    win = [math.floor(px.min() - slack), math.floor(py.min() - slack), math.ceil(px.max() + slack) + 1, math.ceil(py.max() + slack) + 1]
    return [min(max(win[0], 0), W), min(max(win[1], 0), H), min(max(win[2], 0), W), min(max(win[3], 0), H)]
