"""The background kernels restated in numpy (the role tests/render_ref.py plays for the car renderer): yolo_bg_stats and
yolo_bg_render as include/yolo_amd.h defines them, every operation in float32 and in the header's order, so an IEEE device
reproduces it bit for bit -- except the mean, which is taken here from ONE float64 sum (the device adds 16 partial sums: the float32
it rounds to can differ by an ulp).  `ft=np.float64` evaluates the same row in float64 (the stored float32 parameters widened).
Also the bank, the rows and the geometry the two test files share; nothing here imports the package."""
import numpy as np

f32 = np.float32
ROW_WORDS = 40
IMAGE_SIZES = ((9, 7), (37, 53), (48, 64), (5, 5), (32, 48))       # (h, w); mip levels 1, 3, 3, 1, 3
OUTPUTS = ((16, 24), (13, 13))                                     # W % 4 == 0: vector stores / scalar stores, a tail thread
MIP_MIN_SIDE = 8


def unpack(row):
    """One int32 row -> dict of its fields (the layout of include/yolo_amd.h)."""
    row = np.ascontiguousarray(row, np.int32)
    fl = row.view(f32)
    return dict(has=int(row[0]), h=int(row[1]), w=int(row[2]), roi=[int(v) for v in row[3:7]], off=int(row[8:10].view(np.int64)[0]),
                a=fl[10:16].copy(), A=fl[16:25].reshape(3, 3).copy(), D=fl[25:34].reshape(3, 3).copy(), e=fl[34:37].copy())


def make_row(off, h, w, roi, a, A=None, D=None, e=None, has=1):
    """The other way round, for tests that write rows by hand."""
    row = np.zeros(ROW_WORDS, np.int32)
    fl = row.view(f32)
    row[0], row[1], row[2] = has, h, w
    row[3:7] = roi
    row[8:10] = np.array([off], np.int64).view(np.int32)
    fl[10:16] = np.asarray(a, np.float64).reshape(6).astype(f32)
    fl[16:25] = (np.eye(3) if A is None else np.asarray(A, np.float64)).reshape(9).astype(f32)
    fl[25:34] = (np.zeros((3, 3)) if D is None else np.asarray(D, np.float64)).reshape(9).astype(f32)
    fl[34:37] = (np.zeros(3) if e is None else np.asarray(e, np.float64)).astype(f32)
    return row


def level_of(bank, r, bank_bytes=None):
    """The (h, w, 4) uint8 level a row points at, or None when the row is 'no image': the flag, the level against bank_bytes (default:
    all of `bank`), the roi against the level."""
    nb = bank.size if bank_bytes is None else int(bank_bytes)
    x0, y0, x1, y1 = r['roi']
    ok = (r['has'] != 0 and r['h'] > 0 and r['w'] > 0 and r['off'] >= 0 and r['off'] % 4 == 0 and r['off'] <= nb
          and r['h'] * r['w'] <= (nb - r['off']) // 4
          and x0 >= 0 and y0 >= 0 and x1 >= x0 and y1 >= y0 and x1 < r['w'] and y1 < r['h'])
    if not ok:
        return None
    return bank[r['off']:r['off'] + 4 * r['h'] * r['w']].reshape(r['h'], r['w'], 4)


def pixels(level, r, H, W, ft=f32):
    """P for every pixel of an (H, W) output -> (H, W, 3) of type ft; zeros for level None."""
    if level is None:
        return np.zeros((H, W, 3), ft)
    a = r['a'].astype(ft)
    j = np.broadcast_to(np.arange(W, dtype=ft)[None, :], (H, W))
    i = np.broadcast_to(np.arange(H, dtype=ft)[:, None], (H, W))
    sx = (a[0] * j + a[1] * i) + a[2]
    sy = (a[3] * j + a[4] * i) + a[5]
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f)[..., None], (sy - y0f)[..., None]
    assert fx.dtype == ft and fy.dtype == ft
    lim = ft(2.0 ** 30)
    x0 = np.fmin(np.fmax(x0f, -lim), lim).astype(np.int64)
    y0 = np.fmin(np.fmax(y0f, -lim), lim).astype(np.int64)
    rx0, ry0, rx1, ry1 = r['roi']
    cx0, cx1, cy0, cy1 = np.clip(x0, rx0, rx1), np.clip(x0 + 1, rx0, rx1), np.clip(y0, ry0, ry1), np.clip(y0 + 1, ry0, ry1)
    lv = level[..., :3].astype(ft)
    ta, tb, tc, td = lv[cy0, cx0], lv[cy0, cx1], lv[cy1, cx0], lv[cy1, cx1]
    top = ta + fx * (tb - ta)
    bot = tc + fx * (td - tc)
    P = top + fy * (bot - top)
    assert P.dtype == ft
    return P


def render(bank, rows, H, W, bank_bytes=None, ft=f32, return_parts=False):
    """bank uint8 (bytes,), rows (N, ROW_WORDS) int32 -> out (N,3,H,W) of type ft, 0..255 and not clamped
    (return_parts: also P (N,H,W,3) and the mean colour (N,3))."""
    bank = np.asarray(bank, np.uint8).reshape(-1)
    N = len(rows)
    out, Ps, mus = np.zeros((N, 3, H, W), ft), np.zeros((N, H, W, 3), ft), np.zeros((N, 3), ft)
    for n in range(N):
        r = unpack(rows[n])
        P = pixels(level_of(bank, r, bank_bytes), r, H, W, ft)
        mu = (P.astype(np.float64).sum(axis=(0, 1)) / float(H * W)).astype(ft)
        A, D, e = r['A'].astype(ft), r['D'].astype(ft), r['e'].astype(ft)
        k = ((D[:, 0] * mu[0] + D[:, 1] * mu[1]) + D[:, 2] * mu[2]) + e
        for c in range(3):
            v = ((A[c, 0] * P[..., 0] + A[c, 1] * P[..., 1]) + A[c, 2] * P[..., 2]) + k[c]
            assert v.dtype == ft
            out[n, c] = v
        Ps[n], mus[n] = P, mu
    return (out, Ps, mus) if return_parts else out


# ---- what tests/test_background_host.py and tests/test_gpu_background.py share ----------------------------------------------
def bank_images(seed=0, sizes=IMAGE_SIZES):
    """Noise images (h, w, 3) uint8: the steepest slope a tap error can meet."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def mip_chain(px):
    """The bank's mip rule restated: 2x2 average rounded to nearest, an odd last row / column dropped, down to the last level
    whose shorter side is still >= MIP_MIN_SIDE."""
    levels = [np.ascontiguousarray(px, np.uint8)]
    while min(levels[-1].shape[:2]) // 2 >= MIP_MIN_SIDE:
        a = levels[-1]
        h, w = a.shape[0] // 2 * 2, a.shape[1] // 2 * 2
        a = a[:h, :w].astype(np.uint16)
        levels.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return levels


def pack_bank(images, chain=mip_chain):
    """-> (bank bytes, table[s] = [(offset, h, w) per level]): every image as R, G, B, 255 followed by its levels."""
    chunks, table, off = [], [], 0
    for im in images:
        px = np.full(im.shape[:2] + (4,), 255, np.uint8)
        px[..., :3] = im
        rows = []
        for lv in chain(px):
            rows.append((off, lv.shape[0], lv.shape[1]))
            chunks.append(lv.reshape(-1))
            off += lv.size
        table.append(rows)
    return np.concatenate(chunks), table


def crop_row(table, s, crop, out_hw, mirror=False, colour=None, level=None, has=1):
    """The row of image s cropped to crop = (x0, y0, cw, ch) and resized to out_hw, derived here on its own: cv2.resize's
    half-pixel map X = x0 + (j + 0.5) cw / Wo - 0.5 (mirrored: x0 + cw - 1 - that), the level coordinate (X + 0.5) / 2^L - 0.5,
    L by the rule (the residual of max(Wo / cw, Ho / ch) in (0.5, 1] where the image has that level), the roi
    [x0 >> L, (x0 + cw - 1) >> L] clipped to the level."""
    x0, y0, cw, ch = crop
    Ho, Wo = out_hw
    if level is None:
        level, scale = 0, max(Wo / float(cw), Ho / float(ch))
        while scale * 2 ** level <= 0.5 and level + 1 < len(table[s]):
            level += 1
    off, lh, lw = table[s][level]
    ax, ay = cw / float(Wo), ch / float(Ho)
    bx, by = 0.5 * ax - 0.5, 0.5 * ay - 0.5
    mx, cx = (-ax, x0 + cw - 1 - bx) if mirror else (ax, x0 + bx)
    k = 0.5 ** level
    a = [mx * k, 0.0, (cx + 0.5) * k - 0.5, 0.0, ay * k, (y0 + by + 0.5) * k - 0.5]
    roi = [min(x0 >> level, lw - 1), min(y0 >> level, lh - 1), min((x0 + cw - 1) >> level, lw - 1), min((y0 + ch - 1) >> level, lh - 1)]
    A, D, e = colour if colour is not None else (None, None, None)
    return make_row(off, lh, lw, roi, a, A, D, e, has)


def contrast_only(alpha):
    """(A, D, e) of a contrast stage alone: out = alpha x + (1 - alpha) luma(mean x)."""
    coef = np.float64([0.299, 0.587, 0.114])
    return alpha * np.eye(3), (1 - alpha) * np.outer(np.ones(3), coef), np.zeros(3)


def seven_rows(table, H, W, colour):
    """no image (out = e); an identity-size whole crop (the top-left H x W of the 32 x 48 image, every tap on a pixel); the 37 x 53
    image mirrored; an interior crop magnified 4x or more (border taps must clamp to the ROI); the 48 x 64 image shrunk more than 2x
    on level 1; the 9 x 7 image sampled 2.5 pixels apart, past its only level, and beyond its edge (clamped); `colour` (A, D, e with
    D != 0) on a mirrored interior crop."""
    off, h, w = table[0][0]
    return np.stack([make_row(0, 9, 7, [0, 0, 6, 8], [1, 0, 0, 0, 1, 0], e=[3.0, -2.0, 7.5], has=0),
                     crop_row(table, 4, (0, 0, W, H), (H, W)),
                     crop_row(table, 1, (0, 0, 53, 37), (H, W), mirror=True),
                     crop_row(table, 1, (10, 9, max(1, W // 4), max(1, H // 4)), (H, W)),
                     crop_row(table, 2, (0, 0, 64, 48), (H, W)),
                     make_row(off, h, w, [0, 0, w - 1, h - 1], [2.5, 0.0, 0.75, 0.0, 2.5, 0.75]),
                     crop_row(table, 2, (7, 5, 40, 30), (H, W), mirror=True, colour=colour)])
