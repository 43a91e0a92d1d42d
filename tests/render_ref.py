"""The device renderer restated in numpy (the role tests/intake_ref.py plays for the frame intake): yolo_render_stats and
yolo_render_cars as include/yolo_amd.h defines them, every operation in float32 and in the header's order, so an IEEE device
reproduces it bit for bit -- except the canvas mean, which is taken here from ONE float64 sum (the device adds 16 partial sums:
the float32 it rounds to can differ by an ulp).  Also the sprites and rows the two test files share."""
import numpy as np

f32 = np.float32
IDX_LIMIT = f32(2.0 ** 30)
ROW_WORDS = 40


def unpack(row):
    """One int32 row -> dict of its fields (the layout of include/yolo_amd.h)."""
    row = np.ascontiguousarray(row, np.int32)
    fl = row.view(f32)
    return dict(has=int(row[0]), h=int(row[1]), w=int(row[2]), win=[int(v) for v in row[3:7]],
                off=int(row[8:10].view(np.int64)[0]), a=fl[10:16].copy(), w0=f32(fl[16]), w1=f32(fl[17]),
                A=fl[18:27].reshape(3, 3).copy(), D=fl[27:36].reshape(3, 3).copy(), e=fl[36:39].copy())


def make_row(off, h, w, a, win, w0=1.0, w1=0.0, A=None, D=None, e=None, has=1):
    """The other way round, for tests that write rows by hand."""
    row = np.zeros(ROW_WORDS, np.int32)
    fl = row.view(f32)
    row[0], row[1], row[2] = has, h, w
    row[3:7] = win
    row[8:10] = np.array([off], np.int64).view(np.int32)
    fl[10:16] = np.asarray(a, np.float64).reshape(6).astype(f32)
    fl[16], fl[17] = f32(w0), f32(w1)
    fl[18:27] = (np.eye(3) if A is None else np.asarray(A, np.float64)).reshape(9).astype(f32)
    fl[27:36] = (np.zeros((3, 3)) if D is None else np.asarray(D, np.float64)).reshape(9).astype(f32)
    fl[36:39] = (np.zeros(3) if e is None else np.asarray(e, np.float64)).astype(f32)
    return row


def level_of(atlas, r):
    """The (h, w, 4) uint8 level a row points at, or None when it does not lie inside the atlas ('no sprite')."""
    ok = (r['has'] != 0 and r['h'] > 0 and r['w'] > 0 and r['off'] >= 0 and r['off'] % 4 == 0 and r['off'] <= atlas.size
          and r['h'] * r['w'] <= (atlas.size - r['off']) // 4)
    if not ok:
        return None
    return atlas[r['off']:r['off'] + 4 * r['h'] * r['w']].reshape(r['h'], r['w'], 4)


def sample(level, a, x, y):
    """S(x, y) for float32 arrays x, y of one shape -> (..., 4) float32."""
    h, w = level.shape[:2]
    sx = (a[0] * x + a[1] * y) + a[2]
    sy = (a[3] * x + a[4] * y) + a[5]
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f)[..., None], (sy - y0f)[..., None]
    assert fx.dtype == f32 and fy.dtype == f32
    x0 = np.fmin(np.fmax(x0f, -IDX_LIMIT), IDX_LIMIT).astype(np.int64)
    y0 = np.fmin(np.fmax(y0f, -IDX_LIMIT), IDX_LIMIT).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    cx0, cx1, cy0, cy1 = np.clip(x0, 0, w - 1), np.clip(x1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)
    inx0, inx1, iny0, iny1 = cx0 == x0, cx1 == x1, cy0 == y0, cy1 == y1
    lv = level.astype(f32)
    zero = f32(0)
    ta = np.where((inx0 & iny0)[..., None], lv[cy0, cx0], zero)
    tb = np.where((inx1 & iny0)[..., None], lv[cy0, cx1], zero)
    tc = np.where((inx0 & iny1)[..., None], lv[cy1, cx0], zero)
    td = np.where((inx1 & iny1)[..., None], lv[cy1, cx1], zero)
    top = ta + fx * (tb - ta)
    bot = tc + fx * (td - tc)
    val = top + fy * (bot - top)
    assert val.dtype == f32
    return val


def pixels(level, r, H, W):
    """P for every pixel of an (H, W) canvas -> (H, W, 4) float32 (the window is applied by the callers)."""
    j = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
    i = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W))
    a, w0, w1 = r['a'], r['w0'], r['w1']
    if w1 == 0:
        return sample(level, a, j, i)
    one = f32(1)
    rows = []
    for dy in (-1, 0, 1):
        y = i + f32(dy)
        rows.append((w1 * sample(level, a, j - one, y) + w0 * sample(level, a, j, y)) + w1 * sample(level, a, j + one, y))
    P = (w1 * rows[0] + w0 * rows[1]) + w1 * rows[2]
    assert P.dtype == f32
    return P


def render(bg, atlas, rows, return_parts=False):
    """bg (N,3,H,W) float32 0..255, atlas uint8 (bytes,), rows (N, ROW_WORDS) int32 -> out (N,3,H,W) float32 0..1
    (return_parts: also the per-image mean colour float32 (N,3) and mask (N,H,W))."""
    bg = np.asarray(bg, f32)
    atlas = np.asarray(atlas, np.uint8).reshape(-1)
    N, _, H, W = bg.shape
    out = np.clip(bg / f32(255), f32(0), f32(1))
    mus, masks = np.zeros((N, 3), f32), np.zeros((N, H, W), f32)
    for n in range(N):
        r = unpack(rows[n])
        level = level_of(atlas, r)
        l, t, rr, b = max(r['win'][0], 0), max(r['win'][1], 0), min(r['win'][2], W), min(r['win'][3], H)
        if level is None or rr <= l or b <= t:
            continue
        P = pixels(level, r, H, W)[t:b, l:rr]
        mu = (P[..., :3].astype(np.float64).sum(axis=(0, 1)) / float(H * W)).astype(f32)
        k = ((r['D'][:, 0] * mu[0] + r['D'][:, 1] * mu[1]) + r['D'][:, 2] * mu[2]) + r['e']
        mask = P[..., 3] / f32(255)
        for c in range(3):
            A = r['A'][c]
            fg = (((A[0] * P[..., 0] + A[1] * P[..., 1]) + A[2] * P[..., 2]) + k[c]) / f32(255)
            v = (bg[n, c, t:b, l:rr] / f32(255)) * (f32(1) - mask) + fg * mask
            assert v.dtype == f32
            out[n, c, t:b, l:rr] = np.fmin(np.fmax(v, f32(0)), f32(1))
        mus[n], masks[n, t:b, l:rr] = mu, mask
    return (out, mus, masks) if return_parts else out


# ---- what tests/test_render_device_host.py and tests/test_gpu_render_device.py share ----------------------------------------
CLASSES = [[15.0 * i, 0.0] for i in range(24)]
SPRITE_SIZES = ((9, 9), (20, 28), (64, 40))              # (h, w)


def synthetic_sprites(seed=0, binary_alpha=False):
    """Three RGBA sprites of SPRITE_SIZES: noise colour, an alpha ramp with a transparent rim (alpha 0 or 255 only with
    binary_alpha)."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in SPRITE_SIZES:
        s = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if binary_alpha:
            s[..., 3] = np.where(s[..., 3] > 90, 255, 0)
        s[0], s[-1], s[:, 0], s[:, -1] = 0, 0, 0, 0
        out.append(s)
    return out


def pack_atlas(sprites, mip_chain):
    """-> (atlas bytes, table[s] = [(offset, h, w) per level]) with the mip chain function under test."""
    chunks, table, off = [], [], 0
    for s in sprites:
        rows = []
        for lv in mip_chain(s):
            rows.append((off, lv.shape[0], lv.shape[1]))
            chunks.append(lv.reshape(-1))
            off += lv.size
        table.append(rows)
    return np.concatenate(chunks), table


def placement(level_hw, level, scale, deg, cx, cy):
    """The inverse affine (a0..a5, float64) of a sprite whose LEVEL `level` is (h, w) = level_hw, drawn at `scale` (of level 0),
    rotated by deg about its centre, the centre put at the continuous canvas point (cx, cy): output pixel index -> level pixel
    index, half-pixel centres on both sides."""
    import math
    h, w = level_hw
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    k = 1.0 / (scale * 2 ** level)                                             # canvas px -> level px
    lin = np.array([[c * k, s * k], [-s * k, c * k]])
    # level continuous = lin @ ((j + 0.5, i + 0.5) - (cx, cy)) + (w / 2, h / 2);  index = continuous - 0.5
    off = lin @ np.array([0.5 - cx, 0.5 - cy]) + np.array([w / 2.0 - 0.5, h / 2.0 - 0.5])
    return np.array([lin[0, 0], lin[0, 1], off[0], lin[1, 0], lin[1, 1], off[1]])


def window(a, level_hw, H, W, slack=1.01):
    """The conservative window of an inverse affine: samples are non-zero only for level indices in (-1, w) x (-1, h); their
    pre-image's bound, rounded outwards, plus `slack` (1 px of blur, 0.01 for float32), clipped to the canvas."""
    import math
    h, w = level_hw
    M = np.array([[a[0], a[1], a[2]], [a[3], a[4], a[5]], [0.0, 0.0, 1.0]])
    F = np.linalg.inv(M)
    xs, ys = np.float64([-1, w, w, -1]), np.float64([-1, -1, h, h])
    px, py = F[0, 0] * xs + F[0, 1] * ys + F[0, 2], F[1, 0] * xs + F[1, 1] * ys + F[1, 2]
    win = [math.floor(px.min() - slack), math.floor(py.min() - slack), math.ceil(px.max() + slack) + 1, math.ceil(py.max() + slack) + 1]
    return [min(max(win[0], 0), W), min(max(win[1], 0), H), min(max(win[2], 0), W), min(max(win[3], 0), H)]


def write_sprite_dir(root, seed=0, size=(120, 200), opaque_white=False):
    """A sprite directory in RenderCar's layout (<mode>/<cad>/...azi<1/100 deg>_ele<1/100 deg>.png): opaque rectangles on
    transparent canvases, as tests/test_render.py builds them (opaque_white: wholly opaque white sprites)."""
    import os
    from PIL import Image
    k = 0
    for mode in ('train', 'valid'):
        for cad in ('cadA', 'cadB'):
            d = os.path.join(root, mode, cad)
            os.makedirs(d)
            for azi in (0, 4500, 9000, 27000):
                if opaque_white:                                            # (the whole canvas: no transparent margin)
                    im = Image.new('RGBA', (size[1], size[0]), (255, 255, 255, 255))
                else:
                    im = Image.new('RGBA', (size[1], size[0]), (0, 0, 0, 0))
                    im.paste((40 + 20 * k, 200 - 10 * k, 90, 255), (size[1] * 3 // 20, size[0] * 5 // 24, size[1] * 17 // 20, size[0] * 19 // 24))
                im.save(os.path.join(d, 'car%d_azi%d_ele1000.png' % (k, azi)))
                k += 1


def write_pascal_dir(root, seed=5):
    """A PASCAL3D+-shaped set (opaque 'photographs', one annotated car box each, one image with two cars that is skipped;
    .mat annotations nested as render_car.py:440-458 indexes them), as tests/test_render.py builds it."""
    import os
    import scipy.io as sio
    from PIL import Image
    os.makedirs(os.path.join(root, 'car_imagenet_label'))
    rng = np.random.default_rng(seed)
    k = 0
    for mode in ('train', 'valid'):
        d = os.path.join(root, 'car_imagenet_' + mode)
        os.makedirs(d)
        for j in range(4):
            name = 'n0%d_%d' % (k, j)
            w, h = int(rng.integers(180, 260)), int(rng.integers(120, 200))
            Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, name + '.png'))
            nobj = 2 if (mode == 'train' and j == 3) else 1
            objs = np.zeros((1, nobj), dtype=[('class', 'O'), ('bbox', 'O'), ('anchors', 'O'), ('viewpoint', 'O')])
            for o in range(nobj):
                l, t = int(rng.integers(5, 40)), int(rng.integers(5, 30))
                view = np.zeros((1, 1), dtype=[('azimuth_coarse', 'O'), ('elevation_coarse', 'O'), ('azimuth', 'O'), ('elevation', 'O')])
                view[0, 0] = (np.array([[0.0]]), np.array([[0.0]]), np.array([[float(rng.uniform(0, 360))]]), np.array([[float(rng.uniform(-10, 30))]]))
                objs[0, o] = ('car', np.array([[l, t, w - int(rng.integers(5, 40)), h - int(rng.integers(5, 30))]], np.float64), np.zeros((1, 1)), view)
            rec = np.zeros((1, 1), dtype=[('filename', 'O'), ('objects', 'O')])
            rec[0, 0] = (name + '.png', objs)
            sio.savemat(os.path.join(root, 'car_imagenet_label', name + '.mat'), {'record': rec})
            k += 1
