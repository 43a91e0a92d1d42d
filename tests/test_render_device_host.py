"""CPU checks of the device renderer's host side (yolo_amd/render.py: SpriteAtlas, ColorAugmenter.affine, draw_params) and of
its C ABI entries (declared, bound, revision still 5, bad arguments refused without a GPU); the numpy restatement
(tests/render_ref.py) against the PIL path pins the geometry conventions."""
import ctypes as C
import itertools
import math
import os
import random
import re

import numpy as np
import pytest

import render_ref as rr
from yolo_amd import lib as L
from yolo_amd import render

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = ('yolo_render_workspace_bytes', 'yolo_render_stats', 'yolo_render_cars')


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_render_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    assert int(re.search(r'#define YOLO_RENDER_ROW_WORDS (\d+)', h).group(1)) == render.ROW_WORDS == rr.ROW_WORDS
    for name, nargs in zip(NAMES, (3, 8, 10)):
        assert name in L.SIGNATURES
        proto = re.search(r'%s\(([^)]*)\)' % name, h).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs


def test_render_entries_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.yolo_render_workspace_bytes(4, 32, 48) > 0
    assert lib.yolo_render_workspace_bytes(64, 416, 416) == 16 * lib.yolo_render_workspace_bytes(4, 416, 416)
    for bad in ((0, 32, 48), (4, 0, 48), (4, 32, -1)):
        assert lib.yolo_render_workspace_bytes(*bad) == L.EINVAL
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    #        atlas bytes rows work N  H   W   stream
    stats = [p,    1024, p,   p,   2, 32, 48, None]
    #       bg atlas bytes rows work out N  H   W   stream
    cars = [p, p,    1024, p,   p,   p,  2, 32, 48, None]
    for fn, ok, ptrs, sizes in ((lib.yolo_render_stats, stats, (0, 2, 3), (1, 4, 5, 6)),
                                (lib.yolo_render_cars, cars, (0, 1, 3, 4, 5), (2, 6, 7, 8))):
        for k in ptrs:                                                      # a NULL pointer
            a = list(ok); a[k] = None
            assert fn(*a) == L.EINVAL, k
        for k in sizes:                                                     # a non-positive atlas size, N, H, W
            for v in (0, -3):
                a = list(ok); a[k] = v
                assert fn(*a) == L.EINVAL, (k, v)
        a = list(ok); a[sizes[2]], a[sizes[3]] = 2 ** 31 - 1, 8             # H * ceil(W / 4) leaves 32 bits
        assert fn(*a) == L.EUNSUPPORTED
        a = list(ok); a[ptrs[1]] = C.c_void_p(4098)                         # (a misaligned atlas / rows pointer)
        assert fn(*a) == L.EINVAL


def test_render_names_are_exported_lazily():
    import yolo_amd
    assert yolo_amd.RenderCar is render.RenderCar and yolo_amd.SpriteAtlas is render.SpriteAtlas
    assert callable(render.RenderCar.draw_params) and callable(render.RenderCar.render_device)


# ---- colour ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', list(itertools.permutations(range(3))), ids=lambda o: ''.join('bcs'[k] for k in o))
def test_colour_chain_composes_into_one_affine_map(order, monkeypatch):
    """A x + D mean(x) + e against ColorAugmenter()(x) for 20 seeds in each of the six stage orders (random.shuffle is
    replaced by the permutation, for both).  rtol 1e-5 of 255: the composition is exact algebra, the difference is the
    float32 rounding of five sequential stages."""
    def shuffle(ts):
        ts[:] = [ts[k] for k in order]
    monkeypatch.setattr(random, 'shuffle', shuffle)
    aug = render.ColorAugmenter()
    worst = 0.0
    for seed in range(20):
        x = (np.random.default_rng(seed).random((16, 24, 3)) * 255).astype(np.float32)
        random.seed(seed); np.random.seed(seed)
        want = aug(x)
        state = (random.getstate(), np.random.get_state()[1][:4].tolist())
        random.seed(seed); np.random.seed(seed)
        A, D, e = aug.affine()
        assert (random.getstate(), np.random.get_state()[1][:4].tolist()) == state          # the same draws were made
        x64 = x.astype(np.float64)
        got = x64 @ A.T + D @ x64.mean(axis=(0, 1)) + e
        worst = max(worst, float(np.abs(got - want).max()))
        assert A.dtype == np.float64 and np.abs(D).max() > 0
    print('order %s: max |A x + D mean + e - ColorAugmenter(x)| = %.3g' % (order, worst))
    assert worst <= 1e-5 * 255, worst


# ---- the same draws as render_host -----------------------------------------------------------------------------------------
def _label_columns(lab):
    return lab[:, 0, 0], lab[:, 0, 5], lab[:, 0, 6:]


def _fixed_cost_randint(monkeypatch):
    """np.random.randint draws by rejection: how many raw values it takes depends on the RANGE (a width of 128 takes one, a
    width of 130 takes one with probability 130/256, then another, ...).  The analytic box is a pixel or two tighter than
    PIL's, so the two paths' paste ranges differ by a few values, and in a batch the streams part for good at the first
    paste draw that rejects in one and not in the other.  For a test of the ORDER of the draws over a whole batch the integer
    draws of both paths are made from one uniform double each, whatever the range."""
    def randint(low, high=None):
        if high is None:
            low, high = 0, low
        return int(low) + int(np.random.random_sample() * (int(high) - int(low)))
    monkeypatch.setattr(np.random, 'randint', randint)


@pytest.mark.parametrize('pascal_rate', [0.0, 1.0, 0.5])
def test_draw_params_makes_render_hosts_draws(tmp_path, pascal_rate, monkeypatch):
    """One seed: draw_params and render_host (augment=False) pick the same sprites, angles and classes -- identical class,
    rotation and distribution columns, the same no-object rows -- on the PNG set and on a PASCAL3D+ set.  (The box columns
    differ by design on the PNG branch: analytic against PIL's getbbox.)  With PASCAL3D+ crops only, the boxes and with them
    the paste ranges are the same numbers, and the two paths leave numpy's generator in the same state; with PNG sprites in
    the batch see _fixed_cost_randint."""
    rr.write_sprite_dir(str(tmp_path / 'png'))
    rr.write_pascal_dir(str(tmp_path / 'pascal'))
    rc = render.RenderCar(160, 256, rr.CLASSES, str(tmp_path / 'png'), augment=False, pascal_root=str(tmp_path / 'pascal'))
    if pascal_rate != 1.0:
        _fixed_cost_randint(monkeypatch)
    np.random.seed(21); random.seed(21)
    _, _, lab_h = rc.render_host(24, 'train', pascal_rate=pascal_rate, render_rate=0.8)
    after_host = np.random.get_state()[1][:8].tolist()
    np.random.seed(21); random.seed(21)
    lab_d, rows = rc.draw_params(24, 'train', pascal_rate=pascal_rate, render_rate=0.8)
    none = lab_h[:, 0, 0] < 0
    assert 2 <= none.sum() <= 12 and np.array_equal(none, lab_d[:, 0, 0] < 0) and np.array_equal(rows[:, 0] == 0, none)
    assert (lab_d[none] == -1).all()
    for a, b in zip(_label_columns(lab_h), _label_columns(lab_d)):
        assert np.array_equal(a, b)
    assert len(set(lab_d[~none, 0, 5].tolist())) >= (8 if pascal_rate == 0.0 else 1)          # (angles were drawn at all)
    assert np.random.get_state()[1][:8].tolist() == after_host
    if pascal_rate == 1.0:
        np.testing.assert_allclose(lab_d, lab_h, rtol=0, atol=1e-9)
    else:
        # the boxes: PIL's is the analytic one plus its transparent rim, so centre and size agree to a few pixels
        d = np.abs(lab_d[~none, 0, 1:5] - lab_h[~none, 0, 1:5]) * np.float32([160, 256, 160, 256])
        assert d.max() <= 6.0, d.max()
    assert rows.shape == (24, render.ROW_WORDS) and rows.dtype == np.int32


def test_draw_params_with_numpys_own_integer_draws(tmp_path):
    """The unpatched generator, one image per seed (nothing follows the paste draws): sprite, angle, class and distribution
    are render_host's for every seed, and so is 'no object'."""
    rr.write_sprite_dir(str(tmp_path))
    rc = render.RenderCar(160, 256, rr.CLASSES, str(tmp_path), augment=False)
    seen = set()
    for seed in range(40):
        np.random.seed(seed); random.seed(seed)
        _, _, lab_h = rc.render_host(1, 'valid', render_rate=0.8)
        np.random.seed(seed); random.seed(seed)
        lab_d, rows = rc.draw_params(1, 'valid', render_rate=0.8)
        for a, b in zip(_label_columns(lab_h), _label_columns(lab_d)):
            assert np.array_equal(a, b)
        assert (rows[0, 0] == 0) == (lab_h[0, 0, 0] < 0)
        seen.add(float(lab_h[0, 0, 0]))
    assert -1.0 in seen and len(seen) >= 4


def test_pascal_boxes_equal_render_pascals(tmp_path):
    rr.write_sprite_dir(str(tmp_path / 'png'))
    rr.write_pascal_dir(str(tmp_path / 'pascal'))
    rc = render.RenderCar(160, 256, rr.CLASSES, str(tmp_path / 'png'), augment=False, pascal_root=str(tmp_path / 'pascal'))
    for seed in range(40):
        r1 = 0.9 + 0.005 * seed
        np.random.seed(seed)
        want = rc._render_pascal('valid', r1)
        np.random.seed(seed)
        got = rc._draw_pascal('valid', r1)
        np.testing.assert_allclose(got[3:7], want[1:5], rtol=0, atol=1e-9)
        assert got[7] == want[5] and got[8] == want[6] and np.array_equal(got[9], want[7])


# ---- analytic boxes --------------------------------------------------------------------------------------------------------
def _shape_sprites(root):
    """Three shapes (rectangle, ellipse, triangle) at six sizes, opaque colour on a transparent canvas."""
    from PIL import Image, ImageDraw
    d = os.path.join(root, 'train', 'cad')
    os.makedirs(d)
    os.makedirs(os.path.join(root, 'valid', 'cad'))
    k = 0
    for w, h in ((60, 40), (90, 70), (128, 96), (200, 120), (240, 200), (300, 180)):
        for shape in ('rect', 'ellipse', 'triangle'):
            im = Image.new('RGBA', (w, h), (0, 0, 0, 0))
            dr = ImageDraw.Draw(im)
            box = (w // 6, h // 5, w - w // 7, h - h // 6)
            colour = (250 - 9 * k, 30 + 11 * k, 120, 255)
            if shape == 'rect':
                dr.rectangle(box, fill=colour)
            elif shape == 'ellipse':
                dr.ellipse(box, fill=colour)
            else:
                dr.polygon([(box[0], box[3]), (box[2], box[3] - h // 4), (w // 2, box[1])], fill=colour)
            im.save(os.path.join(d, 'car%d_azi%d_ele500.png' % (k, 1500 * k)))
            k += 1


def test_analytic_box_lies_inside_pils_by_at_most_three_pixels(tmp_path):
    """300 seeded draws (scale 0.2-1, +-30 degrees, blur <= 0.3): every edge of the box _render_png takes from PIL's getbbox
    lies OUTSIDE the analytic one, by at most 3 px -- the transparent rim bilinear resize, rotation and blur leave -- and
    never inside."""
    _shape_sprites(str(tmp_path))
    rc = render.RenderCar(416, 416, rr.CLASSES, str(tmp_path), augment=False)
    lo, hi = 1e9, -1e9
    for seed in range(300):
        r1 = 0.9 + 0.2 * ((seed * 7) % 11) / 10.0
        np.random.seed(seed)
        pil = rc._render_png('train', r1)
        np.random.seed(seed)
        got = rc._draw_png('train', r1)
        assert got[7] == pil[5] and got[8] == pil[6]
        l, t, r, b = got[3:7]
        out = (l - pil[1], t - pil[2], pil[3] - r, pil[4] - b)                # how far PIL's edge lies outside ours
        lo, hi = min(lo, min(out)), max(hi, max(out))
        assert min(out) >= 0 and max(out) <= 3, (seed, out)
    print('PIL box outside the analytic box by %.3f .. %.3f px over 300 draws' % (lo, hi))


def test_pixel_hull_and_convex_hull():
    s = np.zeros((10, 12, 4), np.uint8)
    s[2:5, 3:9, 3] = 255
    s[7, 1, 0] = 9                                                            # colour without alpha counts (any band)
    hull = render.pixel_hull(s)
    assert hull[:, 0].min() == 1 and hull[:, 0].max() == 9 and hull[:, 1].min() == 2 and hull[:, 1].max() == 8
    assert {tuple(p) for p in hull.tolist()} == {(3., 2.), (9., 2.), (9., 5.), (2., 8.), (1., 8.), (1., 7.)}
    assert np.array_equal(render.pixel_hull(np.zeros((4, 6, 4), np.uint8)), np.float64([[0, 0], [6, 0], [6, 4], [0, 4]]))
    sq = render.convex_hull([(0, 0), (2, 0), (2, 2), (0, 2), (1, 1), (1, 0)])
    assert {tuple(p) for p in sq.tolist()} == {(0., 0.), (2., 0.), (2., 2.), (0., 2.)}


# ---- atlas -----------------------------------------------------------------------------------------------------------------
def test_mip_levels_tile_the_atlas_and_the_residual_scale_stays_in_half_to_one():
    rng = np.random.default_rng(1)
    sprites = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for h, w in ((256, 320), (9, 9), (20, 28), (64, 40), (131, 257))]
    atlas = render.SpriteAtlas(sprites)
    assert [len(t) for t in atlas.table] == [6, 1, 2, 3, 5]                   # shorter side 256 -> 8, 9, 20 -> 10, 40 -> 10, 131 -> 8
    off = 0
    for s, levels in enumerate(atlas.table):
        h, w = sprites[s].shape[:2]
        for k, (o, lh, lw) in enumerate(levels):
            assert (o, lh, lw) == (off, h >> k, w >> k) and min(lh, lw) >= 8 and o % 4 == 0
            off += 4 * lh * lw
        assert min(levels[-1][1:]) // 2 < 8
    assert off == atlas.data.size and atlas.data.dtype == np.uint8
    # a level is the rounded 2x2 average of the one before
    o, lh, lw = atlas.table[4][1]
    a = sprites[4][:130, :256].astype(np.int64)
    want = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) // 4
    assert np.array_equal(atlas.data[o:o + 4 * lh * lw].reshape(lh, lw, 4), want)
    for scale in np.concatenate([np.linspace(0.05, 1.0, 96), [0.5, 0.25, 0.125, 0.0625, 0.2]]):
        level, resid = atlas.pick_level(0, float(scale))
        assert 0.5 < resid <= 1.0 and resid == scale * 2 ** level, (scale, level, resid)
    assert atlas.pick_level(1, 0.2) == (0, 0.2)                               # a sprite without the level: its coarsest
    assert atlas.pick_level(0, 1.7) == (0, 1.7)                               # a magnification: level 0


def test_the_drawn_level_keeps_both_axes_residual_scales(tmp_path):
    """What a draw really scales by is the integer resized size over the sprite's, per axis (the r1 aspect factor and int() move it
    off the drawn number): the level is picked from the SMALLER axis, so that one's residual stays in (0.5, 1] and the other's
    is at most 1.1 / 0.9 of it, plus the int() step."""
    _shape_sprites(str(tmp_path))
    rc = render.RenderCar(416, 416, rr.CLASSES, str(tmp_path), augment=False, R=0, G=0)
    atlas, seen = rc.atlas(), set()
    for seed in range(200):
        np.random.seed(seed)
        s, scale, to_sprite = rc._draw_png('train', 0.9 + 0.2 * (seed % 11) / 10.0)[:3]
        level, resid = atlas.pick_level(s, scale)
        axes = (2 ** level / to_sprite[0, 0], 2 ** level / to_sprite[1, 1])
        assert abs(min(axes) - resid) < 1e-12
        if level + 1 < len(atlas.table[s]) or resid > 0.5:                   # (not a sprite whose coarsest level is too fine)
            assert 0.5 < min(axes) <= 1.0 and max(axes) <= min(axes) * 1.1 / 0.9 * 1.05, (seed, axes)
        seen.add(level)
    assert seen >= {0, 1, 2}


def test_blur_weights():
    assert render.blur_weights(0.0) == (1.0, 0.0) and render.blur_weights(0.0499) == (1.0, 0.0)
    for sigma in (0.05, 0.1, 0.3, 1.0):
        w0, w1 = render.blur_weights(sigma)
        assert abs(w0 + 2 * w1 - 1) < 1e-15 and abs(w1 / w0 - math.exp(-1 / (2 * sigma * sigma))) < 1e-15


# ---- the restatement against the PIL path ----------------------------------------------------------------------------------
# measured here: mean |restated - PIL composite| = 0.00041 of the 0..1 range without rotation, 0.00058 with (NOTES.md); PIL
# resizes with an antialiasing triangle filter and replicates the edge pixel where the restatement fades to zero, the
# restatement taps a 2x2-averaged mip level: edge pixels differ, interiors agree.  The bars sit just above the measurements.
RESTATEMENT_MAD_BAR = {0: 0.0005, 30.0: 0.0007}


@pytest.mark.parametrize('R', [0, 30.0])
def test_restatement_against_the_pil_path(tmp_path, monkeypatch, R):
    """R = 0 (and, beyond what the conventions need, the rotation of R = 30), G = 0, augment=False, one seed for both: the restated image (rows from draw_params, pixels from
    tests/render_ref.py) against render_host's composite.  Pins the geometry conventions -- half-pixel centres, PIL's integer
    resize size, the paste offset --, not PIL's antialiased pixels."""
    rr.write_sprite_dir(str(tmp_path))
    H, W = 160, 256
    rc = render.RenderCar(H, W, rr.CLASSES, str(tmp_path), augment=False, R=R, G=0)
    bg = (np.random.default_rng(1).random((8, 3, H, W)) * 255).astype(np.float32)
    calls, randint = [], np.random.randint
    monkeypatch.setattr(np.random, 'randint', lambda *a, **k: calls.append((a, k)) or randint(*a, **k))
    np.random.seed(5)
    fg, mask, lab_h = rc.render_host(8, 'train')
    want = np.clip(bg / np.float32(255.) * (1 - mask) + fg * mask, 0, 1)
    # the same sprites at the same paste offsets: the analytic box's paste RANGE is a pixel or two off PIL's, which would move
    # the draw, so draw_params' integer draws are made with render_host's ranges (from the same generator state)
    replay = iter(calls)
    monkeypatch.setattr(np.random, 'randint', lambda *a, **k: (lambda c: randint(*c[0], **c[1]))(next(replay)))
    np.random.seed(5)
    lab_d, rows = rc.draw_params(8, 'train')
    monkeypatch.setattr(np.random, 'randint', randint)
    got, _, got_mask = rr.render(bg, rc.atlas().data, rows, return_parts=True)
    mad = float(np.abs(got.astype(np.float64) - want).mean())
    print('mean |restated - PIL composite| = %.5f' % mad)
    assert mad <= RESTATEMENT_MAD_BAR[R], mad
    ii, jj = np.mgrid[0:H, 0:W]
    for n in range(8):
        m_pil, m_got = mask[n, 0].astype(np.float64), got_mask[n].astype(np.float64)
        c_pil = ((m_pil * jj).sum() / m_pil.sum(), (m_pil * ii).sum() / m_pil.sum())
        c_got = ((m_got * jj).sum() / m_got.sum(), (m_got * ii).sum() / m_got.sum())
        print('image %d: mask centroid PIL (%.3f, %.3f) restated (%.3f, %.3f)' % ((n,) + c_pil + c_got))
        assert abs(c_pil[0] - c_got[0]) <= 1 and abs(c_pil[1] - c_got[1]) <= 1
        assert abs(m_pil.sum() - m_got.sum()) <= 0.05 * m_pil.sum()
