"""CPU checks of the device plate renderer's host side (yolo_amd/render.py: LPGenerator.glyph_atlas, draw_params) and of its C
ABI entries (declared, bound, revision still 5, bad arguments refused without a GPU); Philox4x32-10 and the noise field of the
numpy restatement (tests/plate_ref.py); the restatement against the PIL path pins the geometry conventions."""
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest

import plate_ref as pr
from yolo_amd import lib as L
from yolo_amd import render

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = ('yolo_plate_workspace_bytes', 'yolo_plate_compose', 'yolo_plate_stats', 'yolo_plate_render')
R_MAX = [45, 60, 45]


@pytest.fixture(scope='module')
def gen(tmp_path_factory):
    root = tmp_path_factory.mktemp('plates') / 'fonts'
    pr.write_fonts(str(root))
    return render.LPGenerator(96, 160, str(root), pr.CAMERA, augment=False)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_plate_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    assert int(re.search(r'#define YOLO_PLATE_ROW_WORDS (\d+)', h).group(1)) == render.PLATE_ROW_WORDS == pr.ROW_WORDS == 48
    assert int(re.search(r'#define YOLO_PLATE_GLYPH_BYTES (\d+)', h).group(1)) == render.PLATE_GLYPH_BYTES == pr.GLYPH_BYTES == 553600
    for name, nargs in zip(NAMES, (3, 5, 7, 9)):
        assert name in L.SIGNATURES
        proto = re.search(r'%s\(([^)]*)\)' % name, h).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs
    assert sorted(n for n in L.SIGNATURES if n.startswith('yolo_plate_')) == sorted(NAMES)


def test_plate_entries_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.yolo_plate_workspace_bytes(4, 32, 48) > 0
    assert lib.yolo_plate_workspace_bytes(64, 416, 416) == 16 * lib.yolo_plate_workspace_bytes(4, 416, 416)
    for bad in ((0, 32, 48), (4, 0, 48), (4, 32, -1)):
        assert lib.yolo_plate_workspace_bytes(*bad) == L.EINVAL
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    #          glyphs rows plates N  stream
    compose = [p,     p,   p,     2, None]
    #        plates rows work N  H   W   stream
    stats = [p,     p,   p,   2, 32, 48, None]
    #         bg plates rows work out N  H   W   stream
    rend = [p, p,     p,   p,   p,  2, 32, 48, None]
    for fn, ok, ptrs, sizes in ((lib.yolo_plate_compose, compose, (0, 1, 2), (3,)), (lib.yolo_plate_stats, stats, (0, 1, 2), (3, 4, 5)),
                                (lib.yolo_plate_render, rend, (0, 1, 2, 3, 4), (5, 6, 7))):
        for k in ptrs:
            a = list(ok); a[k] = None                                           # a NULL pointer
            assert fn(*a) == L.EINVAL, k
            a = list(ok); a[k] = C.c_void_p(4098)                               # a misaligned pointer
            assert fn(*a) == L.EINVAL, k
        for k in sizes:                                                         # a non-positive N, H, W
            for v in (0, -3):
                a = list(ok); a[k] = v
                assert fn(*a) == L.EINVAL, (k, v)
        if len(sizes) == 3:
            a = list(ok); a[sizes[1]], a[sizes[2]] = 2 ** 31 - 1, 8             # H * ceil(W / 4) leaves 32 bits
            assert fn(*a) == L.EUNSUPPORTED
    a = list(stats); a[1] = C.c_void_p(4100)                                    # rows are 8-byte aligned
    assert lib.yolo_plate_stats(*a) == L.EINVAL


def test_plate_names_are_exported_lazily():
    import yolo_amd
    assert yolo_amd.LPGenerator is render.LPGenerator
    assert callable(render.LPGenerator.draw_params) and callable(render.LPGenerator.add_device) and callable(render.LPGenerator.glyph_atlas)


# ---- Philox and the noise ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counter, key, want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_known_answers(counter, key, want):
    """The published Random123 known-answer vectors of Philox4x32-10."""
    got = pr.philox4x32_10([np.uint32(c) for c in counter], key)
    assert tuple(int(v) for v in got) == want
    many = pr.philox4x32_10([np.full((3, 5), c, np.uint32) for c in counter], key)          # and as arrays
    assert all((m == w).all() for m, w in zip(many, want))


def test_noise_field_of_the_restatement():
    """64 x 96 x 4 values with the scale for sigma = 1: n = 24576, so the mean's standard error is 1/sqrt(n) = 0.0064 (0.03 is
    4.7 of them) and the variance's relative standard error sqrt(2/n) = 0.9 % (5 % is 5.5 of them)."""
    s = pr.noise_scale(1.0)
    a = pr.noise_z((123, 456), 64, 96) * s
    assert a.dtype == np.float32 and a.shape == (64, 96, 4)
    mean, var = float(a.astype(np.float64).mean()), float(a.astype(np.float64).var())
    print('noise field: mean %.4f variance %.4f' % (mean, var))
    assert abs(mean) <= 0.03
    assert abs(var - 1.0) <= 0.05
    z = pr.noise_z((123, 456), 64, 96)
    assert np.array_equal(z, np.round(z)) and z.min() >= -1020 and z.max() <= 1020
    assert np.array_equal(z, pr.noise_z((123, 456), 64, 96))
    assert not np.array_equal(z, pr.noise_z((123, 457), 64, 96)) and not np.array_equal(z, pr.noise_z((124, 456), 64, 96))
    assert abs(float(render.PLATE_NOISE_UNIT) - pr.NOISE_UNIT) == 0


# ---- draw_params -------------------------------------------------------------------------------------------------------------
def test_glyph_atlas_is_the_generators_images(gen):
    data = gen.glyph_atlas()
    assert data.dtype == np.uint8 and data.shape == (pr.GLYPH_BYTES,) and gen.glyph_atlas() is data
    glyph, dot = pr.split_atlas(data)
    assert all(np.array_equal(glyph[k], np.asarray(gen.glyph[k])) for k in range(34)) and np.array_equal(dot, np.asarray(gen.dot))
    soft = (data.reshape(-1, 4)[:, 3] > 0) & (data.reshape(-1, 4)[:, 3] < 255)
    assert soft.mean() > 0.1                                                    # (soft alpha: the four-byte paste is exercised)


def test_draw_params_first_plate_is_add_hosts(gen):
    for seed in range(6):
        np.random.seed(seed); random.seed(seed)
        _, _, lab_h = gen.add_host(1, 96, 160, R_MAX, add_rate=0.8)
        np.random.seed(seed); random.seed(seed)
        if np.random.rand() <= 0.8:
            ids_h = [g[0] for g in gen.draw_LP()[2]]
        np.random.seed(seed); random.seed(seed)
        lab_d, rows = gen.draw_params(3, 96, 160, R_MAX, add_rate=0.8)
        assert np.array_equal(lab_d[0], lab_h[0])
        assert (rows[0, 0] == 1) == (lab_h[0, 0, 0] > 0)
        if rows[0, 0]:
            assert rows[0, 1:8].tolist() == ids_h
    assert rows.shape == (3, 48) and rows.dtype == np.int32 and lab_d.shape == (3, 1, 10) and lab_d.dtype == np.float32


def test_draw_params_rows_labels_and_ranges(tmp_path):
    pr.write_fonts(str(tmp_path / 'fonts'))
    g = render.LPGenerator(96, 160, str(tmp_path / 'fonts'), pr.CAMERA)           # the colour augmenter on
    np.random.seed(3); random.seed(3)
    lab, rows = g.draw_params(24, 96, 160, R_MAX, add_rate=0.8)
    has = rows[:, 0] == 1
    assert 12 <= has.sum() < 24 and np.array_equal(has, lab[:, 0, 0] == 1) and (lab[~has] == -1).all() and (rows[~has] == 0).all()
    keys = set()
    for row, l in zip(rows[has], lab[has, 0]):
        r = pr.unpack(row)
        assert all(10 <= v <= 33 for v in r['ids'][:3]) and all(0 <= v <= 9 and v != 4 for v in r['ids'][3:])
        # the map carries the label's centre to the plate's centre: float32 entries on coordinates below 640 leave ~1e-4
        m = r['m'].astype(np.float64).reshape(3, 3)
        p = m @ np.array([l[7] - 0.5, l[8] - 0.5, 1.0])
        assert p[2] > 0 and abs(p[0] / p[2] - 189.5) <= 0.01 and abs(p[1] / p[2] - 79.5) <= 0.01, p
        assert 1500 <= l[3] <= 5000 and abs(l[1]) <= l[3] * 0.3 + 1e-3 and abs(l[2]) <= l[3] * 7 / 30. + 1e-3
        assert abs(l[4]) <= np.radians(45) + 1e-6 and abs(l[5]) <= np.radians(60) + 1e-6 and abs(l[6]) <= np.radians(45) + 1e-6 and l[9] == 0
        assert -1 <= l[7] <= 161 and -1 <= l[8] <= 97
        assert r['s'] == np.float32(5.0 / math.sqrt(8 * 65535 / 12.0)) and abs(float(r['w0']) + 2 * float(r['w1']) - 1) < 1e-6
        l_, t_, r_, b_ = r['win']
        assert 0 <= l_ <= r_ <= 160 and 0 <= t_ <= b_ <= 96
        assert np.abs(r['D']).max() > 0
        keys.add(r['key'])
    assert len(keys) == has.sum()
    # augment=False: the identity colour map
    g2 = render.LPGenerator(96, 160, str(tmp_path / 'fonts'), pr.CAMERA, augment=False)
    np.random.seed(3); random.seed(3)
    _, rows2 = g2.draw_params(4, 96, 160, R_MAX)
    r = pr.unpack(rows2[0])
    assert (rows2[:, 0] == 1).all() and np.array_equal(r['A'], np.eye(3, dtype=np.float32)) and not r['D'].any() and not r['e'].any()
    lab0, rows0 = g.draw_params(5, 96, 160, R_MAX, add_rate=0)
    assert (lab0 == -1).all() and (rows0[:, 0] == 0).all()


def test_the_window_holds_every_pixel_the_plate_touches(gen):
    """Over 40 seeded poses: the restated mask with the row's window equals the one with the whole canvas as the window."""
    np.random.seed(11); random.seed(11)
    _, rows = gen.draw_params(40, 48, 80, R_MAX)
    rows[:, 14] = 0                                                             # (noise off: outside the window Q is 0)
    plates = np.full((40, 160, 380, 4), 255, np.uint8)
    wide = rows.copy()
    wide[:, 8:12] = [0, 0, 80, 48]
    bg = np.zeros((40, 3, 48, 80), np.float32)
    a, b = pr.render(bg, plates, rows, return_parts=True)[2], pr.render(bg, plates, wide, return_parts=True)[2]
    assert np.array_equal(a, b) and (a.reshape(40, -1).max(axis=1) > 0).sum() >= 30


# ---- the restatement against the PIL path ------------------------------------------------------------------------------------
def test_restatement_against_the_pil_path(gen, monkeypatch):
    """One plate at Z = 1500 on a 240 x 320 canvas (about 75 px wide), colour augmenter, noise and blur off, turned about all
    three axes so that no edge runs along a pixel row: the restated mask (row from plate_row, plate from the restated compose)
    against random_projection_LP_6D's.  Pins the conventions -- half-pixel centres on the canvas, in the camera image and on
    the plate --, not PIL's pixels.
    The bounds.  Dropping the canvas' half-pixel centre moves the plate by one camera pixel = 0.5 canvas px (the canvas is the
    640 x 480 camera image halved), so the centroid bar is HALF of that, 0.25 px per axis.  The mask is a near-binary indicator
    (the plate is opaque, 5 texels per pixel), which PIL renders by area coverage (its resize antialiases) and the restatement
    by a point sample: per unit of boundary length a point sample misplaces the edge by at most half a pixel, so
    |area difference| <= 0.5 px * perimeter of the projected quad."""
    H, W = 240, 320
    pose = [60.0, -40.0, 1500.0, math.radians(12), math.radians(-18), math.radians(20)]
    # random_projection_LP_6D's draws, made to order: Z, then the three unit draws for X, Y (scaled by Z 9/30, Z 7/30), the angles
    units = [pose[0] / (1500.0 * 9 / 30.), pose[1] / (1500.0 * 7 / 30.)] + [math.degrees(pose[3 + k]) / R_MAX[k] for k in range(3)]
    draws = iter([1500.0] + units)
    monkeypatch.setattr(np.random, 'uniform', lambda low, high: next(draws))
    monkeypatch.setattr(np.random, 'rand', lambda: 0.0)                         # blur radius 0
    monkeypatch.setattr(np.random, 'normal', lambda mu, sd, shape: np.zeros(shape))
    ids = [12, 20, 33, 0, 7, 9, 3]
    row = gen.plate_row(ids, pose, H, W, 0.0, (0, 0), sigma_noise=0.0)
    plates = pr.compose(gen.glyph_atlas(), row[None])
    from PIL import Image
    m_pil, _, label = gen.random_projection_LP_6D(Image.fromarray(plates[0]), (H, W), R_MAX)
    np.testing.assert_allclose(label[1:7], pose, rtol=1e-6)
    m_pil = m_pil[0].astype(np.float64)
    m_got = pr.render(np.zeros((1, 3, H, W), np.float32), plates, row[None], return_parts=True)[2][0].astype(np.float64)
    quad = gen.camera.corners(pose).astype(np.float64) * [W / 640., H / 480.]
    perimeter = float(np.linalg.norm(quad - np.roll(quad, 1, axis=0), axis=1).sum())
    width = float(np.linalg.norm(quad[0] - quad[1]))
    ii, jj = np.mgrid[0:H, 0:W]
    c_pil = ((m_pil * jj).sum() / m_pil.sum(), (m_pil * ii).sum() / m_pil.sum())
    c_got = ((m_got * jj).sum() / m_got.sum(), (m_got * ii).sum() / m_got.sum())
    print('plate %.1f px wide, perimeter %.1f px; mask area PIL %.1f restated %.1f; centroid PIL (%.3f, %.3f) restated (%.3f, %.3f), label (%.3f, %.3f)'
          % (width, perimeter, m_pil.sum(), m_got.sum(), c_pil[0], c_pil[1], c_got[0], c_got[1], label[7] - 0.5, label[8] - 0.5))
    assert 60 <= width <= 90
    assert abs(c_pil[0] - c_got[0]) <= 0.25 and abs(c_pil[1] - c_got[1]) <= 0.25
    assert abs(m_pil.sum() - m_got.sum()) <= 0.5 * perimeter
