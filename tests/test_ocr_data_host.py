"""CPU checks of the OCR data path: the C ABI entries of csrc/ocr_data.hip (declared, bound, revision still 5, bad arguments refused
without a GPU), the restated targets against a literal transcription of loss_mask, LPGenerator.draw_ocr_params against the PIL
route's draws, and the read-back property of the targets."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import ocr_loss_ref as olr
import ocr_render_ref as orr
import plate_ref as pr
from yolo_amd import lib as L
from yolo_amd import render

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = {'yolo_ocr_plate_workspace_bytes': 3, 'yolo_ocr_plate_blur': 8, 'yolo_ocr_plate_render': 9, 'yolo_ocr_targets': 8,
         'yolo_ocr_loss_fwd_bwd': 11, 'yolo_ocr_score': 11}
H, W = 160, 384


@pytest.fixture(scope='module')
def gen(tmp_path_factory):
    root = tmp_path_factory.mktemp('ocr') / 'fonts'
    pr.write_fonts(str(root))
    return render.LPGenerator(H, W, str(root), pr.CAMERA, augment=False)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_ocr_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    assert int(re.search(r'#define YOLO_OCR_TAP_WORDS (\d+)', h).group(1)) == render.OCR_TAP_WORDS == orr.TAP_WORDS == 32
    assert int(re.search(r'#define YOLO_OCR_BLUR_TAPS (\d+)', h).group(1)) == render.OCR_BLUR_TAPS == orr.BLUR_TAPS == 24
    assert int(re.search(r'#define YOLO_OCR_SCORE_WORDS (\d+)', h).group(1)) == 6
    for name, nargs in NAMES.items():
        assert name in L.SIGNATURES
        proto = re.search(r'^(?:int|long long) %s\(([^)]*)\)' % name, h, re.M).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs, name
    assert sorted(n for n in L.SIGNATURES if n.startswith('yolo_ocr_') and n != 'yolo_ocr_decode') == sorted(NAMES)


def _refusals(fn, ok, ptrs, sizes, nullable=()):
    for k in ptrs:
        if k not in nullable:
            a = list(ok); a[k] = None                                           # a NULL pointer
            assert fn(*a) == L.EINVAL, (fn.__name__, k)
        a = list(ok); a[k] = C.c_void_p(4098)                                   # a misaligned pointer
        assert fn(*a) == L.EINVAL, (fn.__name__, k)
    for k in sizes:                                                             # a non-positive size
        for v in (0, -3):
            a = list(ok); a[k] = v
            assert fn(*a) == L.EINVAL, (fn.__name__, k, v)


def test_ocr_entries_refuse_bad_arguments_without_a_gpu(lib):
    """Validation comes before any launch: none of these pointers is ever dereferenced, and no GPU is needed to be refused."""
    assert lib.yolo_version() == 5
    for name in NAMES:
        assert hasattr(lib, name)
    sums, q_off, total, tiles = orr.workspace_layout(4, 160, 384)
    assert lib.yolo_ocr_plate_workspace_bytes(4, 160, 384) == total and tiles == 60 and q_off % 16 == 0
    assert lib.yolo_ocr_plate_workspace_bytes(1, 30, 45) == orr.workspace_layout(1, 30, 45)[2]
    for bad in ((0, 32, 48), (4, 0, 48), (4, 32, -1)):
        assert lib.yolo_ocr_plate_workspace_bytes(*bad) == L.EINVAL
    p = C.c_void_p(4096)
    #       plates rows taps work N  H   W   stream
    blur = [p,     p,   p,   p,   2, 32, 48, None]
    #       bg rows work out N  H   W   unit stream
    rend = [p, p,   p,   p,  2, 32, 48, 0,   None]
    #      labels order score class B  nobj Wp  stream
    targ = [p,    p,    p,    p,    2, 7,   24, None]
    #      logits score class dlogits losses B  Wp  ncls sw   cw   stream
    loss = [p,    p,    p,    p,      p,     2, 24, 34,  0.1, 1.0, None]
    #       codes count labels class logits counts B  nobj Wp  ncls stream
    score = [p,   p,    p,     p,    p,     p,     2, 7,   24, 34,  None]
    _refusals(lib.yolo_ocr_plate_blur, blur, (0, 1, 2, 3), (4, 5, 6))
    _refusals(lib.yolo_ocr_plate_render, rend, (0, 1, 2, 3), (4, 5, 6))
    _refusals(lib.yolo_ocr_targets, targ, (0, 1, 2, 3), (4, 5, 6), nullable=(1,))
    _refusals(lib.yolo_ocr_loss_fwd_bwd, loss, (0, 1, 2, 3, 4), (5, 6, 7), nullable=(3,))
    _refusals(lib.yolo_ocr_score, score, (0, 1, 2, 3, 4, 5), (6, 7, 8, 9))
    a = list(blur); a[1] = C.c_void_p(4100)                                     # rows are 8-byte aligned,
    assert lib.yolo_ocr_plate_blur(*a) == L.EINVAL
    a = list(blur); a[3] = C.c_void_p(4104)                                     # the workspace 16-byte
    assert lib.yolo_ocr_plate_blur(*a) == L.EINVAL
    for fn, ok in ((lib.yolo_ocr_plate_blur, blur), (lib.yolo_ocr_plate_render, rend)):
        a = list(ok); a[5], a[6] = 2 ** 31 - 1, 8                               # H * ceil(W / 4) leaves 32 bits
        assert fn(*a) == L.EUNSUPPORTED
    a = list(targ); a[4], a[6] = 2 ** 16, 2 ** 15                               # B * Wp = 2^31
    assert lib.yolo_ocr_targets(*a) == L.EUNSUPPORTED
    a = list(loss); a[5], a[6], a[7] = 2 ** 12, 2 ** 10, 2 ** 7 - 1             # logits of 2^31 bytes
    assert lib.yolo_ocr_loss_fwd_bwd(*a) == L.EUNSUPPORTED
    for k, v in ((7, 17), (8, 65)):                                             # nobj <= 16, Wp <= 64
        a = list(score); a[k] = v
        assert lib.yolo_ocr_score(*a) == L.EUNSUPPORTED
    a = list(score); a[7], a[8] = 16, 64
    a[6], a[9] = 2 ** 16, 2 ** 9 - 1                                            # logits of 2^31 bytes
    assert lib.yolo_ocr_score(*a) == L.EUNSUPPORTED


def test_ocr_names_are_exported_lazily():
    import yolo_amd
    from yolo_amd import ocr
    assert yolo_amd.OCRValidator is ocr.OCRValidator and yolo_amd.ocr_targets is ocr.ocr_targets and yolo_amd.ocr_loss is ocr.ocr_loss
    assert callable(render.LPGenerator.render) and callable(render.LPGenerator.render_device) and callable(render.LPGenerator.draw_ocr_params)
    with pytest.raises(AttributeError):
        yolo_amd.OCRTrainer


# ---- the targets -------------------------------------------------------------------------------------------------------------
def loss_mask_literal(labels, area, orders):
    """OCR/OCR.py:77-100, loop for loop, on numpy arrays; nd.random.shuffle(label) is the host's draw `orders`."""
    bs = labels.shape[0]
    score_y = np.zeros((bs, 1, area, 1), np.float32)
    class_y = np.ones((bs, 1, area), np.float32) * (-1)
    for b in range(bs):
        label = labels[b][orders[b]]
        for Lb in label:  # all object in the image
            left = int(round(Lb[1] * area))
            right = int(round(Lb[2] * area))
            for i in range(left, right):
                text_cent = (Lb[1] + Lb[2]) / 2.
                box_cent = (i + 0.5) / float(area)
                score = 1 - abs(box_cent - text_cent) / float(Lb[2] - Lb[1])
                score_y[b, 0, i, 0] = score  # others are zero
                class_y[b, 0, i] = Lb[0]
    return score_y, class_y


def inside_labels(rng, B, nobj, Wp):
    """Labels whose columns all fall inside [0, Wp), overlapping now and then, some rows class -1 (left = right = -1, as the
    reference's empty rows are); no L * Wp within 1e-4 of a half-integer (Python 3 and the device round a tie differently)."""
    lab = -np.ones((B, nobj, 3), np.float32)
    for b in range(B):
        for k in range(nobj):
            if rng.random() < 0.2:
                continue
            while True:
                c, wd = rng.uniform(0.05, 0.95), rng.uniform(0.04, 0.3)
                row = np.float32([rng.integers(0, 34), max(c - wd / 2, 0.0), min(c + wd / 2, 1.0)])
                frac = np.abs((row[1:].astype(np.float64) * Wp) % 1.0 - 0.5)
                if frac.min() > 1e-4:
                    break
            lab[b, k] = row
    return lab


@pytest.mark.parametrize('Wp', [24, 25, 1])
def test_restated_targets_equal_the_literal_loss_mask(Wp):
    rng = np.random.default_rng(5 + Wp)
    lab = inside_labels(rng, 9, 7, Wp)
    orders = np.stack([rng.permutation(7) for _ in range(9)]).astype(np.int32)
    score_l, class_l = loss_mask_literal(lab, Wp, orders)
    score_r, class_r = olr.targets(lab, orders, Wp, np.float32)
    assert np.array_equal(class_r, class_l[:, 0].astype(np.int32))
    assert (class_r >= 0).sum() >= min(Wp, 9) and np.abs(score_r - score_l[:, 0, :, 0]).max() <= 2e-6
    assert np.array_equal(score_r > 0, class_r >= 0) or Wp == 1
    # the order matters where labels overlap, and NULL is the given order
    same = olr.targets(lab, None, Wp, np.float32)
    assert np.array_equal(same[1], olr.targets(lab, np.tile(np.arange(7, dtype=np.int32), (9, 1)), Wp, np.float32)[1])
    if Wp > 1:
        assert not np.array_equal(same[1], class_r)


# ---- draw_ocr_params -----------------------------------------------------------------------------------------------------------
def _spy(monkeypatch, gen):
    seen = {'draw': [], 'paste': []}
    draw, paste = gen._ocr_draw, render.LPGenerator._ocr_paste

    def spy_draw(h, w, a):
        seen['draw'].append(draw(h, w, a))
        return seen['draw'][-1]

    def spy_paste(d, h, w):
        seen['paste'].append(paste(d, h, w))
        return seen['paste'][-1]
    monkeypatch.setattr(gen, '_ocr_draw', spy_draw)
    monkeypatch.setattr(gen, '_ocr_paste', spy_paste)
    return seen


def test_draw_ocr_params_is_deterministic_and_its_first_image_is_renders(gen, monkeypatch):
    """render_host draws a field of normals for the noise BEFORE the paste position, draw_ocr_params two key words AFTER it: with
    the normals taken from elsewhere (as tests/test_plate_device_host.py does for the PIL path) the first image of a seeded
    batch has the PIL route's glyphs, sizes, shear, angle, blur radius and paste position, hence its labels."""
    for seed in range(5):
        np.random.seed(seed); random.seed(seed)
        lab, rows, taps, orders = gen.draw_ocr_params(3, H, W)
        np.random.seed(seed); random.seed(seed)
        again = gen.draw_ocr_params(3, H, W)
        assert all(np.array_equal(a, b) for a, b in zip((lab, rows, taps, orders), again))
        seen = _spy(monkeypatch, gen)
        np.random.seed(seed); random.seed(seed)
        gen.draw_ocr_params(1, H, W)
        with monkeypatch.context() as mp:
            mp.setattr(np.random, 'normal', lambda mu, sd, shape: np.zeros(shape))
            np.random.seed(seed); random.seed(seed)
            fg, mask, lab_h = gen.render_host(1, H, W)
        assert seen['draw'][0] == seen['draw'][1] and seen['paste'][0] == seen['paste'][1]
        d = seen['draw'][0]
        assert rows[0, 1:8].tolist() == d['ids'] == lab[0, :, 0].astype(int).tolist()
        assert np.array_equal(lab[0], lab_h[0])
        assert 342 <= d['LP_w'] <= 380 and 129 <= d['LP_h'] <= 176 and abs(d['deg']) <= 5 and abs(d['m']) <= 0.1 and abs(d['n']) <= 0.1
        assert 0 <= d['sigma'] <= 8 and taps[0, 0] == min(int(np.ceil(3 * d['sigma'])), 24)
        assert mask[0].max() == 1.0
    assert lab.shape == (3, 7, 3) and lab.dtype == np.float32 and rows.shape == (3, 48) and rows.dtype == np.int32
    assert taps.shape == (3, 32) and taps.dtype == np.int32 and orders.shape == (3, 7) and orders.dtype == np.int32
    assert all(sorted(o) == list(range(7)) for o in orders.tolist())


def test_the_windows_are_the_paste_rectangles_and_the_taps_are_normalised(gen, monkeypatch):
    """The window of a row against the rectangle PIL's paste covers: the size of the image the PIL stages leave, at the paste
    position, clipped to the canvas."""
    from PIL import Image
    seen = _spy(monkeypatch, gen)
    np.random.seed(21); random.seed(21)
    lab, rows, taps, _ = gen.draw_ocr_params(12, H, W)
    clipped = 0
    for n in range(12):
        d, (px, py) = seen['draw'][n], seen['paste'][n]
        img = Image.new('RGBA', (380, 160)).resize((d['LP_w'], d['LP_h']), Image.BILINEAR)
        xs, ys = abs(d['m']) * d['LP_h'], abs(d['n']) * d['LP_w']
        img = img.transform((d['LP_w'] + int(round(xs)), d['LP_h'] + int(round(ys))), Image.AFFINE, (1, d['m'], 0, d['n'], 1, 0), Image.BILINEAR)
        img = img.rotate(d['deg'], Image.BILINEAR, expand=1)
        want = [min(max(px, 0), W), min(max(py, 0), H), min(max(px + img.size[0], 0), W), min(max(py + img.size[1], 0), H)]
        assert rows[n, 8:12].tolist() == want, n
        clipped += want != [px, py, px + img.size[0], py + img.size[1]]
        r = pr.unpack(rows[n])
        assert r['m'][6] == 0 and r['m'][7] == 0 and r['m'][8] == 1 and r['s'] == np.float32(10.0 / pr.NOISE_UNIT)
        T, w = orr.unpack_taps(taps[n])
        assert abs(float(w[0]) + 2 * float(w[1:].astype(np.float64).sum()) - 1) < 1e-6 and (np.diff(w) < 0).all()
        # the map carries the centre of the paste rectangle to the centre of the plate (every stage keeps its image's centre
        # but for PIL's integer sizes: a pixel or two of the 380 x 160 plate)
        cx, cy = px + img.size[0] / 2. - 0.5, py + img.size[1] / 2. - 0.5
        p = r['m'].astype(np.float64).reshape(3, 3) @ [cx, cy, 1.0]
        assert abs(p[0] - 189.5) <= 3 and abs(p[1] - 79.5) <= 3, (n, p)
    assert clipped >= 3
    no_blur = render.gaussian_taps(0.01)
    assert no_blur[0] == 0 and no_blur.view(np.float32)[1] == 1
    assert render.gaussian_taps(7.9)[0] == 24 and render.gaussian_taps(8.0)[0] == 24 and render.gaussian_taps(0.4)[0] == 2
    with pytest.raises(TypeError):
        gen.draw_ocr_params(1, H, W, blur=3)
    with pytest.raises(ValueError):
        gen.draw_ocr_params(1, 96, 160)


def test_labels_carry_the_shear_term_and_nothing_else_new(gen):
    """M = N = 0: the reference's formula (:203-209) as written; M > 0 adds |m| LP_h / 2 to every edge."""
    d = dict(ids=[10, 11, 12, 0, 1, 2, 3], LP_w=360, LP_h=150, m=0.0, n=0.0, deg=4.0, sigma=0.0)
    r = 4.0 * np.pi / 180 * np.pi / 180
    off = 17 + abs(150 * np.sin(r) / 2)
    want = [[g, (off + c / 380. * 360 * np.cos(r)) / W, (off + (c + 45) / 380. * 360 * np.cos(r)) / W]
            for g, c in zip(d['ids'], (7, 56, 106, 175, 225, 274, 324))]
    plain = render.LPGenerator.ocr_labels(d, 17, W)
    assert np.array_equal(plain, np.float32(want))
    sheared = render.LPGenerator.ocr_labels(dict(d, m=-0.08), 17, W)
    np.testing.assert_allclose(sheared[:, 1:] - plain[:, 1:], 0.08 * 150 / 2 / W, atol=1e-6)
    assert np.array_equal(sheared[:, 0], plain[:, 0])


# ---- the read-back property --------------------------------------------------------------------------------------------------
def test_targets_of_a_plate_inside_the_canvas_read_back_as_its_text(gen):
    """For plates wholly inside the canvas (every label in [0, 1]) the target scores read through predict's 0.6 peak rule give
    exactly the plate's seven characters: a glyph is 2.5 to 2.8 columns of 24 wide, so a column centre lies within half a column of
    its centre (a score of 0.8 or more there), its other columns score 0.5 or more and less than that one, and the columns of
    two neighbouring glyphs meet at their low ends.  2000 seeded draws with the reference's geometry (no shear); the share left out (a label outside [0, 1]:
    about 58 % of draws) is bounded so that the test cannot pass on nothing."""
    np.random.seed(1234); random.seed(1234)
    lab, rows, _, orders = gen.draw_ocr_params(2000, H, W, M=0.0, N=0.0, noise=0.0)
    inside = (lab[:, :, 1:].min(axis=(1, 2)) >= 0) & (lab[:, :, 1:].max(axis=(1, 2)) <= 1)
    left_out = 1.0 - inside.mean()
    score_y, class_y = olr.targets(lab[inside], orders[inside], 24, np.float32)
    lowest = score_y[class_y >= 0].min()
    print('left out %.1f %% of 2000 draws; the lowest labelled score is %.3f' % (100 * left_out, lowest))
    assert left_out <= 0.65
    for n in range(len(score_y)):
        cols = olr.peaks(score_y[n], 0.6)
        assert [int(class_y[n, i]) for i in cols] == lab[inside][n, :, 0].astype(int).tolist(), n
    assert lowest >= 0.5 - 1e-6
