"""CPU checks of the overlay's text and the published row: the three C ABI entries (declared, bound, revision still 5, every bad
argument refused without a GPU), the restated formatting (tests/overlay_text_ref.py) against Python's own '%.3f', the label
geometry, the rasteriser's rule against a hand-drawn picture, and default_font()."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import overlay_ref as R
import overlay_text_ref as T
from yolo_amd import lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = ('yolo_pose_top1', 'yolo_overlay_labels', 'yolo_overlay_text')


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_text_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    from yolo_amd import overlay
    assert int(re.search(r'#define YOLO_OVERLAY_LABEL_WORDS (\d+)', h).group(1)) == overlay.LABEL_WORDS == T.LABEL_WORDS == 16
    assert int(re.search(r'#define YOLO_OVERLAY_LABEL_CHARS (\d+)', h).group(1)) == overlay.LABEL_CHARS == T.LABEL_CHARS == 40
    assert int(re.search(r'#define YOLO_OVERLAY_NAME_BYTES (\d+)', h).group(1)) == overlay.NAME_BYTES == T.NAME_BYTES == 16
    for name, nargs in zip(NAMES, (11, 30, 16)):
        assert name in L.SIGNATURES
        proto = re.search(r'^int %s\(([^)]*)\);' % name, h, flags=re.M).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs, name
    assert 'The radar plot is not offered' in h and 'depth lookup are not offered' not in h


def _pose_args():
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    #       pred B  C  dirs depth Hd  Wd  row5 rows_out pose stream
    return [p,   2, 9, p,   p,    24, 32, 1,   p,       p,   None]


def _labels_args():
    p = C.c_void_p(4096)
    #       table rows kept count scores nbox C  post cpb pred C  pose deg lp names nname cw ch  adv scale gap pad ground colour
    return [p,    p,   p,   p,    p,     10,  8, 3,   2,  p,   8, p,   1,  p, p,    2,    6, 11, 6,  1,    4,  1,  1,     0,
            # B H   W   K  labels stream
            2,  32, 48, 5, p,     None]


def _text_args():
    p = C.c_void_p(4096)
    #       frames labels font nglyph first cw ch  adv scale pad N  H   W   C  K  stream
    return [p,     p,     p,   95,    32,   6, 11, 6,  1,    1,  2, 32, 48, 3, 5, None]


def test_text_entries_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    for name in NAMES:
        assert hasattr(lib, name)
    # yolo_pose_top1
    ok = _pose_args()
    for k in (0, 3, 9):                                                    # NULL pred / class_dirs / pose
        a = list(ok); a[k] = None
        assert lib.yolo_pose_top1(*a) == L.EINVAL, k
    for k, bad in ((1, (0, -2)), (2, (6, 0)), (5, (0, -1)), (6, (0, -1)), (7, (-1, 3))):
        for v in bad:
            a = list(ok); a[k] = v
            assert lib.yolo_pose_top1(*a) == L.EINVAL, (k, v)
    a = list(ok); a[9] = C.c_void_p(4104)
    assert lib.yolo_pose_top1(*a) == L.EINVAL                              # pose not 16-byte aligned
    # yolo_overlay_labels
    ok = _labels_args()
    for k in (0, 28, 2, 3):                                                # NULL table / labels / kept / count
        a = list(ok); a[k] = None
        assert lib.yolo_overlay_labels(*a) == L.EINVAL, k
    a = list(ok); a[14] = None
    assert lib.yolo_overlay_labels(*a) == L.EINVAL                         # names NULL with nname > 0
    for k in (5, 7, 8, 16, 17, 19, 24, 25, 26, 27):                        # non-positive sizes
        for v in (0, -3):
            a = list(ok); a[k] = v
            assert lib.yolo_overlay_labels(*a) == L.EINVAL, (k, v)
    for k, v in ((6, 4), (10, 5), (15, -1), (18, 5), (20, -1), (21, -1), (22, 2), (22, -1), (27, 4)):
        a = list(ok); a[k] = v                                             # rows_C, pred_C, nname, advance < cell_w, gap, pad, ground, K
        assert lib.yolo_overlay_labels(*a) == L.EINVAL, (k, v)
    a = list(ok); a[1] = a[9] = a[13] = None; a[27] = 1
    assert lib.yolo_overlay_labels(*a) == L.EINVAL                         # no source at all
    for k in (0, 28):
        a = list(ok); a[k] = C.c_void_p(4104)
        assert lib.yolo_overlay_labels(*a) == L.EINVAL, k                  # a table / labels pointer not 16-byte aligned
    for k, v in ((16, 33), (17, 33), (19, 17), (25, 16385), (26, 16385)):
        a = list(ok); a[k] = v
        if k == 16:
            a[18] = 33                                                     # (advance stays >= cell_w)
        assert lib.yolo_overlay_labels(*a) == L.EUNSUPPORTED, (k, v)
    a = list(ok); a[7], a[27] = 127, 129
    assert lib.yolo_overlay_labels(*a) == L.EUNSUPPORTED
    # yolo_overlay_text
    ok = _text_args()
    for k in (0, 1, 2):
        a = list(ok); a[k] = None
        assert lib.yolo_overlay_text(*a) == L.EINVAL, k
    for k in (3, 5, 6, 8, 10, 11, 12, 13, 14):                             # nglyph, cell_w, cell_h, scale, N, H, W, C, K
        for v in (0, -3):
            a = list(ok); a[k] = v
            assert lib.yolo_overlay_text(*a) == L.EINVAL, (k, v)
    for k, v in ((7, 5), (9, -1)):                                         # advance < cell_w, pad < 0
        a = list(ok); a[k] = v
        assert lib.yolo_overlay_text(*a) == L.EINVAL, (k, v)
    a = list(ok); a[1] = C.c_void_p(4104)
    assert lib.yolo_overlay_text(*a) == L.EINVAL                           # labels not 16-byte aligned
    a = list(ok); a[2] = C.c_void_p(4098)
    assert lib.yolo_overlay_text(*a) == L.EINVAL                           # font not 4-byte aligned
    for k, v in ((14, 129), (13, 5), (11, 16385), (12, 16385), (5, 33), (6, 33), (8, 17), (3, 257)):
        a = list(ok); a[k] = v
        if k == 5:
            a[7] = 33
        assert lib.yolo_overlay_text(*a) == L.EUNSUPPORTED, (k, v)


# ---- the formatting --------------------------------------------------------------------------------------------------------
def test_score_text_is_percent_3f():
    g = np.random.default_rng(0)
    for s in g.uniform(0.0, 1.0, 4000).astype(np.float32):
        assert T.score_text(s) == '%.3f' % s, s
    # exact ties (x.xxx5 representable in binary: to even) and the edges
    for s, want in ((0.0, '0.000'), (0.0005, None), (0.0625, '0.062'), (0.3125, '0.312'), (0.9995, None), (1.0, '1.000')):
        s = np.float32(s)
        assert T.score_text(s) == '%.3f' % s, s
        if want is not None:
            assert T.score_text(s) == want
    assert T.score_text(np.nextafter(np.float32(1), np.float32(2))) == '1.000'
    assert T.score_text(9.9994) == '9.999' and T.score_text(12.5) == '9.999' and T.score_text(3e38) == '9.999'
    for s in (np.nan, -0.25, np.inf, -np.inf):
        assert T.score_text(s) == '-.---'
    assert all(len(T.score_text(s)) == 5 for s in (0, 0.5, 7, 1e9, np.nan))


def test_degree_text():
    import math
    assert T.deg_text(np.float32(math.pi)) == '180' and T.deg_text(np.float32(-math.pi)) == '-180'
    assert T.deg_text(0.0) == '0' and T.deg_text(-0.4) == '-23' and T.deg_text(-0.001) == '0'
    assert T.deg_text(np.nan) is None and T.deg_text(np.inf) is None and T.deg_text(20.0) is None
    assert T.compose('car', 0.9371, -0.4) == 'car 0.937 -23' and T.compose('', 0.5, None) == '0.500'
    assert T.compose('x' * 16, np.nan, np.float32(-math.pi)) == 'x' * 16 + ' -.--- -180'            # the longest text: 27 bytes
    assert T.name_text(['a', b'bc\0d', ''], 1) == 'bc' and T.name_text(['a'], 1) == '' and T.name_text(None, 0) == ''
    words = T.pack_label(3, -4, 'car 0.937', (1, 2, 3), (0, 0, 0), 3)
    assert words[5] == 9 and T.label_text(words) == b'car 0.937' and words[6] == ord('c') | ord('a') << 8 | ord('r') << 16 | 32 << 24


def test_label_geometry():
    slot = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1, 0, 2, 1, 0]
    m = dict(cell_w=6, cell_h=11, advance=6, scale=1, gap=4, pad=1)
    assert T.place(slot(30, 40, 90, 80), 9, 160, **m) == (30, 25)           # over the top-left corner: y = 40 - 4 - 11
    assert T.place(slot(30, 10, 90, 80), 9, 160, **m) == (30, 14)           # no room above: under the top edge
    assert T.place(slot(30, 16, 90, 80), 9, 160, **m) == (30, 1)            # y - pad = 0 is still room
    assert T.place(slot(130, 40, 159, 80), 9, 160, **m) == (160 - 54 - 1, 25)       # moved left: Tw = 9 x 6
    assert T.place(slot(-20, 40, 30, 80), 9, 160, **m) == (1, 25)           # moved right to pad
    assert T.place(slot(10, 40, 30, 80), 40, 160, **m) == (1, 25)           # wider than the frame: left edge wins
    # a rotated box: the smallest x and the smallest y of the four vertices
    assert T.place([50, 30, 80, 45, 60, 70, 35, 52, 0, 2, 1, 0], 5, 160, **m) == (35, 15)
    m2 = dict(cell_w=5, cell_h=7, advance=7, scale=3, gap=2, pad=0)
    assert T.place(slot(10, 40, 30, 80), 5, 400, **m2) == (10, 40 - 2 - 21)


# ---- the rasteriser's rule -------------------------------------------------------------------------------------------------
def test_rule_draws_the_picture_by_hand():
    """two characters of a 3 x 2 font at scale 2, advance 4, pad 1: the picture written out."""
    font = np.array([[0b101, 0b010], [0b111, 0b001]], np.uint32)            # 'A' = X.X / .X. ; 'B' = XXX / X..
    frames = np.zeros((1, 8, 18, 1), np.uint8)
    lab = T.as_int32([[T.pack_label(2, 2, 'AB', (9,), (1,), 3)]])
    got = T.draw_text(frames, lab, font, 65, 3, 4, 2, 1)[0, :, :, 0]
    want = ['..................',
            '.gggggggggggggggg.',
            '.g##gg##gg######g.',
            '.g##gg##gg######g.',
            '.ggg##gggg##ggggg.',
            '.ggg##gggg##ggggg.',
            '.gggggggggggggggg.',
            '..................']
    key = {'.': 0, 'g': 1, '#': 9}
    assert [[key[ch] for ch in row] for row in want] == got.tolist()
    # without the ground only the ink; a byte outside the font inks nothing; nchar 41 / a far x: disabled
    bare = T.draw_text(frames, T.as_int32([[T.pack_label(2, 2, 'AB', (9,), (1,), 1)]]), font, 65, 3, 4, 2, 1)[0, :, :, 0]
    assert np.array_equal(bare, np.where(got == 9, 9, 0))
    assert not T.draw_text(frames, T.as_int32([[T.pack_label(2, 2, 'zz', (9,), (1,), 1)]]), font, 65, 3, 4, 2, 1).any()
    assert not T.draw_text(frames, T.as_int32([[T.pack_label(2, 2, 'AB', (9,), (1,), 3, nchar=41)]]), font, 65, 3, 4, 2, 1).any()
    assert not T.draw_text(frames, T.as_int32([[T.pack_label(2 ** 20 + 1, 2, 'AB', (9,), (1,), 3)]]), font, 65, 3, 4, 2, 1).any()


def test_labels_of_the_restatement():
    """the slot order, the sources and the disabled slots of labels() on a small shape table."""
    rows, kept, count = R.nms_case(5, 1, 6, 9, 3)
    kept[0], count[0] = [7, 2, -1], 2
    pred, lp = R.top1_rows(3, 1, 9), R.plate_rows(7, 1)
    sh = R.shapes(1, 120, 160, nms=(rows, kept, count), cand_per_box=3, pred=pred, lp=lp, camera=R.CAMERA)
    pose = np.array([[-0.4, 0.7, -1.0, 2.0]], np.float32)
    lab = T.labels(sh['table'], 160, nms=(rows, kept, count), cand_per_box=3, pred=pred, pose=pose, lp=lp, names=['a', 'bb', 'ccc'])
    texts = [T.label_text(w).decode() for w in lab[0]]
    assert texts[0] == 'bb ' + T.score_text(rows[0, 2, 0]) and texts[1] == 'ccc ' + T.score_text(rows[0, 0, 0]) and texts[2] == ''
    assert texts[3] == 'ccc ' + T.score_text(pred[0, 0]) + ' -23' and texts[4] == T.score_text(lp[0, 0])
    assert lab[0, :, 4].tolist() == [3, 3, 0, 3, 3] and not lab[0, 2].any()
    assert np.array_equal(lab[0, [0, 1, 3, 4], 2], sh['table'][0, [0, 1, 3, 4], 8])


# ---- the font --------------------------------------------------------------------------------------------------------------
def test_default_font():
    from yolo_amd.overlay import BitmapFont, default_font
    try:
        from PIL import ImageFont
        has = hasattr(ImageFont, 'load_default_imagefont') or isinstance(ImageFont.load_default(), ImageFont.ImageFont)
    except ImportError:
        has = False
    if not has:
        pytest.skip('this PIL has no built-in bitmap font')
    font = default_font()
    assert isinstance(font, BitmapFont) and font.nglyph == 95 and font.first_code == 32 and font.advance == font.cell_w
    assert font.masks.shape == (95, font.cell_h) and font.masks.dtype == np.uint32
    assert len({m.tobytes() for m in font.masks}) == 95                     # pairwise distinct
    empty = [g for g in range(95) if not font.masks[g].any()]
    assert empty == [0]                                                     # only the space
    assert not (font.masks >> font.cell_w).any() and 1 <= font.cell_w <= 32 and 1 <= font.cell_h <= 32
    with pytest.raises(ValueError):
        BitmapFont(np.full((2, 7), 1 << 5, np.uint32), 5)                   # ink outside the cell
    with pytest.raises(ValueError):
        BitmapFont(np.zeros((2, 7), np.uint32), 5, advance=4)


def test_depth_lookup_of_the_restatement():
    depth = np.arange(12, dtype=np.float32).reshape(3, 4)
    row = lambda y, x: np.array([0.9, y, x], np.float32)
    assert T.depth_at(row(0.5, 0.5), depth) == depth[1, 2] and T.depth_at(row(0.5, 0.5), None) == -1
    assert T.depth_at(row(0.99, 1.0), depth) == -1 and T.depth_at(row(1.0, 0.5), depth) == -1       # index = size
    assert T.depth_at(row(0.0, -0.1), depth) == depth[0, 0]                  # truncation toward zero: (int)(-0.4) = 0
    assert T.depth_at(row(0.0, -0.3), depth) == -1 and T.depth_at(row(np.nan, 0.5), depth) == -1
    assert T.depth_at(row(0.5, np.inf), depth) == -1
    assert T.top_class([1.0, 3.0, 3.0, np.nan]) == 1 and T.top_class([np.nan, np.nan]) == 0
