"""CPU checks of the background bank's host side (yolo_amd/background.py: the crop rule, the geometry, the rows, the epoch order)
and of its C ABI entries (declared, bound, revision still 5, bad arguments refused without a GPU); the numpy restatement
(tests/background_ref.py) on identity rows pins the conventions."""
import ctypes as C
import math
import os
import random
import re

import numpy as np

import background_ref as br
from yolo_amd import background as bgm
from yolo_amd import lib as L
from yolo_amd import render

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NAMES = ('yolo_bg_workspace_bytes', 'yolo_bg_stats', 'yolo_bg_render')


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _bank(h, w, mode='train', augment=True, images=None):
    return bgm.BackgroundBank(br.bank_images(seed=3) if images is None else images, h, w, mode=mode, augment=augment)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_bg_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    assert int(re.search(r'#define YOLO_BG_ROW_WORDS (\d+)', h).group(1)) == bgm.BG_ROW_WORDS == br.ROW_WORDS
    for name, nargs in zip(NAMES, (3, 8, 9)):
        assert name in L.SIGNATURES
        proto = re.search(r'%s\(([^)]*)\)' % name, h).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == nargs


def test_bg_entries_refuse_bad_arguments_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.yolo_bg_workspace_bytes(4, 32, 48) > 0
    assert lib.yolo_bg_workspace_bytes(64, 416, 416) == 16 * lib.yolo_bg_workspace_bytes(4, 416, 416)
    for bad in ((0, 32, 48), (4, 0, 48), (4, 32, -1)):
        assert lib.yolo_bg_workspace_bytes(*bad) == L.EINVAL
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    #        bank bytes rows work N  H   W   stream
    stats = [p,   1024, p,   p,   2, 32, 48, None]
    #         bank bytes rows work out N  H   W   stream
    rend = [p,   1024, p,   p,   p,  2, 32, 48, None]
    for fn, ok, ptrs, sizes in ((lib.yolo_bg_stats, stats, (0, 2, 3), (1, 4, 5, 6)), (lib.yolo_bg_render, rend, (0, 2, 3, 4), (1, 5, 6, 7))):
        for k in ptrs:                                                      # a NULL pointer
            a = list(ok); a[k] = None
            assert fn(*a) == L.EINVAL, k
        for k in sizes:                                                     # a non-positive bank size, N, H, W
            for v in (0, -3):
                a = list(ok); a[k] = v
                assert fn(*a) == L.EINVAL, (k, v)
        a = list(ok); a[sizes[2]], a[sizes[3]] = 2 ** 31 - 1, 8             # H * ceil(W / 4) leaves 32 bits
        assert fn(*a) == L.EUNSUPPORTED
        for k, addr in ((0, 4098), (2, 4100), (3, 4100)):                   # a misaligned bank (4) / rows (8) / workspace (8)
            a = list(ok); a[k] = C.c_void_p(addr)
            assert fn(*a) == L.EINVAL, k


def test_background_bank_is_exported_lazily():
    import yolo_amd
    assert yolo_amd.BackgroundBank is bgm.BackgroundBank


# ---- the crop rule ---------------------------------------------------------------------------------------------------------
def test_every_crop_lies_inside_its_image():
    _seed(11)
    for h, w in ((480, 640), (5, 5), (8, 200)):
        for _ in range(2000):
            x0, y0, cw, ch, _ = bgm.random_sized_crop(h, w, (416, 416))
            assert cw >= 1 and ch >= 1 and x0 >= 0 and y0 >= 0 and x0 + cw <= w and y0 + ch <= h, (h, w, x0, y0, cw, ch)


def test_accepted_crops_keep_the_area_and_aspect_ranges():
    """cw = round(sqrt(target ratio)), ch = round(sqrt(target / ratio)): each side is within half a pixel of its real value, so the
    bounds are checked on the sides moved by that half pixel (the +-1 px the rounding allows, and no more)."""
    _seed(12)
    h, w = 480, 640
    accepted = 0
    for _ in range(2000):
        _, _, cw, ch, fallback = bgm.random_sized_crop(h, w, (416, 416))
        if fallback:
            continue
        accepted += 1
        assert (cw - 0.5) * (ch - 0.5) <= 1.0 * h * w and (cw + 0.5) * (ch + 0.5) >= 0.08 * h * w, (cw, ch)
        assert (cw - 0.5) / (ch + 0.5) <= 4.0 / 3.0 and (cw + 0.5) / (ch - 0.5) >= 3.0 / 4.0, (cw, ch)
    assert accepted > 1900


def test_a_strip_always_takes_the_centred_fallback():
    """8 x 200: ch >= sqrt(0.08 * 1600 / (4/3)) = 9.8 > 8 on every try."""
    _seed(13)
    for out_hw, want in (((416, 416), (96, 0, 8, 8)), ((16, 24), (94, 0, 12, 8)), ((24, 16), (97, 0, 5, 8))):
        for _ in range(300):
            x0, y0, cw, ch, fallback = bgm.random_sized_crop(8, 200, out_hw)
            assert fallback and (x0, y0, cw, ch) == want
        x0, y0, cw, ch = want
        assert abs(cw * out_hw[0] - ch * out_hw[1]) < max(out_hw)                 # the output's aspect, to the pixel
        assert abs((200 - cw) - 2 * x0) <= 1 and abs((8 - ch) - 2 * y0) <= 1      # centred
    # a tall strip: full width, the height follows
    assert bgm.random_sized_crop(200, 8, (416, 416)) == (0, 96, 8, 8, True)


# ---- geometry and rows -----------------------------------------------------------------------------------------------------
def test_whole_image_at_its_own_size_is_the_identity_map():
    bank = _bank(32, 48, augment=False)
    r = bgm.unpack_row(bank.param_row(4, (0, 0, 48, 32)))
    assert r['has'] == 1 and (r['h'], r['w']) == (32, 48) and r['roi'] == [0, 0, 47, 31] and r['off'] == bank.table[4][0][0]
    assert np.array_equal(r['a'], np.float32([1, 0, 0, 0, 1, 0]))
    assert np.array_equal(r['A'], np.eye(3, dtype=np.float32)) and not r['D'].any() and not r['e'].any()
    m = bgm.unpack_row(bank.param_row(4, (0, 0, 48, 32), mirror=True))
    assert np.array_equal(m['a'], np.float32([-1, 0, 47, 0, 1, 0]))


def test_an_exact_halving_picks_level_one_with_integer_coordinates():
    bank = _bank(16, 24, augment=False)
    assert [len(t) for t in bank.table] == [1, 3, 3, 1, 3]
    r = bgm.unpack_row(bank.param_row(4, (0, 0, 48, 32)))
    assert (r['off'], r['h'], r['w']) == bank.table[4][1] == (bank.table[4][0][0] + 4 * 32 * 48, 16, 24)
    assert np.array_equal(r['a'], np.float32([1, 0, 0, 0, 1, 0])) and r['roi'] == [0, 0, 23, 15]
    # the level follows the axis that shrinks LEAST: 48 -> 24 columns is 1/2 but 8 of the 32 rows -> 16 is a magnification
    r = bgm.unpack_row(bank.param_row(4, (0, 12, 48, 8)))
    assert (r['h'], r['w']) == (32, 48)


def test_roi_and_map_follow_the_rule():
    """param_row against tests/background_ref.crop_row, which derives the map on its own; the roi by the rule, clipped to the level."""
    for out_hw in br.OUTPUTS + ((416, 416),):
        bank = _bank(out_hw[0], out_hw[1], augment=False)
        data, table = br.pack_bank(br.bank_images(seed=3))
        assert np.array_equal(bank.data, data) and bank.table == table
        for s, crop in ((1, (10, 9, 6, 4)), (2, (7, 5, 40, 30)), (2, (0, 0, 64, 48)), (1, (0, 0, 53, 37)), (1, (3, 1, 50, 36)), (0, (1, 2, 5, 6)),
                        (3, (0, 0, 5, 5))):
            for mirror in (False, True):
                got, want = bank.param_row(s, crop, mirror), br.crop_row(table, s, crop, out_hw, mirror)
                assert np.array_equal(got[:10], want[:10]), (out_hw, s, crop)
                np.testing.assert_allclose(got.view(np.float32)[10:16], want.view(np.float32)[10:16], rtol=1e-6, atol=1e-6)
    # the 37 x 53 image's level 1 is 18 x 26: its odd last row and column are dropped, and the roi is clipped to what is left
    bank = _bank(13, 13, augment=False)
    r = bgm.unpack_row(bank.param_row(1, (1, 1, 52, 36)))
    assert (r['h'], r['w']) == (18, 26) and r['roi'] == [0, 0, 25, 17]
    r = bgm.unpack_row(bank.param_row(1, (11, 6, 30, 31)))
    assert (r['h'], r['w']) == (18, 26) and r['roi'] == [5, 3, 20, 17]          # [11 >> 1, 40 >> 1] x [6 >> 1, min(36 >> 1, 17)]


def test_rows_round_trip():
    colour = (np.arange(9).reshape(3, 3) * 0.25 - 1, np.arange(9).reshape(3, 3) * -0.5 + 2, [7.0, -8.5, 0.125])
    args = dict(off=2 ** 33 + 4, h=37, w=53, roi=[1, 2, 50, 30], a=[0.5, 0.25, -3.0, 0.0, -2.0, 9.5])
    for make, unpack in ((br.make_row, bgm.unpack_row), (bgm.make_row, br.unpack), (bgm.make_row, bgm.unpack_row)):
        row = make(args['off'], args['h'], args['w'], args['roi'], args['a'], *colour)
        assert row.dtype == np.int32 and row.shape == (br.ROW_WORDS,) and row[7] == 0 and not row[37:].any()
        r = unpack(row)
        assert r['has'] == 1 and (r['off'], r['h'], r['w'], r['roi']) == (args['off'], 37, 53, args['roi'])
        assert np.array_equal(r['a'], np.float32(args['a'])) and np.array_equal(r['A'], np.float32(colour[0]))
        assert np.array_equal(r['D'], np.float32(colour[1])) and np.array_equal(r['e'], np.float32(colour[2]))
    assert np.array_equal(br.make_row(args['off'], 37, 53, args['roi'], args['a'], *colour), bgm.make_row(args['off'], 37, 53, args['roi'], args['a'], *colour))


# ---- colour and seeds ------------------------------------------------------------------------------------------------------
def test_without_augmentation_rows_carry_the_identity_colour_and_the_whole_image():
    bank = _bank(16, 24, mode='val', augment=False)
    state = random.getstate()
    rows = bank.draw_params(7)
    assert random.getstate() == state                                       # no draw at all
    for n, row in enumerate(rows):
        r = bgm.unpack_row(row)
        s = n % 5
        assert np.array_equal(r['A'], np.eye(3, dtype=np.float32)) and not r['D'].any() and not r['e'].any()
        assert np.array_equal(row, bank.param_row(s, (0, 0, bank.size[s][1], bank.size[s][0])))


def test_the_same_seed_gives_the_same_rows_and_the_draws_are_the_documented_ones():
    bank = _bank(16, 24)
    _seed(5)
    first = bank.draw_params(12)
    bank.reset()
    _seed(5)
    again = bank.draw_params(12)
    assert first.shape == (12, br.ROW_WORDS) and first.dtype == np.int32 and np.array_equal(first, again)
    _seed(6)
    bank.reset()
    assert not np.array_equal(bank.draw_params(12), first)
    # the draws by hand, in the documented order
    bank.reset()
    _seed(5)
    order = list(range(5))
    aug = render.ColorAugmenter(brightness=0.5, contrast=0.5, saturation=0.5, hue=1.0, pca_noise=0)
    for n in range(12):
        if n % 5 == 0:
            random.shuffle(order)
        s = order[n % 5]
        x0, y0, cw, ch, _ = bgm.random_sized_crop(bank.size[s][0], bank.size[s][1], (16, 24))
        mirror = random.random() < 0.5
        A, D, e = aug.affine()
        assert np.array_equal(first[n], bank.param_row(s, (x0, y0, cw, ch), mirror, (A, D, e))), n
        assert np.abs(D).max() > 0 and np.abs(e).max() == 0                 # contrast is on; pca_noise = 0 adds nothing to e


# ---- ordering --------------------------------------------------------------------------------------------------------------
def _indices(bank, rows):
    level = {t[k][0]: s for s, t in enumerate(bank.table) for k in range(len(t))}
    return [level[bgm.unpack_row(r)['off']] for r in rows]


def test_val_order_is_sequential_and_wraps():
    bank = _bank(16, 24, mode='val')
    _seed(1)
    assert _indices(bank, bank.draw_params(7)) == [0, 1, 2, 3, 4, 0, 1]
    assert _indices(bank, bank.draw_params(4)) == [2, 3, 4, 0]              # the cursor carries over from batch to batch


def test_train_order_is_a_permutation_per_epoch():
    images = br.bank_images(seed=4, sizes=((9, 9),) * 11)
    bank = _bank(8, 8, images=images)
    _seed(2)
    got = _indices(bank, np.concatenate([bank.draw_params(7), bank.draw_params(7), bank.draw_params(8), bank.draw_params(11)]))
    epochs = [got[0:11], got[11:22], got[22:33]]
    for e in epochs:
        assert sorted(e) == list(range(11))
    assert epochs[0] != list(range(11)) and epochs[0] != epochs[1]          # shuffled, and reshuffled at the wrap


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_restatement_of_an_identity_row_is_the_image():
    images = br.bank_images(seed=3)
    data, table = br.pack_bank(images)
    for s in range(5):
        h, w = br.IMAGE_SIZES[s]
        out = br.render(data, br.crop_row(table, s, (0, 0, w, h), (h, w))[None], h, w)
        assert out.dtype == np.float32 and np.array_equal(out[0], images[s].astype(np.float32).transpose(2, 0, 1))
        out = br.render(data, br.crop_row(table, s, (0, 0, w, h), (h, w), mirror=True)[None], h, w)
        assert np.array_equal(out[0], images[s][:, ::-1].astype(np.float32).transpose(2, 0, 1))
    # the package's bank and rows through the restatement: the same
    bank = _bank(32, 48, mode='val', augment=False, images=[images[4]])
    assert np.array_equal(br.render(bank.data, bank.draw_params(1), 32, 48)[0], images[4].astype(np.float32).transpose(2, 0, 1))
    # a 'no image' row gives e, and a bound smaller than the buffer is honoured
    row = br.crop_row(table, 4, (0, 0, 48, 32), (8, 8), colour=(np.eye(3), np.zeros((3, 3)), [1.0, 2.0, 3.0]))
    assert not np.array_equal(br.render(data, row[None], 8, 8)[0, 0], np.full((8, 8), 1.0, np.float32))
    cut = br.render(data, row[None], 8, 8, bank_bytes=data.size - 4)                # (the last image's last level loses a pixel)
    assert np.array_equal(cut[0], np.broadcast_to(np.float32([1, 2, 3])[:, None, None], (3, 8, 8)))


def test_mip_rule_restated_equals_the_packages():
    px = np.random.default_rng(0).integers(0, 256, (37, 53, 4), dtype=np.uint8)
    for a, b in zip(br.mip_chain(px), render.mip_chain(px)):
        assert np.array_equal(a, b)
    assert math.isclose(render.MIP_MIN_SIDE, br.MIP_MIN_SIDE)
