"""The device renderer (csrc/render.hip: yolo_render_stats + yolo_render_cars) against its numpy restatement
(tests/render_ref.py), against yolo_composite on an identity draw, and RenderCar.render_device end to end.  Canvases 32 x 48
(W % 4 == 0: 16-byte loads and stores) and 30 x 45 (scalar accesses, a tail thread); sprites 9 x 9, 20 x 28 and 64 x 40 with
their mip levels (the 20 x 28 one has two, the 64 x 40 one three)."""
import random

import numpy as np
import pytest

import render_ref as rr
from yolo_amd import lib as L
from yolo_amd import render

pytestmark = pytest.mark.gpu
CANVASES = [(32, 48), (30, 45)]
ATOL = 2e-6        # 0..1 images: mu may differ from the restatement's by one float32 ulp, which moves D mu / 255 by under 5e-7


def device_render(cuda, bg, atlas, rows):
    """-> (out (N,3,H,W) float32 ndarray, the two status codes)."""
    import torch
    lib = L.load()
    N, _, H, W = bg.shape
    bg_d = torch.from_numpy(np.ascontiguousarray(bg, np.float32)).to(cuda)
    atlas_d = torch.from_numpy(np.ascontiguousarray(atlas)).to(cuda)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(cuda)
    work = torch.empty(lib.yolo_render_workspace_bytes(N, H, W), dtype=torch.uint8, device=cuda)
    out = torch.full_like(bg_d, -7.0)
    rc1 = lib.yolo_render_stats(L.ptr(atlas_d), atlas_d.numel(), L.ptr(rows_d), L.ptr(work), N, H, W, L.stream_ptr())
    rc2 = lib.yolo_render_cars(L.ptr(bg_d), L.ptr(atlas_d), atlas_d.numel(), L.ptr(rows_d), L.ptr(work), L.ptr(out), N, H, W, L.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), (rc1, rc2)


def _bg(seed, N, H, W):
    return (np.random.default_rng(seed).random((N, 3, H, W)) * 300 - 20).astype(np.float32)          # (out of range: the clip works)


def _colour(seed):
    random.seed(seed); np.random.seed(seed)
    return render.ColorAugmenter().affine()


def _row(table, s, level, H, W, scale, deg, cx, cy, sigma=0.0, colour=None, has=1):
    off, lh, lw = table[s][level]
    a = rr.placement((lh, lw), level, scale, deg, cx, cy)
    w0, w1 = render.blur_weights(sigma)
    A, D, e = colour if colour is not None else (None, None, None)
    return rr.make_row(off, lh, lw, a, rr.window(a.astype(np.float32).astype(np.float64), (lh, lw), H, W), w0, w1, A, D, e, has)


def _six(table, H, W):
    """no sprite; wholly inside; across the left and top edges (negative paste); across the right and bottom edges; rotated
    30 degrees with blur; every colour stage on (a mip level, blur, rotation as well)."""
    return np.stack([_row(table, 0, 0, H, W, 1.0, 0.0, 10.0, 10.0, has=0),
                     _row(table, 0, 0, H, W, 1.3, 0.0, W / 2.0 + 0.25, H / 2.0 - 0.4),
                     _row(table, 1, 0, H, W, 0.8, 0.0, 3.0, 2.5),
                     _row(table, 2, 1, H, W, 0.45, 0.0, W - 4.0, H - 6.3),
                     _row(table, 1, 0, H, W, 0.9, 30.0, W / 2.0, H / 2.0, sigma=0.3),
                     _row(table, 2, 1, H, W, 0.4, -17.0, W / 2.0 - 3, H / 2.0 + 2, sigma=0.2, colour=_colour(3))])


@pytest.fixture(scope='module')
def atlas():
    data, table = rr.pack_atlas(rr.synthetic_sprites(seed=1), render.mip_chain)
    assert [len(t) for t in table] == [1, 2, 3]
    return data, table


@pytest.fixture(scope='module')
def reference(atlas):
    """The restatement of the six-image batch on both canvases, computed once."""
    out = {}
    for H, W in CANVASES:
        bg, rows = _bg(2, 6, H, W), _six(atlas[1], H, W)
        out[(H, W)] = (bg, rows, rr.render(bg, atlas[0], rows))
    return out


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_batch_against_the_restatement(cuda, atlas, reference, hw):
    bg, rows, want = reference[hw]
    got, rcs = device_render(cuda, bg, atlas[0], rows)
    assert rcs == (L.OK, L.OK)
    for n in range(6):
        err = float(np.abs(got[n].astype(np.float64) - want[n]).max())
        touched = float((want[n] != np.clip(bg[n] / np.float32(255), 0, 1)).mean())
        print('%dx%d image %d: max |device - restatement| = %.3g, %.0f %% of the canvas drawn on' % (hw + (n, err, 100 * touched)))
        assert err <= ATOL, (n, err)
        assert (touched == 0) if n == 0 else (touched > 0.03)
    # images 0..4 carry no contrast term: bit-equal by construction
    assert np.array_equal(got[:5], want[:5])


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_identity_draw_equals_composite_of_a_numpy_paste(cuda, hw):
    """Scale 1, angle 0, an integer paste offset, no blur, no colour: the sprite's own bytes land on the canvas, and the result
    is bit-equal to yolo_composite fed the sprite pasted by numpy slicing.  The sprites' alpha is 0 or 255 here:
    yolo_composite is built with floating-point contraction and takes fg * mask + (bg / 255) * (1 - mask) as ONE fused
    multiply-add, the renderer (no contraction, its header's definition) as a product and a sum -- the same number when
    mask is 0 or 1.  With fractional alpha the two may differ in the last bit: checked to 1.2e-7 (one ulp below 1)."""
    import torch
    H, W = hw
    for binary in (True, False):
        sprites = rr.synthetic_sprites(seed=4, binary_alpha=binary)
        data, table = rr.pack_atlas(sprites, render.mip_chain)
        # (sprite, paste x, paste y): inside, across the left edge, the right and top edges, the right and bottom edges
        places = [(0, 5, 7), (1, -6, 9), (2, W - 30, -20), (0, W - 5, H - 4)]
        rows, fg, mask = [], np.zeros((4, 3, H, W), np.float32), np.zeros((4, 3, H, W), np.float32)
        for n, (s, px, py) in enumerate(places):
            off, h, w = table[s][0]
            a = [1.0, 0.0, -px, 0.0, 1.0, -py]
            rows.append(rr.make_row(off, h, w, a, rr.window(np.float64(a), (h, w), H, W)))
            y0, y1, x0, x1 = max(py, 0), min(py + h, H), max(px, 0), min(px + w, W)
            part = sprites[s][y0 - py:y1 - py, x0 - px:x1 - px].astype(np.float32)
            fg[n, :, y0:y1, x0:x1] = part[..., :3].transpose(2, 0, 1) / np.float32(255)
            mask[n, :, y0:y1, x0:x1] = part[..., 3] / np.float32(255)
        bg = _bg(5, 4, H, W)
        got, rcs = device_render(cuda, bg, data, np.stack(rows))
        assert rcs == (L.OK, L.OK)
        want = render.composite(torch.from_numpy(bg).to(cuda), torch.from_numpy(fg).to(cuda), torch.from_numpy(mask).to(cuda)).cpu().numpy()
        if binary:
            assert (mask.reshape(4, -1).max(axis=1) == 1).all()
            assert np.array_equal(got, want)
        else:
            assert float(np.abs(got - want).max()) <= 1.2e-7


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_widening_the_window_changes_no_bit(cuda, atlas, reference, hw):
    """(Image 5 has D != 0.  A wider window spreads pass 1's pixels over the threads differently, so the ORDER of its double sums
    changes; the added pixels are exact zeros and the sums' last bits are far below the float32 mu is rounded to, so mu -- and
    with it every output bit -- stays, but that is arithmetic slack, not a guarantee: were this ever to flip, it would be mu by
    one ulp, under 5e-7 on the image.)"""
    bg, rows, _ = reference[hw]
    wide = rows.copy()
    wide[:, 3:7] = [0, 0, hw[1], hw[0]]
    narrow, _ = device_render(cuda, bg, atlas[0], rows)
    whole, _ = device_render(cuda, bg, atlas[0], wide)
    assert np.array_equal(narrow, whole)
    # and a window wider than the canvas is clipped to it
    wide[:, 3:7] = [-5, -9, hw[1] + 40, hw[0] + 3]
    assert np.array_equal(device_render(cuda, bg, atlas[0], wide)[0], whole)


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_contrast_only_on_a_clipped_sprite_uses_what_is_on_the_canvas(cuda, atlas, hw):
    """A contrast-only row (A = alpha I, D = (1 - alpha) 1 coef^T, e = 0) on a sprite half off the canvas: mu is the mean over
    the H W canvas pixels of what is ON the canvas (zero elsewhere)."""
    H, W = hw
    data, table = atlas
    alpha = 1.4
    coef = np.float64([0.299, 0.587, 0.114])
    colour = (alpha * np.eye(3), (1 - alpha) * np.outer(np.ones(3), coef), np.zeros(3))
    rows = np.stack([_row(table, 2, 0, H, W, 1.0, 0.0, 2.0, H / 2.0, colour=colour),
                     _row(table, 2, 0, H, W, 1.0, 0.0, float(W // 2), H / 2.0, colour=colour)])     # the same sprite, less of it cut off
    bg = _bg(6, 2, H, W)
    want, mus, _ = rr.render(bg, data, rows, return_parts=True)
    # mu, independently: the sprite's level-0 columns that land on the canvas (identity scale, integer offsets)
    sprite = rr.synthetic_sprites(seed=1)[2].astype(np.float64)
    for n, cx in enumerate((2.0, float(W // 2))):
        x_off, y_off = int(cx - 20), int(H / 2.0 - 32)
        part = sprite[max(-y_off, 0):min(H - y_off, 64), max(-x_off, 0):min(W - x_off, 40), :3]
        np.testing.assert_allclose(mus[n], part.sum(axis=(0, 1)) / (H * W), rtol=1e-6)
    assert mus[0].sum() < 0.8 * mus[1].sum()
    got, rcs = device_render(cuda, bg, data, rows)
    assert rcs == (L.OK, L.OK)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print('contrast only: max |device - restatement| = %.3g' % err)
    assert err <= ATOL


def test_two_calls_are_bit_identical(cuda, atlas, reference):
    for hw in CANVASES:
        bg, rows, _ = reference[hw]
        assert np.array_equal(device_render(cuda, bg, atlas[0], rows)[0], device_render(cuda, bg, atlas[0], rows)[0])


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_rows_that_point_past_the_atlas_render_as_background(cuda, atlas, hw):
    """The kernels check a row's level against the atlas size before any load: such rows are 'no sprite' and the call returns
    YOLO_OK."""
    H, W = hw
    data, table = atlas
    good = _row(table, 1, 0, H, W, 1.0, 0.0, W / 2.0, H / 2.0, sigma=0.3, colour=_colour(1))
    rows = np.stack([good] * 8)
    off, h, w = table[1][0]

    def put(n, off=off, h=h, w=w):
        rows[n, 1], rows[n, 2] = h, w
        rows[n, 8:10] = np.array([off], np.int64).view(np.int32)
    put(1, off=data.size)                       # the offset is the end of the atlas
    put(2, off=data.size - 4 * h * w + 4)       # the level's last pixel lies past the end
    put(3, off=2 ** 40)                         # far away
    put(4, off=-4)
    put(5, h=2 ** 20, w=2 ** 20)                # a size past the atlas (and 4 h w past 32 bits)
    put(6, h=0)
    put(7, off=off + 2)                         # not a whole pixel
    bg = _bg(7, 8, H, W)
    got, rcs = device_render(cuda, bg, data, rows)
    assert rcs == (L.OK, L.OK)
    plain = np.clip(bg / np.float32(255), 0, 1)
    assert not np.array_equal(got[0], plain[0])
    assert np.array_equal(got[1:], plain[1:])
    assert float(np.abs(got[0] - rr.render(bg[:1], data, rows[:1])[0]).max()) <= ATOL


def test_render_device_end_to_end(cuda, tmp_path):
    """RenderCar.render_device on wholly opaque white sprites over a zero background, augment=False: images in [0, 1], labels
    = draw_params' under the same seed, and for every car the box of the non-zero pixels contains the label box clipped to
    the canvas to within 1 px and exceeds it by at most 3 px (the bilinear tap reaches under 1 px past the sprite's edge,
    the blur 1 px more)."""
    import torch
    rr.write_sprite_dir(str(tmp_path), opaque_white=True)
    H, W = 96, 128
    rc = render.RenderCar(H, W, rr.CLASSES, str(tmp_path), device=cuda, augment=False)
    bg = torch.zeros((12, 3, H, W), device=cuda)
    np.random.seed(9); random.seed(9)
    img, lab = rc.render_device(bg, 'train', render_rate=0.85)
    np.random.seed(9); random.seed(9)
    lab_h, rows = rc.draw_params(12, 'train', render_rate=0.85)
    img2 = torch.empty_like(bg)
    np.random.seed(9); random.seed(9)
    out2, _ = rc.render_device(bg, 'train', render_rate=0.85, out=img2)
    torch.cuda.synchronize()
    assert out2 is img2 and torch.equal(img, img2)
    img, lab = img.cpu().numpy(), lab.cpu().numpy()
    assert img.shape == (12, 3, H, W) and img.dtype == np.float32 and img.min() >= 0 and img.max() <= 1
    assert lab.shape == (12, 1, 30) and np.array_equal(lab, lab_h)
    cars = np.nonzero(lab[:, 0, 0] >= 0)[0]
    assert 6 <= len(cars) < 12
    for n in range(12):
        on = (img[n] != 0).any(axis=0)
        if n not in cars:
            assert not on.any()
            continue
        assert img[n].max() > 0.99
        y, x, h, w = [float(v) for v in lab[n, 0, 1:5]]
        l, t, r, b = max((x - w / 2) * W, 0), max((y - h / 2) * H, 0), min((x + w / 2) * W, W), min((y + h / 2) * H, H)
        ys, xs = np.nonzero(on)
        got = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
        out = (l - got[0], t - got[1], got[2] - r, got[3] - b)                  # how far the drawn box lies outside the label box
        print('image %d: drawn box outside the label box by %s' % (n, ['%.2f' % v for v in out]))
        assert min(out) >= -1 and max(out) <= 3, (n, out)


def test_render_device_equals_the_restatement_of_its_rows(cuda, tmp_path):
    """The whole call with everything on -- PNG sprites and PASCAL3D+ crops, rotation, blur, the colour augmenter, a random
    background: what render_device returns is the restatement of the rows draw_params makes under the same seed (the rows,
    the labels and the atlas reach the device as they were made)."""
    import torch
    rr.write_sprite_dir(str(tmp_path / 'png'))
    rr.write_pascal_dir(str(tmp_path / 'pascal'))
    H, W = 64, 96
    rc = render.RenderCar(H, W, rr.CLASSES, str(tmp_path / 'png'), device=cuda, pascal_root=str(tmp_path / 'pascal'))
    bg = _bg(8, 8, H, W)
    np.random.seed(13); random.seed(13)
    img, lab = rc.render_device(torch.from_numpy(bg).to(cuda), 'train', pascal_rate=0.5, render_rate=0.9)
    np.random.seed(13); random.seed(13)
    lab_h, rows = rc.draw_params(8, 'train', pascal_rate=0.5, render_rate=0.9)
    want = rr.render(bg, rc.atlas().data, rows)
    err = float(np.abs(img.cpu().numpy().astype(np.float64) - want).max())
    print('render_device: max |device - restatement| = %.3g' % err)
    assert err <= ATOL and np.array_equal(lab.cpu().numpy(), lab_h)
    assert (rows[:, 0] == 1).sum() >= 5 and np.abs(rows[:, 27:36].view(np.float32)).max() > 0          # (cars, and a contrast term)
