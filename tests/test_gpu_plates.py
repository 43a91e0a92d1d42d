"""The device plate renderer (csrc/plates.hip: yolo_plate_compose + yolo_plate_stats + yolo_plate_render) against PIL's paste, against
its numpy restatement (tests/plate_ref.py), and LPGenerator.add_device end to end.  Canvases 32 x 48 (W % 4 == 0: 16-byte loads
and stores) and 30 x 45 (scalar accesses, a tail thread); both take more than one block per image."""
import random

import numpy as np
import pytest

import plate_ref as pr
from yolo_amd import lib as L
from yolo_amd import render

pytestmark = pytest.mark.gpu
CANVASES = [(32, 48), (30, 45)]
EPS = 2.0 ** -24                                          # half a float32 ulp of 1
FILL = 7                                                  # what the tests put into the plates buffer before a call
R_MAX = [45, 60, 45]


def colour_tolerance(row):
    """How far the device may lie from the restatement on a 0..1 image for a row with D != 0.  The two means differ by at most
    one float32 ulp of mu (mu <= 255), which moves k = D mu + e by that times the row-sum of |D|; evaluating k (6 roundings at
    the magnitude Mk = sum |D| 255 + |e|) can turn that into up to 12 EPS Mk more; lin = A Q + k rounds once more at its own
    magnitude; the three operations after the division by 255 round at the magnitude of fg."""
    r = pr.unpack(row)
    D, A, e = np.abs(r['D'].astype(np.float64)), np.abs(r['A'].astype(np.float64)), np.abs(r['e'].astype(np.float64))
    mk = (D.sum(axis=1) * 255 + e).max()
    lin = (A.sum(axis=1) * 255).max() + mk
    return (float(np.spacing(np.float32(255))) * D.sum(axis=1).max() + 12 * EPS * mk + 2 * EPS * lin) / 255 + 3 * 2 * EPS * max(lin / 255, 1.0)


def device_plates(cuda, bg, glyphs, rows, alias=False):
    """-> (out (N,3,H,W) float32 ndarray, plates (N,160,380,4) uint8 ndarray, the three status codes)."""
    import torch
    lib = L.load()
    N, _, H, W = bg.shape
    bg_d = torch.from_numpy(np.ascontiguousarray(bg, np.float32)).to(cuda)
    glyphs_d = torch.from_numpy(np.ascontiguousarray(glyphs)).to(cuda)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(cuda)
    plates = torch.full((N, 160, 380, 4), FILL, dtype=torch.uint8, device=cuda)
    work = torch.empty(lib.yolo_plate_workspace_bytes(N, H, W), dtype=torch.uint8, device=cuda)
    out = bg_d if alias else torch.full_like(bg_d, -7.0)
    rc0 = lib.yolo_plate_compose(L.ptr(glyphs_d), L.ptr(rows_d), L.ptr(plates), N, L.stream_ptr())
    rc1 = lib.yolo_plate_stats(L.ptr(plates), L.ptr(rows_d), L.ptr(work), N, H, W, L.stream_ptr())
    rc2 = lib.yolo_plate_render(L.ptr(bg_d), L.ptr(plates), L.ptr(rows_d), L.ptr(work), L.ptr(out), N, H, W, L.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), plates.cpu().numpy(), (rc0, rc1, rc2)


def _bg(seed, N, H, W):
    return (np.random.default_rng(seed).random((N, 3, H, W)) * 1.3 - 0.15).astype(np.float32)          # (out of range: the clip works)


def _colour(seed):
    random.seed(seed); np.random.seed(seed)
    return render.ColorAugmenter(brightness=0.7, contrast=0.7, saturation=0.7, hue=1.0, pca_noise=0.1).affine()


def _row(ids, quad, H, W, sigma=0.0, noise=0.0, key=(0, 0), colour=None, has=1):
    """A row for a plate whose corners (bottom-right, bottom-left, top-left, top-right) lie on the continuous canvas points `quad`."""
    m = pr.quad_map(quad, H, W, render.homography, render.LP_CORNERS)
    w0, w1 = render.blur_weights(sigma)
    A, D, e = colour if colour is not None else (None, None, None)
    return pr.make_row(ids, m, pr.window(m.astype(np.float32).astype(np.float64), H, W), key, pr.noise_scale(noise) if noise else 0.0, w0, w1, A, D, e, has)


IDS = ([10, 21, 33, 0, 9, 5, 8], [15, 11, 30, 3, 3, 7, 1], [33, 10, 12, 9, 0, 2, 6], [20, 25, 17, 1, 8, 6, 5], [13, 29, 22, 7, 2, 0, 9])


def _six(H, W):
    """no plate; fronto-parallel, most of the canvas; strongly projective; across the left and top edges; blur and noise; blur,
    noise and every colour stage."""
    h, w = float(H), float(W)
    return np.stack([
        _row(IDS[0], [[w - 3, h - 5], [3, h - 5], [3, 5], [w - 3, 5]], H, W, has=0),
        _row(IDS[0], [[w - 3.25, h - 5.5], [3.5, h - 5.5], [3.5, 5.25], [w - 3.25, 5.25]], H, W),
        _row(IDS[1], [[w - 4, h - 2], [8, 0.62 * h], [8, 0.38 * h], [w - 4, 2]], H, W),
        _row(IDS[2], [[0.5 * w, 0.45 * h], [-8, 0.4 * h], [-10, -6], [0.46 * w, -4]], H, W),
        _row(IDS[3], [[w - 6, h - 4], [7, h - 9], [5, 8], [w - 9, 3]], H, W, sigma=0.6, noise=5.0, key=(0x1234abcd, 77)),
        _row(IDS[4], [[w - 5, h - 8], [4, h - 3], [9, 4], [w - 7, 9]], H, W, sigma=0.45, noise=5.0, key=(5, 0xfedcba98), colour=_colour(3))])


@pytest.fixture(scope='module')
def gen(tmp_path_factory):
    root = tmp_path_factory.mktemp('plates') / 'fonts'
    pr.write_fonts(str(root))
    return render.LPGenerator(64, 96, str(root), pr.CAMERA)


@pytest.fixture(scope='module')
def reference(gen):
    """The restatement of the six-image batch on both canvases, computed once."""
    out = {}
    for H, W in CANVASES:
        bg, rows = _bg(2, 6, H, W), _six(H, W)
        plates = pr.compose(gen.glyph_atlas(), rows, FILL)
        quiet = rows.copy()
        quiet[:, 14] = 0
        cover = (pr.render(bg, plates, quiet, return_parts=True)[2] > 0).reshape(6, -1).mean(axis=1)
        out[(H, W)] = (bg, rows, plates, pr.render(bg, plates, rows), cover)
    return out


def test_compose_equals_pils_paste(cuda, gen):
    """Four plates byte for byte against draw_LP's PIL image; a has == 0 row and one with glyph id 34 leave their plates alone."""
    np.random.seed(6)
    want, rows = [], []
    for _ in range(4):
        plate, _, glyphs = gen.draw_LP()
        want.append(np.asarray(plate))
        rows.append(pr.make_row([g[0] for g in glyphs], np.eye(3).reshape(-1), [0, 0, 0, 0]))
    rows.append(pr.make_row(IDS[0], np.eye(3).reshape(-1), [0, 0, 0, 0], has=0))
    rows.append(pr.make_row([10, 11, 34, 1, 2, 3, 5], np.eye(3).reshape(-1), [0, 0, 0, 0]))
    rows = np.stack(rows)
    _, plates, rcs = device_plates(cuda, np.zeros((6, 3, 32, 48), np.float32), gen.glyph_atlas(), rows)
    assert rcs == (L.OK, L.OK, L.OK)
    assert want[0].shape == (160, 380, 4) and len({w.tobytes() for w in want}) == 4
    for n in range(4):
        assert np.array_equal(plates[n], want[n]), n
    assert (plates[4:] == FILL).all()
    assert np.array_equal(plates, pr.compose(gen.glyph_atlas(), rows, FILL))
    soft = (plates[0][..., 3] > 0) & (plates[0][..., 3] < 255)
    assert soft.any()                                                           # (alpha was pasted, not blended)


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_batch_against_the_restatement(cuda, gen, reference, hw):
    bg, rows, plates, want, cover = reference[hw]
    got, got_plates, rcs = device_plates(cuda, bg, gen.glyph_atlas(), rows)
    assert rcs == (L.OK, L.OK, L.OK) and np.array_equal(got_plates, plates)
    tol = colour_tolerance(rows[5])
    for n in range(6):
        err = float(np.abs(got[n].astype(np.float64) - want[n]).max())
        print('%dx%d image %d: max |device - restatement| = %.3g, the plate covers %.0f %% of the canvas' % (hw + (n, err, 100 * cover[n])))
        assert (cover[n] == 0) if n == 0 else (cover[n] > 0.03)
    print('tolerance for the row with D != 0: %.3g' % tol)
    assert np.array_equal(got[0], np.clip(bg[0], 0, 1))
    assert np.abs(rows[:5, 36:45].view(np.float32)).max() == 0 and np.abs(rows[5, 36:45].view(np.float32)).max() > 0
    assert np.array_equal(got[:5], want[:5])                                    # D == 0: bit-equal by construction
    assert float(np.abs(got[5].astype(np.float64) - want[5]).max()) <= tol
    assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
@pytest.mark.parametrize('noise', [True, False], ids=['noise', 'quiet'])
def test_widening_the_window_changes_no_bit(cuda, gen, reference, hw, noise):
    """(The statistics pass walks the canvas in an order that does not depend on the window, and a pixel outside the plate's
    footprint samples exact zeros: the same sums, the same bits.)"""
    bg, rows, _, _, _ = reference[hw]
    rows = rows.copy()
    if not noise:
        rows[:, 14] = 0
    wide = rows.copy()
    wide[:, 8:12] = [0, 0, hw[1], hw[0]]
    narrow = device_plates(cuda, bg, gen.glyph_atlas(), rows)[0]
    whole = device_plates(cuda, bg, gen.glyph_atlas(), wide)[0]
    assert np.array_equal(narrow, whole)
    wide[:, 8:12] = [-5, -9, hw[1] + 40, hw[0] + 3]                             # a window wider than the canvas is clipped to it
    assert np.array_equal(device_plates(cuda, bg, gen.glyph_atlas(), wide)[0], whole)


def test_two_calls_are_bit_identical_and_out_may_alias_bg(cuda, gen, reference):
    for hw in CANVASES:
        bg, rows, _, _, _ = reference[hw]
        first = device_plates(cuda, bg, gen.glyph_atlas(), rows)[0]
        assert np.array_equal(first, device_plates(cuda, bg, gen.glyph_atlas(), rows)[0])
        assert np.array_equal(first, device_plates(cuda, bg, gen.glyph_atlas(), rows, alias=True)[0])


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_rows_without_a_front_side_render_as_background_or_haze(cuda, gen, hw):
    """m6..m8 = 0 (den = 0 everywhere) and a NaN in m8: S = 0, so without noise the image is clip(bg), and with noise it is the
    haze of the restatement -- defined behaviour, bit for bit (D = 0)."""
    H, W = hw
    good = _row(IDS[1], [[W - 3.0, H - 5.0], [3, H - 5.0], [3, 5], [W - 3.0, 5]], H, W, sigma=0.5)
    rows = np.stack([good] * 4)
    rows[:, 8:12] = [0, 0, W, H]
    fl = rows.view(np.float32)
    fl[0, 22:25], fl[2, 22:25] = 0, 0
    fl[1, 24], fl[3, 24] = np.nan, np.nan
    fl[2:, 14] = pr.noise_scale(5.0)
    rows[2:, 12:14] = [99, 3]
    bg = _bg(9, 4, H, W)
    got, plates, rcs = device_plates(cuda, bg, gen.glyph_atlas(), rows)
    assert rcs == (L.OK, L.OK, L.OK)
    assert np.array_equal(got[:2], np.clip(bg[:2], 0, 1))
    want = pr.render(bg, plates, rows)
    assert np.array_equal(got, want)
    assert not np.array_equal(want[2], np.clip(bg[2], 0, 1)) and not np.array_equal(want[3], np.clip(bg[3], 0, 1))


def test_add_device_end_to_end(cuda, gen):
    """LPGenerator.add_device with everything on: what it returns is the restatement of the rows draw_params makes under the
    same seed (the rows, the labels and the atlas reach the device as they were made); out=imgs draws in place."""
    import torch
    H, W = 64, 96
    bg = _bg(8, 6, H, W)
    np.random.seed(15); random.seed(15)
    img, lab = gen.add_device(torch.from_numpy(bg).to(cuda), R_MAX, add_rate=0.8)
    np.random.seed(15); random.seed(15)
    lab_h, rows = gen.draw_params(6, H, W, R_MAX, add_rate=0.8)
    inplace = torch.from_numpy(bg).to(cuda)
    np.random.seed(15); random.seed(15)
    out2, _ = gen.add_device(inplace, R_MAX, add_rate=0.8, out=inplace)
    torch.cuda.synchronize()
    assert out2 is inplace and torch.equal(out2, img)
    want = pr.render(bg, pr.compose(gen.glyph_atlas(), rows), rows)
    tol = max(colour_tolerance(r) for r in rows[rows[:, 0] == 1])
    err = float(np.abs(img.cpu().numpy().astype(np.float64) - want).max())
    print('add_device: max |device - restatement| = %.3g (tolerance %.3g)' % (err, tol))
    assert err <= tol and np.array_equal(lab.cpu().numpy(), lab_h) and tuple(lab.shape) == (6, 1, 10)
    assert 3 <= (rows[:, 0] == 1).sum() < 6 and np.abs(rows[:, 36:45].view(np.float32)).max() > 0          # (plates, a no-plate image, a contrast term)
    with pytest.raises(ValueError):
        gen.add_device(torch.from_numpy(bg), R_MAX)
    with pytest.raises(ValueError):
        gen.add_device(torch.from_numpy(bg).to(cuda), R_MAX, out=torch.empty((6, 3, H, W + 1), device=cuda))


def test_render_device_then_add_device_feeds_a_train_step(cuda, gen, tmp_path):
    """The whole feed on the device: RenderCar.render_device draws the cars, LPGenerator.add_device the plates onto its output,
    and one Trainer.train_step of the micro CarLPNet takes both label sets; the losses are finite."""
    import torch
    import render_ref as rr
    from oracle import graph as og
    from yolo_amd.net import CarLPNet
    from yolo_amd.train import Trainer
    spec = dict(og.spec_micro(), LP_slice_point=[1, 3, 4, 7, 10], LP_r_max=R_MAX)
    size = (64, 96)
    P = og.init_params(og.build_graph(spec), seed=0, bn='random')
    net = CarLPNet(spec, dtype='f32', device=cuda).load_params(P)
    tr = Trainer(net, size, lp_r_max=spec['LP_r_max'])
    rr.write_sprite_dir(str(tmp_path / 'png'), size=(60, 100))
    cars = render.RenderCar(size[0], size[1], [[90.0 * i, 0.0] for i in range(4)], str(tmp_path / 'png'), device=cuda)
    bg = torch.rand((4, 3) + size, device=cuda) * 255
    np.random.seed(2); random.seed(2)
    x, lab = cars.render_device(bg, 'train')
    x, lpl = gen.add_device(x, spec['LP_r_max'], add_rate=0.75, out=x)
    losses = tr.train_step(x, lab, lp_labels=lpl)
    torch.cuda.synchronize()
    assert tuple(lab.shape) == (4, 1, 10) and tuple(lpl.shape) == (4, 1, 10) and bool((lpl[:, 0, 0] == 1).any())
    assert bool(torch.isfinite(losses).all()) and float(losses.sum()) > 0
