"""The OCR data path on the device (csrc/ocr_data.hip): the plate renderer against its numpy restatement (tests/ocr_render_ref.py)
and, for the geometry, against the PIL route; yolo_ocr_targets, yolo_ocr_loss_fwd_bwd and yolo_ocr_score against
tests/ocr_loss_ref.py; OCRValidator against the sum of its parts.  Canvases 32 x 48 (16-byte accesses), 30 x 45 (scalar accesses, a
tail thread) and 40 x 100 (more than one 32 x 32 tile in each direction)."""
import math
import random

import numpy as np
import pytest

import ocr_loss_ref as olr
import ocr_render_ref as orr
import plate_ref as pr
from yolo_amd import lib as L
from yolo_amd import render

pytestmark = pytest.mark.gpu
CANVASES = [(32, 48), (30, 45), (40, 100)]
EPS = 2.0 ** -24                                          # half a float32 ulp of 1
FILL = 7
IDS = ([10, 21, 33, 0, 9, 5, 8], [15, 11, 30, 3, 3, 7, 1], [33, 10, 12, 9, 0, 2, 6], [20, 25, 17, 1, 8, 6, 5], [13, 29, 22, 7, 2, 0, 9])
BG_MAX = 1.15                                             # the test backgrounds reach 1.15 * 255 (out of range: the clip works)


def colour_tolerance(row):
    """How far the device may lie from the restatement on a 0..1 image for a row with D != 0: the bound of tests/test_gpu_plates.py
    rederived for this pipeline.  Q is bit-equal on both sides (it does not depend on the mean), and so is the background term
    (bg (1 - mask)) / 255.  The two means differ by at most one float32 ulp of mu (mu <= 255): the device adds tile sums, the
    restatement one float64 sum.  That moves k = D mu + e by ulp(255) times the row-sum of |D|; evaluating k (6 roundings at the
    magnitude Mk = sum |D| 255 + |e|) can turn a different input into up to 12 EPS Mk more; lin = A Q + k rounds once more at its
    own magnitude (2 EPS lin).  All that is divided by 255.  Then three operations see a different operand and may round another
    way, each by an ulp (2 EPS) of its result's magnitude: the division lin / 255 and the product fg * mask (mask <= 1) at
    |fg| = lin / 255, and the sum with the background term at lin / 255 + BG_MAX."""
    r = pr.unpack(row)
    D, A, e = np.abs(r['D'].astype(np.float64)), np.abs(r['A'].astype(np.float64)), np.abs(r['e'].astype(np.float64))
    mk = (D.sum(axis=1) * 255 + e).max()
    lin = (A.sum(axis=1) * 255).max() + mk
    return (float(np.spacing(np.float32(255))) * D.sum(axis=1).max() + 12 * EPS * mk + 2 * EPS * lin) / 255 + 2 * EPS * (3 * lin / 255 + BG_MAX)


def device_ocr(cuda, bg, glyphs, rows, taps, bg_unit=False, alias=False, guard=64):
    """-> dict(out (N,3,H,W) ndarray, band: the guard elements before and after out, work: the workspace bytes with `guard`
    bytes after them, rc: the three status codes).  out sits in a NaN-filled buffer, the workspace is poisoned with 0xFF."""
    import torch
    lib = L.load()
    N, _, H, W = bg.shape
    bg_d = torch.from_numpy(np.ascontiguousarray(bg, np.float32)).to(cuda)
    glyphs_d = torch.from_numpy(np.ascontiguousarray(glyphs)).to(cuda)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(cuda)
    taps_d = torch.from_numpy(np.ascontiguousarray(taps, np.int32)).to(cuda)
    plates = torch.full((N, 160, 380, 4), FILL, dtype=torch.uint8, device=cuda)
    nbytes = lib.yolo_ocr_plate_workspace_bytes(N, H, W)
    work = torch.full((nbytes + guard,), 0xFF, dtype=torch.uint8, device=cuda)
    if alias:
        buf, out = None, bg_d
    else:
        buf = torch.full((guard + bg_d.numel() + guard,), float('nan'), dtype=torch.float32, device=cuda)
        out = buf[guard:guard + bg_d.numel()].view(bg_d.shape)
    st = L.stream_ptr()
    rc0 = lib.yolo_plate_compose(L.ptr(glyphs_d), L.ptr(rows_d), L.ptr(plates), N, st)
    rc1 = lib.yolo_ocr_plate_blur(L.ptr(plates), L.ptr(rows_d), L.ptr(taps_d), L.ptr(work), N, H, W, st)
    rc2 = lib.yolo_ocr_plate_render(L.ptr(bg_d), L.ptr(rows_d), L.ptr(work), L.ptr(out), N, H, W, int(bg_unit), st)
    torch.cuda.synchronize()
    band = None if alias else np.concatenate([buf[:guard].cpu().numpy(), buf[-guard:].cpu().numpy()])
    return dict(out=out.cpu().numpy(), band=band, work=work.cpu().numpy(), rc=(rc0, rc1, rc2))


def _bg(seed, N, H, W, unit=False):
    b = (np.random.default_rng(seed).random((N, 3, H, W)) * 1.3 - 0.15).astype(np.float32)
    return b if unit else b * np.float32(255)


def _colour(seed):
    random.seed(seed); np.random.seed(seed)
    return render.ColorAugmenter(brightness=0.5, contrast=0.5, saturation=0.3, hue=1.0, pca_noise=1.0).affine()


def _map(scale, deg, cx, cy):
    """Canvas pixel index -> plate texel index for a plate `scale` times 380 x 160, turned by deg, its centre at continuous (cx, cy)."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    half = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
    back = np.array([[c / scale, s / scale, 190.0 - (c * cx + s * cy) / scale], [-s / scale, c / scale, 80.0 - (-s * cx + c * cy) / scale], [0, 0, 1.0]])
    return np.linalg.inv(half) @ back @ half


def _footprint(m, margin):
    """The bound of the plate's pre-image on the canvas, `margin` px wider: outside it every S the blur of that reach touches is 0."""
    F = np.linalg.inv(m)
    xs, ys = np.float64([-1, 380, 380, -1]), np.float64([-1, -1, 160, 160])
    px, py = F[0, 0] * xs + F[0, 1] * ys + F[0, 2], F[1, 0] * xs + F[1, 1] * ys + F[1, 2]
    return [int(math.floor(px.min())) - margin, int(math.floor(py.min())) - margin, int(math.ceil(px.max())) + 1 + margin, int(math.ceil(py.max())) + 1 + margin]


def _batch(H, W):
    """no plate;  T = 0;  T = 1 with noise;  T = 5 with noise and every colour stage (D != 0);  T = 24 on a window narrower than the
    halo, which leaves the canvas on every side the canvas allows;  T = 24 on a window that spans the tiles;  a plate across the
    left and top edges (T = 1, the window reaches outside the canvas);  T = 0 with noise.  -> (rows (8,48), taps (8,32))."""
    h, w = float(H), float(W)
    scale = 0.7 * w / 380.0
    mid = _map(scale, 6.0, w / 2, h / 2)
    edge = _map(scale, -9.0, 0.22 * w, 0.15 * h)
    rows = [pr.make_row(IDS[0], mid, _footprint(mid, 2), has=0),
            pr.make_row(IDS[0], mid, _footprint(mid, 2)),
            pr.make_row(IDS[1], _map(scale, -4.0, w / 2 + 1.3, h / 2 - 0.6), _footprint(mid, 4), key=(0x1234abcd, 77), s=pr.noise_scale(10.0)),
            pr.make_row(IDS[2], mid, _footprint(mid, 8), key=(5, 0xfedcba98), s=pr.noise_scale(10.0), A=_colour(3)[0], D=_colour(3)[1], e=_colour(3)[2]),
            pr.make_row(IDS[3], mid, [min(W // 2 - 7, 17), H // 2 - 5, min(W // 2 - 7, 17) + 13, H // 2 + 4], key=(9, 9), s=pr.noise_scale(5.0)),
            pr.make_row(IDS[4], mid, [3, 2, W - 2, H - 3]),
            pr.make_row(IDS[1], edge, [-6, -4, int(0.6 * w), int(0.55 * h)]),
            pr.make_row(IDS[2], mid, _footprint(mid, 1), key=(31, 7), s=pr.noise_scale(10.0))]
    taps = [orr.make_taps(0), orr.make_taps(0), orr.make_taps(1, sigma=0.5), orr.make_taps(5, sigma=1.7), orr.make_taps(24, sigma=8.0),
            orr.make_taps(24, sigma=7.0), orr.make_taps(1, sigma=0.4), orr.make_taps(0)]
    return np.stack(rows), np.stack(taps)


@pytest.fixture(scope='module')
def fonts(tmp_path_factory):
    root = tmp_path_factory.mktemp('ocr') / 'fonts'
    pr.write_fonts(str(root))
    return str(root)


@pytest.fixture(scope='module')
def gen(fonts):
    return render.LPGenerator(160, 384, fonts, pr.CAMERA)


@pytest.fixture(scope='module')
def reference(gen):
    """The restatement of the eight-image batch on the three canvases, computed once and left unchanged."""
    out = {}
    for H, W in CANVASES:
        bg, (rows, taps) = _bg(2, 8, H, W), _batch(H, W)
        plates = pr.compose(gen.glyph_atlas(), rows, FILL)
        want, mus, masks, Q = orr.render(bg, plates, rows, taps, return_parts=True)
        out[(H, W)] = dict(bg=bg, rows=rows, taps=taps, plates=plates, want=want, masks=masks, Q=Q)
    return out


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_batch_against_the_restatement(cuda, gen, reference, hw):
    """Bit-equal where D == 0, within colour_tolerance for the row with D != 0; the NaN bands around out stay NaN; of the
    poisoned workspace exactly what the header names is written: every tile sum (0 for a no-plate image and for a tile outside
    the window), Q inside the windows of images with a plate (bit-equal to the restated Q), no other byte."""
    H, W = hw
    ref = reference[hw]
    rows, taps, bg = ref['rows'], ref['taps'], ref['bg']
    got = device_ocr(cuda, bg, gen.glyph_atlas(), rows, taps)
    assert got['rc'] == (L.OK, L.OK, L.OK)
    out, want = got['out'], ref['want']
    tol = colour_tolerance(rows[3])
    for n in range(8):
        err = float(np.abs(out[n].astype(np.float64) - want[n]).max())
        cover = float((ref['masks'][n] > 0).mean())
        print('%dx%d image %d: max |device - restatement| = %.3g, the mask covers %.0f %% of the canvas' % (hw + (n, err, 100 * cover)))
        assert (cover == 0) if n == 0 else (cover > 0.02)
    print('tolerance for the row with D != 0: %.3g' % tol)
    assert np.array_equal(out[0], np.clip(bg[0] / np.float32(255), 0, 1))
    keep = [n for n in range(8) if n != 3]
    assert np.abs(rows[keep, 36:45].view(np.float32)).max() == 0 and np.abs(rows[3, 36:45].view(np.float32)).max() > 0
    assert np.array_equal(out[keep], want[keep])                               # D == 0: bit-equal by construction
    assert float(np.abs(out[3].astype(np.float64) - want[3]).max()) <= tol
    assert out.min() >= 0 and out.max() <= 1 and np.isnan(got['band']).all() and got['band'].size == 128
    # the T = 24 rows: the halo is wider than the narrow window and leaves the canvas
    l, t, r, b = pr.window_of(pr.unpack(rows[4]), H, W)
    assert r - l < 24 and b - t < 24 and t - 24 < 0 and b + 24 > H and l - 24 < 0 and (r + 24 > W or W == 100)
    # the workspace
    sums, q_off, total, tiles = orr.workspace_layout(8, H, W)
    work = got['work']
    assert work.size == total + 64 and (work[total:] == 0xFF).all() and (work[sums:q_off] == 0xFF).all()
    part = work[:sums].view(np.float64).reshape(8, tiles, 3)
    Qd = work[q_off:total].view(np.uint32).reshape(8, H, W, 4)
    tx = (W + 31) // 32
    for n in range(8):
        l, t, r, b = pr.window_of(pr.unpack(rows[n]), H, W)
        inside = np.zeros((H, W), bool)
        if n != 0:
            inside[t:b, l:r] = True
        assert (Qd[n][~inside] == 0xFFFFFFFF).all(), n
        assert np.array_equal(Qd[n][inside].view(np.float32), ref['Q'][n][inside]), n
        for p in range(tiles):
            ty, txx = divmod(p, tx)
            tile = ref['Q'][n][32 * ty:32 * ty + 32, 32 * txx:32 * txx + 32, :3].astype(np.float64).sum(axis=(0, 1))
            np.testing.assert_allclose(part[n, p], tile, rtol=1e-12, atol=0)


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_unit_background_alias_and_repeat(cuda, gen, reference, hw):
    """bg_unit = 1 against the restatement fed a 0..1 background; out may alias bg; two calls give the same bits."""
    ref = reference[hw]
    rows, taps = ref['rows'], ref['taps']
    first = device_ocr(cuda, ref['bg'], gen.glyph_atlas(), rows, taps)['out']
    assert np.array_equal(first, device_ocr(cuda, ref['bg'], gen.glyph_atlas(), rows, taps)['out'])
    assert np.array_equal(first, device_ocr(cuda, ref['bg'], gen.glyph_atlas(), rows, taps, alias=True)['out'])
    ubg = _bg(4, 8, hw[0], hw[1], unit=True)
    want = orr.render(ubg, ref['plates'], rows, taps, bg_unit=True)
    for alias in (False, True):
        got = device_ocr(cuda, ubg, gen.glyph_atlas(), rows, taps, bg_unit=True, alias=alias)['out']
        keep = [n for n in range(8) if n != 3]
        assert np.array_equal(got[keep], want[keep])
        assert float(np.abs(got[3].astype(np.float64) - want[3]).max()) <= colour_tolerance(rows[3])
    assert not np.array_equal(want, ref['want'])


@pytest.mark.parametrize('hw', CANVASES, ids=lambda hw: '%dx%d' % hw)
def test_widening_the_window_over_zeros_changes_no_bit(cuda, gen, hw):
    """Noise off, windows that hold the plate's footprint and the blur's reach (T = 0, 1, 5): the pixels a wider window adds have
    P = 0 (a sum of zeros), so mask = 0 and the tile sums gain zeros only -- the same bits, whole canvas or beyond it."""
    H, W = hw
    m = _map(min(0.55 * W, 1.1 * H) / 380.0, 5.0, W / 2.0, H / 2.0)
    col = _colour(8)
    rows = np.stack([pr.make_row(IDS[k], m, _footprint(m, T + 1), A=col[0], D=col[1], e=col[2]) for k, T in enumerate((0, 1, 5))])
    taps = np.stack([orr.make_taps(0), orr.make_taps(1, sigma=0.5), orr.make_taps(5, sigma=1.6)])
    for r in rows:
        l, t, rr, b = r[8:12]
        assert 0 < l and 0 < t and rr < W and b < H                            # (there is something to widen over)
    bg = _bg(6, 3, H, W)
    narrow = device_ocr(cuda, bg, gen.glyph_atlas(), rows, taps)['out']
    wide = rows.copy()
    wide[:, 8:12] = [0, 0, W, H]
    whole = device_ocr(cuda, bg, gen.glyph_atlas(), wide, taps)['out']
    assert np.array_equal(narrow, whole) and not np.array_equal(narrow, np.clip(bg / np.float32(255), 0, 1))
    wide[:, 8:12] = [-5, -9, W + 40, H + 3]                                     # a window wider than the canvas is clipped to it
    assert np.array_equal(device_ocr(cuda, bg, gen.glyph_atlas(), wide, taps)['out'], whole)


def test_render_device_end_to_end(cuda, gen):
    """LPGenerator.render_device at 160 x 384, B = 6, everything on, against the restatement fed the draw_ocr_params of the same
    seed; the labels and the orders reach the device bit for bit; out=bg draws in place."""
    import torch
    H, W = 160, 384
    bg = _bg(8, 6, H, W)
    np.random.seed(15); random.seed(15)
    img, lab = gen.render_device(torch.from_numpy(bg).to(cuda))
    order = gen.ocr_order
    np.random.seed(15); random.seed(15)
    lab_h, rows, taps, orders = gen.draw_ocr_params(6, H, W)
    inplace = torch.from_numpy(bg).to(cuda)
    np.random.seed(15); random.seed(15)
    out2, _ = gen.render_device(inplace, out=inplace)
    torch.cuda.synchronize()
    assert out2 is inplace and torch.equal(out2, img)
    want = orr.render(bg, pr.compose(gen.glyph_atlas(), rows), rows, taps)
    tol = max(colour_tolerance(r) for r in rows)
    err = float(np.abs(img.cpu().numpy().astype(np.float64) - want).max())
    print('render_device: max |device - restatement| = %.3g (tolerance %.3g); T = %s' % (err, tol, taps[:, 0].tolist()))
    assert err <= tol
    assert np.array_equal(lab.cpu().numpy(), lab_h) and tuple(lab.shape) == (6, 7, 3) and np.array_equal(order.cpu().numpy(), orders)
    assert np.abs(rows[:, 36:45].view(np.float32)).max() > 0 and taps[:, 0].max() >= 12 and (rows[:, 14].view(np.float32) > 0).all()
    assert float(np.abs(want - np.clip(bg / np.float32(255), 0, 1)).max()) > 0.3                          # (plates were drawn)
    with pytest.raises(ValueError):
        gen.render_device(torch.from_numpy(bg))
    with pytest.raises(ValueError):
        gen.render_device(torch.from_numpy(bg).to(cuda), out=torch.empty((6, 3, H, W + 1), device=cuda))


def test_render_device_geometry_against_the_pil_route(cuda, fonts):
    """Blur, noise and colour off, so both routes make the same draws for every image: the bounding box of alpha > 0.5 of the
    device's Q (read from the workspace, inside the windows) against the PIL route's mask, within 1.5 px per edge -- one for PIL's
    integer sizes at every stage (resize, shear and rotate each round their image's size), half for the sampling."""
    import torch
    H, W = 160, 384
    g = render.LPGenerator(H, W, fonts, pr.CAMERA, augment=False)
    np.random.seed(33); random.seed(33)
    _, mask, lab_h = g.render_host(6, H, W, G=0.0, noise=0.0)
    np.random.seed(33); random.seed(33)
    _, lab = g.render_device(torch.zeros((6, 3, H, W), device=cuda), G=0.0, noise=0.0)
    np.random.seed(33); random.seed(33)
    _, rows, taps, _ = g.draw_ocr_params(6, H, W, G=0.0, noise=0.0)
    torch.cuda.synchronize()
    assert np.array_equal(lab.cpu().numpy(), lab_h) and (taps[:, 0] == 0).all()
    work = g._device_state['ocr_work'][(6, H, W)].cpu().numpy()
    _, q_off, total, _ = orr.workspace_layout(6, H, W)
    Q = work[q_off:total].view(np.float32).reshape(6, H, W, 4)
    for n in range(6):
        l, t, r, b = rows[n, 8:12]
        alpha = np.zeros((H, W), np.float32)
        alpha[t:b, l:r] = Q[n, t:b, l:r, 3] / 255
        boxes = []
        for a in (alpha, mask[n, 0]):
            ys, xs = np.nonzero(a > 0.5)
            boxes.append([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1])
        print('image %d: alpha > 0.5 box device %s PIL %s' % (n, boxes[0], boxes[1]))
        assert np.abs(np.float64(boxes[0]) - np.float64(boxes[1])).max() <= 1.5, n


# ---- targets -----------------------------------------------------------------------------------------------------------------
def _labels(rng, B, nobj, Wp):
    """Labels that hang off both ends, overlap, and have class < 0 rows; no L * Wp within 1e-4 of a half-integer."""
    lab = -np.ones((B, nobj, 3), np.float32)
    for b in range(B):
        for k in range(nobj):
            if rng.random() < 0.2:
                continue
            while True:
                c, wd = rng.uniform(-0.1, 1.1), rng.uniform(0.04, 0.5)
                row = np.float32([rng.integers(0, 70), c - wd / 2, c + wd / 2])
                if np.abs((row[1:].astype(np.float64) * Wp) % 1.0 - 0.5).min() > 1e-4:
                    break
            lab[b, k] = row
    if B * nobj >= 3:
        lab[0, 0] = [3, -0.3, 1.4]                                              # off both ends at once
    return lab


def _device_targets(cuda, lab, order, Wp):
    import torch
    from yolo_amd import ocr
    o = None if order is None else torch.from_numpy(order).to(cuda)
    s, c = ocr.ocr_targets(torch.from_numpy(lab).to(cuda), Wp, o)
    torch.cuda.synchronize()
    return s.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize('B, nobj, Wp', [(1, 1, 1), (3, 7, 24), (65, 16, 25), (3, 16, 24), (65, 7, 1), (1, 7, 25)])
def test_targets_against_the_restatement(cuda, B, nobj, Wp):
    """class_y exactly; score_y within 4 x the distance between the float32 and the float64 restatement, of the float64 one."""
    rng = np.random.default_rng(100 * B + 10 * nobj + Wp)
    lab = _labels(rng, B, nobj, Wp)
    orders = [None, np.stack([rng.permutation(nobj) for _ in range(B)]).astype(np.int32), np.tile(np.arange(nobj, dtype=np.int32)[::-1], (B, 1))]
    classes = []
    for order in orders:
        s64, c64 = olr.targets(lab, order, Wp, np.float64)
        s32, c32 = olr.targets(lab, order, Wp, np.float32)
        s, c = _device_targets(cuda, lab, order, Wp)
        yard, dist = float(np.abs(s32 - s64).max()), float(np.abs(s - s64).max())
        print('targets B %d nobj %d Wp %d: float32 restatement %.3g from float64, device %.3g' % (B, nobj, Wp, yard, dist))
        assert np.array_equal(c, c64) and np.array_equal(c32, c64) and c.dtype == np.int32
        assert dist <= 4 * yard
        assert np.array_equal(s == 0, c < 0) or (s[c >= 0] <= 0).any()          # zero exactly where no label covers
        classes.append(c)
    if nobj >= 7 and Wp > 1:
        assert not np.array_equal(classes[1], classes[2])                       # overlapping labels: the order decides
        assert (classes[0] >= 0).any() and ((classes[0] < 0).any() or nobj == 16 or B == 1)      # (sixteen labels cover every column)
    # an entry of `order` outside 0..nobj-1 is passed over
    bad = np.full((B, nobj), nobj, np.int32)
    s, c = _device_targets(cuda, lab, bad, Wp)
    assert (s == 0).all() and (c == -1).all()


# ---- losses ------------------------------------------------------------------------------------------------------------------
def _loss_case(rng, B, Wp, ncls, extreme=False):
    logits = (rng.standard_normal((B, Wp, 1 + ncls)) * 3).astype(np.float32)
    if extreme:
        flat = logits.reshape(-1)
        flat[rng.choice(flat.size, size=max(flat.size // 5, 4), replace=False)] = rng.choice(np.float32([30, -30, 100, -100]), size=max(flat.size // 5, 4))
    lab = _labels(rng, B, 7, Wp)
    lab[:, :, 0] = np.where(lab[:, :, 0] >= 0, lab[:, :, 0] % ncls, lab[:, :, 0])
    if B > 1:
        lab[1] = -1                                                             # an image without a label
    score_y, class_y = olr.targets(lab, None, Wp, np.float32)
    return logits, score_y, class_y


def _device_loss(cuda, logits, score_y, class_y, grad, sw=0.1, cw=1.0):
    import torch
    from yolo_amd import ocr
    out = ocr.ocr_loss(torch.from_numpy(logits).to(cuda), torch.from_numpy(score_y).to(cuda), torch.from_numpy(class_y).to(cuda), grad, sw, cw)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if grad else out.cpu().numpy()


@pytest.mark.parametrize('B, Wp, ncls, extreme', [(1, 1, 34, False), (3, 24, 34, False), (65, 25, 70, False), (3, 25, 1, False), (65, 24, 34, True),
                                                  (3, 24, 70, True), (1, 24, 1, False)])
def test_losses_against_the_restatement(cuda, B, Wp, ncls, extreme):
    """Losses and gradient within 4 x the distance between the float32 and the float64 restatement (the reference's arithmetic is
    float32; the factor covers another summation order and another expf / log1pf), of the float64 one.  dlogits = NULL leaves the
    losses as they are; an image without a label has class loss 0 and a zero class gradient; all finite at +-100."""
    import torch
    rng = np.random.default_rng(1000 * B + 10 * Wp + ncls + extreme)
    logits, score_y, class_y = _loss_case(rng, B, Wp, ncls, extreme)
    l64, g64 = olr.losses(logits, score_y, class_y, dtype=torch.float64, grad=True)
    l32, g32 = olr.losses(logits, score_y, class_y, dtype=torch.float32, grad=True)
    ld, gd = _device_loss(cuda, logits, score_y, class_y, True)
    only = _device_loss(cuda, logits, score_y, class_y, False)
    yl, dl = float(np.abs(l32 - l64).max()), float(np.abs(ld - l64).max())
    yg, dg = float(np.abs(g32 - g64).max()), float(np.abs(gd - g64).max())
    print('losses B %d Wp %d ncls %d%s: float32 restatement %.3g from float64, device %.3g; gradient %.3g, device %.3g'
          % (B, Wp, ncls, ' +-100' if extreme else '', yl, dl, yg, dg))
    assert ld.shape == (2, B) and gd.shape == logits.shape and np.isfinite(ld).all() and np.isfinite(gd).all()
    assert np.array_equal(only, ld)
    assert dl <= 4 * yl and dg <= 4 * yg
    if B > 1:
        assert (class_y[1] == -1).all() and ld[1, 1] == 0 and (gd[1, :, 1:] == 0).all() and ld[0, 1] > 0
    if extreme:
        assert np.abs(logits).max() == 100 and ld.max() > 1
    # other weights scale the two rows
    ld2 = _device_loss(cuda, logits, score_y, class_y, False, 1.0, 0.5)
    np.testing.assert_allclose(ld2[0], ld[0] * 10, rtol=1e-6)
    np.testing.assert_allclose(ld2[1], ld[1] * 0.5, rtol=1e-6)


# ---- score and validator -----------------------------------------------------------------------------------------------------
def _synthetic_logits(score_y, class_y, ncls=34):
    """The score logit is the logit of score_y (limited to +-30), the class logits a one-hot times 10 at class_y."""
    s = np.clip(score_y.astype(np.float64), 1e-13, 1 - 1e-13)
    logits = np.zeros(score_y.shape + (1 + ncls,), np.float32)
    logits[..., 0] = np.clip(np.log(s / (1 - s)), -30, 30)
    b, i = np.nonzero(class_y >= 0)
    logits[b, i, 1 + class_y[b, i]] = 10
    return logits


def _device_score(cuda, logits, labels, class_y, thr):
    import torch
    from yolo_amd import ocr
    lib = L.load()
    B, Wp, C = logits.shape
    lg = torch.from_numpy(logits).to(cuda)
    score = torch.empty((B, Wp), dtype=torch.float32, device=cuda)
    codes = torch.empty((B, Wp), dtype=torch.int32, device=cuda)
    count = torch.empty((B,), dtype=torch.int32, device=cuda)
    L.check(lib.yolo_ocr_decode(L.ptr(lg), None, L.ptr(score), L.ptr(codes), L.ptr(count), B, Wp, C - 1, thr, L.stream_ptr()), 'decode')
    counts = ocr.ocr_score(codes, count, torch.from_numpy(labels).to(cuda), torch.from_numpy(class_y).to(cuda), lg)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), codes.cpu().numpy(), count.cpu().numpy()


def test_score_on_targets_turned_into_logits(cuda, fonts):
    """Plates wholly inside the canvas, logits built from their own targets, read at 0.6: every plate matches, no character is
    wrong, every labelled column is right; and the counts equal the restated ones."""
    g = render.LPGenerator(160, 384, fonts, pr.CAMERA, augment=False)
    np.random.seed(77); random.seed(77)
    lab, _, _, orders = g.draw_ocr_params(160, 160, 384, noise=0.0)
    inside = (lab[:, :, 1:].min(axis=(1, 2)) >= 0) & (lab[:, :, 1:].max(axis=(1, 2)) <= 1)
    lab, orders = lab[inside], orders[inside]
    assert len(lab) >= 40
    score_y, class_y = olr.targets(lab, orders, 24, np.float32)
    logits = _synthetic_logits(score_y, class_y)
    counts, codes, count = _device_score(cuda, logits, lab, class_y, 0.6)
    assert np.array_equal(counts, olr.score_counts(codes, count, lab, class_y, logits))
    tot = counts.sum(axis=0)
    assert (counts[:, 0] == 7).all() and (counts[:, 1] == 7).all() and tot[2] == 0 and tot[3] == len(lab) and tot[4] == tot[5] > 0


def test_score_counts_by_hand(cuda):
    """One layout: seven glyphs 0.1 wide from 0.15 on, columns 0..3 free.  Clean; one wrong class at a peak; one peak missing; one
    extra peak in a free column; a label whose centre lies outside [0, 1) is no part of the truth (its column 23 is still
    labelled and read: one character too many); nothing predicted at all."""
    base = np.float32([[10 + k, 0.15 + 0.115 * k, 0.25 + 0.115 * k] for k in range(7)])
    lab = np.stack([base] * 6)
    lab[4, 6] = [5, 0.96, 1.1]                                                  # centre 1.03: not part of the text
    score_y, class_y = olr.targets(lab, None, 24, np.float32)
    logits = _synthetic_logits(score_y, class_y)
    cols = olr.peaks(score_y[0], 0.6)
    assert len(cols) == 7 and (class_y[0, :3] == -1).all()
    logits[1, cols[2], 1:] = 0
    logits[1, cols[2], 1 + 3] = 10                                              # reads '3' where 12 stands
    logits[2, class_y[2] == 14, 0] = -30                                        # the fifth glyph's columns: its peak is gone
    logits[3, 1, 0] = 5                                                         # a peak in column 1; its classes are all 0: argmax 0
    logits[5, :, 0] = -30
    counts, codes, count = _device_score(cuda, logits, lab, class_y, 0.6)
    assert np.array_equal(counts, olr.score_counts(codes, count, lab, class_y, logits))
    nlab = int((class_y[0] >= 0).sum())
    assert counts[0].tolist() == [7, 7, 0, 1, nlab, nlab]
    assert counts[1].tolist() == [7, 7, 1, 0, nlab, nlab - 1]
    assert counts[2].tolist() == [7, 6, 1, 0, nlab, nlab]
    assert counts[3].tolist() == [7, 8, 1, 0, nlab, nlab]
    assert counts[4].tolist() == [6, 7, 1, 0, int((class_y[4] >= 0).sum()), int((class_y[4] >= 0).sum())] and class_y[4, 23] == 5
    assert counts[5][:4].tolist() == [7, 0, 7, 0]


def test_refused_calls_write_nothing(cuda):
    """Shapes outside the limits come back YOLO_EUNSUPPORTED with the outputs as they were."""
    import torch
    lib = L.load()
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=cuda)
    counts = torch.full((2, 6), 99, dtype=torch.int32, device=cuda)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)
    for nobj, Wp in ((17, 24), (7, 65)):
        rc = lib.yolo_ocr_score(L.ptr(z(2, Wp)), L.ptr(z(2)), L.ptr(f(2, nobj, 3)), L.ptr(z(2, Wp)), L.ptr(f(2, Wp, 35)), L.ptr(counts), 2, nobj, Wp,
                                34, L.stream_ptr())
        assert rc == L.EUNSUPPORTED
    losses = torch.full((2, 2), 99.0, device=cuda)
    rc = lib.yolo_ocr_loss_fwd_bwd(L.ptr(f(2, 24, 35)), L.ptr(f(2, 24)), L.ptr(z(2, 24)), None, L.ptr(losses), 2, 24, 0, 0.1, 1.0, L.stream_ptr())
    assert rc == L.EINVAL
    torch.cuda.synchronize()
    assert (counts == 99).all() and (losses == 99).all()


def test_validator_is_the_sum_of_its_parts(cuda):
    """Two updates on a small randomly initialised OCRNet: result() equals the net, the decode at 0.2, the targets, the losses
    and the counts computed one by one and added up.  The bookkeeping is asserted, not the accuracy of a random net."""
    import torch
    from yolo_amd import ocr
    from yolo_amd.dense import OCRNet, PlateReader
    net = OCRNet(classes=34, num_init_features=16, growth_rate=8, block_config=[2, 3, 2], size=(52, 384), device=cuda)
    net.initialize(5)
    val = ocr.OCRValidator(net)
    assert val.reader.threshold == 0.2 and ocr.OCRValidator(PlateReader(net, 0.6), threshold=0.3).reader.threshold == 0.3
    rng = np.random.default_rng(12)
    tot_counts, tot_losses, n = np.zeros(6, np.int64), np.zeros(2, np.float64), 0
    for B in (3, 5):
        x = torch.from_numpy(rng.random((B, 3, 52, 384), dtype=np.float32)).to(cuda)
        lab_h = _labels(rng, B, 7, 24)
        lab_h[:, :, 0] = np.where(lab_h[:, :, 0] >= 0, lab_h[:, :, 0] % 34, lab_h[:, :, 0])
        lab = torch.from_numpy(lab_h).to(cuda)
        val.update(x, lab)
        _, codes, count = PlateReader(net, 0.2).read_device(x)
        lg = net.logits(x)
        assert tuple(lg.shape) == (B, 24, 35)
        score_y, class_y = ocr.ocr_targets(lab, 24)
        losses = ocr.ocr_loss(lg, score_y, class_y)
        counts = ocr.ocr_score(codes, count, lab, class_y, lg)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), olr.score_counts(codes.cpu().numpy(), count.cpu().numpy(), lab_h, class_y.cpu().numpy(), lg.cpu().numpy()))
        tot_counts += counts.cpu().numpy().astype(np.int64).sum(axis=0)
        tot_losses += losses.cpu().numpy().astype(np.float64).sum(axis=1)
        n += B
    res = val.result()
    assert res['n_plates'] == 8 and res['n_chars'] == tot_counts[0] > 0
    assert res['score_loss'] == pytest.approx(tot_losses[0] / n, rel=1e-12) and res['class_loss'] == pytest.approx(tot_losses[1] / n, rel=1e-12)
    assert res['plate_accuracy'] == tot_counts[3] / n and res['cer'] == tot_counts[2] / tot_counts[0]
    assert res['column_accuracy'] == tot_counts[5] / tot_counts[4] and np.isfinite(tot_losses).all()
    val.reset()
    assert val.result()['n_plates'] == 0 and math.isnan(val.result()['cer'])
