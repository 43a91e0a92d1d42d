"""The background kernels (csrc/background.hip: yolo_bg_stats + yolo_bg_render) against their numpy restatement
(tests/background_ref.py), against the image bytes themselves, and BackgroundBank.next_batch end to end.  Bank: noise images of
9 x 7, 37 x 53, 48 x 64 (three levels), 5 x 5 and 32 x 48; outputs 16 x 24 (W % 4 == 0: 16-byte stores) and 13 x 13 (scalar stores,
a tail thread, fewer rows than stat blocks)."""
import random

import numpy as np
import pytest

import background_ref as br
import render_ref as rr
from yolo_amd import background as bgm
from yolo_amd import lib as L
from yolo_amd import render

pytestmark = pytest.mark.gpu
ATOL = 255 * 2e-6  # tests/test_gpu_render_device.py's ATOL in 0..255 units: mu may differ from the restatement's by one float32 ulp
IDS = dict(ids=lambda hw: '%dx%d' % hw)


def device_bg(cuda, bank, rows, H, W, bank_bytes=None, pad=0, misalign=False):
    """-> (out (N,3,H,W) float32 ndarray, the two status codes).  pad: bytes of 255 appended to the bank's tensor (bank_bytes stays
    the bank's own size unless given); misalign: out is a view one float into a larger buffer."""
    import torch
    lib = L.load()
    N = len(rows)
    bank = np.ascontiguousarray(bank, np.uint8).reshape(-1)
    nb = bank.size if bank_bytes is None else bank_bytes
    bank_d = torch.from_numpy(np.concatenate([bank, np.full(pad, 255, np.uint8)])).to(cuda)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.int32)).to(cuda)
    work = torch.empty(lib.yolo_bg_workspace_bytes(N, H, W), dtype=torch.uint8, device=cuda)
    n = N * 3 * H * W
    buf = torch.full((n + 4,), -7.0, dtype=torch.float32, device=cuda)
    out = buf[1:1 + n] if misalign else buf[:n]
    assert out.data_ptr() % 16 == (4 if misalign else 0)
    rc1 = lib.yolo_bg_stats(L.ptr(bank_d), nb, L.ptr(rows_d), L.ptr(work), N, H, W, L.stream_ptr())
    rc2 = lib.yolo_bg_render(L.ptr(bank_d), nb, L.ptr(rows_d), L.ptr(work), L.ptr(out), N, H, W, L.stream_ptr())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:1] == -7).all() if misalign else True                      # nothing written before the view
    assert (got[1 + n:] == -7).all() if misalign else (got[n:] == -7).all()    # nor past the batch
    return out.cpu().numpy().reshape(N, 3, H, W), (rc1, rc2)


def _colour(seed):
    random.seed(seed); np.random.seed(seed)
    return render.ColorAugmenter(brightness=0.5, contrast=0.5, saturation=0.5, hue=1.0, pca_noise=0).affine()


def _chw(img):
    return np.ascontiguousarray(img.astype(np.float32).transpose(2, 0, 1))


@pytest.fixture(scope='module')
def bank():
    images = br.bank_images(seed=1)
    data, table = br.pack_bank(images, render.mip_chain)
    assert [len(t) for t in table] == [1, 3, 3, 1, 3]
    return images, data, table


@pytest.fixture(scope='module')
def reference(bank):
    """The restatement of the seven-row batch on both outputs, computed once."""
    out = {}
    for H, W in br.OUTPUTS:
        rows = br.seven_rows(bank[2], H, W, _colour(3))
        out[(H, W)] = (rows, br.render(bank[1], rows, H, W))
    return out


@pytest.mark.parametrize('hw', br.OUTPUTS, **IDS)
def test_batch_against_the_restatement(cuda, bank, reference, hw):
    rows, want = reference[hw]
    got, rcs = device_bg(cuda, bank[1], rows, *hw)
    assert rcs == (L.OK, L.OK)
    for n in range(7):
        err = float(np.abs(got[n].astype(np.float64) - want[n]).max())
        print('%dx%d row %d: max |device - restatement| = %.3g (values %.1f .. %.1f)' % (hw + (n, err, want[n].min(), want[n].max())))
        assert err <= ATOL, (n, err)
    assert np.array_equal(want[0], np.broadcast_to(np.float32([3.0, -2.0, 7.5])[:, None, None], want[0].shape))   # no image: out = e
    # rows 0..5 carry no contrast term: bit-equal by construction
    assert not rows[:6, 25:34].any() and np.abs(rows[6, 25:34].view(np.float32)).max() > 0
    assert np.array_equal(got[:6], want[:6])
    # the level >= 1 rows really sit on a coarser level, and row 5's residual step is past 2 pixels
    assert br.unpack(rows[4])['off'] == bank[2][2][1][0] and br.unpack(rows[5])['a'][0] >= 2


@pytest.mark.parametrize('hw', br.OUTPUTS, **IDS)
def test_identity_rows_are_the_image_bytes(cuda, hw):
    """Independent of the restatement: an image of the output's size drawn whole is its own bytes, mirrored its bytes reversed."""
    H, W = hw
    img = br.bank_images(seed=5, sizes=(hw,))[0]
    data, table = br.pack_bank([img], render.mip_chain)
    rows = np.stack([br.crop_row(table, 0, (0, 0, W, H), hw), br.crop_row(table, 0, (0, 0, W, H), hw, mirror=True)])
    got, rcs = device_bg(cuda, data, rows, H, W)
    assert rcs == (L.OK, L.OK)
    assert np.array_equal(got[0], _chw(img)) and np.array_equal(got[1], _chw(img[:, ::-1]))


def test_an_exact_halving_is_mip_level_one(cuda, bank):
    images, data, table = bank
    level1 = render.mip_chain(np.dstack([images[4], np.full((32, 48, 1), 255, np.uint8)]))[1]
    got, rcs = device_bg(cuda, data, br.crop_row(table, 4, (0, 0, 48, 32), (16, 24))[None], 16, 24)
    assert rcs == (L.OK, L.OK) and level1.shape == (16, 24, 4)
    assert np.array_equal(got[0], _chw(level1[..., :3]))


def test_taps_clamp_to_the_roi_and_not_to_the_frame(cuda, bank):
    """An interior 6 x 4 crop drawn to 24 x 16 (scale 1/4: every coordinate is exact in fp32) equals the same draw on that crop stored
    as a bank image of its own -- the crop's neighbours in the frame must not be read."""
    images, data, table = bank
    x0, y0, cw, ch = 10, 9, 6, 4
    own, own_table = br.pack_bank([np.ascontiguousarray(images[1][y0:y0 + ch, x0:x0 + cw])], render.mip_chain)
    for mirror in (False, True):
        inside, rc1 = device_bg(cuda, data, br.crop_row(table, 1, (x0, y0, cw, ch), (16, 24), mirror)[None], 16, 24)
        alone, rc2 = device_bg(cuda, own, br.crop_row(own_table, 0, (0, 0, cw, ch), (16, 24), mirror)[None], 16, 24)
        assert rc1 == rc2 == (L.OK, L.OK)
        assert np.array_equal(inside, alone)
        assert inside.min() >= images[1][y0:y0 + ch, x0:x0 + cw].min() and inside.max() <= images[1][y0:y0 + ch, x0:x0 + cw].max()


@pytest.mark.parametrize('hw', br.OUTPUTS, **IDS)
def test_contrast_only_keeps_the_luma_of_the_mean(cuda, bank, hw):
    """out = alpha P + (1 - alpha) luma(mean P): the luma of the output's mean is the luma of P's mean.  Against a float64 evaluation
    of the same row, to 16 float32 ulp of the largest expected magnitude: the definition has 8 rounded operations per value (three
    products and two sums for A P, the sum with k, and in k the rounding of mu and of D mu + e), half an ulp each at most -- 4 ulp,
    doubled twice for the operands' own magnitudes passing the result's.  The crop is drawn at scale 1/4 or 1/2, so P itself is
    exact in fp32 and nothing else rounds."""
    H, W = hw
    images, data, table = bank
    crop = (10, 9, W // 4, H // 4) if W % 4 == 0 else (7, 5, 2 * W, 2 * H)
    s = 1 if W % 4 == 0 else 2
    alpha = 1.4
    row = br.crop_row(table, s, crop, hw, colour=br.contrast_only(alpha), level=0)[None]
    want, P, mu = br.render(data, row, H, W, ft=np.float64, return_parts=True)
    assert np.array_equal(br.render(data, row, H, W, return_parts=True)[1], P)          # P is exact in float32
    got, rcs = device_bg(cuda, data, row, H, W)
    assert rcs == (L.OK, L.OK)
    tol = 16 * float(np.spacing(np.float32(np.abs(want).max())))
    coef = np.float64([0.299, 0.587, 0.114])
    luma_out = float(coef @ got[0].astype(np.float64).mean(axis=(1, 2)))
    luma_p = float(coef @ P[0].mean(axis=(0, 1)))
    err = float(np.abs(got[0] - want[0]).max())
    print('%dx%d contrast only: luma of the mean %.6f vs %.6f, max |device - float64| = %.3g, tolerance %.3g' % (hw + (luma_out, luma_p, err, tol)))
    assert abs(luma_out - luma_p) <= tol and err <= tol
    assert np.abs(got[0] - _chw(P[0])).max() > 1                              # (the stage did something)


def test_misaligned_out_takes_the_scalar_path_with_the_same_bits(cuda, bank, reference):
    rows, want = reference[(16, 24)]
    aligned, rc1 = device_bg(cuda, bank[1], rows, 16, 24)
    shifted, rc2 = device_bg(cuda, bank[1], rows, 16, 24, misalign=True)
    assert rc1 == rc2 == (L.OK, L.OK)
    assert np.array_equal(aligned, shifted)


def test_two_calls_are_bit_identical_and_one_image_works(cuda, bank, reference):
    for hw in br.OUTPUTS:
        rows, want = reference[hw]
        assert np.array_equal(device_bg(cuda, bank[1], rows, *hw)[0], device_bg(cuda, bank[1], rows, *hw)[0])
        one, rcs = device_bg(cuda, bank[1], rows[6:7], *hw)
        assert rcs == (L.OK, L.OK) and float(np.abs(one[0].astype(np.float64) - want[6]).max()) <= ATOL
        one, rcs = device_bg(cuda, bank[1], rows[3:4], *hw)
        assert rcs == (L.OK, L.OK) and np.array_equal(one[0], want[3])


@pytest.mark.parametrize('hw', br.OUTPUTS, **IDS)
def test_rows_that_point_past_the_bank_render_as_no_image(cuda, bank, hw):
    """The kernels check a row against bank_bytes before any load.  The tensor is LARGER than bank_bytes (the bank, then 4 KiB of
    255): a kernel that ignored the bound would read allocated bytes and fail the comparison, not fault."""
    H, W = hw
    images, data, table = bank
    off, h, w = table[4][2]                                                  # the bank's last level
    assert off + 4 * h * w == data.size
    e = [5.0, 6.0, 7.0]
    good = br.make_row(off, h, w, [0, 0, w - 1, h - 1], [0.5, 0, 0, 0, 0.5, 0], e=e)
    rows = np.stack([good] * 9)

    def put(n, off=off, h=h, w=w, roi=(0, 0, w - 1, h - 1)):
        rows[n, 1], rows[n, 2] = h, w
        rows[n, 3:7] = roi
        rows[n, 8:10] = np.array([off], np.int64).view(np.int32)
    put(1, off=off + 2, h=h - 1, roi=(0, 0, w - 1, h - 2))      # not a whole pixel (and it would still fit)
    put(2, off=off + 4)                         # offset + 4 h w == bank_bytes + 4
    put(3, roi=(3, 0, 2, h - 1))                # an empty roi
    put(4, roi=(0, 0, w, h - 1))                # a roi past the level
    put(5, roi=(0, -1, w - 1, h - 1))
    put(6, off=data.size)                       # the offset is the end of the bank
    put(7, h=2 ** 20, w=2 ** 20)                # a size past the bank (and 4 h w past 32 bits)
    put(8, off=-4)
    got, rcs = device_bg(cuda, data, rows, H, W, pad=4096)
    assert rcs == (L.OK, L.OK)
    want = br.render(data, rows, H, W)
    plain = np.broadcast_to(np.float32(e)[:, None, None], (3, H, W))
    assert np.array_equal(got[0], want[0]) and not np.array_equal(got[0], plain)
    for n in range(1, 9):
        assert np.array_equal(want[n], plain) and np.array_equal(got[n], plain), n
    # the same rows with the padding counted in: row 2 now lies inside and reads it (row 1 is still not a whole pixel)
    wide, _ = device_bg(cuda, data, rows[:3], H, W, bank_bytes=data.size + 4096, pad=4096)
    assert np.array_equal(wide[0], got[0]) and np.array_equal(wide[1], plain) and not np.array_equal(wide[2], plain)


def test_bad_arguments_return_the_documented_codes(cuda, bank, reference):
    import torch
    lib = L.load()
    rows, _ = reference[(16, 24)]
    N, H, W = 7, 16, 24
    bank_d = torch.from_numpy(bank[1]).to(cuda)
    rows_d = torch.from_numpy(rows).to(cuda)
    work = torch.zeros(lib.yolo_bg_workspace_bytes(N, H, W) + 8, dtype=torch.uint8, device=cuda)
    out = torch.full((N, 3, H, W), -7.0, device=cuda)
    st = L.stream_ptr()
    b, nb, r, w, o = L.ptr(bank_d), bank_d.numel(), L.ptr(rows_d), L.ptr(work), L.ptr(out)
    assert lib.yolo_bg_stats(b, nb, r, w, N, H, W, st) == L.OK and lib.yolo_bg_render(b, nb, r, w, o, N, H, W, st) == L.OK
    torch.cuda.synchronize()
    first = out.clone()
    out.fill_(-7.0)
    for args in ((None, nb, r, w), (b, nb, None, w), (b, nb, r, None), (b, 0, r, w), (b, -8, r, w), (b + 2, nb, r, w), (b, nb, r + 4, w), (b, nb, r, w + 4)):
        assert lib.yolo_bg_stats(*args, N, H, W, st) == L.EINVAL, args
        assert lib.yolo_bg_render(*args, o, N, H, W, st) == L.EINVAL, args
    assert lib.yolo_bg_render(b, nb, r, w, None, N, H, W, st) == L.EINVAL
    for sizes in ((0, H, W), (N, 0, W), (N, H, -4)):
        assert lib.yolo_bg_stats(b, nb, r, w, *sizes, st) == L.EINVAL and lib.yolo_bg_render(b, nb, r, w, o, *sizes, st) == L.EINVAL
        assert lib.yolo_bg_workspace_bytes(*sizes) == L.EINVAL
    assert lib.yolo_bg_stats(b, nb, r, w, N, 2 ** 31 - 1, 8, st) == L.EUNSUPPORTED
    assert lib.yolo_bg_render(b, nb, r, w, o, N, 2 ** 31 - 1, 8, st) == L.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                          # nothing was launched
    assert lib.yolo_bg_render(b, nb, r, w, o, N, H, W, st) == L.OK          # (the workspace still holds the sums)
    torch.cuda.synchronize()
    assert torch.equal(out, first)


def test_background_bank_end_to_end(cuda, tmp_path):
    """BackgroundBank over a directory of PNGs: next_batch is the restatement of draw_params' rows under the same seed; shape, dtype,
    device, out=; and RenderCar.render_device takes the result."""
    import torch
    from PIL import Image
    bg_dir = tmp_path / 'bg'
    bg_dir.mkdir()
    images = br.bank_images(seed=7, sizes=((40, 60), (75, 50), (33, 33), (8, 120)))
    for k, im in enumerate(images):
        Image.fromarray(im).save(str(bg_dir / ('bg%02d.png' % k)))
    (bg_dir / 'notes.txt').write_text('not an image')
    H, W = 24, 32
    bank = bgm.BackgroundBank(str(bg_dir), H, W, device=cuda, mode='train')
    assert len(bank) == 4 and bank.size == [(40, 60), (75, 50), (33, 33), (8, 120)]
    random.seed(21); np.random.seed(21)
    got = bank.next_batch(5)
    bank.reset()
    random.seed(21); np.random.seed(21)
    rows = bank.draw_params(5)
    bank.reset()
    mine = torch.full((5, 3, H, W), -7.0, device=cuda)
    random.seed(21); np.random.seed(21)
    again = bank.next_batch(5, out=mine)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (5, 3, H, W) and got.dtype == torch.float32 and got.device == cuda
    assert again is mine and torch.equal(got, mine)
    want = br.render(bank.data, rows, H, W)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print('next_batch: max |device - restatement| = %.3g; values %.1f .. %.1f' % (err, want.min(), want.max()))
    assert err <= ATOL
    assert (rows[:, 0] == 1).all() and np.abs(rows[:, 25:34].view(np.float32)).max() > 0           # (images, and a contrast term)
    with pytest.raises(ValueError):
        bank.next_batch(5, out=torch.empty((4, 3, H, W), device=cuda))
    # the same pixels without augmentation are the resized images: values stay in 0..255
    plain = bgm.BackgroundBank(str(bg_dir), H, W, device=cuda, mode='val', augment=False).next_batch(6)
    assert float(plain.min()) >= 0 and float(plain.max()) <= 255 and torch.equal(plain[0], plain[4])
    # and the car renderer takes the batch
    rr.write_sprite_dir(str(tmp_path / 'png'), size=(20, 28))
    rc = render.RenderCar(H, W, rr.CLASSES, str(tmp_path / 'png'), device=cuda)
    imgs, labels = rc.render_device(got, 'train', render_rate=0.8)
    torch.cuda.synchronize()
    assert tuple(imgs.shape) == (5, 3, H, W) and float(imgs.min()) >= 0 and float(imgs.max()) <= 1
    assert tuple(labels.shape) == (5, 1, 6 + len(rr.CLASSES))
