"""The frame overlay on the device against tests/overlay_ref.py: yolo_overlay_draw bit for bit from hand-made integer tables,
yolo_overlay_shapes (integer vertices and flags equal, float vertices within 1e-3 px, matrices within one float32 step), FrameOverlay
end to end, and the error codes."""
import math

import numpy as np
import pytest
import torch

import intake_ref
import overlay_ref as R
from yolo_amd import lib as L
from yolo_amd.overlay import FrameOverlay

pytestmark = pytest.mark.gpu


def _draw(lib, dev, frames, table, offset=0):
    """frames (N,H,W,C) uint8 ndarray, table (N,K,12) int32 ndarray -> the painted frames; the device frames start `offset` bytes
    into a larger buffer, whose other bytes must come back untouched."""
    N, H, W, Cc = frames.shape
    guard = 64
    buf = torch.full((offset + frames.size + guard,), 0xA5, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + frames.size].view(N, H, W, Cc)
    view.copy_(torch.from_numpy(frames).to(dev))
    tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    rc = lib.yolo_overlay_draw(L.ptr(view), L.ptr(tab), N, H, W, Cc, table.shape[1], L.stream_ptr())
    assert rc == L.OK
    host = buf.cpu().numpy()
    assert (host[:offset] == 0xA5).all() and (host[offset + frames.size:] == 0xA5).all()
    return host[offset:offset + frames.size].reshape(frames.shape)


def _frames(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# slots: (vertices, colour, t, enabled)
FIVE = [([(4, 6), (45, 3), (49, 30), (8, 33)], (10, 20, 30, 40), 2, 1),
        ([(20, -7), (70, 12), (30, 45), (-6, 20)], (200, 1, 2, 3), 5, 1),               # vertices at negative coordinates and beyond W / H
        ([(0, 0), (52, 0), (52, 36), (0, 36)], (9, 9, 9, 9), 1, 0),                      # a disabled slot between enabled ones
        ([(25, 18), (25, 18), (25, 18), (25, 18)], (1, 2, 3, 4), 5, 1),                  # all four vertices equal: a disc
        ([(10, 10), (40, 10), (40, 25), (10, 25)], (0, 255, 0, 77), 1, 1)]
OUTSIDE_SHAPE = ([(-40, -30), (-10, -30), (-10, -5), (-40, -5)], (255, 255, 255, 255), 5, 1)
# 40 rows are two 32-row tiles of four 8-row wave strips: the lines cross y = 8 .. 32 both ways (two tiles across: test_draw_crosses_tile_borders_both_ways)
WIDE = [([(3, 2), (147, 37), (140, 5), (10, 30)], (7, 8, 9, 10), 2, 1), ([(60, -5), (70, 45), (130, 20), (-20, 15)], (90, 80, 70, 60), 5, 1),
        ([(0, 39), (149, 39), (149, 0), (0, 0)], (255, 0, 255, 1), 1, 1)]


@pytest.mark.parametrize('t', [1, 2, 5])
@pytest.mark.parametrize('Cc', [1, 3, 4])
def test_draw_equals_the_restatement(lib, cuda, t, Cc):
    frames = _frames(1, (2, 37, 53, Cc))
    one = R.make_table([([(5, 4), (47, 9), (44, 31), (9, 28)], (11, 22, 33, 44), t, 1)])
    five = R.make_table([(v, c, t, en) for (v, c, _, en) in FIVE])
    for table, offset in ((np.stack([one, one]), 0), (np.stack([five, five[::-1]]), 1)):
        got = _draw(lib, cuda, frames, table, offset)
        assert np.array_equal(got, R.draw(frames, table))
        assert not np.array_equal(got, frames)
    wide = _frames(2, (1, 40, 150, Cc))
    table = R.make_table([(v, c, t, en) for (v, c, _, en) in WIDE])[None]
    assert np.array_equal(_draw(lib, cuda, wide, table, 3), R.draw(wide, table))


def test_draw_crosses_tile_borders_both_ways(lib, cuda):
    """300 x 40 px: two 256-pixel tiles across and two 32-row tiles down, long diagonals through the corner where they meet."""
    frames = _frames(3, (1, 40, 300, 3))
    slots = [([(2, 38), (298, 1), (298, 38), (2, 1)], (1, 2, 3), 2, 1), ([(250, -4), (262, 44), (255, 32), (257, 31)], (4, 5, 6), 5, 1),
             ([(0, 32), (299, 31), (299, 8), (0, 7)], (7, 8, 9), 1, 1)]
    table = R.make_table(slots)[None]
    assert np.array_equal(_draw(lib, cuda, frames, table, 1), R.draw(frames, table))


def test_painters_order_and_shapes_outside(lib, cuda):
    frames = _frames(4, (1, 37, 53, 3))
    a, b = FIVE[0], (FIVE[0][0], (250, 251, 252), 2, 1)
    both = _draw(lib, cuda, frames, R.make_table([a, b])[None])
    assert np.array_equal(both, R.draw(frames, R.make_table([b])[None]))              # the later slot wins every shared pixel
    swapped = _draw(lib, cuda, frames, R.make_table([b, a])[None])
    assert np.array_equal(swapped, R.draw(frames, R.make_table([a])[None]))
    # a shape entirely outside the frame paints nothing; beyond the limits a slot counts as disabled
    far = ([(5, 5), (2 ** 20 + 1, 8), (48, 30), (7, 33)], (1, 1, 1), 2, 1)
    thick = ([(5, 5), (50, 8), (48, 30), (7, 33)], (1, 1, 1), 256, 1)
    assert np.array_equal(_draw(lib, cuda, frames, R.make_table([OUTSIDE_SHAPE, far, thick])[None], 1), frames)
    # vertices at the limit itself: no intermediate overflows, the part inside the frame is painted
    edge = R.make_table([([(-2 ** 20, -2 ** 20), (2 ** 20, 2 ** 20), (2 ** 20, -2 ** 20 + 7), (-2 ** 20, 2 ** 20 - 9)], (3, 2, 1), 5, 1)])[None]
    got = _draw(lib, cuda, frames, edge)
    assert np.array_equal(got, R.draw(frames, edge)) and not np.array_equal(got, frames)


def test_no_enabled_slot_leaves_the_frame_alone(lib, cuda):
    frames = _frames(5, (2, 37, 53, 3))
    table = R.make_table([(v, c, t, 0) for (v, c, t, _) in FIVE])
    assert np.array_equal(_draw(lib, cuda, frames, np.stack([table, table]), 1), frames)


# ---- shapes ----------------------------------------------------------------------------------------------------------------
H0, W0 = 48, 64


def _cases():
    """The inputs of the shapes test, with the special rows put in, and the restatement of both use_r settings (made once)."""
    B, nbox, Cc, post = 8, 12, 9, 6
    rows, kept, count = R.nms_case(5, B, nbox, Cc, post)
    kept[0, 0], count[1] = nbox * 3 + 1, post                               # an id out of range; a full row
    kept[1] = [0, 4, 35, -1, 7, 8]                                          # a pad inside the count
    rows[2, int(kept[2, 0]) // 3, 2] = np.nan                               # a NaN box
    pred = R.top1_rows(3, B, Cc)
    pred[0, 0], pred[1, 0] = 0.5, np.nextafter(np.float32(0.5), np.float32(1))      # exactly the threshold: not enabled
    pred[2, 3] = np.nan
    pred[3, 4] = np.inf
    lp = R.plate_rows(7, B)
    lp[0, 0], lp[1, 0] = 0.5, np.nextafter(np.float32(0.5), np.float32(1))
    lp[2, 1] = np.nan
    lp[3, 1:] = [0, 0, 0, 0, 0, 0]                                          # on the image plane: w = 0
    lp[4, 1:] = [0, 0, 3000, 0, math.pi / 2, 0]                             # edge on: the float32 corners on one line
    lp[5, 1:] = [0, 0, 1e30, 0, 0, 0]                                       # far away: the float32 corners coincide
    want = {}
    for use_r in (False, True):
        want[use_r] = R.shapes(B, H0, W0, nms=(rows, kept, count), cand_per_box=3, pred=pred, use_r=use_r, lp=lp, camera=R.CAMERA)
        # the restatement alone: no finite vertex within 1e-6 px of an integer (the fp64 route's error is ~1e-11 px here)
        assert R.far_from_integers(want[use_r]['v64'])
    return dict(B=B, nbox=nbox, C=Cc, post=post, rows=rows, kept=kept, count=count, pred=pred, lp=lp, want=want)


@pytest.fixture(scope='module')
def cases():
    return _cases()


def _ulp_apart(a, b):
    """float32 arrays: the largest distance in representable steps (finite values of one sign or zero)."""
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max())


@pytest.mark.parametrize('use_r', [False, True])
def test_shapes_equal_the_restatement(cuda, cases, use_r):
    c = cases
    ov = FrameOverlay(camera=R.CAMERA, use_r=use_r, device=cuda)
    frames = torch.zeros((c['B'], H0, W0, 3), dtype=torch.uint8, device=cuda)
    t = lambda a: torch.from_numpy(a).to(cuda)
    _, clipped, valid = ov(frames, pred=t(c['pred']), lp=t(c['lp']), nms=(t(c['rows']), t(c['kept']), t(c['count'])))
    want = c['want'][use_r]
    table, verts, mats = ov.table.cpu().numpy(), ov.vertices.cpu().numpy(), ov.matrices.cpu().numpy()
    assert table.shape == want['table'].shape == (c['B'], c['post'] + 2, R.SLOT_WORDS)
    assert np.array_equal(table[:, :, 10], want['table'][:, :, 10])                  # enabled
    assert np.array_equal(table[:, :, :8], want['table'][:, :, :8])                  # integer vertices
    on = want['table'][:, :, 10] == 1
    assert np.array_equal(table[:, :, 8:10][on], want['table'][:, :, 8:10][on])      # colour, thickness
    # the flags the cases were made for
    post = c['post']
    assert table[0, 0, 10] == 0 and table[1, :post, 10].tolist() == [1, 1, 1, 0, 1, 1] and table[2, 0, 10] == 0
    assert table[:4, post, 10].tolist() == [0, 1, 0, 0] and table[4:, post, 10].all()
    assert table[:3, post + 1, 10].tolist() == [0, 1, 0]
    fin = np.isfinite(want['vertices'])
    assert np.array_equal(np.isfinite(verts), fin)
    assert np.abs(verts[fin] - want['vertices'][fin]).max() <= 1e-3
    assert np.array_equal(valid.cpu().numpy(), want['lp_valid']) and want['lp_valid'].tolist() == [0, 1, 0, 0, 0, 0, 1, 1]
    assert np.all(np.isfinite(mats))
    bad = want['lp_valid'] == 0
    assert np.array_equal(mats[bad], np.broadcast_to(R.OUTSIDE, (int(bad.sum()), 9)))
    assert _ulp_apart(mats[~bad], want['matrices'][~bad]) <= 1
    assert not clipped[torch.from_numpy(bad).to(cuda)].any()                         # an all-zero clipped plate


# ---- FrameOverlay ----------------------------------------------------------------------------------------------------------
def test_frame_overlay_end_to_end(cuda):
    N, H, W = 2, 48, 64
    frames_h = _frames(8, (N, H, W, 3))
    frames_h[..., 2] &= 0x7f                                                # no pixel holds the plate's colour (0, 0, 255) before
    pred, lp = R.top1_rows(11, N), R.plate_rows(12, N)
    lp[:, 1:4] = [[30, -20, 900], [-60, 25, 1200]]                          # near enough to cover a good part of a 64 x 48 frame
    rows, kept, count = R.nms_case(13, N, 10, 8, 4)
    ov = FrameOverlay(camera=R.CAMERA, device=cuda)
    t = lambda a: torch.from_numpy(a).to(cuda)
    args = dict(pred=t(pred), lp=t(lp), nms=(t(rows), t(kept), t(count)))
    frames = t(frames_h)
    out = torch.empty_like(frames)
    got, clipped, valid = ov(frames, out=out, **args)
    assert got is out and np.array_equal(frames.cpu().numpy(), frames_h)             # out= leaves frames untouched
    table, mats = ov.table.cpu().numpy(), ov.matrices.cpu().numpy()
    assert table[:, :, 10].sum() >= 2 * 2 + 2 and valid.cpu().tolist() == [1, 1]
    want = R.draw(frames_h, table)
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, frames_h)
    assert (want == np.uint8([0, 0, 255])).all(axis=-1).any()                        # the plate's edges are in the picture
    # the clipped plate: the intake's restatement with the device-made matrices, from the frames BEFORE drawing
    clip_want = intake_ref.warp_u8(frames_h, mats.reshape(N, 3, 3), (160, 380), border=0)
    clip_got = clipped.cpu().numpy()
    assert clip_got.shape == (N, 3, 160, 380) and np.array_equal(clip_got, clip_want) and clip_got.any()
    assert not np.array_equal(clip_got, intake_ref.warp_u8(want, mats.reshape(N, 3, 3), (160, 380), border=0))
    edge = (clip_got[:, 0] == 0) & (clip_got[:, 1] == 0) & (clip_got[:, 2] == 1)
    assert not edge.any()                                                            # an edge colour never appears in clipped
    # in place: the same picture, the same plate; the second call with this batch size allocates nothing
    keep = clipped.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(cuda)['allocation.all.allocated']
    got2, clipped2, valid2 = ov(frames, **args)
    assert torch.cuda.memory_stats(cuda)['allocation.all.allocated'] == before
    assert got2 is frames and clipped2 is clipped and valid2 is valid
    assert np.array_equal(frames.cpu().numpy(), want) and torch.equal(clipped2, keep)
    # a source alone; no source; lp without a camera
    solo = t(frames_h)
    f3, c3, v3 = ov(solo, pred=args['pred'])
    assert c3 is None and v3 is None and ov.table.shape == (N, 1, R.SLOT_WORDS)
    assert np.array_equal(f3.cpu().numpy(), R.draw(frames_h, ov.table.cpu().numpy()))
    with pytest.raises(ValueError):
        ov(solo)
    with pytest.raises(ValueError):
        FrameOverlay(device=cuda)(solo, lp=args['lp'])


def test_predict_LP_rows_is_predict_LP_batch_on_the_device(cuda):
    from yolo_amd.detect import predict_LP_batch, predict_LP_rows
    o = torch.from_numpy(np.random.default_rng(0).standard_normal((3, 4, 5, 10)).astype(np.float32)).to(cuda)
    rows = predict_LP_rows([o], [1, 3, 4, 7, 10], [45, 60, 45])
    assert rows.is_cuda and rows.shape == (3, 7) and rows.dtype == torch.float32
    assert np.array_equal(rows.cpu().numpy(), predict_LP_batch([o], [1, 3, 4, 7, 10], [45, 60, 45]))


def test_frame_intake_keeps_the_frames_it_read(cuda):
    from yolo_amd.intake import FrameIntake
    intake = FrameIntake((16, 24), device=cuda)
    assert intake.frames is None
    host = _frames(9, (2, 37, 53, 3))
    intake(host)
    assert intake.frames.is_cuda and intake.frames.dtype == torch.uint8 and np.array_equal(intake.frames.cpu().numpy(), host)
    dev = torch.from_numpy(host).to(cuda)
    intake(dev)
    assert intake.frames is dev
    one = dev[0].clone()
    intake(one)                                                             # (H,W,C): the batch view of the caller's tensor
    assert intake.frames.shape == (1, 37, 53, 3) and intake.frames.data_ptr() == one.data_ptr()
    held = torch.cuda.memory_allocated(cuda)
    del dev, one                                                            # held weakly: the intake does not keep a caller's tensor alive
    assert intake.frames is None and torch.cuda.memory_allocated(cuda) <= held - host.size - host.size // 2


# ---- error codes -----------------------------------------------------------------------------------------------------------
def test_error_codes_leave_the_frame_untouched(lib, cuda):
    frames_h = _frames(6, (2, 37, 53, 3))
    frames = torch.from_numpy(frames_h).to(cuda)
    table = torch.from_numpy(np.stack([R.make_table(FIVE)] * 2)).to(cuda)
    big = torch.zeros((2, 129, R.SLOT_WORDS), dtype=torch.int32, device=cuda)
    s = L.stream_ptr()
    f, tb = L.ptr(frames), L.ptr(table)
    assert lib.yolo_overlay_draw(None, tb, 2, 37, 53, 3, 5, s) == L.EINVAL
    assert lib.yolo_overlay_draw(f, None, 2, 37, 53, 3, 5, s) == L.EINVAL
    for bad in ((0, 37, 53, 3, 5), (2, 0, 53, 3, 5), (2, 37, -1, 3, 5), (2, 37, 53, 0, 5), (2, 37, 53, 3, 0)):
        assert lib.yolo_overlay_draw(f, tb, *bad, s) == L.EINVAL, bad
    assert lib.yolo_overlay_draw(f, L.ptr(big), 2, 37, 53, 3, 129, s) == L.EUNSUPPORTED
    assert lib.yolo_overlay_draw(f, tb, 2, 37, 53, 5, 5, s) == L.EUNSUPPORTED
    assert lib.yolo_overlay_draw(f, tb, 2, 16385, 53, 3, 5, s) == L.EUNSUPPORTED
    assert lib.yolo_overlay_draw(f, tb, 2, 37, 16385, 3, 5, s) == L.EUNSUPPORTED
    # shapes: a NULL table, a non-positive size, K beyond the limit
    pred = torch.from_numpy(R.top1_rows(1, 2)).to(cuda)
    out = torch.full((2, 1, R.SLOT_WORDS), 7, dtype=torch.int32, device=cuda)

    def shapes(table_ptr, B, H, W, K, thickness=2):
        return lib.yolo_overlay_shapes(None, None, None, 0, 0, 0, 1, None, 0, L.ptr(pred), 8, 0.5, 0, 255, None, 0.0, 0.0, 0.0, 0.0, 0, 0,
                                       0.5, 255, 160, 380, B, H, W, thickness, table_ptr, K, None, None, None, s)
    assert shapes(None, 2, 37, 53, 1) == L.EINVAL
    for bad in ((0, 37, 53, 1), (2, 0, 53, 1), (2, 37, 0, 1), (2, 37, 53, 0), (2, 37, 53, 2)):
        assert shapes(L.ptr(out), *bad) == L.EINVAL, bad
    assert shapes(L.ptr(out), 2, 37, 53, 1, thickness=0) == L.EINVAL
    assert shapes(L.ptr(out), 2, 16385, 53, 1) == L.EUNSUPPORTED
    assert shapes(L.ptr(out), 2, 37, 53, 1, thickness=256) == L.EUNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), frames_h) and (out == 7).all()
    assert shapes(L.ptr(out), 2, 37, 53, 1) == L.OK
    assert (out.cpu().numpy()[:, 0, 9] == 2).all()
