"""GPU checks of the frame intake (csrc/intake.hip through yolo_amd.intake) against tests/intake_ref.py: affine matrices bit
for bit (w is exactly 1 and every operation is IEEE and uncontracted), the identity against cv_img_2_ndarray, a homography that
leaves the frame (border 0), rectify_plates on a known answer, and FrameIntake feeding the micro net.

Every comparison prints its observed maximum before it asserts (pytest -s)."""
import gc

import numpy as np
import pytest
import torch

import intake_ref as ir
from oracle import graph as og, detect as od
from yolo_amd import intake as it
from yolo_amd import render

pytestmark = pytest.mark.gpu

f32 = np.float32
# the shared affine cases, the vector tail (Wo = 1, 13, 30: scalar stores, a partial last group; 24 and 96 take the 16-byte
# stores), and two launches of more than one block (64 x 96: 6 blocks of 16-byte stores; 40 x 30 above: 2 blocks of scalar ones)
CASES = ir.AFFINE_CASES + [((37, 53), (16, 1), (1., 1.), None),
                           ((37, 53), (16, 13), (0.8, 0.9), 0),
                           ((37, 53), (16, 30), (1., 1.), 1),
                           ((48, 64), (64, 96), (0.75, 1.), 1)]


def _three_matrices(case):
    """The case's matrix, the same crop with another flip, and the case's matrix sheared and shifted (taps leave the roi):
    three different affine maps for one launch."""
    src_hw, dst_hw, clip, flip = case
    M0, roi = it.intake_matrix(src_hw, dst_hw, clip, flip)
    M1, roi1 = it.intake_matrix(src_hw, dst_hw, clip, {None: -1, 1: 0, 0: 1, -1: None}[flip])
    assert roi1 == roi
    M2 = M0.copy()
    M2[0, 1], M2[1, 0] = 0.21, -0.13
    M2[0, 2] += 1.7
    M2[1, 2] -= 2.3
    return np.stack([M0, M1, M2]), roi


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('case', CASES, ids=ir.case_id)
def test_affine_equals_the_restatement_bit_for_bit(cuda, case, C):
    src_hw, dst_hw = case[0], case[1]
    frames = ir.random_frames(21 + C, 3, src_hw[0], src_hw[1], C)
    M, roi = _three_matrices(case)
    gain = None if C == 1 else [1.25, 0.8, 3.0, 0.1][:C]
    for border, bname in ((1, 'replicate'), (0, 'constant')):
        want = ir.warp_u8(frames, M, dst_hw, border=border, roi=roi, gain=gain)
        got = it.warp_u8(frames, M, dst_hw, border=bname, roi=roi, gain=gain).cpu().numpy()
        diff = float(np.abs(got - want).max())
        print('%s C=%d border=%d: max |device - restatement| = %.3g' % (ir.case_id(case), C, border, diff))
        assert np.array_equal(got, want), (bname, diff)


def test_out_buffer_alignment_picks_the_store_path(cuda):
    """Wo % 4 == 0 into a buffer that starts 4 bytes past a 16-byte boundary: scalar stores, same values; nothing is written
    before or behind the output."""
    case = CASES[-1]
    src_hw, dst_hw = case[0], case[1]
    frames = ir.random_frames(31, 3, src_hw[0], src_hw[1], 3)
    M, roi = _three_matrices(case)
    want = ir.warp_u8(frames, M, dst_hw, border=1, roi=roi)
    n = want.size
    buf = torch.full((n + 9,), -7.0, dtype=torch.float32, device=cuda)
    for off in (4, 1):                                                    # aligned (16-byte stores), then misaligned
        buf.fill_(-7.0)
        out = buf[off:off + n].view(want.shape)
        assert (out.data_ptr() % 16 == 0) == (off == 4)
        got = it.warp_u8(torch.from_numpy(frames).to(cuda), M, dst_hw, border='replicate', roi=roi, out=out)
        assert got.data_ptr() == out.data_ptr()
        h = buf.cpu().numpy()
        assert np.array_equal(h[off:off + n].reshape(want.shape), want), off
        assert (h[:off] == -7.0).all() and (h[off + n:] == -7.0).all(), off


def test_identity_equals_cv_img_2_ndarray_bit_for_bit(cuda):
    from yolo_amd.detect import cv_img_2_ndarray
    img = ir.random_frames(41, 1, 45, 52, 3)[0]
    M, roi = it.intake_matrix((45, 52), (45, 52))
    assert np.array_equal(M, np.eye(3)) and roi == (0, 0, 51, 44)
    got = it.warp_u8(img, M, (45, 52), border='replicate', roi=roi)
    want = cv_img_2_ndarray(img, device=cuda)
    assert torch.equal(got, want)
    assert torch.equal(it.FrameIntake((45, 52), device=cuda)(img), want)


def test_projective_border_constant(cuda):
    """A homography that maps part of a 24 x 40 output outside a 31 x 45 frame: exactly 0 where all four taps are outside,
    within 1e-5 of the restatement elsewhere (one fp32 ulp of a coordinate of magnitude <= 64, 4e-6 px, times a slope of at
    most one full level per pixel)."""
    Ho, Wo, Hs, Ws = 24, 40, 31, 45
    frames = np.maximum(ir.random_frames(51, 2, Hs, Ws, 3), 1)             # no zero level: a 0 in the output is the border
    out_quad = np.float64([[Wo - 1, Ho - 1], [0, Ho - 1], [0, 0], [Wo - 1, 0]])
    src_quad = np.float64([[50.5, 28.0], [3.0, 35.5], [-6.0, -4.0], [40.0, 3.0]])
    M = np.stack([render.homography(out_quad, src_quad), render.homography(out_quad, src_quad[::-1] * 0.9 + 2.0)])
    assert abs(M[0][2, 0]) > 1e-4 and abs(M[0][2, 1]) > 1e-4               # a real perspective: w varies over the output
    want = ir.warp_u8(frames, M, (Ho, Wo), border=0)
    got = it.warp_u8(frames, M, (Ho, Wo), border='constant').cpu().numpy()
    j, i = np.meshgrid(np.arange(Wo, dtype=np.float64), np.arange(Ho, dtype=np.float64))
    for n in range(2):
        p = np.einsum('rc,chw->rhw', M[n], np.stack([j, i, np.ones_like(j)]))
        sx, sy = p[0] / p[2], p[1] / p[2]
        eps = 1e-3                                                         # (away from the boundary: float32 coordinates)
        outside = (sx < -1 - eps) | (sx > Ws + eps) | (sy < -1 - eps) | (sy > Hs + eps)
        inside = (sx > eps) & (sx < Ws - 1 - eps) & (sy > eps) & (sy < Hs - 1 - eps)
        assert outside.sum() > 40 and inside.sum() > 200, (outside.sum(), inside.sum())
        assert (got[n][:, outside] == 0).all()
        assert (got[n][:, inside] > 0).all()
    err = float(np.abs(got - want).max())
    print('projective: max |device - restatement| = %.3g' % err)
    assert err <= 1e-5, err


CAMERA = {'image_width': 640, 'image_height': 480,
          'projection_matrix': {'data': [2000., 0., 320., 0., 0., 2000., 240., 0., 0., 0., 1., 0.]}}


def test_rectify_plates(cuda):
    """Against the restatement with the matrix rebuilt here from PlateCamera.corners (1e-5), and a known answer: fx = fy = 2000,
    pose [21, -10.5, 2100, 0, 0, 0] projects the plate to the axis-aligned 380 x 160 rectangle columns 150..530, rows 150..310
    (2e-4: the float32 cast of the corners moves a coordinate by about 3e-5 px, times up to a level per pixel)."""
    cam = render.PlateCamera(CAMERA)
    poses = np.float64([[21.0, -10.5, 2100.0, 0.0, 0.0, 0.0], [100.0, -50.0, 3000.0, 0.2, -0.3, 0.1]])
    frames = ir.random_frames(61, 2, 480, 640, 3)
    got = it.rectify_plates(frames, poses, CAMERA).cpu().numpy()
    assert got.shape == (2, 3, 160, 380) and got.dtype == f32
    LP_corner = np.float32([[380, 160], [0, 160], [0, 0], [380, 0]])
    M = np.stack([render.homography(LP_corner, cam.corners(p)) for p in poses])       # (frame size = camera size: scale 1)
    want = ir.warp_u8(frames, M, (160, 380), border=0)
    err = float(np.abs(got - want).max())
    crop = frames[0, 150:310, 150:530].transpose(2, 0, 1).astype(np.float64) / 255.0
    known = float(np.abs(got[0] - crop).max())
    print('rectify_plates: max |device - restatement| = %.3g, max |device - exact crop| = %.3g' % (err, known))
    assert err <= 1e-5, err
    assert known <= 2e-4, known
    assert got.min() >= 0.0 and got.max() <= 1.0
    # one frame, one pose, a PlateCamera object, a frame of another size than the camera's (add_edges :382-386)
    small = ir.random_frames(62, 1, 240, 320, 3)[0]
    one = it.rectify_plates(small, poses[1], cam).cpu().numpy()
    c2 = cam.corners(poses[1]) * np.float32([320 / 640., 240 / 480.])
    want1 = ir.warp_u8(small, render.homography(LP_corner, c2), (160, 380), border=0)
    assert float(np.abs(one - want1).max()) <= 1e-5


@pytest.fixture(scope='module')
def micro(cuda):
    from yolo_amd.net import CarNet
    from yolo_amd.detect import Detector
    spec, size = og.spec_micro(), (64, 96)
    P = og.init_params(og.build_graph(spec), seed=0, bn='random')
    steps = od.init_steps(spec['layers'], spec['all_anchors'])
    net = CarNet(spec, dtype='f32', device=cuda).load_params(P)
    frames = ir.random_frames(71, 2, 90, 130, 3)
    return {'net': net, 'det': Detector(spec, size, steps, device=cuda), 'size': size, 'frames': frames,
            'kw': dict(clip=(0.9, 0.8), flip=1)}


def test_frame_intake_feeds_the_net(cuda, micro):
    """FrameIntake -> CarNet -> Detector.predict gives the rows of the same net fed the restatement's array."""
    intake = it.FrameIntake(micro['size'], device=cuda, **micro['kw'])
    M, roi = intake.matrix((90, 130))
    ref = ir.warp_u8(micro['frames'], M, micro['size'], border=1, roi=roi)
    x = intake(micro['frames'])
    assert tuple(x.shape) == (2, 3) + micro['size'] and x.dtype == torch.float32 and x.device == cuda
    assert np.array_equal(x.cpu().numpy(), ref)
    rows = micro['det'].predict(micro['net'](x))
    rows_ref = micro['det'].predict(micro['net'](torch.from_numpy(ref).to(cuda)))
    assert rows.shape[0] == 2 and np.isfinite(rows).all()
    assert np.array_equal(rows, rows_ref)


def test_frame_intake_buffers_sources_and_white_balance(cuda, micro):
    frames = micro['frames']
    intake = it.FrameIntake(micro['size'], device=cuda, **micro['kw'])
    M, roi = intake.matrix((90, 130))
    ref = ir.warp_u8(frames, M, micro['size'], border=1, roi=roi)
    # a host ndarray, a pinned tensor and a device tensor give identical outputs, from the object's one buffer
    a = intake(frames)
    ptr, got_a = a.data_ptr(), a.cpu().numpy()
    b = intake(torch.from_numpy(frames).pin_memory())
    got_b = b.cpu().numpy()
    c = intake(torch.from_numpy(frames).to(cuda))
    got_c = c.cpu().numpy()
    assert b.data_ptr() == ptr and c.data_ptr() == ptr
    assert np.array_equal(got_a, ref) and np.array_equal(got_b, ref) and np.array_equal(got_c, ref)
    # a second host call reuses the staging buffers: nothing is allocated once the batch size has been seen
    other = frames[::-1].copy()
    # (cyclic garbage of earlier tests -- the nets of the test above -- holds device memory until the collector runs; collected here,
    #  so that a collection landing inside the call cannot free it there and pass for, or hide, an allocation of the call's own)
    gc.collect()
    before = torch.cuda.memory_allocated(cuda)
    d = intake(other)
    assert torch.cuda.memory_allocated(cuda) == before and d.data_ptr() == ptr
    assert np.array_equal(d.cpu().numpy(), ref[::-1])
    # out= writes the caller's storage
    out = torch.full((2, 3) + micro['size'], -1.0, dtype=torch.float32, device=cuda)
    r = intake(frames, out=out)
    assert r.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), ref)
    with pytest.raises(ValueError):
        intake(frames, out=out[:1])
    # one (H,W,3) frame
    assert np.array_equal(intake(frames[1]).cpu().numpy(), ref[1:2])
    # white_balance = nd_white_balance's bgr triple: the planes scaled exactly (powers of two)
    wb = it.FrameIntake(micro['size'], device=cuda, white_balance=(0.5, 1, 2), **micro['kw'])(frames).cpu().numpy()
    assert np.array_equal(wb, ref * np.float32([0.5, 1, 2]).reshape(1, 3, 1, 1))
    assert np.array_equal(wb, ir.warp_u8(frames, M, micro['size'], border=1, roi=roi, gain=(0.5, 1, 2)))


def test_frame_intake_runs_on_the_current_stream(cuda, micro):
    """Captured into a graph on a side stream: a kernel launched on any other stream would not be part of the graph, and the
    replay would leave the zeroed output as it is."""
    frames = torch.from_numpy(micro['frames']).to(cuda)
    intake = it.FrameIntake(micro['size'], device=cuda, **micro['kw'])
    out = torch.empty((2, 3) + micro['size'], dtype=torch.float32, device=cuda)
    want = intake(frames, out=out).clone()                                 # (also caches the matrix: the capture allocates nothing)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        intake(frames, out=out)
    out.zero_()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                                   # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # and eagerly under torch.cuda.stream(s), ordered by that stream alone
    out.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        intake(frames, out=out)
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()
    assert torch.equal(out, want)


def test_frame_intake_refuses_another_current_device(cuda, micro):
    """Like the other objects: a FrameIntake of cuda:1 does not launch while cuda:0 is the current device (its constructor
    allocates nothing, so this runs on a one-GPU box too)."""
    from yolo_amd import lib as L
    assert torch.cuda.current_device() == 0
    intake = it.FrameIntake(micro['size'], device='cuda:1')
    with pytest.raises(L.YoloError):
        intake(micro['frames'])
