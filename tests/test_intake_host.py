"""CPU checks of the frame intake: the numpy restatement (tests/intake_ref.py) with intake_matrix against an independent
float64 bilinear (torch interpolate on the cropped, flipped frame), the crop / flip / homography arithmetic, the plate geometry
on a known answer, and the C ABI entry (declared, bound, revision still 5, bad arguments refused without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import intake_ref as ir
from yolo_amd import lib as L
from yolo_amd import intake as it
from yolo_amd import render

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
f32 = np.float32


@pytest.mark.parametrize('case', ir.AFFINE_CASES, ids=ir.case_id)
def test_restatement_equals_an_independent_bilinear(case):
    """2e-5 absolute: the restatement rounds its coordinates to fp32 (an ulp of a coordinate of magnitude <= 64 is 4e-6 px, times
    a slope of at most one full level per pixel); the independent resize is float64."""
    src_hw, dst_hw, clip, flip = case
    C_ = 3
    frames = ir.random_frames(11, 2, src_hw[0], src_hw[1], C_)
    M, roi = it.intake_matrix(src_hw, dst_hw, clip, flip)
    got = ir.warp_u8(frames, M, dst_hw, border=1, roi=roi)
    assert got.shape == (2, C_) + tuple(dst_hw) and got.dtype == f32
    for n in range(2):
        crop = np.ascontiguousarray(ir.crop_flip(frames[n], clip, flip))
        assert crop.shape[:2] == (roi[3] - roi[1] + 1, roi[2] - roi[0] + 1)
        x = torch.from_numpy(crop.astype(np.float64)).permute(2, 0, 1)[None]
        want = torch.nn.functional.interpolate(x, size=tuple(dst_hw), mode='bilinear', align_corners=False)[0].numpy() / 255.0
        err = float(np.abs(got[n].astype(np.float64) - want).max())
        print('%s image %d: max |restatement - float64 bilinear| = %.3g' % (ir.case_id(case), n, err))
        assert err < 2e-5, err


def test_the_cropped_upscale_needs_the_roi_clamp():
    """The seventh case with taps clamped to the FRAME instead of the crop reads pixels cv2.resize was never given."""
    src_hw, dst_hw, clip, flip = ir.AFFINE_CASES[6]
    frames = ir.random_frames(12, 1, src_hw[0], src_hw[1], 3)
    M, roi = it.intake_matrix(src_hw, dst_hw, clip, flip)
    assert roi == (3, 3, 13, 15)
    right = ir.warp_u8(frames, M, dst_hw, border=1, roi=roi)
    wrong = ir.warp_u8(frames, M, dst_hw, border=1, roi=None)
    assert float(np.abs(right - wrong).max()) > 1e-2


def test_crop_bounds_are_the_reference_int_arithmetic():
    # (H, W), clip -> top = int((1 - clip[0]) * H / 2.), left = int((1 - clip[1]) * W / 2.), worked by hand
    for (H, W), clip, top, left in (((37, 53), (0.8, 0.9), 3, 2),          # 3.7 -> 3, 2.65 -> 2
                                    ((9, 7), (0.8, 0.8), 0, 0),            # 0.9 -> 0, 0.7 -> 0
                                    ((48, 64), (0.75, 1.), 6, 0),
                                    ((19, 17), (0.6, 0.6), 3, 3),          # 3.8 -> 3, 3.4 -> 3
                                    ((1080, 1920), (0.5, 0.7), 270, 288),
                                    ((481, 641), (0.999, 0.5), 0, 160)):   # 0.24 -> 0, 160.25 -> 160
        M, roi = it.intake_matrix((H, W), (20, 30), clip)
        assert roi == (left, top, W - left - 1, H - top - 1), (H, W, clip, roi)
        crop = ir.crop_flip(np.zeros((H, W, 1), np.uint8), clip, None)
        assert crop.shape[:2] == (H - 2 * top, W - 2 * left)
        Hc, Wc = crop.shape[:2]
        # cv2.resize's half-pixel geometry on the crop, in frame coordinates
        assert M[0, 0] == Wc / 30. and abs(M[0, 2] - (left + 0.5 * Wc / 30. - 0.5)) < 1e-12 and M[0, 1] == 0
        assert M[1, 1] == Hc / 20. and abs(M[1, 2] - (top + 0.5 * Hc / 20. - 0.5)) < 1e-12 and M[1, 0] == 0
        assert M[2].tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        it.intake_matrix((10, 10), (4, 4), clip=(-1.5, 1.))                 # top = 12: nothing left


@pytest.mark.parametrize('flip', [1, 0, -1, None, 2])
def test_flip_codes_at_the_crop_size_copy_pixels(flip):
    """Output size = crop size: every coordinate is an integer, so the restatement returns the cropped, flipped frame / 255
    exactly -- cv2.flip's codes 1 (left-right), 0 (top-down), -1 (both); anything else: no flip, as the reference."""
    H, W, clip = 11, 13, (0.7, 0.8)                                        # top = int(1.65) = 1, left = int(1.3) = 1
    frames = ir.random_frames(13, 1, H, W, 3)
    want = ir.crop_flip(frames[0], clip, flip)
    assert want.shape == (9, 11, 3)
    M, roi = it.intake_matrix((H, W), want.shape[:2], clip, flip)
    got = ir.warp_u8(frames, M, want.shape[:2], border=1, roi=roi)[0]
    assert np.array_equal(got, want.transpose(2, 0, 1).astype(f32) / f32(255))


def test_homography_composed_with_its_inverse_is_the_identity():
    rng = np.random.default_rng(3)
    sq = np.float64([[380, 160], [0, 160], [0, 0], [380, 0]])
    for _ in range(8):
        quad = sq * rng.uniform(0.5, 2.0) + rng.uniform(-40, 40, (4, 2)) + rng.uniform(0, 300, (1, 2))
        fwd, inv = render.homography(sq, quad), render.homography(quad, sq)
        P = fwd @ inv
        assert np.abs(P / P[2, 2] - np.eye(3)).max() < 1e-9
        p = fwd @ np.append(sq[0], 1.0)
        assert np.abs(p[:2] / p[2] - quad[0]).max() < 1e-9


CAMERA = {'image_width': 640, 'image_height': 480,
          'projection_matrix': {'data': [2000., 0., 320., 0., 0., 2000., 240., 0., 0., 0., 1., 0.]}}


def test_plate_matrix_known_answer():
    """fx = fy = 2000 and Z = 2100 project the 399 x 168 mm plate to 380 x 160 px; X = 21, Y = -10.5 put its centre at
    (340, 230): the plate is the axis-aligned rectangle columns 150..530, rows 150..310 of the frame, so the restatement
    returns that crop / 255 (2e-4: the float32 corners are off by about 3e-5 px, times a slope of up to a level per pixel)."""
    cam = render.PlateCamera(CAMERA)
    pose = [21.0, -10.5, 2100.0, 0.0, 0.0, 0.0]
    assert np.abs(cam.corners(pose) - np.float32([[530, 310], [150, 310], [150, 150], [530, 150]])).max() < 1e-3
    M = it.plate_matrix(pose, cam, (480, 640))
    assert np.abs(M - np.float64([[1, 0, 150], [0, 1, 150], [0, 0, 1]])).max() < 1e-3
    frames = ir.random_frames(14, 1, 480, 640, 3)
    got = ir.warp_u8(frames, M, (160, 380), border=0)[0]
    want = frames[0, 150:310, 150:530].transpose(2, 0, 1).astype(np.float64) / 255.0
    assert float(np.abs(got - want).max()) < 2e-4
    # a frame of another size than the camera's: the corners scale with it (add_edges :382-386)
    M2 = it.plate_matrix(pose, cam, (240, 960))
    assert np.abs(M2 - np.float64([[1.5, 0, 225], [0, 0.5, 75], [0, 0, 1]])).max() < 1e-3


def test_intake_names_are_exported_lazily():
    import yolo_amd
    assert yolo_amd.FrameIntake is it.FrameIntake and yolo_amd.warp_u8 is it.warp_u8
    assert yolo_amd.intake_matrix is it.intake_matrix and yolo_amd.rectify_plates is it.rectify_plates


def test_warp_entry_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    name = 'yolo_warp_u8_to_nchw'
    assert name in L.SIGNATURES
    proto = re.search(r'int %s\(([^)]*)\)' % name, h).group(1)
    assert len(proto.split(',')) == len(L.SIGNATURES[name][1]) == 16


def test_warp_entry_refuses_bad_arguments_without_a_gpu(lib):
    assert lib.yolo_version() == 5
    p = C.c_void_p(4096)                   # never dereferenced: validation comes before any launch
    #     frames y  M  gain  N  Hs  Ws  C  Ho  Wo border x0 y0 x1  y1  stream
    ok = [p,     p, p, None, 2, 48, 64, 3, 16, 24, 1,    0, 0, 63, 47, None]
    fn = lib.yolo_warp_u8_to_nchw
    for k in (0, 1, 2):                                                     # NULL frames / y / M
        a = list(ok); a[k] = None
        assert fn(*a) == L.EINVAL, k
    for k in (4, 5, 6, 7, 8, 9):                                            # N = 0, ... : non-positive sizes
        for v in (0, -3):
            a = list(ok); a[k] = v
            assert fn(*a) == L.EINVAL, (k, v)
    for k, v in ((7, 5), (7, 8), (10, 2), (10, -1)):                        # C > 4, border not in {0, 1}
        a = list(ok); a[k] = v
        assert fn(*a) == L.EUNSUPPORTED, (k, v)
    for k, v in ((13, -1), (11, 64), (14, 5), (12, 6)):                     # empty roi (x1 < x0, y1 < y0 with y0 = 6)
        a = list(ok); a[k] = v
        if k == 14:
            a[12] = 6
        if k == 12:
            a[14] = 5
        assert fn(*a) == L.EINVAL, (k, v)
    for k, v in ((11, -1), (12, -1), (13, 64), (14, 48)):                   # roi outside the frame
        a = list(ok); a[k] = v
        assert fn(*a) == L.EINVAL, (k, v)
