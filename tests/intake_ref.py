"""The frame intake restated in numpy (the role tests/eval_ref.py plays for the evaluation): yolo_warp_u8_to_nchw's definition
in include/yolo_amd.h, every operation in float32 and in the header's order, so an IEEE device reproduces it bit for bit."""
import numpy as np

f32 = np.float32
IDX_LIMIT = f32(2.0 ** 30)


def warp_u8(frames, M, out_hw, border=0, roi=None, gain=None):
    """frames (N,Hs,Ws,C) uint8, M (N,3,3) or (3,3) (cast to float32 first, as the device matrix is), border 0 = taps outside
    roi read 0, 1 = tap indices clamped into roi; roi (x0, y0, x1, y1) inclusive (default: the frame); gain (C,) or None.
    -> (N,C,Ho,Wo) float32."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[None]
    assert frames.dtype == np.uint8 and frames.ndim == 4
    N, Hs, Ws, C = frames.shape
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    M = np.broadcast_to(np.asarray(M, np.float64).astype(f32).reshape(-1, 9), (N, 9))
    rx0, ry0, rx1, ry1 = (0, 0, Ws - 1, Hs - 1) if roi is None else [int(v) for v in roi]
    assert 0 <= rx0 <= rx1 < Ws and 0 <= ry0 <= ry1 < Hs
    g = np.ones(C, f32) if gain is None else np.asarray(gain, np.float64).astype(f32).reshape(C)
    j = np.broadcast_to(np.arange(Wo, dtype=f32)[None, :], (Ho, Wo))
    i = np.broadcast_to(np.arange(Ho, dtype=f32)[:, None], (Ho, Wo))
    out = np.empty((N, C, Ho, Wo), f32)
    with np.errstate(all='ignore'):
        for n in range(N):
            m = M[n]
            u = (m[0] * j + m[1] * i) + m[2]
            v = (m[3] * j + m[4] * i) + m[5]
            w = (m[6] * j + m[7] * i) + m[8]
            sx, sy = u / w, v / w
            x0f, y0f = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0f, sy - y0f
            assert fx.dtype == f32 and fy.dtype == f32
            x0 = np.fmin(np.fmax(x0f, -IDX_LIMIT), IDX_LIMIT).astype(np.int64)
            y0 = np.fmin(np.fmax(y0f, -IDX_LIMIT), IDX_LIMIT).astype(np.int64)
            x1, y1 = x0 + 1, y0 + 1
            cx0, cx1 = np.clip(x0, rx0, rx1), np.clip(x1, rx0, rx1)
            cy0, cy1 = np.clip(y0, ry0, ry1), np.clip(y1, ry0, ry1)
            keep = border != 0
            inx0, inx1, iny0, iny1 = (cx0 == x0) | keep, (cx1 == x1) | keep, (cy0 == y0) | keep, (cy1 == y1) | keep
            img = frames[n]
            for c in range(C):
                pl = img[:, :, c].astype(f32)
                a = np.where(inx0 & iny0, pl[cy0, cx0], f32(0))
                b = np.where(inx1 & iny0, pl[cy0, cx1], f32(0))
                cc = np.where(inx0 & iny1, pl[cy1, cx0], f32(0))
                d = np.where(inx1 & iny1, pl[cy1, cx1], f32(0))
                top = a + fx * (b - a)
                bot = cc + fx * (d - cc)
                val = top + fy * (bot - top)
                res = (val / f32(255.0)) * g[c]
                assert res.dtype == f32
                out[n, c] = res
    return out


# ---- shared cases and independent helpers of tests/test_intake_host.py and tests/test_gpu_intake.py -------------------------
# (src_hw, dst_hw, clip, flip).  The first six are the affine cases the intake was specified with.  The sixth, an upscale of a
# "crop", crops nothing: int(0.2 * 9 / 2.) = int(0.2 * 7 / 2.) = 0.  The seventh is the same idea with a crop that exists
# (3 rows and 3 columns off each side): it passes only if taps clamp to the roi and not to the frame.
AFFINE_CASES = [((37, 53), (16, 24), (1., 1.), None),
                ((37, 53), (16, 24), (0.8, 0.9), 1),
                ((9, 7), (20, 30), (1., 1.), -1),
                ((48, 64), (13, 13), (0.75, 1.), 0),
                ((5, 5), (5, 5), (1., 1.), None),
                ((9, 7), (20, 30), (0.8, 0.8), None),
                ((19, 17), (40, 30), (0.6, 0.6), None)]


def case_id(case):
    (H, W), (h, w), clip, flip = case
    return '%dx%d-%dx%d-clip%g_%g-flip%s' % (H, W, h, w, clip[0], clip[1], flip)


def random_frames(seed, N, H, W, C):
    """Noise: neighbouring pixels differ by up to a full level range, the steepest slope a tap error can meet."""
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, C), dtype=np.uint8)


def crop_flip(img, clip, flip):
    """yolo_cv.cv2_flip_and_clip_frame (yolo_cv.py:285-318) on an (H,W,C) array, cv2.flip as numpy slicing."""
    if clip[0] < 1:
        top = int((1 - clip[0]) * img.shape[0] / 2.)
        img = img[top:img.shape[0] - top]
    if clip[1] < 1:
        left = int((1 - clip[1]) * img.shape[1] / 2.)
        img = img[:, left:img.shape[1] - left]
    if flip == 1:
        img = img[:, ::-1]
    elif flip == 0:
        img = img[::-1]
    elif flip == -1:
        img = img[::-1, ::-1]
    return img
