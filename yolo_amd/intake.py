"""The camera end of the pipeline on the device: uint8 HWC frames of any size -> the (N,3,h,w) float32 tensor net.forward takes.

  intake_matrix(src_hw, dst_hw, clip, flip)  <- yolo_cv.cv2_flip_and_clip_frame (yolo_cv.py:285-318) + cv2.resize(img, (w, h))
                                                (car/video_node.py:150,205, licence_plate/LPD_video_node.py:69) as ONE matrix
  warp_u8(frames, M, out_hw, ...)            <- the general call: yolo_warp_u8_to_nchw (csrc/intake.hip), which also does the
                                                /255 + HWC->CHW of yolo_gluon.cv_img_2_ndarray (yolo_gluon.py:335-357)
  FrameIntake(size, ...)(frames)             <- the video node's front end as one object (+ nd_white_balance, yolo_cv.py:224-231)
  rectify_plates(frames, poses, camera)      <- ProjectRectangle6D.add_edges' clipped_LP (licence_plate_render/__init__.py:379-402)

The sampler is a FLOAT bilinear one (its arithmetic is defined in include/yolo_amd.h).  cv2's uint8 INTER_LINEAR works with
11-bit fixed-point coefficients and rounds the result to an integer level, so the two differ by up to about half a level
(2e-3 after the /255); cv2 is not installed here and that difference is not pinned by a test."""
import numpy as np

from . import lib as L

BORDERS = {'constant': 0, 'replicate': 1}


def intake_matrix(src_hw, dst_hw, clip=(1., 1.), flip=None):
    """-> (M, roi): M float64 (3,3) maps an output pixel (column j, row i) of the (h, w) = dst_hw image to source pixel
    coordinates of the (H, W) = src_hw frame; roi = (x0, y0, x1, y1) inclusive is the crop rectangle.
    Crop as the reference does (top = int((1 - clip[0]) * H / 2.), bot = H - top, likewise the width), then cv2.flip's codes
    1 (left-right) / 0 (top-down) / -1 (both) on the crop -- any other value: no flip --, then cv2.resize's half-pixel
    geometry sx = (j + 0.5) * Wc / Wo - 0.5.  With border 'replicate' and this roi no tap reads outside what cv2.resize would
    have been given."""
    H, W = int(src_hw[0]), int(src_hw[1])
    Ho, Wo = int(dst_hw[0]), int(dst_hw[1])
    if H <= 0 or W <= 0 or Ho <= 0 or Wo <= 0:
        raise ValueError('sizes should be positive')
    top = int((1 - clip[0]) * H / 2.) if clip[0] < 1 else 0
    left = int((1 - clip[1]) * W / 2.) if clip[1] < 1 else 0
    Hc, Wc = H - 2 * top, W - 2 * left
    if Hc <= 0 or Wc <= 0:
        raise ValueError('clip %r leaves nothing of a %d x %d frame' % (clip, H, W))
    ax, ay = Wc / float(Wo), Hc / float(Ho)
    bx, by = 0.5 * ax - 0.5, 0.5 * ay - 0.5                 # crop coordinate of output pixel 0
    flip_x = flip is not None and flip in (1, -1)
    flip_y = flip is not None and flip in (0, -1)
    M = np.eye(3)
    M[0, 0], M[0, 2] = (-ax, left + (Wc - 1) - bx) if flip_x else (ax, left + bx)
    M[1, 1], M[1, 2] = (-ay, top + (Hc - 1) - by) if flip_y else (ay, top + by)
    return M, (left, top, left + Wc - 1, top + Hc - 1)


def _as_u8_batch(frames):
    """ndarray / tensor, (H,W,C) or (N,H,W,C) uint8 -> a contiguous torch tensor (N,H,W,C) on whatever side it lives."""
    import torch
    if isinstance(frames, np.ndarray):
        if frames.dtype != np.uint8:
            raise ValueError('frames should be uint8')
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError('frames should be a uint8 ndarray or torch tensor')
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[3] < 1 or frames.shape[3] > 4 or 0 in frames.shape:
        raise ValueError('expected frames of shape (H,W,C) or (N,H,W,C) with 1..4 channels')
    return frames.contiguous()


def _device_matrix(M, N, device):
    """(3,3) or (N,3,3), ndarray or tensor -> (N,9) float32 on the device."""
    import torch
    if not torch.is_tensor(M):
        M = torch.from_numpy(np.ascontiguousarray(np.asarray(M, np.float64).astype(np.float32)))
    M = M.to(device, torch.float32).reshape(-1, 9)
    if M.shape[0] == 1 and N > 1:
        M = M.expand(N, 9)
    if M.shape[0] != N:
        raise ValueError('expected one 3x3 matrix, or one per frame (%d)' % N)
    return M.contiguous()


def _launch(frames, M, out, border, roi, gain):
    N, Hs, Ws, Cc = frames.shape
    L.check(L.load().yolo_warp_u8_to_nchw(L.ptr(frames), L.ptr(out), L.ptr(M), L.ptr(gain), N, Hs, Ws, Cc, out.shape[2],
                                          out.shape[3], border, roi[0], roi[1], roi[2], roi[3], L.stream_ptr()), 'warp_u8_to_nchw')


def warp_u8(frames, M, out_hw, border='constant', roi=None, gain=None, out=None, device=None):
    """Bilinear inverse warp: frames uint8 (H,W,C) or (N,H,W,C), ndarray or tensor, host or device; M (3,3) or (N,3,3) maps an
    OUTPUT pixel (column j, row i) to source pixel coordinates (cv2's WARP_INVERSE_MAP convention; a device float32 tensor is
    used as it is).  border 'constant': taps outside roi read 0 (cv2.warpPerspective's default); 'replicate': tap indices
    are clamped into roi.  roi (x0, y0, x1, y1) inclusive, default the whole frame; gain: one factor per channel.
    -> (N,C,Ho,Wo) float32 /255 on the device (`out` when given), on the current stream, without synchronising.
    Host frames are uploaded to `device` (default: the current one, or out's)."""
    import torch
    if border not in BORDERS:
        raise ValueError("border should be 'constant' or 'replicate'")
    frames = _as_u8_batch(frames)
    if frames.is_cuda:
        dev = frames.device
    elif out is not None:
        dev = out.device
    else:
        dev = L.resolve_device(device if device is not None else 'cuda')
    L.require_current_device(dev, 'this warp_u8 call')
    if not frames.is_cuda:
        frames = frames.to(dev, non_blocking=True)
    N, Hs, Ws, Cc = frames.shape
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    if Ho <= 0 or Wo <= 0:
        raise ValueError('out_hw should be positive')
    if out is None:
        out = torch.empty((N, Cc, Ho, Wo), dtype=torch.float32, device=dev)
    elif (tuple(out.shape) != (N, Cc, Ho, Wo) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()):
        raise ValueError('out should be a contiguous float32 tensor of shape %r on %s' % ((N, Cc, Ho, Wo), dev))
    roi = (0, 0, Ws - 1, Hs - 1) if roi is None else tuple(int(v) for v in roi)
    if gain is not None:
        if not torch.is_tensor(gain):
            gain = torch.from_numpy(np.asarray(gain, np.float64).astype(np.float32))
        gain = gain.to(dev, torch.float32).reshape(-1).contiguous()
        if gain.shape[0] != Cc:
            raise ValueError('gain should have one factor per channel (%d)' % Cc)
    _launch(frames, _device_matrix(M, N, dev), out, BORDERS[border], roi, gain)
    return out


class FrameIntake(object):
    """intake = FrameIntake((h, w)); x = intake(frames); outs = net(x) -- cv2_flip_and_clip_frame + cv2.resize +
    cv_img_2_ndarray (+ nd_white_balance with white_balance = its bgr triple) of the reference's video nodes in one kernel.

    frames: uint8 (H,W,3) or (N,H,W,3), ndarray or tensor.  A host array goes through a pinned staging buffer and a
    non-blocking copy, a pinned tensor is copied from where it is, a device tensor is read in place.  The matrix is cached
    per source size, the buffers per (batch, source size): once a batch size has been seen a call allocates nothing -- the
    returned tensor is THE OBJECT'S buffer for that batch size and is overwritten by the next call with it (pass out= to
    keep results apart).  Runs on the current stream and does not synchronise.
    `frames` is the device uint8 (N,H,W,C) batch the last call read -- the uploaded staging buffer (overwritten by the next upload of
    that shape) or the caller's own tensor --, what FrameOverlay draws on; None before the first call.  The caller's tensor is held
    WEAKLY (the intake does not extend its life): None once the caller has dropped it."""

    def __init__(self, size, device='cuda:0', clip=(1., 1.), flip=None, white_balance=None):
        import torch
        self.size = (int(size[0]), int(size[1]))
        self.device = L.resolve_device(device)
        self.clip, self.flip = (float(clip[0]), float(clip[1])), flip
        self._lib = L.load()
        self._gain = None
        if white_balance is not None:
            wb = np.asarray(white_balance, np.float64).reshape(-1)
            if wb.shape[0] != 3:
                raise ValueError('white_balance should be a bgr triple')
            self._gain = torch.from_numpy(wb.astype(np.float32)).to(self.device)
        self._geom = {}                   # (H, W) -> (device (1,9) matrix, roi)
        self._mat = {}                    # (N, H, W) -> device (N,9) matrix
        self._stage = {}                  # (N, H, W, C) -> [pinned host buffer, device buffer, event of the last upload]
        self._out = {}                    # (N, C) -> device output
        self._read = None                 # the staging buffer of the last call, or a weak reference to the caller's device tensor

    @property
    def frames(self):
        import weakref
        if isinstance(self._read, weakref.ref):
            t = self._read()
            return None if t is None else _as_u8_batch(t)
        return self._read

    def matrix(self, src_hw):
        """(M float64 (3,3), roi) for frames of src_hw: intake_matrix with this object's size, clip and flip."""
        return intake_matrix(src_hw, self.size, self.clip, self.flip)

    def _matrix(self, N, H, W):
        import torch
        geom = self._geom.get((H, W))
        if geom is None:
            M, roi = self.matrix((H, W))
            geom = self._geom[(H, W)] = (torch.from_numpy(M.astype(np.float32).reshape(1, 9)).to(self.device), roi)
        mat = self._mat.get((N, H, W))
        if mat is None:
            mat = self._mat[(N, H, W)] = geom[0].expand(N, 9).contiguous()
        return mat, geom[1]

    def _upload(self, frames):
        import torch
        key = tuple(frames.shape)
        slot = self._stage.get(key)
        if slot is None:
            slot = self._stage[key] = [None, torch.empty(key, dtype=torch.uint8, device=self.device), torch.cuda.Event()]
        pinned, dev_buf, done = slot
        if frames.is_pinned():
            dev_buf.copy_(frames, non_blocking=True)
            return dev_buf
        if pinned is None:
            pinned = slot[0] = torch.empty(key, dtype=torch.uint8, pin_memory=True)
        else:
            done.synchronize()            # the previous upload has left the staging buffer (waits for that copy only)
        pinned.copy_(frames)
        dev_buf.copy_(pinned, non_blocking=True)
        done.record()
        return dev_buf

    def __call__(self, frames, out=None):
        import torch
        import weakref
        L.require_current_device(self.device, 'this FrameIntake')
        given = frames
        frames = _as_u8_batch(frames)
        if frames.shape[3] != 3 and self._gain is not None:
            raise ValueError('white_balance needs 3-channel frames')
        if frames.is_cuda:
            if frames.device != self.device:
                raise ValueError('frames live on %s, this FrameIntake on %s' % (frames.device, self.device))
        else:
            frames = self._upload(frames)
        N, H, W, Cc = frames.shape
        M, roi = self._matrix(N, H, W)
        shape = (N, Cc) + self.size
        if out is None:
            out = self._out.get((N, Cc))
            if out is None:
                out = self._out[(N, Cc)] = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError('out should be a contiguous float32 tensor of shape %r on %s' % (shape, self.device))
        _launch(frames, M, out, BORDERS['replicate'], roi, self._gain)
        self._read = weakref.ref(given) if (torch.is_tensor(given) and given.is_cuda) else frames
        return out


def plate_matrix(pose, camera, frame_hw, LP_size=(160, 380)):
    """add_edges' geometry (:380-397): PlateCamera.corners(pose) scaled from the camera's size to the frame's, and the
    homography from the LP_size plate image (corners in the reference's order: bottom-right, bottom-left, top-left,
    top-right) to those -- the INVERSE map cv2.warpPerspective derives from its M.  -> float64 (3,3)."""
    from . import render
    corner_pts = camera.corners(pose)                                     # float32 (4,2), as the reference's __call__ returns
    corner_pts[:, 0] = corner_pts[:, 0] * (frame_hw[1] / float(camera.w))
    corner_pts[:, 1] = corner_pts[:, 1] * (frame_hw[0] / float(camera.h))
    LP_corner = np.float32([[LP_size[1], LP_size[0]], [0, LP_size[0]], [0, 0], [LP_size[1], 0]])
    return render.homography(LP_corner, corner_pts)


def rectify_plates(frames, poses, camera, LP_size=(160, 380), out=None):
    """ProjectRectangle6D.add_edges' clipped_LP on the device: frames uint8 (H,W,C) / (N,H,W,C), poses (6,) / (N,6) rows
    [X, Y, Z mm, r1, r2, r3 rad] (predict_LP's columns 1..6), camera: a render.PlateCamera or the calibration dict it takes.
    -> (N,C,LP_size[0],LP_size[1]) float32 0..1, 0 where the plate leaves the frame (border 'constant')."""
    from . import render
    if not isinstance(camera, render.PlateCamera):
        camera = render.PlateCamera(camera)
    frames = _as_u8_batch(frames)
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    if poses.shape[0] != frames.shape[0]:
        raise ValueError('expected one pose per frame (%d)' % frames.shape[0])
    hw = (int(frames.shape[1]), int(frames.shape[2]))
    M = np.stack([plate_matrix(p, camera, hw, LP_size) for p in poses])
    return warp_u8(frames, M, LP_size, border='constant', out=out)
