"""The drawing end of the video node on the device: the car box, the NMS boxes, the plate edges and the clipped plate, from rows that
never leave the device.

  FrameOverlay(camera, ...)(frames, pred=, lp=, nms=)   <- Video.visualize (car/video_node.py:309-326): cv2_add_bbox (yolo_cv.py:239-270)
                                                           + CarLPVideo.visualize_carlp (car_and_LP/carLP_video_node.py:74-86):
                                                           ProjectRectangle6D.add_edges (licence_plate_render/__init__.py:379-402)

Three launches on the current stream, no synchronisation: yolo_overlay_shapes (the shape table, the plate's inverse map and lp_valid,
include/yolo_amd.h), yolo_warp_u8_to_nchw (the clipped plate, read from the frames BEFORE they are drawn on, as add_edges clips before
it draws), yolo_overlay_draw.  The pixels are this library's own rule (4 dist^2 <= t^2, exact), not cv2.polylines': cv2 is not
installed here.  Text labels (cv2_add_bbox_text), the radar plot and the depth lookup are not offered."""
import numpy as np

from . import lib as L

SLOT_WORDS = 12
MAX_SLOTS = 128
# yolo_cv._color (yolo_modules/yolo_cv.py:11-20); cv2_add_bbox is called with index 4 (car/video_node.py:317)
PALETTE = ((255, 255, 0), (255, 0, 255), (0, 255, 255), (0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255), (0, 0, 0))


def _colour4(c):
    c = [int(v) for v in c]
    if not 1 <= len(c) <= 4 or any(v < 0 or v > 255 for v in c):
        raise ValueError('a colour is 1..4 bytes')
    return c + [255] * (4 - len(c))


def _pack(c):
    c = _colour4(c)
    return c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24)


class FrameOverlay(object):
    """ov = FrameOverlay(camera); frames_out, clipped, lp_valid = ov(frames, pred=pred, lp=lp_rows, nms=(rows, kept, count))

    frames: device uint8 (N,H,W,C), C in 1..4, contiguous (any byte offset).  Each source is optional, at least one is needed:
      nms   (rows (N,nbox,C'), kept (N,post_nms) int32, kept_count (N,) int32) as Detector.nms / decode_nms return them, nms_mode the
            mode they were made with ('class': candidate id = box * ncls + class, 'obj': id = box); one box per kept candidate in the
            colour palette[class % len(palette)]
      pred  (N,C') float32 rows [score, y, x, h, w, rot, ...] of Detector.predict_device: the box, drawn iff score > car_threshold,
            rotated by -rot iff use_r
      lp    (N,7) float32 rows [score, X, Y, Z, r1, r2, r3] of detect.predict_LP_rows: the plate's edges, drawn iff score > LP_threshold
    painted in that order (the plate on top).  -> (frames, clipped (N,C,LP_size[0],LP_size[1]) float32 0..1, lp_valid (N,) uint8); the
    last two are None without lp; clipped is 0 where lp_valid is 0 (score not above the threshold, or a pose whose corners do not
    determine a map).  out=None draws in place; otherwise frames is copied into out (same shape) and out is drawn on and returned.
    Buffers are cached per batch size: after the first call with a size nothing is allocated, and `clipped`, `lp_valid` and the
    attributes table / vertices / matrices (the device-made shape table of the last call) are THE OBJECT'S buffers, overwritten by the
    next call with that size.  Runs on the current stream and does not synchronise."""

    def __init__(self, camera=None, car_threshold=0.5, LP_threshold=0.5, thickness=2, use_r=False, car_color=PALETTE[4],
                 LP_color=(0, 0, 255), palette=PALETTE, LP_size=(160, 380), device='cuda:0'):
        import torch
        from . import render
        if camera is not None and not isinstance(camera, render.PlateCamera):
            camera = render.PlateCamera(camera)
        self.camera = camera
        self.car_threshold, self.LP_threshold = float(car_threshold), float(LP_threshold)
        self.thickness, self.use_r = int(thickness), bool(use_r)
        if not 1 <= self.thickness <= 255:
            raise ValueError('thickness should be in 1..255')
        self.LP_size = (int(LP_size[0]), int(LP_size[1]))
        if self.LP_size[0] <= 0 or self.LP_size[1] <= 0:
            raise ValueError('LP_size should be positive')
        self.device = L.resolve_device(device)
        self._lib = L.load()
        self._car, self._lp = _pack(car_color), _pack(LP_color)
        pal = np.array([_colour4(c) for c in palette], np.uint8)
        if pal.shape[0] < 1:
            raise ValueError('palette should hold at least one colour')
        self._palette = torch.from_numpy(pal).to(self.device)
        self._shape = {}                  # (N, K) -> (table, vertices)
        self._plate = {}                  # N -> (matrices, lp_valid)
        self._clip = {}                   # (N, C) -> clipped
        self.table = self.vertices = self.matrices = None

    def _rows(self, t, name, width, N):
        import torch
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or t.shape[0] != N
                or t.shape[1] < width or not t.is_contiguous()):
            raise ValueError('%s should be a contiguous float32 tensor (%d, >=%d) on %s' % (name, N, width, self.device))
        return t

    def __call__(self, frames, pred=None, lp=None, nms=None, out=None, nms_mode='class'):
        import torch
        L.require_current_device(self.device, 'this FrameOverlay')
        if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.device != self.device or frames.dim() != 4
                or not frames.is_contiguous() or not 1 <= frames.shape[3] <= 4 or 0 in frames.shape):
            raise ValueError('frames should be a contiguous uint8 tensor (N,H,W,C) with 1..4 channels on %s' % (self.device,))
        N, H, W, Cc = frames.shape
        if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != self.device
                                or tuple(out.shape) != tuple(frames.shape) or not out.is_contiguous()):
            raise ValueError('out should be a contiguous uint8 tensor of shape %r on %s' % (tuple(frames.shape), self.device))
        if pred is None and lp is None and nms is None:
            raise ValueError('nothing to draw: give pred, lp or nms')
        rows = kept = count = None
        nbox = rows_C = post = 0
        cpb = 1
        if nms is not None:
            rows, kept, count = nms
            if (not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.device != self.device or rows.dim() != 3
                    or rows.shape[0] != N or rows.shape[2] < 5 or not rows.is_contiguous()):
                raise ValueError('nms rows should be a contiguous float32 tensor (%d, nbox, >=5) on %s' % (N, self.device))
            nbox, rows_C = int(rows.shape[1]), int(rows.shape[2])
            if (not torch.is_tensor(kept) or kept.dtype != torch.int32 or kept.device != self.device or kept.dim() != 2
                    or kept.shape[0] != N or kept.shape[1] < 1 or not kept.is_contiguous()):
                raise ValueError('nms kept ids should be a contiguous int32 tensor (%d, post_nms) on %s' % (N, self.device))
            if (not torch.is_tensor(count) or count.dtype != torch.int32 or count.device != self.device
                    or tuple(count.shape) != (N,) or not count.is_contiguous()):
                raise ValueError('nms kept count should be an int32 tensor (%d,) on %s' % (N, self.device))
            post = int(kept.shape[1])
            if nms_mode not in ('class', 'obj'):
                raise ValueError("nms_mode should be 'class' or 'obj'")
            cpb = (rows_C - 6) if nms_mode == 'class' else 1
            if cpb < 1:
                raise ValueError("nms_mode 'class' needs rows with class columns")
        pred_C = 0
        if pred is not None:
            pred = self._rows(pred, 'pred', 6, N)
            pred_C = int(pred.shape[1])
        cam = self.camera
        if lp is not None:
            if cam is None:
                raise ValueError('lp rows need the camera: FrameOverlay(camera=...)')
            lp = self._rows(lp, 'lp', 7, N)
            if lp.shape[1] != 7:
                raise ValueError('lp should be (N,7) rows [score, X, Y, Z, r1, r2, r3]')
        K = post + (pred is not None) + (lp is not None)
        if K > MAX_SLOTS:
            raise ValueError('%d shapes per frame: at most %d' % (K, MAX_SLOTS))
        bufs = self._shape.get((N, K))
        if bufs is None:
            bufs = self._shape[(N, K)] = (torch.empty((N, K, SLOT_WORDS), dtype=torch.int32, device=self.device),
                                          torch.empty((N, K, 4, 2), dtype=torch.float32, device=self.device))
        table, verts = bufs
        mats = valid = clipped = None
        if lp is not None:
            pl = self._plate.get(N)
            if pl is None:
                pl = self._plate[N] = (torch.empty((N, 9), dtype=torch.float32, device=self.device),
                                       torch.empty((N,), dtype=torch.uint8, device=self.device))
            mats, valid = pl
            clipped = self._clip.get((N, Cc))
            if clipped is None:
                clipped = self._clip[(N, Cc)] = torch.empty((N, Cc) + self.LP_size, dtype=torch.float32, device=self.device)
        stream = L.stream_ptr()
        L.check(self._lib.yolo_overlay_shapes(
            L.ptr(rows), L.ptr(kept), L.ptr(count), nbox, rows_C, post, cpb, L.ptr(self._palette), int(self._palette.shape[0]),
            L.ptr(pred), pred_C, self.car_threshold, int(self.use_r), self._car,
            L.ptr(lp), cam.fx if cam else 0.0, cam.fy if cam else 0.0, cam.cx if cam else 0.0, cam.cy if cam else 0.0,
            cam.w if cam else 0, cam.h if cam else 0, self.LP_threshold, self._lp, self.LP_size[0], self.LP_size[1],
            N, H, W, self.thickness, L.ptr(table), K, L.ptr(verts), L.ptr(mats), L.ptr(valid), stream), 'overlay_shapes')
        if lp is not None:
            # the same call rectify_plates makes (border 0), with the device-made matrices, on the frames as they came
            L.check(self._lib.yolo_warp_u8_to_nchw(L.ptr(frames), L.ptr(clipped), L.ptr(mats), None, N, H, W, Cc, self.LP_size[0],
                                                   self.LP_size[1], 0, 0, 0, W - 1, H - 1, stream), 'warp_u8_to_nchw')
        if out is not None:
            out.copy_(frames)
            frames = out
        L.check(self._lib.yolo_overlay_draw(L.ptr(frames), L.ptr(table), N, H, W, Cc, K, stream), 'overlay_draw')
        self.table, self.vertices, self.matrices = table, verts, mats
        return frames, clipped, valid
