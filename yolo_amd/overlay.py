"""The drawing end of the video node on the device: the car box, the NMS boxes, the plate edges and the clipped plate, from rows that
never leave the device.

  FrameOverlay(camera, ...)(frames, pred=, lp=, nms=)   <- Video.visualize (car/video_node.py:309-326): cv2_add_bbox (yolo_cv.py:239-270)
                                                           + CarLPVideo.visualize_carlp (car_and_LP/carLP_video_node.py:74-86):
                                                           ProjectRectangle6D.add_edges (licence_plate_render/__init__.py:379-402)

  FrameOverlay(..., labels=True, names=)(..., pose=)    <- what cv2_add_bbox_text (yolo_cv.py:273-282) is for: class, score and azimuth
                                                           on every box, in a bitmap font (BitmapFont / default_font)

Three launches on the current stream, no synchronisation: yolo_overlay_shapes (the shape table, the plate's inverse map and lp_valid,
include/yolo_amd.h), yolo_warp_u8_to_nchw (the clipped plate, read from the frames BEFORE they are drawn on, as add_edges clips before
it draws), yolo_overlay_draw.  With labels=True two more: yolo_overlay_labels after the shapes (the text and place of every slot's
label), yolo_overlay_text after the draw (the text lies over every shape).  The pixels are this library's own rules (4 dist^2 <= t^2
for lines, the font's bits for text, both exact), not cv2.polylines' or cv2.putText's: cv2 is not installed here.  The azimuth and
the depth lookup of Video.process are Detector.pose_device (yolo_pose_top1).  The radar plot is not offered."""
import numpy as np

from . import lib as L

SLOT_WORDS = 12
MAX_SLOTS = 128
LABEL_WORDS = 16
LABEL_CHARS = 40
NAME_BYTES = 16
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


class BitmapFont(object):
    """A fixed-cell bitmap font for yolo_overlay_text: masks (nglyph, cell_h) uint32, bit c of masks[g][r] (bit 0 = the leftmost
    column) the ink of column c, row r of the glyph of byte first_code + g; cell_w <= 32 columns, cell_h <= 32 rows, at most 256
    glyphs; advance (default cell_w) is the distance between two cell origins in font pixels."""

    def __init__(self, masks, cell_w, advance=None, first_code=32):
        masks = np.ascontiguousarray(masks)
        if masks.ndim != 2 or masks.dtype.kind not in 'iu' or not 1 <= masks.shape[0] <= 256 or not 1 <= masks.shape[1] <= 32:
            raise ValueError('masks should be an integer array (1..256 glyphs, 1..32 rows)')
        self.cell_w, self.cell_h = int(cell_w), int(masks.shape[1])
        if not 1 <= self.cell_w <= 32:
            raise ValueError('cell_w should be in 1..32')
        if masks.min() < 0 or int(masks.max()) >> self.cell_w:
            raise ValueError('a mask has ink outside its %d columns' % self.cell_w)
        self.masks = masks.astype(np.uint32)
        self.advance = self.cell_w if advance is None else int(advance)
        if self.advance < self.cell_w:
            raise ValueError('advance should be at least cell_w')
        self.first_code = int(first_code)
        self.nglyph = int(masks.shape[0])


def default_font():
    """PIL's built-in bitmap font as a BitmapFont: the codes 32..126, each rendered once into a mode-'L' cell and thresholded.
    Nothing of PIL's is stored in this package; where this PIL has no bitmap font, bring one: FrameOverlay(font=BitmapFont(...))."""
    from PIL import Image, ImageDraw, ImageFont
    if hasattr(ImageFont, 'load_default_imagefont'):
        font = ImageFont.load_default_imagefont()
    else:
        font = ImageFont.load_default()
        if not isinstance(font, ImageFont.ImageFont):
            raise RuntimeError('this PIL has no built-in bitmap font (load_default() gave %s): pass font=BitmapFont(...) to '
                               'FrameOverlay' % type(font).__name__)
    codes = range(32, 127)
    boxes = [font.getbbox(chr(c)) for c in codes]
    cell_w, cell_h = max(b[2] for b in boxes), max(b[3] for b in boxes)
    if not (1 <= cell_w <= 32 and 1 <= cell_h <= 32):
        raise RuntimeError('PIL\'s built-in font has %d x %d cells, beyond 32 x 32: pass font=BitmapFont(...)' % (cell_w, cell_h))
    masks = np.zeros((len(codes), cell_h), np.uint32)
    weights = (1 << np.arange(cell_w)).astype(np.uint32)
    for g, c in enumerate(codes):
        cell = Image.new('L', (cell_w, cell_h), 0)
        ImageDraw.Draw(cell).text((0, 0), chr(c), fill=255, font=font)
        masks[g] = ((np.asarray(cell) >= 128) * weights).sum(axis=1)
    return BitmapFont(masks, cell_w, first_code=32)


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
    next call with that size.  Runs on the current stream and does not synchronise.

    labels=True writes a text label on every enabled shape, [name ' '] score [' ' degrees], over the box's top-left corner (moved
    inside the frame where it would leave it), in `font` (a BitmapFont; None: default_font()) enlarged font_scale times, label_gap
    pixels from the box, on a ground box of colour label_ground grown by label_pad pixels (None: no ground box), in the shape's
    colour.  names: the class names (bytes or ASCII str, at most 16 bytes each), names[c] for an NMS box of class c ('class' mode)
    and for the top-1 box the class of `pose`.  The call then also takes pose=(N,4) float32 [azimuth, radius, depth, class] of
    Detector.pose_device -- the top-1 label's name and, with show_azimuth, its azimuth in degrees -- and nms_scores=(N,post_nms)
    float32, the kept scores of Detector.nms / decode_nms (without them an NMS label shows its row's column 0).  `.labels` is the
    label table of the last call (include/yolo_amd.h, yolo_overlay_labels).  With labels=False nothing changes."""

    def __init__(self, camera=None, car_threshold=0.5, LP_threshold=0.5, thickness=2, use_r=False, car_color=PALETTE[4],
                 LP_color=(0, 0, 255), palette=PALETTE, LP_size=(160, 380), device='cuda:0', labels=False, names=None, font=None,
                 font_scale=1, label_gap=4, label_pad=1, label_ground=(0, 0, 0), show_azimuth=True):
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
        self.table = self.vertices = self.matrices = self.labels = None
        self.with_labels = bool(labels)
        if self.with_labels:
            if font is None:
                font = default_font()
            if not isinstance(font, BitmapFont):
                raise ValueError('font should be a BitmapFont')
            self.font = font
            self._font = torch.from_numpy(font.masks.view(np.int32)).to(self.device)
            self.font_scale, self.label_gap, self.label_pad = int(font_scale), int(label_gap), int(label_pad)
            if not 1 <= self.font_scale <= 16 or self.label_gap < 0 or self.label_pad < 0:
                raise ValueError('font_scale should be in 1..16, label_gap and label_pad not negative')
            self._ground = 0 if label_ground is None else 1
            self._ground_colour = 0 if label_ground is None else _pack(label_ground)
            self.show_azimuth = bool(show_azimuth)
            table = np.zeros((len(names) if names is not None else 0, NAME_BYTES), np.uint8)
            for k in range(table.shape[0]):
                raw = names[k].encode('ascii') if isinstance(names[k], str) else bytes(names[k])
                if len(raw) > NAME_BYTES or 0 in raw:
                    raise ValueError('a class name is at most %d bytes without a zero byte: %r' % (NAME_BYTES, names[k]))
                table[k, :len(raw)] = np.frombuffer(raw, np.uint8)
            self._names = torch.from_numpy(table).to(self.device) if table.shape[0] else None
            self._label = {}              # (N, K) -> labels

    def _rows(self, t, name, width, N):
        import torch
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 or t.shape[0] != N
                or t.shape[1] < width or not t.is_contiguous()):
            raise ValueError('%s should be a contiguous float32 tensor (%d, >=%d) on %s' % (name, N, width, self.device))
        return t

    def __call__(self, frames, pred=None, lp=None, nms=None, out=None, nms_mode='class', pose=None, nms_scores=None):
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
        labels = None
        if self.with_labels:
            if pose is not None and (pred is None or not torch.is_tensor(pose) or pose.dtype != torch.float32
                                     or pose.device != self.device or tuple(pose.shape) != (N, 4) or not pose.is_contiguous()):
                raise ValueError('pose should be a contiguous float32 tensor (%d, 4) on %s, given with pred' % (N, self.device))
            if nms_scores is not None and (nms is None or not torch.is_tensor(nms_scores) or nms_scores.dtype != torch.float32
                                           or nms_scores.device != self.device or tuple(nms_scores.shape) != (N, post)
                                           or not nms_scores.is_contiguous()):
                raise ValueError('nms_scores should be a contiguous float32 tensor (%d, post_nms) on %s, given with nms' % (N, self.device))
            labels = self._label.get((N, K))
            if labels is None:
                labels = self._label[(N, K)] = torch.empty((N, K, LABEL_WORDS), dtype=torch.int32, device=self.device)
        elif pose is not None or nms_scores is not None:
            raise ValueError('pose and nms_scores are for the text labels: FrameOverlay(labels=True)')
        stream = L.stream_ptr()
        L.check(self._lib.yolo_overlay_shapes(
            L.ptr(rows), L.ptr(kept), L.ptr(count), nbox, rows_C, post, cpb, L.ptr(self._palette), int(self._palette.shape[0]),
            L.ptr(pred), pred_C, self.car_threshold, int(self.use_r), self._car,
            L.ptr(lp), cam.fx if cam else 0.0, cam.fy if cam else 0.0, cam.cx if cam else 0.0, cam.cy if cam else 0.0,
            cam.w if cam else 0, cam.h if cam else 0, self.LP_threshold, self._lp, self.LP_size[0], self.LP_size[1],
            N, H, W, self.thickness, L.ptr(table), K, L.ptr(verts), L.ptr(mats), L.ptr(valid), stream), 'overlay_shapes')
        if labels is not None:
            f = self.font
            L.check(self._lib.yolo_overlay_labels(
                L.ptr(table), L.ptr(rows), L.ptr(kept), L.ptr(count), L.ptr(nms_scores), nbox, rows_C, post, cpb, L.ptr(pred), pred_C,
                L.ptr(pose), int(self.show_azimuth), L.ptr(lp), L.ptr(self._names), 0 if self._names is None else int(self._names.shape[0]),
                f.cell_w, f.cell_h, f.advance, self.font_scale, self.label_gap, self.label_pad, self._ground, self._ground_colour,
                N, H, W, K, L.ptr(labels), stream), 'overlay_labels')
        if lp is not None:
            # the same call rectify_plates makes (border 0), with the device-made matrices, on the frames as they came
            L.check(self._lib.yolo_warp_u8_to_nchw(L.ptr(frames), L.ptr(clipped), L.ptr(mats), None, N, H, W, Cc, self.LP_size[0],
                                                   self.LP_size[1], 0, 0, 0, W - 1, H - 1, stream), 'warp_u8_to_nchw')
        if out is not None:
            out.copy_(frames)
            frames = out
        L.check(self._lib.yolo_overlay_draw(L.ptr(frames), L.ptr(table), N, H, W, Cc, K, stream), 'overlay_draw')
        if labels is not None:
            # after the draw and after the clipped plate was read: the text lies over every shape and never reaches `clipped`
            f = self.font
            L.check(self._lib.yolo_overlay_text(L.ptr(frames), L.ptr(labels), L.ptr(self._font), f.nglyph, f.first_code, f.cell_w, f.cell_h,
                                                f.advance, self.font_scale, self.label_pad, N, H, W, Cc, K, stream), 'overlay_text')
        self.table, self.vertices, self.matrices, self.labels = table, verts, mats, labels
        return frames, clipped, valid
