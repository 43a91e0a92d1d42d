"""The background batch of a training step made on the device: yolo_gluon.load_background + ImageIter_next_batch
(yolo_modules/yolo_gluon.py:43-97) without mxnet's host iterator.

  load_background(mode, bs, h, w)       <- BackgroundBank(source, h, w, mode=mode): the decoded images stay RESIDENT on the device as
                                           4-byte pixels with their mip levels (render.mip_chain), uploaded once
  ImageIter_next_batch(BG_iter)         <- bank.next_batch(bs): the host draws one row of scalars per image (draw_params: which image,
                                           crop, mirror, mip level, colour map); yolo_bg_stats + yolo_bg_render (csrc/background.hip)
                                           write the (bs,3,h,w) float32 0..255 batch RenderCar.render_device / render take as bg

The reference's iterator is ImageIter(rand_crop, rand_resize, rand_mirror, brightness = saturation = contrast = 0.5, hue = 1.0,
pca_noise = 0, inter_method = 10): per image a JPEG decode, a random-sized crop, a resize, a mirror and the colour jitters on host
cores -- which is why car/YOLO.py:323 fetches a new background batch only every tenth step.  Here a batch costs two kernels.

What is NOT mxnet's pixels: the resize is a float bilinear tap on a mip level (mxnet's inter_method=10 draws one of OpenCV's
interpolations at random per image); nothing is rounded to 8 bits between the stages (mxnet resizes uint8, then casts); and the crop
rule below is restated from recall, mxnet is absent here -- [recalled]."""
import math
import os
import random

import numpy as np

from .intake import intake_matrix
from .render import ColorAugmenter, SpriteAtlas, mip_chain

# one row per output image (include/yolo_amd.h, yolo_bg_render):
#   0 has-image   1 h   2 w (of the mip level)   3..6 roi x0, y0, x1, y1 (inclusive, level pixels)   8,9 the level's byte offset (int64)
#   10..15 a0..a5: output pixel index -> level pixel index   16..24 A   25..33 D   34..36 e                (7, 37..39: padding)
BG_ROW_WORDS = 40
CROP_AREA = (0.08, 1.0)                                           # RandomSizedCropAug(size, 0.08, (3/4, 4/3)) [recalled]
CROP_RATIO = (3.0 / 4.0, 4.0 / 3.0)
CROP_TRIES = 10


def random_sized_crop(h, w, out_hw):
    """mxnet.image.random_size_crop as CreateAugmenter builds it for rand_crop + rand_resize (RandomSizedCropAug(size, 0.08,
    (3/4, 4/3))) on an (h, w) image, WITHOUT the pixels -- [recalled]: up to 10 tries of an area fraction uniform in [0.08, 1] and an
    aspect log-uniform in [3/4, 4/3]; the first try that fits is placed with two random.randint draws.  No try fits: the largest
    rectangle of the output's aspect ratio that fits, centred (mxnet's center_crop through scale_down, which is this rectangle
    whenever the image is the smaller one).  Draws from Python's `random`, as mxnet's image module does.
    -> (x0, y0, cw, ch, fallback)."""
    for _ in range(CROP_TRIES):
        target = random.uniform(CROP_AREA[0], CROP_AREA[1]) * h * w
        ratio = math.exp(random.uniform(math.log(CROP_RATIO[0]), math.log(CROP_RATIO[1])))
        cw = int(round(math.sqrt(target * ratio)))
        ch = int(round(math.sqrt(target / ratio)))
        if 1 <= cw <= w and 1 <= ch <= h:
            x0 = random.randint(0, w - cw)
            y0 = random.randint(0, h - ch)
            return x0, y0, cw, ch, False
    Ho, Wo = out_hw
    if w * Ho >= h * Wo:                                          # the image is the wider one: full height
        ch, cw = h, max(1, (h * Wo) // Ho)
    else:
        cw, ch = w, max(1, (w * Ho) // Wo)
    return (w - cw) // 2, (h - ch) // 2, cw, ch, True


def unpack_row(row):
    """One int32 row -> dict of its fields (the layout of include/yolo_amd.h)."""
    row = np.ascontiguousarray(row, np.int32)
    fl = row.view(np.float32)
    return dict(has=int(row[0]), h=int(row[1]), w=int(row[2]), roi=[int(v) for v in row[3:7]], off=int(row[8:10].view(np.int64)[0]),
                a=fl[10:16].copy(), A=fl[16:25].reshape(3, 3).copy(), D=fl[25:34].reshape(3, 3).copy(), e=fl[34:37].copy())


def make_row(off, h, w, roi, a, A=None, D=None, e=None, has=1):
    """One parameter row (BG_ROW_WORDS int32 words, floats stored by bit pattern); A, D, e default to the identity colour map."""
    row = np.zeros(BG_ROW_WORDS, np.int32)
    fl = row.view(np.float32)
    row[0], row[1], row[2] = has, h, w
    row[3:7] = roi
    row[8:10] = np.array([off], np.int64).view(np.int32)
    fl[10:16] = np.asarray(a, np.float64).reshape(6).astype(np.float32)
    fl[16:25] = (np.eye(3) if A is None else np.asarray(A, np.float64)).reshape(9).astype(np.float32)
    fl[25:34] = (np.zeros((3, 3)) if D is None else np.asarray(D, np.float64)).reshape(9).astype(np.float32)
    fl[34:37] = (np.zeros(3) if e is None else np.asarray(e, np.float64)).astype(np.float32)
    return row


def _load_dir(path):
    """Every file of a directory that PIL opens, sorted by name, as (h, w, 3) uint8 RGB arrays."""
    from PIL import Image
    out = []
    for name in sorted(os.listdir(path)):
        full = os.path.join(path, name)
        if not os.path.isfile(full):
            continue
        try:
            with Image.open(full) as im:
                out.append(np.asarray(im.convert('RGB'), np.uint8))
        except (OSError, ValueError):                             # (not an image PIL opens)
            continue
    return out


def _shrink(im, max_side):
    """An (h, w, 3) uint8 image whose longer side exceeds max_side, resized by PIL (bilinear) so that it is max_side."""
    from PIL import Image
    f = max_side / float(max(im.shape[:2]))
    size = (max(1, int(round(im.shape[1] * f))), max(1, int(round(im.shape[0] * f))))
    return np.asarray(Image.fromarray(im).resize(size, Image.BILINEAR), np.uint8)


class BackgroundBank(object):
    """bank = BackgroundBank(source, h, w); bg = bank.next_batch(B) -- the (B,3,h,w) float32 0..255 device tensor
    RenderCar.render_device takes.

    source: a directory (every file PIL opens, sorted by name, converted to RGB) or a sequence of (h,w,3) uint8 arrays;
    max_side: images whose longer side exceeds it are shrunk once at load (PIL, bilinear) to bound the bank's size.
    mode 'train': the images are visited in a shuffled order, reshuffled at each wrap (random.shuffle, ImageIter's shuffle=True);
    'val': in order, wrapping (what ImageIter_next_batch's reset amounts to).  augment=False: the whole image, no mirror, the
    identity colour map (only the resize is left).

    `data` is the bank (uint8: every image as 4-byte pixels R, G, B, 255 followed by its mip levels, packed densely),
    `table[s]` lists (byte offset, h, w) per level of image s and stays on the host, `size[s]` is its (h, w)."""
    pick_level = SpriteAtlas.pick_level                           # the same rule, on this object's `table`

    def __init__(self, source, h, w, device='cuda:0', mode='train', max_side=None, augment=True):
        if mode not in ('train', 'val'):
            raise ValueError("mode should be 'train' or 'val'")
        self.h, self.w = int(h), int(w)
        if self.h <= 0 or self.w <= 0:
            raise ValueError('the output size should be positive')
        self.device, self.mode = device, mode
        self.augs = ColorAugmenter(brightness=0.5, contrast=0.5, saturation=0.5, hue=1.0, pca_noise=0) if augment else None
        images = _load_dir(os.fspath(source)) if isinstance(source, (str, os.PathLike)) else [np.asarray(im) for im in source]
        if not images:
            raise ValueError('no background images in %r' % (source,))
        self.table, self.size = [], []
        chunks, off = [], 0
        for im in images:
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or 0 in im.shape:
                raise ValueError('background images should be (h, w, 3) uint8')
            if max_side is not None and max(im.shape[:2]) > max_side:
                im = _shrink(im, max_side)
            px = np.full(im.shape[:2] + (4,), 255, np.uint8)
            px[..., :3] = im
            rows = []
            for lv in mip_chain(px):
                rows.append((off, lv.shape[0], lv.shape[1]))
                chunks.append(lv.reshape(-1))
                off += lv.size
            self.table.append(rows)
            self.size.append((im.shape[0], im.shape[1]))
        self.data = np.concatenate(chunks)
        self._order, self._cursor = list(range(len(self.table))), 0

    def __len__(self):
        return len(self.table)

    def reset(self):
        """Back to where a new object starts: the first image of the first epoch ('train': the next draw shuffles the sorted
        order, so the same seed gives the same epochs again)."""
        self._order, self._cursor = list(range(len(self.table))), 0

    def _next_index(self):
        if self._cursor == 0 and self.mode == 'train':
            random.shuffle(self._order)
        s = self._order[self._cursor]
        self._cursor = (self._cursor + 1) % len(self._order)
        return s

    def param_row(self, s, crop, mirror=False, color=None):
        """One parameter row for image s cropped to crop = (x0, y0, cw, ch) (level-0 pixels), mirrored or not, resized to this
        object's (h, w); color = (A, D, e) or None for the identity.  intake_matrix's half-pixel map on the crop (cv2.resize's
        geometry, flip = 1 for the mirror) gives level-0 coordinates X; the level coordinate is (X + 0.5) / 2^L - 0.5, composed in
        float64.  L is pick_level's for max(w / cw, h / ch) -- the axis that shrinks LEAST, so no axis is blurred more than it
        needs (the other one's residual scale can then fall below 0.5).  The roi at the level: [x0 >> L, (x0 + cw - 1) >> L],
        clipped to the level (an odd last column is dropped by mip_chain); likewise y."""
        x0, y0, cw, ch = [int(v) for v in crop]
        ih, iw = self.size[s]
        if cw < 1 or ch < 1 or x0 < 0 or y0 < 0 or x0 + cw > iw or y0 + ch > ih:
            raise ValueError('crop %r does not lie inside the %d x %d image' % (tuple(crop), iw, ih))
        M, _ = intake_matrix((ch, cw), (self.h, self.w), flip=1 if mirror else None)
        level, _ = self.pick_level(s, max(self.w / float(cw), self.h / float(ch)))
        off, lh, lw = self.table[s][level]
        k = 0.5 ** level
        a = [M[0, 0] * k, M[0, 1] * k, (M[0, 2] + x0 + 0.5) * k - 0.5, M[1, 0] * k, M[1, 1] * k, (M[1, 2] + y0 + 0.5) * k - 0.5]
        roi = [min(x0 >> level, lw - 1), min(y0 >> level, lh - 1), min((x0 + cw - 1) >> level, lw - 1), min((y0 + ch - 1) >> level, lh - 1)]
        A, D, e = (None, None, None) if color is None else color
        return make_row(off, lh, lw, roi, a, A, D, e)

    def draw_params(self, B):
        """-> rows (B, BG_ROW_WORDS) int32.  Host only: needs neither torch nor a GPU.  Per image, in this order: the next index
        of the epoch order; the crop (random_sized_crop); the mirror, random.random() < 0.5 (HorizontalFlipAug); the colour map,
        ColorAugmenter(0.5, 0.5, 0.5, hue 1.0, pca_noise 0).affine().  All of it from Python's `random`, except one draw:
        affine() draws its lighting vector np.random.normal(0, 0, 3) whatever pca_noise is -- three zeros that add nothing to e
        (mxnet's CreateAugmenter leaves LightingAug out for pca_noise = 0 and draws nothing); the draw is kept so that the
        augmenter stays one code path, and it moves np.random's stream only.  augment=False: no draw but the epoch order's."""
        rows = np.zeros((B, BG_ROW_WORDS), np.int32)
        for i in range(B):
            s = self._next_index()
            ih, iw = self.size[s]
            if self.augs is None:
                rows[i] = self.param_row(s, (0, 0, iw, ih))
                continue
            x0, y0, cw, ch, _ = random_sized_crop(ih, iw, (self.h, self.w))
            mirror = random.random() < 0.5
            rows[i] = self.param_row(s, (x0, y0, cw, ch), mirror, self.augs.affine())
        return rows

    def next_batch(self, B, out=None):
        """-> (B,3,h,w) float32 0..255 on the device (`out` when given): draw_params' rows go up in one pinned, non-blocking copy;
        yolo_bg_stats takes each resized crop's mean colour (what the contrast stage needs), yolo_bg_render samples the resident
        bank again and colours.  Runs on the current stream and does not synchronise."""
        import torch
        from . import lib as L
        lib = L.load()
        B = int(B)
        if B <= 0:
            raise ValueError('the batch size should be positive')
        dev = L.resolve_device(self.device)
        L.require_current_device(dev, 'this BackgroundBank')
        shape = (B, 3, self.h, self.w)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError('out should be a contiguous float32 tensor of shape %r on %s' % (shape, dev))
        rows = self.draw_params(B)
        state = self.__dict__.setdefault('_device_state', {})
        if state.get('device') != dev:
            state.clear()
            state.update(device=dev, bank=torch.from_numpy(self.data).to(dev), stage={}, work={})
        slot = state['stage'].get(B)
        if slot is None:
            slot = state['stage'][B] = [torch.empty(rows.size * 4, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        else:
            slot[1].synchronize()         # the previous upload has left the staging buffer (waits for that copy only)
        slot[0].numpy()[:] = rows.reshape(-1).view(np.uint8)
        up = torch.empty(rows.size * 4, dtype=torch.uint8, device=dev)
        up.copy_(slot[0], non_blocking=True)
        slot[1].record()
        work = state['work'].get(B)
        if work is None:
            nbytes = lib.yolo_bg_workspace_bytes(B, self.h, self.w)
            if nbytes <= 0:
                raise L.YoloError('bg_workspace_bytes failed with status %d' % nbytes)
            work = state['work'][B] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        bank = state['bank']
        st = L.stream_ptr()
        L.check(lib.yolo_bg_stats(L.ptr(bank), bank.numel(), L.ptr(up), L.ptr(work), B, self.h, self.w, st), 'bg_stats')
        L.check(lib.yolo_bg_render(L.ptr(bank), bank.numel(), L.ptr(up), L.ptr(work), L.ptr(out), B, self.h, self.w, st), 'bg_render')
        return out
