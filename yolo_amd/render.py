"""Synthetic training targets: the label side of RenderCar.render (car/render_car.py:52-138)
and its GPU compositing step, and RenderCar.render itself for the PNG sprite set (host geometry with PIL as in the
reference, blend on the device).  The car sprites themselves (the PNG / PASCAL3D+ image sets, render_car.py:24,49-50)
are training data that is not part of the reference repository: RenderCar takes the directory they live in.

    label row = [cls, y, x, h, w, r, class distribution...]   (render_car.py:66-67,124-133)
    cls / distribution = get_label_dist(ele, azi)             (render_car.py:410-438)
    image = clip(bg / 255 * (1 - mask) + fg * mask, 0, 1)     (render_car.py:135-137)   -> yolo_composite (HIP)

RenderCar.render_device makes the same batch with the PIXELS drawn on the device too (csrc/render.hip): the host only makes the
draws (draw_params: one row of scalars per image), a resident uint8 RGBA SpriteAtlas holds the sprites and their mip levels.
LPGenerator.add_device does the same for the licence plates (csrc/plates.hip), from a resident glyph atlas.
"""
import math
import os
import random

import numpy as np


def get_label_dist(ele, azi, classes, sigma=0.1):
    """render_car.py:410-438: great-circle angle between (ele, azi) [rad] and every class direction
    (`classes` rows = [azimuth deg, elevation deg], spec.yaml `classes`), Gaussian in that angle, normalised.
    Returns (arg-min class, float32 distribution)."""
    cl = np.asarray(classes, np.float64)
    azi_l, ele_l = np.deg2rad(cl[:, 0]), np.deg2rad(cl[:, 1])
    ang = np.arccos(np.clip(math.sin(ele) * np.sin(ele_l) + math.cos(ele) * np.cos(ele_l) * np.cos(azi - azi_l), -1, 1))
    g = np.exp(-(ang.astype(np.float32)) ** 2 / np.float32(sigma))
    return int(np.argmin(ang)), (g / g.sum()).astype(np.float32)


def paste_range(r_box_l, r_box_t, r_box_r, r_box_b, img_h, img_w):
    """render_car.py:101-108: the integer ranges [low, high) the paste offsets are drawn from, so that at least
    70 % of the rotated sprite box stays inside the image."""
    w, h = r_box_r - r_box_l, r_box_b - r_box_t
    return ((int(-r_box_l - 0.3 * w), int(img_w - r_box_l - 0.7 * w)),
            (int(-r_box_t - 0.3 * h), int(img_h - r_box_t - 0.7 * h)))


def car_label(img_cls, r_box_l, r_box_t, r_box_r, r_box_b, paste_x, paste_y, r, label_distribution, img_h, img_w):
    """render_car.py:110-133: (1, 6+ncls) label [cls, y, x, h, w (fractions of the image), r, distribution]."""
    box_y = (r_box_b + r_box_t) / 2. + paste_y
    box_x = (r_box_r + r_box_l) / 2. + paste_x
    box_h, box_w = float(r_box_b - r_box_t), float(r_box_r - r_box_l)
    head = np.asarray([img_cls, box_y / img_h, box_x / img_w, box_h / img_h, box_w / img_w, r], np.float32)
    return np.concatenate([head, np.asarray(label_distribution, np.float32).reshape(-1)])[None]


def empty_labels(batch, num_class):
    """render_car.py:80: rows of -1 = 'no object' (skipped by _loss_mask, car/YOLO.py:468)."""
    return -np.ones((batch, 1, 6 + num_class), np.float32)


def composite(bg, fg, mask, unit_bg=False):
    """render_car.py:135-137 on device: bg (B,3,H,W) float32 0..255, fg / mask 0..1 CUDA tensors -> images 0..1.
    unit_bg: bg is already 0..1 (LPGenerator.add's blend, licence_plate_render/__init__.py:163)."""
    import torch
    from . import lib as L
    bg, fg, mask = bg.contiguous(), fg.contiguous(), mask.contiguous()
    if not (bg.shape == fg.shape == mask.shape) or bg.dtype != torch.float32:
        raise ValueError('bg, fg and mask must be float32 tensors of one shape')
    out = torch.empty_like(bg)
    fn = L.load().yolo_composite_unit if unit_bg else L.load().yolo_composite
    L.check(fn(L.ptr(bg), L.ptr(fg), L.ptr(mask), L.ptr(out), bg.numel(), L.stream_ptr()), 'composite')
    return out


# ---- RenderCar (car/render_car.py:29-138, 339-408): the host side of the synthetic-target generator -------------------
# The reference builds every training batch on the host with PIL (sprite -> random resize, rotate, blur -> paste at a random
# offset) and composites on the device; so does this class: PIL + numpy here, yolo_composite (HIP) for the blend.  The sprite
# sets themselves (blender renders named ...azi<1/100 deg>_ele<1/100 deg>.png under <root>/{train,valid}/<cad>/, and the
# PASCAL3D+ crops) are training data outside the reference repository: `root` points at a directory in that layout.  The
# sequence of np.random / random draws is the reference's, so a seeded run picks the same sprites, scales, angles and offsets.
PNG_MIN_SCALE, PNG_MAX_SCALE = 0.2, 1.0                         # render_car.py:20-21
PASCAL_MIN_SCALE, PASCAL_MAX_SCALE = 0.2, 0.9                   # render_car.py:23-24


class ColorAugmenter(object):
    """The colour part of mxnet.image.CreateAugmenter(data_shape, pca_noise=0.1, brightness=0.3, contrast=0.5,
    saturation=0.5, hue=1.0) as RenderCar uses it (render_car.py:45-47), restated from mxnet/image/image.py (mxnet is
    absent here -- [recalled]): ColorJitterAug (brightness, contrast, saturation in a random order) -> HueJitterAug ->
    LightingAug; the geometric augmenters of that list are no-ops for an image that already has the data shape.  Input and
    output: (H,W,3) float32 in 0..255."""
    COEF = np.array([[[0.299, 0.587, 0.114]]], np.float32)
    TYIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.321], [0.211, -0.523, 0.311]])
    ITYIQ = np.array([[1.0, 0.956, 0.621], [1.0, -0.272, -0.647], [1.0, -1.107, 1.705]])
    EIGVAL = np.array([55.46, 4.794, 1.148])
    EIGVEC = np.array([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]])

    def __init__(self, brightness=0.3, contrast=0.5, saturation=0.5, hue=1.0, pca_noise=0.1):
        self.b, self.c, self.s, self.h, self.pca = brightness, contrast, saturation, hue, pca_noise

    def _brightness(self, src):
        return src * np.float32(1.0 + random.uniform(-self.b, self.b))

    def _contrast(self, src):
        alpha = 1.0 + random.uniform(-self.c, self.c)
        gray = (3.0 * (1.0 - alpha) / src.size) * float((src * self.COEF).sum())
        return src * np.float32(alpha) + np.float32(gray)

    def _saturation(self, src):
        alpha = 1.0 + random.uniform(-self.s, self.s)
        gray = (src * self.COEF).sum(axis=2, keepdims=True) * np.float32(1.0 - alpha)
        return src * np.float32(alpha) + gray

    def __call__(self, src):
        src = np.asarray(src, np.float32)
        ts = [self._brightness, self._contrast, self._saturation]
        random.shuffle(ts)                                        # RandomOrderAug
        for t in ts:
            src = t(src)
        alpha = random.uniform(-self.h, self.h)                   # HueJitterAug
        u, w = math.cos(alpha * math.pi), math.sin(alpha * math.pi)
        bt = np.array([[1.0, 0.0, 0.0], [0.0, u, -w], [0.0, w, u]])
        src = src @ np.dot(np.dot(self.ITYIQ, bt), self.TYIQ).T.astype(np.float32)
        a = np.random.normal(0, self.pca, size=(3,))              # LightingAug
        return (src + np.dot(self.EIGVEC * a, self.EIGVAL).astype(np.float32)).astype(np.float32)

    def affine(self):
        """The whole chain as ONE map  out = A x + D mean(x) + e  (x: a pixel, mean(x): the per-channel mean of the image the
        chain is given), float64 (A (3,3), D (3,3), e (3,)).  Every stage is affine in the pixel; only contrast looks at the
        image, through its mean.  Makes __call__'s draws, in __call__'s order, from the same `random` / `np.random` streams."""
        coef = self.COEF.reshape(3).astype(np.float64)
        gray = np.outer(np.ones(3), coef)                         # every channel <- the luma of the pixel
        st = {'A': np.eye(3), 'D': np.zeros((3, 3)), 'e': np.zeros(3)}

        def left(M):
            st['A'], st['D'], st['e'] = M @ st['A'], M @ st['D'], M @ st['e']

        def brightness():
            left(np.eye(3) * float(np.float32(1.0 + random.uniform(-self.b, self.b))))

        def contrast():
            alpha = 1.0 + random.uniform(-self.c, self.c)
            # gray = (1 - alpha) * luma of the MEAN of what this stage is given = coef . ((A + D) mean(x) + e)
            add_d, add_e = (1.0 - alpha) * gray @ (st['A'] + st['D']), (1.0 - alpha) * gray @ st['e']
            left(np.eye(3) * float(np.float32(alpha)))
            st['D'], st['e'] = st['D'] + add_d, st['e'] + add_e

        def saturation():
            alpha = 1.0 + random.uniform(-self.s, self.s)
            left(np.eye(3) * float(np.float32(alpha)) + float(np.float32(1.0 - alpha)) * gray)

        ts = [brightness, contrast, saturation]
        random.shuffle(ts)
        for t in ts:
            t()
        alpha = random.uniform(-self.h, self.h)
        u, w = math.cos(alpha * math.pi), math.sin(alpha * math.pi)
        bt = np.array([[1.0, 0.0, 0.0], [0.0, u, -w], [0.0, w, u]])
        left(np.dot(np.dot(self.ITYIQ, bt), self.TYIQ))
        a = np.random.normal(0, self.pca, size=(3,))
        st['e'] = st['e'] + np.dot(self.EIGVEC * a, self.EIGVAL)
        return st['A'], st['D'], st['e']


# ---- the device renderer's host side: sprite atlas, analytic boxes, parameter rows (csrc/render.hip) -----------------------
# render_host draws every image with PIL; render_device makes the same DECISIONS on the host (which sprite, scale, angle, blur,
# offset, colour) as a row of scalars per image and leaves the pixels to yolo_render_stats / yolo_render_cars.  One row is
# ROW_WORDS 32-bit words (include/yolo_amd.h, yolo_render_cars):
#   0 has-sprite   1 h   2 w (of the mip level)   3..6 window l, t, r, b (r, b exclusive)   8,9 the level's byte offset (int64)
#   10..15 the inverse affine a0..a5   16 w0   17 w1   18..26 A   27..35 D   36..38 e        (7, 39: padding)
ROW_WORDS = 40
MIP_MIN_SIDE = 8
BLUR_MIN_SIGMA = 0.05


def convex_hull(pts):
    """Andrew's monotone chain on an (n,2) array -> the hull's vertices (m,2) float64."""
    pts = sorted(set(map(tuple, np.asarray(pts, np.float64).tolist())))
    if len(pts) <= 2:
        return np.asarray(pts, np.float64).reshape(-1, 2)

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(p)
        return out[:-1]
    return np.asarray(half(pts) + half(pts[::-1]), np.float64)


def pixel_hull(rgba):
    """Convex hull of the CORNER points of the pixels of an (h,w,4) uint8 image that are non-zero in any band (the pixel set
    PIL's getbbox(alpha_only=False) looks at), in continuous coordinates: pixel (row i, column j) is [j, j+1] x [i, i+1].
    A sprite with no such pixel gets its whole rectangle (as _render_png does)."""
    h, w = rgba.shape[:2]
    on = (rgba != 0).any(axis=2)
    rows = np.nonzero(on.any(axis=1))[0]
    if len(rows) == 0:
        return np.float64([[0, 0], [w, 0], [w, h], [0, h]])
    first = on.argmax(axis=1)[rows]
    last = w - on[:, ::-1].argmax(axis=1)[rows]                   # exclusive
    pts = [(x, y) for xs in (first, last) for ys in (rows, rows + 1) for x, y in zip(xs.tolist(), ys.tolist())]
    return convex_hull(pts)


def mip_chain(rgba):
    """[level 0, level 1, ...]: each level the 2x2 average (rounded to nearest) of the one before, an odd last row / column
    dropped, down to the last level whose shorter side is still >= MIP_MIN_SIDE."""
    levels = [np.ascontiguousarray(rgba, np.uint8)]
    while min(levels[-1].shape[:2]) // 2 >= MIP_MIN_SIDE:
        a = levels[-1]
        h, w = a.shape[0] // 2 * 2, a.shape[1] // 2 * 2
        a = a[:h, :w].astype(np.uint16)
        levels.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return levels


class SpriteAtlas(object):
    """Every sprite as uint8 RGBA with its mip chain, packed densely ((h, w, 4) after (h, w, 4)) into ONE byte buffer
    (`data`) that is uploaded once; `table[s]` lists (byte offset, h, w) per level of sprite s, `hull[s]` is pixel_hull of
    its level 0 and `size[s]` its (h, w)."""

    def __init__(self, sprites):
        self.table, self.hull, self.size = [], [], []
        chunks, off = [], 0
        for rgba in sprites:
            rgba = np.asarray(rgba, np.uint8)
            if rgba.ndim != 3 or rgba.shape[2] != 4:
                raise ValueError('sprites should be (h, w, 4) uint8 RGBA')
            rows = []
            for lv in mip_chain(rgba):
                rows.append((off, lv.shape[0], lv.shape[1]))
                chunks.append(lv.reshape(-1))
                off += lv.size
            self.table.append(rows)
            self.hull.append(pixel_hull(rgba))
            self.size.append((rgba.shape[0], rgba.shape[1]))
        self.data = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)

    def pick_level(self, s, scale):
        """-> (level, residual scale = scale * 2**level): the level at which the residual lies in (0.5, 1], so that a plain
        bilinear tap does not skip source pixels; the coarsest level the sprite has when that one does not exist (the
        residual is then <= 0.5), level 0 for a magnification."""
        level = 0
        while scale * 2 ** level <= 0.5 and level + 1 < len(self.table[s]):
            level += 1
        return level, scale * 2 ** level


def pil_rotate_matrix(w, h, deg):
    """PIL's Image.rotate(deg, expand=1) as numbers: -> (nw, nh, M (3,3) float64) with M mapping a point of the rotated
    (nw, nh) image to the point of the (w, h) image it shows, both in continuous coordinates (pixel k spans [k, k+1])."""
    ang = -math.radians(deg % 360.0)
    m = [round(math.cos(ang), 15), round(math.sin(ang), 15), 0.0, round(-math.sin(ang), 15), round(math.cos(ang), 15), 0.0]

    def tf(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2], m[5] = tf(-w / 2., -h / 2.)
    m[2] += w / 2.
    m[5] += h / 2.
    pts = [tf(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))]
    nw = math.ceil(max(p[0] for p in pts)) - math.floor(min(p[0] for p in pts))
    nh = math.ceil(max(p[1] for p in pts)) - math.floor(min(p[1] for p in pts))
    m[2], m[5] = tf(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return nw, nh, np.array([m[:3], m[3:], [0.0, 0.0, 1.0]])


def blur_weights(sigma):
    """The 3-tap weights (w0 centre, w1 either side) of the device renderer's blur: w1 / w0 = exp(-1 / (2 sigma^2)),
    normalised to w0 + 2 w1 = 1; no blur below BLUR_MIN_SIGMA.  (A definition of its own, not PIL's box-blur GaussianBlur.)"""
    if sigma < BLUR_MIN_SIGMA:
        return 1.0, 0.0
    g = math.exp(-1.0 / (2.0 * sigma * sigma))
    return 1.0 / (1.0 + 2.0 * g), g / (1.0 + 2.0 * g)


def pascal3d_view(mat):
    """get_pascal3d_azi_ele (render_car.py:440-458) on one loaded PASCAL3D+ annotation (the dict scipy.io.loadmat returns):
    -> (elevation rad, azimuth rad, [l, t, r, b]) of the image's single car, or None when the image holds several
    (the reference skips those).  The record's fields are addressed by POSITION, as the reference does: record[1] =
    objects, object[1] = bbox, object[3] = viewpoint, viewpoint[2] / [3] = azimuth / elevation in degrees."""
    objects = mat['record'][0][0][1][0]
    if len(objects) != 1:
        return None
    view = objects[0][3][0][0]
    return (float(np.ravel(view[3])[0]) * math.pi / 180., float(np.ravel(view[2])[0]) * math.pi / 180., [int(v) for v in objects[0][1][0]])


class RenderCar(object):
    """render_car.RenderCar(img_h, img_w, classes, ctx): the PNG sprite set (`_render_png`) and, when `pascal_root` is
    given, the PASCAL3D+ crops (`_render_pascal`; <pascal_root>/car_imagenet_label/*.mat, car_imagenet_{train,valid}/,
    pre-loaded as the reference does with pre_load=True, render_car.py:221-260)."""

    def __init__(self, img_h, img_w, classes, root, device='cuda:0', augment=True, R=30.0, G=0.3, pascal_root=None):
        self.h, self.w = int(img_h), int(img_w)
        self.classes = [list(c) for c in classes]
        self.num_cls = len(classes)
        self.device = device
        self.R, self.G = R, G                                     # PILImageEnhance(M=0, N=0, R=30.0, G=0.3, noise_var=0), :43-44
        self.augs = ColorAugmenter() if augment else None
        self.rawcar_dataset = {'train': [], 'valid': []}          # load_png_images, :187-219 (os.listdir order)
        for mode in self.rawcar_dataset:
            mdir = os.path.join(root, mode)
            if not os.path.isdir(mdir):
                continue
            for cad in os.listdir(mdir):
                for img in os.listdir(os.path.join(mdir, cad)):
                    self.rawcar_dataset[mode].append(os.path.join(mdir, cad, img))
        self.pascal_dataset = {'train': [], 'valid': []}          # load_pascal_images, :221-260
        if pascal_root is not None:
            from PIL import Image
            import scipy.io as sio
            ldir = os.path.join(pascal_root, 'car_imagenet_label')
            anno = {f: sio.loadmat(os.path.join(ldir, f)) for f in os.listdir(ldir)}
            for mode in self.pascal_dataset:
                idir = os.path.join(pascal_root, 'car_imagenet_' + mode)
                for img in os.listdir(idir):
                    view = pascal3d_view(anno[img.split('.')[0] + '.mat'])
                    if view is None:
                        continue
                    cls, dist = get_label_dist(view[0], view[1], self.classes)
                    self.pascal_dataset[mode].append((Image.open(os.path.join(idir, img)).convert('RGBA'), view[2], cls, dist))

    def _resize(self, pil_img, min_scale, max_scale, r1):
        """render_car.py:370-392."""
        from PIL import Image
        resize = np.random.uniform(low=min_scale, high=max_scale)
        resize_w = resize * pil_img.size[0]
        resize_h = resize * pil_img.size[1] * r1
        return resize, resize_w, resize_h, pil_img.resize((int(resize_w), int(resize_h)), Image.BILINEAR)

    def _enhance(self, img):
        """yolo_cv.PILImageEnhance.__call__ with M = N = 0, noise_var = 0 (yolo_cv.py:105-157): random_rotate, random_blur."""
        from PIL import Image, ImageFilter
        r = 0
        if self.R != 0:
            rd = np.random.uniform(low=-self.R, high=self.R)
            img = img.rotate(rd, Image.BILINEAR, expand=1)
            r = float(rd * np.pi) / 180
        if self.G != 0:
            img = img.filter(ImageFilter.GaussianBlur(radius=np.random.rand() * self.G))
        return img, r

    def _render_png(self, mode, r1=1.0):
        """render_car.py:339-368: one sprite -> (RGBA image, its bounding box after the rotation, r, class, distribution)."""
        from PIL import Image
        n = np.random.randint(len(self.rawcar_dataset[mode]))
        img_path = self.rawcar_dataset[mode][n]
        img = img_path.split('/')[-1]
        ele = float(img.split('ele')[1].split('.')[0]) * math.pi / 18000.
        azi = float(img.split('azi')[1].split('_')[0]) * math.pi / 18000.
        img_cls, label_distribution = get_label_dist(ele, azi, self.classes)
        pil_img = Image.open(img_path).convert('RGBA')
        _, _, _, pil_img = self._resize(pil_img, PNG_MIN_SCALE, PNG_MAX_SCALE, r1)
        pil_img, r = self._enhance(pil_img)
        # the box of pixels that are non-zero in ANY band, as the PIL of the reference's day computed it (Pillow >= 10 looks
        # at the alpha band only by default; bilinear rotation leaves colour in a rim of fully transparent pixels, so the
        # two differ by a pixel or two -- found by the oracle comparison, tests/test_render.py)
        try:
            box = pil_img.getbbox(alpha_only=False)
        except TypeError:
            box = pil_img.getbbox()
        if box is None:                                           # (a fully transparent sprite: the reference would fail here)
            box = (0, 0, pil_img.size[0], pil_img.size[1])
        return (pil_img,) + tuple(box) + (r, img_cls, label_distribution)

    def _render_pascal(self, mode, r1=1.0):
        """render_car.py:262-337: a PASCAL3D+ crop scaled so that its annotated car box spans 20-90 % of the image; the box
        itself -- not the alpha channel: the crops are opaque photographs -- is carried through the resize and the
        (zero-degree, see below) rotation to give the label box."""
        from PIL import Image, ImageFilter
        data = self.pascal_dataset[mode]
        sprite, box, img_cls, dist = data[np.random.randint(len(data))]
        box = np.asarray(box, np.float64)                         # l, t, r, b
        span_w, span_h = box[2] - box[0], (box[3] - box[1]) * r1
        hi = min(PASCAL_MAX_SCALE * self.w / span_w, PASCAL_MAX_SCALE * self.h / span_h)
        lo = max(PASCAL_MIN_SCALE * self.w / span_w, PASCAL_MIN_SCALE * self.h / span_h)
        scale, new_w, new_h, sprite = self._resize(sprite, lo, hi, r1)
        # pil_image_enhance(pil_img, R=0) (:306): the enhancer was built with R = 30, so its rotation step still runs, with
        # the call's R = 0: ONE uniform(-0, 0) draw and a rotation by 0 degrees; then the blur
        deg = np.random.uniform(low=-0.0, high=0.0)
        sprite = sprite.rotate(deg, Image.BILINEAR, expand=1)
        r = float(deg * np.pi) / 180
        if self.G != 0:
            sprite = sprite.filter(ImageFilter.GaussianBlur(radius=np.random.rand() * self.G))
        # box corners relative to the image centre -> rotated by r -> relative to the corner of the expanded canvas
        cx = box[[0, 2]] * scale - 0.5 * new_w
        cy = box[[1, 3]] * scale * r1 - 0.5 * new_h
        gx, gy = np.meshgrid(cx, cy, indexing='ij')
        rx, ry = gx * math.cos(r) - gy * math.sin(r), gy * math.cos(r) + gx * math.sin(r)
        half_w = 0.5 * (abs(new_h * math.sin(r)) + abs(new_w * math.cos(r)))
        half_h = 0.5 * (abs(new_h * math.cos(r)) + abs(new_w * math.sin(r)))
        return (sprite, rx.min() + half_w, ry.min() + half_h, rx.max() + half_w, ry.max() + half_h, r, img_cls, dist)

    def render_host(self, batch, mode, pascal_rate=0.0, render_rate=1.0):
        """The host half of render(): (fg (B,3,H,W) float32 0..1, mask (B,3,H,W) float32 0..1, labels (B,1,6+ncls))."""
        from PIL import Image
        if pascal_rate != 0.0 and not self.pascal_dataset[mode]:
            raise ValueError('pascal_rate > 0 needs the PASCAL3D+ crops: RenderCar(..., pascal_root=...)')
        fg = np.zeros((batch, 3, self.h, self.w), np.float32)
        mask = np.zeros((batch, 3, self.h, self.w), np.float32)
        labels = empty_labels(batch, self.num_cls)
        for i in range(batch):
            if np.random.rand() > render_rate:
                continue
            r1 = np.random.uniform(low=0.9, high=1.1)
            if np.random.rand() < pascal_rate:                    # (:88; the draw is made whatever the rate)
                pil_img, l, t, r_, b, r, img_cls, dist = self._render_pascal(mode, r1)
            else:
                pil_img, l, t, r_, b, r, img_cls, dist = self._render_png(mode, r1)
            (xlo, xhi), (ylo, yhi) = paste_range(l, t, r_, b, self.h, self.w)
            paste_x = np.random.randint(low=xlo, high=xhi)
            paste_y = np.random.randint(low=ylo, high=yhi)
            tmp = Image.new('RGBA', (self.w, self.h))
            tmp.paste(pil_img, (paste_x, paste_y))
            rgb = np.asarray(Image.merge('RGB', tmp.split()[:3]), np.float32)          # pil_rgb_2_rgb_ndarray, yolo_gluon.py:303-313
            if self.augs is not None:
                rgb = self.augs(rgb)
            fg[i] = rgb.transpose(2, 0, 1) / np.float32(255.)
            m = np.asarray(tmp.split()[-1], np.float32) / np.float32(255.)              # pil_mask_2_rgb_ndarray, :298-300
            mask[i] = np.broadcast_to(m, (3, self.h, self.w))
            labels[i] = car_label(img_cls, l, t, r_, b, paste_x, paste_y, r, dist, self.h, self.w)
        return fg, mask, labels

    def render(self, bg, mode, pascal_rate=0.0, render_rate=1.0):
        """render_car.py:52-138: bg (B,3,H,W) float32 0..255 CUDA tensor -> (images 0..1 on the device, labels on the
        device); the blend clip(bg/255*(1-mask) + fg*mask, 0, 1) runs in yolo_composite."""
        import torch
        fg, mask, labels = self.render_host(len(bg), mode, pascal_rate, render_rate)
        dev = bg.device
        img = composite(bg, torch.from_numpy(fg).to(dev), torch.from_numpy(mask).to(dev))
        return img, torch.from_numpy(labels).to(dev)

    # ---- the same batch drawn on the device (csrc/render.hip): decisions here, pixels there ----------------------------
    def atlas(self):
        """The SpriteAtlas of this object's sprites, built on first use: the PNG set (opened once, here) and the PASCAL3D+
        crops; `_sprite_of[(kind, mode)][n]` is the atlas index of the n-th sprite of that list, `_png_view` its class and
        class distribution (from the file name, as _render_png reads them on every draw)."""
        if getattr(self, '_atlas', None) is None:
            from PIL import Image
            sprites, self._sprite_of, self._png_view = [], {}, {}
            for mode, paths in self.rawcar_dataset.items():
                self._sprite_of[('png', mode)] = list(range(len(sprites), len(sprites) + len(paths)))
                self._png_view[mode] = []
                for path in paths:
                    img = path.split('/')[-1]
                    ele = float(img.split('ele')[1].split('.')[0]) * math.pi / 18000.
                    azi = float(img.split('azi')[1].split('_')[0]) * math.pi / 18000.
                    self._png_view[mode].append(get_label_dist(ele, azi, self.classes))
                    sprites.append(np.asarray(Image.open(path).convert('RGBA')))
            for mode, data in self.pascal_dataset.items():
                self._sprite_of[('pascal', mode)] = list(range(len(sprites), len(sprites) + len(data)))
                sprites.extend(np.asarray(d[0]) for d in data)
            self._atlas = SpriteAtlas(sprites)
        return self._atlas

    def _draw_png(self, mode, r1):
        """_render_png's draws and its label box WITHOUT the pixels: the box is the bound of the sprite's pixel hull under
        PIL's resize (to the integer size PIL resizes to) and rotate(expand=1) geometry.
        -> (sprite, scale, map from the rotated image to level 0 (3,3), l, t, r, b, r, class, distribution, sigma); scale is
        the SMALLER of the two axes' real scales (integer resized size over sprite size: the r1 aspect factor and int() move
        them off the drawn number), which is what the mip level is picked from."""
        atlas = self.atlas()
        n = np.random.randint(len(self.rawcar_dataset[mode]))
        s = self._sprite_of[('png', mode)][n]
        img_cls, dist = self._png_view[mode][n]
        h0, w0 = atlas.size[s]
        resize = np.random.uniform(low=PNG_MIN_SCALE, high=PNG_MAX_SCALE)
        rw, rh = int(resize * w0), int(resize * h0 * r1)
        deg, r = 0.0, 0
        if self.R != 0:
            deg = np.random.uniform(low=-self.R, high=self.R)
            r = float(deg * np.pi) / 180
        sigma = np.random.rand() * self.G if self.G != 0 else 0.0
        if rw <= 0 or rh <= 0:
            raise ValueError('a %d x %d sprite at scale %g has no pixels' % (w0, h0, resize))
        _, _, rot = pil_rotate_matrix(rw, rh, deg)
        to_sprite = np.diag([w0 / float(rw), h0 / float(rh), 1.0]) @ rot
        fwd = np.linalg.inv(to_sprite)
        hull = atlas.hull[s]
        px, py = fwd[0, 0] * hull[:, 0] + fwd[0, 1] * hull[:, 1] + fwd[0, 2], fwd[1, 0] * hull[:, 0] + fwd[1, 1] * hull[:, 1] + fwd[1, 2]
        return s, min(rw / float(w0), rh / float(h0)), to_sprite, px.min(), py.min(), px.max(), py.max(), r, img_cls, dist, sigma

    def _draw_pascal(self, mode, r1):
        """_render_pascal's draws and its label box (the annotated box through the same arithmetic) without the pixels."""
        atlas = self.atlas()
        data = self.pascal_dataset[mode]
        n = np.random.randint(len(data))
        _, box, img_cls, dist = data[n]
        s = self._sprite_of[('pascal', mode)][n]
        h0, w0 = atlas.size[s]
        box = np.asarray(box, np.float64)
        span_w, span_h = box[2] - box[0], (box[3] - box[1]) * r1
        hi = min(PASCAL_MAX_SCALE * self.w / span_w, PASCAL_MAX_SCALE * self.h / span_h)
        lo = max(PASCAL_MIN_SCALE * self.w / span_w, PASCAL_MIN_SCALE * self.h / span_h)
        scale = np.random.uniform(low=lo, high=hi)
        new_w, new_h = scale * w0, scale * h0 * r1
        rw, rh = int(new_w), int(new_h)
        deg = np.random.uniform(low=-0.0, high=0.0)
        r = float(deg * np.pi) / 180
        sigma = np.random.rand() * self.G if self.G != 0 else 0.0
        if rw <= 0 or rh <= 0:
            raise ValueError('a %d x %d crop at scale %g has no pixels' % (w0, h0, scale))
        _, _, rot = pil_rotate_matrix(rw, rh, deg)
        to_sprite = np.diag([w0 / float(rw), h0 / float(rh), 1.0]) @ rot
        cx = box[[0, 2]] * scale - 0.5 * new_w
        cy = box[[1, 3]] * scale * r1 - 0.5 * new_h
        gx, gy = np.meshgrid(cx, cy, indexing='ij')
        rx, ry = gx * math.cos(r) - gy * math.sin(r), gy * math.cos(r) + gx * math.sin(r)
        half_w = 0.5 * (abs(new_h * math.sin(r)) + abs(new_w * math.cos(r)))
        half_h = 0.5 * (abs(new_h * math.cos(r)) + abs(new_w * math.sin(r)))
        return (s, min(rw / float(w0), rh / float(h0)), to_sprite, rx.min() + half_w, ry.min() + half_h, rx.max() + half_w,
                ry.max() + half_h, r, img_cls, dist, sigma)

    def param_row(self, s, scale, to_sprite, paste_x, paste_y, sigma, color=None):
        """One parameter row (ROW_WORDS int32 words, floats stored by bit pattern) for sprite s of the atlas drawn at
        `scale` (the smaller axis scale: the other axis' residual can then pass 1 by the aspect factor, a slight magnification) with `to_sprite` (3,3) mapping the resized + rotated image to level 0 (continuous coordinates), pasted at the
        integer offset (paste_x, paste_y); color = (A, D, e) or None for the identity.  The inverse affine takes an output
        pixel INDEX (column j, row i) to a level pixel INDEX: half-pixel centres on both sides, composed in float64."""
        atlas = self.atlas()
        level, _ = atlas.pick_level(s, scale)
        off, lh, lw = atlas.table[s][level]
        paste = np.array([[1.0, 0.0, -float(paste_x)], [0.0, 1.0, -float(paste_y)], [0.0, 0.0, 1.0]])
        cont = np.diag([0.5 ** level, 0.5 ** level, 1.0]) @ to_sprite @ paste          # canvas -> level, continuous
        half = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
        M = np.linalg.inv(half) @ cont @ half
        # the window: a sample is non-zero only where its level coordinate lies within half a pixel of the level's rectangle
        fwd = np.linalg.inv(cont)
        cx, cy = np.float64([-0.5, lw + 0.5, lw + 0.5, -0.5]), np.float64([-0.5, -0.5, lh + 0.5, lh + 0.5])
        wx, wy = fwd[0, 0] * cx + fwd[0, 1] * cy + fwd[0, 2], fwd[1, 0] * cx + fwd[1, 1] * cy + fwd[1, 2]
        slack = 1.01                                              # 1 px for the blur, 0.01 for the float32 matrix
        win = [int(math.floor(wx.min() - 0.5 - slack)), int(math.floor(wy.min() - 0.5 - slack)),
               int(math.ceil(wx.max() - 0.5 + slack)) + 1, int(math.ceil(wy.max() - 0.5 + slack)) + 1]
        win = [min(max(win[0], 0), self.w), min(max(win[1], 0), self.h), min(max(win[2], 0), self.w), min(max(win[3], 0), self.h)]
        row = np.zeros(ROW_WORDS, np.int32)
        fl = row.view(np.float32)
        row[0], row[1], row[2] = 1, lh, lw
        row[3:7] = win
        row[8:10] = np.array([off], np.int64).view(np.int32)
        fl[10:16] = M[:2].reshape(-1).astype(np.float32)
        fl[16:18] = np.float64(blur_weights(sigma)).astype(np.float32)
        A, D, e = (np.eye(3), np.zeros((3, 3)), np.zeros(3)) if color is None else color
        fl[18:27], fl[27:36], fl[36:39] = (np.asarray(A, np.float64).reshape(-1).astype(np.float32),
                                           np.asarray(D, np.float64).reshape(-1).astype(np.float32), np.asarray(e, np.float64).astype(np.float32))
        return row

    def draw_params(self, batch, mode, pascal_rate=0.0, render_rate=1.0):
        """render_host's draws, in its order and from the same np.random / random streams, without touching a pixel:
        -> (labels (B,1,6+ncls) float32, rows (B, ROW_WORDS) int32).  Host only: needs neither torch nor a GPU.
        Same seed, same decisions -- image by image, up to the paste offsets: their ranges come from the analytic box, a pixel
        or two tighter than PIL's, and np.random.randint draws by rejection, so the number of raw values a paste draw takes
        can differ between the two routes; from the first image where it does, a batch's streams have parted."""
        if pascal_rate != 0.0 and not self.pascal_dataset[mode]:
            raise ValueError('pascal_rate > 0 needs the PASCAL3D+ crops: RenderCar(..., pascal_root=...)')
        labels = empty_labels(batch, self.num_cls)
        rows = np.zeros((batch, ROW_WORDS), np.int32)
        for i in range(batch):
            if np.random.rand() > render_rate:
                continue
            r1 = np.random.uniform(low=0.9, high=1.1)
            draw = self._draw_pascal if np.random.rand() < pascal_rate else self._draw_png
            s, scale, to_sprite, l, t, r_, b, r, img_cls, dist, sigma = draw(mode, r1)
            (xlo, xhi), (ylo, yhi) = paste_range(l, t, r_, b, self.h, self.w)
            paste_x = np.random.randint(low=xlo, high=xhi)
            paste_y = np.random.randint(low=ylo, high=yhi)
            color = self.augs.affine() if self.augs is not None else None
            rows[i] = self.param_row(s, scale, to_sprite, paste_x, paste_y, sigma, color)
            labels[i] = car_label(img_cls, l, t, r_, b, paste_x, paste_y, r, dist, self.h, self.w)
        return labels, rows

    def render_device(self, bg, mode, pascal_rate=0.0, render_rate=1.0, out=None):
        """render() with the pixels made on the device: bg (B,3,H,W) float32 0..255 CUDA tensor -> (images 0..1, labels), both
        on the device.  The host draws the parameter rows (draw_params); rows and labels go up in ONE pinned, non-blocking
        copy; yolo_render_stats takes each canvas's mean colour (what the contrast stage needs), yolo_render_cars samples the
        resident atlas, colours and blends.  Runs on the current stream and does not synchronise."""
        import torch
        from . import lib as L
        lib = L.load()
        B = len(bg)
        if tuple(bg.shape) != (B, 3, self.h, self.w) or bg.dtype != torch.float32 or not bg.is_cuda:
            raise ValueError('bg should be a float32 CUDA tensor of shape (B, 3, %d, %d)' % (self.h, self.w))
        dev = bg.device
        L.require_current_device(dev, 'this render_device call')
        bg = bg.contiguous()
        if out is None:
            out = torch.empty_like(bg)
        elif tuple(out.shape) != tuple(bg.shape) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError('out should be a contiguous float32 tensor of shape %r on %s' % (tuple(bg.shape), dev))
        labels, rows = self.draw_params(B, mode, pascal_rate, render_rate)
        state = self.__dict__.setdefault('_device_state', {})
        if state.get('device') != dev:
            state.clear()
            state.update(device=dev, atlas=torch.from_numpy(self.atlas().data).to(dev), stage={}, work={})
        nrow, nlab = rows.size * 4, labels.size * 4
        slot = state['stage'].get(B)
        if slot is None:
            slot = state['stage'][B] = [torch.empty(nrow + nlab, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        else:
            slot[1].synchronize()         # the previous upload has left the staging buffer (waits for that copy only)
        host = slot[0].numpy()
        host[:nrow] = rows.reshape(-1).view(np.uint8)
        host[nrow:] = labels.reshape(-1).view(np.uint8)
        up = torch.empty(nrow + nlab, dtype=torch.uint8, device=dev)
        up.copy_(slot[0], non_blocking=True)
        slot[1].record()
        work = state['work'].get(B)
        if work is None:
            nbytes = lib.yolo_render_workspace_bytes(B, self.h, self.w)
            if nbytes <= 0:
                raise L.YoloError('render_workspace_bytes failed with status %d' % nbytes)
            work = state['work'][B] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        atlas = state['atlas']
        L.check(lib.yolo_render_stats(L.ptr(atlas), atlas.numel(), L.ptr(up), L.ptr(work), B, self.h, self.w, L.stream_ptr()), 'render_stats')
        L.check(lib.yolo_render_cars(L.ptr(bg), L.ptr(atlas), atlas.numel(), L.ptr(up), L.ptr(work), L.ptr(out), B, self.h, self.w,
                                     L.stream_ptr()), 'render_cars')
        return out, up[nrow:].view(torch.float32).view(B, 1, 6 + self.num_cls)


# ---- LPGenerator.add (yolo_modules/licence_plate_render/__init__.py:21-166, 273-371): licence plates for CarLPNet ---------
LP_CORNERS = np.float32([[380, 160], [0, 160], [0, 0], [380, 0]])       # (:118: the plate image's corners, as projected)
LP_GLYPH_X = (7, 56, 106, 158, 175, 225, 274, 324)                      # (:28: glyph columns of the 'ABC-1234' plate)
# the device route (csrc/plates.hip; include/yolo_amd.h, yolo_plate_render): one row of PLATE_ROW_WORDS 32-bit words per image
#   0 has-plate   1..7 glyph ids   8..11 window l, t, r, b   12,13 noise key   14 noise scale   16..24 the projective map m0..m8
#   25 w0   26 w1   27..35 A   36..44 D   45..47 e                                                         (15: padding)
PLATE_ROW_WORDS = 48
PLATE_GLYPH_BYTES = 34 * 90 * 45 * 4 + 70 * 10 * 4
# the noise is sigma times an 8-term Irwin-Hall sum of bytes: its standard deviation before scaling (a byte's variance is 65535/12)
PLATE_NOISE_UNIT = math.sqrt(8 * 65535 / 12.0)


# the OCR batch (csrc/ocr_data.hip; include/yolo_amd.h, yolo_ocr_plate_blur): per image one plate row whose map is affine, and one
# row of OCR_TAP_WORDS words for the blur: word 0 T (taps per side, 0..OCR_BLUR_TAPS), words 1..T+1 the float32 weights w[0..T]
OCR_TAP_WORDS = 32
OCR_BLUR_TAPS = 24
# LPGenerator.render's arguments: the reference's call (:181-189) for scale, aspect, R and G; noise is PILImageEnhance's own
# default (:47-48; the call passes no noise_var); M and N are 0.1 where the call passes 10.0 (see LPGenerator.render)
OCR_RENDER_DEFAULTS = dict(scale=(0.9, 1.0), aspect=(0.9, 1.1), R=5.0, G=8.0, noise=10.0, M=0.1, N=0.1)


def gaussian_taps(sigma):
    """The tap row of the OCR renderer's blur: a true Gaussian w[k] = exp(-k^2 / (2 sigma^2)), k = 0..T, truncated at
    T = min(ceil(3 sigma), OCR_BLUR_TAPS) and normalised (in float64) to w[0] + 2 sum w[1..T] = 1; below BLUR_MIN_SIGMA T = 0 and
    w[0] = 1: no blur.  -> OCR_TAP_WORDS int32 words, the weights stored by bit pattern."""
    row = np.zeros(OCR_TAP_WORDS, np.int32)
    fl = row.view(np.float32)
    if sigma < BLUR_MIN_SIGMA:
        fl[1] = 1.0
        return row
    T = min(int(math.ceil(3.0 * sigma)), OCR_BLUR_TAPS)
    k = np.arange(T + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * sigma * sigma))
    row[0] = T
    fl[1:T + 2] = (g / (g[0] + 2.0 * g[1:].sum())).astype(np.float32)
    return row


def homography(src, dst):
    """cv2.getPerspectiveTransform(src, dst) (cv2 is absent here): the projective map through four point pairs, as the
    3x3 matrix normalised to M[2, 2] = 1 -- the eight unknowns of  u = (a x + b y + c) / (g x + h y + 1),
    v = (d x + e y + f) / (g x + h y + 1)  from the eight linear equations the pairs give."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    x, y, u, v = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    one, zero = np.ones(4), np.zeros(4)
    A = np.concatenate([np.stack([x, y, one, zero, zero, zero, -x * u, -y * u], axis=1),
                        np.stack([zero, zero, zero, x, y, one, -x * v, -y * v], axis=1)])
    return np.append(np.linalg.solve(A, np.concatenate([u, v])), 1.0).reshape(3, 3)


class PlateCamera(object):
    """ProjectRectangle6D (:273-371): the pinhole camera the plates are projected through.  `camera`: the calibration
    the reference reads from its camera yaml -- image_width, image_height, projection_matrix.data (row-major 3x4)."""
    HALF_W, HALF_H = 199.5, 84.0                                  # (the reference's constants, mm)

    def __init__(self, camera):
        self.w, self.h = int(camera['image_width']), int(camera['image_height'])
        P = camera['projection_matrix']['data']
        self.fx, self.fy, self.cx, self.cy = float(P[0]), float(P[5]), float(P[2]), float(P[6])

    def corners(self, pose):
        """Pixel positions of the plate's corners (bottom-right, bottom-left, top-left, top-right as the reference orders
        them) for pose [X, Y, Z mm, r1, r2, r3 rad]: K (R3 R2 R1 P + T) in closed form (:337-363)."""
        X, Y, Z, r1, r2, r3 = [float(v) for v in pose]
        Rx = np.array([[1, 0, 0], [0, math.cos(r1), -math.sin(r1)], [0, math.sin(r1), math.cos(r1)]])
        Ry = np.array([[math.cos(r2), 0, math.sin(r2)], [0, 1, 0], [-math.sin(r2), 0, math.cos(r2)]])
        Rz = np.array([[math.cos(r3), -math.sin(r3), 0], [math.sin(r3), math.cos(r3), 0], [0, 0, 1]])
        P = np.array([[self.HALF_W, -self.HALF_W, -self.HALF_W, self.HALF_W], [self.HALF_H, self.HALF_H, -self.HALF_H, -self.HALF_H],
                      [0.0, 0.0, 0.0, 0.0]])
        cam = Rz @ Ry @ Rx @ P + np.array([[X], [Y], [Z]])
        K = np.array([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1]])
        pix = K @ cam
        return (pix[:2] / pix[2]).T.astype(np.float32)

    def centre(self, X, Y, Z, out_h, out_w):
        """(:126-130) the plate centre in pixels of the (out_h, out_w) training image."""
        return ((X * self.fx / Z + self.cx) * out_w / float(self.w), (Y * self.fy / Z + self.cy) * out_h / float(self.h))


class LPGenerator(object):
    """LPGenerator(img_h, img_w) (:21-56) for `add` (:134-166): draws an 'ABC-1234' plate from glyph images, projects it
    with a random 6-D pose through the camera, blurs / noises it and pastes it onto a batch of 0..1 images on the device.
    `fonts_dir` holds the glyphs 0.png .. 33.png (digits, then letters) and the dot 34.png as the reference's
    licence_plate_render/fonts does -- data that stays with the reference; `camera`: see PlateCamera."""

    def __init__(self, img_h, img_w, fonts_dir, camera, augment=True):
        from PIL import Image
        self.h, self.w = int(img_h), int(img_w)
        self.camera = PlateCamera(camera)
        self.glyph = [Image.open(os.path.join(fonts_dir, '%d.png' % k)).resize((45, 90), Image.BILINEAR) for k in range(34)]
        self.dot = Image.open(os.path.join(fonts_dir, '34.png')).resize((10, 70), Image.BILINEAR)
        # (:52-55: augs2 = CreateAugmenter(pca_noise=0.1, brightness=0.7, contrast=0.7, saturation=0.7, hue=1.0))
        self.augs = ColorAugmenter(brightness=0.7, contrast=0.7, saturation=0.7, hue=1.0, pca_noise=0.1) if augment else None
        # (:50-53: augs = CreateAugmenter(pca_noise=1.0, brightness=0.5, contrast=0.5, saturation=0.3, hue=1.0), render's)
        self.ocr_augs = ColorAugmenter(brightness=0.5, contrast=0.5, saturation=0.3, hue=1.0, pca_noise=1.0) if augment else None

    def draw_LP(self):
        """(:58-77) -> (RGBA plate 380 x 160 on white, type 0, [[glyph id, left, right (fractions of the width)] x 7])."""
        from PIL import Image
        plate = Image.new('RGBA', (380, 160), (255, 255, 255))
        letters = np.random.randint(10, 34, size=3)
        ids = list(letters)
        for k, g in enumerate(letters):
            plate.paste(self.glyph[g], (LP_GLYPH_X[k], 35))
        plate.paste(self.dot, (LP_GLYPH_X[3], 45))
        digits = np.random.randint(0, 9, size=4)
        for k, g in enumerate(digits):
            g = 9 if g == 4 else g                                # (no digit four on a plate)
            ids.append(g)
            plate.paste(self.glyph[g], (LP_GLYPH_X[k + 4], 35))
        cols = LP_GLYPH_X[:3] + LP_GLYPH_X[4:]
        return plate, 0, [[int(g), c / 380., (c + 45) / 380.] for g, c in zip(ids, cols)]

    def random_projection_LP_6D(self, plate, out_size, r_max):
        """(:98-132) -> (mask (3,H,W), image (3,H,W) float32 0..1, label [1, X, Y, Z, r1, r2, r3, x_px, y_px])."""
        from PIL import Image, ImageFilter
        Z = np.random.uniform(low=1500., high=5000.)
        X = (Z * 9 / 30.) * np.random.uniform(low=-1, high=1)
        Y = (Z * 7 / 30.) * np.random.uniform(low=-1, high=1)
        rot = [np.random.uniform(low=-1, high=1) * r_max[k] * math.pi / 180. for k in range(3)]
        M = homography(self.camera.corners([X, Y, Z] + rot), LP_CORNERS)
        plate = plate.transform((self.camera.w, self.camera.h), Image.PERSPECTIVE, tuple(M.reshape(-1)[:8]), Image.BILINEAR)
        plate = plate.resize((out_size[1], out_size[0]), Image.BILINEAR)
        # pil_image_enhance(LP, G=1.0, noise_var=5.0) of PILImageEnhance(M=0, N=0, R=0, G=1.0, noise_var=10.): blur, noise
        plate = plate.filter(ImageFilter.GaussianBlur(radius=np.random.rand() * 1.0))
        px = np.array(plate)
        plate = Image.fromarray(np.uint8(np.clip(px + np.random.normal(0., 5.0, px.shape), 0, 255)))
        bands = plate.split()
        rgb = np.asarray(Image.merge('RGB', bands[:3]), np.float32)
        if self.augs is not None:
            rgb = self.augs(rgb)
        alpha = np.asarray(bands[-1], np.float32) / np.float32(255.)
        x, y = self.camera.centre(X, Y, Z, out_size[0], out_size[1])
        label = np.asarray([1, X, Y, Z, rot[0], rot[1], rot[2], x, y], np.float32)
        return np.broadcast_to(alpha, (3,) + alpha.shape), rgb.transpose(2, 0, 1) / np.float32(255.), label

    def add_host(self, batch, h, w, r_max, add_rate=1.0):
        """The host half of add(): (fg, mask (B,3,h,w) float32, labels (B,1,10) [1, X, Y, Z, r1, r2, r3, x, y, type]; -1: none)."""
        fg = np.zeros((batch, 3, h, w), np.float32)
        mask = np.zeros((batch, 3, h, w), np.float32)
        labels = -np.ones((batch, 1, 10), np.float32)
        for i in range(batch):
            if np.random.rand() > add_rate:
                continue
            plate, lp_type, _ = self.draw_LP()
            mask[i], fg[i], labels[i, 0, :9] = self.random_projection_LP_6D(plate, (h, w), r_max)
            labels[i, 0, 9] = lp_type
        return fg, mask, labels

    # ---- the same plates drawn on the device (csrc/plates.hip): decisions here, pixels there ----------------------------------
    def glyph_atlas(self):
        """The glyph images as the device holds them: uint8 RGBA bytes, the 34 glyphs as (90,45,4) in id order, then the dot
        as (70,10,4) -- PLATE_GLYPH_BYTES in all (include/yolo_amd.h, yolo_plate_compose).  Built once."""
        if getattr(self, '_glyph_atlas', None) is None:
            parts = [np.asarray(g if g.mode == 'RGBA' else g.convert('RGBA'), np.uint8).reshape(-1) for g in self.glyph + [self.dot]]
            data = np.ascontiguousarray(np.concatenate(parts))
            if data.size != PLATE_GLYPH_BYTES:
                raise ValueError('the glyph atlas has %d bytes, not %d' % (data.size, PLATE_GLYPH_BYTES))
            self._glyph_atlas = data
        return self._glyph_atlas

    def plate_row(self, ids, pose, h, w, sigma_blur, key, sigma_noise=5.0, color=None):
        """One parameter row (PLATE_ROW_WORDS int32 words, floats stored by bit pattern) of a plate with the 7 glyph `ids`
        at `pose` [X, Y, Z, r1, r2, r3] on an (h, w) canvas; key = (k0, k1); color = (A, D, e) or None for the identity.
        The map takes a canvas pixel INDEX to a plate texel INDEX: index -> continuous (+0.5) -> camera pixel (the canvas is the
        camera image resized) -> the plate through homography(corners(pose), LP_CORNERS) -> index (-0.5); composed in
        float64, stored as float32, not normalised."""
        cam = self.camera
        half = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
        to_cam = np.diag([cam.w / float(w), cam.h / float(h), 1.0])
        M = np.linalg.inv(half) @ homography(cam.corners(pose), LP_CORNERS) @ to_cam @ half
        # the window: a sample is non-zero only for texel indices in (-1, 380) x (-1, 160); that rectangle carried to the canvas
        F = np.linalg.inv(M)
        tx, ty = np.float64([-1, 380, 380, -1]), np.float64([-1, -1, 160, 160])
        den = F[2, 0] * tx + F[2, 1] * ty + F[2, 2]
        if (den * den[0] <= 0).any():                             # (the rectangle crosses the map's horizon: no bound to take)
            win = [0, 0, w, h]
        else:
            px, py = (F[0, 0] * tx + F[0, 1] * ty + F[0, 2]) / den, (F[1, 0] * tx + F[1, 1] * ty + F[1, 2]) / den
            slack = 1.01                                          # 1 px for the blur, 0.01 for the float32 matrix
            win = [int(math.floor(px.min() - slack)), int(math.floor(py.min() - slack)),
                   int(math.ceil(px.max() + slack)) + 1, int(math.ceil(py.max() + slack)) + 1]
            win = [min(max(win[0], 0), w), min(max(win[1], 0), h), min(max(win[2], 0), w), min(max(win[3], 0), h)]
        row = np.zeros(PLATE_ROW_WORDS, np.int32)
        fl = row.view(np.float32)
        row[0] = 1
        row[1:8] = ids
        row[8:12] = win
        row[12:14] = np.asarray(key, np.uint32).view(np.int32)
        fl[14] = np.float32(sigma_noise / PLATE_NOISE_UNIT)
        fl[16:25] = M.reshape(-1).astype(np.float32)
        fl[25:27] = np.float64(blur_weights(sigma_blur)).astype(np.float32)
        A, D, e = (np.eye(3), np.zeros((3, 3)), np.zeros(3)) if color is None else color
        fl[27:36], fl[36:45], fl[45:48] = (np.asarray(A, np.float64).reshape(-1).astype(np.float32),
                                           np.asarray(D, np.float64).reshape(-1).astype(np.float32), np.asarray(e, np.float64).astype(np.float32))
        return row

    def draw_params(self, batch, h, w, r_max, add_rate=1.0):
        """add_host's draws, in its order and from the same np.random / random streams, without touching a pixel:
        -> (labels (B,1,10) float32, rows (B, PLATE_ROW_WORDS) int32).  Host only: needs neither torch nor a GPU.
        Per image: the add-rate draw, three letters, four digits (4 -> 9), Z, X, Y, three angles, the blur radius; then TWO
        uint32 key words (np.random.randint) where the host route draws h*w*4 normals; then the colour augmenter's draws.
        So the first plate of a batch has add_host's glyphs, pose and label; after it the two routes' streams have parted."""
        labels = -np.ones((batch, 1, 10), np.float32)
        rows = np.zeros((batch, PLATE_ROW_WORDS), np.int32)
        for i in range(batch):
            if np.random.rand() > add_rate:
                continue
            ids = [int(g) for g in np.random.randint(10, 34, size=3)]
            ids += [9 if g == 4 else int(g) for g in np.random.randint(0, 9, size=4)]
            Z = np.random.uniform(low=1500., high=5000.)
            X = (Z * 9 / 30.) * np.random.uniform(low=-1, high=1)
            Y = (Z * 7 / 30.) * np.random.uniform(low=-1, high=1)
            rot = [np.random.uniform(low=-1, high=1) * r_max[k] * math.pi / 180. for k in range(3)]
            sigma = np.random.rand() * 1.0
            key = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint32)
            color = self.augs.affine() if self.augs is not None else None
            rows[i] = self.plate_row(ids, [X, Y, Z] + rot, h, w, sigma, key, 5.0, color)
            x, y = self.camera.centre(X, Y, Z, h, w)
            labels[i, 0] = np.asarray([1, X, Y, Z, rot[0], rot[1], rot[2], x, y, 0], np.float32)
        return labels, rows

    def _device(self, dev):
        """What the device routes keep per device: the glyph atlas, staging buffers, plates and workspaces by batch size."""
        import torch
        state = self.__dict__.setdefault('_device_state', {})
        if state.get('device') != dev:
            state.clear()
            state.update(device=dev, atlas=torch.from_numpy(self.glyph_atlas()).to(dev), stage={}, plates={}, work={}, ocr_stage={}, ocr_work={})
        return state

    def add_device(self, imgs, r_max, add_rate=1.0, out=None):
        """add() with the pixels made on the device: imgs (B,3,h,w) float32 0..1 CUDA tensor (RenderCar.render_device's output)
        -> (images with plates, labels (B,1,10)), both on the device.  The host draws the parameter rows (draw_params); rows and
        labels go up in ONE pinned, non-blocking copy; yolo_plate_compose writes the plates from the resident glyph atlas,
        yolo_plate_stats takes each canvas's mean colour, yolo_plate_render samples, blurs, noises, colours and blends.  Runs on
        the current stream and does not synchronise.  out=imgs draws in place."""
        import torch
        from . import lib as L
        lib = L.load()
        if imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.dtype != torch.float32 or not imgs.is_cuda:
            raise ValueError('imgs should be a float32 CUDA tensor of shape (B, 3, h, w)')
        B, _, h, w = imgs.shape
        dev = imgs.device
        L.require_current_device(dev, 'this add_device call')
        imgs = imgs.contiguous()
        if out is None:
            out = torch.empty_like(imgs)
        elif tuple(out.shape) != tuple(imgs.shape) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError('out should be a contiguous float32 tensor of shape %r on %s' % (tuple(imgs.shape), dev))
        labels, rows = self.draw_params(B, h, w, r_max, add_rate)
        state = self._device(dev)
        nrow, nlab = rows.size * 4, labels.size * 4
        slot = state['stage'].get(B)
        if slot is None:
            slot = state['stage'][B] = [torch.empty(nrow + nlab, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        else:
            slot[1].synchronize()         # the previous upload has left the staging buffer (waits for that copy only)
        host = slot[0].numpy()
        host[:nrow] = rows.reshape(-1).view(np.uint8)
        host[nrow:] = labels.reshape(-1).view(np.uint8)
        up = torch.empty(nrow + nlab, dtype=torch.uint8, device=dev)
        up.copy_(slot[0], non_blocking=True)
        slot[1].record()
        plates = state['plates'].get(B)
        if plates is None:
            plates = state['plates'][B] = torch.empty((B, 160, 380, 4), dtype=torch.uint8, device=dev)
        work = state['work'].get((B, h, w))
        if work is None:
            nbytes = lib.yolo_plate_workspace_bytes(B, h, w)
            if nbytes <= 0:
                raise L.YoloError('plate_workspace_bytes failed with status %d' % nbytes)
            work = state['work'][(B, h, w)] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        st = L.stream_ptr()
        L.check(lib.yolo_plate_compose(L.ptr(state['atlas']), L.ptr(up), L.ptr(plates), B, st), 'plate_compose')
        L.check(lib.yolo_plate_stats(L.ptr(plates), L.ptr(up), L.ptr(work), B, h, w, st), 'plate_stats')
        L.check(lib.yolo_plate_render(L.ptr(imgs), L.ptr(plates), L.ptr(up), L.ptr(work), L.ptr(out), B, h, w, st), 'plate_render')
        return out, up[nrow:].view(torch.float32).view(B, 1, 10)

    def add(self, bg_batch, r_max, add_rate=1.0):
        """(:134-166) bg_batch (B,3,h,w) float32 0..1 CUDA tensor (RenderCar.render's output) -> (images with plates, labels)."""
        import torch
        B, _, h, w = bg_batch.shape
        fg, mask, labels = self.add_host(B, h, w, r_max, add_rate)
        dev = bg_batch.device
        img = composite(bg_batch, torch.from_numpy(fg).to(dev), torch.from_numpy(mask).to(dev), unit_bg=True)
        return img, torch.from_numpy(labels).to(dev)

    # ---- render (:168-214): the OCR batch -- a plate resized, sheared, rotated, blurred, noised, pasted on a 160 x 384 canvas ---
    def _ocr_args(self, kw):
        a = dict(OCR_RENDER_DEFAULTS)
        unknown = set(kw) - set(a)
        if unknown:
            raise TypeError('unknown OCR render arguments: %s' % ', '.join(sorted(unknown)))
        a.update(kw)
        return a

    def _ocr_draw(self, h, w, a):
        """The draws of one image of render(), in its order, up to and including the blur radius (then render() draws the noise
        field): -> dict(ids, glyph labels, LP_w, LP_h, m, n, deg, sigma)."""
        ids = [int(g) for g in np.random.randint(10, 34, size=3)]
        ids += [9 if g == 4 else int(g) for g in np.random.randint(0, 9, size=4)]
        resize = np.random.uniform(low=a['scale'][0], high=a['scale'][1])
        LP_w = int(380 * resize)
        LP_h = int(160 * resize * np.random.uniform(low=a['aspect'][0], high=a['aspect'][1]))
        m = n = deg = sigma = 0.0
        if a['M'] > 0 or a['N'] > 0:                              # (yolo_cv.py:106-109, 127)
            m, n = np.random.random() * a['M'] * 2 - a['M'], np.random.random() * a['N'] * 2 - a['N']
        if a['R'] != 0:
            deg = np.random.uniform(low=-a['R'], high=a['R'])
        if a['G'] != 0:
            sigma = np.random.rand() * a['G']
        if int(w - 0.9 * LP_w) <= int(-0.1 * LP_w) or int(h - 0.9 * LP_h) <= int(-0.1 * LP_h):
            raise ValueError('a %d x %d canvas leaves no paste position for a %d x %d plate' % (h, w, LP_h, LP_w))
        return dict(ids=ids, LP_w=LP_w, LP_h=LP_h, m=float(m), n=float(n), deg=float(deg), sigma=float(sigma))

    @staticmethod
    def _ocr_paste(d, h, w):
        """(:191-192) the paste position, drawn after the plate is made."""
        return (int(np.random.randint(int(-0.1 * d['LP_w']), int(w - 0.9 * d['LP_w']))),
                int(np.random.randint(int(-0.1 * d['LP_h']), int(h - 0.9 * d['LP_h']))))

    @staticmethod
    def ocr_labels(d, paste_x, w):
        """(:203-209) [[class, left, right]] x 7 as fractions of the canvas width, float32.  As written there: :203 converts the
        angle to radians although random_rotate has already done so (yolo_cv.py:151), so the formula sees r (pi / 180)^2 -- kept.
        ONE deliberate correction: the term |m| LP_h / 2, the shear's shift at the plate's mid-height, which the reference leaves
        out (its labels ignore the shear); it vanishes at M = 0."""
        r = math.radians(d['deg']) * math.pi / 180
        offset = paste_x + abs(d['LP_h'] * math.sin(r) / 2) + abs(d['m']) * d['LP_h'] / 2.
        cols = LP_GLYPH_X[:3] + LP_GLYPH_X[4:]
        return np.float32([[g, (offset + (c / 380.) * d['LP_w'] * math.cos(r)) / w, (offset + ((c + 45) / 380.) * d['LP_w'] * math.cos(r)) / w]
                           for g, c in zip(d['ids'], cols)])

    @staticmethod
    def ocr_geometry(d, paste_x, paste_y):
        """-> (M (3,3) float64: canvas pixel INDEX -> plate texel INDEX, affine; [l, t, r, b]: the paste rectangle, unclipped).
        The stages of render() as maps between continuous coordinates (pixel k spans [k, k+1]), composed: canvas -> (less the
        paste position) the rotated image -> (PIL's rotate, expand=1) the sheared image -> (random_shearing's AFFINE data) the
        resized plate -> (scale) the 380 x 160 plate.  PIL crops at every stage's image; the composed map does not."""
        LP_w, LP_h, m, n = d['LP_w'], d['LP_h'], d['m'], d['n']
        xshift, yshift = abs(m) * LP_h, abs(n) * LP_w
        w2, h2 = LP_w + int(round(xshift)), LP_h + int(round(yshift))
        shear = np.array([[1.0, m, -xshift if m > 0 else 0.0], [n, 1.0, -yshift if n > 0 else 0.0], [0.0, 0.0, 1.0]])
        if d['deg'] != 0:
            nw, nh, rot = pil_rotate_matrix(w2, h2, d['deg'])
        else:
            nw, nh, rot = w2, h2, np.eye(3)
        half = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
        back = np.array([[1.0, 0.0, -paste_x], [0.0, 1.0, -paste_y], [0.0, 0.0, 1.0]])
        M = np.linalg.inv(half) @ np.diag([380. / LP_w, 160. / LP_h, 1.0]) @ shear @ rot @ back @ half
        return M, [paste_x, paste_y, paste_x + int(nw), paste_y + int(nh)]

    def ocr_row(self, d, paste_x, paste_y, h, w, key, sigma_noise, color=None):
        """One parameter row (PLATE_ROW_WORDS int32 words; include/yolo_amd.h, yolo_ocr_plate_blur): the affine map in words
        16..24, the canvas-clipped paste rectangle as the window, words 25 and 26 unused."""
        M, win = self.ocr_geometry(d, paste_x, paste_y)
        row = np.zeros(PLATE_ROW_WORDS, np.int32)
        fl = row.view(np.float32)
        row[0] = 1
        row[1:8] = d['ids']
        row[8:12] = [min(max(win[0], 0), w), min(max(win[1], 0), h), min(max(win[2], 0), w), min(max(win[3], 0), h)]
        row[12:14] = np.asarray(key, np.uint32).view(np.int32)
        fl[14] = np.float32(sigma_noise / PLATE_NOISE_UNIT)
        fl[16:25] = M.reshape(-1).astype(np.float32)
        A, D, e = (np.eye(3), np.zeros((3, 3)), np.zeros(3)) if color is None else color
        fl[27:36], fl[36:45], fl[45:48] = (np.asarray(A, np.float64).reshape(-1).astype(np.float32),
                                           np.asarray(D, np.float64).reshape(-1).astype(np.float32), np.asarray(e, np.float64).astype(np.float32))
        return row

    def draw_ocr_params(self, batch, h, w, **kw):
        """render_host's draws without touching a pixel -> (labels (B,7,3) float32, rows (B, PLATE_ROW_WORDS) int32, taps
        (B, OCR_TAP_WORDS) int32, orders (B,7) int32: loss_mask's nd.random.shuffle of each image's labels, drawn after the images).
        Host only.  Per image: three letters, four digits (4 -> 9), resize, aspect, shear m and n, the angle, the blur radius --
        render_host's draws so far --, then the paste position, TWO uint32 key words where the host route draws a field of normals
        BEFORE the paste position, then the colour augmenter's draws.  So the first image has render_host's glyphs, sizes, shear,
        angle and blur; its paste position too when the host's noise field is not drawn from the stream."""
        a = self._ocr_args(kw)
        labels = -np.ones((batch, 7, 3), np.float32)
        rows = np.zeros((batch, PLATE_ROW_WORDS), np.int32)
        taps = np.zeros((batch, OCR_TAP_WORDS), np.int32)
        for i in range(batch):
            d = self._ocr_draw(h, w, a)
            paste_x, paste_y = self._ocr_paste(d, h, w)
            key = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint32) if a['noise'] != 0 else (0, 0)
            color = self.ocr_augs.affine() if self.ocr_augs is not None else None
            rows[i] = self.ocr_row(d, paste_x, paste_y, h, w, key, a['noise'], color)
            taps[i] = gaussian_taps(d['sigma'])
            labels[i] = self.ocr_labels(d, paste_x, w)
        orders = np.stack([np.random.permutation(7) for _ in range(batch)]).astype(np.int32)
        return labels, rows, taps, orders

    def render_host(self, batch, h, w, **kw):
        """The host half of render() (:178-209), with PIL as written: (fg, mask (B,3,h,w) float32, labels (B,7,3))."""
        from PIL import Image, ImageFilter
        a = self._ocr_args(kw)
        fg = np.zeros((batch, 3, h, w), np.float32)
        mask = np.zeros((batch, 3, h, w), np.float32)
        labels = -np.ones((batch, 7, 3), np.float32)
        cols = LP_GLYPH_X[:3] + LP_GLYPH_X[4:]
        for i in range(batch):
            d = self._ocr_draw(h, w, a)
            plate = Image.new('RGBA', (380, 160), (255, 255, 255))
            for g, c in zip(d['ids'], cols):
                plate.paste(self.glyph[g], (c, 35))
            plate.paste(self.dot, (LP_GLYPH_X[3], 45))
            plate = plate.resize((d['LP_w'], d['LP_h']), Image.BILINEAR)
            if a['M'] > 0 or a['N'] > 0:                          # random_shearing (yolo_cv.py:120-135)
                m, n = d['m'], d['n']
                xshift, yshift = abs(m) * d['LP_h'], abs(n) * d['LP_w']
                plate = plate.transform((d['LP_w'] + int(round(xshift)), d['LP_h'] + int(round(yshift))), Image.AFFINE,
                                        (1, m, -xshift if m > 0 else 0, n, 1, -yshift if n > 0 else 0), Image.BILINEAR)
            if a['R'] != 0:
                plate = plate.rotate(d['deg'], Image.BILINEAR, expand=1)
            if a['G'] != 0:
                plate = plate.filter(ImageFilter.GaussianBlur(radius=d['sigma']))
            if a['noise'] != 0:
                px = np.array(plate)
                plate = Image.fromarray(np.uint8(np.clip(px + np.random.normal(0., a['noise'], px.shape), 0, 255)))
            paste_x, paste_y = self._ocr_paste(d, h, w)
            tmp = Image.new('RGBA', (w, h))
            tmp.paste(plate, (paste_x, paste_y))
            bands = tmp.split()
            rgb = np.asarray(Image.merge('RGB', bands[:3]), np.float32)
            if self.ocr_augs is not None:
                rgb = self.ocr_augs(rgb)
            mask[i] = np.asarray(bands[-1], np.float32) / np.float32(255.)
            fg[i] = rgb.transpose(2, 0, 1) / np.float32(255.)
            labels[i] = self.ocr_labels(d, paste_x, w)
        return fg, mask, labels

    def render(self, bg, **kw):
        """(:168-214) bg (B,3,h,w) float32 0..255 CUDA tensor (BackgroundBank.next_batch's output) -> (images 0..1, labels
        (B,7,3) [class, left, right]) on the device: the plates drawn with PIL on the host, the blend on the device.
        Keyword arguments (OCR_RENDER_DEFAULTS): scale, aspect, R, G as the reference's call passes them; noise = 10.0,
        PILImageEnhance's own default (the call passes no noise_var); M = N = 0.1 where the call passes 10.0 -- as
        random_shearing stands (yolo_cv.py:120-135) M is a shear FACTOR, so 10.0 smears a plate over up to ten times its height
        while the labels ignore it; 10.0 can be passed and is rendered faithfully."""
        import torch
        B, _, h, w = bg.shape
        fg, mask, labels = self.render_host(B, h, w, **kw)
        dev = bg.device
        return composite(bg, torch.from_numpy(fg).to(dev), torch.from_numpy(mask).to(dev)), torch.from_numpy(labels).to(dev)

    def render_device(self, bg, out=None, **kw):
        """render() with the pixels made on the device: bg (B,3,h,w) float32 0..255 CUDA tensor -> (images 0..1, labels (B,7,3)),
        both on the device.  The host draws rows, taps, labels and shuffle orders (draw_ocr_params); they go up in ONE pinned,
        non-blocking copy; yolo_plate_compose writes the plates, yolo_ocr_plate_blur samples, blurs and noises the paste
        rectangle and takes the colour sums, yolo_ocr_plate_render colours and blends.  Runs on the current stream and does not
        synchronise.  out=bg draws in place.  The orders of this call stay on the device as self.ocr_order (B,7) int32, for
        ocr_targets.  The blur is a true Gaussian of sigma = rand * G truncated at min(ceil(3 sigma), 24) taps -- this library's
        rule, not PIL's box-blur approximation: the same kind of picture, not the same pixels.  Keyword arguments: see render()."""
        import torch
        from . import lib as L
        lib = L.load()
        if bg.dim() != 4 or bg.shape[1] != 3 or bg.dtype != torch.float32 or not bg.is_cuda:
            raise ValueError('bg should be a float32 CUDA tensor of shape (B, 3, h, w)')
        B, _, h, w = bg.shape
        dev = bg.device
        L.require_current_device(dev, 'this render_device call')
        bg = bg.contiguous()
        if out is None:
            out = torch.empty_like(bg)
        elif tuple(out.shape) != tuple(bg.shape) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
            raise ValueError('out should be a contiguous float32 tensor of shape %r on %s' % (tuple(bg.shape), dev))
        labels, rows, taps, orders = self.draw_ocr_params(B, h, w, **kw)
        state = self._device(dev)
        sizes = [rows.size * 4, taps.size * 4, labels.size * 4, orders.size * 4]
        ends = np.cumsum(sizes)
        slot = state['ocr_stage'].get(B)
        if slot is None:
            slot = state['ocr_stage'][B] = [torch.empty(int(ends[-1]), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        else:
            slot[1].synchronize()         # the previous upload has left the staging buffer (waits for that copy only)
        host = slot[0].numpy()
        for part, end, size in zip((rows, taps, labels, orders), ends, sizes):
            host[end - size:end] = part.reshape(-1).view(np.uint8)
        up = torch.empty(int(ends[-1]), dtype=torch.uint8, device=dev)
        up.copy_(slot[0], non_blocking=True)
        slot[1].record()
        plates = state['plates'].get(B)
        if plates is None:
            plates = state['plates'][B] = torch.empty((B, 160, 380, 4), dtype=torch.uint8, device=dev)
        work = state['ocr_work'].get((B, h, w))
        if work is None:
            nbytes = lib.yolo_ocr_plate_workspace_bytes(B, h, w)
            if nbytes <= 0:
                raise L.YoloError('ocr_plate_workspace_bytes failed with status %d' % nbytes)
            work = state['ocr_work'][(B, h, w)] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        st = L.stream_ptr()
        taps_d = up[int(ends[0]):int(ends[1])]
        L.check(lib.yolo_plate_compose(L.ptr(state['atlas']), L.ptr(up), L.ptr(plates), B, st), 'plate_compose')
        L.check(lib.yolo_ocr_plate_blur(L.ptr(plates), L.ptr(up), L.ptr(taps_d), L.ptr(work), B, h, w, st), 'ocr_plate_blur')
        L.check(lib.yolo_ocr_plate_render(L.ptr(bg), L.ptr(up), L.ptr(work), L.ptr(out), B, h, w, 0, st), 'ocr_plate_render')
        self.ocr_order = up[int(ends[2]):int(ends[3])].view(torch.int32).view(B, 7)
        return out, up[int(ends[1]):int(ends[2])].view(torch.float32).view(B, 7, 3)
