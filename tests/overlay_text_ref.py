"""The overlay's text and the published row restated in numpy / plain Python integers (the role tests/overlay_ref.py plays for the
shapes and the lines): include/yolo_amd.h's definitions of yolo_overlay_labels -- the score and degree formatting, the label
geometry --, of yolo_overlay_text -- the rasteriser, pixel by pixel --, and of yolo_pose_top1's class and depth lookup."""
import math

import numpy as np

import overlay_ref as R

f32 = np.float32
LABEL_WORDS = 16
LABEL_CHARS = 40
NAME_BYTES = 16
MAX_COORD = 2 ** 20
SAT = 2 ** 30
DEG = 57.29577951308232


# ---- text ----------------------------------------------------------------------------------------------------------------------
def score_text(s):
    """five bytes: d.ddd of min(round-half-even(s * 1000), 9999) for a finite s >= 0, else '-.---'."""
    s = float(f32(s))
    if not (s >= 0.0 and math.isfinite(s)):
        return '-.---'
    d = s * 1000.0                                       # exact in float64: 24 x 10 significant bits
    n = 9999 if d >= 9999.0 else int(round(d))           # Python's round(): to nearest, ties to even
    return '%d.%03d' % (n // 1000, n % 1000)


def deg_text(azimuth):
    """the degrees of an azimuth in radians: optional '-' and 1..3 digits, or None when it is not shown."""
    a = float(f32(azimuth))
    if not math.isfinite(a):
        return None
    d = float(np.rint(a * DEG))                          # ties to even, as rint
    if abs(d) > 999.0:
        return None
    return '%d' % int(d)                                 # (-0.0 prints '0')


def name_text(names, c):
    if names is None or c < 0 or c >= len(names):
        return ''
    raw = names[c].encode('ascii') if isinstance(names[c], str) else bytes(names[c])
    raw = raw[:NAME_BYTES].split(b'\0')[0]
    return raw.decode('latin-1')


def compose(name, score, azimuth=None):
    """[name ' '] score [' ' deg]; azimuth None: no degrees asked for."""
    t = (name + ' ' if name else '') + score_text(score)
    deg = deg_text(azimuth) if azimuth is not None else None
    return t + (' ' + deg if deg is not None else '')


def pack_label(x, y, text, ink, ground, flags, nchar=None):
    """-> the 16 words as Python ints (text: str or bytes, at most 40 bytes packed; nchar may be given beyond that)."""
    raw = text.encode('latin-1') if isinstance(text, str) else bytes(text)
    words = [int(x), int(y), R.pack_colour(ink) if not isinstance(ink, int) else ink,
             R.pack_colour(ground) if not isinstance(ground, int) else ground, int(flags), len(raw) if nchar is None else int(nchar)]
    words += [0] * 10
    for i, ch in enumerate(raw[:LABEL_CHARS]):
        words[6 + i // 4] |= ch << (8 * (i % 4))
    return words


def as_int32(words):
    return (np.asarray(words, np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)


def label_text(words):
    w = [int(v) & 0xffffffff for v in words]
    return bytes((w[6 + i // 4] >> (8 * (i % 4))) & 255 for i in range(min(max(int(words[5]), 0), LABEL_CHARS)))


# ---- labels --------------------------------------------------------------------------------------------------------------------
def place(slot, nchar, W, cell_w, cell_h, advance, scale, gap, pad):
    """the label geometry in Python integers -> (x, y), saturated to +-2^30."""
    v = [int(t) for t in slot[:8]]
    bx0, by0 = min(v[0::2]), min(v[1::2])
    Th, Tw = cell_h * scale, ((nchar - 1) * advance + cell_w) * scale
    y = by0 - gap - Th
    if y - pad < 0:
        y = by0 + gap
    x = bx0
    if x + Tw + pad > W:
        x = W - Tw - pad
    if x - pad < 0:
        x = pad
    sat = lambda t: max(-SAT, min(SAT, t))
    return sat(x), sat(y)


def labels(table, W, nms=None, kept_scores=None, cand_per_box=1, pred=None, pose=None, show_deg=True, lp=None, names=None,
           cell_w=6, cell_h=11, advance=6, scale=1, gap=4, pad=1, ground=(0, 0, 0)):
    """yolo_overlay_labels: table int32 (B,K,12) as yolo_overlay_shapes made it -> int32 (B,K,16).  ground None: no ground box."""
    table = np.asarray(table)
    B, K = table.shape[:2]
    post = nms[1].shape[1] if nms is not None else 0
    assert K == post + (pred is not None) + (lp is not None)
    out = np.zeros((B, K, LABEL_WORDS), np.int64)
    for b in range(B):
        for s in range(K):
            slot = table[b, s]
            on = bool(slot[10] != 0)
            c, azimuth = -1, None
            if s < post:
                rows, kept, count = nms
                idx = int(kept[b, s]) if s < min(int(count[b]), post) else -1
                box = idx // cand_per_box if idx >= 0 else -1
                on = on and 0 <= box < rows.shape[1]
                if not on:
                    continue
                c = idx % cand_per_box if cand_per_box > 1 else -1
                score = kept_scores[b, s] if kept_scores is not None else rows[b, box, 0]
            elif pred is not None and s == post:
                score = pred[b, 0]
                if pose is not None:
                    pc = float(pose[b, 3])
                    c = int(pc) if -1.0 < pc < (len(names) if names is not None else 0) else -1
                    azimuth = pose[b, 0] if show_deg else None
            else:
                score = lp[b, 0]
            if not on:
                continue
            text = compose(name_text(names, c), score, azimuth)
            x, y = place(slot, len(text), W, cell_w, cell_h, advance, scale, gap, pad)
            colour = int(slot[8]) & 0xffffffff
            out[b, s] = pack_label(x, y, text, colour, 0 if ground is None else R.pack_colour(ground), 1 | (0 if ground is None else 2))
    return as_int32(out)


# ---- the rasteriser ------------------------------------------------------------------------------------------------------------
def label_enabled(words):
    return bool(int(words[4]) & 1 and 0 <= int(words[5]) <= LABEL_CHARS and abs(int(words[0])) <= MAX_COORD and abs(int(words[1])) <= MAX_COORD)


def _paints(x, y, flags, nchar, text, font, first_code, cell_w, advance, scale, pad, px, py):
    nglyph, cell_h = len(font), len(font[0])
    Th, Tw = cell_h * scale, ((nchar - 1) * advance + cell_w) * scale
    if y <= py < y + Th and px >= x:
        i = (px - x) // (advance * scale)                # cells do not overlap (advance >= cell_w): the only cell P can lie in
        ox = x + i * advance * scale
        if i < nchar and px < ox + cell_w * scale:
            g = text[i] - first_code
            if 0 <= g < nglyph and (font[g][(py - y) // scale] >> ((px - ox) // scale)) & 1:
                return 'ink'
    if flags & 2 and nchar > 0 and x - pad <= px < x + Tw + pad and y - pad <= py < y + Th + pad:
        return 'ground'
    return None


def paints(words, font, first_code, cell_w, advance, scale, pad, px, py):
    """the rule for ONE label and ONE pixel -> 'ink', 'ground' or None (Python integers)."""
    if not label_enabled(words):
        return None
    rows = [[int(v) for v in g] for g in np.asarray(font)]
    return _paints(int(words[0]), int(words[1]), int(words[4]), int(words[5]), label_text(words), rows, first_code, cell_w, advance, scale,
                   pad, px, py)


def draw_text(frames, label_table, font, first_code, cell_w, advance, scale, pad):
    """yolo_overlay_text: frames (N,H,W,C) uint8, labels (N,K,16) int32, font (nglyph, cell_h) -> a painted copy.  Every pixel of
    every label's rectangle is asked the rule above, the labels ascending: a later label paints over an earlier one."""
    out = np.array(frames, copy=True)
    N, H, W, C = out.shape
    font = [[int(v) for v in g] for g in np.asarray(font)]
    cell_h = len(font[0])
    for n in range(N):
        for words in np.asarray(label_table)[n]:
            if not label_enabled(words) or int(words[5]) == 0:
                continue
            x, y, flags, nchar, text = int(words[0]), int(words[1]), int(words[4]), int(words[5]), label_text(words)
            Th, Tw = cell_h * scale, ((nchar - 1) * advance + cell_w) * scale
            ink = [(int(words[2]) >> (8 * c)) & 0xff for c in range(C)]
            ground = [(int(words[3]) >> (8 * c)) & 0xff for c in range(C)]
            for py in range(max(0, y - pad), min(H, y + Th + pad)):
                for px in range(max(0, x - pad), min(W, x + Tw + pad)):
                    what = _paints(x, y, flags, nchar, text, font, first_code, cell_w, advance, scale, pad, px, py)
                    if what is not None:
                        out[n, py, px] = ink if what == 'ink' else ground
    return out


def synthetic_font(seed, nglyph=12, cell_w=5, cell_h=7):
    """a seeded font for the codes 65..: glyph 0 all ink, glyph 1 empty, the others random."""
    g = np.random.default_rng(seed)
    font = g.integers(0, 1 << cell_w, (nglyph, cell_h)).astype(np.uint32)
    font[0] = (1 << cell_w) - 1
    font[1] = 0
    return font


# ---- the published row ---------------------------------------------------------------------------------------------------------
def top_class(logits):
    """the index of the largest logit, the lowest among equals; a NaN never wins."""
    best, top = 0, -math.inf
    for c, v in enumerate(logits):
        if float(v) > top:
            best, top = c, float(v)
    return best


def depth_at(row, depth):
    """depth (Hd,Wd) float32 or None, row [score, y, x, ...] -> float32 (video_node.py:239-243; -1 where the index leaves the image)."""
    if depth is None:
        return f32(-1)
    Hd, Wd = depth.shape
    y, x = float(f32(row[1])), float(f32(row[2]))
    if not (math.isfinite(x) and math.isfinite(y)):
        return f32(-1)
    xi, yi = int(Wd * x), int(Hd * y)                     # int(): truncation toward zero
    if not (0 <= xi < Wd and 0 <= yi < Hd):
        return f32(-1)
    return depth[yi, xi]
