"""The device OCR plate renderer restated in numpy: yolo_ocr_plate_blur and yolo_ocr_plate_render as include/yolo_amd.h defines
them, every operation in float32 and in the header's order (the sample S, the rows, the noise and the plates are
tests/plate_ref.py's), so an IEEE device reproduces it bit for bit -- except the canvas mean, which is taken here from ONE float64
sum (the device adds the sums of its 32 x 32 tiles: the float32 it rounds to can differ by an ulp)."""
import numpy as np

import plate_ref as pr

f32 = np.float32
TAP_WORDS = 32
BLUR_TAPS = 24
TILE = 32


def make_taps(T, weights=None, sigma=None):
    """A tap row by hand: T taps per side with the given w[0..T], or a normalised Gaussian of `sigma`."""
    row = np.zeros(TAP_WORDS, np.int32)
    fl = row.view(f32)
    row[0] = T
    if weights is None:
        k = np.arange(T + 1, dtype=np.float64)
        g = np.exp(-k * k / (2.0 * sigma * sigma)) if T else np.ones(1)
        weights = g / (g[0] + 2.0 * g[1:].sum())
    fl[1:T + 2] = np.asarray(weights, np.float64).astype(f32)
    return row


def unpack_taps(row):
    row = np.ascontiguousarray(row, np.int32)
    T = min(max(int(row[0]), 0), BLUR_TAPS)
    return T, row.view(f32)[1:T + 2].copy()


def _pass(S, T, w, axis):
    """sum over k = -T..T in ascending order of w[|k|] * S shifted by k along `axis`; the result is 2 T shorter there."""
    n = S.shape[axis] - 2 * T

    def cut(k):
        idx = [slice(None)] * S.ndim
        idx[axis] = slice(k, k + n)
        return S[tuple(idx)]
    acc = w[T] * cut(0)
    for k in range(1, 2 * T + 1):
        acc = acc + w[abs(k - T)] * cut(k)
    assert acc.dtype == f32
    return acc


def quad(plate, r, taps, H, W):
    """Q for every pixel of an (H, W) canvas -> (H, W, 4) float32: 0 outside the window."""
    T, w = unpack_taps(taps)
    l, t, rr, b = pr.window_of(r, H, W)
    Q = np.zeros((H, W, 4), f32)
    if rr <= l or b <= t:
        return Q
    j = np.broadcast_to(np.arange(l - T, rr + T, dtype=np.float64).astype(f32)[None, :], (b - t + 2 * T, rr - l + 2 * T))
    i = np.broadcast_to(np.arange(t - T, b + T, dtype=np.float64).astype(f32)[:, None], (b - t + 2 * T, rr - l + 2 * T))
    with np.errstate(all='ignore'):
        S = pr.sample(plate, r['m'], j, i)
        P = S if T == 0 else _pass(_pass(S, T, w, 1), T, w, 0)
        if r['s'] != 0:
            P = np.fmin(np.fmax(P + pr.noise_z(r['key'], H, W)[t:b, l:rr] * r['s'], f32(0)), f32(255))
    assert P.dtype == f32 and P.shape == (b - t, rr - l, 4)
    Q[t:b, l:rr] = P
    return Q


def render(bg, plates, rows, taps, bg_unit=False, return_parts=False):
    """bg (N,3,H,W) float32 0..255 (bg_unit: 0..1), plates (N,160,380,4) uint8, rows (N, 48) int32, taps (N, 32) int32 -> out
    (N,3,H,W) float32 0..1 (return_parts: also the per-image mean colour float32 (N,3), the mask (N,H,W) and Q (N,H,W,4))."""
    bg = np.asarray(bg, f32)
    N, _, H, W = bg.shape
    unit = bg if bg_unit else bg / f32(255)
    out = np.fmin(np.fmax(unit, f32(0)), f32(1))
    mus, masks, Qs = np.zeros((N, 3), f32), np.zeros((N, H, W), f32), np.zeros((N, H, W, 4), f32)
    for n in range(N):
        r = pr.unpack(rows[n])
        if not pr.has_plate(r):
            continue
        Q = quad(plates[n], r, taps[n], H, W)
        l, t, rr, b = pr.window_of(r, H, W)
        if rr <= l or b <= t:
            continue
        with np.errstate(all='ignore'):
            mu = (Q[..., :3].astype(np.float64).sum(axis=(0, 1)) / float(H * W)).astype(f32)
            k = ((r['D'][:, 0] * mu[0] + r['D'][:, 1] * mu[1]) + r['D'][:, 2] * mu[2]) + r['e']
            Qw = Q[t:b, l:rr]
            mask = Qw[..., 3] / f32(255)
            for c in range(3):
                A = r['A'][c]
                fg = (((A[0] * Qw[..., 0] + A[1] * Qw[..., 1]) + A[2] * Qw[..., 2]) + k[c]) / f32(255)
                under = bg[n, c, t:b, l:rr] * (f32(1) - mask)
                v = (under if bg_unit else under / f32(255)) + fg * mask
                assert v.dtype == f32
                out[n, c, t:b, l:rr] = np.fmin(np.fmax(v, f32(0)), f32(1))
        mus[n], Qs[n] = mu, Q
        masks[n, t:b, l:rr] = mask
    return (out, mus, masks, Qs) if return_parts else out


def workspace_layout(N, H, W):
    """(bytes of the tile sums, byte offset of Q, bytes in all, tiles per image) -- include/yolo_amd.h, yolo_ocr_plate_blur."""
    tiles = ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    sums = N * tiles * 3 * 8
    q_off = (sums + 15) // 16 * 16
    return sums, q_off, q_off + N * H * W * 16, tiles
