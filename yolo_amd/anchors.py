"""Anchor fitting: the reference's `kmean` mode (car/YOLO.py:599-638) and its IoU k-means (yolo_modules/iou_kmeans.py) -- what
spec['all_anchors'] is made with -- on the device (csrc/anchors.hip; the definition is in include/yolo_amd.h, yolo_anchor_assign).

  sample_sizes(renderer, n)      <- the kmean mode's loop            car/YOLO.py:610-616 (labels only: no pixel is drawn)
  fit_anchors(sizes, k)          <- iou_kmeans.main                  iou_kmeans.py:11-52, many restarts, each to convergence
  anchor_quality(sizes, anchors)    mean best IoU of the anchors a spec already has (one yolo_anchor_assign call)

The reference makes one random start and exactly 10 rounds on 1000 samples, and fails when a cluster runs empty
(iou_kmeans.py:42); here every restart runs until its centroids stop changing, the best one is kept, and an empty cluster keeps
its centroid.  dis_method='L2' is not offered: the kmean mode never uses it.  `device=None` runs the same definition in numpy
(no GPU and no torch needed); it is the host restatement of the kernels, not a fallback: a device that is asked for and missing
is an error."""
import numpy as np

MAX_K, MAX_RESTARTS, MAX_ITERS = 32, 65535, 10000        # the library's limits (include/yolo_amd.h)


# ---- the definition in numpy (device=None) ---------------------------------------------------------------------------------
def _valid(sizes):
    h, w = sizes[:, 0], sizes[:, 1]
    with np.errstate(invalid='ignore'):
        return np.isfinite(h) & np.isfinite(w) & (h > 0) & (w > 0)


def _assign_host(sizes, cent):
    """-> (assign (n) int32, best_iou (n) float32, counts (k) int32, mean_iou float, n_valid int); float32 operation by operation."""
    sizes, cent = np.asarray(sizes, np.float32), np.asarray(cent, np.float32)
    ok = _valid(sizes)
    h, w = sizes[ok, 0:1], sizes[ok, 1:2]
    ch, cw = cent[None, :, 0], cent[None, :, 1]
    with np.errstate(all='ignore'):
        inter = np.minimum(h, ch) * np.minimum(w, cw)
        q = inter / ((h * w + ch * cw) - inter)
    best = np.argmax(q, axis=1) if len(q) else np.zeros(0, np.int64)        # the first of equal maxima: the lowest j
    assign = np.full(len(sizes), -1, np.int32)
    best_iou = np.zeros(len(sizes), np.float32)
    assign[ok] = best
    best_iou[ok] = q[np.arange(len(q)), best]
    counts = np.bincount(best, minlength=len(cent)).astype(np.int32)
    n_valid = int(ok.sum())
    mean_iou = float(best_iou[ok].astype(np.float64).sum() / n_valid) if n_valid else 0.0
    return assign, best_iou, counts, mean_iou, n_valid


def _kmeans_host(sizes, init, max_iters):
    """One restart: -> (centroids (k,2), counts, mean_iou, iters, converged)."""
    sizes = np.asarray(sizes, np.float32)
    cent = np.array(init, np.float32)
    iters, converged = 0, 0
    while True:
        assign, _, counts, mean_iou, _ = _assign_host(sizes, cent)
        if converged or iters >= max_iters:
            return cent, counts, mean_iou, iters, converged
        new = cent.copy()
        for j in range(len(cent)):
            if counts[j] > 0:
                rows = sizes[assign == j].astype(np.float64)
                new[j] = (rows.sum(axis=0) / np.float64(counts[j])).astype(np.float32)
        iters += 1
        converged = int(np.array_equal(new.view(np.uint32), cent.view(np.uint32)))
        cent = new


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _is_tensor(x):
    return type(x).__module__.split('.')[0] == 'torch'


def _check_shape(shape):
    """The one rule for every route and every kind of input: (n, 2) rows [h, w], or labels (B, nobj, >= 5).  -> True for labels."""
    shape = tuple(shape)
    if len(shape) == 3 and shape[2] >= 5:
        return True
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError('sizes must be (n, 2) [h, w] or a label tensor (B, nobj, >= 5), got %s' % (shape,))
    return False


def _host_rows(sizes):
    """(n, 2) float32 [h, w] on the host of any accepted input (a device input is copied here, once)."""
    if _is_tensor(sizes):
        sizes = sizes.detach().cpu().numpy()
    a = np.asarray(sizes, np.float32)
    if _check_shape(a.shape):
        a = a[:, :, 3:5].reshape(-1, 2)                   # labels [cls, y, x, h, w, ...]: car/YOLO.py:616
    return np.ascontiguousarray(a)


def _device_rows(sizes, device, host=None):
    """-> (tensor to keep alive, pointer of row 0, stride in floats, n): a float32 CUDA tensor is read in place where its layout
    allows; anything else goes up as dense (n, 2) rows (`host`, when the caller already has them).  The shape is checked before
    any pointer is formed: what the numpy route refuses is refused here with the same ValueError."""
    import torch
    labels = _check_shape(sizes.shape if _is_tensor(sizes) else np.shape(sizes))
    if _is_tensor(sizes) and sizes.is_cuda and sizes.dtype == torch.float32 and sizes.device == device:
        t = sizes
        if not labels and t.stride(1) == 1 and t.stride(0) >= 2:
            return t, t.data_ptr(), t.stride(0), t.shape[0]
        if labels and t.stride(2) == 1 and t.stride(1) >= 5 and t.stride(0) == t.shape[1] * t.stride(1):
            return t, t.data_ptr() + 3 * 4, t.stride(1), t.shape[0] * t.shape[1]
    host = _host_rows(sizes) if host is None else host
    t = torch.from_numpy(host).to(device)
    return t, t.data_ptr(), 2, host.shape[0]


def _check_k(k, restarts=1, max_iters=1):
    if not 1 <= k <= MAX_K:
        raise ValueError('k must be 1..%d (yolo_grid_desc holds 4 scales x 8 anchors), got %d' % (MAX_K, k))
    if not 1 <= restarts <= MAX_RESTARTS or not 1 <= max_iters <= MAX_ITERS:
        raise ValueError('restarts must be 1..%d and max_iters 1..%d' % (MAX_RESTARTS, MAX_ITERS))


# ---- the public interface --------------------------------------------------------------------------------------------------
class AnchorFit(object):
    """The result of fit_anchors: `anchors` (k, 2) float32 [h, w] of the restart with the highest mean IoU (the lowest index among
    equals), sorted by area ascending, `counts` (k) in the same order, that restart's `mean_iou`, `iters`, `converged` and index
    `restart`, and `runs`: the per-restart 'mean_iou', 'iters' and 'converged' arrays."""

    def __init__(self, centroids, counts, mean_iou, iters, converged):
        mean_iou = np.asarray(mean_iou, np.float64)
        r = int(np.argmax(mean_iou))
        cent = np.asarray(centroids, np.float32)[r]
        order = np.argsort(cent[:, 0] * cent[:, 1], kind='stable')
        self.anchors, self.counts = cent[order], np.asarray(counts, np.int32)[r][order]
        self.mean_iou, self.iters, self.converged, self.restart = float(mean_iou[r]), int(iters[r]), bool(converged[r]), r
        self.runs = {'mean_iou': mean_iou, 'iters': np.asarray(iters, np.int32), 'converged': np.asarray(converged, np.int32) != 0}

    def all_anchors(self, scales=3):
        """The nested list spec['all_anchors'] holds (car/v1/spec.yaml:7-11): the finest scale first, the smallest anchors first."""
        k = len(self.anchors)
        if scales < 1 or k % scales != 0:
            raise ValueError('%d anchors do not divide into %d scales' % (k, scales))
        per = k // scales
        return [[[float(h), float(w)] for h, w in self.anchors[s * per:(s + 1) * per]] for s in range(scales)]


def sample_sizes(renderer, n, mode='train', pascal_rate=0.2, render_rate=1.0, batch=256):
    """The kmean mode's sample (car/YOLO.py:610-616: label[0, 0, 3:5] of n rendered images) from RenderCar.draw_params, which
    makes render's draws without touching a pixel: -> (m, 2) float32 [h, w] as fractions of the image, m <= n (an image without
    an object is dropped).  Host only."""
    out = []
    for b0 in range(0, n, batch):
        labels, _ = renderer.draw_params(min(batch, n - b0), mode, pascal_rate, render_rate)
        hw = labels[:, 0, 3:5]
        out.append(hw[_valid(hw)])
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 2), np.float32)


def fit_anchors(sizes, k=9, restarts=16, max_iters=300, device='cuda:0'):
    """IoU k-means on box sizes -> AnchorFit.  sizes: numpy (n, 2) [h, w], a CUDA tensor (n, 2), or a label tensor
    (B, nobj, >= 5) [cls, y, x, h, w, ...], which is read in place; rows that are not finite and positive (the -1 of 'no
    object') are ignored.  Each restart starts from k distinct valid rows, np.random.choice(valid rows, k, replace=False)
    (iou_kmeans.py:22; numpy's global generator, as the renderers use it), runs until its centroids stop changing or for max_iters
    rounds, and the one with the highest mean IoU is kept.  All restarts run in ONE launch, one workgroup each.
    An offline call: a device input is copied to the host once for the init draw, and the call synchronises to read its results.
    device=None runs the same definition in numpy."""
    _check_k(k, restarts, max_iters)
    host = _host_rows(sizes)
    rows = np.flatnonzero(_valid(host))
    if len(rows) < k:
        raise ValueError('%d valid rows cannot start %d clusters' % (len(rows), k))
    init = np.stack([host[np.random.choice(rows, k, replace=False)] for _ in range(restarts)]).astype(np.float32)
    if device is None:
        runs = [_kmeans_host(host, init[r], max_iters) for r in range(restarts)]
        return AnchorFit(*[np.stack([np.asarray(run[c]) for run in runs]) for c in range(5)])
    import torch
    from . import lib as L
    lib = L.load()
    device = L.resolve_device(device)
    L.require_current_device(device, 'fit_anchors')
    keep, ptr, stride, n = _device_rows(sizes, device, host)
    d_init = torch.from_numpy(init).to(device)
    cent = torch.empty((restarts, k, 2), dtype=torch.float32, device=device)
    counts = torch.empty((restarts, k), dtype=torch.int32, device=device)
    mean_iou = torch.empty((restarts,), dtype=torch.float64, device=device)
    small = torch.empty((2 * restarts + 1,), dtype=torch.int32, device=device)          # iters, converged, n_valid
    ws = torch.empty((lib.yolo_anchor_workspace_bytes(n, restarts, k),), dtype=torch.uint8, device=device)
    L.check(lib.yolo_anchor_kmeans(ptr, stride, n, L.ptr(d_init), restarts, k, max_iters, L.ptr(cent), L.ptr(counts), L.ptr(mean_iou),
                                   small.data_ptr(), small.data_ptr() + 4 * restarts, small.data_ptr() + 8 * restarts, L.ptr(ws),
                                   L.stream_ptr()), 'anchor_kmeans')
    small = small.cpu().numpy()
    del keep
    return AnchorFit(cent.cpu().numpy(), counts.cpu().numpy(), mean_iou.cpu().numpy(), small[:restarts], small[restarts:2 * restarts])


def anchor_quality(sizes, all_anchors, device='cuda:0'):
    """How well the anchors of a spec fit a sample: {'mean_iou': mean over the valid rows of the best IoU with any anchor,
    'counts': rows per anchor in all_anchors' order (flattened), 'n_valid'}.  One assignment pass (yolo_anchor_assign); an
    offline call, it synchronises.  device=None runs the same definition in numpy."""
    cent = np.asarray(all_anchors, np.float32).reshape(-1, 2)
    _check_k(len(cent))
    if device is None:
        _, _, counts, mean_iou, n_valid = _assign_host(_host_rows(sizes), cent)
        return {'mean_iou': mean_iou, 'counts': counts, 'n_valid': n_valid}
    import torch
    from . import lib as L
    lib = L.load()
    device = L.resolve_device(device)
    L.require_current_device(device, 'anchor_quality')
    keep, ptr, stride, n = _device_rows(sizes, device)
    k = len(cent)
    if n == 0:                                            # (no row: what the numpy route gives, without a launch)
        return {'mean_iou': 0.0, 'counts': np.zeros(k, np.int32), 'n_valid': 0}
    d_cent = torch.from_numpy(np.ascontiguousarray(cent)).to(device)
    counts = torch.empty((k + 1,), dtype=torch.int32, device=device)                    # counts, n_valid
    mean_iou = torch.empty((1,), dtype=torch.float64, device=device)
    ws = torch.empty((lib.yolo_anchor_workspace_bytes(n, 1, k),), dtype=torch.uint8, device=device)
    L.check(lib.yolo_anchor_assign(ptr, stride, n, L.ptr(d_cent), k, None, None, L.ptr(counts), L.ptr(mean_iou),
                                   counts.data_ptr() + 4 * k, L.ptr(ws), L.stream_ptr()), 'anchor_assign')
    counts = counts.cpu().numpy()
    del keep
    return {'mean_iou': float(mean_iou.cpu().numpy()[0]), 'counts': counts[:k].copy(), 'n_valid': int(counts[k])}
