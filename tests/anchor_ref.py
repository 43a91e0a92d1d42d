"""The anchor fit restated naively in numpy from the definition in include/yolo_amd.h (yolo_anchor_assign / yolo_anchor_kmeans): row
by row and cluster by cluster, every float32 operation made one by one on numpy float32 scalars, the sums in double.  Shares no
code with yolo_amd/anchors.py or the kernels; slow on purpose (the tests keep n small)."""
import numpy as np

F = np.float32


def sizes(n, seed, area=(0.02, 0.6), aspect_sigma=0.35):
    """n box sizes [h, w] as fractions of an image: log-uniform area, log-normal aspect h / w."""
    rng = np.random.default_rng(seed)
    a = np.exp(rng.uniform(np.log(area[0]), np.log(area[1]), n))
    r = np.exp(rng.normal(0.0, aspect_sigma, n))
    return np.stack([np.sqrt(a * r), np.sqrt(a / r)], axis=1).astype(np.float32)


def is_valid(h, w):
    return bool(np.isfinite(h) and np.isfinite(w) and h > 0 and w > 0)


def iou(h, w, ch, cw):
    """q of one row against one centroid; float32 scalars in, float32 out."""
    ih = min(h, ch)
    iw = min(w, cw)
    inter = F(ih * iw)
    union = F(F(F(h * w) + F(ch * cw)) - inter)
    return F(inter / union)


def assign(rows, cent):
    """One assignment pass -> dict(assign (n) int32, best_iou (n) float32, counts (k) int32, mean_iou float, n_valid int, gap):
    gap is the smallest difference between a valid row's best and second-best q (inf for k = 1 or no valid row)."""
    rows, cent = np.asarray(rows, np.float32), np.asarray(cent, np.float32)
    n, k = len(rows), len(cent)
    a = np.full(n, -1, np.int32)
    q = np.zeros(n, np.float32)
    counts = np.zeros(k, np.int32)
    total, n_valid, gap = 0.0, 0, float('inf')
    for i in range(n):
        h, w = rows[i, 0], rows[i, 1]
        if not is_valid(h, w):
            continue
        best, second = 0, None
        with np.errstate(all='ignore'):
            qs = [iou(h, w, cent[j, 0], cent[j, 1]) for j in range(k)]
        for j in range(1, k):
            if qs[j] > qs[best]:
                best = j
        for j in range(k):
            if j != best and (second is None or qs[j] > second):
                second = qs[j]
        if second is not None:
            gap = min(gap, float(qs[best]) - float(second))
        a[i], q[i] = best, qs[best]
        counts[best] += 1
        total += float(qs[best])
        n_valid += 1
    return dict(assign=a, best_iou=q, counts=counts, mean_iou=total / n_valid if n_valid else 0.0, n_valid=n_valid, gap=gap)


def update(rows, cent, a):
    """The centroids after one update with the assignment a: the double mean of a cluster's rows, rounded to float32 once; an empty
    cluster keeps its centroid."""
    rows = np.asarray(rows, np.float32)
    new = np.array(cent, np.float32)
    for j in range(len(new)):
        sh, sw, c = 0.0, 0.0, 0
        for i in range(len(rows)):
            if a[i] == j:
                sh += float(rows[i, 0])
                sw += float(rows[i, 1])
                c += 1
        if c > 0:
            new[j, 0], new[j, 1] = F(sh / float(c)), F(sw / float(c))
    return new


def step(rows, cent):
    """assign + update: the centroids one round later."""
    return update(rows, cent, assign(rows, cent)['assign'])


def fit(rows, init, max_iters):
    """One restart -> dict(centroids, counts, mean_iou, n_valid, iters, converged, gap): gap is the smallest best-to-second-best
    margin over every assignment pass of the run."""
    cent = np.array(init, np.float32)
    iters, converged, gap = 0, 0, float('inf')
    while True:
        p = assign(rows, cent)
        gap = min(gap, p['gap'])
        if converged or iters >= max_iters:
            return dict(centroids=cent, counts=p['counts'], mean_iou=p['mean_iou'], n_valid=p['n_valid'], iters=iters,
                        converged=converged, gap=gap)
        new = update(rows, cent, p['assign'])
        iters += 1
        converged = int(new.tobytes() == cent.tobytes())
        cent = new


def ulp_diff(a, b):
    """The largest distance in float32 steps between two arrays of positive finite numbers."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0
