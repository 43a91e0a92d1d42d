// Anchor fitting on the device for gfx950: the reference's kmean mode (car/YOLO.py:599-638, yolo_modules/iou_kmeans.py) -- k-means on
// box sizes (h, w) under the distance 1 / IoU of two boxes that share a corner -- with the restarts side by side, each run to
// convergence:
//   anchor_kmeans_kernel   one workgroup per restart, the whole Lloyd loop inside the kernel (assign, update, compare; at most
//                          max_iters rounds), then the statistics of the returned centroids
//   anchor_assign_kernel   one assignment pass of the same code with the per-row outputs (what anchor_quality asks for)
// Compiled with -ffp-contract=off: the arithmetic is the op-by-op fp32 definition of include/yolo_amd.h (yolo_anchor_assign), so
// tests/anchor_ref.py reproduces assignments and IoUs bit for bit and the means to the order of a double sum.
// A restart is one workgroup of 1024 threads on one CU: the sizes (8 B a row; 8 MB for a million rows) stay cache resident across the
// iterations and every block reads all of them each round, so a call costs one CU's time for n k IoUs a round, times ceil(R / 256);
// whether that CU waits for its vector pipe or for its row loads has not been measured (HBM it is not).  Thread t walks rows t, t + 1024, ... and keeps (sum h, sum w) in double and the count per cluster in
// registers -- predicated adds over ANCHOR_KA clusters with constant indices, as many passes over the rows as k needs (one up to 16) --
// then a shuffle tree inside the wave, a slab [wave][cluster] in LDS, and thread j adds the 16 waves in index order.  No atomics and
// no communication between workgroups: the same inputs give the same bits, and a restart does not see its neighbours.
#include "common.h"

constexpr int ANCHOR_THREADS = 1024;
constexpr int ANCHOR_WAVES = ANCHOR_THREADS / 64;
constexpr int ANCHOR_MAX_K = 32;                          // the Detector's 4 scales x 8 anchors
constexpr int ANCHOR_WORKSPACE_BYTES = 256;               // (nothing is kept there: a restart lives in one workgroup's LDS)

struct AnchorShared {
    float cent[ANCHOR_MAX_K][2];                          // the centroids of the round, [h, w]
    double sh[ANCHOR_WAVES][ANCHOR_MAX_K], sw[ANCHOR_WAVES][ANCHOR_MAX_K];
    int cnt[ANCHOR_WAVES][ANCHOR_MAX_K];
    double q[ANCHOR_WAVES];
    int valid[ANCHOR_WAVES];
    double sum_h[ANCHOR_MAX_K], sum_w[ANCHOR_MAX_K], sum_q;     // the block's totals
    int count[ANCHOR_MAX_K], n_valid;
    int stop;                                             // 0 go on, 1 converged, 2 max_iters reached: one more statistics pass
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    return v;
}

// (h, w) of row i; VEC: stride == 2 and an 8-byte aligned base
template <bool VEC>
__device__ __forceinline__ void anchor_row(const float* __restrict__ sizes, long long stride, long long i, float& h, float& w) {
    if (VEC) {
        const float2 v = reinterpret_cast<const float2*>(sizes)[i];
        h = v.x;
        w = v.y;
    } else {
        const float* p = sizes + i * stride;
        h = p[0];
        w = p[1];
    }
}

// the cluster of (h, w): the lowest j with the largest q; -1 and q = 0 for an invalid row
__device__ __forceinline__ int anchor_best(const AnchorShared& S, int k, float h, float w, float& best) {
    best = 0.f;
    // (finite and > 0: a NaN fails the comparison, +inf is excluded by the bound)
    if (!(h > 0.f && w > 0.f && h <= 3.402823466e+38f && w <= 3.402823466e+38f)) return -1;
    const float area = h * w;
    int a = 0;
    for (int j = 0; j < k; ++j) {
        const float ch = S.cent[j][0], cw = S.cent[j][1];
        const float ih = fminf(h, ch), iw = fminf(w, cw);
        const float inter = ih * iw;
        const float uni = (area + ch * cw) - inter;
        const float q = inter / uni;
        if (j == 0 || q > best) {
            best = q;
            a = j;
        }
    }
    return a;
}

// One assignment pass over all rows with the centroids of S.cent: afterwards (behind the barrier this ends with) S.sum_h, S.sum_w,
// S.count of every cluster, S.sum_q and S.n_valid hold the block's totals.  KA clusters are accumulated per walk over the rows;
// OUT also stores the per-row results (either pointer may be null).
template <bool VEC, int KA, bool OUT>
__device__ __forceinline__ void anchor_pass(AnchorShared& S, const float* __restrict__ sizes, long long stride, int n, int k,
                                            int* __restrict__ assign, float* __restrict__ best_iou) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int base = 0; base < k; base += KA) {
        double sh[KA], sw[KA], sq = 0.0;
        int cnt[KA], nv = 0;
#pragma unroll
        for (int j = 0; j < KA; ++j) {
            sh[j] = 0.0;
            sw[j] = 0.0;
            cnt[j] = 0;
        }
        for (long long i = tid; i < n; i += ANCHOR_THREADS) {
            float h, w, q;
            anchor_row<VEC>(sizes, stride, i, h, w);
            const int a = anchor_best(S, k, h, w, q);
            if (base == 0) {
                if (a >= 0) {
                    sq += (double)q;
                    ++nv;
                }
                if (OUT) {
                    if (assign) assign[i] = a;
                    if (best_iou) best_iou[i] = q;
                }
            }
            const int rel = a - base;
#pragma unroll
            for (int j = 0; j < KA; ++j) {                // (+ 0.0 leaves a sum of positive terms as it is)
                const bool mine = rel == j;
                sh[j] += mine ? (double)h : 0.0;
                sw[j] += mine ? (double)w : 0.0;
                cnt[j] += mine ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < KA; ++j) {
            const double th = wave_sum(sh[j]), tw = wave_sum(sw[j]);
            const int tc = wave_sum(cnt[j]);
            if (lane == 0 && base + j < k) {
                S.sh[wave][base + j] = th;
                S.sw[wave][base + j] = tw;
                S.cnt[wave][base + j] = tc;
            }
        }
        if (base == 0) {
            const double tq = wave_sum(sq);
            const int tv = wave_sum(nv);
            if (lane == 0) {
                S.q[wave] = tq;
                S.valid[wave] = tv;
            }
        }
    }
    __syncthreads();
    if (tid < k) {
        double th = 0.0, tw = 0.0;
        int tc = 0;
        for (int v = 0; v < ANCHOR_WAVES; ++v) {
            th += S.sh[v][tid];
            tw += S.sw[v][tid];
            tc += S.cnt[v][tid];
        }
        S.sum_h[tid] = th;
        S.sum_w[tid] = tw;
        S.count[tid] = tc;
    } else if (tid == 64) {                               // (another wave than the cluster totals')
        double tq = 0.0;
        int tv = 0;
        for (int v = 0; v < ANCHOR_WAVES; ++v) {
            tq += S.q[v];
            tv += S.valid[v];
        }
        S.sum_q = tq;
        S.n_valid = tv;
    }
    __syncthreads();
}

// grid (R): restart r from init[r]
template <bool VEC, int KA>
__global__ __launch_bounds__(ANCHOR_THREADS) void anchor_kmeans_kernel(const float* __restrict__ sizes, long long stride, int n,
                                                                       const float* __restrict__ init, int k, int max_iters,
                                                                       float* __restrict__ centroids, int* __restrict__ counts,
                                                                       double* __restrict__ mean_iou, int* __restrict__ iters,
                                                                       int* __restrict__ converged, int* __restrict__ n_valid) {
    __shared__ AnchorShared S;
    const int tid = threadIdx.x;
    const long long r = blockIdx.x;
    if (tid < 2 * k) S.cent[tid >> 1][tid & 1] = init[r * 2 * k + tid];
    __syncthreads();
    int done = 0, stop = 0;                               // rounds so far and S.stop as of the last barrier: every thread holds both, the exits are block-uniform
    for (;;) {
        anchor_pass<VEC, KA, false>(S, sizes, stride, n, k, nullptr, nullptr);
        if (stop == 2) break;                             // that was the pass on the centroids max_iters left
        ++done;
        if (tid == 0) {                                   // the update and the decision, by one thread
            bool same = true;
            for (int j = 0; j < k; ++j) {
                if (S.count[j] <= 0) continue;            // an empty cluster keeps its centroid
                const float nh = (float)(S.sum_h[j] / (double)S.count[j]);
                const float nw = (float)(S.sum_w[j] / (double)S.count[j]);
                same = same && __float_as_uint(nh) == __float_as_uint(S.cent[j][0]) && __float_as_uint(nw) == __float_as_uint(S.cent[j][1]);
                S.cent[j][0] = nh;
                S.cent[j][1] = nw;
            }
            S.stop = same ? 1 : (done >= max_iters ? 2 : 0);
        }
        __syncthreads();
        stop = S.stop;                                    // (written again only behind the next pass's barriers)
        if (stop == 1) break;                             // unchanged: the pass just made is the one on the returned centroids
    }
    if (tid < 2 * k) centroids[r * 2 * k + tid] = S.cent[tid >> 1][tid & 1];
    if (tid < k) counts[r * k + tid] = S.count[tid];
    if (tid == 0) {
        mean_iou[r] = S.n_valid > 0 ? S.sum_q / (double)S.n_valid : 0.0;
        iters[r] = done;
        converged[r] = stop == 1 ? 1 : 0;
        if (r == 0) *n_valid = S.n_valid;
    }
}

// grid (1)
template <bool VEC, int KA>
__global__ __launch_bounds__(ANCHOR_THREADS) void anchor_assign_kernel(const float* __restrict__ sizes, long long stride, int n,
                                                                       const float* __restrict__ cent, int k, int* __restrict__ assign,
                                                                       float* __restrict__ best_iou, int* __restrict__ counts,
                                                                       double* __restrict__ mean_iou, int* __restrict__ n_valid) {
    __shared__ AnchorShared S;
    const int tid = threadIdx.x;
    if (tid < 2 * k) S.cent[tid >> 1][tid & 1] = cent[tid];
    __syncthreads();
    anchor_pass<VEC, KA, true>(S, sizes, stride, n, k, assign, best_iou);
    if (tid < k) counts[tid] = S.count[tid];
    if (tid == 0) {
        *mean_iou = S.n_valid > 0 ? S.sum_q / (double)S.n_valid : 0.0;
        *n_valid = S.n_valid;
    }
}

static inline bool anchor_misaligned(const void* p, unsigned long long mask) { return (reinterpret_cast<unsigned long long>(p) & mask) != 0; }

static int anchor_check(const float* sizes, long long stride, int n, const float* cent, int k, const int* counts, const double* mean_iou,
                        const int* n_valid, const void* workspace) {
    if (!sizes || !cent || !counts || !mean_iou || !n_valid || !workspace) return YOLO_EINVAL;
    if (n < 1 || k < 1 || stride < 2) return YOLO_EINVAL;
    if (anchor_misaligned(sizes, 3) || anchor_misaligned(cent, 3) || anchor_misaligned(counts, 3) || anchor_misaligned(n_valid, 3) ||
        anchor_misaligned(mean_iou, 7) || anchor_misaligned(workspace, 7))
        return YOLO_EINVAL;
    return YOLO_OK;                                       // (the YOLO_EUNSUPPORTED limits come after EVERY YOLO_EINVAL condition of an entry)
}

static inline bool anchor_vec(const float* sizes, long long stride) { return stride == 2 && !anchor_misaligned(sizes, 7); }

extern "C" long long yolo_anchor_workspace_bytes(int n, int R, int k) {
    if (n < 1 || R < 1 || k < 1) return YOLO_EINVAL;
    return ANCHOR_WORKSPACE_BYTES;
}

extern "C" int yolo_anchor_assign(const float* sizes, long long stride, int n, const float* centroids, int k, int* assign, float* best_iou,
                                  int* counts, double* mean_iou, int* n_valid, void* workspace, void* stream) {
    const int rc = anchor_check(sizes, stride, n, centroids, k, counts, mean_iou, n_valid, workspace);
    if (rc != YOLO_OK) return rc;
    if (anchor_misaligned(assign, 3) || anchor_misaligned(best_iou, 3)) return YOLO_EINVAL;
    if (k > ANCHOR_MAX_K) return YOLO_EUNSUPPORTED;
    const bool vec = anchor_vec(sizes, stride);
#define ANCHOR_ASSIGN(V, KA)                                                                                                           \
    YOLO_LAUNCH((anchor_assign_kernel<V, KA>), dim3(1), dim3(ANCHOR_THREADS), 0, (hipStream_t)stream, sizes, stride, n, centroids, k, \
                assign, best_iou, counts, mean_iou, n_valid)
    if (k <= 9) {
        if (vec) ANCHOR_ASSIGN(true, 9); else ANCHOR_ASSIGN(false, 9);
    } else {
        if (vec) ANCHOR_ASSIGN(true, 16); else ANCHOR_ASSIGN(false, 16);
    }
#undef ANCHOR_ASSIGN
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_anchor_kmeans(const float* sizes, long long stride, int n, const float* init, int R, int k, int max_iters,
                                  float* centroids, int* counts, double* mean_iou, int* iters, int* converged, int* n_valid,
                                  void* workspace, void* stream) {
    if (!centroids || !iters || !converged || R < 1 || max_iters < 1) return YOLO_EINVAL;
    const int rc = anchor_check(sizes, stride, n, init, k, counts, mean_iou, n_valid, workspace);
    if (rc != YOLO_OK) return rc;
    if (anchor_misaligned(centroids, 3) || anchor_misaligned(iters, 3) || anchor_misaligned(converged, 3)) return YOLO_EINVAL;
    if (k > ANCHOR_MAX_K || R > 65535 || max_iters > 10000) return YOLO_EUNSUPPORTED;
    const bool vec = anchor_vec(sizes, stride);
#define ANCHOR_KMEANS(V, KA)                                                                                                          \
    YOLO_LAUNCH((anchor_kmeans_kernel<V, KA>), dim3(R), dim3(ANCHOR_THREADS), 0, (hipStream_t)stream, sizes, stride, n, init, k,     \
                max_iters, centroids, counts, mean_iou, iters, converged, n_valid)
    if (k <= 9) {
        if (vec) ANCHOR_KMEANS(true, 9); else ANCHOR_KMEANS(false, 9);
    } else {
        if (vec) ANCHOR_KMEANS(true, 16); else ANCHOR_KMEANS(false, 16);
    }
#undef ANCHOR_KMEANS
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
