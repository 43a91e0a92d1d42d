// Train-mode BatchNorm for gfx950: batch statistics, forward (fused with LeakyReLU and the residual add) and backward, for the
// single-plane and the split activation types.  Reference: the mxnet/gluon BatchNorm the training loop of car/YOLO.py calls
// (SURVEY App. A.3).
#include "common.h"
#include "train_access.h"

// ------------------------------------------------------------------------------------------------
// BatchNorm (train): per-channel batch statistics over (N,H,W) of an NHWC tensor (C % 8 == 0).
// Both passes are HBM-bound.  Thread = one 8-channel octet x one pixel lane of a block-owned pixel range:
// 16/32-byte coalesced accesses, BN_U independent loads in flight per thread (the first version had one and
// ran at ~0.5 TB/s -- latency-bound), per-channel constants held in registers.  Block partial sums are
// combined through LDS and added to the global sums in double.  The sums live in the caller's workspace, which
// must be zero on first use; the finalize / parameter-gradient kernels zero it again after reading (no memset
// launch per call).
// ------------------------------------------------------------------------------------------------
// channels a block of the REDUCTION covers (the apply pass covers all C): wide layers are cut into 256-channel groups
// (blockIdx.y), so that the number of blocks does not have to shrink with C to bound the atomics (C = 2048 over the
// 13x13 maps ran on 64 blocks at 0.65 TB/s)
constexpr int BN_CG = 256;

// (tests/test_gpu_large_offsets_train.py `_bn_chain` restates these constants to bound the fp32 terms a thread of the reduction adds:
//  change them there too)
static void bn_partition(long long npix, int C, int elem, bool reduces, int* ppb, unsigned* nb) {
    const int cb = (reduces && C > BN_CG) ? BN_CG : C;          // channels per block
    // (measured over the training step: 64 KB per block beats 32 / 128 KB by 0.3 / 0.4 ms; twice / four times the atomics
    // budget costs 0.6 / 1.3 ms, half of it changes nothing)
    const long long kBytes = 65536, kAtom = 131072, kMaxb = 2048;
    long long p = kBytes / ((long long)cb * elem);              // ~64 KB of one tensor per block ...
    if (p < 16) p = 16;
    // ... and a bounded number of blocks: every block of the reduction ends with 2*cb double atomics; their total
    // (2C per pixel range) dominates the small deep layers unless the number of pixel ranges shrinks with C
    long long maxb = kMaxb;
    if (reduces) {
        maxb = kAtom / C;
        if (maxb < 64) maxb = 64;
        if (maxb > kMaxb) maxb = kMaxb;
    }
    if ((npix + p - 1) / p > maxb) p = (npix + maxb - 1) / maxb;
    *ppb = (int)p;
    *nb = (unsigned)((npix + p - 1) / p);
}

// MODE 0: sums[0..C) = sum(y), sums[C..2C) = sum(y*y) -- or, with `shift`, the same sums of (y - k_c), k_c = the channel's value
//         at pixel 0: a one-pass variance from fp32 partial sums loses digits when mean^2 >> variance (0.4 % in invstd at a ratio of
//         10^6 -- a few nearly equal values, i.e. the tiny deepest maps of small inputs; found by tools/fuzz_bn.py /
//         fuzz_labels.py), and around a value of the channel itself that ratio is of order one.  The finalize adds k_c back.
// MODE 1: sums[0..C) = sum(da), sums[C..2C) = sum(da*xhat), da = dz * lrelu'(gamma*xhat+beta)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_reduce_kernel(const T* __restrict__ y, const T* __restrict__ dz,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        double* __restrict__ sums, int C, long long npix,
                                                        int pix_per_block, float slope, int shift = 0) {
    // (loads in flight per thread.  Round 4: the backward reduction 4 -> 3 and the apply passes 4 -> 2 (forward) / 3 (backward):
    //  fewer registers -- 186-204 -> 114-132 for the apply kernels -- and twice the waves per SIMD; the whole training step
    //  -1.2 % in same-box A/B runs (the isolated passes do not change: the gain is in how these HBM-bound kernels share the
    //  CUs with the side stream's weight gradients); 6 in flight: +3 %)
#ifndef YOLO_BNR_U1
#define YOLO_BNR_U1 3
#endif
    constexpr int U = MODE == 0 ? 8 : YOLO_BNR_U1;
    __shared__ float red[2][256][8];
    const int noct = C >> 3;
    const long long PS = dense_ps<T>(C);                        // pixel stride (C; split: both padded planes)
    const int LO = dense_lo<T>(C);
    const int goct = BN_CG / 8;                                 // octets of a channel group
    const int per = noct < goct ? noct : goct;                  // octets handled by this block
    const int lanes = 256 / per;                                // pixel lanes per octet in this block
    const long long p0 = (long long)blockIdx.x * pix_per_block;
    const long long p1 = min(p0 + pix_per_block, npix);
    {
        const int ob = blockIdx.y * goct;                       // first octet of this block's channel group
        const int oct = ob + (threadIdx.x % per);
        const int pl = threadIdx.x / per;
        float s[8], q[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
        if (oct < noct && pl < lanes) {
            float mu[8], is[8], g[8], b[8];
            if (MODE == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) mu[e] = shift ? load1s<T>(y + oct * 8 + e, LO) : 0.f;      // the pivots k_c
            }
            if (MODE == 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { mu[e] = mean[oct * 8 + e]; is[e] = invstd[oct * 8 + e]; g[e] = gamma[oct * 8 + e]; b[e] = beta[oct * 8 + e]; }
            }
            auto accum = [&](const float (&v)[8], const float (&d)[8]) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (MODE == 0) { const float dv = v[e] - mu[e]; s[e] += dv; q[e] += dv * dv; }
                    else {
                        const float xh = (v[e] - mu[e]) * is[e];
                        const float da = d[e] * ((g[e] * xh + b[e]) > 0.f ? 1.f : slope);
                        s[e] += da; q[e] += da * xh;
                    }
                }
            };
            const T* yp = y + oct * 8;
            const T* dp = dz + oct * 8;
            long long p = p0 + pl;
            for (; p + (long long)(U - 1) * lanes < p1; p += (long long)U * lanes) {
                float v[U][8], d[U][8];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    load8s<T>(yp + (p + (long long)u * lanes) * PS, LO, v[u]);
                    if (MODE == 1) load8s<T>(dp + (p + (long long)u * lanes) * PS, LO, d[u]);
                }
                if (MODE == 0 && IsSplit<T>::value) {
                    // Split values carry 16 significant bits, so next to a running sum of a few hundred EVERY fp32 addition is a
                    // tie or exact, and ties to an even sum all round the same way: over the hundreds of terms a thread adds on
                    // a tensor of 10^7 pixels the mean lost 5 bits (9e-7 at values of std 2 -- tests/
                    // test_gpu_large_offsets_train.py).  The U values of a step are summed on their own first: small sums, exact
                    // for such values, and an eighth of the additions into the running one.
                    float ts[8], tq[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) ts[e] = tq[e] = 0.f;
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float dv = v[u][e] - mu[e]; ts[e] += dv; tq[e] += dv * dv; }
#pragma unroll
                    for (int e = 0; e < 8; ++e) { s[e] += ts[e]; q[e] += tq[e]; }
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) accum(v[u], MODE == 1 ? d[u] : v[u]);
                }
            }
            for (; p < p1; p += lanes) {
                float v[8], d[8];
                load8s<T>(yp + p * PS, LO, v);
                if (MODE == 1) load8s<T>(dp + p * PS, LO, d);
                accum(v, MODE == 1 ? d : v);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { red[0][threadIdx.x][e] = s[e]; red[1][threadIdx.x][e] = q[e]; }
        __syncthreads();
        // 2*per*8 (quantity, octet, element) sums of `lanes` partials each, spread over the whole block
        for (int i = threadIdx.x; i < 2 * per * 8; i += 256) {
            const int e = i & 7, o = (i >> 3) % per, w = i / (per * 8);
            if (ob + o < noct) {
                double a = 0;
                for (int l = 0; l < lanes; ++l) a += red[w][l * per + o][e];
                atomicAdd(&sums[w * C + (ob + o) * 8 + e], a);
            }
        }
        __syncthreads();
    }
}

// mean / invstd (biased variance, eps) + running-stat update (momentum m: r = m*r + (1-m)*batch;
// running_var takes the BIASED batch variance -- the MXNet CPU convention).
template <typename T>
__global__ void bn_finalize_kernel(double* __restrict__ sums, float* __restrict__ mean,
                                   float* __restrict__ invstd, float* __restrict__ running_mean,
                                   float* __restrict__ running_var, int C, double inv_n, float eps, float momentum,
                                   const T* __restrict__ pivot, int pivot_lo) {   // pivot: pixel 0 of y when the sums are shifted, else NULL
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double d = sums[c] * inv_n;
    double v = sums[C + c] * inv_n - d * d;
    if (v < 0) v = 0;
    const double m = d + (pivot ? (double)load1s<T>(pivot + c, pivot_lo) : 0.0);
    mean[c] = (float)m;
    invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
    sums[c] = 0.0;                                   // leave the workspace zeroed for the next call
    sums[C + c] = 0.0;
    if (running_mean) {
        running_mean[c] = momentum * running_mean[c] + (1.f - momentum) * (float)m;
        running_var[c] = momentum * running_var[c] + (1.f - momentum) * (float)v;
    }
}

// dbeta = sum(da), dgamma = sum(da*xhat) (the apply pass divides them by the pixel count)
__global__ void bn_param_grad_kernel(double* __restrict__ sums, float* __restrict__ dgamma,
                                     float* __restrict__ dbeta, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    dbeta[c] = (float)sums[c];
    dgamma[c] = (float)sums[C + c];
    sums[c] = 0.0;
    sums[C + c] = 0.0;
}

// MODE 0 (forward):  z = lrelu(gamma*(y-mean)*invstd + beta) (+ residual)
// MODE 1 (backward): dy = gamma*invstd * (da - mean(da) - xhat*mean(da*xhat))
// Same thread <-> (octet, pixel lane) mapping as the reduction: channel constants live in registers.
// FUSED = 1: the per-layer finalize launches folded in.  The reduction's sums (double) are read by every block and turned
// into the per-channel constants on the fly with bn_finalize_kernel's / bn_param_grad_kernel's exact expressions; block 0
// also writes them out (mean / invstd / running statistics, or dgamma / dbeta) and zeroes `zero_next`, the workspace of the
// caller's NEXT BatchNorm call (callers alternate two workspaces: this call's sums stay readable until the kernel ends).
struct BnFused {
    const double* sums;       // [2C] of this call (dirty after the call)
    double* zero_next;        // [zero_n] zeroed for the next call (whose channel count may differ), or nullptr
    int zero_n;
    float* mean_out; float* invstd_out; float* running_mean; float* running_var;     // MODE 0
    float* dgamma_out; float* dbeta_out;                                             // MODE 1
    double inv_n;
    float eps, momentum;
    int shifted;              // MODE 0: the sums are of (y - y[pixel 0][c]) (bn_reduce_kernel's shift)
};

template <typename T, int MODE, int FUSED = 0>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ y, const T* __restrict__ other,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                       float inv_n, T* __restrict__ out, int C, long long npix,
                                                       int pix_per_block, float slope, BnFused f) {
    #ifndef YOLO_BN_U0
#define YOLO_BN_U0 2
#endif
#ifndef YOLO_BN_U1
#define YOLO_BN_U1 3
#endif
    constexpr int U = MODE == 0 ? YOLO_BN_U0 : YOLO_BN_U1;
    const int noct = C >> 3;
    const long long PS = dense_ps<T>(C);                        // pixel stride (C; split: both padded planes)
    const int LO = dense_lo<T>(C);
    const int per = noct < 256 ? noct : 256;
    const int lanes = 256 / per;
    const long long p0 = (long long)blockIdx.x * pix_per_block;
    const long long p1 = min(p0 + pix_per_block, npix);
    if (FUSED && blockIdx.x == 0) {
        for (int c = threadIdx.x; c < C; c += 256) {
            if (MODE == 0) {
                const double d = f.sums[c] * f.inv_n;
                double v = f.sums[C + c] * f.inv_n - d * d;
                if (v < 0) v = 0;
                const double m = d + (f.shifted ? (double)load1s<T>(y + c, LO) : 0.0);
                f.mean_out[c] = (float)m;
                f.invstd_out[c] = (float)(1.0 / sqrt(v + (double)f.eps));
                if (f.running_mean) {
                    f.running_mean[c] = f.momentum * f.running_mean[c] + (1.f - f.momentum) * (float)m;
                    f.running_var[c] = f.momentum * f.running_var[c] + (1.f - f.momentum) * (float)v;
                }
            } else {
                f.dbeta_out[c] = (float)f.sums[c];
                f.dgamma_out[c] = (float)f.sums[C + c];
            }
        }
        if (f.zero_next)
            for (int i = threadIdx.x; i < f.zero_n; i += 256) f.zero_next[i] = 0.0;
    }
    const int pl = threadIdx.x / per;
    if (pl >= lanes) return;
    for (int oct = threadIdx.x % per; oct < noct; oct += 256) {
        float sc[8], sh[8], k1[8], k2[8], mu[8], is[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = oct * 8 + e;
            if (FUSED && MODE == 0) {
                const double d = f.sums[c] * f.inv_n;
                double v = f.sums[C + c] * f.inv_n - d * d;
                if (v < 0) v = 0;
                const double m = d + (f.shifted ? (double)load1s<T>(y + c, LO) : 0.0);
                mu[e] = (float)m; is[e] = (float)(1.0 / sqrt(v + (double)f.eps));
            } else {
                mu[e] = mean[c]; is[e] = invstd[c];
            }
            sc[e] = gamma[c]; sh[e] = beta[c];
            if (MODE == 1) {
                if (FUSED) { k1[e] = 0.f; k2[e] = 0.f; }                       // (set below, k1 and k2 in loops of their own)
                else { k1[e] = dbeta[c] * inv_n; k2[e] = dgamma[c] * inv_n; }
            }
        }
        if (MODE == 1 && FUSED) {
#pragma unroll
            for (int e = 0; e < 8; ++e) k1[e] = (float)f.sums[oct * 8 + e] * inv_n;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 8; ++e) k2[e] = (float)f.sums[C + oct * 8 + e] * inv_n;
        }
        auto apply = [&](const float (&v)[8], const float (&o)[8], float (&r)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = (v[e] - mu[e]) * is[e];
                const float a = sc[e] * xh + sh[e];
                if (MODE == 0) {
                    float z = a > 0.f ? a : a * slope;
                    if (other) z += o[e];
                    r[e] = z;
                } else {
                    const float da = o[e] * (a > 0.f ? 1.f : slope);
                    r[e] = sc[e] * is[e] * (da - k1[e] - xh * k2[e]);
                }
            }
        };
        const long long co = oct * 8;
        long long p = p0 + pl;
        for (; p + (long long)(U - 1) * lanes < p1; p += (long long)U * lanes) {
            float v[U][8], o[U][8], r[8];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                load8s<T>(y + (p + (long long)u * lanes) * PS + co, LO, v[u]);
                if (other) load8s<T>(other + (p + (long long)u * lanes) * PS + co, LO, o[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                apply(v[u], other ? o[u] : v[u], r);
                store8s<T>(out + (p + (long long)u * lanes) * PS + co, LO, r);
            }
        }
        for (; p < p1; p += lanes) {
            float v[8], o[8], r[8];
            load8s<T>(y + p * PS + co, LO, v);
            if (other) load8s<T>(other + p * PS + co, LO, o);
            apply(v, other ? o : v, r);
            store8s<T>(out + p * PS + co, LO, r);
        }
    }
}

// The per-channel sums from the partial rows a convolution's statistics epilogue wrote (conv_epilogue.h, STATS):
// part [rows][2][Cp] float32 -> sums[0..C) += sum over rows of part[.][0][c], sums[C..2C) += ... part[.][1][c], in double.
// Block = 64 channels x 4 row lanes over a slice of the rows; one double atomic per (slice, channel, quantity).
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const float* __restrict__ part, int rows, int C, int Cp,
                                                              double* __restrict__ sums, int rows_per_block) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(r0 + rows_per_block, rows);
    double s = 0, q = 0;
    if (c < C) {
        int r = r0 + rl;
        for (; r + 12 < r1; r += 16) {                          // four independent loads per quantity in flight
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = part[((long long)(r + 4 * u) * 2) * Cp + c];
                b[u] = part[((long long)(r + 4 * u) * 2 + 1) * Cp + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { s += a[u]; q += b[u]; }
        }
        for (; r < r1; r += 4) { s += part[((long long)r * 2) * Cp + c]; q += part[((long long)r * 2 + 1) * Cp + c]; }
    }
    red[0][rl][cl] = s; red[1][rl][cl] = q;
    __syncthreads();
    if (threadIdx.x < 128) {
        const int w = threadIdx.x >> 6;
        const double t = red[w][0][cl] + red[w][1][cl] + red[w][2][cl] + red[w][3][cl];
        if (c < C) atomicAdd(&sums[w * C + c], t);
    }
}

static void bn_stats_finish(const float* part, int rows, int C, int Cp, double* sums, hipStream_t st) {
    const int cg = (C + 63) / 64;
    int split = (192 + cg - 1) / cg;                             // ~192 blocks
    if (split > (rows + 15) / 16) split = (rows + 15) / 16;      // at least 16 rows per block
    if (split < 1) split = 1;
    const int rpb = (rows + split - 1) / split;
    split = (rows + rpb - 1) / rpb;
    YOLO_LAUNCH(bn_stats_finish_kernel, dim3(cg, split), dim3(256), 0, st, part, rows, C, Cp, sums, rpb);
}

template <typename T>
static int bn_fwd_t(const T* y, const float* gamma, const float* beta, const T* residual, T* z, float* mean,
                    float* invstd, float* running_mean, float* running_var, double* workspace, long long npix, int C,
                    float eps, float momentum, float slope, hipStream_t st, bool fused = false, double* zero_next = nullptr, int zero_n = 0,
                    const float* part = nullptr, int part_rows = 0, int part_cp = 0) {
    (void)hipGetLastError();
    int ppb, ppa; unsigned nb, na;
    bn_partition(npix, C, value_bytes<T>(), true, &ppb, &nb);
    bn_partition(npix, C, value_bytes<T>(), false, &ppa, &na);
    if (part)       // the producing convolution already took the sums (its statistics epilogue): no pass over y
        bn_stats_finish(part, part_rows, C, part_cp, workspace, st);
    else                                                      // (shifted sums: see bn_reduce_kernel)
        YOLO_LAUNCH((bn_reduce_kernel<T, 0>), dim3(nb, (C + BN_CG - 1) / BN_CG), dim3(256), 0, st, y, (const T*)nullptr, (const float*)nullptr,
                    (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, workspace, C, npix, ppb, slope, 1);
    BnFused f = {};
    f.shifted = part ? 0 : 1;
    if (fused) {
        f.sums = workspace; f.zero_next = zero_next; f.zero_n = zero_n; f.mean_out = mean; f.invstd_out = invstd;
        f.running_mean = running_mean; f.running_var = running_var; f.inv_n = 1.0 / (double)npix; f.eps = eps; f.momentum = momentum;
        YOLO_LAUNCH((bn_apply_kernel<T, 0, 1>), dim3(na), dim3(256), 0, st, y, residual, (const float*)nullptr, (const float*)nullptr,
                    gamma, beta, (const float*)nullptr, (const float*)nullptr, 0.f, z, C, npix, ppa, slope, f);
        YOLO_LAUNCH_CHECK();
        return YOLO_OK;
    }
    YOLO_LAUNCH(bn_finalize_kernel<T>, dim3((C + 255) / 256), dim3(256), 0, st, workspace, mean, invstd, running_mean,
                running_var, C, 1.0 / (double)npix, eps, momentum, part ? (const T*)nullptr : y, dense_lo<T>(C));
    YOLO_LAUNCH((bn_apply_kernel<T, 0>), dim3(na), dim3(256), 0, st, y, residual, mean, invstd, gamma, beta,
                (const float*)nullptr, (const float*)nullptr, 0.f, z, C, npix, ppa, slope, f);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_bn_train_fwd(const void* y, const float* gamma, const float* beta, const void* residual, void* z,
                                 float* mean, float* invstd, float* running_mean, float* running_var,
                                 double* workspace, long long npix, int C, float eps, float momentum, float slope,
                                 int dtype, void* stream) {
    if (!y || !gamma || !beta || !z || !mean || !invstd || !workspace || npix <= 0 || C <= 0) return YOLO_EINVAL;
    if (C % 8) return YOLO_EUNSUPPORTED;
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        return bn_fwd_t<T>((const T*)y, gamma, beta, (const T*)residual, (T*)z, mean, invstd, running_mean, running_var, workspace,
                           npix, C, eps, momentum, slope, (hipStream_t)stream);
    });
}

template <typename T>
static int bn_bwd_t(const T* dz, const T* y, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, T* dy, float* dgamma, float* dbeta, double* workspace, long long npix, int C,
                    float slope, hipStream_t st, bool fused = false, double* zero_next = nullptr, int zero_n = 0,
                    const float* part = nullptr, int part_rows = 0, int part_cp = 0) {
    (void)hipGetLastError();
    int ppb, ppa; unsigned nb, na;
    bn_partition(npix, C, value_bytes<T>(), true, &ppb, &nb);
    bn_partition(npix, C, value_bytes<T>(), false, &ppa, &na);
    if (part)       // the data gradient that produced dz already took sum(da), sum(da * xhat): no pass over dz and y
        bn_stats_finish(part, part_rows, C, part_cp, workspace, st);
    else
        YOLO_LAUNCH((bn_reduce_kernel<T, 1>), dim3(nb, (C + BN_CG - 1) / BN_CG), dim3(256), 0, st, y, dz, mean, invstd, gamma, beta, workspace, C,
                    npix, ppb, slope);
    BnFused f = {};
    if (fused) {
        f.sums = workspace; f.zero_next = zero_next; f.zero_n = zero_n; f.dgamma_out = dgamma; f.dbeta_out = dbeta;
        YOLO_LAUNCH((bn_apply_kernel<T, 1, 1>), dim3(na), dim3(256), 0, st, y, dz, mean, invstd, gamma, beta,
                    (const float*)nullptr, (const float*)nullptr, (float)(1.0 / (double)npix), dy, C, npix, ppa, slope, f);
        YOLO_LAUNCH_CHECK();
        return YOLO_OK;
    }
    YOLO_LAUNCH(bn_param_grad_kernel, dim3((C + 255) / 256), dim3(256), 0, st, workspace, dgamma, dbeta, C);
    YOLO_LAUNCH((bn_apply_kernel<T, 1>), dim3(na), dim3(256), 0, st, y, dz, mean, invstd, gamma, beta,
                (const float*)dgamma, (const float*)dbeta, (float)(1.0 / (double)npix), dy, C, npix, ppa, slope, f);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_bn_train_bwd(const void* dz, const void* y, const float* mean, const float* invstd,
                                 const float* gamma, const float* beta, void* dy, float* dgamma, float* dbeta,
                                 double* workspace, long long npix, int C, float slope, int dtype, void* stream) {
    if (!dz || !y || !mean || !invstd || !gamma || !beta || !dy || !dgamma || !dbeta || !workspace) return YOLO_EINVAL;
    if (npix <= 0 || C <= 0) return YOLO_EINVAL;
    if (C % 8) return YOLO_EUNSUPPORTED;
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        return bn_bwd_t<T>((const T*)dz, (const T*)y, mean, invstd, gamma, beta, (T*)dy, dgamma, dbeta, workspace, npix, C, slope,
                           (hipStream_t)stream);
    });
}

// The same two calls with the per-layer finalize launches folded into the apply pass (bn_apply_kernel<.., FUSED = 1>): two
// launches per call instead of three.  `workspace` (2*C doubles) must be ZERO on entry and is left dirty; `zero_next`
// (a different buffer of zero_next_count doubles -- the NEXT call may have more channels --, or NULL) is zeroed for the
// caller's next BatchNorm call: callers alternate two workspaces.
extern "C" int yolo_bn_train_fwd_pp(const void* y, const float* gamma, const float* beta, const void* residual, void* z,
                                    float* mean, float* invstd, float* running_mean, float* running_var,
                                    double* workspace, double* zero_next, int zero_next_count, long long npix, int C,
                                    float eps, float momentum, float slope, int dtype, void* stream) {
    if (!y || !gamma || !beta || !z || !mean || !invstd || !workspace || npix <= 0 || C <= 0 || workspace == zero_next || zero_next_count < 0) return YOLO_EINVAL;
    // no aliasing: EVERY block of the fused apply pass re-reads y at pixel 0 (the pivot of the shifted sums) to rebuild the mean
    // while the block that owns pixel 0 writes z -- with z == y that is a cross-block race (the three-launch yolo_bn_train_fwd
    // reads the pivot in its finalize launch, before the apply pass, and is safe in place)
    if (z == y) return YOLO_EINVAL;
    if (C % 8) return YOLO_EUNSUPPORTED;
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        return bn_fwd_t<T>((const T*)y, gamma, beta, (const T*)residual, (T*)z, mean, invstd, running_mean, running_var, workspace,
                           npix, C, eps, momentum, slope, (hipStream_t)stream, true, zero_next, zero_next_count);
    });
}

extern "C" int yolo_bn_train_bwd_pp(const void* dz, const void* y, const float* mean, const float* invstd,
                                    const float* gamma, const float* beta, void* dy, float* dgamma, float* dbeta,
                                    double* workspace, double* zero_next, int zero_next_count, long long npix, int C,
                                    float slope, int dtype, void* stream) {
    if (!dz || !y || !mean || !invstd || !gamma || !beta || !dy || !dgamma || !dbeta || !workspace || workspace == zero_next || zero_next_count < 0) return YOLO_EINVAL;
    if (npix <= 0 || C <= 0) return YOLO_EINVAL;
    if (C % 8) return YOLO_EUNSUPPORTED;
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        return bn_bwd_t<T>((const T*)dz, (const T*)y, mean, invstd, gamma, beta, (T*)dy, dgamma, dbeta, workspace, npix, C, slope,
                           (hipStream_t)stream, true, zero_next, zero_next_count);
    });
}

// yolo_bn_train_fwd_pp / _bwd_pp with the reduction pass replaced by the partial rows of a convolution's statistics
// epilogue (yolo_conv_desc.stats; rows = yolo_conv_stats_rows(), cout_pad = yolo_padded_channels(C)); bf16 only.
extern "C" int yolo_bn_train_fwd_partials(const float* partials, int rows, int cout_pad, const void* y, const float* gamma,
                                          const float* beta, const void* residual, void* z, float* mean, float* invstd,
                                          float* running_mean, float* running_var, double* workspace, double* zero_next,
                                          int zero_next_count, long long npix, int C, float eps, float momentum, float slope,
                                          int dtype, void* stream) {
    if (!partials || rows <= 0 || cout_pad < C || !y || !gamma || !beta || !z || !mean || !invstd || !workspace || npix <= 0 ||
        C <= 0 || workspace == zero_next || zero_next_count < 0) return YOLO_EINVAL;
    if ((C % 8) || dtype != YOLO_BF16) return YOLO_EUNSUPPORTED;
    return bn_fwd_t<bf16_t>((const bf16_t*)y, gamma, beta, (const bf16_t*)residual, (bf16_t*)z, mean, invstd, running_mean,
                            running_var, workspace, npix, C, eps, momentum, slope, (hipStream_t)stream, true, zero_next,
                            zero_next_count, partials, rows, cout_pad);
}

extern "C" int yolo_bn_train_bwd_partials(const float* partials, int rows, int cout_pad, const void* dz, const void* y,
                                          const float* mean, const float* invstd, const float* gamma, const float* beta,
                                          void* dy, float* dgamma, float* dbeta, double* workspace, double* zero_next,
                                          int zero_next_count, long long npix, int C, float slope, int dtype, void* stream) {
    if (!partials || rows <= 0 || cout_pad < C || !dz || !y || !mean || !invstd || !gamma || !beta || !dy || !dgamma || !dbeta ||
        !workspace || workspace == zero_next || zero_next_count < 0 || npix <= 0 || C <= 0) return YOLO_EINVAL;
    if ((C % 8) || dtype != YOLO_BF16) return YOLO_EUNSUPPORTED;
    return bn_bwd_t<bf16_t>((const bf16_t*)dz, (const bf16_t*)y, mean, invstd, gamma, beta, (bf16_t*)dy, dgamma, dbeta, workspace,
                            npix, C, slope, (hipStream_t)stream, true, zero_next, zero_next_count, partials, rows, cout_pad);
}
