// The DenseNet bodies' TRAIN-MODE forward: BatchNorm with the batch's statistics (include/yolo_amd.h, "DenseNet bodies, train-mode
// forward").  The inference kernels of dense.hip are launched unchanged with (scale, bias) pairs folded from BATCH statistics; this
// unit only measures those statistics and folds them:
//   * a block's feature map is one buffer and a channel's statistics are fixed the moment it is written, so every BN1 of a block is
//     a fold of the block's per-channel (mean, var) with its own gamma and beta: yolo_dense_channel_stats measures channels as stored;
//   * BN2 normalises the bottleneck m = W1 relu(bn1(x)), which the fused layer kernel never stores: yolo_dense_bottleneck_stats
//     forms m exactly as stage 1 of dense_layer_kernel does (dense_mma.h: the same loads, select, rounding and MFMA chain per
//     accumulator) and reduces it without storing it;
//   * the stem's BN normalises the raw 7x7 convolution: yolo_dense_stem_stats repeats dense_stem_kernel's fmaf chain per output.
// Every reduction is deterministic: a block adds its values in double in a fixed order and writes ONE partial row (sum, sum of
// squares per channel) to the workspace; a finishing launch of one block adds the rows in a fixed order, writes mean and biased
// variance, and -- given a yolo_bn_batch_fold -- folds a BatchNorm from them with yolo_fold_bn's arithmetic and updates its running
// statistics.  No atomics; every row the finishing launch reads was written by the launch before it, so the workspace needs no zeroing.
#include "common.h"
#include "dense_mma.h"

namespace {
constexpr int MT_MAX = 8;                        // Cm <= 128
constexpr int ROWS_MAX = YOLO_DENSE_STATS_ROWS;  // partial rows of one reduction

struct FoldArgs {
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* scale;
    float* bias;
    int C, Cpad;
    float eps, momentum;
};

template <typename T> __device__ __forceinline__ float load1(const char* p);
template <> __device__ __forceinline__ float load1<bf16_t>(const char* p) { return bf16_bits_to_f32(*(const uint16_t*)p); }
template <> __device__ __forceinline__ float load1<float>(const char* p) { return *(const float*)p; }

__device__ __forceinline__ double wave_sum16(double x) {      // over the 16 lanes that share lane >> 4, the same bits in each
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off);
    return x;
}
}  // namespace

// ---- finishing: rows -> mean, biased variance [-> folded BatchNorm, running statistics] -----------------------------------------------
// rows: [R][2][n] doubles, or NULL (fold only).  Thread (s = tid / 32, j = tid % 32) adds rows s, s + 8, ... of channel j of a 32-channel
// chunk, thread (0, j) the eight sums in index order.
__global__ __launch_bounds__(256) void dense_stats_finish_kernel(const double* rows, int R, int n, int c0, double count, float* mean,
                                                                 float* var, FoldArgs f) {
    __shared__ double part[2][8][32];
    const int tid = threadIdx.x, j = tid & 31, s = tid >> 5;
    if (rows) {
        for (int cb = 0; cb < n; cb += 32) {
            const int c = cb + j;
            double a = 0.0, q = 0.0;
            if (c < n)
                for (int r = s; r < R; r += 8) {
                    a += rows[(2 * r) * n + c];
                    q += rows[(2 * r + 1) * n + c];
                }
            part[0][s][j] = a;
            part[1][s][j] = q;
            __syncthreads();
            if (s == 0 && c < n) {
                double S = 0.0, Q = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) { S += part[0][k][j]; Q += part[1][k][j]; }
                const double m = S / count;
                double v = Q / count - m * m;
                if (v < 0) v = 0;
                mean[c0 + c] = (float)m;
                var[c0 + c] = (float)v;
            }
            __syncthreads();
        }
    }
    if (!f.scale) return;
    __threadfence_block();                        // the fold reads what this block has just written
    __syncthreads();
    for (int c = tid; c < f.Cpad; c += 256) {
        float sc = 0.f, b = 0.f;
        if (c < f.C) {
            const float m = mean[c], v = var[c];
            sc = f.gamma[c] / sqrtf(v + f.eps);    // yolo_fold_bn's arithmetic
            b = f.beta[c] - m * sc;
            if (f.running_mean) {                  // Gluon: running_var takes the biased variance (yolo_bn_train_fwd)
                f.running_mean[c] = f.momentum * f.running_mean[c] + (1.f - f.momentum) * m;
                f.running_var[c] = f.momentum * f.running_var[c] + (1.f - f.momentum) * v;
            }
        }
        f.scale[c] = sc;
        f.bias[c] = b;
    }
}

// ---- the bottleneck's statistics ----------------------------------------------------------------------------------------------------
// A wave takes 32 consecutive pixels per step as two groups of 16 (one A fragment serves both, as in dense_layer_kernel); a lane ends
// up with channels 16 m + 4 (lane >> 4) + i of pixel lane & 15 and adds them, and their squares, to doubles of its own.  After the last
// step the 16 pixel lanes are added by a butterfly, the four waves through LDS in wave order.
struct BStatsArgs {
    const char* buf;
    const char* w1;
    const float* s1;
    const float* t1;
    double* rows;
    long long P;
    int Cs, Cin, Cm, iters;
};

template <typename T>
__global__ __launch_bounds__(256) void dense_bottleneck_stats_kernel(BStatsArgs a) {
    constexpr int ES = sizeof(T);
    __shared__ double red[4][2][MT_MAX * 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int MT = a.Cm / 16, KC = (a.Cin + 31) / 32;
    double ds[MT_MAX][4], dq[MT_MAX][4];
#pragma unroll
    for (int m = 0; m < MT_MAX; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) ds[m][i] = dq[m][i] = 0.0;
    for (int it = 0; it < a.iters; ++it) {
        const long long base = (((long long)it * gridDim.x + blockIdx.x) * 4 + wave) * 32;
        if (base >= a.P) break;                           // (wave-uniform)
        const bool g1 = base + 16 < a.P;
        bool in[2];
        const char* px[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const long long pi = base + p * 16 + r;
            in[p] = pi < a.P;
            px[p] = a.buf + pi * a.Cs * ES;
        }
        f32x4 acc[2][MT_MAX];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m) acc[p][m] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < KC; ++kc) {
            const int c0 = kc * 32 + q * 8;
            Frag<T> b[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                b[p].zero();
                if (in[p]) {                                // (a pixel past the last one is not loaded and counts for nothing below)
                    float f[8];
                    b[p].load(px[p] + c0 * ES);
                    b[p].unpack(f);
                    bn_relu8(f, a.s1, a.t1, c0, a.Cin);
                    b[p].pack(f);
                }
            }
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m) {
                if (m < MT) {
                    Frag<T> w;
                    w.load(a.w1 + ((long long)(m * KC + kc) * 64 + lane) * 8 * ES);
                    acc[0][m] = mma(w, b[0], acc[0][m]);
                    if (g1) acc[1][m] = mma(w, b[1], acc[1][m]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m)
                if (m < MT) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double v = in[p] ? (double)acc[p][m][i] : 0.0;
                        ds[m][i] += v;
                        dq[m][i] += v * v;
                    }
                }
    }
#pragma unroll
    for (int m = 0; m < MT_MAX; ++m)
        if (m < MT) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double S = wave_sum16(ds[m][i]), Q = wave_sum16(dq[m][i]);
                if (r == 0) {
                    red[wave][0][m * 16 + q * 4 + i] = S;
                    red[wave][1][m * 16 + q * 4 + i] = Q;
                }
            }
        }
    __syncthreads();
    if (tid < a.Cm) {
        double* row = a.rows + (long long)blockIdx.x * 2 * a.Cm;
        row[tid] = ((red[0][0][tid] + red[1][0][tid]) + red[2][0][tid]) + red[3][0][tid];
        row[a.Cm + tid] = ((red[0][1][tid] + red[1][1][tid]) + red[2][1][tid]) + red[3][1][tid];
    }
}

// ---- the statistics of channels [c0, c0 + n) of a block buffer, as stored -------------------------------------------------------------
// cw (8, 16, 32 or 64; 64 whenever n > 64) consecutive threads take consecutive channels of one pixel, the block 256 / cw pixels per
// step; a thread adds its pixels in pixel order, thread (0, j) the 256 / cw pixel slots of channel j in slot order.
template <typename T>
__global__ __launch_bounds__(256) void dense_channel_stats_kernel(const char* buf, double* rows, long long P, int Cs, int c0, int n, int cw,
                                                                  int iters) {
    constexpr int ES = sizeof(T);
    __shared__ double red[2][256];
    const int tid = threadIdx.x, j = tid % cw, s = tid / cw, ppb = 256 / cw;
    for (int cb = 0; cb < n; cb += cw) {
        const int c = cb + j;
        double a = 0.0, q = 0.0;
        if (c < n)
            for (int it = 0; it < iters; ++it) {
                const long long p = ((long long)it * gridDim.x + blockIdx.x) * ppb + s;
                if (p >= P) break;
                const double v = (double)load1<T>(buf + (p * Cs + c0 + c) * ES);
                a += v;
                q += v * v;
            }
        red[0][tid] = a;
        red[1][tid] = q;
        __syncthreads();
        if (tid < cw && c < n) {
            double S = 0.0, Q = 0.0;
            for (int k = 0; k < ppb; ++k) { S += red[0][k * cw + j]; Q += red[1][k * cw + j]; }
            double* row = rows + (long long)blockIdx.x * 2 * n;
            row[c] = S;
            row[n + c] = Q;
        }
        __syncthreads();
    }
}

// ---- the statistics of the stem's raw convolution -----------------------------------------------------------------------------------------
// A block walks 16 x 16 tiles of convolution outputs for 8 channels, one output per thread: the 37 x 37 x 3 input patch and the 8
// filters live in LDS; per output the products and their order are dense_stem_kernel's (fmaf over c, ky, kx from 0).
constexpr int ST = 16, STP = 2 * (ST - 1) + 7, STPW = STP + 1;
__global__ __launch_bounds__(256) void dense_stem_stats_kernel(const float* x, const float* w, double* rows, int H, int W, int Hc, int Wc,
                                                               int tiles_x, int tiles, int items, int iters, int F0) {
    __shared__ float patch[3 * STP * STPW];
    __shared__ float wl[8 * 147];
    __shared__ double red[4][2][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int co0 = blockIdx.y * 8;
    const int ly = tid >> 4, lx = tid & 15;
    for (int i = tid; i < 8 * 147; i += 256) wl[i] = w[(long long)co0 * 147 + i];
    double ds[8], dq[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) ds[o] = dq[o] = 0.0;
    for (int it = 0; it < iters; ++it) {
        const long long item = (long long)it * gridDim.x + blockIdx.x;
        if (item >= items) break;                           // (block-uniform)
        const int n = (int)(item / tiles), t = (int)(item % tiles);
        const int cy0 = (t / tiles_x) * ST, cx0 = (t % tiles_x) * ST;
        const float* img = x + (long long)n * 3 * H * W;
        __syncthreads();                                    // the step before has read its patch
        for (int i = tid; i < 3 * STP * STP; i += 256) {
            const int c = i / (STP * STP), py = i / STP % STP, px = i % STP;
            const int iy = 2 * cy0 - 3 + py, ix = 2 * cx0 - 3 + px;
            patch[(c * STP + py) * STPW + px] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? img[((long long)c * H + iy) * W + ix] : 0.f;
        }
        __syncthreads();
        if (cy0 + ly < Hc && cx0 + lx < Wc) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int c = 0; c < 3; ++c)
#pragma unroll 1
                for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const float v = patch[(c * STP + 2 * ly + ky) * STPW + 2 * lx + kx];
                        const int k = (c * 7 + ky) * 7 + kx;
#pragma unroll
                        for (int o = 0; o < 8; ++o) acc[o] = fmaf(v, wl[o * 147 + k], acc[o]);
                    }
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const double v = (double)acc[o];
                ds[o] += v;
                dq[o] += v * v;
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        double S = ds[o], Q = dq[o];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { S += __shfl_xor(S, off); Q += __shfl_xor(Q, off); }
        if (lane == 0) { red[wave][0][o] = S; red[wave][1][o] = Q; }
    }
    __syncthreads();
    if (tid < 8) {
        double* row = rows + (long long)blockIdx.x * 2 * F0;
        row[co0 + tid] = ((red[0][0][tid] + red[1][0][tid]) + red[2][0][tid]) + red[3][0][tid];
        row[F0 + co0 + tid] = ((red[0][1][tid] + red[1][1][tid]) + red[2][1][tid]) + red[3][1][tid];
    }
}

// ---- entries ------------------------------------------------------------------------------------------------------------------------
static int fold_args(const yolo_bn_batch_fold* fold, FoldArgs* f) {
    *f = FoldArgs{};
    if (!fold) return YOLO_OK;
    if (!fold->gamma || !fold->beta || !fold->scale || !fold->bias || fold->C <= 0) return YOLO_EINVAL;
    if ((fold->running_mean == nullptr) != (fold->running_var == nullptr)) return YOLO_EINVAL;
    if (!(fold->eps > 0.f) || !(fold->momentum >= 0.f && fold->momentum <= 1.f)) return YOLO_EINVAL;
    *f = FoldArgs{fold->gamma, fold->beta, fold->running_mean, fold->running_var, fold->scale, fold->bias, fold->C,
                  round_up(fold->C, YOLO_COUT_PAD), fold->eps, fold->momentum};
    return YOLO_OK;
}

static inline int blocks_for(long long work, long long per_block) {
    const long long b = (work + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > ROWS_MAX ? ROWS_MAX : b);
}

extern "C" long long yolo_dense_stats_workspace_bytes(int channels) {
    if (channels <= 0) return YOLO_EINVAL;
    return (long long)ROWS_MAX * 2 * channels * (long long)sizeof(double);
}

extern "C" int yolo_dense_bn_batch_fold(const float* mean, const float* var, const yolo_bn_batch_fold* fold, void* stream) {
    if (!mean || !var || !fold) return YOLO_EINVAL;
    FoldArgs f;
    if (int rc = fold_args(fold, &f)) return rc;
    YOLO_LAUNCH(dense_stats_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)nullptr, 0, 0, 0, 1.0,
                const_cast<float*>(mean), const_cast<float*>(var), f);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_dense_bottleneck_stats(const void* buf, const void* w1_image, const float* scale1, const float* bias1, float* mean,
                                           float* var, void* workspace, const yolo_bn_batch_fold* fold, int N, int H, int W, int Cs,
                                           int Cin, int Cm, int dtype, void* stream) {
    if (!buf || !w1_image || !scale1 || !bias1 || !mean || !var || !workspace) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || Cs <= 0 || Cin <= 0 || Cm <= 0) return YOLO_EINVAL;
    if (!dtype_valid(dtype)) return YOLO_EINVAL;
    FoldArgs f;
    if (int rc = fold_args(fold, &f)) return rc;
    if (dtype != YOLO_BF16 && dtype != YOLO_F32) return YOLO_EUNSUPPORTED;
    if ((Cm % 16) || Cm > 16 * MT_MAX || Cin < 8 || (Cs % 32) || Cin > Cs) return YOLO_EUNSUPPORTED;
    if (fold && fold->C != Cm) return YOLO_EUNSUPPORTED;
    const int es = elem_size(dtype);
    if (too_large((long long)N * H * W * Cs, es)) return YOLO_EUNSUPPORTED;
    const long long P = (long long)N * H * W;
    const int R = blocks_for(P, 128);
    BStatsArgs a{(const char*)buf, (const char*)w1_image, scale1, bias1, (double*)workspace, P, Cs, Cin, Cm,
                 (int)((P + 128LL * R - 1) / (128LL * R))};
    if (dtype == YOLO_BF16) YOLO_LAUNCH(dense_bottleneck_stats_kernel<bf16_t>, dim3(R), dim3(256), 0, (hipStream_t)stream, a);
    else YOLO_LAUNCH(dense_bottleneck_stats_kernel<float>, dim3(R), dim3(256), 0, (hipStream_t)stream, a);
    YOLO_LAUNCH_CHECK();
    YOLO_LAUNCH(dense_stats_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, R, Cm, 0, (double)P, mean,
                var, f);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_dense_channel_stats(const void* buf, float* mean, float* var, void* workspace, const yolo_bn_batch_fold* fold, int N,
                                        int H, int W, int Cs, int c0, int n, int dtype, void* stream) {
    if (!buf || !mean || !var || !workspace) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || Cs <= 0 || c0 < 0 || n <= 0) return YOLO_EINVAL;
    if (!dtype_valid(dtype)) return YOLO_EINVAL;
    FoldArgs f;
    if (int rc = fold_args(fold, &f)) return rc;
    if (dtype != YOLO_BF16 && dtype != YOLO_F32) return YOLO_EUNSUPPORTED;
    if ((long long)c0 + n > Cs) return YOLO_EUNSUPPORTED;
    const int es = elem_size(dtype);
    if (too_large((long long)N * H * W * Cs, es)) return YOLO_EUNSUPPORTED;
    const long long P = (long long)N * H * W;
    int cw = 8;
    while (cw < n && cw < 64) cw *= 2;
    const int ppb = 256 / cw, R = blocks_for(P, ppb);
    const int iters = (int)((P + (long long)ppb * R - 1) / ((long long)ppb * R));
    if (dtype == YOLO_BF16)
        YOLO_LAUNCH(dense_channel_stats_kernel<bf16_t>, dim3(R), dim3(256), 0, (hipStream_t)stream, (const char*)buf, (double*)workspace, P, Cs,
                    c0, n, cw, iters);
    else
        YOLO_LAUNCH(dense_channel_stats_kernel<float>, dim3(R), dim3(256), 0, (hipStream_t)stream, (const char*)buf, (double*)workspace, P, Cs,
                    c0, n, cw, iters);
    YOLO_LAUNCH_CHECK();
    YOLO_LAUNCH(dense_stats_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, R, n, c0, (double)P, mean,
                var, f);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_dense_stem_stats(const float* x_nchw, const float* w_oihw, float* mean, float* var, void* workspace,
                                     const yolo_bn_batch_fold* fold, int N, int H, int W, int F0, void* stream) {
    if (!x_nchw || !w_oihw || !mean || !var || !workspace) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || F0 <= 0) return YOLO_EINVAL;
    FoldArgs f;
    if (int rc = fold_args(fold, &f)) return rc;
    if ((F0 % 8) || F0 > 64) return YOLO_EUNSUPPORTED;
    if (fold && fold->C != F0) return YOLO_EUNSUPPORTED;
    if (too_large((long long)N * 3 * H * W, 4)) return YOLO_EUNSUPPORTED;
    const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1;             // floor((n + 6 - 7) / 2) + 1
    const int tiles_x = (Wc + ST - 1) / ST, tiles = tiles_x * ((Hc + ST - 1) / ST);
    const long long items = (long long)N * tiles;
    if (items >= (1LL << 31)) return YOLO_EUNSUPPORTED;
    const int R = blocks_for(items, 1);
    YOLO_LAUNCH(dense_stem_stats_kernel, dim3(R, F0 / 8), dim3(256), 0, (hipStream_t)stream, x_nchw, w_oihw, (double*)workspace, H, W, Hc, Wc,
                tiles_x, tiles, (int)items, (int)((items + R - 1) / R), F0);
    YOLO_LAUNCH_CHECK();
    YOLO_LAUNCH(dense_stats_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, R, F0, 0,
                (double)N * Hc * Wc, mean, var, f);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
