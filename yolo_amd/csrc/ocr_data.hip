// The OCR reader's labelled data on the device for gfx950: LPGenerator.render (licence_plate_render/__init__.py:168-214), loss_mask
// (OCR/OCR.py:77-100), the two losses of train_the (OCR/OCR.py:103-119, 264-265) and the bookkeeping of the valid mode
// (OCR/OCR.py:301-343).  The host decides (yolo_amd/render.py LPGenerator.draw_ocr_params); the kernels here do the pixels and sums:
//   ocr_blur_kernel     Q of the paste rectangle: the plate through the row's affine map, a separable Gaussian of up to 24 taps
//                       per side through the LDS, the noise; Q goes to the workspace with each tile's colour sums (double)
//   ocr_blend_kernel    mean colour from the tile sums, colour map, blend over the 0..255 (or 0..1) background, clip
//   ocr_targets_kernel  loss_mask: one thread per (image, column) takes the last label that covers it
//   ocr_loss_kernel     logistic loss of the score column, score-weighted softmax cross-entropy of the class columns, d/dlogits
//   ocr_score_kernel    per image: truth and predicted text lengths, their Levenshtein distance, column accuracy counts
// Compiled with -ffp-contract=off: the arithmetic is the op-by-op fp32 definition of include/yolo_amd.h, which tests/ocr_render_ref.py
// and tests/ocr_loss_ref.py restate.  The row, the sample S and the noise are plates.hip's (plate_row.h).
#include "plate_row.h"

constexpr int OCR_THREADS = 256;
constexpr int OCR_TILE = 32;                               // a block makes a 32 x 32 tile of Q
constexpr int OCR_TMAX = YOLO_OCR_BLUR_TAPS;               // taps per side
constexpr int OCR_SPAN = OCR_TILE + 2 * OCR_TMAX;          // 80: the tile with its halo
constexpr int OCR_CHUNK = 8;                               // rows sampled at a time
static_assert(OCR_TMAX + 2 <= YOLO_OCR_TAP_WORDS, "T and w[0..T] fit the tap row");
static_assert(OCR_CHUNK * OCR_TILE == OCR_THREADS, "one horizontal sum per thread and chunk");

static bool misaligned(const void* p, unsigned long long mask) { return (reinterpret_cast<unsigned long long>(p) & mask) != 0; }

static long long ocr_tiles(int H, int W) { return (long long)((H + OCR_TILE - 1) / OCR_TILE) * ((W + OCR_TILE - 1) / OCR_TILE); }
// the workspace: N * tiles * 3 doubles (tile sums), padded to 16 bytes, then N * H * W float4 (Q)
static long long ocr_q_offset(int N, int H, int W) { return round_up_ll((long long)N * ocr_tiles(H, W) * 3 * (long long)sizeof(double), 16); }

struct OcrWindow {
    int l, t, r, b;
};
__device__ __forceinline__ OcrWindow ocr_window(const PlateRow& R, int H, int W) {       // clipped to the canvas whatever the row holds
    return OcrWindow{max(R.l, 0), max(R.t, 0), min(R.r, W), min(R.b, H)};
}

// grid (tiles across, tiles down, images).  LDS: hbuf 80 x 32 float4 (40960 B) + sbuf 8 x 80 float4 (10240 B) + 25 weights = 51300 B,
// so three blocks (twelve waves) per compute unit: three waves per SIMD.  The tile's rows with their halo are sampled eight at a time into
// sbuf, summed along the row into hbuf, and when all rows are there summed down the columns.  T is uniform over the block.
__global__ __launch_bounds__(OCR_THREADS) void ocr_blur_kernel(const unsigned char* __restrict__ plates, const PlateRow* __restrict__ rows,
                                                               const int* __restrict__ taps, double* __restrict__ partial,
                                                               float4* __restrict__ Qws, int H, int W) {
    __shared__ float4 hbuf[OCR_SPAN * OCR_TILE];
    __shared__ float4 sbuf[OCR_CHUNK * OCR_SPAN];
    __shared__ float wgt[OCR_TMAX + 1];
    const long long n = blockIdx.z;
    const int tid = threadIdx.x;
    const long long tile = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    double* psum = partial + (n * ((long long)gridDim.x * gridDim.y) + tile) * 3;
    const PlateRow& R = rows[n];
    const OcrWindow win = ocr_window(R, H, W);
    const int j0 = blockIdx.x * OCR_TILE, i0 = blockIdx.y * OCR_TILE;
    // (block-uniform) a tile without a pixel of the window, or an image without a plate: its sums are 0, nothing else is written
    if (!plate_ok(R) || j0 >= win.r || j0 + OCR_TILE <= win.l || i0 >= win.b || i0 + OCR_TILE <= win.t) {
        if (tid < 3) psum[tid] = 0.0;
        return;
    }
    const int* tp = taps + n * YOLO_OCR_TAP_WORDS;
    const int T = min(max(tp[0], 0), OCR_TMAX);
    if (tid <= OCR_TMAX) wgt[tid] = (T == 0) ? 1.f : (tid <= T ? __int_as_float(tp[1 + tid]) : 0.f);
    const unsigned char* plate = plates + n * (4LL * PLATE_H * PLATE_W);
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = R.m[k];
    const int span_w = OCR_TILE + 2 * T, span_h = OCR_TILE + 2 * T;
    __syncthreads();
    for (int y0 = 0; y0 < span_h; y0 += OCR_CHUNK) {
        const int nrow = min(OCR_CHUNK, span_h - y0);
        for (int q = tid; q < nrow * span_w; q += OCR_THREADS) {
            const int r = q / span_w, x = q - r * span_w;
            float val[4];
            plate_sample(plate, m, (float)(j0 - T + x), (float)(i0 - T + y0 + r), val);
            sbuf[r * OCR_SPAN + x] = make_float4(val[0], val[1], val[2], val[3]);
        }
        __syncthreads();
        {
            const int r = tid / OCR_TILE, col = tid % OCR_TILE;
            if (r < nrow) {
                // taps -T..T in ascending order: sbuf column col + T + k is canvas column j0 + col + k
                const float4* s = sbuf + r * OCR_SPAN + col;
                const float w = wgt[T];
                float4 a = s[0];
                a = make_float4(w * a.x, w * a.y, w * a.z, w * a.w);
                for (int k = 1; k <= 2 * T; ++k) {
                    const float wk = wgt[abs(k - T)];
                    const float4 v = s[k];
                    a = make_float4(a.x + wk * v.x, a.y + wk * v.y, a.z + wk * v.z, a.w + wk * v.w);
                }
                hbuf[(y0 + r) * OCR_TILE + col] = a;
            }
        }
        __syncthreads();
    }
    double acc[3] = {0.0, 0.0, 0.0};
    {
        const int col = tid % OCR_TILE, j = j0 + col;
        const float s = R.s;
#pragma unroll 1
        for (int rr = 0; rr < OCR_TILE / OCR_CHUNK; ++rr) {
            const int row = tid / OCR_TILE + OCR_CHUNK * rr, i = i0 + row;
            if (j < win.l || j >= win.r || i < win.t || i >= win.b) continue;
            const float4* hcol = hbuf + row * OCR_TILE + col;             // hbuf row `row + T + k` is canvas row i + k
            const float w = wgt[T];
            float4 a = hcol[0];
            float q[4] = {w * a.x, w * a.y, w * a.z, w * a.w};
            for (int k = 1; k <= 2 * T; ++k) {
                const float wk = wgt[abs(k - T)];
                const float4 v = hcol[k * OCR_TILE];
                q[0] = q[0] + wk * v.x;
                q[1] = q[1] + wk * v.y;
                q[2] = q[2] + wk * v.z;
                q[3] = q[3] + wk * v.w;
            }
            if (s != 0.f) plate_noise(q, j, i, s, R.k0, R.k1);
            Qws[(n * H + i) * (long long)W + j] = make_float4(q[0], q[1], q[2], q[3]);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += (double)q[c];
        }
    }
    __syncthreads();                                                      // sbuf is free: the tree of the tile's sums lives there
    double* red = reinterpret_cast<double*>(sbuf);
    static_assert(sizeof(sbuf) >= 3 * OCR_THREADS * sizeof(double), "the reduction fits sbuf");
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c * OCR_THREADS + tid] = acc[c];
    __syncthreads();
    for (int st = OCR_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c * OCR_THREADS + tid] += red[c * OCR_THREADS + tid + st];
        }
        __syncthreads();
    }
    if (tid < 3) psum[tid] = red[tid * OCR_THREADS];
}

// grid (ceil(H * G / 256), images), G = ceil(W / 4): thread q of an image makes row q / G, columns 4 (q % G)..+3 of the three planes.
// bg and out may be one buffer (no __restrict__ on them): a thread reads its 12 values before it writes them.
template <bool VEC>
__global__ __launch_bounds__(OCR_THREADS) void ocr_blend_kernel(const float* bg, const PlateRow* __restrict__ rows, const double* __restrict__ partial,
                                                                const float4* __restrict__ Qws, float* out, int H, int W, int G, int tiles,
                                                                int bg_unit) {
    __shared__ float kk[3];
    const long long n = blockIdx.y;
    const PlateRow& R = rows[n];
    const bool plate = plate_ok(R);
    if (plate && threadIdx.x == 0) {
        // the mean of the canvas: the image's tile sums in index order, rounded to float32 once; then k = D mu + e
        double sum[3] = {0.0, 0.0, 0.0};
        for (int p = 0; p < tiles; ++p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += partial[(n * tiles + p) * 3 + c];
        }
        float mu[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = (float)(sum[c] / (double)((long long)H * W));
#pragma unroll
        for (int c = 0; c < 3; ++c) kk[c] = ((R.D[3 * c] * mu[0] + R.D[3 * c + 1] * mu[1]) + R.D[3 * c + 2] * mu[2]) + R.e[c];
    }
    __syncthreads();
    const int q = blockIdx.x * OCR_THREADS + threadIdx.x;
    if (q >= H * G) return;
    const int i = q / G, j0 = (q - i * G) * 4;
    const long long plane = (long long)H * W;
    const long long base = n * 3 * plane + (long long)i * W + j0;
    float b[3][4], o[3][4];
    render_load_planes<VEC>(bg, base, plane, j0, W, b);
    const OcrWindow win = ocr_window(R, H, W);
    const bool row_in = plate && i >= win.t && i < win.b;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = j0 + e;
        if (row_in && j >= win.l && j < win.r) {
            const float4 Q = Qws[(n * H + i) * (long long)W + j];
            const float mask = Q.w / 255.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float lin = ((R.A[3 * c] * Q.x + R.A[3 * c + 1] * Q.y) + R.A[3 * c + 2] * Q.z) + kk[c];
                const float fg = lin / 255.f;
                const float under = b[c][e] * (1.f - mask);
                const float t = (bg_unit ? under : under / 255.f) + fg * mask;
                o[c][e] = fminf(fmaxf(t, 0.f), 1.f);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c][e] = fminf(fmaxf(bg_unit ? b[c][e] : b[c][e] / 255.f, 0.f), 1.f);
        }
    }
    render_store_planes<VEC>(out, base, plane, j0, W, o);
}

static int ocr_plate_check(const void* rows, const void* workspace, int N, int H, int W) {
    if (!rows || !workspace) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0) return YOLO_EINVAL;
    if (misaligned(rows, 7ull) || misaligned(workspace, 15ull)) return YOLO_EINVAL;
    // one image's thread index and its tile count are 32-bit in the kernels
    if ((long long)H * ((W + 3) / 4) > 0x7fffff00LL || (H + OCR_TILE - 1) / OCR_TILE > 65535) return YOLO_EUNSUPPORTED;
    return YOLO_OK;
}

extern "C" long long yolo_ocr_plate_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return YOLO_EINVAL;
    return ocr_q_offset(N, H, W) + (long long)N * H * W * (long long)sizeof(float4);
}

extern "C" int yolo_ocr_plate_blur(const unsigned char* plates, const void* rows, const void* taps, void* workspace, int N, int H, int W,
                                   void* stream) {
    if (!plates || !taps) return YOLO_EINVAL;
    const int rc = ocr_plate_check(rows, workspace, N, H, W);
    if (rc != YOLO_OK) return rc;
    if (misaligned(plates, 3ull) || misaligned(taps, 3ull)) return YOLO_EINVAL;
    const PlateRow* r = static_cast<const PlateRow*>(rows);
    const int* tp = static_cast<const int*>(taps);
    const long long tiles = ocr_tiles(H, W);
    double* part = static_cast<double*>(workspace);
    float4* Q = reinterpret_cast<float4*>(static_cast<char*>(workspace) + ocr_q_offset(N, H, W));
    const dim3 grid((W + OCR_TILE - 1) / OCR_TILE, (H + OCR_TILE - 1) / OCR_TILE, 1);
    for (int n0 = 0; n0 < N; n0 += 65535) {                          // (grid.z holds at most 65535 images)
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        YOLO_LAUNCH(ocr_blur_kernel, dim3(grid.x, grid.y, nb), dim3(OCR_THREADS), 0, (hipStream_t)stream,
                    plates + 4LL * n0 * PLATE_H * PLATE_W, r + n0, tp + (long long)n0 * YOLO_OCR_TAP_WORDS, part + n0 * tiles * 3,
                    Q + (long long)n0 * H * W, H, W);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_ocr_plate_render(const float* bg, const void* rows, const void* workspace, float* out, int N, int H, int W, int bg_unit,
                                     void* stream) {
    if (!bg || !out) return YOLO_EINVAL;
    const int rc = ocr_plate_check(rows, workspace, N, H, W);
    if (rc != YOLO_OK) return rc;
    if (misaligned(bg, 3ull) || misaligned(out, 3ull)) return YOLO_EINVAL;
    const PlateRow* r = static_cast<const PlateRow*>(rows);
    const long long tiles = ocr_tiles(H, W);
    if (tiles > 0x7fffffffLL) return YOLO_EUNSUPPORTED;
    const double* part = static_cast<const double*>(workspace);
    const float4* Q = reinterpret_cast<const float4*>(static_cast<const char*>(workspace) + ocr_q_offset(N, H, W));
    const int G = (W + 3) / 4;
    const bool vec = (W % 4) == 0 && !misaligned(bg, 15ull) && !misaligned(out, 15ull);
    const unsigned gx = (unsigned)(((long long)H * G + OCR_THREADS - 1) / OCR_THREADS);
    const long long img = 3LL * H * W;
    for (int n0 = 0; n0 < N; n0 += 65535) {
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        if (vec)
            YOLO_LAUNCH((ocr_blend_kernel<true>), dim3(gx, nb), dim3(OCR_THREADS), 0, (hipStream_t)stream, bg + n0 * img, r + n0,
                        part + n0 * tiles * 3, Q + (long long)n0 * H * W, out + n0 * img, H, W, G, (int)tiles, bg_unit);
        else
            YOLO_LAUNCH((ocr_blend_kernel<false>), dim3(gx, nb), dim3(OCR_THREADS), 0, (hipStream_t)stream, bg + n0 * img, r + n0,
                        part + n0 * tiles * 3, Q + (long long)n0 * H * W, out + n0 * img, H, W, G, (int)tiles, bg_unit);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

// ---- loss_mask -----------------------------------------------------------------------------------------------------------------
// round half away from zero, limited to +-2^30 before it becomes an integer (a NaN goes to -2^30)
__device__ __forceinline__ int ocr_round(float v) { return (int)fminf(fmaxf(roundf(v), -RENDER_IDX_LIMIT), RENDER_IDX_LIMIT); }

__global__ __launch_bounds__(OCR_THREADS) void ocr_targets_kernel(const float* __restrict__ labels, const int* __restrict__ order,
                                                                  float* __restrict__ score_y, int* __restrict__ class_y, long long total,
                                                                  int nobj, int Wp) {
    const long long q = (long long)blockIdx.x * OCR_THREADS + threadIdx.x;
    if (q >= total) return;
    const long long b = q / Wp;
    const int i = (int)(q - b * Wp);
    const float wp = (float)Wp;
    float score = 0.f;
    int cls = -1;
    for (int p = 0; p < nobj; ++p) {
        const int k = order ? order[b * nobj + p] : p;
        if (k < 0 || k >= nobj) continue;
        const float* Lb = labels + (b * nobj + k) * 3;
        const float c = Lb[0], L1 = Lb[1], L2 = Lb[2];
        if (!(c >= 0.f)) continue;
        const int left = max(ocr_round(L1 * wp), 0), right = min(ocr_round(L2 * wp), Wp);
        if (i < left || i >= right) continue;
        const float box_cent = ((float)i + 0.5f) / wp;
        const float text_cent = (L1 + L2) / 2.f;
        score = 1.f - fabsf(box_cent - text_cent) / (L2 - L1);
        cls = (int)fminf(c, RENDER_IDX_LIMIT);
    }
    score_y[q] = score;
    class_y[q] = cls;
}

extern "C" int yolo_ocr_targets(const float* labels, const int* order, float* score_y, int* class_y, int B, int nobj, int Wp, void* stream) {
    if (!labels || !score_y || !class_y) return YOLO_EINVAL;
    if (B <= 0 || nobj <= 0 || Wp <= 0) return YOLO_EINVAL;
    if (misaligned(labels, 3ull) || misaligned(order, 3ull) || misaligned(score_y, 3ull) || misaligned(class_y, 3ull)) return YOLO_EINVAL;
    const long long total = (long long)B * Wp;
    if (total >= (1LL << 31) || (long long)B * nobj * 3 >= (1LL << 31)) return YOLO_EUNSUPPORTED;
    YOLO_LAUNCH(ocr_targets_kernel, dim3((unsigned)((total + OCR_THREADS - 1) / OCR_THREADS)), dim3(OCR_THREADS), 0, (hipStream_t)stream, labels,
                order, score_y, class_y, total, nobj, Wp);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// ---- the two losses ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {                // a fixed butterfly: every lane gets the same bits
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// grid (images), 256 threads: wave w of 4 takes columns w, w + 4, ...; its lanes share the classes of a column (lane l: classes
// l, l + 64, ...).  The column terms of a wave are added in column order, the four waves' sums in wave order.
__global__ __launch_bounds__(OCR_THREADS) void ocr_loss_kernel(const float* __restrict__ logits, const float* __restrict__ score_y,
                                                               const int* __restrict__ class_y, float* __restrict__ dlogits,
                                                               float* __restrict__ losses, int B, int Wp, int ncls, float score_w, float class_w) {
    __shared__ float part[2][OCR_THREADS / 64];
    const long long b = blockIdx.x;
    const int C = 1 + ncls, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float wp = (float)Wp;
    float s_sum = 0.f, c_sum = 0.f;
    for (int i = wave; i < Wp; i += OCR_THREADS / 64) {
        const float* row = logits + (b * Wp + i) * C;
        float* drow = dlogits ? dlogits + (b * Wp + i) * C : nullptr;
        const float y = score_y[b * Wp + i];
        const int k = min(max(class_y[b * Wp + i], 0), ncls - 1);          // pick's clip mode
        const float z = row[0];
        const float en = expf(-fabsf(z));
        s_sum = s_sum + ((fmaxf(z, 0.f) - z * y) + log1pf(en));
        float mx = -__builtin_huge_valf();
        for (int c = lane; c < ncls; c += 64) mx = fmaxf(mx, row[1 + c]);
        mx = wave_max(mx);
        float se = 0.f;
        for (int c = lane; c < ncls; c += 64) se = se + expf(row[1 + c] - mx);
        se = wave_sum(se);
        const float lse = mx + logf(se);
        c_sum = c_sum + y * (lse - row[1 + k]);
        if (drow) {
            if (lane == 0) {
                const float sig = z >= 0.f ? 1.f / (1.f + en) : en / (1.f + en);
                drow[0] = (score_w / wp) * (sig - y);
            }
            const float g = (class_w / wp) * y;
            for (int c = lane; c < ncls; c += 64) {
                const float p = expf(row[1 + c] - mx) / se;
                drow[1 + c] = g * (p - (c == k ? 1.f : 0.f));
            }
        }
    }
    if (lane == 0) {
        part[0][wave] = s_sum;
        part[1][wave] = c_sum;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float* p = part[threadIdx.x];
        const float total = ((p[0] + p[1]) + p[2]) + p[3];
        losses[(long long)threadIdx.x * B + b] = (threadIdx.x == 0 ? score_w : class_w) * (total / wp);
    }
}

extern "C" int yolo_ocr_loss_fwd_bwd(const float* logits, const float* score_y, const int* class_y, float* dlogits, float* losses, int B,
                                     int Wp, int ncls, float score_w, float class_w, void* stream) {
    if (!logits || !score_y || !class_y || !losses) return YOLO_EINVAL;
    if (B <= 0 || Wp <= 0 || ncls <= 0) return YOLO_EINVAL;
    if (misaligned(logits, 3ull) || misaligned(score_y, 3ull) || misaligned(class_y, 3ull) || misaligned(dlogits, 3ull) || misaligned(losses, 3ull))
        return YOLO_EINVAL;
    if ((long long)B * Wp * (1 + ncls) * (long long)sizeof(float) >= (1LL << 31)) return YOLO_EUNSUPPORTED;      // logits of 2^31 bytes or more
    YOLO_LAUNCH(ocr_loss_kernel, dim3(B), dim3(OCR_THREADS), 0, (hipStream_t)stream, logits, score_y, class_y, dlogits, losses, B, Wp, ncls,
                score_w, class_w);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// ---- the bookkeeping of a validation step --------------------------------------------------------------------------------------
constexpr int OCR_SCORE_NOBJ = YOLO_OCR_SCORE_MAX_NOBJ, OCR_SCORE_WP = YOLO_OCR_SCORE_MAX_WP;

// one thread per image: the truth text (labels sorted by centre, a stable insertion sort), the predicted text (the first count[b]
// non-negative codes), the Levenshtein distance by the two-row dynamic programme (one row kept: nobj + 1 cells), the column counts
__global__ __launch_bounds__(64) void ocr_score_kernel(const int* __restrict__ codes, const int* __restrict__ count, const float* __restrict__ labels,
                                                       const int* __restrict__ class_y, const float* __restrict__ logits, int* __restrict__ counts,
                                                       int B, int nobj, int Wp, int ncls) {
    const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int truth[OCR_SCORE_NOBJ];
    float centre[OCR_SCORE_NOBJ];
    int nt = 0;
    for (int k = 0; k < nobj; ++k) {
        const float* Lb = labels + (b * nobj + k) * 3;
        const float c = Lb[0], mid = (Lb[1] + Lb[2]) / 2.f;
        if (!(c >= 0.f) || !(mid >= 0.f && mid < 1.f)) continue;
        int at = nt;
        while (at > 0 && centre[at - 1] > mid) {
            centre[at] = centre[at - 1];
            truth[at] = truth[at - 1];
            --at;
        }
        centre[at] = mid;
        truth[at] = (int)fminf(c, RENDER_IDX_LIMIT);
        ++nt;
    }
    const int want = min(max(count[b], 0), Wp);
    int dp[OCR_SCORE_NOBJ + 1];
    for (int t = 0; t <= nt; ++t) dp[t] = t;
    int np = 0;
    for (int i = 0; i < Wp && np < want; ++i) {
        const int code = codes[b * Wp + i];
        if (code < 0) continue;
        ++np;
        int diag = dp[0];
        dp[0] = np;
        for (int t = 1; t <= nt; ++t) {
            const int up = dp[t];
            dp[t] = min(min(up + 1, dp[t - 1] + 1), diag + (truth[t - 1] == code ? 0 : 1));
            diag = up;
        }
    }
    const int dist = dp[nt];
    int labelled = 0, right = 0;
    const int C = 1 + ncls;
    for (int i = 0; i < Wp; ++i) {
        const int y = class_y[b * Wp + i];
        if (y < 0) continue;
        ++labelled;
        const float* cl = logits + (b * Wp + i) * C + 1;
        float best = cl[0];
        int arg = 0;
        for (int k = 1; k < ncls; ++k)
            if (cl[k] > best) { best = cl[k]; arg = k; }                   // the first maximum: np.argmax
        right += arg == y;
    }
    int* o = counts + b * YOLO_OCR_SCORE_WORDS;
    o[0] = nt;
    o[1] = np;
    o[2] = dist;
    o[3] = dist == 0;
    o[4] = labelled;
    o[5] = right;
}

extern "C" int yolo_ocr_score(const int* codes, const int* count, const float* labels, const int* class_y, const float* logits, int* counts,
                              int B, int nobj, int Wp, int ncls, void* stream) {
    if (!codes || !count || !labels || !class_y || !logits || !counts) return YOLO_EINVAL;
    if (B <= 0 || nobj <= 0 || Wp <= 0 || ncls <= 0) return YOLO_EINVAL;
    if (misaligned(codes, 3ull) || misaligned(count, 3ull) || misaligned(labels, 3ull) || misaligned(class_y, 3ull) || misaligned(logits, 3ull) ||
        misaligned(counts, 3ull))
        return YOLO_EINVAL;
    if (nobj > OCR_SCORE_NOBJ || Wp > OCR_SCORE_WP) return YOLO_EUNSUPPORTED;
    if ((long long)B * Wp * (1 + ncls) * (long long)sizeof(float) >= (1LL << 31)) return YOLO_EUNSUPPORTED;
    YOLO_LAUNCH(ocr_score_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, codes, count, labels, class_y, logits, counts, B, nobj,
                Wp, ncls);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
