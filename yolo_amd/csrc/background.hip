// Training backgrounds made on the device for gfx950: what mxnet.image.ImageIter does per image for yolo_gluon.load_background
// (yolo_modules/yolo_gluon.py:43-97: random-sized crop, resize, mirror, brightness / contrast / saturation / hue) with the pixels
// made here.  The host decides -- image, mip level, crop, mirror, colour map -- as one row of scalars per output image
// (yolo_amd/background.py draw_params); two kernels do the pixels from a resident uint8 bank of 4-byte pixels:
//   bg_stats_kernel    the mean colour of the resized crop (what the contrast stage of the colour chain needs)
//   bg_render_kernel   sample again, colour, store the three fp32 planes 0..255 that yolo_render_cars takes as bg
// Compiled with -ffp-contract=off: the arithmetic is the op-by-op fp32 definition of include/yolo_amd.h (yolo_bg_render), so
// tests/background_ref.py reproduces it bit for bit (the mean to one float32 ulp: the order of its double sum differs).
// HBM-bound: 12 B written per output pixel, the taps (16 B per pixel asked for, neighbours share them) mostly hit in cache; the
// second pass samples again rather than carry P through memory (12 B written + 12 B read per pixel).  One thread makes 4 adjacent
// columns of the three planes (16-byte stores when W % 4 == 0 and out is 16-byte aligned, scalar ones with a tail thread
// otherwise).  The row of an image is read at a block-uniform address, so it arrives through scalar loads.
#include "common.h"
#include "render_sample.h"

constexpr int BG_THREADS = 256;
constexpr int BG_STAT_BLOCKS = 16;                        // partial sums per image (the workspace holds 3 doubles for each)

struct BgRow {                                            // YOLO_BG_ROW_WORDS 32-bit words (include/yolo_amd.h)
    int has, h, w;
    int x0, y0, x1, y1;                                   // the roi, inclusive, in level pixels
    int pad0;
    long long offset;
    float a[6];
    float A[9], D[9], e[3];
    int pad1[3];
};
static_assert(sizeof(BgRow) == 4 * YOLO_BG_ROW_WORDS, "the parameter row is YOLO_BG_ROW_WORDS words");

// What a kernel needs of a row after the checks: level == nullptr means "no image" (the flag is off, the level does not lie
// inside the bank, or the roi is empty or not inside the level -- then nothing is loaded from the bank at all).
struct BgLevel {
    const unsigned char* level;
    int w, x0, y0, x1, y1;
};

__device__ __forceinline__ BgLevel bg_level(const BgRow& R, const unsigned char* bank, long long bank_bytes) {
    BgLevel v;
    const bool inside = R.has != 0 && R.h > 0 && R.w > 0 && R.offset >= 0 && (R.offset & 3) == 0 && R.offset <= bank_bytes &&
                        (long long)R.h * R.w <= (bank_bytes - R.offset) / 4;
    const bool roi = R.x0 >= 0 && R.y0 >= 0 && R.x1 >= R.x0 && R.y1 >= R.y0 && R.x1 < R.w && R.y1 < R.h;
    v.level = (inside && roi) ? bank + R.offset : nullptr;
    v.w = R.w;
    v.x0 = R.x0;
    v.y0 = R.y0;
    v.x1 = R.x1;
    v.y1 = R.y1;
    return v;
}

// R, G, B of the sample at level position (sx, sy): render_tap's bilinear (render_sample.h) with the other border rule -- every
// tap INDEX is clamped into the roi (replicate), so no tap reads 0 and no load leaves the roi whatever the position is.
__device__ __forceinline__ void bg_tap(const BgLevel& v, float sx, float sy, float* val) {
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    // (fmaxf / fminf return the other operand for a NaN: a NaN coordinate indexes far outside, and the value is NaN through fx)
    const int x0 = (int)fminf(fmaxf(x0f, -RENDER_IDX_LIMIT), RENDER_IDX_LIMIT), x1 = x0 + 1;
    const int y0 = (int)fminf(fmaxf(y0f, -RENDER_IDX_LIMIT), RENDER_IDX_LIMIT), y1 = y0 + 1;
    const int cx0 = min(max(x0, v.x0), v.x1), cx1 = min(max(x1, v.x0), v.x1);
    const int cy0 = min(max(y0, v.y0), v.y1), cy1 = min(max(y1, v.y0), v.y1);
    const uint32_t* px = reinterpret_cast<const uint32_t*>(v.level);
    const long long r0 = (long long)cy0 * v.w, r1 = (long long)cy1 * v.w;
    const uint32_t pa = px[r0 + cx0], pb = px[r0 + cx1], pc = px[r1 + cx0], pd = px[r1 + cx1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float ta = (float)((pa >> (8 * c)) & 255u), tb = (float)((pb >> (8 * c)) & 255u);
        const float tc = (float)((pc >> (8 * c)) & 255u), td = (float)((pd >> (8 * c)) & 255u);
        const float top = ta + fx * (tb - ta);
        const float bot = tc + fx * (td - tc);
        val[c] = top + fy * (bot - top);
    }
}

// P of output pixels (j0..j0+3, i), R G B 0..255 before the colour map; a column past W, and every pixel of "no image", is 0
__device__ __forceinline__ void bg_quad(const BgLevel& v, const float* a, int j0, int i, int W, float (*px)[3]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        px[e][0] = px[e][1] = px[e][2] = 0.f;
        if (v.level != nullptr && j0 + e < W) {
            const float x = (float)(j0 + e), y = (float)i;
            const float sx = (a[0] * x + a[1] * y) + a[2];
            const float sy = (a[3] * x + a[4] * y) + a[5];
            bg_tap(v, sx, sy, px[e]);
        }
    }
}

// grid (BG_STAT_BLOCKS, images).  The threads of an image walk the H * G column groups of the canvas (G = ceil(W / 4)) with a fixed
// stride, each adding its pixels' R, G, B in double, columns in order; a fixed-order tree over the block; block p of image n
// writes partial[(n * BG_STAT_BLOCKS + p) * 3 + c].  No atomics: the sums do not depend on scheduling.
__global__ __launch_bounds__(BG_THREADS) void bg_stats_kernel(const unsigned char* __restrict__ bank, long long bank_bytes,
                                                              const BgRow* __restrict__ rows, double* __restrict__ partial, int H, int W,
                                                              int G) {
    __shared__ double red[3][BG_THREADS];
    const long long n = blockIdx.y;
    const BgRow& R = rows[n];
    const BgLevel v = bg_level(R, bank, bank_bytes);
    double acc[3] = {0.0, 0.0, 0.0};
    if (v.level != nullptr) {
        float a[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = R.a[k];
        const long long total = (long long)H * G;
        for (long long q = blockIdx.x * BG_THREADS + threadIdx.x; q < total; q += BG_STAT_BLOCKS * BG_THREADS) {
            const int i = (int)(q / G), j0 = (int)(q - (long long)i * G) * 4;
            float px[4][3];
            bg_quad(v, a, j0, i, W, px);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j0 + e < W) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += (double)px[e][c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][threadIdx.x] = acc[c];
    __syncthreads();
    for (int s = BG_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[(n * BG_STAT_BLOCKS + blockIdx.x) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// grid (ceil(H * G / 256), images), G = ceil(W / 4) column groups per row; thread q of an image: row q / G, columns 4 (q % G)..+3
template <bool VEC>
__global__ __launch_bounds__(BG_THREADS) void bg_render_kernel(const unsigned char* __restrict__ bank, long long bank_bytes,
                                                               const BgRow* __restrict__ rows, const double* __restrict__ partial,
                                                               float* __restrict__ out, int H, int W, int G) {
    const int q = blockIdx.x * BG_THREADS + threadIdx.x;
    if (q >= H * G) return;
    const long long n = blockIdx.y;
    const int i = q / G, j0 = (q - i * G) * 4;
    const long long plane = (long long)H * W;
    const long long base = n * 3 * plane + (long long)i * W + j0;           // 64-bit: B 3 H W passes 2^31 from 1380 images of 416^2 on
    const BgRow& R = rows[n];
    const BgLevel v = bg_level(R, bank, bank_bytes);
    float a[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = R.a[k];
    float px[4][3];
    bg_quad(v, a, j0, i, W, px);
    // the mean of the resized crop: the image's partial sums in index order, rounded to float32 once; then k = D mu + e
    double sum[3] = {0.0, 0.0, 0.0};
    for (int p = 0; p < BG_STAT_BLOCKS; ++p) {
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] += partial[(n * BG_STAT_BLOCKS + p) * 3 + c];
    }
    float mu[3], kk[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) mu[c] = (float)(sum[c] / (double)plane);
#pragma unroll
    for (int c = 0; c < 3; ++c) kk[c] = ((R.D[3 * c] * mu[0] + R.D[3 * c + 1] * mu[1]) + R.D[3 * c + 2] * mu[2]) + R.e[c];
    float o[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c][e] = ((R.A[3 * c] * px[e][0] + R.A[3 * c + 1] * px[e][1]) + R.A[3 * c + 2] * px[e][2]) + kk[c];
    render_store_planes<VEC>(out, base, plane, j0, W, o);
}

static int bg_check(const void* bank, long long bank_bytes, const void* rows, const void* workspace, int N, int H, int W) {
    if (!bank || !rows || !workspace) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || bank_bytes <= 0) return YOLO_EINVAL;
    if ((reinterpret_cast<unsigned long long>(bank) & 3ull) || (reinterpret_cast<unsigned long long>(rows) & 7ull) ||
        (reinterpret_cast<unsigned long long>(workspace) & 7ull))
        return YOLO_EINVAL;
    // one image's thread index is 32-bit in the kernels
    if ((long long)H * ((W + 3) / 4) > 0x7fffff00LL) return YOLO_EUNSUPPORTED;
    return YOLO_OK;
}

extern "C" long long yolo_bg_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return YOLO_EINVAL;
    return (long long)N * BG_STAT_BLOCKS * 3 * (long long)sizeof(double);
}

extern "C" int yolo_bg_stats(const unsigned char* bank, long long bank_bytes, const void* rows, void* workspace, int N, int H, int W,
                             void* stream) {
    const int rc = bg_check(bank, bank_bytes, rows, workspace, N, H, W);
    if (rc != YOLO_OK) return rc;
    const BgRow* r = static_cast<const BgRow*>(rows);
    double* part = static_cast<double*>(workspace);
    const int G = (W + 3) / 4;
    for (int n0 = 0; n0 < N; n0 += 65535) {                          // (grid.y holds at most 65535 images)
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        YOLO_LAUNCH(bg_stats_kernel, dim3(BG_STAT_BLOCKS, nb), dim3(BG_THREADS), 0, (hipStream_t)stream, bank, bank_bytes, r + n0,
                    part + (long long)n0 * BG_STAT_BLOCKS * 3, H, W, G);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_bg_render(const unsigned char* bank, long long bank_bytes, const void* rows, const void* workspace, float* out,
                              int N, int H, int W, void* stream) {
    if (!out) return YOLO_EINVAL;
    const int rc = bg_check(bank, bank_bytes, rows, workspace, N, H, W);
    if (rc != YOLO_OK) return rc;
    const BgRow* r = static_cast<const BgRow*>(rows);
    const double* part = static_cast<const double*>(workspace);
    const int G = (W + 3) / 4;
    const bool vec = (W % 4) == 0 && (reinterpret_cast<unsigned long long>(out) & 15ull) == 0;
    const unsigned gx = (unsigned)(((long long)H * G + BG_THREADS - 1) / BG_THREADS);
    const long long img = 3LL * H * W;
    for (int n0 = 0; n0 < N; n0 += 65535) {
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        if (vec)
            YOLO_LAUNCH((bg_render_kernel<true>), dim3(gx, nb), dim3(BG_THREADS), 0, (hipStream_t)stream, bank, bank_bytes, r + n0,
                        part + (long long)n0 * BG_STAT_BLOCKS * 3, out + n0 * img, H, W, G);
        else
            YOLO_LAUNCH((bg_render_kernel<false>), dim3(gx, nb), dim3(BG_THREADS), 0, (hipStream_t)stream, bank, bank_bytes, r + n0,
                        part + (long long)n0 * BG_STAT_BLOCKS * 3, out + n0 * img, H, W, G);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}
