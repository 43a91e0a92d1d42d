// Training batches drawn on the device for gfx950: RenderCar.render (car/render_car.py:52-138) with the pixels made here.  The
// host decides -- sprite, mip level, inverse affine, blur weights, colour map, window -- as one row of scalars per image
// (yolo_amd/render.py draw_params); two kernels do the pixels from a resident uint8 RGBA atlas:
//   render_stats_kernel   the mean colour of the un-augmented pasted canvas (what the contrast stage of the colour chain needs)
//   render_cars_kernel    sample, blur, colour, blend over the background, clip
// Compiled with -ffp-contract=off: the arithmetic is the op-by-op fp32 definition of include/yolo_amd.h (yolo_render_cars), so
// tests/render_ref.py reproduces it bit for bit (the mean to one float32 ulp: the order of its double sum differs).
// HBM-bound: 12 B read + 12 B written per output pixel; the sprite taps hit in cache.  One thread makes 4 adjacent columns of
// the three planes (16-byte loads and stores when W % 4 == 0 and bg / out are 16-byte aligned, scalar ones with a tail thread
// otherwise).  The row of an image is read at a block-uniform address, so it arrives through scalar loads.
#include "common.h"
#include "render_sample.h"

constexpr int RENDER_THREADS = 256;
constexpr int RENDER_STAT_BLOCKS = 16;                    // partial sums per image (the workspace holds 3 doubles for each)

struct RenderRow {                                        // YOLO_RENDER_ROW_WORDS 32-bit words (include/yolo_amd.h)
    int has, h, w;
    int l, t, r, b;
    int pad0;
    long long offset;
    float a[6];
    float w0, w1;
    float A[9], D[9], e[3];
    int pad1;
};
static_assert(sizeof(RenderRow) == 4 * YOLO_RENDER_ROW_WORDS, "the parameter row is YOLO_RENDER_ROW_WORDS words");

// What a kernel needs of a row after the checks: level == nullptr means "no sprite" (the flag is off, or the level does not lie
// inside the atlas -- then nothing is loaded from the atlas at all).
struct RenderLevel {
    const unsigned char* level;
    int h, w, l, t, r, b;
};

__device__ __forceinline__ RenderLevel render_level(const RenderRow& R, const unsigned char* atlas, long long atlas_bytes, int H, int W) {
    RenderLevel v;
    const bool ok = R.has != 0 && R.h > 0 && R.w > 0 && R.offset >= 0 && (R.offset & 3) == 0 && R.offset <= atlas_bytes &&
                    (long long)R.h * R.w <= (atlas_bytes - R.offset) / 4;
    v.level = ok ? atlas + R.offset : nullptr;
    v.h = R.h;
    v.w = R.w;
    v.l = max(R.l, 0);                                   // the window is clipped to the canvas whatever the row holds
    v.t = max(R.t, 0);
    v.r = min(R.r, W);
    v.b = min(R.b, H);
    return v;
}

// The four channels of the sample at output position (x, y): the bilinear tap (render_sample.h) at the affine's image of it.
__device__ __forceinline__ void render_sample(const unsigned char* __restrict__ level, int h, int w, const float* a, float x, float y,
                                              float* val) {
    const float sx = (a[0] * x + a[1] * y) + a[2];
    const float sy = (a[3] * x + a[4] * y) + a[5];
    render_tap(level, h, w, sx, sy, val);
}

// RGBA 0..255 of output pixels (j0..j0+3, i) before the colour map: the sample, or its 3x3 separable blur (render_sample.h)
__device__ __forceinline__ void render_quad(const RenderLevel& v, const float* a, float w0, float w1, int j0, int i, float (*px)[4]) {
    render_blur_quad([&](float x, float y, float* val) { render_sample(v.level, v.h, v.w, a, x, y, val); }, w0, w1, j0, i, px);
}

// grid (RENDER_STAT_BLOCKS, images).  The threads of an image walk the column groups of its WINDOW only (rows t..b-1, groups
// l/4 .. (r+3)/4 - 1) with a fixed stride, each adding its pixels' R, G, B in double; a fixed-order tree over the block; block p
// of image n writes partial[(n * RENDER_STAT_BLOCKS + p) * 3 + c].  No atomics: the sums do not depend on scheduling.
__global__ __launch_bounds__(RENDER_THREADS) void render_stats_kernel(const unsigned char* __restrict__ atlas, long long atlas_bytes,
                                                                      const RenderRow* __restrict__ rows, double* __restrict__ partial,
                                                                      int H, int W) {
    __shared__ double red[3][RENDER_THREADS];
    const long long n = blockIdx.y;
    const RenderRow& R = rows[n];
    const RenderLevel v = render_level(R, atlas, atlas_bytes, H, W);
    double acc[3] = {0.0, 0.0, 0.0};
    if (v.level != nullptr && v.r > v.l && v.b > v.t) {
        float a[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = R.a[k];
        const float w0 = R.w0, w1 = R.w1;
        const int g0 = v.l / 4, ng = (v.r + 3) / 4 - g0;
        const long long total = (long long)(v.b - v.t) * ng;
        for (long long q = blockIdx.x * RENDER_THREADS + threadIdx.x; q < total; q += RENDER_STAT_BLOCKS * RENDER_THREADS) {
            const int i = v.t + (int)(q / ng), j0 = (g0 + (int)(q % ng)) * 4;
            float px[4][4];
            render_quad(v, a, w0, w1, j0, i, px);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j0 + e >= v.l && j0 + e < v.r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += (double)px[e][c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][threadIdx.x] = acc[c];
    __syncthreads();
    for (int s = RENDER_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[(n * RENDER_STAT_BLOCKS + blockIdx.x) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// grid (ceil(H * G / 256), images), G = ceil(W / 4) column groups per row; thread q of an image: row q / G, columns 4 (q % G)..+3
template <bool VEC>
__global__ __launch_bounds__(RENDER_THREADS) void render_cars_kernel(const float* __restrict__ bg, const unsigned char* __restrict__ atlas,
                                                                     long long atlas_bytes, const RenderRow* __restrict__ rows,
                                                                     const double* __restrict__ partial, float* __restrict__ out, int H,
                                                                     int W, int G) {
    const int q = blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (q >= H * G) return;
    const long long n = blockIdx.y;
    const int i = q / G, j0 = (q - i * G) * 4;
    const long long plane = (long long)H * W;
    const long long base = n * 3 * plane + (long long)i * W + j0;           // 64-bit: B 3 H W passes 2^31 from 1380 images of 416^2 on
    float b[3][4];
    render_load_planes<VEC>(bg, base, plane, j0, W, b);
    const RenderRow& R = rows[n];
    const RenderLevel v = render_level(R, atlas, atlas_bytes, H, W);
    float o[3][4];
    const bool touched = v.level != nullptr && i >= v.t && i < v.b && j0 + 3 >= v.l && j0 < v.r;
    if (touched) {
        float a[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = R.a[k];
        float px[4][4];
        render_quad(v, a, R.w0, R.w1, j0, i, px);
        // the mean of the canvas: the image's partial sums in index order, rounded to float32 once; then c = D mu + e
        double sum[3] = {0.0, 0.0, 0.0};
        for (int p = 0; p < RENDER_STAT_BLOCKS; ++p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += partial[(n * RENDER_STAT_BLOCKS + p) * 3 + c];
        }
        float mu[3], cc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = (float)(sum[c] / (double)plane);
#pragma unroll
        for (int c = 0; c < 3; ++c) cc[c] = ((R.D[3 * c] * mu[0] + R.D[3 * c + 1] * mu[1]) + R.D[3 * c + 2] * mu[2]) + R.e[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = j0 + e >= v.l && j0 + e < v.r;
            const float mask = in ? px[e][3] / 255.f : 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float lin = ((R.A[3 * c] * px[e][0] + R.A[3 * c + 1] * px[e][1]) + R.A[3 * c + 2] * px[e][2]) + cc[c];
                const float fg = in ? lin / 255.f : 0.f;
                const float t = (b[c][e] / 255.f) * (1.f - mask) + fg * mask;
                o[c][e] = in ? fminf(fmaxf(t, 0.f), 1.f) : fminf(fmaxf(b[c][e] / 255.f, 0.f), 1.f);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[c][e] = fminf(fmaxf(b[c][e] / 255.f, 0.f), 1.f);
    }
    render_store_planes<VEC>(out, base, plane, j0, W, o);
}

static int render_check(const void* atlas, long long atlas_bytes, const void* rows, int N, int H, int W) {
    if (!atlas || !rows) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || atlas_bytes <= 0) return YOLO_EINVAL;
    if ((reinterpret_cast<unsigned long long>(atlas) & 3ull) || (reinterpret_cast<unsigned long long>(rows) & 7ull)) return YOLO_EINVAL;
    // one image's thread index is 32-bit in the kernels
    if ((long long)H * ((W + 3) / 4) > 0x7fffff00LL) return YOLO_EUNSUPPORTED;
    return YOLO_OK;
}

extern "C" long long yolo_render_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return YOLO_EINVAL;
    return (long long)N * RENDER_STAT_BLOCKS * 3 * (long long)sizeof(double);
}

extern "C" int yolo_render_stats(const unsigned char* atlas, long long atlas_bytes, const void* rows, void* workspace, int N, int H,
                                 int W, void* stream) {
    if (!workspace) return YOLO_EINVAL;
    const int rc = render_check(atlas, atlas_bytes, rows, N, H, W);
    if (rc != YOLO_OK) return rc;
    if (reinterpret_cast<unsigned long long>(workspace) & 7ull) return YOLO_EINVAL;
    const RenderRow* r = static_cast<const RenderRow*>(rows);
    double* part = static_cast<double*>(workspace);
    for (int n0 = 0; n0 < N; n0 += 65535) {                          // (grid.y holds at most 65535 images)
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        YOLO_LAUNCH(render_stats_kernel, dim3(RENDER_STAT_BLOCKS, nb), dim3(RENDER_THREADS), 0, (hipStream_t)stream, atlas, atlas_bytes,
                    r + n0, part + (long long)n0 * RENDER_STAT_BLOCKS * 3, H, W);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_render_cars(const float* bg, const unsigned char* atlas, long long atlas_bytes, const void* rows,
                                const void* workspace, float* out, int N, int H, int W, void* stream) {
    if (!bg || !out || !workspace) return YOLO_EINVAL;
    const int rc = render_check(atlas, atlas_bytes, rows, N, H, W);
    if (rc != YOLO_OK) return rc;
    if (reinterpret_cast<unsigned long long>(workspace) & 7ull) return YOLO_EINVAL;
    const RenderRow* r = static_cast<const RenderRow*>(rows);
    const double* part = static_cast<const double*>(workspace);
    const int G = (W + 3) / 4;
    const bool vec = (W % 4) == 0 && ((reinterpret_cast<unsigned long long>(bg) | reinterpret_cast<unsigned long long>(out)) & 15ull) == 0;
    const unsigned gx = (unsigned)(((long long)H * G + RENDER_THREADS - 1) / RENDER_THREADS);
    const long long img = 3LL * H * W;
    for (int n0 = 0; n0 < N; n0 += 65535) {
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        if (vec)
            YOLO_LAUNCH((render_cars_kernel<true>), dim3(gx, nb), dim3(RENDER_THREADS), 0, (hipStream_t)stream, bg + n0 * img, atlas,
                        atlas_bytes, r + n0, part + (long long)n0 * RENDER_STAT_BLOCKS * 3, out + n0 * img, H, W, G);
        else
            YOLO_LAUNCH((render_cars_kernel<false>), dim3(gx, nb), dim3(RENDER_THREADS), 0, (hipStream_t)stream, bg + n0 * img, atlas,
                        atlas_bytes, r + n0, part + (long long)n0 * RENDER_STAT_BLOCKS * 3, out + n0 * img, H, W, G);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}
