// Licence plates drawn onto training batches on the device for gfx950: LPGenerator.add (licence_plate_render/__init__.py:58-166)
// with the pixels made here.  The host decides -- glyphs, projective map, blur weights, noise key, colour map, window -- as one row
// of scalars per image (yolo_amd/render.py LPGenerator.draw_params); three kernels do the pixels:
//   plate_compose_kernel  the 380 x 160 RGBA plate of every image from the resident glyph atlas (PIL's mask-less paste)
//   plate_stats_kernel    the mean colour of the un-augmented plate canvas (what the contrast stage of the colour chain needs)
//   plate_render_kernel   sample through the projective map, blur, noise, colour, blend over the 0..1 background, clip
// Compiled with -ffp-contract=off: the arithmetic is the op-by-op fp32 definition of include/yolo_amd.h (yolo_plate_render), so
// tests/plate_ref.py reproduces it bit for bit (the mean to one float32 ulp: the order of its double sum differs).  The noise is
// integer work (Philox4x32-10, byte sums), so it is exact as well.  The tap and the blur are render.hip's (render_sample.h); the row,
// the sample through its map and the noise are shared with the OCR batch's renderer (plate_row.h, ocr_data.hip).  One thread makes
// 4 adjacent columns of the three planes.  The row of an image is read at a block-uniform address.
#include "plate_row.h"

constexpr int PLATE_THREADS = 256;
constexpr int PLATE_STAT_BLOCKS = 16;                     // partial sums per image (the workspace holds 3 doubles for each)
constexpr int GLYPH_H = 90, GLYPH_W = 45, GLYPH_TOP = 35;
constexpr int DOT_H = 70, DOT_W = 10, DOT_TOP = 45, DOT_LEFT = 158;
constexpr int GLYPH_PIXELS = GLYPH_H * GLYPH_W;
static_assert(GLYPH_COUNT * GLYPH_PIXELS * 4 + DOT_H * DOT_W * 4 == YOLO_PLATE_GLYPH_BYTES, "the atlas layout of include/yolo_amd.h");

// the left column of glyph cell k of 7 (LP_GLYPH_X without the dot's entry)
__device__ __forceinline__ int plate_cell_x(int k) {
    switch (k) {
        case 0: return 7;
        case 1: return 56;
        case 2: return 106;
        case 3: return 175;
        case 4: return 225;
        case 5: return 274;
        default: return 324;
    }
}

// grid (ceil(160 * 380 / 256), images): one thread, one texel, one 4-byte store
__global__ __launch_bounds__(PLATE_THREADS) void plate_compose_kernel(const uint32_t* __restrict__ glyphs, const PlateRow* __restrict__ rows,
                                                                      uint32_t* __restrict__ plates) {
    const int q = blockIdx.x * PLATE_THREADS + threadIdx.x;
    if (q >= PLATE_H * PLATE_W) return;
    const long long n = blockIdx.y;
    const PlateRow& R = rows[n];
    if (!plate_ok(R)) return;
    const int y = q / PLATE_W, x = q - y * PLATE_W;
    int src = -1;                                         // the atlas pixel this texel shows, -1: the white ground
    if (y >= GLYPH_TOP && y < GLYPH_TOP + GLYPH_H) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int dx = x - plate_cell_x(k);
            if (dx >= 0 && dx < GLYPH_W) src = R.glyph[k] * GLYPH_PIXELS + (y - GLYPH_TOP) * GLYPH_W + dx;
        }
    }
    if (y >= DOT_TOP && y < DOT_TOP + DOT_H && x >= DOT_LEFT && x < DOT_LEFT + DOT_W)
        src = GLYPH_COUNT * GLYPH_PIXELS + (y - DOT_TOP) * DOT_W + (x - DOT_LEFT);
    plates[n * (PLATE_H * PLATE_W) + q] = src >= 0 ? glyphs[src] : 0xffffffffu;
}

// What the pixel kernels need of a row after the checks; plate == nullptr means "no plate".
struct PlateView {
    const unsigned char* plate;
    int l, t, r, b;
    float m[9];
    float w0, w1, s;
    uint32_t k0, k1;
};

__device__ __forceinline__ PlateView plate_view(const PlateRow& R, const unsigned char* plates, long long n, int H, int W) {
    PlateView v;
    v.plate = plate_ok(R) ? plates + n * (4LL * PLATE_H * PLATE_W) : nullptr;
    v.l = max(R.l, 0);                                    // the window is clipped to the canvas whatever the row holds
    v.t = max(R.t, 0);
    v.r = min(R.r, W);
    v.b = min(R.b, H);
#pragma unroll
    for (int k = 0; k < 9; ++k) v.m[k] = R.m[k];
    v.w0 = R.w0;
    v.w1 = R.w1;
    v.s = R.s;
    v.k0 = R.k0;
    v.k1 = R.k1;
    return v;
}

// does any of columns j0..j0+3 of row i lie in the window
__device__ __forceinline__ bool plate_in_window(const PlateView& v, int j0, int i) { return i >= v.t && i < v.b && j0 + 3 >= v.l && j0 < v.r; }

// Q of output pixels (j0..j0+3, i), v.plate != nullptr: the plate through the projective map (0 outside the window, nothing sampled
// there), blurred, then the noise -- made after the blur sum, so the Philox rounds do not live beside the blur's taps.
__device__ __forceinline__ void plate_quad(const PlateView& v, int j0, int i, float (*Q)[4]) {
    if (plate_in_window(v, j0, i)) {
        const float* m = v.m;
        const unsigned char* plate = v.plate;
        render_blur_quad(
            [&](float x, float y, float* val) { plate_sample(plate, m, x, y, val); },
            v.w0, v.w1, j0, i, Q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = j0 + e >= v.l && j0 + e < v.r;
#pragma unroll
            for (int c = 0; c < 4; ++c) Q[e][c] = in ? Q[e][c] : 0.f;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) Q[e][c] = 0.f;
    }
    if (v.s != 0.f) {
#pragma unroll
        for (int e = 0; e < 4; ++e) plate_noise(Q[e], j0 + e, i, v.s, v.k0, v.k1);
    }
}

// grid (PLATE_STAT_BLOCKS, images).  The threads of an image walk ALL column groups of the canvas with a fixed stride (so the
// order of the sums does not depend on the window), each adding its pixels' R, G, B in double; a group whose Q is known to be 0
// (no noise, outside the window) is passed over.  A fixed-order tree over the block; block p of image n writes
// partial[(n * PLATE_STAT_BLOCKS + p) * 3 + c].  No atomics: the sums do not depend on scheduling.
__global__ __launch_bounds__(PLATE_THREADS) void plate_stats_kernel(const unsigned char* __restrict__ plates, const PlateRow* __restrict__ rows,
                                                                    double* __restrict__ partial, int H, int W, int G) {
    __shared__ double red[3][PLATE_THREADS];
    const long long n = blockIdx.y;
    const PlateView v = plate_view(rows[n], plates, n, H, W);
    double acc[3] = {0.0, 0.0, 0.0};
    if (v.plate != nullptr) {
        const int total = H * G;
        for (int q = blockIdx.x * PLATE_THREADS + threadIdx.x; q < total; q += PLATE_STAT_BLOCKS * PLATE_THREADS) {
            const int i = q / G, j0 = (q - i * G) * 4;
            if (v.s == 0.f && !plate_in_window(v, j0, i)) continue;
            float Q[4][4];
            plate_quad(v, j0, i, Q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j0 + e < W) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += (double)Q[e][c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][threadIdx.x] = acc[c];
    __syncthreads();
    for (int s = PLATE_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[(n * PLATE_STAT_BLOCKS + blockIdx.x) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// grid (ceil(H * G / 256), images), G = ceil(W / 4) column groups per row; thread q of an image: row q / G, columns 4 (q % G)..+3.
// bg and out may be one buffer (no __restrict__ on them): a thread reads its 12 values before it writes them, and no other
// thread touches them.
template <bool VEC>
__global__ __launch_bounds__(PLATE_THREADS) void plate_render_kernel(const float* bg, const unsigned char* __restrict__ plates,
                                                                     const PlateRow* __restrict__ rows, const double* __restrict__ partial,
                                                                     float* out, int H, int W, int G) {
    const int q = blockIdx.x * PLATE_THREADS + threadIdx.x;
    if (q >= H * G) return;
    const long long n = blockIdx.y;
    const int i = q / G, j0 = (q - i * G) * 4;
    const long long plane = (long long)H * W;
    const long long base = n * 3 * plane + (long long)i * W + j0;
    float b[3][4];
    render_load_planes<VEC>(bg, base, plane, j0, W, b);
    const PlateRow& R = rows[n];
    const PlateView v = plate_view(R, plates, n, H, W);
    float o[3][4];
    const bool noisy = v.s != 0.f;
    if (v.plate != nullptr && (noisy || plate_in_window(v, j0, i))) {
        float Q[4][4];
        plate_quad(v, j0, i, Q);
        // the mean of the canvas: the image's partial sums in index order, rounded to float32 once; then k = D mu + e
        double sum[3] = {0.0, 0.0, 0.0};
        for (int p = 0; p < PLATE_STAT_BLOCKS; ++p) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += partial[(n * PLATE_STAT_BLOCKS + p) * 3 + c];
        }
        float mu[3], cc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = (float)(sum[c] / (double)plane);
#pragma unroll
        for (int c = 0; c < 3; ++c) cc[c] = ((R.D[3 * c] * mu[0] + R.D[3 * c + 1] * mu[1]) + R.D[3 * c + 2] * mu[2]) + R.e[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = noisy || (j0 + e >= v.l && j0 + e < v.r);
            const float mask = Q[e][3] / 255.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float lin = ((R.A[3 * c] * Q[e][0] + R.A[3 * c + 1] * Q[e][1]) + R.A[3 * c + 2] * Q[e][2]) + cc[c];
                const float fg = lin / 255.f;
                const float t = b[c][e] * (1.f - mask) + fg * mask;
                o[c][e] = fminf(fmaxf(in ? t : b[c][e], 0.f), 1.f);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[c][e] = fminf(fmaxf(b[c][e], 0.f), 1.f);
    }
    render_store_planes<VEC>(out, base, plane, j0, W, o);
}

static bool misaligned(const void* p, unsigned long long mask) { return (reinterpret_cast<unsigned long long>(p) & mask) != 0; }

static int plate_check(const void* plates, const void* rows, const void* workspace, int N, int H, int W) {
    if (!plates || !rows || !workspace) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0) return YOLO_EINVAL;
    if (misaligned(plates, 3ull) || misaligned(rows, 7ull) || misaligned(workspace, 7ull)) return YOLO_EINVAL;
    // one image's thread index is 32-bit in the kernels
    if ((long long)H * ((W + 3) / 4) > 0x7fffff00LL) return YOLO_EUNSUPPORTED;
    return YOLO_OK;
}

extern "C" long long yolo_plate_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return YOLO_EINVAL;
    return (long long)N * PLATE_STAT_BLOCKS * 3 * (long long)sizeof(double);
}

extern "C" int yolo_plate_compose(const unsigned char* glyphs, const void* rows, unsigned char* plates, int N, void* stream) {
    if (!glyphs || !rows || !plates || N <= 0) return YOLO_EINVAL;
    if (misaligned(glyphs, 3ull) || misaligned(rows, 7ull) || misaligned(plates, 3ull)) return YOLO_EINVAL;
    const PlateRow* r = static_cast<const PlateRow*>(rows);
    const unsigned gx = (PLATE_H * PLATE_W + PLATE_THREADS - 1) / PLATE_THREADS;
    for (int n0 = 0; n0 < N; n0 += 65535) {                          // (grid.y holds at most 65535 images)
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        YOLO_LAUNCH(plate_compose_kernel, dim3(gx, nb), dim3(PLATE_THREADS), 0, (hipStream_t)stream,
                    reinterpret_cast<const uint32_t*>(glyphs), r + n0, reinterpret_cast<uint32_t*>(plates) + (long long)n0 * PLATE_H * PLATE_W);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_plate_stats(const unsigned char* plates, const void* rows, void* workspace, int N, int H, int W, void* stream) {
    const int rc = plate_check(plates, rows, workspace, N, H, W);
    if (rc != YOLO_OK) return rc;
    const PlateRow* r = static_cast<const PlateRow*>(rows);
    double* part = static_cast<double*>(workspace);
    const int G = (W + 3) / 4;
    for (int n0 = 0; n0 < N; n0 += 65535) {
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        YOLO_LAUNCH(plate_stats_kernel, dim3(PLATE_STAT_BLOCKS, nb), dim3(PLATE_THREADS), 0, (hipStream_t)stream,
                    plates + 4LL * n0 * PLATE_H * PLATE_W, r + n0, part + (long long)n0 * PLATE_STAT_BLOCKS * 3, H, W, G);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_plate_render(const float* bg, const unsigned char* plates, const void* rows, const void* workspace, float* out, int N,
                                 int H, int W, void* stream) {
    if (!bg || !out) return YOLO_EINVAL;
    const int rc = plate_check(plates, rows, workspace, N, H, W);
    if (rc != YOLO_OK) return rc;
    if (misaligned(bg, 3ull) || misaligned(out, 3ull)) return YOLO_EINVAL;
    const PlateRow* r = static_cast<const PlateRow*>(rows);
    const double* part = static_cast<const double*>(workspace);
    const int G = (W + 3) / 4;
    const bool vec = (W % 4) == 0 && !misaligned(bg, 15ull) && !misaligned(out, 15ull);
    const unsigned gx = (unsigned)(((long long)H * G + PLATE_THREADS - 1) / PLATE_THREADS);
    const long long img = 3LL * H * W;
    for (int n0 = 0; n0 < N; n0 += 65535) {
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        const unsigned char* pl = plates + 4LL * n0 * PLATE_H * PLATE_W;
        if (vec)
            YOLO_LAUNCH((plate_render_kernel<true>), dim3(gx, nb), dim3(PLATE_THREADS), 0, (hipStream_t)stream, bg + n0 * img, pl, r + n0,
                        part + (long long)n0 * PLATE_STAT_BLOCKS * 3, out + n0 * img, H, W, G);
        else
            YOLO_LAUNCH((plate_render_kernel<false>), dim3(gx, nb), dim3(PLATE_THREADS), 0, (hipStream_t)stream, bg + n0 * img, pl, r + n0,
                        part + (long long)n0 * PLATE_STAT_BLOCKS * 3, out + n0 * img, H, W, G);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}
