// Frame intake for gfx950: an inverse-mapped bilinear sampler from uint8 HWC frames to the net's fp32 NCHW input, one 3x3
// matrix per image.  Clip + flip + resize (yolo_cv.py:285-318 cv2_flip_and_clip_frame, cv2.resize, yolo_gluon.py:335-357
// cv_img_2_ndarray) are one affine matrix; the plate rectification of ProjectRectangle6D.add_edges
// (licence_plate_render/__init__.py:379-402, cv2.warpPerspective) is one homography.
// Compiled with -ffp-contract=off: the arithmetic is the op-by-op fp32 definition of include/yolo_amd.h (yolo_warp_u8_to_nchw),
// so tests/intake_ref.py reproduces it bit for bit.
// HBM-bound: one thread makes 4 adjacent output columns of every channel.  The planes of an image are contiguous over (row,
// column), so with Wo % 4 == 0 thread q writes the 16-byte unit q of each plane and a wave stores 1 KiB per plane; otherwise the
// last thread of a row holds the tail and every store is a scalar one.
#include "common.h"

constexpr int WARP_THREADS = 256;
constexpr int WARP_MAX_C = 4;
constexpr float WARP_IDX_LIMIT = 1073741824.f;          // 2^30: tap indices are clamped here before the int conversion

// C channels of output pixel (column j, row i).  Every tap ADDRESS is clamped into the roi (which lies inside the frame), so
// no load leaves the image whatever the matrix holds; with border 0 the value of a tap whose index was outside reads as 0.
template <int C>
__device__ __forceinline__ void warp_pixel(const unsigned char* __restrict__ img, const float* m, const float* g, int Ws, int j,
                                           int i, int border, int rx0, int ry0, int rx1, int ry1, float* val) {
    const float fj = (float)j, fi = (float)i;
    const float u = (m[0] * fj + m[1] * fi) + m[2];
    const float v = (m[3] * fj + m[4] * fi) + m[5];
    const float w = (m[6] * fj + m[7] * fi) + m[8];
    const float sx = u / w, sy = v / w;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    // (fmaxf / fminf return the other operand for a NaN: a NaN coordinate indexes far outside, and the value is NaN through fx)
    const int x0 = (int)fminf(fmaxf(x0f, -WARP_IDX_LIMIT), WARP_IDX_LIMIT), x1 = x0 + 1;
    const int y0 = (int)fminf(fmaxf(y0f, -WARP_IDX_LIMIT), WARP_IDX_LIMIT), y1 = y0 + 1;
    const int cx0 = min(max(x0, rx0), rx1), cx1 = min(max(x1, rx0), rx1);
    const int cy0 = min(max(y0, ry0), ry1), cy1 = min(max(y1, ry0), ry1);
    const bool keep = border != 0;
    const bool inx0 = keep || cx0 == x0, inx1 = keep || cx1 == x1, iny0 = keep || cy0 == y0, iny1 = keep || cy1 == y1;
    const long long row = (long long)Ws * C;
    const unsigned char* r0 = img + cy0 * row;
    const unsigned char* r1 = img + cy1 * row;
    const int o0 = cx0 * C, o1 = cx1 * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float a = (inx0 && iny0) ? (float)r0[o0 + c] : 0.f;
        const float b = (inx1 && iny0) ? (float)r0[o1 + c] : 0.f;
        const float cc = (inx0 && iny1) ? (float)r1[o0 + c] : 0.f;
        const float d = (inx1 && iny1) ? (float)r1[o1 + c] : 0.f;
        const float top = a + fx * (b - a);
        const float bot = cc + fx * (d - cc);
        const float t = top + fy * (bot - top);
        val[c] = (t / 255.f) * g[c];
    }
}

// grid (ceil(Ho * G / 256), images), G = ceil(Wo / 4) column groups per row; thread q of an image: row q / G, columns 4 (q % G)..+3
template <int C, bool VEC>
__global__ __launch_bounds__(WARP_THREADS) void warp_u8_to_nchw_kernel(const unsigned char* __restrict__ frames,
                                                                       float* __restrict__ y, const float* __restrict__ M,
                                                                       const float* __restrict__ gain, int Hs, int Ws, int Ho,
                                                                       int Wo, int G, int border, int rx0, int ry0, int rx1,
                                                                       int ry1) {
    const int q = blockIdx.x * WARP_THREADS + threadIdx.x;
    if (q >= Ho * G) return;
    const long long n = blockIdx.y;
    const int i = q / G, j0 = (q - i * G) * 4;
    float m[9], g[C];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = M[n * 9 + k];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = gain ? gain[c] : 1.f;
    const unsigned char* img = frames + n * Hs * Ws * C;           // 64-bit: N Hs Ws C passes 2^31 from ~86 4K frames on
    const long long plane = (long long)Ho * Wo;
    float* out = y + n * C * plane + (long long)i * Wo + j0;
    float val[4][C];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (VEC || j0 + e < Wo) warp_pixel<C>(img, m, g, Ws, j0 + e, i, border, rx0, ry0, rx1, ry1, val[e]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (VEC) {
            const f32x4 o = {val[0][c], val[1][c], val[2][c], val[3][c]};
            *reinterpret_cast<f32x4*>(out + c * plane) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e < Wo) out[c * plane + e] = val[e][c];
        }
    }
}

template <int C>
static int warp_launch(const unsigned char* frames, float* y, const float* M, const float* gain, int N, int Hs, int Ws, int Ho,
                       int Wo, int border, int rx0, int ry0, int rx1, int ry1, hipStream_t stream) {
    const int G = (Wo + 3) / 4;
    const bool vec = (Wo % 4) == 0 && (reinterpret_cast<unsigned long long>(y) & 15ull) == 0;
    const unsigned gx = (unsigned)(((long long)Ho * G + WARP_THREADS - 1) / WARP_THREADS);
    const long long in_img = (long long)Hs * Ws * C, out_img = (long long)C * Ho * Wo;
    for (int n0 = 0; n0 < N; n0 += 65535) {                          // (grid.y holds at most 65535 images)
        const int nb = N - n0 < 65535 ? N - n0 : 65535;
        const unsigned char* f = frames + n0 * in_img;
        float* o = y + n0 * out_img;
        const float* mm = M + 9LL * n0;
        if (vec)
            YOLO_LAUNCH((warp_u8_to_nchw_kernel<C, true>), dim3(gx, nb), dim3(WARP_THREADS), 0, stream, f, o, mm, gain, Hs, Ws, Ho,
                        Wo, G, border, rx0, ry0, rx1, ry1);
        else
            YOLO_LAUNCH((warp_u8_to_nchw_kernel<C, false>), dim3(gx, nb), dim3(WARP_THREADS), 0, stream, f, o, mm, gain, Hs, Ws, Ho,
                        Wo, G, border, rx0, ry0, rx1, ry1);
        YOLO_LAUNCH_CHECK();
    }
    return YOLO_OK;
}

extern "C" int yolo_warp_u8_to_nchw(const unsigned char* frames, float* y, const float* M, const float* gain, int N, int Hs,
                                    int Ws, int C, int Ho, int Wo, int border, int roi_x0, int roi_y0, int roi_x1, int roi_y1,
                                    void* stream) {
    if (!frames || !y || !M) return YOLO_EINVAL;
    if (N <= 0 || Hs <= 0 || Ws <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return YOLO_EINVAL;
    if (roi_x0 < 0 || roi_y0 < 0 || roi_x1 >= Ws || roi_y1 >= Hs || roi_x1 < roi_x0 || roi_y1 < roi_y0) return YOLO_EINVAL;
    if (C > WARP_MAX_C || (border != 0 && border != 1)) return YOLO_EUNSUPPORTED;
    // one image's thread index and one source row's byte offset are 32-bit in the kernel
    if ((long long)Ho * ((Wo + 3) / 4) > 0x7fffff00LL || (long long)Ws * C > 0x7fffffffLL) return YOLO_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: return warp_launch<1>(frames, y, M, gain, N, Hs, Ws, Ho, Wo, border, roi_x0, roi_y0, roi_x1, roi_y1, s);
        case 2: return warp_launch<2>(frames, y, M, gain, N, Hs, Ws, Ho, Wo, border, roi_x0, roi_y0, roi_x1, roi_y1, s);
        case 3: return warp_launch<3>(frames, y, M, gain, N, Hs, Ws, Ho, Wo, border, roi_x0, roi_y0, roi_x1, roi_y1, s);
        default: return warp_launch<4>(frames, y, M, gain, N, Hs, Ws, Ho, Wo, border, roi_x0, roi_y0, roi_x1, roi_y1, s);
    }
}
