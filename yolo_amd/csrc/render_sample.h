// What the two device renderers share (render.hip: cars from the sprite atlas; plates.hip: licence plates): the bilinear tap over
// 4-byte RGBA pixels and the 3x3 separable blur over four adjacent columns.  Both units are compiled with -ffp-contract=off; the
// arithmetic is the op-by-op fp32 definition of include/yolo_amd.h (yolo_render_cars).
#pragma once
#include "common.h"

constexpr float RENDER_IDX_LIMIT = 1073741824.f;          // 2^30: tap indices are clamped here before the int conversion

// The four channels of the sample at level position (sx, sy): bilinear over 4-byte RGBA pixels, one 32-bit load per tap.  Every
// tap ADDRESS is clamped into the level, so no load leaves it whatever the position is; a tap whose index was outside reads 0.
__device__ __forceinline__ void render_tap(const unsigned char* __restrict__ level, int h, int w, float sx, float sy, float* val) {
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    // (fmaxf / fminf return the other operand for a NaN: a NaN coordinate indexes far outside, and the value is NaN through fx)
    const int x0 = (int)fminf(fmaxf(x0f, -RENDER_IDX_LIMIT), RENDER_IDX_LIMIT), x1 = x0 + 1;
    const int y0 = (int)fminf(fmaxf(y0f, -RENDER_IDX_LIMIT), RENDER_IDX_LIMIT), y1 = y0 + 1;
    const int cx0 = min(max(x0, 0), w - 1), cx1 = min(max(x1, 0), w - 1);
    const int cy0 = min(max(y0, 0), h - 1), cy1 = min(max(y1, 0), h - 1);
    const bool inx0 = cx0 == x0, inx1 = cx1 == x1, iny0 = cy0 == y0, iny1 = cy1 == y1;
    const uint32_t* px = reinterpret_cast<const uint32_t*>(level);
    const long long r0 = (long long)cy0 * w, r1 = (long long)cy1 * w;
    const uint32_t pa = (inx0 && iny0) ? px[r0 + cx0] : 0u;
    const uint32_t pb = (inx1 && iny0) ? px[r0 + cx1] : 0u;
    const uint32_t pc = (inx0 && iny1) ? px[r1 + cx0] : 0u;
    const uint32_t pd = (inx1 && iny1) ? px[r1 + cx1] : 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float ta = (float)((pa >> (8 * c)) & 255u), tb = (float)((pb >> (8 * c)) & 255u);
        const float tc = (float)((pc >> (8 * c)) & 255u), td = (float)((pd >> (8 * c)) & 255u);
        const float top = ta + fx * (tb - ta);
        const float bot = tc + fx * (td - tc);
        val[c] = top + fy * (bot - top);
    }
}

// RGBA 0..255 of output pixels (j0..j0+3, i) before the colour map; sample(x, y, val) gives S at output position (x, y).
// w1 == 0 (uniform per image): the sample itself.  Otherwise the separable 3x3 sum in a fixed order: rows i-1, i, i+1 each as
// (w1 S(j-1) + w0 S(j)) + w1 S(j+1), then the same over the rows.  The six columns j0-1..j0+4 of a row are sampled once and
// shared by the four pixels (the same values, so the same bits).
template <class Sample>
__device__ __forceinline__ void render_blur_quad(const Sample& sample, float w0, float w1, int j0, int i, float (*px)[4]) {
    if (w1 == 0.f) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sample((float)(j0 + e), (float)i, px[e]);
        return;
    }
    // (one row at a time, not unrolled: the three rows' 72 taps in flight at once cost ~170 VGPRs and half the resident waves)
#pragma unroll 1
    for (int dy = 0; dy < 3; ++dy) {
        float s[6][4];
#pragma unroll
        for (int k = 0; k < 6; ++k) sample((float)(j0 - 1 + k), (float)(i - 1 + dy), s[k]);
        const float wy = dy == 1 ? w0 : w1;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float row = (w1 * s[e][c] + w0 * s[e + 1][c]) + w1 * s[e + 2][c];
                px[e][c] = dy == 0 ? wy * row : px[e][c] + wy * row;
            }
    }
}

// One thread's four columns of the three planes at `p` (element `base`, planes `plane` apart): 16-byte accesses when VEC, scalar
// ones that stop at column W otherwise (a column past W reads 0).
template <bool VEC>
__device__ __forceinline__ void render_load_planes(const float* p, long long base, long long plane, int j0, int W, float (*b)[4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (VEC) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + base + c * plane);
#pragma unroll
            for (int e = 0; e < 4; ++e) b[c][e] = t[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) b[c][e] = (j0 + e < W) ? p[base + c * plane + e] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void render_store_planes(float* p, long long base, long long plane, int j0, int W, const float (*o)[4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (VEC) {
            const f32x4 t = {o[c][0], o[c][1], o[c][2], o[c][3]};
            *reinterpret_cast<f32x4*>(p + base + c * plane) = t;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e < W) p[base + c * plane + e] = o[c][e];
        }
    }
}
