// What the two plate renderers share (plates.hip: the 6-D projected plate of LPGenerator.add; ocr_data.hip: the OCR batch of
// LPGenerator.render): the parameter row, the "no plate" rule, the sample S through the row's map, and the Philox / Irwin-Hall
// noise.  Both units are compiled with -ffp-contract=off; the arithmetic is the op-by-op fp32 definition of include/yolo_amd.h
// (yolo_plate_render).
#pragma once
#include "common.h"
#include "render_sample.h"

constexpr int PLATE_H = 160, PLATE_W = 380;               // the plate image (draw_LP)
constexpr int GLYPH_COUNT = 34;

struct PlateRow {                                         // YOLO_PLATE_ROW_WORDS 32-bit words (include/yolo_amd.h)
    int has;
    int glyph[7];
    int l, t, r, b;
    uint32_t k0, k1;
    float s;
    int pad;
    float m[9];
    float w0, w1;
    float A[9], D[9], e[3];
};
static_assert(sizeof(PlateRow) == 4 * YOLO_PLATE_ROW_WORDS, "the parameter row is YOLO_PLATE_ROW_WORDS words");

// "no plate": the flag is off, or a glyph id does not name a glyph of the atlas -- then nothing is composed, sampled or blended
__device__ __forceinline__ bool plate_ok(const PlateRow& R) {
    bool ok = R.has != 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) ok = ok && R.glyph[k] >= 0 && R.glyph[k] < GLYPH_COUNT;
    return ok;
}

// S(x, y): the four channels of the plate seen through the map m at output position (column x, row y), any position inside or
// outside the canvas; 0 where the map's denominator is not a positive finite number.
__device__ __forceinline__ void plate_sample(const unsigned char* plate, const float* m, float x, float y, float* val) {
    const float nx = (m[0] * x + m[1] * y) + m[2];
    const float ny = (m[3] * x + m[4] * y) + m[5];
    const float den = (m[6] * x + m[7] * y) + m[8];
    const bool front = den > 0.f && den < __builtin_huge_valf();       // (false for a NaN)
    // the tap's addresses are clamped whatever nx / den is, so it is taken anyway and dropped: no divergent branch
    render_tap(plate, PLATE_H, PLATE_W, nx / den, ny / den, val);
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = front ? val[c] : 0.f;
}

// Philox4x32-10 (Salmon et al., SC11; the Random123 constants): counter c[4], key (k0, k1) -> c[4]
__device__ __forceinline__ void philox4x32_10(uint32_t* c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// the sum of the 8 bytes of two words, less its mean 1020: an 8-term Irwin-Hall variate, an integer in -1020..1020
__device__ __forceinline__ float plate_noise_z(uint32_t a, uint32_t b) {
    const uint32_t t = __builtin_amdgcn_sad_u8(b, 0u, __builtin_amdgcn_sad_u8(a, 0u, 0u));
    return (float)((int)t - 1020);
}

// the noise rule of yolo_plate_render on the four channels q of canvas pixel (column j, row i): two Philox calls with counters
// (j, i, 0, 0) and (j, i, 1, 0), q_c = min(max(q_c + z_c * s, 0), 255)
__device__ __forceinline__ void plate_noise(float* q, int j, int i, float s, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t c[4] = {(uint32_t)j, (uint32_t)i, (uint32_t)h, 0u};
        philox4x32_10(c, k0, k1);
        const float z0 = plate_noise_z(c[0], c[1]), z1 = plate_noise_z(c[2], c[3]);
        q[2 * h] = fminf(fmaxf(q[2 * h] + z0 * s, 0.f), 255.f);
        q[2 * h + 1] = fminf(fmaxf(q[2 * h + 1] + z1 * s, 0.f), 255.f);
    }
}
