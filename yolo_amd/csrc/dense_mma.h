// The MFMA fragment types of the DenseNet kernels (dense.hip, dense_train.hip): one 16 x 16 x 32 step of a dense operand image
// against 8 channels of one pixel per lane, and the folded BN + ReLU in front of it.
#pragma once
#include "common.h"

// 8 K-elements of one lane: the A or B fragment of one 16 x 16 x 32 step
template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
    uint4 v;
    __device__ __forceinline__ void load(const void* p) { v = *(const uint4*)p; }
    __device__ __forceinline__ void unpack(float (&f)[8]) const {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[2 * i] = bf16_bits_to_f32(w[i] & 0xffffu); f[2 * i + 1] = bf16_bits_to_f32(w[i] >> 16); }
    }
    __device__ __forceinline__ void pack(const float (&f)[8]) {
        v = make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
    }
    __device__ __forceinline__ void zero() { v = make_uint4(0, 0, 0, 0); }
};
template <> struct Frag<float> {
    float4 a, b;
    __device__ __forceinline__ void load(const void* p) { a = ((const float4*)p)[0]; b = ((const float4*)p)[1]; }
    __device__ __forceinline__ void unpack(float (&f)[8]) const {
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    }
    __device__ __forceinline__ void pack(const float (&f)[8]) { a = make_float4(f[0], f[1], f[2], f[3]); b = make_float4(f[4], f[5], f[6], f[7]); }
    __device__ __forceinline__ void zero() { a = make_float4(0, 0, 0, 0); b = a; }
};
__device__ __forceinline__ f32x4 mma(const Frag<bf16_t>& a, const Frag<bf16_t>& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a.v), __builtin_bit_cast(bf16x8, b.v), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const Frag<float>& a, const Frag<float>& b, f32x4 c) {
    float fa[8], fb[8];
    a.unpack(fa);
    b.unpack(fb);
#pragma unroll
    for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[j], fb[j], c, 0, 0, 0);      // lane's k of step j: 8 (l >> 4) + j, as above
    return c;
}

// max(0, x s + t) on the 8 channels c0 .. c0 + 7 of one pixel, channels >= C selected to zero
__device__ __forceinline__ void bn_relu8(float (&f)[8], const float* s, const float* t, int c0, int C) {
    const float4 s0 = *(const float4*)(s + c0), s1 = *(const float4*)(s + c0 + 4);
    const float4 t0 = *(const float4*)(t + c0), t1 = *(const float4*)(t + c0 + 4);
    const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = fmaxf(f[j] * sv[j] + tv[j], 0.f);
        f[j] = (c0 + j < C) ? v : 0.f;                    // a select: the masked value may be NaN
    }
}

static inline bool too_large(long long elems, int es) { return elems * es >= (1LL << 31); }
