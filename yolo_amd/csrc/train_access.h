// Element access for the kernels that walk NHWC tensors of any activation type (bn_train.hip, train_ops.hip, elementwise.hip):
// values in and out as fp32, eight channels or one at a time, single-plane and split storage behind the same names.
#pragma once
#include "common.h"

// 8-channel vector access for NHWC tensors of either element type
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&v)[8]) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float (&v)[8]) {
    const uint4 u = *(const uint4*)p;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[2 * q] = bf16_bits_to_f32(w[q] & 0xffffu); v[2 * q + 1] = bf16_bits_to_f32(w[q] >> 16); }
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&v)[8]) {
    f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    *(f32x4*)p = a; *(f32x4*)(p + 4) = b;
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float (&v)[8]) {
    *(uint4*)p = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}
template <typename T> __device__ __forceinline__ float load1(const T* p);
template <> __device__ __forceinline__ float load1<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float load1<bf16_t>(const bf16_t* p) { return bf16_bits_to_f32(p->bits); }
template <typename T> __device__ __forceinline__ void store1(T* p, float v);
template <> __device__ __forceinline__ void store1<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store1<bf16_t>(bf16_t* p, float v) { p->bits = (uint16_t)f32_to_bf16_bits(v); }

// The same accesses on a split tensor (YOLO_BF16X3): a value is READ as hi + lo in fp32 and STORED as hi = bf16_rne(v),
// lo = bf16_rne(v - hi); its lo plane sits `lo` elements behind the hi plane.  For the single-plane types `lo` is not used.
// dense_ps / dense_lo: pixel stride and lo offset of a dense (N,H,W,C) tensor (split: per pixel round_up(C, 32) hi values, then
// as many lo values; the pad channels are never read or written here).
template <typename T> __host__ __device__ __forceinline__ long long dense_ps(int C) { return IsSplit<T>::value ? 2LL * round_up(C, 32) : C; }
template <typename T> __host__ __device__ __forceinline__ int dense_lo(int C) { return IsSplit<T>::value ? round_up(C, 32) : 0; }
// element offset of channel c of pixel `pix` in a dense tensor of C channels; for the single-plane types that is the flat index
// i = pix * C + c the caller split into (pix, c), taken as it is
template <typename T> __device__ __forceinline__ long long dense_at(long long i, long long pix, int c, int C) {
    return IsSplit<T>::value ? pix * dense_ps<T>(C) + c : i;
}
// bytes an HBM pass moves per value (the BatchNorm partition)
template <typename T> constexpr int value_bytes() { return IsSplit<T>::value ? 4 : (int)sizeof(T); }
__device__ __forceinline__ uint32_t split_lo_bf16x2(float a, float b, uint32_t hi) {
    return pack_bf16x2(a - bf16_bits_to_f32(hi & 0xffffu), b - bf16_bits_to_f32(hi >> 16));
}
template <typename T> __device__ __forceinline__ void load8s(const T* p, int, float (&v)[8]) { load8<T>(p, v); }
template <> __device__ __forceinline__ void load8s<bf16x3_t>(const bf16x3_t* p, int lo, float (&v)[8]) {
    float h[8], l[8];
    load8<bf16_t>((const bf16_t*)p, h);
    load8<bf16_t>((const bf16_t*)p + lo, l);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = h[e] + l[e];
}
template <typename T> __device__ __forceinline__ void store8s(T* p, int, const float (&v)[8]) { store8<T>(p, v); }
template <> __device__ __forceinline__ void store8s<bf16x3_t>(bf16x3_t* p, int lo, const float (&v)[8]) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { h[q] = pack_bf16x2(v[2 * q], v[2 * q + 1]); l[q] = split_lo_bf16x2(v[2 * q], v[2 * q + 1], h[q]); }
    *(uint4*)p = make_uint4(h[0], h[1], h[2], h[3]);
    *(uint4*)((bf16_t*)p + lo) = make_uint4(l[0], l[1], l[2], l[3]);
}
template <typename T> __device__ __forceinline__ float load1s(const T* p, int) { return load1<T>(p); }
template <> __device__ __forceinline__ float load1s<bf16x3_t>(const bf16x3_t* p, int lo) {
    return bf16_bits_to_f32(p->bits) + bf16_bits_to_f32(p[lo].bits);
}
template <typename T> __device__ __forceinline__ void store1s(T* p, int, float v) { store1<T>(p, v); }
template <> __device__ __forceinline__ void store1s<bf16x3_t>(bf16x3_t* p, int lo, float v) {
    const uint32_t h = f32_to_bf16_bits(v);
    p->bits = (uint16_t)h;
    p[lo].bits = (uint16_t)f32_to_bf16_bits(v - bf16_bits_to_f32(h));
}

// Eight channels MOVED, not computed with (the dilation): between load8m and store8m the single-plane types hold them as the fp32
// values of load8 / store8; a split value keeps both of its stored halves as they are -- hi + lo -> fp32 -> hi', lo' does not
// always give the same pair back.  `typename Moved8<T>::type v; zero8m(v);` starts from zeros.
template <typename T> struct Moved8 { typedef float type[8]; };
template <> struct Moved8<bf16x3_t> { typedef uint4 type[2]; };
__device__ __forceinline__ void zero8m(float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
}
__device__ __forceinline__ void zero8m(uint4 (&v)[2]) { v[0] = v[1] = make_uint4(0, 0, 0, 0); }
template <typename T> __device__ __forceinline__ void load8m(const T* p, int, float (&v)[8]) { load8<T>(p, v); }
__device__ __forceinline__ void load8m(const bf16x3_t* p, int lo, uint4 (&v)[2]) { v[0] = *(const uint4*)p; v[1] = *(const uint4*)(p + lo); }
template <typename T> __device__ __forceinline__ void store8m(T* p, int, const float (&v)[8]) { store8<T>(p, v); }
__device__ __forceinline__ void store8m(bf16x3_t* p, int lo, const uint4 (&v)[2]) { *(uint4*)p = v[0]; *(uint4*)(p + lo) = v[1]; }
