// Weight gradient of the convolutions for gfx950 (everything but the row-walk / LDS-DMA kernels of wgrad_walk.hip): the fp32
// parity kernel (MFMA 32x32x2 f32), the bf16 per-tap / strip / row-group kernels, the split (YOLO_BF16X3) per-tap kernel, their
// launchers (one for both per-tap kernels) and the yolo_conv_wgrad* entry points (bf16: ids -> families, then the ladder strip,
// row groups, per-tap).
#include "common.h"
#include <stdlib.h>
#include "conv_args.h"
#include "train_access.h"
#include "wgrad_walk.h"

// ------------------------------------------------------------------------------------------------
// Weight gradient: dW[co][ci][kh][kw] += sum_p dy[p][co] * x[p @ tap][ci]   (fp32, MFMA 32x32x2)
// ------------------------------------------------------------------------------------------------
// One wave = one (32 cout x 32 cin) tile of one tap over a slice of the stacked output rows; the MFMA
// contracts 2 output pixels per step (lane half h = pixel parity).  D[i = cout][j = cin].
// Partial sums are added atomically (caller zero-fills dW).
__global__ __launch_bounds__(256) void wgrad_f32_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                        float* __restrict__ dw, int N, int H, int W, int Cin, int Ho,
                                                        int Wo, int Cout, int ks, int stride, long long dy_ps,
                                                        int tiles_ci, int rows_per_slice) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x;
    const int tci = tile % tiles_ci, tco = tile / tiles_ci;
    const int tap = blockIdx.y;
    const int kh = tap / ks, kw = tap - kh * ks;
    const int pad = ks / 2;
    const int co = tco * 32 + l31, ci = tci * 32 + l31;
    const bool co_ok = co < Cout, ci_ok = ci < Cin;
    const long long slice = (long long)blockIdx.z * 4 + wave;
    const long long r0 = slice * rows_per_slice;
    const long long r1 = min(r0 + rows_per_slice, (long long)N * Ho);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const int n = (int)(r / Ho), oy = (int)(r - (long long)n * Ho);
        const int iy = oy * stride + kh - pad;
        if (iy < 0 || iy >= H) continue;                                   // wave-uniform
        const float* dyr = dy + r * Wo * dy_ps;
        const float* xr = x + ((long long)n * H + iy) * W * Cin;
        for (int ox0 = 0; ox0 < Wo; ox0 += 2) {
            const int ox = ox0 + h;
            const int ix = ox * stride + kw - pad;
            const bool ok = ox < Wo && ix >= 0 && ix < W;
            const float a = (ok && co_ok) ? dyr[(long long)ox * dy_ps + co] : 0.f;
            const float b = (ok && ci_ok) ? xr[(long long)ix * Cin + ci] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    if (!ci_ok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int oc = tco * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (oc < Cout) atomicAdd(&dw[(((long long)oc * Cin + ci) * ks + kh) * ks + kw], acc[r]);
    }
}

static int yolo_conv_wgrad_f32(const float* dy, const float* x, float* dw_oihw, int N, int H, int W, int Cin,
                                   int Cout, int ksize, int stride, long long dy_pixel_stride, void* stream) {
    if (!dy || !x || !dw_oihw || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return YOLO_EINVAL;
    if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2)) return YOLO_EUNSUPPORTED;
    const int pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const int tiles_ci = (Cin + 31) / 32, tiles_co = (Cout + 31) / 32;
    const long long rows = (long long)N * Ho;
    // enough K-slices to fill the chip: ~2048 waves in flight
    const long long tiles = (long long)tiles_ci * tiles_co * ksize * ksize;
    long long slices = (4096 + tiles - 1) / tiles;
    if (slices < 1) slices = 1;
    if (slices > rows) slices = rows;
    slices = (slices + 3) / 4 * 4;
    const int rps = (int)((rows + slices - 1) / slices);
    const long long ps = dy_pixel_stride ? dy_pixel_stride : Cout;
    YOLO_LAUNCH(wgrad_f32_kernel, dim3((unsigned)(tiles_ci * tiles_co), ksize * ksize, (unsigned)(slices / 4)),
                dim3(256), 0, (hipStream_t)stream, dy, x, dw_oihw, N, H, W, Cin, Ho, Wo, Cout, ksize, stride, ps,
                tiles_ci, rps);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// ------------------------------------------------------------------------------------------------
// bf16 weight gradient: MFMA 32x32x16 with K = output pixels.  Both operands live in HBM/LDS as
// [pixel][channel] (NHWC), i.e. K is the STRIDED axis -- exactly the case gfx950's transposing LDS read
// ds_read_b64_tr_b16 exists for: a 16-lane group supplies a 4(k) x 16(channel) block as 8-byte row pieces and
// every lane receives 4 consecutive k of ONE channel (semantics probed on hardware: tools/probes/).
// Block = 128 cout x 128 cin x one tap, 4 waves (64x64 each), 64 pixels per K-chunk staged through registers
// into LDS rows padded to 288 B (conflict-free transposing reads).  Result layout [tap][Cout][Cin] fp32
// (coalesced; atomics only when the pixel range is split), folded into OIHW by wgrad_finish_kernel.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
#ifndef YOLO_WG_KC
#define YOLO_WG_KC 64
#endif
constexpr int WG_KC = YOLO_WG_KC;      // pixels per K-chunk

template <int PITCH>
__device__ __forceinline__ uint4 tr_frag(const char* tile, int krow0, int col0, int lane) {
    // 8 consecutive k (pixels) of channel (col0 + (lane&15) + 16*((lane>>4)&1)), k = krow0 + 8*(lane>>5) ...
    const int g = lane >> 4, j = lane & 15;
    const int krow = krow0 + (g >> 1) * 8 + (j >> 2);
    const int col = col0 + (g & 1) * 16 + 4 * (j & 3);
    const char* p = tile + krow * PITCH + col * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * PITCH));
    const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
    return make_uint4(a.x, a.y, b.x, b.y);
}

// Block = (MI*64) cout x (NI*64) cin x one tap, 4 waves (2 x 2, wave tile MI*32 x NI*32).  The loop is paced by the
// global-load latency of the next chunk (registers -> LDS, one chunk ahead), so the wider tiles, which do 2-4x the
// MFMA work per loaded byte and per barrier, are what the big layers use; 128 x 128 remains for small Cin/Cout.
template <int MI, int NI>
__global__ __launch_bounds__(256) void wgrad_bf16_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
                                                         float* __restrict__ dwt, int N, int H, int W, int Cin, int Ho,
                                                         int Wo, int Cout, int ks, int stride, long long dy_ps,
                                                         int tiles_ci, int chunks_per_slice, int use_atomic,
                                                         FastDiv d_howo, FastDiv d_wo) {
    constexpr int BM = MI * 64, BN = NI * 64;
    constexpr int PA = BM * 2 + 32, PB = BN * 2 + 32;            // LDS pitches (padded: conflict-free transposing reads)
    constexpr int UA = WG_KC * (BM / 8) / 256, UB = WG_KC * (BN / 8) / 256;   // 16-byte units per thread per chunk
    __shared__ __attribute__((aligned(16))) char smem[WG_KC * (PA + PB)];
    char* dyl = smem;
    char* xl = smem + WG_KC * PA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int tile = blockIdx.x;
    const int tci = tile % tiles_ci, tco = tile / tiles_ci;
    const int co0 = tco * BM, ci0 = tci * BN;
    const int tap = blockIdx.y, kh = tap / ks, kw = tap - kh * ks, pad = ks / 2;
    const long long P = (long long)N * Ho * Wo;
    const long long c_first = (long long)blockIdx.z * chunks_per_slice;
    const long long c_last = min(c_first + chunks_per_slice, (P + WG_KC - 1) / WG_KC);
    uint4 dr[UA], xr[UB];
    // Unconditional range-checked buffer loads: a unit that must read zeros (past the pixel range, channel tail, padding)
    // gets an out-of-range offset.  (Predicated loads -- zero-initialise, exec branch, load -- cost the branch and make the
    // compiler wait for every outstanding load before each zero-initialisation.)  dy: a per-chunk base + loop-invariant lane
    // offsets; x: offsets from the tensor start (the host checks that it is < 4 GiB).
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    int d_off[UA];
#pragma unroll
    for (int j = 0; j < UA; ++j) {
        const int u = tid + j * 256;
        const int px = u / (BM / 8), part = u % (BM / 8);
        d_off[j] = (co0 + part * 8 < Cout) ? (int)((px * dy_ps + part * 8) * 2) : -1;
    }
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)0xffffffffu, 0x00020000);
    auto load_chunk = [&](long long c) {
        const long long p0 = c * WG_KC;
        const int left = (int)min((long long)WG_KC, P - p0);                 // live pixels of this chunk
        const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc((void*)(dy + p0 * dy_ps + co0), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int j = 0; j < UA; ++j) {
            const int u = tid + j * 256;
            const int px = u / (BM / 8);
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs_d, px < left ? d_off[j] : -1, 0, 0);
            dr[j] = make_uint4(v.x, v.y, v.z, v.w);
        }
#pragma unroll
        for (int j = 0; j < UB; ++j) {
            const int u = tid + j * 256;
            const int px = u / (BN / 8), part = u % (BN / 8);
            const int p = (int)p0 + px;
            // pixel -> (image, row, column) by multiply-shift (a 64-bit division here cost more than the MFMAs)
            const int n = fdiv(p, d_howo);
            const int rem = p - n * Ho * Wo;
            const int oy = fdiv(rem, d_wo), ox = rem - oy * Wo;
            const int iy = oy * stride + kh - pad, ix = ox * stride + kw - pad;
            const bool ok = px < left && ci0 + part * 8 < Cin && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const unsigned off = ((unsigned)((n * H + iy) * W + ix) * (unsigned)Cin + (unsigned)(ci0 + part * 8)) * 2u;
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? (int)off : -1, 0, 0);
            xr[j] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    if (c_first < c_last) load_chunk(c_first);
    for (long long c = c_first; c < c_last; ++c) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < UA; ++j) {
            const int u = tid + j * 256;
            *(uint4*)(dyl + (u / (BM / 8)) * PA + (u % (BM / 8)) * 16) = dr[j];
        }
#pragma unroll
        for (int j = 0; j < UB; ++j) {
            const int u = tid + j * 256;
            *(uint4*)(xl + (u / (BN / 8)) * PB + (u % (BN / 8)) * 16) = xr[j];
        }
        __syncthreads();
        if (c + 1 < c_last) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < WG_KC / 16; ++kk) {
            uint4 af[MI], bf[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) af[mi] = tr_frag<PA>(dyl, kk * 16, (wm * MI + mi) * 32, lane);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) bf[ni] = tr_frag<PB>(xl, kk * 16, (wn * NI + ni) * 32, lane);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[mi]),
                                                                          __builtin_bit_cast(bf16x8, bf[ni]), acc[mi][ni],
                                                                          0, 0, 0);
        }
    }
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int ci = ci0 + (wn * NI + ni) * 32 + l31;
            if (ci >= Cin) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wm * MI + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co >= Cout) continue;
                float* dst = dwt + ((long long)tap * Cout + co) * Cin + ci;
                if (use_atomic) atomicAdd(dst, acc[mi][ni][r]);
                else *dst = acc[mi][ni][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------
// SPLIT weight gradient (YOLO_BF16X3): the per-tap kernel above on (hi, lo) pairs.  dy and x each come as two bf16 planes;
// a K-chunk of SWG_KC pixels stages BOTH planes of both operands in LDS, and every fragment pair issues three MFMAs,
// dy_hi x_hi + dy_hi x_lo + dy_lo x_hi (the dy_lo x_lo term, 2^-16 of a product, is dropped -- the split convolution's
// own rule), accumulated in fp32.  Block = (MI*64) cout x (NI*64) cin x one tap, 4 waves; result [tap][Cout][Cin] fp32
// (atomics when the pixel range is split), folded into OIHW by wgrad_finish_kernel.  32 pixels per chunk: four planes
// of 64 pixels would take 72 KB of LDS at 128 x 128 and halve the resident blocks.
// ------------------------------------------------------------------------------------------------
constexpr int SWG_KC = 32;

template <int MI, int NI>
__global__ __launch_bounds__(256) void wgrad_split_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
                                                          float* __restrict__ dwt, int N, int H, int W, int Cin, int Ho,
                                                          int Wo, int Cout, int ks, int stride, long long dy_ps, int dy_lo,
                                                          long long x_ps, int x_lo, int tiles_ci, int chunks_per_slice,
                                                          int use_atomic, FastDiv d_howo, FastDiv d_wo) {
    constexpr int BM = MI * 64, BN = NI * 64;
    constexpr int PA = BM * 2 + 32, PB = BN * 2 + 32;            // LDS pitches (padded: conflict-free transposing reads)
    constexpr int UA = SWG_KC * (BM / 8) / 256, UB = SWG_KC * (BN / 8) / 256;   // 16-byte units per thread, plane and chunk
    static_assert(UA >= 1 && UB >= 1, "tile too small for the chunk");
    __shared__ __attribute__((aligned(16))) char smem[2 * SWG_KC * (PA + PB)];
    char* dyh = smem;
    char* dyl = smem + SWG_KC * PA;
    char* xh = smem + 2 * SWG_KC * PA;
    char* xl = xh + SWG_KC * PB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int tile = blockIdx.x;
    const int tci = tile % tiles_ci, tco = tile / tiles_ci;
    const int co0 = tco * BM, ci0 = tci * BN;
    const int tap = blockIdx.y, kh = tap / ks, kw = tap - kh * ks, pad = ks / 2;
    const long long P = (long long)N * Ho * Wo;
    const long long c_first = (long long)blockIdx.z * chunks_per_slice;
    const long long c_last = min(c_first + chunks_per_slice, (P + SWG_KC - 1) / SWG_KC);
    uint4 drh[UA], drl[UA], xrh[UB], xrl[UB];
    // range-checked buffer loads as in wgrad_bf16_kernel: a unit that must read zeros gets an out-of-range offset (-1)
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    int d_off[UA];
#pragma unroll
    for (int j = 0; j < UA; ++j) {
        const int u = tid + j * 256;
        const int px = u / (BM / 8), part = u % (BM / 8);
        d_off[j] = (co0 + part * 8 < Cout) ? (int)((px * dy_ps + part * 8) * 2) : -1;
    }
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)0xffffffffu, 0x00020000);
    auto load_chunk = [&](long long c) {
        const long long p0 = c * SWG_KC;
        const int left = (int)min((long long)SWG_KC, P - p0);                // live pixels of this chunk
        const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc((void*)(dy + p0 * dy_ps + co0), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int j = 0; j < UA; ++j) {
            const int u = tid + j * 256;
            const bool ok = u / (BM / 8) < left && d_off[j] >= 0;
            const u32x4_t a = __builtin_amdgcn_raw_buffer_load_b128(rs_d, ok ? d_off[j] : -1, 0, 0);
            const u32x4_t b = __builtin_amdgcn_raw_buffer_load_b128(rs_d, ok ? d_off[j] + dy_lo * 2 : -1, 0, 0);
            drh[j] = make_uint4(a.x, a.y, a.z, a.w);
            drl[j] = make_uint4(b.x, b.y, b.z, b.w);
        }
#pragma unroll
        for (int j = 0; j < UB; ++j) {
            const int u = tid + j * 256;
            const int px = u / (BN / 8), part = u % (BN / 8);
            const int p = (int)p0 + px;
            const int n = fdiv(p, d_howo);
            const int rem = p - n * Ho * Wo;
            const int oy = fdiv(rem, d_wo), ox = rem - oy * Wo;
            const int iy = oy * stride + kh - pad, ix = ox * stride + kw - pad;
            const bool ok = px < left && ci0 + part * 8 < Cin && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const unsigned off = ((unsigned)((n * H + iy) * W + ix) * (unsigned)x_ps + (unsigned)(ci0 + part * 8)) * 2u;
            const u32x4_t a = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? (int)off : -1, 0, 0);
            const u32x4_t b = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? (int)(off + (unsigned)x_lo * 2u) : -1, 0, 0);
            xrh[j] = make_uint4(a.x, a.y, a.z, a.w);
            xrl[j] = make_uint4(b.x, b.y, b.z, b.w);
        }
    };
    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    if (c_first < c_last) load_chunk(c_first);
    for (long long c = c_first; c < c_last; ++c) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < UA; ++j) {
            const int u = tid + j * 256;
            const int o = (u / (BM / 8)) * PA + (u % (BM / 8)) * 16;
            *(uint4*)(dyh + o) = drh[j];
            *(uint4*)(dyl + o) = drl[j];
        }
#pragma unroll
        for (int j = 0; j < UB; ++j) {
            const int u = tid + j * 256;
            const int o = (u / (BN / 8)) * PB + (u % (BN / 8)) * 16;
            *(uint4*)(xh + o) = xrh[j];
            *(uint4*)(xl + o) = xrl[j];
        }
        __syncthreads();
        if (c + 1 < c_last) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < SWG_KC / 16; ++kk) {
            uint4 ah[MI], al[MI], bh[NI], bl[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                ah[mi] = tr_frag<PA>(dyh, kk * 16, (wm * MI + mi) * 32, lane);
                al[mi] = tr_frag<PA>(dyl, kk * 16, (wm * MI + mi) * 32, lane);
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                bh[ni] = tr_frag<PB>(xh, kk * 16, (wn * NI + ni) * 32, lane);
                bl[ni] = tr_frag<PB>(xl, kk * 16, (wn * NI + ni) * 32, lane);
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    acc[mi][ni] = mfma16<bf16_t>(ah[mi], bh[ni], acc[mi][ni]);
                    acc[mi][ni] = mfma16<bf16_t>(ah[mi], bl[ni], acc[mi][ni]);
                    acc[mi][ni] = mfma16<bf16_t>(al[mi], bh[ni], acc[mi][ni]);
                }
        }
    }
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int ci = ci0 + (wn * NI + ni) * 32 + l31;
            if (ci >= Cin) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (wm * MI + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co >= Cout) continue;
                float* dst = dwt + ((long long)tap * Cout + co) * Cin + ci;
                if (use_atomic) atomicAdd(dst, acc[mi][ni][r]);
                else *dst = acc[mi][ni][r];
            }
        }
}

// How a launch cuts the pixel range into slices (grid z): about `target` blocks in all, at least `min_chunks` K-chunks per slice
// because every slice ends in an atomic tile.
//   bf16: 768 = the resident capacity, 3 blocks per CU, and the quotient is rounded DOWN: 774 blocks (one over a full round) cost
//     212 us where 756 take 185.  16 chunks: the atomic tiles dominated the small 1x1 layers (26x26 512->256 at batch 64:
//     60.7 -> 45.5 us; 8 and 32 chunks are worse).
//   split: about three resident rounds of blocks (1536 of the 64 x 64 tile, else 768); 32 chunks = 1024 pixels.
struct TapSlices {
    long long target;
    int min_chunks;
};

template <int MI, int NI, int PLANES>
static void wgrad_tap_launch(const uint16_t* dy, const uint16_t* x, float* ws, int N, int H, int W, int Cin, int Ho, int Wo,
                             int Cout, int ksize, int stride, long long dy_ps, int dy_lo, long long x_ps, int x_lo,
                             TapSlices pol, bool force_atomic, hipStream_t st) {
    constexpr int BM = MI * 64, BN = NI * 64, KC = PLANES == 1 ? WG_KC : SWG_KC;
    const int tiles_ci = (Cin + BN - 1) / BN, tiles_co = (Cout + BM - 1) / BM, taps = ksize * ksize;
    const long long chunks = ((long long)N * Ho * Wo + KC - 1) / KC;
    const long long tiles = (long long)tiles_ci * tiles_co * taps;
    long long slices = pol.target / tiles;
    if (slices > chunks / pol.min_chunks) slices = chunks / pol.min_chunks;
    if (slices < 1) slices = 1;
    const int cps = (int)((chunks + slices - 1) / slices);
    slices = (chunks + cps - 1) / cps;
    const dim3 grid((unsigned)(tiles_ci * tiles_co), taps, (unsigned)slices);
    const int use_atomic = (slices > 1 || force_atomic) ? 1 : 0;
    const FastDiv d_howo = make_fastdiv((unsigned)Ho * Wo), d_wo = make_fastdiv((unsigned)Wo);
    if constexpr (PLANES == 1)
        YOLO_LAUNCH((wgrad_bf16_kernel<MI, NI>), grid, dim3(256), 0, st, dy, x, ws, N, H, W, Cin, Ho, Wo, Cout, ksize, stride,
                    dy_ps, tiles_ci, cps, use_atomic, d_howo, d_wo);
    else
        YOLO_LAUNCH((wgrad_split_kernel<MI, NI>), grid, dim3(256), 0, st, dy, x, ws, N, H, W, Cin, Ho, Wo, Cout, ksize, stride,
                    dy_ps, dy_lo, x_ps, x_lo, tiles_ci, cps, use_atomic, d_howo, d_wo);
}

// ------------------------------------------------------------------------------------------------
// bf16 weight gradient of the early 3x3 layers (Cin <= 64: few output tiles, millions of pixels).  The per-tap
// kernel above re-reads dy and x nine times and pads 32 channels to 128; here ONE WAVE (= one block, no block
// barriers) owns a 32-pixel-wide column strip of one image and walks down its output rows with a rolling window
// of input rows in LDS, so x and dy are read once and all nine taps accumulate from the same staged rows:
// (CO_F*32 cout) x (32 cin) x 9 taps of fp32 accumulators per wave (144 AGPRs at CO_F = 1).
// Next rows are fetched into registers while the current ones feed the MFMAs.  Partial sums of the strips are
// added atomically into the [tap][Cout][Cin] workspace.
// ------------------------------------------------------------------------------------------------
template <int CO_F, int S, int TH>
__global__ __launch_bounds__(64) void wgrad_strip_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
                                                         float* __restrict__ dwt, int N, int H, int W, int Cin, int Ho,
                                                         int Wo, int Cout, long long dy_ps, int tiles_ci, int tiles_co,
                                                         int strips_w, int rows_per_slice, int pair_xcd) {
    constexpr int TW = 32;                          // output pixels per strip row = 2 MFMA K-steps
    constexpr int XW = (TW - 1) * S + 3;            // input pixels per staged row (with halo)
    // LDS pitches (bytes per pixel row).  The fragments come from ds_read_b64_tr_b16: a 16-lane group reads 4 consecutive
    // K rows x 32 bytes and the four groups rows r..r+3 / r+8..r+11 x two 32-byte halves, so a row stride of 64 bytes puts the
    // 512 bytes of a read on every bank exactly twice (the minimum); the 80 the kernel started with made three rows share banks
    // (PMC: a quarter of the wave cycles were LDS bank-conflict cycles).  Stride 2 reads every other pixel: 2 * 80 = 160 = 32 mod
    // 128 spreads almost as well and keeps four blocks per CU.
    constexpr int XP = (S == 1) ? 64 : 80, DP = CO_F * 64;
    constexpr int INUSE = (TH - 1) * S + 3, NEW = S * TH, RING = INUSE + NEW;
    constexpr int XROW = XW * XP, DYB = TH * TW * DP;
    constexpr int XU = (NEW * XW * 4 + 63) / 64, DU = TH * TW * CO_F * 4 / 64;
    __shared__ __attribute__((aligned(16))) char smem[RING * XROW + 2 * DYB];
    char* xl = smem;
    char* dyl = smem + RING * XROW;
    const int lane = threadIdx.x;
    int b = blockIdx.x;
    int tco;
    if (pair_xcd) {
        // the tiles_co blocks that read the same x strip sit 8 apart in launch order: same XCD, same L2, dispatched together
        const int xcd = b & 7, q = b >> 3;
        tco = q % tiles_co;
        b = (q / tiles_co) * 8 + xcd;
    } else {
        tco = b % tiles_co; b /= tiles_co;
    }
    const int tci = b % tiles_ci; b /= tiles_ci;
    const int sw = b % strips_w;
    const int n = b / strips_w;
    const int ci0 = tci * 32, co0 = tco * CO_F * 32;
    const int ox0 = sw * TW, ix0 = ox0 * S - 1;
    const int oy_begin = blockIdx.y * rows_per_slice;
    const int oy_end = min(oy_begin + rows_per_slice, Ho);
    if (oy_begin >= oy_end) return;

    // Staging registers: TWO sets.  A wave is alone on its SIMD (390 registers), so nothing but its own loads in flight hides
    // the HBM latency: the rows of step k + 2 are requested at the top of step k and stored to LDS at the bottom of step k + 1
    // (one set, i.e. a single step of ~0.25 us of MFMA work between request and use, left every step waiting ~1.5 us).
    uint4 xr[2][XU], dr[2][DU];
    // per-lane staging units, loop invariant: byte offset from the step's (wave-uniform) base and the row inside the step, or
    // -1 for a unit that never loads (past the strip / the tensor's columns / the channel tail).  Loads are UNCONDITIONAL
    // buffer loads: a unit that must read zeros gets an out-of-range offset and the hardware returns zeros.  (Predicated
    // loads -- zero-initialise, branch, load -- cost ~20 instructions each and made the compiler wait for ALL outstanding
    // loads before every zero-initialisation; reading a zero page instead makes 75 % of the stem's lanes hit one line: 2-6x slower.)
    int x_off[XU], x_row[XU], d_off[DU], d_row[DU];
#pragma unroll
    for (int j = 0; j < XU; ++j) {
        const int u = lane + j * 64;
        const int r = u / (XW * 4), rem = u - r * (XW * 4), px = rem >> 2, part = rem & 3;
        const int ix = ix0 + px;
        x_row[j] = (r < NEW && ix >= 0 && ix < W && ci0 + part * 8 < Cin) ? r : -1;
        x_off[j] = ((r * W + px) * Cin + part * 8) * 2;
    }
#pragma unroll
    for (int j = 0; j < DU; ++j) {
        const int u = lane + j * 64;
        const int part = u % (CO_F * 4), px = (u / (CO_F * 4)) % TW, t = u / (CO_F * 4 * TW);
        d_row[j] = (ox0 + px < Wo && co0 + part * 8 < Cout) ? t : -1;
        d_off[j] = (int)((((long long)t * Wo + px) * dy_ps + part * 8) * 2);       // (the host bounds TH rows of dy below 2^31 bytes)
    }
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    auto load_x = [&](auto set_c, int iy0) {
        constexpr int SET = decltype(set_c)::value;
        const char* base = (const char*)x + ((((long long)n * H + iy0) * W + ix0) * Cin + ci0) * 2;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            const int iy = iy0 + x_row[j];
            const bool ok = x_row[j] >= 0 && iy >= 0 && iy < H;
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? x_off[j] : -1, 0, 0);
            xr[SET][j] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    int s_row[XU], s_off[XU];                           // (row inside the step, byte offset inside the LDS row)
#pragma unroll
    for (int j = 0; j < XU; ++j) {
        const int u = lane + j * 64;
        const int r = u / (XW * 4), rem = u - r * (XW * 4);
        s_row[j] = r;
        s_off[j] = (rem >> 2) * XP + (rem & 3) * 16;
    }
    auto store_x = [&](auto set_c, int slot0) {
        constexpr int SET = decltype(set_c)::value;
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            int slot = slot0 + s_row[j];
            if (slot >= RING) slot -= RING;
            // (only the last pass has lanes past the NEW rows: the others store without an exec branch)
            if ((j + 1) * 64 <= NEW * XW * 4 || s_row[j] < NEW) *(uint4*)(xl + slot * XROW + s_off[j]) = xr[SET][j];
        }
    };
    auto load_dy = [&](auto set_c, int oy) {
        constexpr int SET = decltype(set_c)::value;
        const char* base = (const char*)dy + ((((long long)n * Ho + oy) * Wo + ox0) * dy_ps + co0) * 2;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int j = 0; j < DU; ++j) {
            const bool ok = d_row[j] >= 0 && oy + d_row[j] < oy_end;
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? d_off[j] : -1, 0, 0);
            dr[SET][j] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    auto store_dy = [&](auto set_c, int buf) {
        constexpr int SET = decltype(set_c)::value;
#pragma unroll
        for (int j = 0; j < DU; ++j) {
            const int u = lane + j * 64;
            const int part = u % (CO_F * 4), px = (u / (CO_F * 4)) % TW, t = u / (CO_F * 4 * TW);
            *(uint4*)(dyl + buf * DYB + (t * TW + px) * DP + part * 16) = dr[SET][j];
        }
    };
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;

    f32x16 acc[CO_F][9];
#pragma unroll
    for (int cf = 0; cf < CO_F; ++cf)
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cf][tp][r] = 0.f;

    // prologue: the input rows the first TH output rows need, and their dy; then the request for step 1 (set 1)
    const int iyb0 = oy_begin * S - 1;
#pragma unroll
    for (int r0 = 0; r0 < INUSE; r0 += NEW) {
        load_x(Set0{}, iyb0 + r0);
        store_x(Set0{}, r0);
    }
    load_dy(Set0{}, oy_begin);
    store_dy(Set0{}, 0);
    // (the requests are UNCONDITIONAL -- past the slice end dy gets out-of-range offsets, x rows that exist are read and
    //  dropped: a uniform branch around them makes the compiler's s_waitcnt for the OTHER set's stores assume the no-load
    //  path, i.e. wait for everything in flight, which turns two sets into one)
    load_x(Set1{}, oy_begin * S - 1 + INUSE);
    load_dy(Set1{}, oy_begin + TH);
    __syncthreads();

    const int g = lane >> 4, j16 = lane & 15;
    const int frag_row = (g >> 1) * 8 + (j16 >> 2), frag_col2 = ((g & 1) * 16 + 4 * (j16 & 3)) * 2;
    const int a_off = frag_row * DP + frag_col2;
    const int b_off = frag_row * S * XP + frag_col2;
    int slot0 = 0, buf = 0;
    // step k = output rows [oy, oy + TH); its parity selects the register set that is FREE at its top (step k's own rows were
    // stored at the bottom of step k - 1) and receives step k + 2; the other set holds step k + 1 and is stored at the bottom
    auto step = [&](auto par_c, int oy) {
        constexpr int PAR = decltype(par_c)::value;
        using Mine = std::integral_constant<int, PAR>;
        using Other = std::integral_constant<int, PAR ^ 1>;
        load_x(Mine{}, (oy + TH) * S - 1 + INUSE);
        load_dy(Mine{}, oy + 2 * TH);
#pragma unroll
        for (int t = 0; t < TH; ++t) {
            int slot[3];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                slot[kh] = slot0 + t * S + kh;
                if (slot[kh] >= RING) slot[kh] -= RING;
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 af[CO_F];
#pragma unroll
                for (int cf = 0; cf < CO_F; ++cf) {
                    const char* p = dyl + buf * DYB + (t * TW + kk * 16) * DP + cf * 64 + a_off;
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * DP));
                    const uint2 a = __builtin_bit_cast(uint2, lo), c = __builtin_bit_cast(uint2, hi);
                    af[cf] = __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, c.x, c.y));
                }
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const char* p = xl + slot[kh] * XROW + (kk * 16 * S + kw) * XP + b_off;
                        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
                        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * S * XP));
                        const uint2 a = __builtin_bit_cast(uint2, lo), c = __builtin_bit_cast(uint2, hi);
                        const bf16x8 bfr = __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, c.x, c.y));
#pragma unroll
                        for (int cf = 0; cf < CO_F; ++cf)
                            acc[cf][kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[cf], bfr, acc[cf][kh * 3 + kw], 0, 0, 0);
                    }
            }
        }
        if (oy + TH < oy_end) {
            int ns = slot0 + INUSE;
            if (ns >= RING) ns -= RING;
            store_x(Other{}, ns);
            store_dy(Other{}, buf ^ 1);
        }
        slot0 += NEW;
        if (slot0 >= RING) slot0 -= RING;
        buf ^= 1;
        __syncthreads();
    };
    for (int oy = oy_begin; oy < oy_end; oy += 2 * TH) {
        step(Set0{}, oy);
        if (oy + TH < oy_end) step(Set1{}, oy + TH);
    }

    const int l31 = lane & 31, h = lane >> 5;
    const int ci = ci0 + l31;
    if (ci >= Cin) return;
#pragma unroll
    for (int cf = 0; cf < CO_F; ++cf)
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + cf * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co < Cout) atomicAdd(dwt + ((long long)tp * Cout + co) * Cin + ci, acc[cf][tp][r]);
            }
}

template <int CO_F, int S, int TH>
static void wgrad_strip_launch(const uint16_t* dy, const uint16_t* x, float* dwt, int N, int H, int W, int Cin, int Ho,
                               int Wo, int Cout, long long ps, hipStream_t st) {
    const int tiles_ci = (Cin + 31) / 32, tiles_co = (Cout + CO_F * 32 - 1) / (CO_F * 32), strips_w = (Wo + 31) / 32;
    const long long bx = (long long)tiles_ci * tiles_co * strips_w * N;
    static const long long tgt = YOLO_LAB_ENV("YOLO_STRIP_TARGET", 1024);
    long long slices = (tgt + bx / 2) / bx;                   // ~4 single-wave blocks per CU resident
    if (slices < 1) slices = 1;
    int rps = (int)((Ho + slices - 1) / slices);
    rps = (rps + TH - 1) / TH * TH;
    slices = (Ho + rps - 1) / rps;
    static const int no_pair = YOLO_LAB_SET("YOLO_STRIP_NO_PAIR") ? 1 : 0;                                       // (ablation knob)
    const int pair_xcd = (!no_pair && tiles_co > 1 && bx % (8 * tiles_co) == 0) ? 1 : 0;
    YOLO_LAUNCH((wgrad_strip_kernel<CO_F, S, TH>), dim3((unsigned)bx, (unsigned)slices), dim3(64), 0, st, dy, x, dwt, N, H,
                W, Cin, Ho, Wo, Cout, ps, tiles_ci, tiles_co, strips_w, rps, pair_xcd);
}

// ------------------------------------------------------------------------------------------------
// bf16 weight gradient of the 3x3 stride-1 layers with many channels on small maps (Wo <= 78).  The per-tap kernel
// is bound by L2 traffic there: every (cout tile, cin tile, tap) block re-reads its dy and x slices, 9x per tile
// pair.  Here a block (4 waves, 64 cout x 64 cin) stages a group of TH whole output rows of one image -- dy and the
// x rows with their halo -- ONCE and accumulates all nine taps from it (9 accumulator tiles of 32x32 per wave,
// 144 AGPRs).  The MFMA K index runs over the TH*Wo pixels of the group in row-major order; because
// ds_read_b64_tr_b16 takes a per-lane row address, a K-step may straddle output rows: each lane's row offsets are
// precomputed per K-step (unused K slots read zero-filled dy rows).  Global loads of the next group are in flight
// in registers while the current group is multiplied.
// ------------------------------------------------------------------------------------------------
template <int TH, int KSTEPS>
__global__ __launch_bounds__(256, 2) void wgrad_rows_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
                                                         float* __restrict__ dwt, int N, int H, int W, int Cin, int Cout,
                                                         long long dy_ps, int tiles_ci, int groups_per_block, int gpi,
                                                         FastDiv d_w, FastDiv d_xw8, FastDiv d_gpi) {
    constexpr int MAXQ = KSTEPS * 16;                   // K slots per group (>= TH*W)
    constexpr int XWMAX = MAXQ / TH + 2;
    constexpr int DP = 144, XP = 144;                   // LDS pitches: 64 channels x 2 B + 16 B pad
    constexpr int XROWS = (TH + 2) * XWMAX;
    constexpr int DU = (MAXQ * 8 + 255) / 256, XU = (XROWS * 8 + 255) / 256;
    __shared__ __attribute__((aligned(16))) char smem[MAXQ * DP + XROWS * XP];
    char* dyl = smem;
    char* xl = smem + MAXQ * DP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int tci = blockIdx.x % tiles_ci, tco = blockIdx.x / tiles_ci;
    const int co0 = tco * 64, ci0 = tci * 64;
    // the block's share of the (image, row group) sequence: gpi groups of TH rows per image
    const int g_begin = blockIdx.y * groups_per_block;
    const int g_end = min(g_begin + groups_per_block, N * gpi);
    if (g_begin >= g_end) return;
    const int XW = W + 2, Q = TH * W;

    // per-thread staging units (loop invariant), packed to keep the kernel at two waves per SIMD:
    //   code = LDS byte offset | row-in-group << 20 | (unit takes part in loads) << 28 ; -1 = unit unused
    int d_code[DU], d_goff[DU];
#pragma unroll
    for (int j = 0; j < DU; ++j) {
        const int u = tid + j * 256, q = u >> 3, part = u & 7;
        const int ty = fdiv(q, d_w), tx = q - ty * W;
        const bool live = q < Q && co0 + part * 8 < Cout;
        d_code[j] = (u < MAXQ * 8) ? (q * DP + part * 16) | (ty << 20) | ((live ? 1 : 0) << 28) : -1;
        d_goff[j] = (int)((ty * W + tx) * dy_ps) + part * 8;
    }
    int x_code[XU], x_goff[XU];
#pragma unroll
    for (int j = 0; j < XU; ++j) {
        const int u = tid + j * 256;
        const int r = fdiv(u, d_xw8), rem = u - r * (XW * 8), px = rem >> 3, part = rem & 7;
        const int ix = px - 1;
        const bool live = ix >= 0 && ix < W && ci0 + part * 8 < Cin;
        x_code[j] = (r < TH + 2) ? ((r * XW + px) * XP + part * 16) | (r << 20) | ((live ? 1 : 0) << 28) : -1;
        x_goff[j] = ((r - 1) * W + ix) * Cin + part * 8;
    }
    uint4 dr[DU], xr[XU];
    auto load_group = [&](int gi) {
        const int n = fdiv(gi, d_gpi);
        const int oy = (gi - n * gpi) * TH;
        const uint16_t* dyn = dy + ((long long)n * H + oy) * W * dy_ps + co0;
        const uint16_t* xn = x + ((long long)n * H + oy) * W * Cin + ci0;
#pragma unroll
        for (int j = 0; j < DU; ++j) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (d_code[j] >= 0 && (d_code[j] >> 28) && oy + ((d_code[j] >> 20) & 0xff) < H)
                v = *(const uint4*)(dyn + d_goff[j]);
            dr[j] = v;
        }
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            uint4 v = make_uint4(0, 0, 0, 0);
            const int iy = oy - 1 + ((x_code[j] >> 20) & 0xff);
            if (x_code[j] >= 0 && (x_code[j] >> 28) && iy >= 0 && iy < H)
                v = *(const uint4*)(xn + x_goff[j]);
            xr[j] = v;
        }
    };
    auto store_group = [&]() {
#pragma unroll
        for (int j = 0; j < DU; ++j)
            if (d_code[j] >= 0) *(uint4*)(dyl + (d_code[j] & 0xfffff)) = dr[j];
#pragma unroll
        for (int j = 0; j < XU; ++j)
            if (x_code[j] >= 0) *(uint4*)(xl + (x_code[j] & 0xfffff)) = xr[j];
    };

    // per-lane fragment row offsets: dy rows are linear in the K slot (one base register), x rows wrap at the
    // row width (lo = k 0..3 of the lane's group, hi = k 4..7)
    const int g = lane >> 4, j16 = lane & 15;
    const int col2 = ((g & 1) * 16 + 4 * (j16 & 3)) * 2;
    const int a_base = ((g >> 1) * 8 + (j16 >> 2)) * DP + wm * 64 + col2;
    int b_off[KSTEPS][2];
#pragma unroll
    for (int s_ = 0; s_ < KSTEPS; ++s_)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int q = s_ * 16 + (g >> 1) * 8 + (j16 >> 2) + 4 * hf;
            const int qq = q < Q ? q : 0;                 // (dy row q is zero there; any x row will do)
            const int ty = fdiv(qq, d_w), tx = qq - ty * W;
            b_off[s_][hf] = (ty * XW + tx) * XP + wn * 64 + col2;
        }

    f32x16 acc[9];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tp][r] = 0.f;

    load_group(g_begin);
    for (int gi = g_begin; gi < g_end; ++gi) {
        __syncthreads();                                  // everyone is done reading the previous group
        store_group();
        __syncthreads();
        if (gi + 1 < g_end) load_group(gi + 1);
#pragma unroll
        for (int s_ = 0; s_ < KSTEPS; ++s_) {
            const s16x4 alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(dyl + a_base + s_ * 16 * DP));
            const s16x4 ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(dyl + a_base + (s_ * 16 + 4) * DP));
            const uint2 a0 = __builtin_bit_cast(uint2, alo), a1 = __builtin_bit_cast(uint2, ahi);
            const bf16x8 af = __builtin_bit_cast(bf16x8, make_uint4(a0.x, a0.y, a1.x, a1.y));
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int toff = (kh * XW + kw) * XP;
                    const s16x4 blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(xl + b_off[s_][0] + toff));
                    const s16x4 bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(xl + b_off[s_][1] + toff));
                    const uint2 b0 = __builtin_bit_cast(uint2, blo), b1 = __builtin_bit_cast(uint2, bhi);
                    const bf16x8 bfr = __builtin_bit_cast(bf16x8, make_uint4(b0.x, b0.y, b1.x, b1.y));
                    acc[kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[kh * 3 + kw], 0, 0, 0);
                }
        }
    }

    const int l31 = lane & 31, h = lane >> 5;
    const int ci = ci0 + wn * 32 + l31;
    if (ci >= Cin) return;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (co < Cout) atomicAdd(dwt + ((long long)tp * Cout + co) * Cin + ci, acc[tp][r]);
        }
}

template <int TH, int KSTEPS>
static void wgrad_rows_launch(const uint16_t* dy, const uint16_t* x, float* dwt, int N, int H, int W, int Cin, int Cout,
                              long long ps, hipStream_t st) {
    const int tiles_ci = (Cin + 63) / 64, tiles_co = (Cout + 63) / 64;
    const int tiles = tiles_ci * tiles_co;
    const int gpi = (H + TH - 1) / TH;
    const long long groups = (long long)N * gpi;
    const long long target = 512;                             // measured best of 256..1024 (2 blocks per CU)
    long long nb = (target + tiles - 1) / tiles;              // every block ends with a 64x64x9 atomic tile
    if (nb > groups) nb = groups;
    if (nb < 1) nb = 1;
    const int gpb = (int)((groups + nb - 1) / nb);
    nb = (groups + gpb - 1) / gpb;
    YOLO_LAUNCH((wgrad_rows_kernel<TH, KSTEPS>), dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, st, dy, x, dwt, N, H, W,
                Cin, Cout, ps, tiles_ci, gpb, gpi, make_fastdiv((unsigned)W), make_fastdiv((unsigned)(W + 2) * 8),
                make_fastdiv((unsigned)gpi));
}

// (TH, KSTEPS) of the row-group kernel for an output width, or false when none of the instantiations fits
static bool wgrad_rows_dispatch(const uint16_t* dy, const uint16_t* x, float* dwt, int N, int H, int W, int Cin, int Cout,
                                long long ps, hipStream_t st) {
    int best_th = 0, best_k = 0;
    double best_eff = 0;
    static const int table[][2] = {{6, 5}, {5, 6}, {3, 5}, {2, 5}, {2, 7}, {1, 5}, {4, 4}, {1, 4}, {1, 7}};
    for (const auto& t : table) {
        const int th = t[0], k = t[1];
        if (th * W > k * 16 || (k - 1) * 16 >= th * W) continue;          // K-steps must match exactly
        const double eff = (double)th * W / (k * 16.0);
        if (eff > best_eff) { best_eff = eff; best_th = th; best_k = k; }
    }
    if (!best_th) return false;
#define ROWS_CASE(TH_, K_) if (best_th == TH_ && best_k == K_) { wgrad_rows_launch<TH_, K_>(dy, x, dwt, N, H, W, Cin, Cout, ps, st); return true; }
    ROWS_CASE(6, 5) ROWS_CASE(5, 6) ROWS_CASE(3, 5) ROWS_CASE(2, 5) ROWS_CASE(2, 7) ROWS_CASE(1, 5) ROWS_CASE(4, 4)
    ROWS_CASE(1, 4) ROWS_CASE(1, 7)
#undef ROWS_CASE
    return false;
}

// dw_oihw[co][ci][tap] += dwt[tap][co][ci]
__global__ void wgrad_finish_kernel(float* __restrict__ dwt, float* __restrict__ dw, int Cout, int Cin, int taps,
                                    long long total) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;     // over [co][ci][tap]
    if (i >= total) return;
    const int tap = (int)(i % taps);
    const long long cc = i / taps;                                             // co*Cin + ci
    const long long j = (long long)tap * Cout * Cin + cc;
    dw[i] += dwt[j];
    dwt[j] = 0.f;                                    // leave the workspace zeroed for the next call (no memset launch)
}

// The dy side of the bf16 and split kernels: a 64-bit base per chunk / strip step / row group, and `int` lane offsets behind it
// that span `pixels` pixels of the caller's pitch (d_off, d_goff).  They must stay below 2^31 bytes.
static bool dy_lanes_fit(long long pixels, long long ps) { return ps <= (0x7fffffffLL - 4096) / (2 * pixels); }

// the finishing launch behind every kernel that accumulates into the [tap][Cout][Cin] workspace
static int wgrad_finish(float* ws, float* dw_oihw, int Cout, int Cin, int taps, hipStream_t st) {
    const long long total = (long long)Cin * Cout * taps;
    YOLO_LAUNCH(wgrad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, dw_oihw, Cout, Cin, taps, total);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// The register-staged bf16 families as yolo_conv_wgrad_algo tries them, in this order: each launches into the workspace and
// returns YOLO_OK, or YOLO_EUNSUPPORTED for a shape outside its domain or past its offset limits.
struct WgradShape {
    const uint16_t* dy;
    const uint16_t* x;
    float* ws;
    int N, H, W, Cin, Ho, Wo, Cout, ksize, stride;
    long long ps;
    hipStream_t st;
};

// strip kernel: 3x3, Cin <= 64
// (the 64 -> 128 stride-2 layer: the per-tap kernel measures 388 us against the strip kernel's 503 at 208^2 bs 64)
// (x: 64-bit bases per step, so any extent; dy: the lane offsets span TH rows of a 32-pixel strip -- a pitch too wide for that
//  goes on to the per-tap kernel, and so does a row so wide that the `int x_off` of the two staged rows would pass 2^31 bytes:
//  millions of columns)
static int wgrad_strip_try(const WgradShape& g) {
    if (!(g.ksize == 3 && g.Cin <= 64 && !(g.stride == 2 && g.Cin == 64) && dy_lanes_fit((g.stride == 2 ? 0LL : g.Wo) + 32, g.ps) &&
          (2LL * g.W + 128) * g.Cin * 2 < 0x7fffffffLL))
        return YOLO_EUNSUPPORTED;
    // CO_F = 1 (144 accumulator registers): CO_F = 2 needs 288 and spills
    if (g.stride == 2) wgrad_strip_launch<1, 2, 1>(g.dy, g.x, g.ws, g.N, g.H, g.W, g.Cin, g.Ho, g.Wo, g.Cout, g.ps, g.st);
    else wgrad_strip_launch<1, 1, 2>(g.dy, g.x, g.ws, g.N, g.H, g.W, g.Cin, g.Ho, g.Wo, g.Cout, g.ps, g.st);
    return YOLO_OK;
}

// row-group kernel: wins on the narrow deep maps (26x26: 210 -> 163 us, 13x13: 211 -> 175 us at batch 64); on wider
// maps its atomic epilogue (one 64x64x9 tile per block) costs more than the saved L2 traffic
// (x: a 64-bit base per row group, so any extent; dy: the lane offsets span a group of at most 7 * 16 pixels -- as above)
static int wgrad_rows_try(const WgradShape& g) {
    if (!(g.ksize == 3 && g.stride == 1 && g.W <= 40 && dy_lanes_fit(112, g.ps))) return YOLO_EUNSUPPORTED;
    return wgrad_rows_dispatch(g.dy, g.x, g.ws, g.N, g.H, g.W, g.Cin, g.Cout, g.ps, g.st) ? YOLO_OK : YOLO_EUNSUPPORTED;
}

// per-tap kernel, 128 x 128 tiles (256x128 / 128x256 / 256x256 tiles were measured 10-40 % slower: one wave per SIMD)
static int wgrad_tap_try(const WgradShape& g) {
    if ((long long)g.N * g.H * g.W * g.Cin * 2 >= 0xffffff00LL || (long long)g.N * g.Ho * g.Wo >= 0x7fffffffLL)
        return YOLO_EUNSUPPORTED;                            // (32-bit buffer offsets into x)
    if (!dy_lanes_fit(WG_KC, g.ps)) return YOLO_EUNSUPPORTED;    // (dy: the lane offsets span one K-chunk)
    static const long long target_env = YOLO_LAB_ENV("YOLO_PT_TARGET", 0);   // (ablation knob)
    wgrad_tap_launch<2, 2, 1>(g.dy, g.x, g.ws, g.N, g.H, g.W, g.Cin, g.Ho, g.Wo, g.Cout, g.ksize, g.stride, g.ps, 0, g.Cin, 0,
                              TapSlices{target_env ? target_env : 768, 16}, false, g.st);
    return YOLO_OK;
}

extern "C" long long yolo_conv_wgrad_workspace_bytes(int Cin, int Cout, int ksize, int dtype) {
    if (Cin <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3) || (dtype != YOLO_BF16 && dtype != YOLO_F32)) return YOLO_EINVAL;
    if (dtype != YOLO_BF16) return 0;
    return (long long)Cin * Cout * ksize * ksize * 4;
}

extern "C" int yolo_conv_wgrad(const void* dy, const void* x, float* dw_oihw, int N, int H, int W, int Cin, int Cout,
                               int ksize, int stride, long long dy_pixel_stride, int dtype, void* workspace,
                               void* stream) {
    static const int legacy = YOLO_LAB_SET("YOLO_WGRAD_LEGACY") ? 1 : 0;      // (A/B knob: the register-staged kernels only)
    return yolo_conv_wgrad_algo(dy, x, dw_oihw, N, H, W, Cin, Cout, ksize, stride, dy_pixel_stride, dtype, workspace,
                                legacy, stream);
}

// algo: 0 = the library's choice; 1 = the register-staged kernels (per-tap / strip / row-group); 2 / 3 = the row-walk
// kernel with one 16-column walker / four 4-column walkers per block, 4 = 3 with 8-wave blocks that reduce two K-slices
// through LDS before the atomics (EUNSUPPORTED outside its domain)
extern "C" int yolo_conv_wgrad_algo(const void* dy, const void* x, float* dw_oihw, int N, int H, int W, int Cin, int Cout,
                                    int ksize, int stride, long long dy_pixel_stride, int dtype, void* workspace, int algo,
                                    void* stream) {
    if (!dy || !x || !dw_oihw || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return YOLO_EINVAL;
    if (algo < 0 || algo > 6) return YOLO_EINVAL;
    if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2)) return YOLO_EUNSUPPORTED;
    if (dtype == YOLO_F32)
        return yolo_conv_wgrad_f32((const float*)dy, (const float*)x, dw_oihw, N, H, W, Cin, Cout, ksize, stride,
                                   dy_pixel_stride, stream);
    if (dtype != YOLO_BF16) return YOLO_EINVAL;
    if (dy_pixel_stride < 0) return YOLO_EINVAL;
    const long long ps = dy_pixel_stride ? dy_pixel_stride : Cout;
    if (!workspace || (Cin % 8) || (ps % 8)) return YOLO_EUNSUPPORTED;
    if ((long long)N * H * W >= 0x7fffffffLL) return YOLO_EUNSUPPORTED;
    const int pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    const bool k1 = ksize == 1, k3s1 = ksize == 3 && stride == 1;
    // a kernel named by its id: its status is final.  (Both add straight into dw_oihw -- [cout][cin] is the OIHW layout of a
    // 1x1 -- with no workspace and no finishing pass.)
    if (algo >= 5) return k1 ? wgrad_gemm_dispatch(dy, x, dw_oihw, (long long)N * H * W, Cin, Cout, ps, algo - 4, st) : YOLO_EUNSUPPORTED;
    if (algo >= 2) return k3s1 ? wgrad_walk_dispatch(dy, x, dw_oihw, N, H, W, Cin, Cout, ps, algo - 1, st) : YOLO_EUNSUPPORTED;
    // the library's choice: the GEMM / the row walk where they take the shape, ahead of the register-staged kernels
    int rc = YOLO_EUNSUPPORTED;
    if (algo == 0 && k1) rc = wgrad_gemm_dispatch(dy, x, dw_oihw, (long long)N * H * W, Cin, Cout, ps, 0, st);
    if (algo == 0 && k3s1) rc = wgrad_walk_dispatch(dy, x, dw_oihw, N, H, W, Cin, Cout, ps, 0, st);
    if (rc != YOLO_EUNSUPPORTED) return rc;
    const WgradShape g = {(const uint16_t*)dy, (const uint16_t*)x, (float*)workspace, N, H, W, Cin, Ho, Wo, Cout, ksize, stride, ps, st};
    rc = wgrad_strip_try(g);
    if (rc == YOLO_EUNSUPPORTED) rc = wgrad_rows_try(g);
    if (rc == YOLO_EUNSUPPORTED) rc = wgrad_tap_try(g);
    return rc == YOLO_OK ? wgrad_finish(g.ws, dw_oihw, Cout, Cin, ksize * ksize, st) : rc;
}

// Split weight gradient (YOLO_BF16X3).  algo 0 = the library's choice, 1 = 64 x 64 tiles, 2 = 128 x 128 tiles.
extern "C" long long yolo_conv_wgrad_split_workspace_bytes(int Cin, int Cout, int ksize, int dtype) {
    if (Cin <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3) || dtype != YOLO_BF16X3) return YOLO_EINVAL;
    return (long long)Cin * Cout * ksize * ksize * 4;
}

extern "C" int yolo_conv_wgrad_split(const void* dy, const void* x, float* dw_oihw, int N, int H, int W, int Cin, int Cout,
                                     int ksize, int stride, long long dy_pixel_stride, long long dy_lo_offset, int dtype,
                                     void* workspace, int algo, void* stream) {
    if (!dy || !x || !dw_oihw || !workspace || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return YOLO_EINVAL;
    if (algo < 0 || algo > 2 || dy_pixel_stride < 0 || dy_lo_offset < 0) return YOLO_EINVAL;
    if (dtype != YOLO_BF16X3) return YOLO_EINVAL;
    if ((ksize != 1 && ksize != 3) || (stride != 1 && stride != 2) || (Cin % 8)) return YOLO_EUNSUPPORTED;
    const long long lo = dy_lo_offset ? dy_lo_offset : round_up(Cout, 32);
    const long long ps = dy_pixel_stride ? dy_pixel_stride : 2 * lo;
    // the lo plane of every dy row lies after its hi values and inside the pixel (rows of at least the 8-channel units read)
    if (lo < round_up(Cout, 8) || ps < lo + round_up(Cout, 8) || (ps % 8) || (lo % 8)) return YOLO_EINVAL;
    const int pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const long long x_ps = dense_ps<bf16x3_t>(Cin);
    const int x_lo = dense_lo<bf16x3_t>(Cin);
    // The kernel's buffer offsets into x are 32-bit (dy offsets are relative to a chunk): a batch whose x reaches 4 GiB -- both planes
    // count, so at half the images of the bf16 path -- runs as several launches over slices of whole images, each below the limit,
    // all accumulating into the workspace with atomics.
    const long long img_bytes = (long long)H * W * x_ps * 2;
    long long per = N;
    if (per * img_bytes >= 0xffffff00LL) per = (0xffffff00LL - 1) / img_bytes;
    if (per * Ho * Wo >= 0x7fffffffLL) per = (0x7fffffffLL - 1) / ((long long)Ho * Wo);
    if (per < 1 || lo * 2 >= 0x7fff0000LL) return YOLO_EUNSUPPORTED;            // (one image alone past the limit)
    if (!dy_lanes_fit(SWG_KC + 1, ps)) return YOLO_EUNSUPPORTED;                // (dy: a K-chunk of pixels and the lo plane behind the last)
    hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError();
    const int variant = algo ? algo : ((Cin <= 64 || Cout <= 64) ? 1 : 2);
    const bool sliced = per < N;
    for (long long n0 = 0; n0 < N; n0 += per) {
        const int n = (int)min(per, (long long)N - n0);
        const uint16_t* d16 = (const uint16_t*)dy + n0 * Ho * Wo * ps;
        const uint16_t* x16 = (const uint16_t*)x + n0 * H * W * x_ps;
        if (variant == 1)
            wgrad_tap_launch<1, 1, 2>(d16, x16, (float*)workspace, n, H, W, Cin, Ho, Wo, Cout, ksize, stride, ps, (int)lo, x_ps, x_lo,
                                      TapSlices{1536, 32}, sliced, st);
        else
            wgrad_tap_launch<2, 2, 2>(d16, x16, (float*)workspace, n, H, W, Cin, Ho, Wo, Cout, ksize, stride, ps, (int)lo, x_ps, x_lo,
                                      TapSlices{768, 32}, sliced, st);
    }
    return wgrad_finish((float*)workspace, dw_oihw, Cout, Cin, ksize * ksize, st);
}
