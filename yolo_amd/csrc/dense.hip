// gluoncv's DenseNet body for inference: the backbone of the reference's OCRDenseNet (OCR/OCR.py:34-74), LPDenseNet
// (licence_plate/LP_detection.py:59-97) and CarDenseNet (car/utils.py:48-61).  gluoncv is not part of the reference tree; its builder
// is restated from recall in yolo_amd/dense.py and tests/dense_ref.py, and nothing here is copied from it.
//
// A dense layer is BN -> ReLU -> conv1x1 (Cin -> Cm) -> BN -> ReLU -> conv3x3 (Cm -> G), its G channels appended to the map it read.
// The first BN cannot be folded into a producer (every later layer reads the same raw channels through a BN of its own), the net has
// ~50 such layers of a few dozen channels and is bound by launches, so the layer is ONE kernel working in place on the block's buffer:
//   * a block of 4 waves owns an 8 x 8 pixel tile; its 10 x 10 halo of the Cm-channel bottleneck lives in LDS;
//   * stage 1: a lane loads 8 channels of one halo pixel straight into registers (its MFMA B fragment is exactly that), applies
//     max(0, x s1 + t1) in fp32, masks channels >= Cin with a SELECT (they may hold anything, this launch's own output in flight
//     from another block included), rounds once to the operand type and multiplies with W1 on v_mfma_f32_16x16x32_bf16 (YOLO_F32:
//     eight v_mfma_f32_16x16x4_f32 per chunk, the same lane map); the result through max(0, m s2 + t2) is rounded once and
//     written to LDS -- EXACTLY 0 for a halo pixel outside the image: the 3x3 pads the activated map, not the 1x1's output;
//   * stage 2: wave w takes output rows 2w, 2w + 1 of the tile, 9 taps x Cm / 32 chunks read from LDS; a lane ends up with four
//     consecutive new channels of one pixel and stores exactly those (bf16, G = 12: 8-byte stores at 24-byte steps); nothing
//     outside channels [Cin, Cin + G) is written.
// Operand images ("dense operand image" in include/yolo_amd.h): a (M, K) matrix as [M / 16][K / 32][64 lanes][8], lane l element j
// = A[16 mt + (l & 15)][32 kc + 8 (l >> 4) + j], zero padded -- a wave reads one 16 x 32 A fragment as 64 contiguous vectors.
#include "common.h"
#include "dense_mma.h"

namespace {
constexpr int TS = 8, HS = TS + 2, HPIX = HS * HS, HGROUPS = 7, HALLOC = HGROUPS * 16;      // 100 halo pixels in 7 groups of 16
constexpr int MT_MAX = 8;                                                                  // Cm <= 128

// four consecutive channels of one pixel, `al` = the largest of 4, 2, 1 elements the address is aligned to (wave-uniform)
template <typename T> __device__ __forceinline__ void store4(char* p, const float (&v)[4], int al);
template <> __device__ __forceinline__ void store4<bf16_t>(char* p, const float (&v)[4], int al) {
    const uint32_t lo = pack_bf16x2(v[0], v[1]), hi = pack_bf16x2(v[2], v[3]);
    if (al == 4) {
        *(uint2*)p = make_uint2(lo, hi);
    } else if (al == 2) {
        ((uint32_t*)p)[0] = lo;
        ((uint32_t*)p)[1] = hi;
    } else {
        ((uint16_t*)p)[0] = (uint16_t)lo; ((uint16_t*)p)[1] = (uint16_t)(lo >> 16);
        ((uint16_t*)p)[2] = (uint16_t)hi; ((uint16_t*)p)[3] = (uint16_t)(hi >> 16);
    }
}
template <> __device__ __forceinline__ void store4<float>(char* p, const float (&v)[4], int al) {
    if (al == 4) {
        *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    } else if (al == 2) {
        ((float2*)p)[0] = make_float2(v[0], v[1]);
        ((float2*)p)[1] = make_float2(v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) ((float*)p)[i] = v[i];
    }
}
template <typename T> __device__ __forceinline__ void store1(char* p, float v);
template <> __device__ __forceinline__ void store1<bf16_t>(char* p, float v) { *(uint16_t*)p = (uint16_t)f32_to_bf16_bits(v); }
template <> __device__ __forceinline__ void store1<float>(char* p, float v) { *(float*)p = v; }

struct DenseArgs {
    char* buf;
    const char* w1;
    const float* s1;
    const float* t1;
    const char* w2;
    const float* s2;
    const float* t2;
    int N, H, W, Cs, Cin, Cm, G;
};
}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void dense_layer_kernel(DenseArgs a) {
    constexpr int ES = sizeof(T);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Cmp = round_up(a.Cm, 32);
    const int pitch = Cmp * ES + 16;                       // bytes per halo pixel (+16: rows do not all start in one bank)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int tx0 = blockIdx.x * TS, ty0 = blockIdx.y * TS, n = blockIdx.z;
    const int H = a.H, W = a.W;
    char* img = a.buf + (long long)n * H * W * a.Cs * ES;

    // channels Cm .. Cmp (Cm = 48: a half chunk) are operands of zero weights and must not be NaN; pixels 100 .. 111 are never read
    for (int i = tid; i < HALLOC * pitch / 16; i += 256) ((uint4*)smem)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    // ---- stage 1: the bottleneck of halo pixel groups `wave` and `wave + 4` (one A fragment serves both) -----------------
    {
        const int MT = a.Cm / 16, KC = (a.Cin + 31) / 32;
        const bool g1 = wave + 4 < HGROUPS;
        int hp[2];
        bool in[2];
        const char* px[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            hp[p] = (wave + 4 * p) * 16 + r;
            const int iy = ty0 - 1 + hp[p] / HS, ix = tx0 - 1 + hp[p] % HS;
            in[p] = hp[p] < HPIX && iy >= 0 && iy < H && ix >= 0 && ix < W;
            px[p] = img + ((long long)iy * W + ix) * a.Cs * ES;
        }
        f32x4 acc[2][MT_MAX];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m) acc[p][m] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < KC; ++kc) {
            const int c0 = kc * 32 + q * 8;
            Frag<T> b[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                b[p].zero();
                if (in[p]) {                                // (a pixel outside the image is not loaded; its result is forced to 0 below)
                    float f[8];
                    b[p].load(px[p] + c0 * ES);
                    b[p].unpack(f);
                    bn_relu8(f, a.s1, a.t1, c0, a.Cin);
                    b[p].pack(f);
                }
            }
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m) {
                if (m < MT) {
                    Frag<T> w;
                    w.load(a.w1 + ((long long)(m * KC + kc) * 64 + lane) * 8 * ES);
                    acc[0][m] = mma(w, b[0], acc[0][m]);
                    if (g1) acc[1][m] = mma(w, b[1], acc[1][m]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (p == 1 && !g1) break;
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m) {
                if (m < MT) {
                    const int j0 = m * 16 + q * 4;
                    const float4 s = *(const float4*)(a.s2 + j0), t = *(const float4*)(a.t2 + j0);
                    float v[4] = {fmaxf(acc[p][m][0] * s.x + t.x, 0.f), fmaxf(acc[p][m][1] * s.y + t.y, 0.f),
                                  fmaxf(acc[p][m][2] * s.z + t.z, 0.f), fmaxf(acc[p][m][3] * s.w + t.w, 0.f)};
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = in[p] ? v[i] : 0.f;      // the 3x3's zero padding, not max(0, t2)
                    store4<T>(smem + hp[p] * pitch + j0 * ES, v, 4);
                }
            }
        }
    }
    __syncthreads();

    // ---- stage 2: the 3x3 over the LDS halo; wave w = output rows 2w, 2w + 1 of the tile ----------------------------------
    {
        const int GT = (a.G + 15) / 16, KC = Cmp / 32;
        const int oy = 2 * wave + (r >> 3), ox = r & 7;
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        for (int tap = 0; tap < 9; ++tap) {
            const char* src = smem + ((oy + tap / 3) * HS + ox + tap % 3) * pitch + q * 8 * ES;
            for (int kc = 0; kc < KC; ++kc) {
                Frag<T> b;
                b.load(src + kc * 32 * ES);
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    if (g < GT) {
                        Frag<T> w;
                        w.load(a.w2 + ((long long)((g * 9 + tap) * KC + kc) * 64 + lane) * 8 * ES);
                        acc[g] = mma(w, b, acc[g]);
                    }
                }
            }
        }
        const int iy = ty0 + oy, ix = tx0 + ox;
        const int al = (a.Cin % 4 == 0) ? 4 : (a.Cin % 2 == 0) ? 2 : 1;
        if (iy < H && ix < W) {
            char* dst = img + (((long long)iy * W + ix) * a.Cs + a.Cin) * ES;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int g0 = g * 16 + q * 4;
                if (g < GT && g0 < a.G) {                   // G % 4 == 0: a lane's four channels are all new channels or none is
                    const float v[4] = {acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
                    store4<T>(dst + g0 * ES, v, al);
                }
            }
        }
    }
}

// ---- transition: BN -> ReLU -> AvgPool 2x2 s2 -> conv1x1 C -> C / 2 (the pool first: it is linear and quarters the work) ------
struct TransArgs {
    const char* x;
    char* y;
    const char* w;
    const float* s;
    const float* t;
    int N, H, W, C, Cs_in, Cs_out;
};

template <typename T>
__global__ __launch_bounds__(256) void dense_transition_kernel(TransArgs a) {
    constexpr int ES = sizeof(T);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int Ho = a.H / 2, Wo = a.W / 2, Cout = a.C / 2;
    const long long P = (long long)a.N * Ho * Wo;
    const long long pi = ((long long)blockIdx.x * 4 + wave) * 16 + r;
    const bool ok = pi < P;
    const int ox = ok ? (int)(pi % Wo) : 0, oy = ok ? (int)(pi / Wo % Ho) : 0, n = ok ? (int)(pi / Wo / Ho) : 0;
    const long long rowb = (long long)a.W * a.Cs_in * ES;
    const char* src = a.x + (((long long)n * a.H + 2 * oy) * a.W + 2 * ox) * a.Cs_in * ES;
    const int KC = (a.C + 31) / 32, MTOT = (Cout + 15) / 16;
    f32x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < KC; ++kc) {
        const int c0 = kc * 32 + q * 8;
        Frag<T> b;
        b.zero();
        if (ok) {
            float f[4][8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b.load(src + (k >> 1) * rowb + (k & 1) * a.Cs_in * ES + c0 * ES);
                b.unpack(f[k]);
                bn_relu8(f[k], a.s, a.t, c0, a.C);
            }
            float m[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = ((f[0][j] + f[1][j]) + (f[2][j] + f[3][j])) * 0.25f;
            b.pack(m);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int mt = blockIdx.y * 4 + m;
            if (mt < MTOT) {
                Frag<T> w;
                w.load(a.w + ((long long)(mt * KC + kc) * 64 + lane) * 8 * ES);
                acc[m] = mma(w, b, acc[m]);
            }
        }
    }
    if (!ok) return;
    char* dst = a.y + pi * a.Cs_out * ES;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int ch = (blockIdx.y * 4 + m) * 16 + q * 4;
        const float v[4] = {acc[m][0], acc[m][1], acc[m][2], acc[m][3]};
        if (ch + 4 <= Cout) {
            store4<T>(dst + ch * ES, v, 4);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (ch + i < Cout) store1<T>(dst + (ch + i) * ES, v[i]);
        }
    }
}

// ---- the final BN + ReLU into a dense tensor ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dense_bn_relu_kernel(const char* x, char* y, const float* s, const float* t, int N, int H, int W,
                                                            int C, int Cs, int Cp, int columns) {
    constexpr int ES = sizeof(T);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * H * W * Cp) return;
    const int c = (int)(idx % Cp);
    const long long pix = idx / Cp;
    float v = 0.f;
    if (c < C) {
        float xv;
        if constexpr (ES == 2) xv = bf16_bits_to_f32(*(const uint16_t*)(x + (pix * Cs + c) * ES));
        else xv = *(const float*)(x + (pix * Cs + c) * ES);
        v = fmaxf(xv * s[c] + t[c], 0.f);
    }
    long long o = idx;
    if (columns) {
        const int w = (int)(pix % W), h = (int)(pix / W % H);
        const long long n = pix / W / H;
        o = ((n * W + w) * H + h) * Cp + c;
    }
    store1<T>(y + o * ES, v);
}

// ---- stem: Conv 7x7 s2 p3 (3 -> F0) + BN + ReLU + MaxPool 3x3 s2 p1, a direct convolution on the vector pipe (K = 147) ------------
// A block makes an 8 x 8 tile of pooled pixels for 8 output channels: the 39 x 39 x 3 input patch, the 8 filters and the 17 x 17
// tile of activated convolution outputs live in LDS.  A pool tap outside the convolution's map reads 0: after the ReLU that equals
// the -inf padding of the pooling.
constexpr int SP = 39, SPW = 40, SC = 17;
template <typename T>
__global__ __launch_bounds__(256) void dense_stem_kernel(const float* x, const float* w, const float* s, const float* t, char* y, int N,
                                                         int H, int W, int Hc, int Wc, int Hp, int Wp, int Cs, int tiles_x) {
    constexpr int ES = sizeof(T);
    __shared__ float patch[3 * SP * SPW];
    __shared__ float wl[8 * 147];
    __shared__ float cv[SC * SC * 8];
    const int tid = threadIdx.x;
    const int px0 = (blockIdx.x % tiles_x) * 8, py0 = (blockIdx.x / tiles_x) * 8, co0 = blockIdx.y * 8, n = blockIdx.z;
    const float* img = x + (long long)n * 3 * H * W;
    for (int i = tid; i < 3 * SP * SP; i += 256) {
        const int c = i / (SP * SP), py = i / SP % SP, px = i % SP;
        const int iy = 4 * py0 - 5 + py, ix = 4 * px0 - 5 + px;
        patch[(c * SP + py) * SPW + px] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? img[((long long)c * H + iy) * W + ix] : 0.f;
    }
    for (int i = tid; i < 8 * 147; i += 256) wl[i] = w[(long long)co0 * 147 + i];
    __syncthreads();
    for (int pos = tid; pos < SC * SC; pos += 256) {
        const int ly = pos / SC, lx = pos % SC;
        const int cy = 2 * py0 - 1 + ly, cx = 2 * px0 - 1 + lx;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool valid = cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
        if (valid) {
#pragma unroll 1
            for (int c = 0; c < 3; ++c)
#pragma unroll 1
                for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const float v = patch[(c * SP + 2 * ly + ky) * SPW + 2 * lx + kx];
                        const int k = (c * 7 + ky) * 7 + kx;
#pragma unroll
                        for (int o = 0; o < 8; ++o) acc[o] = fmaf(v, wl[o * 147 + k], acc[o]);
                    }
        }
#pragma unroll
        for (int o = 0; o < 8; ++o) cv[pos * 8 + o] = valid ? fmaxf(acc[o] * s[co0 + o] + t[co0 + o], 0.f) : 0.f;
    }
    __syncthreads();
    if (tid < 64) {
        const int ly = tid >> 3, lx = tid & 7;
        const int py = py0 + ly, px = px0 + lx;
        if (py < Hp && px < Wp) {
            float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int d = 0; d < 9; ++d) {
                const float* p = cv + ((2 * ly + d / 3) * SC + 2 * lx + d % 3) * 8;
#pragma unroll
                for (int o = 0; o < 8; ++o) m[o] = fmaxf(m[o], p[o]);
            }
            char* dst = y + ((((long long)n * Hp + py) * Wp + px) * Cs + co0) * ES;
            const float lo[4] = {m[0], m[1], m[2], m[3]}, hi[4] = {m[4], m[5], m[6], m[7]};
            store4<T>(dst, lo, 4);
            store4<T>(dst + 4 * ES, hi, 4);
        }
    }
}

// ---- entries ------------------------------------------------------------------------------------------------------------------------
extern "C" long long yolo_dense_operand_bytes(int M, int K, int dtype) {
    if (M <= 0 || K <= 0) return YOLO_EINVAL;
    if (dtype != YOLO_BF16 && dtype != YOLO_F32) return dtype_valid(dtype) ? YOLO_EUNSUPPORTED : YOLO_EINVAL;
    return (long long)round_up(M, 16) * round_up_ll(K, 32) * elem_size(dtype);
}

extern "C" int yolo_dense_layer_fwd(void* buf, const void* w1_image, const float* scale1, const float* bias1, const void* w2_image,
                                    const float* scale2, const float* bias2, int N, int H, int W, int Cs, int Cin, int Cm, int G,
                                    int dtype, void* stream) {
    if (!buf || !w1_image || !scale1 || !bias1 || !w2_image || !scale2 || !bias2) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || Cs <= 0 || Cin <= 0 || Cm <= 0 || G <= 0) return YOLO_EINVAL;
    if (!dtype_valid(dtype)) return YOLO_EINVAL;
    if (dtype != YOLO_BF16 && dtype != YOLO_F32) return YOLO_EUNSUPPORTED;
    if ((G % 4) || G > 32 || (Cm % 16) || Cm > 16 * MT_MAX || Cin < 8 || (Cs % 32) || Cin + G > Cs) return YOLO_EUNSUPPORTED;
    const int es = elem_size(dtype);
    if (too_large((long long)N * H * W * Cs, es) || N > 65535 || (H + TS - 1) / TS > 65535) return YOLO_EUNSUPPORTED;
    DenseArgs a{(char*)buf, (const char*)w1_image, scale1, bias1, (const char*)w2_image, scale2, bias2, N, H, W, Cs, Cin, Cm, G};
    const dim3 grid((W + TS - 1) / TS, (H + TS - 1) / TS, N);
    const size_t lds = (size_t)HALLOC * (round_up(Cm, 32) * es + 16);
    if (dtype == YOLO_BF16) YOLO_LAUNCH(dense_layer_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else YOLO_LAUNCH(dense_layer_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_dense_transition_fwd(const void* x, const void* w_image, const float* scale, const float* bias, void* y, int N,
                                         int H, int W, int C, int Cs_in, int Cs_out, int dtype, void* stream) {
    if (!x || !w_image || !scale || !bias || !y) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Cs_in <= 0 || Cs_out <= 0) return YOLO_EINVAL;
    if (!dtype_valid(dtype)) return YOLO_EINVAL;
    if (dtype != YOLO_BF16 && dtype != YOLO_F32) return YOLO_EUNSUPPORTED;
    if (H < 2 || W < 2 || C < 2 || (Cs_in % 32) || (Cs_out % 32) || C > Cs_in || C / 2 > Cs_out) return YOLO_EUNSUPPORTED;
    const int es = elem_size(dtype);
    if (too_large((long long)N * H * W * Cs_in, es) || too_large((long long)N * (H / 2) * (W / 2) * Cs_out, es)) return YOLO_EUNSUPPORTED;
    TransArgs a{(const char*)x, (char*)y, (const char*)w_image, scale, bias, N, H, W, C, Cs_in, Cs_out};
    const long long P = (long long)N * (H / 2) * (W / 2);
    const dim3 grid((unsigned)((P + 63) / 64), (C / 2 + 63) / 64);
    if (dtype == YOLO_BF16) YOLO_LAUNCH(dense_transition_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else YOLO_LAUNCH(dense_transition_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_dense_bn_relu(const void* x, const float* scale, const float* bias, void* y, int N, int H, int W, int C, int Cs,
                                  int Cp, int columns, int dtype, void* stream) {
    if (!x || !scale || !bias || !y) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Cs <= 0 || Cp <= 0) return YOLO_EINVAL;
    if (!dtype_valid(dtype)) return YOLO_EINVAL;
    if (dtype != YOLO_BF16 && dtype != YOLO_F32) return YOLO_EUNSUPPORTED;
    if (C > Cs || C > Cp) return YOLO_EUNSUPPORTED;
    const int es = elem_size(dtype);
    if (too_large((long long)N * H * W * Cs, es) || too_large((long long)N * H * W * Cp, es)) return YOLO_EUNSUPPORTED;
    const long long total = (long long)N * H * W * Cp;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == YOLO_BF16)
        YOLO_LAUNCH(dense_bn_relu_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)x, (char*)y, scale, bias, N, H, W, C,
                    Cs, Cp, columns ? 1 : 0);
    else
        YOLO_LAUNCH(dense_bn_relu_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const char*)x, (char*)y, scale, bias, N, H, W, C,
                    Cs, Cp, columns ? 1 : 0);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_dense_stem_fwd(const float* x_nchw, const float* w_oihw, const float* scale, const float* bias, void* y, int N, int H,
                                   int W, int F0, int Cs, int dtype, void* stream) {
    if (!x_nchw || !w_oihw || !scale || !bias || !y) return YOLO_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || F0 <= 0 || Cs <= 0) return YOLO_EINVAL;
    if (!dtype_valid(dtype)) return YOLO_EINVAL;
    if (dtype != YOLO_BF16 && dtype != YOLO_F32) return YOLO_EUNSUPPORTED;
    if ((F0 % 8) || F0 > 64 || (Cs % 32) || F0 > Cs) return YOLO_EUNSUPPORTED;
    const int Hc = (H - 1) / 2 + 1, Wc = (W - 1) / 2 + 1;             // floor((n + 6 - 7) / 2) + 1
    const int Hp = (Hc - 1) / 2 + 1, Wp = (Wc - 1) / 2 + 1;           // floor((n + 2 - 3) / 2) + 1
    const int es = elem_size(dtype);
    if (too_large((long long)N * 3 * H * W, 4) || too_large((long long)N * Hp * Wp * Cs, es) || N > 65535) return YOLO_EUNSUPPORTED;
    const int tiles_x = (Wp + 7) / 8, tiles_y = (Hp + 7) / 8;
    const dim3 grid(tiles_x * tiles_y, F0 / 8, N);
    if (dtype == YOLO_BF16)
        YOLO_LAUNCH(dense_stem_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, x_nchw, w_oihw, scale, bias, (char*)y, N, H, W, Hc,
                    Wc, Hp, Wp, Cs, tiles_x);
    else
        YOLO_LAUNCH(dense_stem_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, x_nchw, w_oihw, scale, bias, (char*)y, N, H, W, Hc, Wc,
                    Hp, Wp, Cs, tiles_x);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
