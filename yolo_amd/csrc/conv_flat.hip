// Flat streaming 1x1 convolution for the residual / head 1x1 layers of stages 2 and 3 (bf16 / IEEE half; Cin -> Cout in
// {256 -> 128, 512 -> 256}; dense NHWC input and output; algo 43).  Over a dense map a 1x1 is a GEMM over the N * H * W
// contiguous pixel rows: no rows, no halos.  These layers move 30-70 MB for ~6 GFLOP -- what matters is that the input is read
// once, in long coalesced runs, with loads in flight the whole time; the tiled kernels (conv_pipe.hip) run them as ONE round of
// tiles, each block load -> compute -> store in sequence behind a barrier per 32 channels.
//
//   * WEIGHTS-STATIONARY, as conv_stream.hip: a wave keeps the A fragments of its 32 output channels for the whole K
//     (Cin / 16 fragments = Cin / 4 VGPRs) in registers for the lifetime of the block -- read once from the packed image.
//   * PERSISTENT blocks (COUT / 32 waves: every wave sees every pixel of the tile) walk tiles of TP = 32 pixels of the flat
//     pixel index p = (n H + y) W + x with stride gridDim.x.  A tile is one contiguous byte range of the input and of the
//     output; tiles cross rows and images; the last one is ragged (its missing pixels are range-checked away: read as zeros
//     through the tile's buffer resource, never stored).
//   * the pipeline runs ACROSS tiles: tile i + 2 is in flight into one of two register sets while tile i is multiplied out of
//     one of two LDS buffers and tile i + 1 is written into the other -- one workgroup barrier per tile.  The B fragments of a
//     tile are shared by the block's waves through LDS at a pixel pitch of Cin * 2 + 16 bytes (an odd number of 16-byte units:
//     conflict-free fragment reads).
//   * one accumulator chain per output, K steps ascending on the 32x32x16 MFMA -- the order of the tiled 1x1, so the stored
//     bytes are equal; epilogue as in conv_stream.hip (row_walk.h: transpose through a private LDS scratch, folded BN or
//     identity, LeakyReLU, residual in fp32 -- requested before the tile's MFMAs --, one rounding, 16-byte row stores).
#include "common.h"
#include "conv_args.h"
#include "row_walk.h"
#include <stdio.h>
#include <type_traits>

struct FlatArgs {
    const char* x;
    const char* wp;
    const float* scale;
    const float* bias;
    const char* res;
    char* y;
    long long npix;             // N * H * W
    int ntiles;                 // ceil(npix / TP)
    int Cout_pad;
    float slope;
};

namespace flat {
constexpr int TP = 32;          // pixels per tile: one MFMA column group
// resident blocks per CU the grid is sized for -- two waves per SIMD either way: 256 -> 128 is 4 waves, 184 registers and 51 KB
// of LDS (a third block fits the LDS, but at 168 registers the kernel spills), 512 -> 256 is 8 waves, 232 registers and 101 KB
constexpr int blocks_per_cu(int cin, int cout) { return (cin == 256 && cout == 128) ? 2 : 1; }
constexpr bool pair_ok(int cin, int cout) { return (cin == 256 && cout == 128) || (cin == 512 && cout == 256); }
}  // namespace flat

template <int CIN, int COUT, typename T>
__global__ __launch_bounds__(COUT / 32 * 64) void conv_flat_kernel(FlatArgs a) {
    constexpr int TP = flat::TP;
    constexpr int WAVES = COUT / 32, NT = WAVES * 64;
    constexpr int KC = CIN / 16;
    constexpr int ROWB = CIN * 2, PARTS = ROWB / 16, PITCH = ROWB + 16;
    constexpr int TILEB = TP * ROWB;                    // input bytes of a tile
    constexpr int XBUF = TP * PITCH;
    constexpr int XU = TP * PARTS / NT;                 // 16-byte units per thread and tile
    static_assert(TP * PARTS % NT == 0, "a tile = whole passes of the block");
    constexpr int SCR = rw::SCR;                        // per-wave epilogue scratch
    __shared__ __attribute__((aligned(16))) char smem[2 * XBUF + WAVES * SCR];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    char* scr = smem + 2 * XBUF + wave * SCR;

    const int G = gridDim.x, t0 = blockIdx.x, ntiles = a.ntiles;

    // ---- input staging (registers; two sets, requested UNCONDITIONALLY two tiles ahead -- conv_stream.hip says why) ------------
    // A tile's bytes are contiguous: unit u of the block is byte u * 16 of the tile.  The tile's buffer resource ends at the map's
    // last pixel (or is empty for a tile past the last): what lies beyond reads zeros without an access.
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    uint4 xr[2][XU];
    auto load_x = [&](auto set_c, int t) {
        constexpr int SET = decltype(set_c)::value;
        const long long left = (a.npix - (long long)t * TP) * ROWB;
        const int nrec = t >= ntiles ? 0 : (left < TILEB ? (int)left : TILEB);
        const char* base = a.x + (nrec ? (long long)t * TILEB : 0);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, nrec, 0x00020000);
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, (tid + j * NT) * 16, 0, 0);
            xr[SET][j] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    auto store_x = [&](auto set_c, int buf) {
        constexpr int SET = decltype(set_c)::value;
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            const int u = tid + j * NT;
            *(uint4*)(smem + buf * XBUF + (u / PARTS) * PITCH + (u % PARTS) * 16) = xr[SET][j];
        }
    };
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;

    load_x(Set0{}, t0);
    // ---- the wave's weights: A fragments of its 32 couts for every K step, straight from the packed image ------------------------
    uint4 A[KC];
    rw::load_a_frags<1, CIN>(A, a.wp, a.Cout_pad, wave * 32, lane);
    load_x(Set1{}, t0 + G);
    // ---- per-lane epilogue constants (after the transpose a lane owns 8 couts of a pixel row) ----------------------------------
    const int ecol = lane & 3, erow0 = lane >> 2;
    const int eco = wave * 32 + ecol * 8;
    float sc[8], bi[8];
    const bool ident = a.scale == nullptr;               // identity epilogue (conv_epilogue.h)
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = 1.f; bi[e] = 0.f; }
    if (!ident) rw::load_bn_row(sc, bi, a.scale, a.bias, eco);
    const float slope = a.slope;
    const bool has_res = a.res != nullptr;

    store_x(Set0{}, 0);
    __syncthreads();

    const int b_off = l31 * PITCH + h * 16;
    const int yoff = (erow0 * COUT + eco) * 2;          // this lane's first pixel row in a tile's output bytes (the second: + 16 rows)
    // step k = tile t0 + k G; its parity names the LDS buffer it multiplies and the register set that is free at its top (it
    // receives tile k + 2); the other set holds tile k + 1, written into the other buffer at the step's bottom
    auto step = [&](auto par_c, int t) {
        constexpr int PAR = decltype(par_c)::value;
        using Mine = std::integral_constant<int, PAR>;
        using Other = std::integral_constant<int, PAR ^ 1>;
        // The tile's output bytes (and its residual's: same offsets) as buffer resources that end at the map's last pixel: every
        // residual load and output store is an UNCONDITIONAL range-checked access, a missing pixel (or no residual: an empty
        // resource) is no access.  Behind a branch the loads would be zero-initialisations + predicated loads, and the compiler
        // waits for every load in flight -- the tiles requested ahead -- before each zero-initialisation (row_walk.h).
        const long long yleft = (a.npix - (long long)t * TP) * (COUT * 2);
        const int ynrec = yleft < TP * COUT * 2 ? (int)yleft : TP * COUT * 2;
        const long long ybase = (long long)t * (TP * COUT * 2);
        const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.y + ybase), 0, ynrec, 0x00020000);
        const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc((void*)(has_res ? a.res + ybase : a.y), 0, has_res ? ynrec : 0, 0x00020000);
        // residual prefetch, requested BEFORE the tile two ahead: the wait for it then leaves that tile's loads in flight
        uint4 rv[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rrs, yoff + k * (16 * COUT * 2), 0, 0);
            rv[k] = make_uint4(v.x, v.y, v.z, v.w);
        }
        load_x(Mine{}, t + 2 * G);

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const char* bp = smem + PAR * XBUF + b_off;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) acc = mfma16<T>(A[kc], *(const uint4*)(bp + kc * 32), acc);

        // ---- epilogue: folded BN, LeakyReLU, residual, one rounding, 16-byte row stores ---------------------------
        rw::scratch_put(scr, acc, lane);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float v[8];
            rw::scratch_get(v, scr, lane, k);
            if (!ident) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float tt = v[e] * sc[e] + bi[e];
                    v[e] = leaky(tt, slope);
                }
            }
            if (has_res) rw::add8<T>(v, rv[k]);
            const uint4 o = rw::pack8<T>(v);
            const u32x4_t ov = {o.x, o.y, o.z, o.w};
            __builtin_amdgcn_raw_buffer_store_b128(ov, yrs, yoff + k * (16 * COUT * 2), 0, 0);
        }
        wave_lds_fence();                               // (the next step's scratch_put must not move above these reads)

        if (t + G < ntiles) store_x(Other{}, PAR ^ 1);
        __syncthreads();
    };
    for (int t = t0; t < ntiles; t += 2 * G) {
        step(Set0{}, t);
        if (t + G < ntiles) step(Set1{}, t + G);
    }
}

template <int CIN, int COUT, typename T>
static int launch_flat(const ConvArgs& c, hipStream_t st, const NameOut* nm) {
    if (nm) {
        snprintf(nm->buf, nm->len, "void conv_flat_kernel<%d, %d, %s>(FlatArgs)", CIN, COUT, Elem<T>::name);
        if (nm->stats_rows) *nm->stats_rows = -1;
        return YOLO_OK;
    }
    FlatArgs a;
    a.x = c.x; a.wp = c.wp; a.scale = c.scale; a.bias = c.bias; a.res = c.res; a.y = c.y;
    a.npix = (long long)c.N * c.H * c.W;
    a.ntiles = (int)((a.npix + flat::TP - 1) / flat::TP);
    a.Cout_pad = c.Cout_pad;
    a.slope = c.slope;
    static int cus_of[64];                                   // CU count per device ordinal (0 = not asked yet)
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return YOLO_EINVAL;
    if (dev >= 0 && dev < 64) cus = cus_of[dev];
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        if (dev >= 0 && dev < 64) cus_of[dev] = cus;
    }
    const long long slots = (long long)cus * flat::blocks_per_cu(CIN, COUT);
    const unsigned grid = (unsigned)(a.ntiles < slots ? a.ntiles : slots);
    YOLO_LAUNCH((conv_flat_kernel<CIN, COUT, T>), dim3(grid), dim3(COUT / 32 * 64), 0, st, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// algo 43
int conv_flat_dispatch(const ConvArgs& c, int ks, int stride, int dtype, hipStream_t st, const NameOut* nm) {
    if (ks != 1 || stride != 1 || (dtype != YOLO_BF16 && dtype != YOLO_F16)) return YOLO_EUNSUPPORTED;
    if (c.out_f32 || c.up2 || c.stats || c.t_wp) return YOLO_EUNSUPPORTED;
    if (c.x_ps != c.Cin || c.y_ps != c.Cout || c.y_bs != (long long)c.Ho * c.Wo * c.Cout) return YOLO_EUNSUPPORTED;
    if ((long long)c.N * c.H * c.W > 0x7fffffffLL - 4 * 768 * flat::TP) return YOLO_EUNSUPPORTED;      // (tile indices are ints, requested two grid strides ahead)
    const bool half = dtype == YOLO_F16;
#define FLAT_CASE(CIN_, COUT_)                                                                   \
    if (c.Cin == CIN_ && c.Cout == COUT_)                                                        \
        return half ? launch_flat<CIN_, COUT_, f16_t>(c, st, nm) : launch_flat<CIN_, COUT_, bf16_t>(c, st, nm);
    FLAT_CASE(256, 128)
    FLAT_CASE(512, 256)
#undef FLAT_CASE
    return YOLO_EUNSUPPORTED;
}

// The tile size in pixels and the resident blocks per compute unit yolo_conv_fwd's algo 43 sizes its grid with (host only, no
// launch): grid = min(ceil(N H W / tile_px), compute units x blocks_per_cu).
extern "C" int yolo_conv_flat_geometry(int Cin, int Cout, int* tile_px, int* blocks_per_cu) {
    if (!tile_px || !blocks_per_cu) return YOLO_EINVAL;
    if (!flat::pair_ok(Cin, Cout)) return YOLO_EUNSUPPORTED;
    *tile_px = flat::TP;
    *blocks_per_cu = flat::blocks_per_cu(Cin, Cout);
    return YOLO_OK;
}
