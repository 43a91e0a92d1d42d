// The network's first FOUR convolutions as ONE inference kernel: the stem (Conv3x3 s1, 3 -> 32), the first stage's
// down-sampling conv (Conv3x3 s2, 32 -> 64) and that stage's residual block (x + conv3x3(64)(conv1x1(32)(x))), each conv
// with folded BN + LeakyReLU, from the (N,3,H,W) float32 NCHW image to the (N,H/2,W/2,64) NHWC output of the block.
//
// stem_down_kernel and res_block_kernel<64> are both row walkers whose parts add up instead of overlapping: all four waves of
// a block pass through the same phases between the same barriers, and a second block on the SIMD is in the same phase.  Here
// the two walkers share a block of 8 waves in two role groups, in lock step:
//   * waves 0-3 (producer) run stem_down_kernel's row step: 8-row image window, 3 MFMAs per 32 stem pixels, 5-row stem ring,
//     the down conv with its 18 register-resident A-fragments.  The down conv's epilogue writes its row, rounded once, into
//     the consumer's 3-row input ring (pixel pitch C * 2 + 16) straight from the MFMA layout -- no transpose, no global store.
//     Pixels outside the map are written as zeros;
//   * waves 4-7 (consumer) run res_block_kernel<64>'s row step: 1x1 into the mid ring, 3x3, + x in fp32, one rounding, 16-byte
//     row stores.  Its input row and its residual come from that ring: the register sets of rows in flight are gone.
// Each SIMD holds one wave of each role, i.e. two DIFFERENT dependency chains.  The 64-channel map between the two halves
// (written once and read once by the separate kernels) never leaves LDS.
// A row step has ONE block barrier, executed by all 8 waves in common code.  In step oy the producer makes ring row oy + 3
// (image loads of two steps ahead, the down conv's 18 MFMAs, the two new stem rows, the epilogue into ring slot (oy + 3) % 4) while
// the consumer makes mid row oy + 2 for the NEXT step and then output row oy (3x3 over mid rows oy-1 .. oy+1, residual = ring row
// oy).  Both rings have four slots, so nothing a step writes is read before the barrier that ends it.  (A first version kept the
// walkers' 3-slot rings and the consumer's barrier between its 1x1 and its 3x3: every step then waited twice for the slower
// role of a phase.)
// Geometry: the consumer's strip is w <= 60 output columns, the producer makes w + 2 (one halo column each side) within its
// 64-column MFMA step; a row slice makes the producer start one row early and end one row late (the recompute).
// Same operand order, K order, accumulation order and rounding points as yolo_stem_down_fwd followed by yolo_res_block_fwd:
// results are bit-identical.
#include "common.h"
#include "row_walk.h"
#include <type_traits>

using namespace rw;

namespace {
constexpr int C1 = STEM_C, C = 64;
constexpr int SW_MAX = 60;               // consumer strip width: + 2 halo columns = the producer's 62
// ---- consumer (res_block_kernel<64>'s rings) ----------------------------------------------------------------------------
constexpr int PX = C * 2 + 16, PM = C1 * 2 + 16;
constexpr int XROW = MW * PX, MROW = (MW + 2) * PM;
// ---- LDS map: the producer's stem ring and image window (row_walk.h), the two rings of the consumer, its scratch -------------
constexpr int OFF_IMG = RING * STEM_ROW;
constexpr int OFF_X = OFF_IMG + IROWS * IPW * 8;
constexpr int XSLOTS = 4, MSLOTS = 4;   // rows oy .. oy+3 of the input ring, oy-1 .. oy+2 of the mid ring are live in step oy
constexpr int OFF_M = OFF_X + XSLOTS * XROW;
constexpr int OFF_SCR = OFF_M + MSLOTS * MROW;
constexpr int LDS_BYTES = OFF_SCR + 4 * SCR;
static_assert(OFF_IMG % 16 == 0 && OFF_X % 16 == 0 && OFF_M % 16 == 0 && OFF_SCR % 16 == 0, "16-byte LDS accesses");
static_assert(LDS_BYTES <= 163840, "one block per CU");
static_assert(PITCH == PM, "both 3x3 loops read 32-channel pixels at the same pitch");
constexpr double PROLOGUE_ROWS = 7.0;    // a slice's prologue in row steps: ring fills, four producer rows, weights

struct SRArgs {
    const float* x;
    const float* w0;                      // stem, OIHW float32
    const float* scale0;
    const float* bias0;
    const char* wpd;                      // down conv, packed
    const float* scaled;
    const float* biasd;
    const char* wp1;                      // 1x1, packed
    const float* scale1;
    const float* bias1;
    const char* wp2;                      // 3x3, packed
    const float* scale2;
    const float* bias2;
    char* y;
    int N, H, W, Ho, Wo, Cpad;
    int nstrips, strip_w, rows_per_slice;
    float slope;
};

struct SRGeom { int nstrips, strip_w, rows_per_slice, slices; long long bx; };
}  // namespace

template <typename T>
__global__ __launch_bounds__(512) void stem_res_kernel(SRArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    char* xl = smem + OFF_X;                                 // the consumer's input ring = the producer's output
    char* ml = smem + OFF_M;                                 // mid ring
    const int tid = threadIdx.x & 255, lane = tid & 63;      // thread / wave index inside the role group
    const int wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool prod = wave8 < 4;
    const int wave = wave8 & 3;
    const int l31 = lane & 31, h = lane >> 5;
    const int wave_c = wave & 1, wave_p = wave >> 1;         // both 3x3s: wave = (cout slice of 32, pixel group of 32)
    char* scr = smem + OFF_SCR + wave * SCR;

    const int strip = blockIdx.x % a.nstrips;
    const int n = blockIdx.x / a.nstrips;
    const int ox0 = strip * a.strip_w;
    const int ox_end = min(ox0 + a.strip_w, a.Wo);
    const int oy0 = blockIdx.y * a.rows_per_slice;
    const int oy1 = min(oy0 + a.rows_per_slice, a.Ho);
    if (oy0 >= oy1) return;                                  // (the whole block, before its first barrier)
    const int Ho = a.Ho, Wo = a.Wo;
    const int mx0 = ox0 - 1;                  // map column of ring pixel 0 (= the producer's first output column)
    const int pr0 = oy0 - 1;                  // the producer's first row
    StemWin sw;
    sw.HW = (long long)a.H * a.W;
    sw.xn = a.x + (long long)n * 3 * sw.HW;
    sw.H = a.H; sw.W = a.W;
    sw.sx0 = 2 * mx0 - 1;
    sw.icol0 = sw.sx0 - 1;
    sw.iyb = 2 * pr0 - 2;
    sw.img = (uint2*)(smem + OFF_IMG);
    sw.ring = smem;
    sw.tid = tid;
    const int iyb = sw.iyb;

    // ---- hygiene: pixels of the LDS arrays that are never written are only read by discarded lanes ---------------------
    for (int i = threadIdx.x; i < OFF_SCR / 16; i += 512) ((uint4*)smem)[i] = make_uint4(0, 0, 0, 0);

    // ---- the role's weights and folded-BN constants, in the same registers for both roles -----------------------------------
    // 3x3: 18 A-fragments (32 couts x K = 288), down conv | the block's 3x3
    uint4 A[18];
    load_a_frags<3, C1>(A, prod ? a.wpd : a.wp2, a.Cpad, wave_c * 32, lane);
    // small conv: the stem's 3 weight fragments (one per kernel row) | the 1x1's 4 A-fragments, and its BN in the MFMA layout
    uint4 ws[4];
    if (prod) {
        stem_weight_frags<T>(ws, a.w0, lane);
        ws[3] = make_uint4(0, 0, 0, 0);
    } else {
        load_a_frags<1, C>(ws, a.wp1, a.Cpad, 0, lane);
    }
    float sc1[16], bi1[16];
    load_bn_mfma(sc1, bi1, prod ? a.scale0 : a.scale1, prod ? a.bias0 : a.bias1, 0, h);
    // folded BN of the 3x3.  Producer: the 16 couts of the MFMA layout (it writes the ring without a transpose); consumer:
    // the 8 couts of a pixel row a lane owns after the transpose (entries 0..7)
    const int eco = wave_c * 32 + (lane & 3) * 8;
    float sc2[16], bi2[16];
    if (prod) {
        load_bn_mfma(sc2, bi2, a.scaled, a.biasd, wave_c * 32, h);
    } else {
        load_bn_row(sc2, bi2, a.scale2, a.bias2, eco);
#pragma unroll
        for (int e = 8; e < 16; ++e) sc2[e] = bi2[e] = 0.f;
    }
    const float slope = a.slope;
    auto slot4 = [](int row) { return (row + 4) & 3; };       // rows >= -1 (both rings have four slots)

    // ==== producer: stem_down_kernel's row step, with the output row going to the ring ==========================================
    const int b_off = (wave_p * 32 + l31) * PITCH + h * 16;
    int slot0 = 0;                                           // stem ring slot of stem row 2 R - 1
    float cimg[2][3];
    bool okimg[2] = {false, false};
    // ring row R: request the image rows of two steps ahead (load_img), the down conv of row R (9 taps x 2 k-steps over the stem
    // ring), the two stem rows row R + 1 adds, the down conv's epilogue (folded BN, LeakyReLU, one rounding) into ring slot R % 4
    // straight from the MFMA layout -- zeros outside the map: the consumer's padding --, the image window rows of the next step
    auto prod_row = [&](auto par_c, int R) {
        constexpr int PAR = decltype(par_c)::value;
        load_img(sw, 2 * R + 7, 0, cimg[PAR ^ 1], okimg[PAR ^ 1]);
        f32x16 pacc[1];
        conv3x3_rows<T, 2, 1, PITCH>(pacc, A, [&](int kh) {
            int slot = slot0 + kh;
            if (slot >= RING) slot -= RING;
            return smem + slot * STEM_ROW + b_off;
        }, TapS2{});
        const bool more = R < oy1;                           // (the producer's last row is oy1)
        if (more) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int slot = slot0 + 3 + r;
                if (slot >= RING) slot -= RING;
                stem_group<T>(sw, ws, sc1, bi1, slope, lane, 2 * R + 2 + r, slot, wave);
            }
        }
        const int j = wave_p * 32 + l31;
        const int col = mx0 + j;
        store_tile<T>(xl + slot4(R) * XROW + j * PX + wave_c * 64, pacc[0], sc2, bi2, slope, h, R >= 0 && R < Ho && col >= 0 && col < Wo);
        if (more) store_img<T>(sw, 2 * R + 5, 0, cimg[PAR], okimg[PAR]);
        slot0 += 2;
        if (slot0 >= RING) slot0 -= RING;
    };

    // ==== consumer: res_block_kernel<64>'s row step, its input row and residual taken from the ring ==============================
    // mid row my from the input ring: waves 0, 1 of the group make one 32-pixel tile each; zeros outside the map
    auto mid_row = [&](int my) {
        if (wave >= 2) return;
        const int px = wave * 32 + l31, mx = mx0 + px;
        mid_tile<T>(xl + slot4(my) * XROW + px * PX + h * 16, ml + slot4(my) * MROW + px * PM, ws, sc1, bi1, slope, h,
                    my >= 0 && my < Ho && mx >= 0 && mx < Wo);
    };
    // the 3x3 of output row oy over mid rows oy-1 .. oy+1, then its epilogue: folded BN, LeakyReLU, + x (ring row oy, fp32),
    // one rounding, 16-byte row stores
    auto cons_b = [&](int oy) {
        f32x16 acc[1];
        conv3x3_rows<T, 2, 1, PM>(acc, A, [&](int kh) { return ml + slot4(oy - 1 + kh) * MROW + (wave_p * 32 + l31) * PM + h * 16; },
                                  TapS1<PM>{});
        res_epilogue<T, C, PX>(scr, acc[0], lane, sc2, bi2, slope, xl + slot4(oy) * XROW + eco * 2,
                               a.y + ((((long long)n * Ho + oy) * Wo + ox0) * C + eco) * 2, wave_p * 32, ox_end - ox0);
        wave_lds_fence();
    };

    // ==== the schedule: every barrier below is executed by all 8 waves =========================================================
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    __syncthreads();                                        // the zero fill
    // producer prologue: image rows iyb .. iyb+6, then stem rows 2 pr0 - 1 .. 2 pr0 + 1 into stem ring slots 0..2
    if (prod) {
        float c[4][3];
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) load_img(sw, iyb, r, c[r], ok[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < 3 || tid < 128) store_img<T>(sw, iyb, r, c[r], ok[r]);      // 7 rows: the 8th slot belongs to row iyb + 7
    }
    __syncthreads();
    if (prod) {
#pragma unroll
        for (int r = 0; r < 3; ++r) stem_group<T>(sw, ws, sc1, bi1, slope, lane, 2 * pr0 - 1 + r, r, wave);
    }
    __syncthreads();
    // ring rows oy0 - 1 .. oy0 + 2 (a row past oy1 is not made); the consumer's mid rows oy0 - 1 .. oy0 + 1 follow one barrier behind
    if (prod) { load_img(sw, 2 * pr0 + 5, 0, cimg[0], okimg[0]); prod_row(P0{}, pr0); }
    __syncthreads();
    if (prod) prod_row(P1{}, pr0 + 1); else mid_row(oy0 - 1);
    __syncthreads();
    if (prod) prod_row(P0{}, pr0 + 2); else mid_row(oy0);
    __syncthreads();
    if (prod) { if (pr0 + 3 <= oy1) prod_row(P1{}, pr0 + 3); } else mid_row(oy0 + 1);
    __syncthreads();

    // step oy, ONE barrier: the consumer makes mid row oy + 2 (for the next step) and output row oy while the producer makes ring
    // row oy + 3 (none past row oy1).  Nothing a step writes is read in that step: ring row oy + 3 takes the slot of row oy - 1,
    // mid row oy + 2 that of row oy - 2
    auto step = [&](auto par_c, int oy) {
        if (prod) {
            if (oy + 3 <= oy1) prod_row(par_c, oy + 3);
        } else {
            if (oy + 2 <= oy1) mid_row(oy + 2);
            cons_b(oy);
        }
        __syncthreads();
    };
    for (int oy = oy0; oy < oy1; oy += 2) {
        step(P0{}, oy);
        if (oy + 1 < oy1) step(P1{}, oy + 1);
    }
}

// strips x images x row slices to one block per CU (walker_row_slices)
static int sr_geometry(int N, int H, int W, SRGeom& g) {
    const int Ho = H / 2, Wo = W / 2;
    // full-width strips, the last one takes the rest: a row step costs the same at every width (one 64-column MFMA step)
    walker_strips(Wo, SW_MAX, g.nstrips, g.strip_w);
    g.strip_w = SW_MAX;
    g.bx = (long long)N * g.nstrips;
    if (g.bx > 0x7fffffffLL) return YOLO_EUNSUPPORTED;
    static int cus_of[64];                                   // CU count per device ordinal (0 = not asked yet)
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return YOLO_EINVAL;
    if (dev >= 0 && dev < 64) cus = cus_of[dev];
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        if (dev >= 0 && dev < 64) cus_of[dev] = cus;
    }
    g.rows_per_slice = walker_row_slices(g.bx, Ho, cus, PROLOGUE_ROWS);   // one block per CU (134 KB of LDS, 8 waves)
    g.slices = (Ho + g.rows_per_slice - 1) / g.rows_per_slice;
    if (g.slices > 65535) return YOLO_EUNSUPPORTED;
    return YOLO_OK;
}

static int sr_shape_status(int N, int H, int W, int C1_, int C2_, int dtype) {
    if (N <= 0 || H <= 0 || W <= 0) return YOLO_EINVAL;
    if (C1_ != C1 || C2_ != C || (dtype != YOLO_BF16 && dtype != YOLO_F16) || (H & 1) || (W & 1)) return YOLO_EUNSUPPORTED;
    return YOLO_OK;
}

// The launch geometry yolo_stem_res_fwd uses for this shape on the current device (host only, no launch): column strips per
// image, their width, output rows per row slice and the number of row slices; the grid is (N * nstrips, slices).
extern "C" int yolo_stem_res_geometry(int N, int H, int W, int* nstrips, int* strip_w, int* rows_per_slice, int* slices) {
    if (!nstrips || !strip_w || !rows_per_slice || !slices) return YOLO_EINVAL;
    int rc = sr_shape_status(N, H, W, C1, C, YOLO_BF16);
    if (rc != YOLO_OK) return rc;
    SRGeom g;
    if ((rc = sr_geometry(N, H, W, g)) != YOLO_OK) return rc;
    *nstrips = g.nstrips; *strip_w = g.strip_w; *rows_per_slice = g.rows_per_slice; *slices = g.slices;
    return YOLO_OK;
}

// Fused stem + first down-sampling conv + first residual block (inference).  w0_oihw (32,3,3,3) float32; wd / w1 / w2_packed:
// yolo_pack_conv_weights images of the (64,32,3,3), (32,64,1,1) and (64,32,3,3) convs; scale / bias: folded BN of each layer.
extern "C" int yolo_stem_res_fwd(const float* x_nchw, const float* w0_oihw, const float* scale0, const float* bias0,
                                 const void* wd_packed, const float* scaled, const float* biasd, const void* w1_packed,
                                 const float* scale1, const float* bias1, const void* w2_packed, const float* scale2,
                                 const float* bias2, void* y, int N, int H, int W, int C1_, int C2_, int dtype, float slope,
                                 void* stream) {
    if (!x_nchw || !w0_oihw || !scale0 || !bias0 || !wd_packed || !scaled || !biasd || !w1_packed || !scale1 || !bias1 ||
        !w2_packed || !scale2 || !bias2 || !y)
        return YOLO_EINVAL;
    int rc = sr_shape_status(N, H, W, C1_, C2_, dtype);
    if (rc != YOLO_OK) return rc;
    if (!(slope >= 0.f && slope <= 1.f)) return YOLO_EINVAL;
    SRGeom g;
    if ((rc = sr_geometry(N, H, W, g)) != YOLO_OK) return rc;
    SRArgs a;
    a.x = x_nchw; a.w0 = w0_oihw; a.scale0 = scale0; a.bias0 = bias0;
    a.wpd = (const char*)wd_packed; a.scaled = scaled; a.biasd = biasd;
    a.wp1 = (const char*)w1_packed; a.scale1 = scale1; a.bias1 = bias1;
    a.wp2 = (const char*)w2_packed; a.scale2 = scale2; a.bias2 = bias2; a.y = (char*)y;
    a.N = N; a.H = H; a.W = W; a.Ho = H / 2; a.Wo = W / 2;
    a.Cpad = round_up(C, YOLO_COUT_PAD);                     // (= that of the 32-cout 1x1: both pad to YOLO_COUT_PAD)
    a.nstrips = g.nstrips; a.strip_w = g.strip_w; a.rows_per_slice = g.rows_per_slice;
    a.slope = slope;
    if (dtype == YOLO_F16)
        YOLO_LAUNCH(stem_res_kernel<f16_t>, dim3((unsigned)g.bx, (unsigned)g.slices), dim3(512), 0, (hipStream_t)stream, a);
    else
        YOLO_LAUNCH(stem_res_kernel<bf16_t>, dim3((unsigned)g.bx, (unsigned)g.slices), dim3(512), 0, (hipStream_t)stream, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
