// One DarknetBasicBlockV3 of the first two stages as ONE inference kernel (basic_yolo.py:26; gluoncv darknet.py:
// x + conv3x3(2c)(conv1x1(c)(x)), each conv with folded BN + LeakyReLU, no activation after the add), bf16 NHWC,
// for C = 2c in {64, 128}.
//
// Run as two kernels these blocks are HBM-bound three times over: the 1x1 reads x and writes the half-width map, the
// 3x3 reads that map and x again (the residual) and writes the output -- 2.5x the bytes of "read x, write out", at the
// largest maps of the network (15 % of the 608x608 pass).  Here the half-width map never leaves LDS and x is read once:
//   * a block (4 waves) owns a column strip (<= 62 output pixels) of one image and walks down its output rows, as
//     conv_stream_kernel / stem_down_kernel do; BOTH layers' weights stay in registers for the block's lifetime
//     (C = 64: 4 + 18 A-fragments per wave; C = 128: 8 + 36);
//   * input rows live in a rolling LDS ring (row oy: the residual of the output row; row oy + 1: the operand of the
//     1x1 for the mid row the 3x3 needs next); the loads of the NEXT D - 1 steps are in flight in registers meanwhile (a
//     row-step is a dependent chain load -> LDS -> 1x1 -> LDS -> 3x3 -> store of ~1.5k cycles, shorter than one HBM round
//     trip under load: with one row in flight the kernel ran at the memory latency, 2.7 us per row-step);
//   * the 1x1's output (mid) lives in a rolling LDS ring in the layout the 3x3 reads its B fragments from; it is
//     COMPUTED there.  Mid pixels outside the image are written as zeros: they are the 3x3's zero padding, not
//     conv1x1(padding);
//   * the 3x3 epilogue (conv_stream's: transpose through a per-wave LDS scratch, 16-byte row stores) takes its residual
//     from the input ring instead of reading x a second time.
// Measured (tools/rb_probe.py with ablation builds, 32 x 208 x 208 x 64: 144 us against 164 us for the two layers; HBM floor
// 56 us): the parts add up instead of overlapping -- 3x3 MFMAs 36 us, output stores 40, mid row 26, input loads 13,
// skeleton (barriers, ring fill, weights, transposes) 36 -- two waves per SIMD do not cover each other's latencies, and
// deeper register prefetch (D = 2, 4, 6 against 3) changed nothing.  Two kernels, one per width; the variants that lost (NOTES.md)
// are not built: one row per step at C = 128 ran its MFMA phase 6x below the matrix rate and lost to the two separate
// layers, two rows per step at C = 64 drops from two blocks per CU to one.
// Same packed weight images, operand rounding points (mid is rounded to bf16 once; the residual is added in fp32 before
// the output's one rounding) and K order ((kh, kw, channel)) as conv_stream_kernel.
#include "common.h"
#include "row_walk.h"

using namespace rw;

namespace {
constexpr int SW_MAX = MW - 2;           // mid / input rows are MW = 64 pixels (2 MFMA column groups) wide; strip width <= MW - 2

struct ResArgs {
    const char* x;
    const char* wp1;
    const float* scale1;
    const float* bias1;
    const char* wp2;
    const float* scale2;
    const float* bias2;
    char* y;
    int N, H, W, Cpad1, Cpad2;
    int nstrips, strip_w, rows_per_slice;
    float slope;
};
}  // namespace

// ---- one output row per step: C = 64, two blocks per CU ---------------------------------------------------------------
template <int C, typename T>
__global__ __launch_bounds__(256) void res_block_kernel(ResArgs a) {
    static_assert(C == 64, "waves = 2 cout slices x 2 pixel groups, one mid tile each for waves 0, 1 (C = 128: res_block2_kernel)");
    constexpr int D = 3;                                                      // register sets of input rows
    constexpr int CM = C / 2;
    constexpr int K1 = C / 16, K2 = CM / 16;                                  // k-steps of 16 channels
    constexpr int PX = C * 2 + 16, PM = CM * 2 + 16;                          // pixel pitch in the rings (+16: conflict-free reads)
    constexpr int XROW = MW * PX, MROW = (MW + 2) * PM;
    constexpr int XU = XStage<C>::XU;                                         // 16-byte input loads per thread per row
    __shared__ __attribute__((aligned(16))) char smem[3 * XROW + 3 * MROW + 4 * SCR];
    char* xl = smem;
    char* ml = smem + 3 * XROW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wave_c = wave & 1, wave_p = wave >> 1;                          // 3x3: wave = (cout slice, pixel group)
    char* scr = smem + 3 * XROW + 3 * MROW + wave * SCR;

    const int strip = blockIdx.x % a.nstrips;
    const int n = blockIdx.x / a.nstrips;
    const int ox0 = strip * a.strip_w;
    const int ox_end = min(ox0 + a.strip_w, a.W);
    const int oy0 = blockIdx.y * a.rows_per_slice;
    const int oy1 = min(oy0 + a.rows_per_slice, a.H);
    if (oy0 >= oy1) return;
    const int H = a.H, W = a.W;
    const int mx0 = ox0 - 1;                  // image column of ring pixel 0

    // ---- hygiene: ring pixels that are never written are only read by lanes whose results are discarded ----------
    for (int i = tid; i < (3 * XROW + 3 * MROW) / 16; i += 256) ((uint4*)smem)[i] = make_uint4(0, 0, 0, 0);

    // ---- weights and folded BN: the 3x3 (after the transpose), the 1x1 (wave w < 2 makes the mid tile of pixel group w) ---
    uint4 A2[9 * K2];
    load_a_frags<3, CM>(A2, a.wp2, a.Cpad2, wave_c * 32, lane);
    uint4 A1[K1];
    load_a_frags<1, C>(A1, a.wp1, a.Cpad1, 0, lane);
    float sc1[16], bi1[16];
    load_bn_mfma(sc1, bi1, a.scale1, a.bias1, 0, h);
    const int eco = wave_c * 32 + (lane & 3) * 8;
    float sc2[8], bi2[8];
    load_bn_row(sc2, bi2, a.scale2, a.bias2, eco);
    const float slope = a.slope;

    // ---- input rows: registers -> ring slot (row mod 3) ------------------------------------------------------------
    uint4 xr[D][XU];                                        // register sets: rows oy+2 .. oy+D in flight (static indices only)
    const XStage<C> xs(tid, mx0, W);
    auto slot3 = [](int row) { return (row + 3) % 3; };       // rows >= -1
    auto load_x = [&](uint4 (&r)[XU], int iy) { xs.load(r, a.x + (((long long)n * H + iy) * W + mx0) * (C * 2), iy >= 0 && iy < H); };
    auto store_x = [&](const uint4 (&r)[XU], int row) { xs.template store<PX>(r, xl + slot3(row) * XROW); };
    // ---- mid row my from the input ring: this wave's tile, BN + LeakyReLU, one rounding, zeros outside the image ---
    auto mid_row = [&](int my) {
        if (wave >= 2) return;
        const int px = wave * 32 + l31, mx = mx0 + px;
        mid_tile<T>(xl + slot3(my) * XROW + px * PX + h * 16, ml + slot3(my) * MROW + px * PM, A1, sc1, bi1, slope, h,
                    my >= 0 && my < H && mx >= 0 && mx < W);
    };

    __syncthreads();                                        // the zero fill
    // ---- prologue: input rows oy0-1, oy0, oy0+1; mid rows oy0-1, oy0 --------------------------------------------------
    load_x(xr[0], oy0 - 1);
    load_x(xr[1], oy0);
    store_x(xr[0], oy0 - 1);
    store_x(xr[1], oy0);
    load_x(xr[D - 1], oy0 + 1);
    // rows oy0+2 .. oy0+D go into sets 0 .. D-2 (set of row r = (r - oy0 - 2) % D); step oy stores set (oy - oy0) % D and
    // re-loads the set the previous step stored
#pragma unroll
    for (int k = 0; k < D - 1; ++k) load_x(xr[k], oy0 + 2 + k);   // (unconditional: XStage)
    __syncthreads();
    mid_row(oy0 - 1);
    mid_row(oy0);
    store_x(xr[D - 1], oy0 + 1);
    __syncthreads();

    for (int oyb = oy0; oyb < oy1; oyb += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int oy = oyb + u;
        if (oy >= oy1) break;
        const bool more = oy + 1 < oy1;
        load_x(xr[(u + D - 1) % D], oy + D + 1);             // D - 1 rows ahead of the row stored below (unconditional: XStage)
        mid_row(oy + 1);
        __syncthreads();

        // ---- 3x3 over mid rows oy-1 .. oy+1, then folded BN, LeakyReLU, + x (from the input ring), one rounding ---------
        f32x16 acc[1];
        conv3x3_rows<T, K2, 1, PM>(acc, A2, [&](int kh) { return ml + slot3(oy - 1 + kh) * MROW + (wave_p * 32 + l31) * PM + h * 16; },
                                   TapS1<PM>{});
        res_epilogue<T, C, PX>(scr, acc[0], lane, sc2, bi2, slope, xl + slot3(oy) * XROW + eco * 2,
                               a.y + ((((long long)n * H + oy) * W + ox0) * C + eco) * 2, wave_p * 32, ox_end - ox0);
        if (more) store_x(xr[u], oy + 2);
        __syncthreads();
    }
    }
}

// ---- two output rows per step: C = 128, one block per CU --------------------------------------------------------------
// The kernel above is latency-bound (tools/pmc_kernel.sh: an instruction active 35 % of the wave cycles, MFMA busy 34 %, VALU
// 35 %, LDS 20 %): one or two waves per SIMD walk a dependent chain per row step and nothing fills the gaps.  Here a step
// produces TWO output rows: two independent accumulator chains per wave, every B fragment of the two shared mid rows feeds
// two MFMAs (4 mid rows x 3 x K2 fragment reads for 2 x 9 x K2 MFMAs: a third less LDS traffic per MFMA), and the barriers,
// ring bookkeeping and loop overhead are paid once per two rows.  Input ring: 5 rows (oy, oy+1: residuals; oy+1, oy+2: operands
// of the step's mid rows; oy+3, oy+4: arriving); mid ring: 4 rows (oy-1 .. oy+2).  Same operands, accumulation order (kernel
// row, kernel column, channel) and rounding points.
template <int C, typename T>
__global__ __launch_bounds__(256) void res_block2_kernel(ResArgs a) {
    static_assert(C == 128, "waves = 4 cout slices of both pixel groups; 1x1: wave = (cout slice, pixel group) of both mid rows");
    constexpr int D = 2;                                                      // register sets: a set = the two rows one step stores
    constexpr int CM = C / 2;
    constexpr int NI = 2;
    constexpr int K1 = C / 16, K2 = CM / 16;
    constexpr int PX = C * 2 + 16, PM = CM * 2 + 16;
    constexpr int XROW = MW * PX, MROW = (MW + 2) * PM;
    constexpr int XU = XStage<C>::XU;
    constexpr int XR = 5, MR = 4;
    static_assert(XR * XROW + MR * MROW + 4 * SCR <= 163840, "LDS");
    __shared__ __attribute__((aligned(16))) char smem[XR * XROW + MR * MROW + 4 * SCR];
    char* xl = smem;
    char* ml = smem + XR * XROW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wave_c = wave % 4;                             // 3x3: the wave's cout slice, both pixel groups
    char* scr = smem + XR * XROW + MR * MROW + wave * SCR;

    const int strip = blockIdx.x % a.nstrips;
    const int n = blockIdx.x / a.nstrips;
    const int ox0 = strip * a.strip_w;
    const int ox_end = min(ox0 + a.strip_w, a.W);
    const int oy0 = blockIdx.y * a.rows_per_slice;
    const int oy1 = min(oy0 + a.rows_per_slice, a.H);
    if (oy0 >= oy1) return;
    const int H = a.H, W = a.W;
    const int mx0 = ox0 - 1;

    for (int i = tid; i < (XR * XROW + MR * MROW) / 16; i += 256) ((uint4*)smem)[i] = make_uint4(0, 0, 0, 0);

    uint4 A2[9 * K2];
    load_a_frags<3, CM>(A2, a.wp2, a.Cpad2, wave_c * 32, lane);
    const int m1 = wave % 2, p1 = wave / 2;                  // 1x1: this wave's mid tile (cout slice, 32-pixel group) of each row
    uint4 A1[K1];
    load_a_frags<1, C>(A1, a.wp1, a.Cpad1, m1 * 32, lane);
    float sc1[16], bi1[16];
    load_bn_mfma(sc1, bi1, a.scale1, a.bias1, m1 * 32, h);
    const int ecol = lane & 3, erow0 = lane >> 2;
    const int eco = wave_c * 32 + ecol * 8;
    float sc2[8], bi2[8];
    load_bn_row(sc2, bi2, a.scale2, a.bias2, eco);
    const float slope = a.slope;

    uint4 xr[D][2][XU];
    const XStage<C> xs(tid, mx0, W);
    auto xslot = [](int row) { return (row + XR) % XR; };    // rows >= -1
    auto mslot = [](int row) { return (row + MR) & (MR - 1); };
    auto load_x = [&](uint4 (&r)[XU], int iy) { xs.load(r, a.x + (((long long)n * H + iy) * W + mx0) * (C * 2), iy >= 0 && iy < H); };
    auto store_x = [&](const uint4 (&r)[XU], int row) { xs.template store<PX>(r, xl + xslot(row) * XROW); };
    auto mid_row = [&](int my) {
        const int px = p1 * 32 + l31, mx = mx0 + px;
        mid_tile<T>(xl + xslot(my) * XROW + px * PX + h * 16, ml + mslot(my) * MROW + px * PM + m1 * 64, A1, sc1, bi1, slope, h,
                    my >= 0 && my < H && mx >= 0 && mx < W);
    };

    __syncthreads();                                        // the zero fill
    // ---- prologue: input rows oy0-1 .. oy0+2 into the ring, mid rows oy0-1, oy0 ------------------------------------------
    load_x(xr[0][0], oy0 - 1);
    load_x(xr[0][1], oy0);
    store_x(xr[0][0], oy0 - 1);
    store_x(xr[0][1], oy0);
    load_x(xr[0][0], oy0 + 1);
    load_x(xr[0][1], oy0 + 2);
    store_x(xr[0][0], oy0 + 1);
    store_x(xr[0][1], oy0 + 2);
    // step k (output rows oy0 + 2k, + 1) stores rows oy0 + 2k + 3, + 4 from set k % D; sets 0 .. D-2 are requested here, set
    // (k - 1) % D is re-requested at the top of step k with the rows of step k + D - 1 (unconditionally: XStage)
#pragma unroll
    for (int k = 0; k < D - 1; ++k) { load_x(xr[k][0], oy0 + 2 * k + 3); load_x(xr[k][1], oy0 + 2 * k + 4); }
    __syncthreads();
    mid_row(oy0 - 1);
    mid_row(oy0);
    __syncthreads();

    for (int oyb = oy0; oyb < oy1; oyb += 2 * D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int oy = oyb + 2 * u;
        if (oy >= oy1) break;
        load_x(xr[(u + D - 1) % D][0], oy + 2 * D + 1);
        load_x(xr[(u + D - 1) % D][1], oy + 2 * D + 2);
        mid_row(oy + 1);                                     // mid rows oy + 1, oy + 2 from input rows oy + 1, oy + 2
        mid_row(oy + 2);
        __syncthreads();

        // ---- 3x3 of output rows oy, oy + 1 over mid rows oy - 1 .. oy + 2: every fragment of the shared rows feeds both ------
        f32x16 acc[2][NI];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[r][ni][e] = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const char* rowp = ml + mslot(oy - 1 + m) * MROW + l31 * PM + h * 16;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int kc = 0; kc < K2; ++kc)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        const uint4 bf = *(const uint4*)(rowp + (ni * 32 + kw) * PM + kc * 32);
                        if (m <= 2)
                            acc[0][ni] = mfma16<T>(A2[(m * 3 + kw) * K2 + kc], bf, acc[0][ni]);
                        if (m >= 1)
                            acc[1][ni] = mfma16<T>(A2[((m - 1) * 3 + kw) * K2 + kc], bf, acc[1][ni]);
                    }
        }
        // ---- epilogue of both rows (an odd slice ends in a half-used step): row_walk.h's res_epilogue, spelled out ---------------
        // Through the shared function this kernel (one wave per SIMD, 406 registers) was scheduled with each pixel row's
        // residual read AFTER the wait for its scratch reads and measured +2.4 .. +4.6 % against its parent (NOTES.md); in this
        // form the three LDS reads of a pixel row are issued together, as before.  The layout constants are row_walk.h's.
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (oy + r >= oy1) break;
            const char* xres = xl + xslot(oy + r) * XROW + eco * 2;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v = {acc[r][ni][4 * g], acc[r][ni][4 * g + 1], acc[r][ni][4 * g + 2], acc[r][ni][4 * g + 3]};
                    *(f32x4*)(scr + l31 * SCR_PITCH + (8 * g + 4 * h) * 4) = v;
                }
                wave_lds_fence();
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int px = ni * 32 + erow0 + 16 * k;
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const f32x4 t4 = *(const f32x4*)(scr + (erow0 + 16 * k) * SCR_PITCH + (ecol * 8 + 4 * q) * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[4 * q + e] = t4[e];
                    }
                    const uint4 rv = *(const uint4*)(xres + (px + 1) * PX);
                    const uint32_t w[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = leaky(v[e] * sc2[e] + bi2[e], slope);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        v[2 * q] += Elem<T>::lo(w[q]);
                        v[2 * q + 1] += Elem<T>::hi(w[q]);
                    }
                    const int ox = ox0 + px;
                    if (ox < ox_end)
                        *(uint4*)(a.y + ((((long long)n * H + oy + r) * W + ox) * C + eco) * 2) =
                            make_uint4(Elem<T>::pack2(v[0], v[1]), Elem<T>::pack2(v[2], v[3]), Elem<T>::pack2(v[4], v[5]), Elem<T>::pack2(v[6], v[7]));
                }
            }
        }
        if (oy + 2 < oy1) { store_x(xr[u][0], oy + 3); store_x(xr[u][1], oy + 4); }
        __syncthreads();
    }
    }
}

template <typename T>
static int launch_res_block(ResArgs& a, int C, hipStream_t st) {
    walker_strips(a.W, SW_MAX, a.nstrips, a.strip_w);
    const long long bx = (long long)a.N * a.nstrips;
    if (bx > 0x7fffffffLL) return YOLO_EUNSUPPORTED;
    // row slices (walker_row_slices): a slice's prologue is the ring fill, two extra mid rows and the weights.  C = 64: two
    // resident blocks per CU; C = 128: one (140 KB of LDS), and even slices -- no half-used step in the middle of the image
    if (C == 64) {
        a.rows_per_slice = walker_row_slices(bx, a.H, 512, 3.5);
    } else {
        a.rows_per_slice = walker_row_slices(bx, a.H, 256, 4.5);
        a.rows_per_slice += a.rows_per_slice & 1;
    }
    const dim3 grid((unsigned)bx, (unsigned)((a.H + a.rows_per_slice - 1) / a.rows_per_slice));
    // two output rows per step at C = 128 only: 102 against 117 us at 32 x 104 x 104, 474 against 507 at 64 x 152 x 152 (same-box
    // probes); at C = 64 it loses, 141 against 122 us
    if (C == 64)
        YOLO_LAUNCH((res_block_kernel<64, T>), grid, dim3(256), 0, st, a);
    else
        YOLO_LAUNCH((res_block2_kernel<128, T>), grid, dim3(256), 0, st, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// Fused residual block (inference): y = x + lrelu(bn2(conv3x3(lrelu(bn1(conv1x1(x)))))); x, y (N,H,W,C) bf16 NHWC;
// w1_packed / w2_packed: yolo_pack_conv_weights images of the (C/2, C, 1, 1) and (C, C/2, 3, 3) convs; scale / bias:
// yolo_fold_bn of each layer.  bf16 / f16, C in {64, 128} only (YOLO_EUNSUPPORTED otherwise: run the two layers separately).
extern "C" int yolo_res_block_fwd(const void* x, const void* w1_packed, const float* scale1, const float* bias1,
                                  const void* w2_packed, const float* scale2, const float* bias2, void* y, int N, int H,
                                  int W, int C, int dtype, float slope, void* stream) {
    if (!x || !w1_packed || !scale1 || !bias1 || !w2_packed || !scale2 || !bias2 || !y || N <= 0 || H <= 0 || W <= 0)
        return YOLO_EINVAL;
    if (!(slope >= 0.f && slope <= 1.f)) return YOLO_EINVAL;
    if ((dtype != YOLO_BF16 && dtype != YOLO_F16) || (C != 64 && C != 128)) return YOLO_EUNSUPPORTED;
    ResArgs a;
    a.x = (const char*)x; a.wp1 = (const char*)w1_packed; a.scale1 = scale1; a.bias1 = bias1;
    a.wp2 = (const char*)w2_packed; a.scale2 = scale2; a.bias2 = bias2; a.y = (char*)y;
    a.N = N; a.H = H; a.W = W; a.slope = slope;
    a.Cpad1 = round_up(C / 2, YOLO_COUT_PAD); a.Cpad2 = round_up(C, YOLO_COUT_PAD);
    hipStream_t st = (hipStream_t)stream;
    return dtype == YOLO_F16 ? launch_res_block<f16_t>(a, C, st) : launch_res_block<bf16_t>(a, C, st);
}
