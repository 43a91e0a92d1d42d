// The network's first two layers as ONE inference kernel: the stem _conv2d (basic_yolo.py:20: Conv3x3 s1 p1, 3 -> 32)
// and the first stage's down-sampling _conv2d (basic_yolo.py:24: Conv3x3 s2 p1, 32 -> 64), each with folded BN +
// LeakyReLU, from the (N,3,H,W) float32 NCHW image to the (N,H/2,W/2,64) bf16 NHWC map.
//
// Run separately (stem.hip + conv_stream.hip) both are HBM-bound on the full-resolution 32-channel map between them:
// written once and read once it is 3.0 GB of the 3.3 GB the two kernels move at 608x608 bs 64 (1.0 ms of a 15.8 ms
// forward pass).  Here it never leaves LDS:
//   * a block (4 waves) owns a column strip (<= 62 output pixels) of one image and walks down its output rows, as
//     conv_stream_kernel does; the down conv's weights stay in registers (18 A-fragments per wave);
//   * the stem output lives in a 5-row rolling LDS ring in exactly the layout conv_stream stages its input in, but it
//     is COMPUTED there: each step the four waves produce the two new stem rows (3 MFMAs per 32 pixels, K = one kernel
//     row of the NHWC4 image as in stem.hip) from an 8-row rolling image window, while the image rows of the next
//     step are in flight in registers;
//   * stem pixels outside the image are written as zeros (they are the down conv's zero padding, NOT stem(padding)).
// Same operand order, accumulation order and rounding points as the two separate kernels: results are bit-identical.
#include "common.h"
#include "row_walk.h"
#include <type_traits>

using namespace rw;

namespace {
constexpr int C1 = STEM_C, C2 = 64;
// a step covers 64 output pixels (MFMA columns); the usable strip width is <= 62 so that a stem row is 4 groups of 32
constexpr int SW_MAX = 62;

struct Args {
    const float* x;
    const float* w1;
    const float* scale1;
    const float* bias1;
    const char* wp2;
    const float* scale2;
    const float* bias2;
    char* y;
    int N, H, W, Ho, Wo, Cout_pad2;
    int nstrips, strip_w, rows_per_slice;
    float slope;
};
}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void stem_down_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) char smem[RING * STEM_ROW + IROWS * IPW * 8 + 4 * SCR];
    char* xl = smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int wave_c = wave & 1, wave_p = wave >> 1;
    char* scr = smem + RING * STEM_ROW + IROWS * IPW * 8 + wave * SCR;

    const int strip = blockIdx.x % a.nstrips;
    const int n = blockIdx.x / a.nstrips;
    const int ox0 = strip * a.strip_w;
    const int ox_end = min(ox0 + a.strip_w, a.Wo);
    const int oy0 = blockIdx.y * a.rows_per_slice;
    const int oy1 = min(oy0 + a.rows_per_slice, a.Ho);
    if (oy0 >= oy1) return;
    const int Ho = a.Ho, Wo = a.Wo;
    StemWin sw;
    sw.HW = (long long)a.H * a.W;
    sw.xn = a.x + (long long)n * 3 * sw.HW;
    sw.H = a.H; sw.W = a.W;
    sw.sx0 = 2 * ox0 - 1;
    sw.icol0 = sw.sx0 - 1;
    sw.iyb = 2 * oy0 - 2;
    sw.img = (uint2*)(smem + RING * STEM_ROW);
    sw.ring = xl;
    sw.tid = tid;
    const int iyb = sw.iyb;

    // ---- hygiene: pixels of both LDS arrays that are never written are only read by discarded lanes ---------------
    for (int i = tid; i < (RING * STEM_ROW + IROWS * IPW * 8) / 16; i += 256) ((uint4*)smem)[i] = make_uint4(0, 0, 0, 0);

    // ---- the wave's weights and folded-BN constants: down conv (32 couts x K = 288; after the transpose), stem (MFMA layout) ----
    uint4 A[18];
    load_a_frags<3, C1>(A, a.wp2, a.Cout_pad2, wave_c * 32, lane);
    uint4 wf[3];
    stem_weight_frags<T>(wf, a.w1, lane);
    const int ecol = lane & 3, erow0 = lane >> 2;
    const int eco = wave_c * 32 + ecol * 8;
    float sc2[8], bi2[8];
    load_bn_row(sc2, bi2, a.scale2, a.bias2, eco);
    const float slope = a.slope;
    float sc1[16], bi1[16];
    load_bn_mfma(sc1, bi1, a.scale1, a.bias1, 0, h);

    __syncthreads();                                        // the zero fill
    // ---- prologue: image rows iyb .. iyb+6, then stem rows 2 oy0 - 1 .. 2 oy0 + 1 into ring slots 0..2 ------------
    {
        float c[4][3];
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) load_img(sw, iyb, r, c[r], ok[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r < 3 || tid < 128) store_img<T>(sw, iyb, r, c[r], ok[r]);      // 7 rows: the 8th slot belongs to row iyb + 7
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 3; ++r) stem_group<T>(sw, wf, sc1, bi1, slope, lane, 2 * oy0 - 1 + r, r, wave);
    __syncthreads();

    const int b_off = (wave_p * 32 + l31) * PITCH + h * 16;
    int slot0 = 0;
    // image rows 2oy+5, 2oy+6 are used by step oy+1's stem rows and stored at the bottom of step oy; they are requested TWO
    // steps ahead (top of step oy-1) into one of two register sets (load_img)
    float cimg[2][3];
    bool okimg[2] = {false, false};
    load_img(sw, 2 * oy0 + 5, 0, cimg[0], okimg[0]);
    auto step = [&](auto par_c, int oy) {
        constexpr int PAR = decltype(par_c)::value;
        const bool more = oy + 1 < oy1;
        load_img(sw, 2 * oy + 7, 0, cimg[PAR ^ 1], okimg[PAR ^ 1]);
        long long yo[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ox = ox0 + wave_p * 32 + erow0 + 16 * k;
            yo[k] = ox < ox_end ? ((((long long)n * Ho + oy) * Wo + ox) * C2 + eco) * 2 : -1;
        }
        // ---- down conv of output row oy: 9 taps x 2 k-steps over the stem ring ----------------------------------
        f32x16 acc[1];
        conv3x3_rows<T, 2, 1, PITCH>(acc, A, [&](int kh) {
            int slot = slot0 + kh;
            if (slot >= RING) slot -= RING;
            return xl + slot * STEM_ROW + b_off;
        }, TapS2{});
        // ---- the two stem rows the next output row adds (2oy+2, 2oy+3): this wave's pixel group of each ----------
        if (more) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int slot = slot0 + 3 + r;
                if (slot >= RING) slot -= RING;
                stem_group<T>(sw, wf, sc1, bi1, slope, lane, 2 * oy + 2 + r, slot, wave);
            }
        }
        // ---- epilogue of the down conv: folded BN, LeakyReLU, one rounding, 16-byte row stores --------------------
        row_epilogue<T>(scr, acc[0], lane, sc2, bi2, slope, [](int) { return NoResidual{}; },
                        [&](int k, const uint4& o) { if (yo[k] >= 0) *(uint4*)(a.y + yo[k]) = o; });
        if (more) store_img<T>(sw, 2 * oy + 5, 0, cimg[PAR], okimg[PAR]);
        slot0 += 2;
        if (slot0 >= RING) slot0 -= RING;
        __syncthreads();
    };
    for (int oy = oy0; oy < oy1; oy += 2) {
        step(std::integral_constant<int, 0>{}, oy);
        if (oy + 1 < oy1) step(std::integral_constant<int, 1>{}, oy + 1);
    }
}

// Fused stem + first down-sampling conv (inference).  w1_oihw (32,3,3,3) float32; w2_packed: yolo_pack_conv_weights image
// of the (64,32,3,3) conv; scale / bias: folded BN of each layer.  bf16 only; C1 == 32 and C2 == 64 only.
extern "C" int yolo_stem_down_fwd(const float* x_nchw, const float* w1_oihw, const float* scale1, const float* bias1,
                                  const void* w2_packed, const float* scale2, const float* bias2, void* y, int N, int H,
                                  int W, int C1_, int C2_, int dtype, float slope, void* stream) {
    if (!x_nchw || !w1_oihw || !scale1 || !bias1 || !w2_packed || !scale2 || !bias2 || !y || N <= 0 || H <= 0 || W <= 0)
        return YOLO_EINVAL;
    if (!(slope >= 0.f && slope <= 1.f)) return YOLO_EINVAL;
    if (C1_ != C1 || C2_ != C2 || (dtype != YOLO_BF16 && dtype != YOLO_F16)) return YOLO_EUNSUPPORTED;
    Args a;
    a.x = x_nchw; a.w1 = w1_oihw; a.scale1 = scale1; a.bias1 = bias1;
    a.wp2 = (const char*)w2_packed; a.scale2 = scale2; a.bias2 = bias2; a.y = (char*)y;
    a.N = N; a.H = H; a.W = W; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
    a.Cout_pad2 = round_up(C2, YOLO_COUT_PAD);
    a.slope = slope;
    walker_strips(a.Wo, SW_MAX, a.nstrips, a.strip_w);
    const long long bx = (long long)N * a.nstrips;
    if (bx > 0x7fffffffLL) return YOLO_EUNSUPPORTED;
    long long slices = (1536 + bx - 1) / bx;                 // a slice re-computes 3 stem rows: keep them >= 16 rows
    if (slices > a.Ho / 16) slices = a.Ho / 16;
    if (slices < 1) slices = 1;
    a.rows_per_slice = (int)((a.Ho + slices - 1) / slices);
    slices = (a.Ho + a.rows_per_slice - 1) / a.rows_per_slice;
    if (dtype == YOLO_F16)
        YOLO_LAUNCH(stem_down_kernel<f16_t>, dim3((unsigned)bx, (unsigned)slices), dim3(256), 0, (hipStream_t)stream, a);
    else
        YOLO_LAUNCH(stem_down_kernel<bf16_t>, dim3((unsigned)bx, (unsigned)slices), dim3(256), 0, (hipStream_t)stream, a);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
