// The formats the row-walker kernels share (conv_stream.hip, stem_down.hip, res_block.hip, stem_res.hip), each defined once:
// the packed-weight A fragments, the folded-BN constants in the two layouts a lane meets them in, the tile store from the MFMA
// layout, the transpose through a wave's LDS scratch with the epilogue on top of it, the stem computed into an LDS ring, the
// 1x1 and 3x3 of a ring, the residual block's input-row staging, and on the host the strip split and the row-slice search.
// A walker is a block that owns a column strip of one image and walks down its output rows with its weights in registers;
// what differs between the walkers (schedule, barriers, ring sizes, LDS map) stays in their files.
// Lane coordinates throughout: l31 = lane & 31 (the cout of an A fragment / the pixel of a B fragment), h = lane >> 5 (the
// k-half); after the transpose a lane owns the 8 couts ecol * 8 .. of pixel rows erow0 and erow0 + 16.
#pragma once
#include "common.h"

namespace rw {

// ---- packed-weight A fragments ------------------------------------------------------------------------------------------------
// The wave's A fragments of couts cout0 .. cout0 + 31 for every K step (tap-major, then 16-channel steps) of a KS x KS conv over
// CIN channels, straight from the yolo_pack_conv_weights image: 64-byte chunks of 32 channels per (chunk, tap, cout), their four
// 16-byte units swizzled by the cout.
template <int KS, int CIN>
__device__ __forceinline__ void load_a_frags(uint4 (&A)[KS * KS * (CIN / 16)], const char* wp, int cout_pad, int cout0, int lane) {
    constexpr int NTAP = KS * KS, KC = CIN / 16;
    const int l31 = lane & 31, h = lane >> 5;
    const int row = cout0 + l31, swz = (l31 >> 2) & 3;
#pragma unroll
    for (int ks = 0; ks < NTAP * KC; ++ks) {
        const int tap = ks / KC, kc = ks % KC;
        const int chunk = kc >> 1, unit = ((kc & 1) * 2 + h) ^ swz;
        A[ks] = *(const uint4*)(wp + ((long long)(chunk * NTAP + tap) * cout_pad + row) * 64 + unit * 16);
    }
}

// ---- folded-BN constants ------------------------------------------------------------------------------------------------------
// the 16 couts a lane holds after its MFMAs: rows 8g + 4h + e of the 32-cout slice at c0
__device__ __forceinline__ void load_bn_mfma(float (&sc)[16], float (&bi)[16], const float* scale, const float* bias, int c0, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 s4 = *(const f32x4*)(scale + c0 + 8 * g + 4 * h), b4 = *(const f32x4*)(bias + c0 + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[4 * g + e] = s4[e]; bi[4 * g + e] = b4[e]; }
    }
}
// the 8 couts eco .. eco + 7 of a pixel row a lane owns after the transpose (entries 0 .. 7)
template <int N>
__device__ __forceinline__ void load_bn_row(float (&sc)[N], float (&bi)[N], const float* scale, const float* bias, int eco) {
    static_assert(N >= 8, "8 couts");
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const f32x4 s4 = *(const f32x4*)(scale + eco + 4 * q), b4 = *(const f32x4*)(bias + eco + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[4 * q + e] = s4[e]; bi[4 * q + e] = b4[e]; }
    }
}

template <typename T> __device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    return make_uint4(Elem<T>::pack2(v[0], v[1]), Elem<T>::pack2(v[2], v[3]), Elem<T>::pack2(v[4], v[5]), Elem<T>::pack2(v[6], v[7]));
}
// v += the 8 stored values of rv, in fp32 (a residual is added before the output's one rounding)
template <typename T> __device__ __forceinline__ void add8(float (&v)[8], const uint4& rv) {
    const uint32_t w[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[2 * q] += Elem<T>::lo(w[q]);
        v[2 * q + 1] += Elem<T>::hi(w[q]);
    }
}

// ---- MFMA-layout tile store ---------------------------------------------------------------------------------------------------
// One 32 x 32 accumulator (32 couts of this lane's pixel): folded BN, LeakyReLU, one rounding, four 8-byte stores of couts
// 8g + 4h .. + 3 at `pixel` (the address of the slice's cout 0 of the lane's pixel in an LDS ring) -- no transpose.  A pixel
// outside the map is written as ZEROS: it is the next conv's zero padding, not conv(padding).
template <typename T>
__device__ __forceinline__ void store_tile(char* pixel, const f32x16& acc, const float (&sc)[16], const float (&bi)[16], float slope,
                                           int h, bool inside) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = leaky(acc[4 * g + e] * sc[4 * g + e] + bi[4 * g + e], slope);
        *(uint2*)(pixel + (8 * g + 4 * h) * 2) = inside ? make_uint2(Elem<T>::pack2(v[0], v[1]), Elem<T>::pack2(v[2], v[3])) : make_uint2(0u, 0u);
    }
}

// ---- scratch transpose --------------------------------------------------------------------------------------------------------
// A wave turns an accumulator (lane = pixel, 16 couts) into pixel rows (lane = 8 couts of two pixels) through a private LDS
// scratch of 32 pixel rows x (32 f32 + pad), so that the output leaves in 16-byte row stores.
constexpr int SCR_PITCH = 144;
constexpr int SCR = 32 * SCR_PITCH;
__device__ __forceinline__ void scratch_put(char* scr, const f32x16& acc, int lane) {
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        *(f32x4*)(scr + l31 * SCR_PITCH + (8 * g + 4 * h) * 4) = v;
    }
    wave_lds_fence();
}
// the lane's 8 couts of pixel row (lane >> 2) + 16 k
__device__ __forceinline__ void scratch_get(float (&v)[8], const char* scr, int lane, int k) {
    const int ecol = lane & 3, erow = (lane >> 2) + 16 * k;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const f32x4 t4 = *(const f32x4*)(scr + erow * SCR_PITCH + (ecol * 8 + 4 * q) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = t4[e];
    }
}
// The epilogue of a 32-pixel tile on top of the transpose: folded BN, LeakyReLU, + residual in fp32, one rounding.  For each of the
// lane's two pixel rows k (pixel (lane >> 2) + 16 k of the tile, couts (lane & 3) * 8 ..): residual(k) returns the 16 bytes to add
// (or NoResidual{}), store(k, packed) writes the 16 bytes (or drops them).  The residual is requested together with the scratch
// reads, ahead of the arithmetic: asked for after it, each pixel row waited twice for LDS.
struct NoResidual {};
template <typename T> __device__ __forceinline__ void add8(float (&)[8], NoResidual) {}
template <typename T, int N, typename Res, typename Store>
__device__ __forceinline__ void row_epilogue(char* scr, const f32x16& acc, int lane, const float (&sc)[N], const float (&bi)[N],
                                             float slope, Res&& residual, Store&& store) {
    scratch_put(scr, acc, lane);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float v[8];
        scratch_get(v, scr, lane, k);
        const auto rv = residual(k);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = leaky(v[e] * sc[e] + bi[e], slope);
        add8<T>(v, rv);
        store(k, pack8<T>(v));
    }
}
// The residual block's form, for the tile of strip pixels px0 .. px0 + 31: the residual is the block's own input, ring pixel
// px + 1 of `xres` (the input-ring row of this output row at the lane's couts, pixel pitch PX; ring pixel 0 is the strip's left
// halo); pixel px < npx is stored at ypix + px * C * 2 (ypix: the lane's couts of the strip's first pixel in the output row).
template <typename T, int C, int PX, int N>
__device__ __forceinline__ void res_epilogue(char* scr, const f32x16& acc, int lane, const float (&sc)[N], const float (&bi)[N],
                                             float slope, const char* xres, char* ypix, int px0, int npx) {
    const int px = px0 + (lane >> 2);
    row_epilogue<T>(scr, acc, lane, sc, bi, slope,
                    [&](int k) { return *(const uint4*)(xres + (px + 16 * k + 1) * PX); },
                    [&](int k, const uint4& o) { if (px + 16 * k < npx) *(uint4*)(ypix + (long long)(px + 16 * k) * (C * 2)) = o; });
}

// ---- the stem computed into an LDS ring -----------------------------------------------------------------------------------------
// The stem (Conv3x3 s1, 3 -> 32) of a strip lives in a rolling ring of stem rows that a stride-2 3x3 reads; it is computed there,
// two rows per step, from an 8-row rolling window of the image held as NHWC4 pixels (K = one kernel row, as in stem.hip).
constexpr int STEM_C = 32;
constexpr int XW = 129;                  // stem ring row capacity (pixel 128 is only read by discarded lanes)
constexpr int PITCH = STEM_C * 2 + 16;   // bytes per stem pixel in the ring (+16: conflict-free 16-byte reads)
// A ring row holds its even pixels first, then the odd ones (pixel p at ((p & 1) * XHALF + (p >> 1)) * PITCH): the stride-2 down conv
// reads every other pixel, and at a lane stride of 2 * PITCH = 160 bytes a 16-lane ds_read_b128 group covers only 8 of the 16 bank
// quads (two-way conflicts on every fragment read: SQ_LDS_BANK_CONFLICT was 34 % of the LDS-active cycles); at PITCH it covers all 16.
constexpr int XHALF = (XW + 1) / 2;
constexpr int STEM_ROW = XW * PITCH;
constexpr int RING = 5;                  // 3 stem rows in use + 2 being produced
constexpr int IPW = 136;                 // image window row pitch in pixels (8 B each: NHWC4)
constexpr int IROWS = 8;                 // image window rows (4 in use + 2 arriving, power of two)
__device__ __forceinline__ constexpr int stem_px_off(int px) { return ((px & 1) * XHALF + (px >> 1)) * PITCH; }

// the stem's weight fragments (cout = l31, k-half h), one per kernel row, from the OIHW fp32 weights (stem.hip's K order)
template <typename T, int N>
__device__ __forceinline__ void stem_weight_frags(uint4 (&wf)[N], const float* w, int lane) {
    static_assert(N >= 3, "one per kernel row");
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        float v[2][3];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const int kw = 2 * h + q;          // h=0: kw 0,1 ; h=1: kw 2,(3 = padding)
                v[q][ci] = kw < 3 ? w[((l31 * 3 + ci) * 3 + kh) * 3 + min(kw, 2)] : 0.f;
            }
        wf[kh] = make_uint4(Elem<T>::pack2(v[0][0], v[0][1]), Elem<T>::pack2(v[0][2], 0.f), Elem<T>::pack2(v[1][0], v[1][1]),
                            Elem<T>::pack2(v[1][2], 0.f));
    }
}

// where a strip's image window and stem ring sit: tid counts the 256 threads that stage the window
struct StemWin {
    const float* xn;                     // the image's three planes
    long long HW;
    int H, W;
    int icol0;                           // image column of window pixel 0
    int sx0;                             // image column of stem pixel 0 (= icol0 + 1)
    int iyb;                             // image row held in window slot 0 at the start
    uint2* img;                          // the window: IROWS x IPW pixels
    char* ring;                          // the stem ring: RING x STEM_ROW bytes
    int tid;
};
// image window: one pixel (3 planes) per thread per pass of two rows; pass r of the rows from iy_first.  The load is unconditional
// from a clamped address (always readable) and `ok` says whether the pixel is inside the image: the walkers request rows TWO steps
// ahead into one of two register sets, and a branch around a request would make the compiler wait for every load in flight
// before the other set's store.
__device__ __forceinline__ void load_img(const StemWin& s, int iy_first, int r, float (&c)[3], bool& ok) {
    const int q = s.tid & 127;
    const int iy = iy_first + r * 2 + (s.tid >> 7), ix = s.icol0 + q;
    ok = iy >= 0 && iy < s.H && ix >= 0 && ix < s.W;
    const long long o = (long long)min(max(iy, 0), s.H - 1) * s.W + min(max(ix, 0), s.W - 1);
    c[0] = s.xn[o]; c[1] = s.xn[s.HW + o]; c[2] = s.xn[2 * s.HW + o];
}
template <typename T>
__device__ __forceinline__ void store_img(const StemWin& s, int iy_first, int r, const float (&c)[3], bool ok) {
    const int q = s.tid & 127;
    const int iy = iy_first + r * 2 + (s.tid >> 7);
    s.img[((iy - s.iyb) & (IROWS - 1)) * IPW + q] = ok ? make_uint2(Elem<T>::pack2(c[0], c[1]), Elem<T>::pack2(c[2], 0.f)) : make_uint2(0u, 0u);
}
// one group of 32 stem pixels of stem row sy: 3 MFMAs, BN + LeakyReLU, one rounding, into ring slot `slot`
template <typename T, int N>
__device__ __forceinline__ void stem_group(const StemWin& s, const uint4 (&wf)[N], const float (&sc)[16], const float (&bi)[16],
                                           float slope, int lane, int sy, int slot, int pxg) {
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int p = ((sy - 1 + kh - s.iyb) & (IROWS - 1)) * IPW + pxg * 32 + l31 + 2 * h;
        const uint2 lo = s.img[p], hi = s.img[p + 1];
        acc = mfma16<T>(wf[kh], make_uint4(lo.x, lo.y, hi.x, hi.y), acc);
    }
    const int px = pxg * 32 + l31;
    const int sx = s.sx0 + px;
    const bool inside = sy >= 0 && sy < s.H && sx >= 0 && sx < s.W;
    store_tile<T>(s.ring + slot * STEM_ROW + stem_px_off(px), acc, sc, bi, slope, h, inside);
}

// ---- the convs of a ring ------------------------------------------------------------------------------------------------------
// 1x1 mid row: K1 MFMAs over this lane's ring pixel (xp: its channel 8h), then the tile store at `pixel` of the mid ring
template <typename T, int K1>
__device__ __forceinline__ void mid_tile(const char* xp, char* pixel, const uint4 (&A1)[K1], const float (&sc)[16], const float (&bi)[16],
                                         float slope, int h, bool inside) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kc = 0; kc < K1; ++kc) acc = mfma16<T>(A1[kc], *(const uint4*)(xp + kc * 32), acc);
    store_tile<T>(pixel, acc, sc, bi, slope, h, inside);
}
// byte offset of kernel column kw from the lane's pixel: in a plain ring row | in an even/odd-split row read at stride 2
template <int PITCH_> struct TapS1 { __device__ __forceinline__ constexpr int operator()(int kw) const { return kw * PITCH_; } };
struct TapS2 { __device__ __forceinline__ constexpr int operator()(int kw) const { return stem_px_off(kw); } };
// 3x3 over three ring rows: acc[ni] += 9 taps x KC k-steps for NI groups of 32 pixels; rowp(kh) is the address of the lane's
// pixel (channel 8h) of group 0 in the ring row of kernel row kh, groups lie 32 * PITCH_ bytes apart
template <typename T, int KC, int NI, int PITCH_, typename RowPtr, typename Tap>
__device__ __forceinline__ void conv3x3_rows(f32x16 (&acc)[NI], const uint4 (&A)[9 * KC], RowPtr&& rowp, Tap tap) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const char* p = rowp(kh);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int kc = 0; kc < KC; ++kc)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const uint4 bf = *(const uint4*)(p + ni * 32 * PITCH_ + tap(kw) + kc * 32);
                    acc[ni] = mfma16<T>(A[(kh * 3 + kw) * KC + kc], bf, acc[ni]);
                }
    }
}

// ---- input-row staging of the residual block ----------------------------------------------------------------------------------
// A row of MW = 64 pixels x C channels from image column mx0 on: XU 16-byte units per thread of a 256-thread block, through
// registers into a ring row of pixel pitch PX.
// The loads are unconditional range-checked buffer loads (a unit outside the image gets an out-of-range offset and reads zeros): a
// predicated load is a zero-initialisation + an exec branch, and the compiler waits for EVERY load in flight before each
// zero-initialisation -- which serialised the register sets a walker keeps in flight.  For the same reason the walkers request
// rows unconditionally (rows past the slice are read and dropped): behind a uniform branch the compiler's s_waitcnt for the
// stores of the other sets must assume the no-load path, i.e. wait for every load in flight -- the sets then behave like one.
constexpr int MW = 64;
template <int C> struct XStage {
    static constexpr int PARTS = C * 2 / 16, XU = MW * PARTS / 256;
    static_assert(MW * PARTS % 256 == 0, "input row = whole passes of the block");
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    int off[XU];                         // byte offset of the thread's units from a row's first pixel, -1 outside the image
    int tid;
    __device__ __forceinline__ XStage(int tid_, int mx0, int W) : tid(tid_) {
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            const int u = tid + j * 256;
            const int px = u / PARTS, part = u % PARTS;
            const int ix = mx0 + px;
            off[j] = (ix >= 0 && ix < W) ? px * (C * 2) + part * 16 : -1;
        }
    }
    // row_base: the address of pixel (iy, mx0) of the image (never dereferenced outside the map); row_ok: 0 <= iy < H
    __device__ __forceinline__ void load(uint4 (&r)[XU], const char* row_base, bool row_ok) const {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)row_base, 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, row_ok ? off[j] : -1, 0, 0);
            r[j] = make_uint4(v.x, v.y, v.z, v.w);
        }
    }
    template <int PX> __device__ __forceinline__ void store(const uint4 (&r)[XU], char* ring_row) const {
#pragma unroll
        for (int j = 0; j < XU; ++j) {
            const int u = tid + j * 256;
            *(uint4*)(ring_row + (u / PARTS) * PX + (u % PARTS) * 16) = r[j];
        }
    }
};

// ---- host: the launch geometry ------------------------------------------------------------------------------------------------
// balanced column strips of at most sw_max output columns
static inline void walker_strips(int Wo, int sw_max, int& nstrips, int& strip_w) {
    nstrips = (Wo + sw_max - 1) / sw_max;
    strip_w = (Wo + nstrips - 1) / nstrips;
}
// Rows per row slice: a slice costs `prologue_rows` row steps before its first output row (ring fill, extra mid / stem rows,
// weights) and the launch runs in rounds of `slots` resident blocks; among slices of >= 8 rows, the count with the least
// rounds x (rows per slice + prologue).  bx = blocks per slice (images x strips).
static inline int walker_row_slices(long long bx, int Ho, long long slots, double prologue_rows) {
    long long best_s = 1;
    double best_cost = 1e30;
    for (long long sl = 1; sl <= (Ho >= 16 ? Ho / 8 : 1); ++sl) {
        const long long rows = (Ho + sl - 1) / sl, nsl = (Ho + rows - 1) / rows;
        const double cost = (double)((bx * nsl + slots - 1) / slots) * ((double)rows + prologue_rows);
        if (cost < best_cost - 1e-9) { best_cost = cost; best_s = nsl; }
    }
    return (int)((Ho + best_s - 1) / best_s);
}

}  // namespace rw
