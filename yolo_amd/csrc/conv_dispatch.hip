// Convolution dispatch (host code only): from a yolo_conv_desc to one unit's conv_*_dispatch (conv_args.h) -- the ConvArgs fill and
// its validation, the id -> unit map, the automatic choice for algo == 0 and its fallback chain.
// Ids (yolo_conv_desc.algo); a tile is pixels x output channels, its shape is what the owning unit's case label instantiates:
//    0        automatic: conv_auto_candidates
//    1        conv_igemm.hip   the generic kernel: every shape and element type the library accepts
//    2-12     conv_pipe.hip    2 3 4 5 6 7 8 11: 3x3 stride 1 and (not 6 7) 1x1 tiles; 12: 1x1; 9 10: 3x3 stride 2;
//                              2 6 10 4 also name the 2x2-window tiles of yolo_conv_dgrad_s2
//    13 14    conv_stream.hip  weights-stationary streaming kernel, the small-channel layers (14: two pixel groups per wave)
//    16-18    conv_pipe.hip    3x3 stride 2: 10 / 9 / 10 with a smaller halo buffer and a 4-slot weight ring
//    19-25    conv_pipe.hip    1x1: deep rings (19 20 21), two K chunks per phase (22-25)
//    26-28    conv_pipe.hip    3x3 stride 1: one wave per SIMD (26), the pixel-heavy tiles (27 28)
//    30-33 35 conv_sk.hip      1x1 with the K range split over the waves of a block
//    36-39    conv_pipe.hip    1x1: 3-slot rings
//    40-42    conv_pipe.hip    split types only: 64-cout tiles, 1x1 / 3x3 stride 1 / 3x3 stride 2
//    43       conv_flat.hip    persistent 1x1 over the flat pixel index, dense 256 -> 128 / 512 -> 256
//    15 29 34 and 44 up: unassigned (YOLO_EUNSUPPORTED from the unit their range falls to)
#include "common.h"
#include "conv_args.h"
#include <stdlib.h>

// conv_epilogue.h form: 1 = unconditional buffer accesses (the default), 0 = the branching form (also what extents beyond 31 bits
// get).  Lab knob: YOLO_NO_BUF32 -> 0.
static int conv_buf32_form() {
    static const int v = YOLO_LAB_SET("YOLO_NO_BUF32") ? 0 : 1;
    return v;
}

// The kernel argument block of a forward convolution, value-initialised and then filled from the descriptor, with every check
// that goes with a member.  What a unit's launch adds (strips, tiles, divisors) stays zero here.  The tail_* / stats_* ARGUMENT
// checks are conv_check_tail_stats: yolo_conv_fwd runs them behind its algo-43 branch, as it always has.
static int conv_args_from_desc(const yolo_conv_desc* d, ConvArgs& a) {
    if (!d || !d->x || !d->w_packed || !d->y || (!d->scale != !d->bias)) return YOLO_EINVAL;      // (both NULL: identity epilogue)
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0) return YOLO_EINVAL;
    if (d->ksize != 1 && d->ksize != 3) return YOLO_EUNSUPPORTED;
    if (d->stride != 1 && d->stride != 2) return YOLO_EUNSUPPORTED;
    if (d->ksize == 1 && d->stride != 1) return YOLO_EUNSUPPORTED;
    if (!dtype_valid(d->dtype)) return YOLO_EINVAL;
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return YOLO_EINVAL;       // LeakyReLU is computed as max(t, t*slope)
    const int es = elem_size(d->dtype);
    const bool split = dtype_split(d->dtype);                         // (YOLO_BF16X3: common.h)
    const int planes = dtype_planes(d->dtype);
    if ((d->Cin * es) % 16) return YOLO_EUNSUPPORTED;                 // 16-byte K units
    if (!d->out_f32 && (d->Cout % 4)) return YOLO_EUNSUPPORTED;       // 4-channel store groups
    if (split && (d->stats || d->tail_w_packed || (!d->out_f32 && (d->Cout % 8)))) return YOLO_EUNSUPPORTED;
    // split tensors: each plane of a pixel is padded to whole 32-channel K-chunks (include/yolo_amd.h); the pad channels read zeros
    const int cin_p = split ? round_up(d->Cin, 32) : d->Cin, cout_p = (split && !d->out_f32) ? round_up(d->Cout, 32) : d->Cout;
    const int pad = d->ksize / 2;
    a = ConvArgs{};
    a.x = (const char*)d->x;
    a.wp = (const char*)d->w_packed;
    a.scale = d->scale;
    a.bias = d->bias;
    a.res = (const char*)d->residual;
    a.y = (char*)d->y;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
    a.Ho = (d->H + 2 * pad - d->ksize) / d->stride + 1;
    a.Wo = (d->W + 2 * pad - d->ksize) / d->stride + 1;
    a.Cout_pad = round_up(d->Cout, YOLO_COUT_PAD);
    a.nchunks = (cin_p * es + 63) / 64 * dtype_kpasses(d->dtype);
    a.out_f32 = d->out_f32;
    a.up2 = d->upsample2x ? 1 : 0;
    // (the bound is on BYTES: the kernels hold the pixel pitch x_ps * sizeof(T) as an int)
    if (d->x_pixel_stride < 0 || (d->x_pixel_stride && d->x_pixel_stride < (long long)cin_p * planes) || d->x_pixel_stride > 0x7fffffffLL / es) return YOLO_EINVAL;
    a.x_ps = d->x_pixel_stride ? (int)d->x_pixel_stride : cin_p * planes;
    if (split) {
        const long long xlo = d->x_lo_offset ? d->x_lo_offset : cin_p;
        const long long ylo = d->y_lo_offset ? d->y_lo_offset : cout_p;
        // (the kernels read whole chunks: cin_p channels from x + xlo, not Cin -- they must end inside the pixel.  Where a slice
        //  starts in its buffer the library cannot see: include/yolo_amd.h, x_lo_offset.  The plane offsets are 32-bit byte
        //  adjustments in the kernels)
        if (xlo < cin_p || xlo + cin_p > a.x_ps || (xlo * es) % 16 || xlo * es > 0x3fffffffLL) return YOLO_EINVAL;
        if (!d->out_f32 && (ylo < d->Cout || (ylo * es) % 16)) return YOLO_EINVAL;      // (fp32 logits are not split: y_lo unused)
        a.x3_n = cin_p * es / 64;
        a.x3_adj1 = (int)(xlo * es) - a.x3_n * 64;
        a.x3_adj2 = -a.x3_n * 64 - (int)(xlo * es);
        a.y_lo = ylo; a.r_lo = cout_p;
    }
    if ((a.x_ps * es) % 16) return YOLO_EUNSUPPORTED;                 // 16-byte aligned pixel rows
    a.slope = d->slope;
    const int oplanes = d->out_f32 ? 1 : planes;                          // (fp32 logits are not split)
    a.y_ps = d->y_pixel_stride ? d->y_pixel_stride : cout_p * oplanes;
    if (split && !d->out_f32 && a.y_lo + d->Cout > a.y_ps) return YOLO_EINVAL;
    a.y_bs = d->y_batch_stride ? d->y_batch_stride : (long long)a.Ho * a.Wo * a.y_ps * (a.up2 ? 4 : 1);
    a.r_ps = cout_p * planes; a.r_bs = (long long)a.Ho * a.Wo * a.r_ps;  // the residual is dense
    if (a.res && d->out_f32) return YOLO_EUNSUPPORTED;
    if (a.up2 && (a.res || d->out_f32)) return YOLO_EUNSUPPORTED;
    if (d->algo < 0) return YOLO_EINVAL;
    a.stats = (float*)d->stats; a.stats_mode = d->stats_mode;
    a.s_y = (const char*)d->stats_y; a.s_mean = d->stats_mean; a.s_invstd = d->stats_invstd;
    a.s_gamma = d->stats_gamma; a.s_beta = d->stats_beta; a.s_slope = d->stats_slope;
    a.t_wp = (const char*)d->tail_w_packed; a.t_scale = d->tail_scale; a.t_bias = d->tail_bias; a.t_y = (char*)d->tail_y;
    a.t_cout = d->tail_cout; a.t_out_f32 = d->tail_out_f32; a.t_slope = d->tail_slope;
    a.t_y_ps = d->tail_y_pixel_stride ? d->tail_y_pixel_stride : d->tail_cout;
    a.t_y_bs = d->tail_y_batch_stride ? d->tail_y_batch_stride : (long long)a.Ho * a.Wo * a.t_y_ps;
    // extents in bytes of everything the epilogue addresses (conv_epilogue.h buf32)
    const long long lim = 0x7fffffffLL;
    const long long yb = (long long)a.N * a.y_bs * (a.out_f32 ? 4 : es);
    const long long rbytes = a.res ? (long long)a.N * a.r_bs * es : 0;
    const long long tb = a.t_wp ? (long long)a.N * a.t_y_bs * (a.t_out_f32 ? 4 : es) : 0;
    a.buf32 = (yb < lim && rbytes < lim && tb < lim) ? conv_buf32_form() : 0;
    static const int lab = (int)YOLO_LAB_ENV("YOLO_EPI_AB", 0);
    a.lab = lab;
    return YOLO_OK;
}

// A fused tail 1x1 (pipelined 3x3 kernels of 2-byte elements only) and the BatchNorm statistics: their arguments.
static int conv_check_tail_stats(const yolo_conv_desc* d, const ConvArgs& a) {
    if (a.t_wp) {
        if (!d->tail_y || (!d->tail_scale != !d->tail_bias) || d->tail_cout <= 0 || !(d->tail_slope >= 0.f && d->tail_slope <= 1.f)) return YOLO_EINVAL;
        if (a.stats || elem_size(d->dtype) != 2 || d->ksize != 3) return YOLO_EUNSUPPORTED;
        if (!d->tail_out_f32 && (d->tail_cout % 4)) return YOLO_EUNSUPPORTED;
    } else if (a.stats) {
        if (a.stats_mode != 1 && a.stats_mode != 2) return YOLO_EINVAL;
        if (a.stats_mode == 2 && (!a.s_y || !a.s_mean || !a.s_invstd || !a.s_gamma || !a.s_beta)) return YOLO_EINVAL;
    }
    return YOLO_OK;
}

// id -> unit (the map at the top of the file).  A fused tail exists in conv_pipe.hip only, whatever the id; 43 is yolo_conv_fwd's
// own branch.
static int conv_run(ConvArgs& a, int ks, int stride, int dtype, int id, hipStream_t st, const NameOut* nm) {
    if (a.t_wp) return conv_pipe_dispatch(a, ks, stride, dtype, id, st, nm);
    if (id == 1) return conv_igemm_dispatch(a, ks, stride, dtype, st, nm);
    if (id == 13 || id == 14) return conv_stream_dispatch(a, ks, stride, dtype, id, st, nm);
    if (id >= 30 && id <= 35) return conv_sk_dispatch(a, ks, stride, dtype, id, st, nm);
    return conv_pipe_dispatch(a, ks, stride, dtype, id, st, nm);
}

// The fallback chain: the ids in order, each on a copy of the arguments; the first answer that is not YOLO_EUNSUPPORTED is it.
static int conv_try(const ConvArgs& a, int ks, int stride, int dtype, const int* ids, int n, hipStream_t st, const NameOut* nm) {
    for (int k = 0; k < n; ++k) {
        ConvArgs b = a;
        const int rc = conv_run(b, ks, stride, dtype, ids[k], st, nm);
        if (rc != YOLO_EUNSUPPORTED) return rc;
    }
    return YOLO_EUNSUPPORTED;
}

// The conv_pipe.hip tiles the two cost functions below choose among: bp pixels x bc output channels (what launch_pipe's template
// arguments of that id give: BP = WAVES_P * NI * 32, BC = WAVES_C * MI * 32), bpc resident blocks per compute unit, f the measured
// cost factor of the forward kernels (tools/conv_bench.py), and what takes the tile: the forward 3x3 stride 1, the forward 1x1,
// the 2x2 window of yolo_conv_dgrad_s2 (algo 4 there: large regular maps only, conv_pipe.hip).
//  (round 5: the pixel-heavy 3x3 tiles 27 / 28 -- ~40 % less L2 -> LDS weight stream per output, measured 0.5-3.4 % faster than
//   6 / 2 wherever they fill the chip, tools/ab_tiles.sh)
struct PipeTile { int id, bp, bc, bpc; float f; bool k3, k1, win; };
static const PipeTile kPipeTiles[] = {
    {2, 256, 256, 1, 1.00f, true, true, true},   {3, 256, 128, 1, 1.10f, true, true, false},  {4, 128, 128, 2, 1.05f, true, true, true},
    {6, 192, 256, 1, 1.00f, true, false, true},  {8, 192, 128, 2, 1.05f, true, true, false},  {10, 128, 256, 1, 0.f, false, false, true},
    {27, 384, 128, 1, 0.98f, true, false, false}, {28, 512, 128, 1, 0.97f, true, false, false}};

// Heuristic choice of the pipelined variant for algo == 0 (1 = stay on the generic kernel): minimise
// rounds x tile work, where rounds = ceil(tiles / (256 CUs x resident blocks per CU)) -- at the
// reference's batch sizes tile quantisation on the 13x13 / 26x26 maps costs more than any difference
// between the variants' inner loops.  Equal costs: the earlier row.
static int conv_auto_algo(const ConvArgs& a, int ks, int stride, int dtype, bool px_heavy = true) {
    if ((!dtype_split(dtype) && (a.Cin * elem_size(dtype)) % 64) || (ks == 1 && a.nchunks < 2)) return 1;      // (split planes are padded to whole chunks)
    if (dtype_split(dtype)) {
        // split types (round 6, measured at 416x416 bs 32, tools/layer_times.py --dtype bf16x3): the first stages' narrow layers are not
        // covered by fused / streaming kernels there -- the 64-cout tiles for them (1x1 64 -> 32 at 208^2: 129 us against 567 on a
        // 256-cout tile), the generic kernel for the large-map stride-2 layers (32 -> 64 at 416^2: 432 us against 602)
        if (ks == 1 && a.Cout <= 64) return 40;
        if (ks == 3 && stride == 1 && a.Cout <= 64) return 41;
        if (ks == 3 && stride == 2 && a.Cin <= 64) return 1;
    }
    if (stride == 2) return ks == 3 ? (a.Cout > 128 ? 18 : 9) : 1;      // (18 = 10 with the 4-slot weight ring)
    const long long px = (long long)a.N * a.Ho * a.Wo;
    int best = 1;
    double best_cost = 1e30;
    for (const PipeTile& v : kPipeTiles) {
        if (!(ks == 1 ? v.k1 : v.k3)) continue;
        if (!px_heavy && v.id >= 27) continue;
        const long long tiles = ((px + v.bp - 1) / v.bp) * ((a.Cout + v.bc - 1) / v.bc);
        const long long slots = 256LL * v.bpc;
        // full rounds keep every CU's bpc block slots busy (the co-resident blocks share the CU: bpc block times); the last,
        // partial round puts ceil(rest / 256) blocks on the busiest CU -- a launch of fewer tiles than CUs runs one block per CU
        // at full speed whatever bpc is (13^2 512 -> 1024 at batch 32: 232 tiles of the two-per-CU 192 x 128 tile beat 120 of
        // the 384 x 128 one, 50.7 against 64.2 us)
        const long long full = tiles / slots, rest = tiles - full * slots;
        const double cost = (double)(full * v.bpc + (rest + 255) / 256) * v.bp * v.bc * v.f;
        if (cost < best_cost) { best_cost = cost; best = v.id; }
    }
    return best;
}

// The ordered candidates of algo == 0 (13: the streaming kernel, 1: the generic one); the number written to ids (<= 5).
static int conv_auto_candidates(const ConvArgs& a, int ks, int stride, int dtype, int* ids) {
    int n = 0;
    if (a.t_wp) {
        // fused tail: tiles that hold every channel of a pixel -- 128-cout tiles first when Cout <= 128, then the 256-cout ones;
        // no other unit computes a tail
        static const int s1[] = {7, 6, 2}, s2[] = {17, 9, 18, 16, 10};
        const int total = stride == 2 ? 5 : 3, skip = a.Cout <= 128 ? 0 : (stride == 2 ? 2 : 1);
        for (int k = skip; k < total; ++k) ids[n++] = (stride == 2 ? s2 : s1)[k];
        return n;
    }
    // small-channel 3x3 layers: the streaming kernel (measured 1.2-1.45x the generic one; the 1x1s and the
    // 64->128 stride-2 layer are a wash and stay where they were)
    if (!dtype_split(dtype) && ks == 3 && a.Cin <= 64 && !(stride == 2 && a.Cin == 64)) ids[n++] = 13;
    const int pick = conv_auto_algo(a, ks, stride, dtype);
    if (pick >= 2) {
        ids[n++] = pick;
        // 18's halo buffer does not hold every strip shape: 10, the same tile with the larger buffer.  NOT with statistics: the
        // statistics path has never had this step (a stride-2 layer that 18 refuses computes its sums on the generic kernel), and
        // adding it changes which kernel the training forward runs.
        if (pick == 18 && !a.stats) ids[n++] = 10;
        if (pick >= 27) ids[n++] = conv_auto_algo(a, ks, stride, dtype, false);      // (the halo of a 384 / 512-pixel tile does not fit every map: the next best)
    }
    ids[n++] = 1;      // (with statistics: bf16 forward sums only, conv_igemm.hip launch_cfg)
    return n;
}

static int conv_fwd(const yolo_conv_desc* d, void* stream, const NameOut* nm) {
    ConvArgs a;
    int rc = conv_args_from_desc(d, a);
    if (rc != YOLO_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (d->algo == 43) return conv_flat_dispatch(a, d->ksize, d->stride, d->dtype, st, nm);      // (refuses a tail, statistics, strided views itself)
    if ((rc = conv_check_tail_stats(d, a)) != YOLO_OK) return rc;
    if (d->algo) return conv_run(a, d->ksize, d->stride, d->dtype, d->algo, st, nm);
    int ids[5];
    const int n = conv_auto_candidates(a, d->ksize, d->stride, d->dtype, ids);
    return conv_try(a, d->ksize, d->stride, d->dtype, ids, n, st, nm);
}

extern "C" int yolo_conv_fwd(const yolo_conv_desc* d, void* stream) { return conv_fwd(d, stream, nullptr); }

extern "C" int yolo_conv_kernel_name(const yolo_conv_desc* d, char* buf, int len) {
    if (!buf || len < 16) return YOLO_EINVAL;
    NameOut nm{buf, len, nullptr};
    return conv_fwd(d, nullptr, &nm);
}

// Number of partial rows ([rows][2][yolo_padded_channels(Cout)] float32) yolo_conv_fwd writes into d->stats for this
// descriptor, or YOLO_EUNSUPPORTED when the kernel it would run has no statistics epilogue.  Host-only, no launch
// (d->stats only has to be non-NULL).
extern "C" int yolo_conv_stats_rows(const yolo_conv_desc* d) {
    if (!d || !d->stats) return YOLO_EINVAL;
    char buf[256];
    int rows = -1;
    NameOut nm{buf, (int)sizeof(buf), &rows};
    const int rc = conv_fwd(d, nullptr, &nm);
    if (rc != YOLO_OK) return rc;
    return rows > 0 ? rows : YOLO_EUNSUPPORTED;
}

// Data gradient of a 3x3 stride-2 pad-1 convolution without the zero-dilated dy: the four sub-pixel phases of dx are
// four output-channel blocks of ONE 2x2-window convolution over dy (16 instead of 36 tap-products per dy pixel) whose
// epilogue stores depth-to-space.  Even H/W of dx only (2H x 2W); bf16; pipelined variants only -- callers fall back
// to yolo_dilate2x + yolo_conv_fwd on YOLO_EUNSUPPORTED.
extern "C" int yolo_conv_dgrad_s2(const yolo_conv_desc* d, void* stream) {
    if (!d || !d->x || !d->w_packed || !d->y || (!d->scale != !d->bias)) return YOLO_EINVAL;      // (both NULL: identity epilogue)
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->algo < 0) return YOLO_EINVAL;
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return YOLO_EINVAL;
    if (d->dtype != YOLO_BF16 || d->out_f32 || d->y_pixel_stride || d->y_batch_stride) return YOLO_EUNSUPPORTED;
    if ((d->Cout % 32) || (d->Cin * 2) % 64) return YOLO_EUNSUPPORTED;      // a lane's 8 couts stay inside one phase
    if (d->x_pixel_stride || d->upsample2x || d->stats) return YOLO_EUNSUPPORTED;
    // The shared fill sees the window as a dense stride-1 map (Ho = H, Wo = W, the same K chunks); ksize / stride / tail_* of the
    // descriptor are not read by this entry.  After the checks above it cannot refuse.
    yolo_conv_desc f = *d;
    f.ksize = 1; f.stride = 1; f.tail_w_packed = nullptr;
    ConvArgs a;
    const int rc = conv_args_from_desc(&f, a);
    if (rc != YOLO_OK) return rc;
    // dx is (N, 2Ho, 2Wo, Cout / 4), stored depth-to-space; a residual is dx itself (accumulation: same addressing)
    a.d2s = 1;
    a.y_ps = d->Cout / 4;
    a.y_bs = (long long)a.Ho * a.Wo * d->Cout;
    a.r_ps = a.y_ps; a.r_bs = a.y_bs;
    hipStream_t st = (hipStream_t)stream;
    if (d->algo) return conv_pipe_dispatch(a, 2, 1, d->dtype, d->algo, st, nullptr);
    // rounds x tile cost, then the first variant whose halo fits; equal costs: the larger tile
    const long long px = (long long)a.N * a.Ho * a.Wo;
    int ids[4], area[4], n = 0;
    double cost[4];
    for (const PipeTile& v : kPipeTiles) {
        if (!v.win) continue;
        const long long tiles = ((px + v.bp - 1) / v.bp) * ((a.Cout + v.bc - 1) / v.bc);
        const long long slots = 256LL * v.bpc;
        const double c = (double)((tiles + slots - 1) / slots) * v.bp * v.bc * v.bpc;
        int k = n++;      // (insertion sort)
        for (; k > 0 && (c < cost[k - 1] || (c == cost[k - 1] && v.bp * v.bc > area[k - 1])); --k) { cost[k] = cost[k - 1]; area[k] = area[k - 1]; ids[k] = ids[k - 1]; }
        cost[k] = c; area[k] = v.bp * v.bc; ids[k] = v.id;
    }
    return conv_try(a, 2, 1, d->dtype, ids, n, st, nullptr);
}
