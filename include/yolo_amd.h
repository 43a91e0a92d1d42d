/* yolo_amd.h -- C ABI of libyolo_amd.so: the MI355X (gfx950) YOLOv3 hot path.
 *
 * The reference (n8886919/YOLO) has no FFI/plugin interface: its seam is the Python object
 * protocol between the task drivers and MXNet operators.  Each entry
 * point below names the reference call site / MXNet operator it replaces.  All pointers are
 * DEVICE pointers unless a name ends in _host.  The caller owns every buffer; the library
 * allocates no persistent device memory.  Every function is asynchronous on `stream`
 * (a hipStream_t passed as void*), returns 0 on success, <0 on invalid argument /
 * unsupported shape, >0 = hipError_t from the launch.  Nothing throws across the ABI.
 *
 * Layout: activations are NHWC ("pixel-major, channel-contiguous") in HBM, dtype
 * YOLO_F32, YOLO_BF16, YOLO_F16 or a split type (YOLO_BF16X3 / YOLO_F16X3: two planes per pixel, below); images enter as NCHW float32 exactly as the reference feeds them
 * (car/YOLO.py:381, yolo_gluon.py:354) and head logits leave as (B, sum HW, A, C) float32
 * exactly as CarNet returns them (car/utils.py:95, basic_yolo.py:102-103).
 */
#ifndef YOLO_AMD_H
#define YOLO_AMD_H
#ifdef __cplusplus
extern "C" {
#endif

#define YOLO_F32 0
#define YOLO_BF16 1
#define YOLO_F16 2     /* IEEE half: the reference's own reduced precision (use_fp16 -> net.cast('float16'), car/YOLO.py:98-100; executor fp16 flag
                          yolo_gluon.py:204-214).  Inference entry points only (pack, fold, nchw<->nhwc, conv_fwd, stem, res_block); the
                          training entries take YOLO_F32 | YOLO_BF16 (and YOLO_BF16X3, below) */

/* SPLIT bf16 ("bf16x3", round 6): the path on which the north-star tolerance (decoded boxes within 1e-3 of the fp32 reference) and the
 * bf16 MFMA rate meet.  A value v is stored as TWO bf16 numbers, hi = bf16(v) and lo = bf16(v - hi) (16 significant bits), and every
 * product w * x of a convolution is taken as w_hi x_hi + w_hi x_lo + w_lo x_hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
 * (three MFMAs per product; the exact-fp32 MFMA of YOLO_F32 is sixteen times slower than one).  Storage of an (N,H,W,C) activation:
 * per pixel a hi PLANE of Cp = round_up(C, 32) values (C real, the rest zero: whole 32-channel K-chunks), then -- `lo offset`
 * elements further (dense: Cp) -- the lo plane: dense pixel stride 2 * Cp elements of 2 bytes.  The kernels never write the pad
 * channels and read them as operands of zero weights: THE CALLER ZEROES A BUFFER WITH C % 32 != 0 ONCE (a NaN there would poison the
 * sums).  Entry points that take it: yolo_packed_weight_bytes / yolo_pack_conv_weights (image [w_hi | w_hi | w_lo] over
 * 3 * Cp / 32 K-chunks; Cin % 8 == 0), yolo_conv_fwd (pipelined kernels; Cout % 8 == 0 unless out_f32; no stats / tail),
 * yolo_stem_conv_fwd, and -- the split training step (revision 5) -- yolo_pack_conv_weights_dgrad (dgrad image as three K passes
 * [w'_hi | w'_hi | w'_lo]), yolo_bn_train_fwd / _bwd / _fwd_pp / _bwd_pp, yolo_nchw_to_nhwc, yolo_upsample2x_concat (+ _bwd),
 * yolo_dilate2x, yolo_gather_rows, yolo_bias_grad, yolo_add_split and yolo_conv_wgrad_split.  Their split tensors are dense
 * (C logical channels, planes of round_up(C, 32)); values are read as hi + lo in fp32 and stored as hi = bf16_rne(v),
 * lo = bf16_rne(v - hi).  Everything else returns YOLO_EUNSUPPORTED / YOLO_EINVAL for it (the _partials entries,
 * yolo_conv_dgrad_s2, yolo_pack_batch_blocks, yolo_conv_wgrad / _algo and yolo_add among them). */
#define YOLO_BF16X3 3
/* The same scheme on IEEE-half pairs: decoded boxes indistinguishable from the fp32 path's (6e-5 on the D53 random-BN nets, where
 * YOLO_BF16X3 measures 3e-4) at the same three MFMAs per product.  Precision: 22 significant bits (the dropped term 2^-22 of a
 * product) ONLY while the lo plane is normal or near it -- lo lives in half's subnormals, whose spacing is 2^-24 (which
 * v_mfma_f32_32x32x16_f16 honours: tools/probes/f16_denorm_probe.py), so below |v| ~ 2^-3 a stored value has an ABSOLUTE error floor
 * of 2^-25 instead: 11 bits are left at |v| = 2^-14, where hi turns subnormal too (measured against float64 on a 64 -> 64 3x3:
 * 4.6e-7 relative on O(1) operands, 2.3e-5 with x * 2^-10, 3.8e-4 with x * 2^-14; YOLO_BF16X3: 7.0e-6 at every scale).  Range:
 * |v| <= 65504; beyond it hi is Inf and lo = v - hi is Inf or NaN, and an Inf even in a channel that only meets zero weights turns the
 * sums into NaN.  Nothing checks either limit.  Same entry points, layout and restrictions as YOLO_BF16X3. */
#define YOLO_F16X3 4

#define YOLO_OK 0
#define YOLO_EINVAL (-1)
#define YOLO_EUNSUPPORTED (-2)

/* ABI revision = the layout of every struct and the argument list of every entry below.  A caller compiled against another
 * revision must not call anything else: the library reads the WHOLE yolo_conv_desc on every call (revision 2 appended the
 * tail_* fields, revision 3 added YOLO_F16, revision 4 YOLO_BF16X3 and the *_lo_offset fields, revision 5 the split training entries), so a shorter struct from an older header would be read past its end.
 * yolo_amd/lib.py:load() refuses a library whose yolo_version() differs from the YOLO_ABI_VERSION it was written against. */
#define YOLO_ABI_VERSION 5
int yolo_version(void);

/* ---- parameter preparation ------------------------------------------------------------- */

/* Bytes of the packed weight image for a conv (Cout, Cin, ksize) in `dtype`. */
long long yolo_packed_weight_bytes(int Cout, int Cin, int ksize, int dtype);

/* OIHW float32 weights (gluon Conv2D layout, basic_yolo.py:20-26,98) -> the K-chunked,
 * LDS-swizzled image the implicit-GEMM kernel streams: [chunk][tap][Cout_pad][64 B]. */
int yolo_pack_conv_weights(const float* w_oihw, void* packed, int Cout, int Cin, int ksize,
                           int dtype, void* stream);

/* Inference-mode BatchNorm folding (gluon BatchNorm eps=1e-5):
 * scale = gamma/sqrt(var+eps), bias = beta - mean*scale, both padded with zeros to
 * yolo_padded_channels(C) floats.  gamma==NULL: scale=1, bias=beta (plain conv bias,
 * YOLOOutput basic_yolo.py:98; beta may be NULL -> 0). */
int yolo_padded_channels(int C);
int yolo_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var,
                 float eps, float* scale, float* bias, int C, void* stream);

/* ---- image plumbing -------------------------------------------------------------------- */

/* (N,C,H,W) float32 -> (N,H,W,Cpad) dtype, channels C..Cpad-1 zero.  Replaces the implicit
 * layout the reference hands to its first Convolution (car/YOLO.py:381). */
int yolo_nchw_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int Cpad, int dtype,
                      void* stream);
/* (N,H,W,C) uint8 -> (N,C,H,W) float32 / 255: cv_img_2_ndarray, yolo_gluon.py:335-357. */
int yolo_image_u8_to_nchw(const unsigned char* img, float* y, int N, int H, int W, int C,
                          void* stream);
/* Frame intake: inverse-mapped bilinear sampling of uint8 frames into the net's input.  Clip + flip + resize
 * (yolo_cv.py:285-318 cv2_flip_and_clip_frame, cv2.resize, yolo_gluon.py:335-357 cv_img_2_ndarray) are one affine M; the plate
 * rectification of ProjectRectangle6D.add_edges (licence_plate_render/__init__.py:379-402) is one homography.
 * frames (N,Hs,Ws,C) u8 dense, y (N,C,Ho,Wo) f32 dense, M (N,9) f32 ON THE DEVICE, row-major 3x3 mapping an OUTPUT pixel
 * (column j, row i) to SOURCE pixel coordinates (integer = pixel centre, cv2's WARP_INVERSE_MAP convention);
 * border 0 = taps outside roi read 0 (cv2.warpPerspective's default), 1 = tap indices clamped into roi (cv2.resize on a crop);
 * roi = {x0, y0, x1, y1} inclusive, host ints, shared by the batch; gain: C floats on the device or NULL (= 1).
 * The arithmetic, every operation in fp32, in this order, nothing fused (this is the definition; tests/intake_ref.py restates it):
 *   u = (m0*j + m1*i) + m2;  v = (m3*j + m4*i) + m5;  w = (m6*j + m7*i) + m8;     sx = u / w;  sy = v / w
 *   x0 = floor(sx), fx = sx - x0;  y0 = floor(sy), fy = sy - y0
 *   taps a = (y0, x0), b = (y0, x0+1), c = (y0+1, x0), d = (y0+1, x0+1), each converted to float
 *   top = a + fx*(b - a);  bot = c + fx*(d - c);  val = top + fy*(bot - top);     y = (val / 255.f) * gain[ch]
 * Channel order is untouched.  x0 / y0 are limited to +-2^30 before they become integers; a coordinate that is not a number
 * (w = 0) indexes outside and gives NaN through fx / fy.  No load leaves the roi whatever M holds.
 * YOLO_EINVAL: a NULL frames / y / M, a non-positive size, a roi that is empty or not inside the frame.  YOLO_EUNSUPPORTED:
 * C > 4, a border not in {0, 1} (and Ho * ceil(Wo / 4) or Ws * C beyond 2^31).  16-byte plane stores when Wo % 4 == 0 and y is
 * 16-byte aligned, scalar stores otherwise. */
int yolo_warp_u8_to_nchw(const unsigned char* frames, float* y, const float* M, const float* gain, int N, int Hs, int Ws, int C,
                         int Ho, int Wo, int border, int roi_x0, int roi_y0, int roi_x1, int roi_y1, void* stream);
/* NHWC dtype -> NCHW float32 (debug / parity taps). */
int yolo_nhwc_to_nchw(const void* x, float* y, int N, int C, int H, int W, int dtype, void* stream);

/* ---- convolution ----------------------------------------------------------------------- */

/* Fused Conv(k in {1,3}, stride in {1,2}, pad k/2, no bias) + folded BN + LeakyReLU(slope)
 * [+ residual add after the activation].  Replaces gluoncv _conv2d (Convolution + BatchNorm
 * + LeakyReLU, call sites basic_yolo.py:20,24,26,118,121), DarknetBasicBlockV3's elementwise
 * add, and YOLOOutput's Conv2D+bias+transpose+reshape (basic_yolo.py:98-103) when out_f32=1. */
typedef struct yolo_conv_desc {
    const void* x;         /* (N,H,W,Cin) dtype                                               */
    const void* w_packed;  /* yolo_pack_conv_weights image                                    */
    const float* scale;    /* [padded Cout] folded BN scale                                   */
    const float* bias;     /* [padded Cout] folded BN bias / conv bias; scale and bias both NULL =
                              identity epilogue: y = conv(x) (+ residual), slope ignored       */
    const void* residual;  /* (N,Ho,Wo,Cout) dtype or NULL; added after the activation        */
    void* y;               /* (N,Ho,Wo,Cout) dtype, or float32 when out_f32                   */
    int N, H, W, Cin, Cout;
    int ksize, stride;
    int dtype;             /* YOLO_F32 | YOLO_BF16 | YOLO_F16 | YOLO_BF16X3 | YOLO_F16X3: activations and weights */
    int out_f32;           /* 1: y is float32 (head logits)                                   */
    float slope;           /* LeakyReLU negative slope in [0, 1]; 1.0f = linear               */
    long long y_batch_stride; /* elements between images in y; 0 = dense Ho*Wo*Cout           */
    long long y_pixel_stride; /* elements between pixels in y; 0 = dense Cout                 */
    int algo;              /* 0 = library heuristic; 1 = generic kernel; >= 2 = a specific pipelined
                              tile variant (csrc/conv_pipe.hip; 13 / 14: csrc/conv_stream.hip, 30-35: csrc/conv_sk.hip,
                              43: csrc/conv_flat.hip), YOLO_EUNSUPPORTED if not eligible              */
    long long x_pixel_stride; /* elements between pixels in x; 0 = dense Cin.  > Cin: x is a channel slice of a wider
                              NHWC buffer (the route half of a concat buffer, car/utils.py:93); images stay
                              H*W*x_pixel_stride apart.  Split types: see x_lo_offset for what a slice with
                              Cin % 32 != 0 needs behind it.  The pitch in BYTES must stay below 2^31
                              (YOLO_EINVAL); pinned tile variants also refuse an x of 0xffffff00 bytes or more
                              (YOLO_EUNSUPPORTED; algo 0 runs the generic kernel then)        */
    int upsample2x;        /* 1: every output pixel is stored to the 2x2 patch (2oy..2oy+1, 2ox..2ox+1) of a
                              (N,2Ho,2Wo,*) map -- gluoncv _upsample(x, stride=2) (car/utils.py:92) fused into the
                              producing convolution; strides then refer to that map (y_batch_stride 0 =
                              4*Ho*Wo*y_pixel_stride); no residual, no out_f32                */
    /* Training step: Gluon BatchNorm's batch statistics taken in the convolution's epilogue instead of
     * in a pass of their own over the tensor.  stats != NULL: the kernel also writes yolo_conv_stats_rows() partial rows
     * [row][2][yolo_padded_channels(Cout)] float32 of per-channel sums over its pixel tiles (no atomics), which
     * yolo_bn_train_fwd_partials / yolo_bn_train_bwd_partials reduce in double.  stats_mode 1: sum(y), sum(y^2) of the
     * output y (the BatchNorm that follows this convolution in the forward pass).  stats_mode 2 (a data gradient,
     * y = d(loss)/d(z) of the layer BEHIND it): sum(da), sum(da * xhat) with da = y * lrelu'(gamma*xhat + beta),
     * xhat = (stats_y - mean) * invstd, stats_y = that layer's raw convolution output (same shape as y, dense).
     * bf16, pipelined kernels only (YOLO_EUNSUPPORTED otherwise: run the separate reduction). */
    void* stats;
    int stats_mode;
    const void* stats_y;
    const float* stats_mean;
    const float* stats_invstd;
    const float* stats_gamma;
    const float* stats_beta;
    float stats_slope;
    /* A 1x1 convolution fused BEHIND this one (the "tail"): tail_y = act(conv1x1(y)) -- the next DarknetBasicBlockV3's first
     * _conv2d (basic_yolo.py:26), a YOLODetectionBlockV3's 1x1 after its 3x3 (basic_yolo.py:118), or YOLOOutput after the tip
     * (basic_yolo.py:98-105, tail_out_f32 = 1) -- computed by the same kernel from the output tile it has just stored: no second
     * launch, no HBM read of y; y is still written.  tail_w_packed: yolo_pack_conv_weights image of the (tail_cout, Cout, 1, 1)
     * weights; tail_scale / tail_bias padded like scale / bias; tail_y (N,Ho,Wo,tail_cout) dtype or float32; strides as for y.
     * Bit-identical to the separate 1x1 launch.  Needs: bf16, ksize 3, Cout <= 256 and a multiple of 32, tail_cout <= 128, no
     * out_f32 / upsample2x / stats on this convolution, and an 8-wave pipelined variant whose tile holds every channel of a pixel
     * (256-cout tiles: algo 2, 6; stride 2: 10, 16, 18; Cout <= 128 also the 128-cout tiles 7; 9, 17; algo 0 picks one) -- YOLO_EUNSUPPORTED otherwise (run the two launches). */
    const void* tail_w_packed;
    const float* tail_scale;
    const float* tail_bias;
    void* tail_y;
    int tail_cout;
    int tail_out_f32;
    float tail_slope;
    long long tail_y_batch_stride;
    long long tail_y_pixel_stride;
    /* split types only (YOLO_BF16X3 / YOLO_F16X3; ignored otherwise): elements between a pixel's hi plane and its lo plane in x and in y; 0 = dense
     * (round_up(Cin, 32), round_up(Cout, 32)).  A channel slice of a wider split buffer of Ctot channels (the halves of a concat
     * buffer, car/utils.py:93) has pixel stride 2 * Ctot and lo offset Ctot.  Dense strides of a split tensor count both padded
     * planes (pixel stride 2 * round_up(C, 32)); the residual is dense; y_lo_offset is not used when out_f32.
     * THE KERNELS READ x IN WHOLE 32-CHANNEL K-CHUNKS, whatever Cin is: round_up(Cin, 32) channels from x and round_up(Cin, 32)
     * from x + x_lo_offset.  Both runs must lie inside the pixel (inside [pixel start, pixel start + x_pixel_stride) of the buffer
     * x was sliced from), and whatever they hold beyond the first Cin channels must be FINITE: it meets zero weights, and an Inf or
     * NaN there turns the sums into NaN.  YOLO_EINVAL when x_lo_offset + round_up(Cin, 32) > x_pixel_stride; the library cannot
     * see where in its buffer a slice starts, so for channels [c0, c0 + Cin) of a buffer with planes of Cp channels the caller
     * provides Cp >= c0 + round_up(Cin, 32) (zeroed pad channels count).  Stores have no such reach: exactly channels
     * [0, Cout) of both planes of y are written. */
    long long x_lo_offset;
    long long y_lo_offset;
} yolo_conv_desc;

int yolo_conv_fwd(const yolo_conv_desc* d, void* stream);
/* Partial rows yolo_conv_fwd would write into d->stats (> 0), or YOLO_EUNSUPPORTED if the kernel it would launch for `d`
 * has no statistics epilogue.  Host-only, no launch; d->stats only has to be non-NULL. */
int yolo_conv_stats_rows(const yolo_conv_desc* d);
/* Name of the kernel instantiation yolo_conv_fwd would launch for `d` (as rocprofv3 prints it);
 * used by bench.py to attribute measured time to the dominant kernel.  Host-only, no launch. */
int yolo_conv_kernel_name(const yolo_conv_desc* d, char* buf, int len);
/* algo 43 (csrc/conv_flat.hip): the persistent 1x1 over the flat pixel index -- YOLO_BF16 / YOLO_F16, Cin -> Cout in
 * {256 -> 128, 512 -> 256}, dense x, y and residual, no out_f32 / upsample2x / stats / tail (YOLO_EUNSUPPORTED otherwise);
 * bit-identical to the tiled 1x1 variants.  Its tile size in pixels and the resident blocks per compute unit its grid is
 * sized with: grid = min(ceil(N*H*W / tile_px), compute units * blocks_per_cu).  Host-only, no launch. */
int yolo_conv_flat_geometry(int Cin, int Cout, int* tile_px, int* blocks_per_cu);

/* The network's first _conv2d (basic_yolo.py:20) fused with the image layout change: Conv3x3 s1 p1 over
 * the (N,3,H,W) float32 NCHW image exactly as the reference feeds it (car/YOLO.py:381) + folded BN +
 * LeakyReLU -> (N,H,W,Cout) bf16 NHWC.  w_oihw: (Cout,3,3,3) float32 (unpacked); Cout % 4 == 0, <= 64;
 * dtype YOLO_BF16 / YOLO_F16 (YOLO_F32 callers use yolo_nchw_to_nhwc + yolo_conv_fwd: EUNSUPPORTED here), or YOLO_BF16X3 / YOLO_F16X3: a direct
 * fp32 convolution on the vector pipe (K = 27: nothing for the matrix pipe to win) whose output is stored split, dense
 * (N,H,W,[hi Cout | lo Cout]); Cout % 8 == 0 there. */
int yolo_stem_conv_fwd(const float* x_nchw, const float* w_oihw, const float* scale, const float* bias,
                       void* y, int N, int H, int W, int Cin, int Cout, int dtype, float slope,
                       void* stream);

/* The same with BatchNorm's batch sums of the stored output taken in the kernel (training step; see yolo_conv_desc.stats):
 * partials = yolo_stem_stats_rows() rows of [2][Cout] float32 (pass cout_pad = Cout to yolo_bn_train_fwd_partials).
 * Cout % 8 == 0 and 64 % (Cout / 8) == 0 (YOLO_EUNSUPPORTED otherwise). */
int yolo_stem_stats_rows(int N, int H, int W, int Cout);
int yolo_stem_conv_fwd_stats(const float* x_nchw, const float* w_oihw, const float* scale, const float* bias,
                             void* y, int N, int H, int W, int Cin, int Cout, int dtype, float slope,
                             float* partials, void* stream);

/* One DarknetBasicBlockV3 (basic_yolo.py:26; gluoncv darknet.py: x + conv3x3(C)(conv1x1(C/2)(x)), each conv with
 * folded BN + LeakyReLU, no activation after the add) as ONE inference kernel for the first stages: x, y (N,H,W,C)
 * bf16 NHWC; w1_packed / w2_packed = yolo_pack_conv_weights images of the (C/2,C,1,1) and (C,C/2,3,3) convs; scale /
 * bias = yolo_fold_bn of each layer.  The C/2-channel map between the two convs stays in LDS and x is read once.  Same
 * rounding points as yolo_conv_fwd run twice (mid rounded to bf16 once; residual added in fp32 before the output's
 * one rounding).  YOLO_BF16 and C in {64, 128} only (YOLO_EUNSUPPORTED otherwise: run the two layers separately). */
int yolo_res_block_fwd(const void* x, const void* w1_packed, const float* scale1, const float* bias1,
                       const void* w2_packed, const float* scale2, const float* bias2, void* y, int N, int H, int W,
                       int C, int dtype, float slope, void* stream);

/* The first TWO layers fused for inference: the stem above and the first stage's down-sampling _conv2d (basic_yolo.py:24,
 * Conv3x3 s2 p1, C1 -> C2) + folded BN + LeakyReLU -> y (N,(H-1)/2+1,(W-1)/2+1,C2) bf16 NHWC; the full-resolution
 * C1-channel map between them stays in LDS.  w1_oihw (C1,3,3,3) float32; w2_packed = yolo_pack_conv_weights image of
 * the (C2,C1,3,3) conv.  Bit-identical to yolo_stem_conv_fwd followed by yolo_conv_fwd.  C1 == 32, C2 == 64 and
 * YOLO_BF16 only (YOLO_EUNSUPPORTED otherwise: run the two layers separately). */
int yolo_stem_down_fwd(const float* x_nchw, const float* w1_oihw, const float* scale1, const float* bias1,
                       const void* w2_packed, const float* scale2, const float* bias2, void* y, int N, int H, int W,
                       int C1, int C2, int dtype, float slope, void* stream);

/* The first FOUR convolutions fused for inference: yolo_stem_down_fwd followed by yolo_res_block_fwd at C = 64 as ONE kernel
 * (csrc/stem_res.hip), (N,3,H,W) float32 NCHW image -> y (N,H/2,W/2,C2) NHWC, the output of the first stage's residual block; the
 * C2-channel map between the down-sampling conv and the block stays in LDS.  w0_oihw (C1,3,3,3) float32; wd / w1 / w2_packed =
 * yolo_pack_conv_weights images of the (C2,C1,3,3), (C2/2,C2,1,1) and (C2,C2/2,3,3) convs; scale / bias = yolo_fold_bn of each
 * layer.  Bit-identical to the two calls it replaces.  C1 == 32, C2 == 64, YOLO_BF16 / YOLO_F16, even H and W only
 * (YOLO_EUNSUPPORTED otherwise, nothing is launched: run the two kernels). */
int yolo_stem_res_fwd(const float* x_nchw, const float* w0_oihw, const float* scale0, const float* bias0,
                      const void* wd_packed, const float* scaled, const float* biasd, const void* w1_packed,
                      const float* scale1, const float* bias1, const void* w2_packed, const float* scale2,
                      const float* bias2, void* y, int N, int H, int W, int C1, int C2, int dtype, float slope, void* stream);
/* Its launch geometry for an image shape on the current device (host only): column strips per image, their width in output
 * columns, output rows per row slice, row slices; the grid is (N * nstrips, slices), sized to one block per compute unit. */
int yolo_stem_res_geometry(int N, int H, int W, int* nstrips, int* strip_w, int* rows_per_slice, int* slices);

/* Synthetic-target compositing of RenderCar.render (car/render_car.py:135-137): out = clip((bg / 255) * (1 - mask) +
 * fg * mask, 0, 1) over n float32 elements (n % 4 == 0; (B,3,H,W) tensors: bg 0..255, fg and mask 0..1). */
int yolo_composite(const float* bg, const float* fg, const float* mask, float* out, long long n, void* stream);
/* The blend of LPGenerator.add (yolo_modules/licence_plate_render/__init__.py:163-164), which pastes the projected plate
 * onto images that are ALREADY 0..1: out = clip(bg * (1 - mask) + fg * mask, 0, 1). */
int yolo_composite_unit(const float* bg, const float* fg, const float* mask, float* out, long long n, void* stream);

/* RenderCar.render (car/render_car.py:52-138) with the PIXELS made on the device: the host decides (sprite, scale, angle, blur,
 * offset, colour: yolo_amd/render.py draw_params) and hands over one row of YOLO_RENDER_ROW_WORDS 32-bit words per image:
 *   0 has-sprite (int)     1 h  2 w: the mip level's size (int)      3..6 window l, t, r, b (int; r, b exclusive)     7 unused
 *   8,9 the level's byte offset in the atlas (one 64-bit int)        10..15 a0..a5 (float)     16 w0  17 w1 (float)
 *   18..26 A  27..35 D (3x3 row-major, float)   36..38 e (float)     39 unused
 * atlas: uint8 RGBA levels packed as (h, w, 4), atlas_bytes in all, 4-byte aligned; rows ON THE DEVICE, 8-byte aligned;
 * bg (N,3,H,W) f32 0..255, out (N,3,H,W) f32 0..1, dense.  The arithmetic, every operation in fp32, in this order, nothing fused
 * (this is the definition; tests/render_ref.py restates it):
 *  the sample S(x, y) at output position (column x, row y), four channels RGBA interpolated independently:
 *   sx = (a0*x + a1*y) + a2;  sy = (a3*x + a4*y) + a5;   x0 = floor(sx), fx = sx - x0;  y0 = floor(sy), fy = sy - y0
 *   taps a = (y0, x0), b = (y0, x0+1), c = (y0+1, x0), d = (y0+1, x0+1): a tap inside the level reads its byte as a float, one
 *   outside reads 0;   top = a + fx*(b - a);  bot = c + fx*(d - c);  S = top + fy*(bot - top)
 *  the value at output pixel (j, i):  w1 == 0:  P = S(j, i);   otherwise, with R(dy) = (w1*S(j-1, i+dy) + w0*S(j, i+dy)) + w1*S(j+1, i+dy),
 *   P = (w1*R(-1) + w0*R(0)) + w1*R(1)       (a 3x3 separable blur; NOT PIL's box-blur GaussianBlur)
 *  yolo_render_stats: per image and channel c of R, G, B the sum of P_c over the window's pixels, each converted to double and added
 *   in double, as RENDER_STAT_BLOCKS = 16 partial sums (workspace: yolo_render_workspace_bytes(N, H, W) bytes, 8-byte aligned,
 *   caller-owned); no atomics, so the sums do not depend on scheduling.
 *  yolo_render_cars: sum_c = the image's partials added in index order (double);  mu_c = (float)(sum_c / (double)(H*W));
 *   k_c = ((D[c][0]*mu_0 + D[c][1]*mu_1) + D[c][2]*mu_2) + e_c;      per pixel of the window:
 *   fg_c = (((A[c][0]*P_0 + A[c][1]*P_1) + A[c][2]*P_2) + k_c) / 255.f;   mask = P_3 / 255.f
 *   out_c = min(max((bg_c / 255.f) * (1.f - mask) + fg_c * mask, 0), 1)          (yolo_composite's operation order)
 *  A pixel outside the window, and every pixel of an image without a sprite: out_c = min(max(bg_c / 255.f, 0), 1), the atlas is
 *  not touched.  x0 / y0 are limited to +-2^30 before they become integers.  No load leaves the atlas whatever a row holds: a row
 *  whose level (offset not a multiple of 4, or offset + 4 h w beyond atlas_bytes, or h, w <= 0) does not lie inside the atlas is
 *  "no sprite", the window is clipped to the canvas, tap addresses are clamped into the level.
 * YOLO_EINVAL: a NULL pointer, a non-positive N, H, W or atlas_bytes, a misaligned atlas / rows / workspace.  YOLO_EUNSUPPORTED:
 * H * ceil(W / 4) beyond 2^31.  yolo_render_workspace_bytes returns YOLO_EINVAL for a non-positive size.
 * 16-byte bg loads and plane stores when W % 4 == 0 and bg, out are 16-byte aligned, scalar ones otherwise.
 * yolo_render_cars must follow yolo_render_stats on the same rows, in stream order. */
#define YOLO_RENDER_ROW_WORDS 40
long long yolo_render_workspace_bytes(int N, int H, int W);
int yolo_render_stats(const unsigned char* atlas, long long atlas_bytes, const void* rows, void* workspace, int N, int H, int W,
                      void* stream);
int yolo_render_cars(const float* bg, const unsigned char* atlas, long long atlas_bytes, const void* rows, const void* workspace,
                     float* out, int N, int H, int W, void* stream);

/* LPGenerator.add (yolo_modules/licence_plate_render/__init__.py:58-166) with the PIXELS made on the device, the plate counterpart
 * of yolo_render_cars: the host decides (glyphs, 6-D pose, blur, noise key, colour: yolo_amd/render.py LPGenerator.draw_params) and
 * hands over one row of YOLO_PLATE_ROW_WORDS 32-bit words per image:
 *   0 has-plate (int)      1..7 glyph ids (int; 3 letters 10..33, then 4 digits 0..9)      8..11 window l, t, r, b (int; r, b exclusive)
 *   12,13 noise key k0, k1 (uint32)     14 noise scale s (float; 0 = no noise)     15 unused
 *   16..24 m0..m8 (float): output pixel INDEX -> plate texel INDEX, projective     25 w0  26 w1 (float)
 *   27..35 A  36..44 D (3x3 row-major, float)   45..47 e (float)
 * glyphs: the resident uint8 RGBA atlas in a fixed layout, YOLO_PLATE_GLYPH_BYTES in all, 4-byte aligned: the 34 glyphs as (90,45,4)
 * in id order 0..33, then the dot as (70,10,4) -- the images LPGenerator holds after its PIL resize.  rows ON THE DEVICE, 8-byte
 * aligned; plates (N,160,380,4) uint8, caller-owned, 4-byte aligned; bg (N,3,H,W) f32 ALREADY 0..1, out the same shape, dense.
 *  yolo_plate_compose: every texel of an image's plate starts as (255,255,255,255); a glyph cell overwrites all four bytes (PIL's
 *   mask-less paste): glyph k of 7 at column (7, 56, 106, 175, 225, 274, 324)[k], row 35, 45 wide, 90 high; the dot at column 158,
 *   row 45, 10 wide, 70 high (the cells do not overlap).  A row with has == 0 or any glyph id outside 0..33 is "no plate": its
 *   plate is NOT written, and the two other entries treat the image as background only.  No load leaves the atlas whatever a row holds.
 * The arithmetic of the pixels, every operation in fp32, in this order, nothing fused, division correctly rounded (this is the
 * definition; tests/plate_ref.py restates it).  For output position (column x, row y):
 *   nx = (m0*x + m1*y) + m2;  ny = (m3*x + m4*y) + m5;  den = (m6*x + m7*y) + m8
 *   !(den > 0) or den not finite:  S = 0 (transparent);   otherwise sx = nx / den, sy = ny / den and S is yolo_render_cars' bilinear
 *   tap over the image's plate at (sx, sy): x0 = floor(sx), fx = sx - x0, ..., taps outside read 0, indices limited to +-2^30,
 *   addresses clamped into the plate.
 *  P(j, i): inside the window S(j, i), or for w1 != 0 the 3x3 separable sum in yolo_render_cars' order; outside the window P = 0 and
 *   nothing is sampled.
 *  Q(j, i), four channels, for EVERY canvas pixel:  s == 0: Q = P.  Otherwise two Philox4x32-10 calls with key (k0, k1), call h of
 *   0, 1 with counter (j, i, h, 0); call 0 gives words 0,1 for R and 2,3 for G, call 1 gives B and A the same way; per channel
 *   t = the sum of the 8 bytes of its two words, z = (float)(t - 1020), Q_c = min(max(P_c + z*s, 0), 255).  Integer-only on
 *   purpose: an 8-term Irwin-Hall sum, exactly reproducible (Box-Muller's logf / cosf would not be); the host sets
 *   s = float32(sigma / sqrt(8 * 65535 / 12)), which gives z*s the standard deviation sigma.
 *   The noise falls on ALL FOUR channels of the WHOLE canvas, as the reference's np.clip(px + normal(0, 5)) on the RGBA array does
 *   (alpha outside the plate becomes a faint haze).  Nothing is quantised to integer levels: PIL quantises at every stage, this is
 *   a float pipeline like the cars'.
 *  yolo_plate_stats: per image and channel c of R, G, B the sum of Q_c over ALL canvas pixels (pixels whose Q is known to be 0 --
 *   s == 0 and outside the window -- are passed over), each converted to double and added in double, as 16 partial sums whose
 *   order does not depend on the window (workspace: yolo_plate_workspace_bytes(N, H, W) bytes, 8-byte aligned, caller-owned); no
 *   atomics.
 *  yolo_plate_render: mu_c, k_c as yolo_render_cars computes them from the partials, D and e;  per pixel
 *   fg_c = (((A[c][0]*Q_0 + A[c][1]*Q_1) + A[c][2]*Q_2) + k_c) / 255.f;   mask = Q_3 / 255.f
 *   out_c = min(max(bg_c * (1.f - mask) + fg_c * mask, 0), 1)                     (yolo_composite_unit's operation order)
 *  With s == 0 a pixel outside the window, and every pixel of a no-plate image whatever s is: out_c = min(max(bg_c, 0), 1).
 *  out may alias bg: each thread reads its pixels before it writes them.
 * YOLO_EINVAL: a NULL pointer, a non-positive N, H or W, a misaligned pointer.  YOLO_EUNSUPPORTED: H * ceil(W / 4) beyond 2^31.
 * Validation comes before any launch.  yolo_plate_workspace_bytes returns YOLO_EINVAL for a non-positive size.
 * 16-byte bg loads and plane stores when W % 4 == 0 and bg, out are 16-byte aligned, scalar ones otherwise.
 * Stream order: yolo_plate_compose, yolo_plate_stats, yolo_plate_render on the same rows. */
#define YOLO_PLATE_ROW_WORDS 48
#define YOLO_PLATE_GLYPH_BYTES 553600
long long yolo_plate_workspace_bytes(int N, int H, int W);
int yolo_plate_compose(const unsigned char* glyphs, const void* rows, unsigned char* plates, int N, void* stream);
int yolo_plate_stats(const unsigned char* plates, const void* rows, void* workspace, int N, int H, int W, void* stream);
int yolo_plate_render(const float* bg, const unsigned char* plates, const void* rows, const void* workspace, float* out, int N, int H,
                      int W, void* stream);

/* The background batch of a training step (yolo_modules/yolo_gluon.py:43-97: load_background's mxnet.image.ImageIter with rand_crop,
 * rand_resize, rand_mirror and the colour jitters, read by ImageIter_next_batch) with the PIXELS made on the device: the host decides
 * (image, mip level, crop, mirror, colour: yolo_amd/background.py BackgroundBank.draw_params) and hands over one row of
 * YOLO_BG_ROW_WORDS 32-bit words per OUTPUT image:
 *   0 has-image (int)      1 h  2 w: the mip level's size (int)      3..6 roi x0, y0, x1, y1 (int; inclusive, in level pixels)     7 unused
 *   8,9 the level's byte offset in the bank (one 64-bit int)         10..15 a0..a5 (float): output pixel INDEX -> level pixel INDEX
 *   16..24 A  25..33 D (3x3 row-major, float)   34..36 e (float)     37..39 unused
 * bank: 4-byte pixels (R, G, B and a pad byte), every image and its mip levels packed densely as (h, w, 4), bank_bytes in all, 4-byte
 * aligned; rows ON THE DEVICE, 8-byte aligned; out (N,3,H,W) f32 0..255, dense -- what yolo_render_cars takes as bg.
 * The arithmetic, every operation in fp32, in this order, nothing fused (this is the definition; tests/background_ref.py restates it):
 *  the sample P(j, i) at output pixel (column j, row i), three channels R, G, B interpolated independently:
 *   sx = (a0*j + a1*i) + a2;  sy = (a3*j + a4*i) + a5;   x0 = floor(sx), fx = sx - x0;  y0 = floor(sy), fy = sy - y0
 *   taps a = (y0, x0), b = (y0, x0+1), c = (y0+1, x0), d = (y0+1, x0+1), every INDEX clamped into the roi (replicate: cv2.resize on
 *   the crop; no tap reads 0, unlike yolo_render_cars'), each read as its byte's float;
 *   top = a + fx*(b - a);  bot = c + fx*(d - c);  P = top + fy*(bot - top)
 *  yolo_bg_stats: per image and channel c the sum of P_c over ALL H*W output pixels, each converted to double and added in double,
 *   as BG_STAT_BLOCKS = 16 partial sums in a fixed order (workspace: yolo_bg_workspace_bytes(N, H, W) bytes, 8-byte aligned,
 *   caller-owned); no atomics, so the sums do not depend on scheduling.
 *  yolo_bg_render: sum_c = the image's partials added in index order (double);  mu_c = (float)(sum_c / (double)(H*W));
 *   k_c = ((D[c][0]*mu_0 + D[c][1]*mu_1) + D[c][2]*mu_2) + e_c
 *   out_c = ((A[c][0]*P_0 + A[c][1]*P_1) + A[c][2]*P_2) + k_c          (NO clamp and NO / 255: mxnet's augmenters do not clamp, and
 *   yolo_render_cars clamps at its blend)
 *  x0 / y0 are limited to +-2^30 before they become integers.  No load leaves the bank whatever a row holds: a row is "no image" if
 *  has == 0, or its level does not lie inside the bank (offset negative or not a multiple of 4, h or w <= 0, offset + 4 h w beyond
 *  bank_bytes), or its roi is empty or not inside the level (x0 < 0, y0 < 0, x1 < x0, y1 < y0, x1 >= w, y1 >= h).  For such a row
 *  P = 0 everywhere -- so mu = 0 and out_c = e_c -- and the bank is not touched.
 * YOLO_EINVAL: a NULL pointer, a non-positive N, H, W or bank_bytes, a misaligned bank / rows / workspace.  YOLO_EUNSUPPORTED:
 * H * ceil(W / 4) beyond 2^31.  Validation comes before any launch.  yolo_bg_workspace_bytes returns YOLO_EINVAL for a non-positive
 * size.  16-byte plane stores when W % 4 == 0 and out is 16-byte aligned, scalar ones otherwise.
 * yolo_bg_render must follow yolo_bg_stats on the same rows, in stream order. */
#define YOLO_BG_ROW_WORDS 40
long long yolo_bg_workspace_bytes(int N, int H, int W);
int yolo_bg_stats(const unsigned char* bank, long long bank_bytes, const void* rows, void* workspace, int N, int H, int W, void* stream);
int yolo_bg_render(const unsigned char* bank, long long bank_bytes, const void* rows, const void* workspace, float* out, int N, int H,
                   int W, void* stream);

/* Anchor fitting: the reference's kmean mode (car/YOLO.py:599-638) and its IoU k-means (yolo_modules/iou_kmeans.py:11-52, get_dis :55-75)
 * on the device, the restarts side by side and each run to convergence (the reference makes one random start and exactly 10 rounds, and
 * fails on an empty cluster, iou_kmeans.py:42).  dis_method = 'L2' (:77-79) is not offered: the kmean mode never uses it.
 * sizes: a device pointer to n rows, row i at sizes + i * stride floats, h = row[0], w = row[1], stride >= 2 -- a label tensor
 * (B, nobj, 6 + ncls) is read in place from &labels[0][0][3] with stride = 6 + ncls (car/YOLO.py:616).  centroids / init: [h, w] pairs.
 * The arithmetic, every operation in fp32, in this order, nothing fused (this is the definition; tests/anchor_ref.py restates it):
 *  row i is VALID iff h and w are finite and > 0 (the -1 of "no object", 0, NaN and inf are not);
 *  q(i, j) against centroid (ch, cw) (iou_kmeans.py:68-74):   ih = min(h, ch);  iw = min(w, cw);  inter = ih * iw;
 *   union = (h * w + ch * cw) - inter;   q = inter / union  (IEEE division)
 *  assignment: a_i = the lowest j with the largest q -- start from j = 0, replace only on q > best (the argmin of 1 / iou,
 *   iou_kmeans.py:32, is the same rule); q_i = that q; an invalid row has a_i = -1, q_i = 0 and is counted nowhere
 *  update (iou_kmeans.py:43-44) of a cluster with count_j > 0:  ch_j' = (float)(sum_i (double)h_i / (double)count_j), cw_j' likewise
 *   (the order of the double sum is the implementation's: fixed, so the same inputs give the same bits); a cluster with
 *   count_j == 0 keeps its centroid
 * yolo_anchor_assign: one assignment pass.  assign (n) and best_iou (n) may be NULL; counts (k); mean_iou (1) =
 *  sum over valid rows of (double)q_i / n_valid, 0 when n_valid == 0; n_valid (1).
 * yolo_anchor_kmeans: restart r starts from init[r] (R, k, 2) and repeats assign + update.  It is CONVERGED after the first round whose
 *  new centroids equal the old ones bit for bit (that round is counted in iters[r]); otherwise it stops after max_iters rounds with
 *  converged[r] = 0.  centroids (R, k, 2); counts (R, k) and mean_iou (R) are those of one more assignment pass on the RETURNED
 *  centroids, so they agree with yolo_anchor_assign on them; iters (R), converged (R), n_valid (1).  Restarts are independent: restart
 *  r of an R-restart call equals, bit for bit, a one-restart call with init[r].  init must be finite and positive; with anything else
 *  that restart's result is unspecified, but the loop still ends at max_iters and no access leaves the buffers.
 * One workgroup per restart, no atomics, no communication between workgroups.  workspace: yolo_anchor_workspace_bytes(n, R, k) bytes,
 * 8-byte aligned, caller-owned (the present decomposition keeps nothing there; the size is small and positive).
 * YOLO_EINVAL: a NULL pointer other than assign / best_iou, n, k, R or max_iters < 1, stride < 2, a pointer not aligned to its
 * element (mean_iou and workspace: 8 bytes).  YOLO_EUNSUPPORTED: k > 32 (yolo_grid_desc's 4 scales x 8 anchors), R > 65535,
 * max_iters > 10000.  Validation comes before any launch.  yolo_anchor_workspace_bytes returns YOLO_EINVAL for a size < 1.
 * 8-byte row loads when stride == 2 and sizes is 8-byte aligned, scalar ones otherwise. */
long long yolo_anchor_workspace_bytes(int n, int R, int k);
int yolo_anchor_assign(const float* sizes, long long stride, int n, const float* centroids, int k, int* assign, float* best_iou,
                       int* counts, double* mean_iou, int* n_valid, void* workspace, void* stream);
int yolo_anchor_kmeans(const float* sizes, long long stride, int n, const float* init, int R, int k, int max_iters, float* centroids,
                       int* counts, double* mean_iou, int* iters, int* converged, int* n_valid, void* workspace, void* stream);

/* Frame overlay: the drawing end of the reference's video node (car/video_node.py:235-326 Video.process / visualize,
 * car_and_LP/carLP_video_node.py:74-86 visualize_carlp) from rows that are still on the device: the car box of cv2_add_bbox
 * (yolo_modules/yolo_cv.py:239-270), the plate edges and the clipped plate's map of ProjectRectangle6D.add_edges
 * (licence_plate_render/__init__.py:379-402), and the NMS boxes (no counterpart in the reference).  Text labels: yolo_overlay_labels
 * and yolo_overlay_text below; the azimuth and the depth lookup of Video.process: yolo_pose_top1.  The radar plot is not offered.
 * The shape table, 16-byte aligned: per image K slots of YOLO_OVERLAY_SLOT_WORDS int32 words
 *   0..7 the four vertices x0 y0 x1 y1 x2 y2 x3 y3 (frame pixels)   8 colour (4 bytes, byte c = channel c)   9 thickness t   10 enabled
 *   11 unused
 * yolo_overlay_table_bytes(B, K) is its size (YOLO_EINVAL for a size < 1, YOLO_EUNSUPPORTED for K > YOLO_OVERLAY_MAX_SLOTS).
 *
 * yolo_overlay_shapes fills the table (B, K, 12) and optionally `vertices` (B, K, 4, 2) fp32 (may be NULL), one thread per slot.  The
 * slots in painter's order (a later slot paints over an earlier one), each source present iff its first pointer is not NULL, and K must
 * be their sum:
 *  post_nms NMS slots -- rows (B, nbox, rows_C) [score, l, t, r, b, rot, cls...], kept (B, post_nms), kept_count (B), cand_per_box as
 *   yolo_decode_nms / yolo_nms_from_scores return them.  Slot j is kept position j: id = kept[b][j]; disabled if j >= min(kept_count[b],
 *   post_nms), id < 0 or box = id / cand_per_box >= nbox.  Colour = palette[(id % cand_per_box) % npalette] (palette: npalette x 4 bytes
 *   on the device).  Vertices (l W, t H), (r W, t H), (r W, b H), (l W, b H): no rotation.
 *  one top-1 slot -- pred (B, pred_C) [score, y, x, h, w, rot, cls...] (yolo_predict_top1): cv2_add_bbox's corners, in its order
 *   (:259-264), r = use_r ? -rot : 0;  h = pred[3] H;  w = pred[4] W;  s = (pred[2] W, pred[1] H);
 *   wc = (w cos r) / 2;  hs = (h sin r) / 2;  ws = (w sin r) / 2;  hc = (h cos r) / 2
 *   v0 = ((wc - hs) + s.x, (ws + hc) + s.y)    v1 = ((-wc - hs) + s.x, (-ws + hc) + s.y)
 *   v2 = ((-wc + hs) + s.x, (-ws - hc) + s.y)  v3 = ((wc + hs) + s.x, (ws - hc) + s.y)
 *   enabled iff score > car_threshold (strict, car/video_node.py:316); colour car_color.
 *  one plate slot -- lp (B, 7) [score, X, Y, Z, r1, r2, r3] (yolo_predict_lp_nhwc), the camera fx, fy, cx, cy, cam_w, cam_h:
 *   projection_matrix's closed form (:352-377), a = sin r1 cos r2 84, b = sin r1 sin r2 cos r3 84, c = sin r2 199.5, d = sin r3 cos r1 84,
 *   e = cos r2 cos r3 199.5, f = sin r1 sin r2 sin r3 84, g = sin r3 cos r2 199.5, h = cos r1 cos r3 84 (products left to right), and the
 *   three rows of `ans` as written there (sums left to right); corner i = (float)(ans[0][i] / ans[2][i]), (float)(ans[1][i] / ans[2][i])
 *   as __call__ returns it (:344-348), then scaled IN FP32 by xs = (float)((double)W / cam_w), ys = (float)((double)H / cam_h)
 *   (add_edges :382-386).  Enabled iff score > lp_threshold; colour lp_color.
 *  Every operation is fp64 (the inputs converted from fp32 first; sin and cos are the device library's) in the written order, nothing
 *  fused, except the plate's two fp32 steps above.  `vertices` are the fp64 vertices rounded to fp32 (the plate's: the fp32 scaled
 *  corners).  A vertex becomes an integer by truncation toward zero (numpy's astype(int)); a slot one of whose vertices is not finite or
 *  has |coordinate| > 2^20 is disabled and its integer vertices are 0.  The thickness of every slot is `thickness`.
 *  With lp the kernel also writes matrices (B, 9) fp32 -- the map from a pixel of the (lp_h, lp_w) plate image to frame pixels that
 *  yolo_warp_u8_to_nchw takes (yolo_amd/intake.py plate_matrix on the host) -- and lp_valid (B) bytes.  The eight unknowns m0..m7 of
 *   u = (m0 x + m1 y + m2) / (m6 x + m7 y + 1),  v = (m3 x + m4 y + m5) / (m6 x + m7 y + 1)   through the four pairs
 *   (x, y) = (lp_w, lp_h), (0, lp_h), (0, 0), (lp_w, 0) [the reference's order, :392-395]  ->  (u, v) = the fp32 scaled corners, as doubles:
 *   rows 0..3 = [x, y, 1, 0, 0, 0, -x u, -y u | u], rows 4..7 = [0, 0, 0, x, y, 1, -x v, -y v | v].  Gaussian elimination in fp64: for
 *   column k = 0..7 the pivot row is the one of rows k..7 with the largest |A[r][k]| (the lowest such row among equals), swapped into
 *   row k; for r = k+1..7: f = A[r][k] / A[k][k], A[r][c] = A[r][c] - f A[k][c] for c = k..8.  Back-substitution for k = 7..0:
 *   s = A[k][8]; s = s - A[k][c] m_c for c = k+1..7 in that order; m_k = s / A[k][k].  The matrix is [(float)m0..(float)m7, 1].
 *   lp_valid = score > lp_threshold, and the four ans[2][i] are non-zero, and the corners are finite, and every pivot is non-zero and
 *   finite, and m0..m7 are finite.  Otherwise the matrix is [0, 0, -4, 0, 0, -4, 0, 0, 1]: the warp then reads only outside the frame
 *   and, with border 0, returns zeros.  No NaN is ever written to a matrix.
 * YOLO_EINVAL: a NULL table, B, H, W, K or thickness < 1, all three sources NULL, K not the sum above, an incomplete source (rows without
 *  kept / kept_count / palette, nbox, post_nms, cand_per_box or npalette < 1, rows_C < 5, pred_C < 6, lp without matrices / lp_valid or
 *  with a non-positive camera or plate size), a table not 16-byte aligned, a vertices / matrices pointer not 4-byte aligned.  YOLO_EUNSUPPORTED:
 *  K > YOLO_OVERLAY_MAX_SLOTS, H or W > 16384, thickness > 255.
 *
 * yolo_overlay_draw paints a table (N, K, 12) onto frames (N, H, W, C) uint8 in place, C in 1..4, frames at ANY byte address.  This is
 * a definition of its own, not cv2.polylines' pixels (a Bresenham line thickened to 2 px; this rule gives 3 px on an axis-aligned edge
 * at t = 2).  Shape s paints pixel P = (x, y) iff for one of its four closed segments A -> B (vertices 0-1, 1-2, 2-3, 3-0) the distance
 * from the integer point to the segment satisfies 4 dist^2 <= t^2, decided exactly in integers: d = B - A, p = P - A, u = p . d;
 *   u <= 0: 4 |p|^2 <= t^2;    u >= d . d: 4 |p - d|^2 <= t^2;    otherwise: 4 cross(p, d)^2 <= t^2 (d . d)
 * (A = B is the first case: a disc).  The pixel takes bytes 0..C-1 of the colour of the HIGHEST enabled slot that paints it; a pixel no
 * enabled slot paints is not written, and the frame of an image without an enabled slot is not accessed at all.  A slot counts as
 * enabled iff word 10 != 0, 1 <= t <= 255 and every vertex coordinate lies in [-2^20, 2^20]; with those limits and H, W <= 16384 no
 * intermediate leaves 64 bits (|cross| >= 2^31 is already outside).  No frame byte is read; no atomics and no dependence on block
 * order: the result is bitwise reproducible.
 * YOLO_EINVAL: a NULL pointer, N, H, W, C or K < 1, a table not 16-byte aligned.  YOLO_EUNSUPPORTED: K > YOLO_OVERLAY_MAX_SLOTS, C > 4,
 *  H or W > 16384.  Validation comes before any launch. */
#define YOLO_OVERLAY_SLOT_WORDS 12
#define YOLO_OVERLAY_MAX_SLOTS 128
long long yolo_overlay_table_bytes(int B, int K);
int yolo_overlay_shapes(const float* rows, const int* kept, const int* kept_count, int nbox, int rows_C, int post_nms, int cand_per_box,
                        const unsigned char* palette, int npalette, const float* pred, int pred_C, float car_threshold, int use_r,
                        unsigned car_color, const float* lp, double fx, double fy, double cx, double cy, int cam_w, int cam_h,
                        float lp_threshold, unsigned lp_color, int lp_h, int lp_w, int B, int H, int W, int thickness, int* table, int K,
                        float* vertices, float* matrices, unsigned char* lp_valid, void* stream);
int yolo_overlay_draw(unsigned char* frames, const int* table, int N, int H, int W, int C, int K, void* stream);

/* Text labels on the overlay: what cv2_add_bbox_text (yolo_modules/yolo_cv.py:273-282) is for -- class, score and azimuth at a box's
 * top-left corner.  The reference never calls that helper, so the text is this library's own definition (a bitmap font the caller
 * brings, an exact integer rule), not cv2.putText's Hershey pixels.
 * The label table, 16-byte aligned: per image K labels of YOLO_OVERLAY_LABEL_WORDS int32 words, label k belonging to slot k
 *   0 x   1 y (the top-left pixel of the first character cell; may be negative)   2 text colour   3 ground colour (4 bytes each, byte c =
 *   channel c)   4 flags (bit 0 enabled, bit 1 ground box on)   5 nchar, 0..YOLO_OVERLAY_LABEL_CHARS
 *   6..15 the text: byte i in word 6 + i / 4 at bits 8 (i % 4)
 *
 * yolo_overlay_labels writes the label table (B, K, 16) for a shape table (B, K, 12) that yolo_overlay_shapes has filled, from the same
 * sources in the same slot order (rows / kept / kept_count / nbox / rows_C / post_nms / cand_per_box, pred / pred_C, lp: as there; each
 * present iff its first pointer is not NULL, K their sum), one thread per slot.  A label is enabled iff its slot's word 10 is non-zero
 * (and, for an NMS slot, its id passes yolo_overlay_shapes' test again: no row is read through an id refused there); a disabled
 * label is sixteen zero words.  Text colour = the slot's colour word, ground colour = ground_colour, flags = 1 | (ground ? 2 : 0).
 *  Text = [name ' '] score [' ' deg]:
 *   name   names[c] up to its first zero byte, at most YOLO_OVERLAY_NAME_BYTES (names: nname x 16 bytes, zero padded, on the device;
 *          may be NULL with nname 0); left out with its space when c < 0, c >= nname or the name is empty
 *   score  five bytes.  For a finite s >= 0: n = min(llrint((double)s * 1000.0), 9999) [round to nearest, ties to even] printed as
 *          d.ddd -- (double)s * 1000.0 is exact, so this is C's "%.3f" digit for digit up to 9.999; otherwise the bytes "-.---"
 *   deg    d = rint((double)azimuth * 57.29577951308232) printed as an optional '-' and 1..3 digits without padding (-0 prints "0");
 *          only for the top-1 slot, only with pose and show_deg != 0, only for a finite azimuth with |d| <= 999
 *  per source:
 *   NMS slot j   id = kept[b][j];  c = cand_per_box > 1 ? id % cand_per_box : -1;
 *                s = kept_scores ? kept_scores[b][j] : rows[b][id / cand_per_box][0]   (kept_scores (B, post_nms) may be NULL)
 *   top-1 slot   s = pred[b][0];  with pose (B, 4) [azimuth, radius, depth, class] of yolo_pose_top1 (may be NULL, else 16-byte aligned):
 *                c = (int)pose[b][3] when -1 < pose[b][3] < nname, else no name; azimuth = pose[b][0].  Without pose: no name, no deg
 *   plate slot   s = lp[b][0], no name
 *  Geometry, integers only (64-bit, x and y saturated to [-2^30, 2^30] at the end): bx0 / by0 = the smallest x / y of the slot's four
 *  integer vertices (for an unrotated box cv2_add_bbox_text's (left, top));  Th = cell_h scale;  Tw = ((nchar - 1) advance + cell_w) scale
 *   y = by0 - gap - Th;  if y - pad < 0: y = by0 + gap          (no room above: the label moves under the box's top edge)
 *   x = bx0;  if x + Tw + pad > W: x = W - Tw - pad;  after that, if x - pad < 0: x = pad
 * YOLO_EINVAL: a NULL table or labels, B, H, W or K < 1, all three sources NULL, K not their sum, an incomplete source (rows without kept
 *  / kept_count, nbox, post_nms or cand_per_box < 1, rows_C < 5, pred_C < 6), nname < 0 or names NULL with nname > 0, cell_w, cell_h or
 *  scale < 1, advance < cell_w, gap or pad < 0, ground not 0 / 1, a table, labels or pose pointer not 16-byte aligned.
 *  YOLO_EUNSUPPORTED: K > YOLO_OVERLAY_MAX_SLOTS, cell_w or cell_h > 32, scale > 16, H or W > 16384.  Validation comes before any launch.
 *
 * yolo_overlay_text paints a label table (N, K, 16) onto frames (N, H, W, C) uint8 in place, C in 1..4, frames at ANY byte address.
 * font is (nglyph, cell_h) uint32 on the device: bit c of font[g][r] (bit 0 = the leftmost column) is the ink of column c, row r of glyph
 * g; glyph g draws the byte first_code + g.  With Th and Tw as above:
 *   character i of a label occupies the cell with origin (ox_i, y) = (x + i advance scale, y) and size (cell_w scale, cell_h scale)
 *   pixel P is INK of the label iff P lies in the cell of some i < nchar with g = byte_i - first_code in [0, nglyph) and bit
 *     (Px - ox_i) / scale of font[g][(Py - y) / scale] is set (cells never overlap: advance >= cell_w); a byte outside the font inks nothing
 *   pixel P is GROUND of the label iff bit 1 of its flags is set, nchar > 0 and P lies in [x - pad, x + Tw + pad) x [y - pad, y + Th + pad)
 * A pixel inside the frame takes bytes 0..C-1 of the colour of the HIGHEST enabled label of which it is ink or ground -- the text colour
 * for ink, the ground colour for ground that is not ink; a pixel no label paints is not written, no frame byte is read, and the frame
 * of an image without an enabled label is not accessed at all.  A label counts as enabled iff bit 0 of its flags is set,
 * 0 <= nchar <= YOLO_OVERLAY_LABEL_CHARS and |x|, |y| <= 2^20.  No atomics and no dependence on block order: the result is bitwise
 * reproducible; no store leaves the frame whatever a label holds.
 * YOLO_EINVAL: a NULL pointer, N, H, W, C, K, nglyph, cell_w, cell_h or scale < 1, advance < cell_w, pad < 0, labels not 16-byte aligned,
 *  font not 4-byte aligned.  YOLO_EUNSUPPORTED: K > YOLO_OVERLAY_MAX_SLOTS, C > 4, H or W > 16384, cell_w or cell_h > 32, scale > 16,
 *  nglyph > 256.  Validation comes before any launch. */
#define YOLO_OVERLAY_LABEL_WORDS 16
#define YOLO_OVERLAY_LABEL_CHARS 40
#define YOLO_OVERLAY_NAME_BYTES 16
int yolo_overlay_labels(const int* table, const float* rows, const int* kept, const int* kept_count, const float* kept_scores, int nbox,
                        int rows_C, int post_nms, int cand_per_box, const float* pred, int pred_C, const float* pose, int show_deg,
                        const float* lp, const unsigned char* names, int nname, int cell_w, int cell_h, int advance, int scale, int gap,
                        int pad, int ground, unsigned ground_colour, int B, int H, int W, int K, int* labels, void* stream);
int yolo_overlay_text(unsigned char* frames, const int* labels, const unsigned* font, int nglyph, int first_code, int cell_w, int cell_h,
                      int advance, int scale, int pad, int N, int H, int W, int C, int K, void* stream);

/* 2x nearest up-sample of `up` (N,H/2,W/2,C1) + channel concat with `route` (N,H,W,C2) ->
 * (N,H,W,C1+C2), up-sampled channels first: gluoncv _upsample + F.concat, car/utils.py:92-93. */
int yolo_upsample2x_concat(const void* up, const void* route, void* y, int N, int H, int W,
                           int C1, int C2, int dtype, void* stream);

/* ---- detection post-processing --------------------------------------------------------- */

/* Anchor-grid description shared by decode / assignment (car/YOLO.py:112-155):
 * nscale scales fine->coarse; scale i has grid (gh[i], gw[i]), stride step[i] px and A anchors
 * anchors_hw[(i*A+a)*2+{0,1}] = (h, w) as fractions of the image. */
typedef struct yolo_grid_desc {
    int nscale, A;
    int img_h, img_w;
    int gh[4], gw[4], step[4];
    float anchors_hw[4 * 8 * 2];
} yolo_grid_desc;

/* out (B, N, A, C) float32 logits, channel order [obj, ty, tx, th, tw, rot, cls...]
 * (slice_point [1,3,5,6,C], car/v1/spec.yaml:6) -> rows (B, N*A, C) float32
 * [sigmoid(obj), l, t, r, b, rot, cls...]: _yxhw_to_ltrb + the concat in predict,
 * car/YOLO.py:552-579. */
int yolo_decode(const float* out, float* rows, int B, int C, const yolo_grid_desc* g, void* stream);

/* Per-image arg-max of sigmoid(obj) over N*A boxes (lowest index among ties, mxnet argmax),
 * and the reference's output row [score, y, x, h, w, rot, cls...]: car/YOLO.py:581-597.
 * `out` are the raw logits (B,N,A,C); pred (B,C) float32; best_idx (B) int32. */
int yolo_predict_top1(const float* out, float* pred, int* best_idx, int B, int C,
                      const yolo_grid_desc* g, void* stream);

/* LicencePlateDetectioin.predict_LP (licence_plate/LP_detection.py:147-162; BASELINE config 1 plumbing):
 * out (1,C,h,w) float32 NCHW -> pred (C) [sigmoid(score), xyz*1000, 3 angles (sigmoid-.5)*2*r_max*pi/180, rest
 * raw] of the cell with the highest channel-0 value (first among ties); best_idx (1) int32. */
int yolo_predict_lp(const float* out, float* pred, int* best_idx, int C, int h, int w, float r_max0,
                    float r_max1, float r_max2, void* stream);

/* CarLPNet.predict_LP + LP_pose_activation (car_and_LP/YOLO.py:133-169): out (B, h*w, C) float32 NHWC (the LP branch
 * output, C = LP_slice_point[-1] >= 7, channel order [score, x, y, z, r1, r2, r3, class...]) -> pred (B, 7): per image
 * the cell with the highest sigmoid(score) (first among ties): [sigmoid(score), xyz * 1000, three angles
 * (sigmoid - 0.5) * 2 * r_max * pi / 180]; best_idx (B) the chosen cells. */
int yolo_predict_lp_nhwc(const float* out, float* pred, int* best_idx, int B, int hw, int C, float r_max0,
                         float r_max1, float r_max2, void* stream);

/* get_iou(predict, target, mode=2), yolo_gluon.py:127-168: boxes (n,4) ltrb vs one target
 * [c,y,x,h,w] (5 floats, device) -> iou (n). */
int yolo_iou_ltrb_vs_yxhw(const float* boxes, const float* target, float* iou, int n, void* stream);
/* get_iou(predict, target, mode=1) -- the reference's DEFAULT mode (yolo_gluon.py:127): target [c,l,t,r,b]; keeps the
 * reference's target_area = target[3] * target[4] (yolo_gluon.py:166; = r * b in this mode), so a caller that omits
 * `mode` gets the reference's numbers, quirk included. */
int yolo_iou_ltrb_vs_cltrb(const float* boxes, const float* target, float* iou, int n, void* stream);

/* Greedy per-class NMS over decoded rows (not in the reference -- SURVEY.md S1; semantics =
 * SURVEY App. A.8).  mode 0: score = sigmoid(obj), class-agnostic; mode 1: candidates are
 * (box, class) pairs scored sigmoid(obj)*softmax(cls)_c, suppression within a class.
 * kept (B, post_nms) int32 candidate ids in score order padded with -1; kept_scores same
 * shape; kept_count (B).  workspace: yolo_nms_workspace_bytes() = the score array + the selection workspace. */
long long yolo_nms_workspace_bytes(int B, int nbox, int ncls, int mode, int topk);
/* The two halves of yolo_nms, exposed so the score array can be inspected / injected:
 * scores (B, nbox) [mode 0] or (B, nbox*ncls) [mode 1]; candidate id = box*cand_per_box + class.
 * select_workspace (yolo_nms_select_workspace_bytes(B), may be NULL): with it the top-k pre-selection runs as
 * chip-wide passes over all images instead of one block per image (same result; ~6x faster at 608x608). */
long long yolo_nms_select_workspace_bytes(int B);
int yolo_nms_scores(const float* rows, float* scores, int B, int nbox, int C, int mode, void* stream);
/* yolo_decode + yolo_nms_scores in one pass over the logits (the logits are read once; bit-identical results):
 * out (B,N,A,C) -> rows (B,nbox,C) and scores as above. */
int yolo_decode_scores(const float* out, float* rows, float* scores, int B, int C, const yolo_grid_desc* g, int mode,
                       void* stream);
int yolo_nms_from_scores(const float* rows, const float* scores, int B, int nbox, int C,
                         int cand_per_box, float valid_thresh, float iou_thresh, int topk,
                         int post_nms, int* kept, float* kept_scores, int* kept_count,
                         void* select_workspace, void* stream);
int yolo_nms(const float* rows, int B, int nbox, int C, int mode, float valid_thresh,
             float iou_thresh, int topk, int post_nms, int* kept, float* kept_scores,
             int* kept_count, void* workspace, void* stream);
/* yolo_decode_scores + yolo_nms_from_scores as ONE call -- the post-processing of BASELINE configs[4] (608x608 inference incl.
 * anchor decode + NMS; no counterpart in the reference): the decode pass takes the selection's first
 * radix histogram from the scores it holds in LDS, so the score array is streamed twice instead of three times.  Identical
 * rows, scores and kept ids to the two calls.  select_workspace: yolo_nms_select_workspace_bytes(B), REQUIRED here. */
int yolo_decode_nms(const float* out, float* rows, float* scores, int B, int C, const yolo_grid_desc* g, int mode,
                    float valid_thresh, float iou_thresh, int topk, int post_nms, int* kept, float* kept_scores,
                    int* kept_count, void* select_workspace, void* stream);

/* ---- evaluation (detection quality on the device) -------------------------------------------- */

/* Matching of ranked detections to ground truth, PASCAL-VOC devkit semantics (no counterpart in the reference, whose only
 * quality figures are the top-1 ones below; scores what the per-class NMS of SURVEY App. A.8 keeps).  rows (B, nbox, C) decoded
 * rows, kept (B, post_nms) / kept_count (B) as yolo_nms_from_scores / yolo_decode_nms return them (candidate id = box *
 * cand_per_box + class); labels (B, nobj, label_cols >= 5) float32 in the training layout [cls, y, x, h, w, ...] (car/YOLO.py:525),
 * cls < 0 = no object.  Per detection, in kept (= score) order: the valid ground truth (of the detection's class when
 * class_aware) with the largest IoU, lowest index among equals; a true positive iff that IoU > iou_thresh and no earlier
 * detection chose the same ground truth above the threshold (a later one is a false positive: no second choice).
 * Outputs, one slot per (image, kept position): det_class, det_tp (1 / 0), det_gt (-1: none), det_iou; slots at or beyond
 * kept_count, or holding an id outside [0, nbox * cand_per_box), are pads: class -1, tp -1, gt -1, iou 0.  gt_class (B, nobj):
 * int(cls), 0 for every valid label when not class_aware, -1 for no object.  One block per image, no global atomics:
 * bitwise reproducible.  nobj <= 512 and post_nms <= 1024 (YOLO_EUNSUPPORTED beyond). */
int yolo_eval_match_supported(int nobj, int post_nms);
int yolo_eval_match(const float* rows, const int* kept, const int* kept_count, const float* labels, int B, int nbox, int C,
                    int cand_per_box, int post_nms, int nobj, int label_cols, int class_aware, float iou_thresh,
                    int* det_class, int* det_tp, int* det_gt, float* det_iou, int* gt_class, void* stream);

/* The per-image arithmetic of _valid_iou (car/YOLO.py:501-534) plus the azimuth of RadarProb.cls2ang (yolo_cv.py:85-95):
 * pred (B, C) = yolo_predict_top1's rows [score, y, x, h, w, rot, cls...]; labels (B, nobj, label_cols) as above, only object 0
 * of an image is read (car/YOLO.py:525); class_dirs (C - 6, 2) float32 [cos, sin] of the class azimuths.  out (B, 4), 16-byte
 * aligned: [iou, azimuth (rad), radius, valid] -- iou = get_iou(mode 2) of the box rebuilt as car/YOLO.py:518-521 does,
 * azimuth = atan2(sum sin p, sum cos p) with p = softmax(cls logits), radius = score * |mean direction|, valid = cls >= 0
 * (an image without an object is marked invalid; the reference scores it against a box of -1s). */
int yolo_eval_top1(const float* pred, const float* labels, const float* class_dirs, float* out, int B, int C, int nobj,
                   int label_cols, void* stream);

/* The row Video.process publishes (car/video_node.py:235-255, car_and_LP/carLP_video_node.py:48-72), made where the top-1 row is:
 * pred (B, C) = yolo_predict_top1's rows, C > 6; class_dirs (C - 6, 2) [cos, sin] as above.  pose (B, 4), 16-byte aligned:
 *   [azimuth (rad), radius, depth, class]
 *  azimuth, radius  yolo_eval_top1's, by the same device function: the same bits for the same row
 *  class            (float) of the index of the largest class logit, the lowest index among equals; a NaN never wins (all NaN: 0)
 *  depth            depth is NULL or (B, Hd, Wd) float32, one depth frame per image.  NULL: -1 (:243).  Otherwise
 *                   xi = (int)((double)Wd * (double)pred[2]), yi = (int)((double)Hd * (double)pred[1]), truncated toward zero (:239-240),
 *                   and depth[b][yi][xi] copied as it is, a NaN included.  DEVIATION: -1 when pred[1] or pred[2] is not finite or xi is
 *                   outside [0, Wd) or yi outside [0, Hd) -- numpy raises there, or wraps a negative index.
 * rows_out is NULL or (B, C), and may be pred itself: a copy of the row with column 5 left alone (row5 == 0), set to the azimuth
 * (row5 == 1, :251) or to the depth (row5 == 2, carLP_video_node.py:52-57).  One thread per image; it reads its row before it writes it.
 * YOLO_EINVAL: a NULL pred, class_dirs or pose, B < 1, C <= 6, depth with Hd or Wd < 1, row5 outside 0..2, pose not 16-byte aligned.
 * Validation comes before any launch. */
int yolo_pose_top1(const float* pred, int B, int C, const float* class_dirs, const float* depth, int Hd, int Wd, int row5,
                   float* rows_out, float* pose, void* stream);

/* ---- training step (fp32 parity path) ------------------------------------------------------- */

/* Packed weight image of the data-gradient convolution of a forward conv (Cout_f, Cin_f, k): dx =
 * conv_stride1(dy [dilated 2x for stride 2], W'), W'[ci][co][a][b] = W[co][ci][k-1-a][k-1-b]; run it with
 * yolo_conv_fwd (scale 1, bias 0, slope 1, residual = gradient to accumulate into).  Bytes:
 * yolo_packed_weight_bytes(Cin_f, Cout_f, k, dtype).  Replaces the autograd backward of Convolution
 * (sum(losses).backward(), car/YOLO.py:394). */
int yolo_pack_conv_weights_dgrad(const float* w_oihw, void* packed, int Cout_f, int Cin_f, int ksize,
                                 int dtype, void* stream);

/* Sub-pixel form of the data gradient of a 3x3 stride-2 pad-1 convolution (Cout_f, Cin_f) -- the down-sampling convs of
 * every stage, basic_yolo.py:24 -- for even input sizes: instead of zero-dilating dy (4x the arithmetic), the four
 * sub-pixel phases of dx are four output-channel blocks of one 2x2-window convolution over dy:
 *   dx[n, 2m+a, 2n+b, c] = sum_{ty,tx in {0,1}} sum_k W'[(2a+b) Cin_f + c][k][ty][tx] dy[n, m+ty, n+tx, k]   (zero beyond)
 * with W'[..a..][k][ty] = W[k][c][1] for (a,ty) = (0,0), W[k][c][2] for (1,0), W[k][c][0] for (1,1), 0 for (0,1)
 * (likewise b/tx).  yolo_pack_conv_weights_dgrad_s2 writes that image (yolo_packed_weight_bytes(4 Cin_f, Cout_f, 2,
 * dtype) bytes; batch records: Cout = 4 Cin_f, Cin = Cout_f, ksize = 2, dgrad = 2).  yolo_conv_dgrad_s2 runs it:
 * d->x = dy (N,H,W,Cin = Cout_f), d->Cout = 4 Cin_f, d->y = dx (N,2H,2W,Cin_f) dense, d->residual = a gradient to
 * accumulate onto (same shape as dx) or NULL, d->scale / d->bias over 4 Cin_f (padded) channels, ksize / stride /
 * strides ignored; bf16 only.  YOLO_EUNSUPPORTED (Cin_f % 8, Cout_f % 32, halo does not fit): use yolo_dilate2x +
 * yolo_conv_fwd instead.  d->algo: 0 = heuristic, or one of 2 / 6 / 10 / 4 (256 / 192 / 128 px x 256, 128 x 128). */
int yolo_pack_conv_weights_dgrad_s2(const float* w_oihw, void* packed, int Cout_f, int Cin_f, int dtype, void* stream);
int yolo_conv_dgrad_s2(const yolo_conv_desc* d, void* stream);

/* Every conv of a network packed in ONE launch (the training step re-packs all images after each update).
 * items_device: device array of n_items records { const float* w_oihw; void* packed; int Cout, Cin, ksize, dgrad; }
 * (32 bytes each; dgrad = 1: the data-gradient image of the FORWARD conv (Cin, Cout swapped as in
 * yolo_pack_conv_weights_dgrad's arguments)); first_block_device: n_items + 1 prefix sums of
 * yolo_pack_batch_blocks(Cout, Cin, ksize, dtype) over the items; total_blocks = the last prefix. */
typedef struct yolo_pack_item { const float* w_oihw; void* packed; int Cout, Cin, ksize, dgrad; } yolo_pack_item;
long long yolo_pack_batch_blocks(int Cout, int Cin, int ksize, int dtype);
int yolo_pack_conv_weights_batch(const void* items_device, const long long* first_block_device, int n_items,
                                 long long total_blocks, int dtype, void* stream);
/* The forward and the data-gradient image of every listed conv from ONE read of its weights (YOLO_BF16; Cout and Cin
 * multiples of 32; 1x1 and 3x3): items_device = n_items records { const float* w_oihw; void* packed_fwd; void*
 * packed_dgrad; int Cout, Cin, ksize, reserved; } (40 bytes), first_block_device = prefix sums of yolo_pack_pair_blocks()
 * (YOLO_EUNSUPPORTED for a conv this entry does not take).  Bit-identical to yolo_pack_conv_weights +
 * yolo_pack_conv_weights_dgrad except that the padding rows of the images are not written: zero-fill the buffers once. */
typedef struct yolo_pack_pair { const float* w_oihw; void* packed_fwd; void* packed_dgrad; int Cout, Cin, ksize, reserved; } yolo_pack_pair;
long long yolo_pack_pair_blocks(int Cout, int Cin, int ksize);
int yolo_pack_conv_weights_pairs(const void* items_device, const long long* first_block_device, int n_items,
                                 long long total_blocks, void* stream);

/* Gluon BatchNorm in training mode fused with LeakyReLU (+ residual add):
 * batch mean / biased variance over (N,H,W) of the NHWC conv output y (npix x C, dtype; C % 8 == 0),
 * z = lrelu(gamma*(y-mean)*invstd + beta) [+ residual]; running stats r = momentum*r + (1-momentum)*batch
 * (running_var takes the biased variance).  Statistics are accumulated in double.  workspace: 2*C doubles (shared by the
 * backward), ZERO-FILLED by the caller before its first use; every call leaves it zeroed again. */
int yolo_bn_train_fwd(const void* y, const float* gamma, const float* beta, const void* residual,
                      void* z, float* mean, float* invstd, float* running_mean, float* running_var,
                      double* workspace, long long npix, int C, float eps, float momentum, float slope,
                      int dtype, void* stream);
/* Backward of the above w.r.t. y, gamma, beta given dz (the residual branch receives dz unchanged). */
int yolo_bn_train_bwd(const void* dz, const void* y, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, void* dy, float* dgamma, float* dbeta,
                      double* workspace, long long npix, int C, float slope, int dtype, void* stream);

/* The same two calls as TWO launches each: the per-layer finalize / parameter-gradient launches are folded into the apply
 * pass.  `workspace` (2*C doubles) must be ZERO on entry and is left dirty; `zero_next` (a different buffer of
 * zero_next_count doubles -- the next call may have more channels --, or NULL) is zeroed for the caller's next BatchNorm
 * call: callers alternate two workspaces.  Same arithmetic as yolo_bn_train_fwd / _bwd.  yolo_bn_train_fwd_pp does NOT
 * work in place: z == y is refused with YOLO_EINVAL (every block re-reads y at pixel 0, the pivot of its shifted sums,
 * while another block writes z there); yolo_bn_train_fwd may run in place. */
int yolo_bn_train_fwd_pp(const void* y, const float* gamma, const float* beta, const void* residual,
                         void* z, float* mean, float* invstd, float* running_mean, float* running_var,
                         double* workspace, double* zero_next, int zero_next_count, long long npix, int C, float eps,
                         float momentum, float slope, int dtype, void* stream);
int yolo_bn_train_bwd_pp(const void* dz, const void* y, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, void* dy, float* dgamma, float* dbeta,
                         double* workspace, double* zero_next, int zero_next_count, long long npix, int C, float slope,
                         int dtype, void* stream);
/* The same two calls with the reduction pass over the tensor(s) replaced by the partial rows a convolution's statistics
 * epilogue wrote (yolo_conv_desc.stats: stats_mode 1 for the forward call, 2 for the backward call; rows =
 * yolo_conv_stats_rows(), cout_pad = yolo_padded_channels(C)): one small kernel sums the rows in double, then the apply
 * pass runs as in the _pp calls.  YOLO_BF16 only. */
int yolo_bn_train_fwd_partials(const float* partials, int rows, int cout_pad, const void* y, const float* gamma,
                               const float* beta, const void* residual, void* z, float* mean, float* invstd,
                               float* running_mean, float* running_var, double* workspace, double* zero_next,
                               int zero_next_count, long long npix, int C, float eps, float momentum, float slope,
                               int dtype, void* stream);
int yolo_bn_train_bwd_partials(const float* partials, int rows, int cout_pad, const void* dz, const void* y,
                               const float* mean, const float* invstd, const float* gamma, const float* beta,
                               void* dy, float* dgamma, float* dbeta, double* workspace, double* zero_next,
                               int zero_next_count, long long npix, int C, float slope, int dtype, void* stream);


/* Weight gradient of Conv(k, stride, pad k/2): dw (Cout,Cin,k,k) float32 += sum over pixels of
 * dy (N,Ho,Wo,[dy_pixel_stride]) x (N,H,W,Cin), NHWC `dtype`.  The caller zero-fills dw once per step.
 * YOLO_F32: MFMA 32x32x2 f32.  YOLO_BF16: MFMA 32x32x16 bf16 fed by transposing LDS reads
 * (ds_read_b64_tr_b16), fp32 accumulation; needs `workspace` of yolo_conv_wgrad_workspace_bytes(), ZERO-FILLED by
 * the caller before its first use; every call leaves it zeroed again.
 * Extents (NOTES.md, "Offsets past 2^31 and 2^32 bytes: the training step").  YOLO_F32: 64-bit offsets, any extent of x and
 * dy.  YOLO_BF16, by the path yolo_conv_wgrad takes:
 *   - 1x1 with Cin and Cout multiples of 128 (the LDS-DMA GEMM): x and dy each below 0xfffffe00 bytes; from there on the
 *     per-tap kernel;
 *   - 3x3 stride 1 with Cin and Cout multiples of 64 (the row walk): x and dy each below 0xffffff00 bytes; from there on the
 *     next path that takes the shape;
 *   - 3x3 with Cin <= 64, the stride-2 layer with Cin == 64 apart (the column-strip kernel), and 3x3 stride 1 with W <= 40 at
 *     a width the row-group kernel has a variant for: 64-bit bases, ANY extent of x and dy, 4 GiB and more included;
 *   - everything else (the per-tap kernel): x below 0xffffff00 bytes (32-bit buffer offsets), YOLO_EUNSUPPORTED from there
 *     on; dy any extent.
 * So an x of 4 GiB or more is computed by the strip and row-group paths and refused with YOLO_EUNSUPPORTED, nothing written,
 * by the last.  N*H*W and N*Ho*Wo stay below 2^31 - 1.  dy_pixel_stride (bf16: % 8 == 0, not negative): the strip, row-group
 * and per-tap kernels reach 32 (stride 1: Wo + 32), 112 and 64 pixels of dy through 32-bit lane offsets; at a pitch at which
 * that span passes 2^31 bytes the first two hand the call on to the per-tap kernel, and the per-tap kernel answers
 * YOLO_EUNSUPPORTED (pitches of tens of MB per pixel: no caller has one). */
long long yolo_conv_wgrad_workspace_bytes(int Cin, int Cout, int ksize, int dtype);
int yolo_conv_wgrad(const void* dy, const void* x, float* dw_oihw, int N, int H, int W, int Cin, int Cout,
                    int ksize, int stride, long long dy_pixel_stride, int dtype, void* workspace,
                    void* stream);
/* The same with an explicit kernel choice (tuning and tests): algo 0 = the library's choice (what yolo_conv_wgrad
 * runs); 1 = the register-staged kernels (per-tap / column-strip / row-group); 2 / 3 = the pipelined row-walk kernel of
 * the 3x3 stride-1 layers with Cin and Cout multiples of 64 (LDS-DMA ring, x fragments of the three kernel rows held
 * in registers), one 16-column walker / four 4-column walkers per block; 4 = 3 with 8-wave blocks whose two halves walk
 * different row slices and are summed through LDS before the atomics; 5 / 6 = the LDS-DMA GEMM of the 1x1 layers (Cin, Cout
 * multiples of 128) with a 128 x 128 / 256 cout x 128 cin tile; YOLO_EUNSUPPORTED outside a kernel's domain. */
int yolo_conv_wgrad_algo(const void* dy, const void* x, float* dw_oihw, int N, int H, int W, int Cin, int Cout,
                         int ksize, int stride, long long dy_pixel_stride, int dtype, void* workspace, int algo,
                         void* stream);
/* Split weight gradient (YOLO_BF16X3; yolo_conv_wgrad refuses split types): the same sum with dy and x as (hi, lo) pairs and
 * every product taken as dy_hi x_hi + dy_hi x_lo + dy_lo x_hi on v_mfma_f32_32x32x16_bf16 (fp32 accumulation).  x: dense split
 * (N,H,W,Cin), Cin % 8 == 0; dy rows: hi values at dy + p * dy_pixel_stride, lo values dy_lo_offset elements further (0, 0 =
 * dense: lo offset round_up(Cout, 32), pixel stride twice that) -- the padded gradient rows of an output convolution are a
 * slice of wider rows.  k in {1, 3}, stride in {1, 2}.  workspace: yolo_conv_wgrad_split_workspace_bytes(), ZERO-FILLED by the
 * caller before its first use; every call leaves it zeroed again.  algo: 0 = the library's choice, 1 = 64 x 64 tiles,
 * 2 = 128 x 128 tiles.  The kernel's offsets into x are 32-bit: a batch whose x reaches 4 GiB (both planes count) runs as several
 * launches over slices of whole images; YOLO_EUNSUPPORTED only when ONE image's x does.  dy: any extent (a 64-bit base per
 * 32-pixel chunk); 33 pixels of dy_pixel_stride stay below 2^31 bytes (YOLO_EUNSUPPORTED otherwise). */
long long yolo_conv_wgrad_split_workspace_bytes(int Cin, int Cout, int ksize, int dtype);
int yolo_conv_wgrad_split(const void* dy, const void* x, float* dw_oihw, int N, int H, int W, int Cin, int Cout,
                          int ksize, int stride, long long dy_pixel_stride, long long dy_lo_offset, int dtype,
                          void* workspace, int algo, void* stream);
/* db[c] += sum over npix rows of dy (row stride pixel_stride, 0 = C; YOLO_BF16X3: 0 = 2 * round_up(C, 32), the lo value
 * round_up(C, 32) behind the hi value): YOLOOutput's bias gradient. */
int yolo_bias_grad(const void* dy, float* db, long long npix, int C, long long pixel_stride, int dtype,
                   void* stream);
/* float32 (B, rows, [src strides]) C values per row -> dense (B*rows, Cpad) of `dtype`, zero padded (YOLO_BF16X3: dense split
 * rows of Cpad channels; the plane pad beyond Cpad is not written). */
int yolo_gather_rows(const float* src, void* dst, int B, long long rows_per_batch, int C, int Cpad,
                     long long src_batch_stride, long long src_row_stride, int dtype, void* stream);
/* D (N,H,W,C): D[n,2y,2x,:] = dy[n,y,x,:] (dy is (N,Ho,Wo,C)), zeros elsewhere: turns the stride-2 data
 * gradient into a stride-1 convolution.  C % 8 == 0. */
int yolo_dilate2x(const void* dy, void* d, int N, int H, int W, int Ho, int Wo, int C, int dtype,
                  void* stream);
/* Backward of yolo_upsample2x_concat: dcat (N,H,W,C1+C2) -> dup (N,H/2,W/2,C1), droute (N,H,W,C2);
 * accumulate_* != 0 adds into the destination. */
int yolo_upsample2x_concat_bwd(const void* dcat, void* dup, void* droute, int N, int H, int W, int C1,
                               int C2, int accumulate_up, int accumulate_route, int dtype, void* stream);
int yolo_add(const void* a, const void* b, void* y, long long n, int dtype, void* stream);
/* The same for dense split tensors (YOLO_BF16X3) of npix pixels x C channels: an element count alone cannot locate a value's lo
 * plane, which lies round_up(C, 32) behind its hi value.  Sums in fp32, stored as a pair; the pad channels are not written. */
int yolo_add_split(const void* a, const void* b, void* y, long long npix, int C, int dtype, void* stream);

/* _find_best + the scatter of _loss_mask (car/YOLO.py:401-480): labels (B,nobj,6+ncls)
 * [cls,y,x,h,w,rot,dist...] (cls < 0 = no object), anchors_ltrb (nbox,4) = _get_default_ltrb
 * (car/YOLO.py:209-240) -> records (B,nobj,7+ncls) [valid, box index, ty,tx,th,tw, rot, cls...]. */
int yolo_assign_targets(const float* labels, const float* anchors_ltrb, float* records, int B, int nobj,
                        int ncls, const yolo_grid_desc* g, void* stream);
/* _score_weight + _get_loss + the backward of sum(losses) (car/YOLO.py:482-498, :394): logits
 * (B,nbox,C) -> dlogits (B,nbox,C), losses (5,B) [score, box_yx, box_hw, rotate, class].
 * scales5_host: 5 floats on the HOST (spec `scale`; rotate is 0 unless car_rotate). */
int yolo_loss_fwd_bwd(const float* logits, const float* records, float* dlogits, float* losses, int B,
                      int nbox, int C, int nobj, const float* scales5_host, float pos_w, float neg_w,
                      void* stream);

/* CarLPNet's licence-plate branch (licence_plate/LP_detection.py:258-360, car_and_LP/YOLO.py:262-300).
 * yolo_assign_targets_lp = _find_best_LP + the scatter of _loss_mask_LP: labels (B, nobj, lab_w >= 10) rows
 * [flag (<0: none), X, Y, Z (mm), r1, r2, r3 (rad), x_px, y_px, ..., type] -> records (B, nobj, 8 + ncls)
 * [valid, cell = clip(int(y_px/step))*w_ + clip(int(x_px/step)), XYZ/1000, inv_sigmoid(r/r_max/2 + 0.5) x3,
 * one-hot type].  yolo_loss_lp_fwd_bwd = _score_weight_LP + _get_loss_LP + backward on the LP output
 * (B, ncell, C) [score, xy(2), z(1), r(3), class(C-7)]: losses (5, B) [LP_score, LP_xy, LP_z, LP_r, LP_class]. */
int yolo_assign_targets_lp(const float* labels, float* records, int B, int nobj, int lab_w, int ncls, int img_h,
                           int img_w, int step, float r_max0_deg, float r_max1_deg, float r_max2_deg, void* stream);
int yolo_loss_lp_fwd_bwd(const float* logits, const float* records, float* dlogits, float* losses, int B,
                         int ncell, int C, int nobj, const float* scales5, float pos_w, float neg_w, void* stream);
/* mxnet Adam, t = 1-based update count, rescale = 1/global batch
 * (trainer.step(batch_size), car/YOLO.py:396). */
int yolo_adam_step(float* w, const float* grad, float* m, float* v, long long n, int t, float lr,
                   float beta1, float beta2, float eps, float rescale, void* stream);
/* The same update with rescale = 1 / *global_batch_dev read ON THE DEVICE: the batch_size of trainer.step(batch_size)
 * (car/YOLO.py:396) as the SUM of the ranks' shard sizes, which the caller's gradient all-reduce delivers in a slot
 * of the last bucket (yolo_amd/train.py) -- uneven shards (split_render_data, yolo_gluon.py:100-124) need no
 * collective of their own and no host synchronisation. */
int yolo_adam_step_dev(float* w, const float* grad, float* m, float* v, long long n, int t, float lr,
                       float beta1, float beta2, float eps, const float* global_batch_dev, void* stream);

/* ---- DenseNet bodies, inference (csrc/dense.hip) ------------------------------------------------------------------------------
 * gluoncv's DenseNet as the reference's OCRDenseNet (OCR/OCR.py:34-74), LPDenseNet (licence_plate/LP_detection.py:59-97) and
 * CarDenseNet (car/utils.py:48-61) build it: stem, dense blocks, transitions, a final BN + ReLU.  yolo_amd/dense.py states the
 * network; YOLO_BF16 and YOLO_F32 only (YOLO_EUNSUPPORTED for the other valid dtypes).
 * A block's feature map is ONE buffer (N,H,W) pixels x Cs elements, Cs = round_up(the block's final channel count, 32); its layers
 * work in place: layer k reads channels [0, Cin) and writes [Cin, Cin + G).  Channels nobody has written yet may hold anything.
 * Folded BN vectors (scale, bias) are what yolo_fold_bn writes: yolo_padded_channels(C) floats, 16-byte aligned -- the kernels read
 * them in whole 32-channel chunks.
 * DENSE OPERAND IMAGE of a matrix A (M, K), the weight layout of this unit: [ceil(M/16)][ceil(K/32)][64][8] elements of `dtype`,
 * element j of lane l of tile (mt, kc) = A[16 mt + (l & 15)][32 kc + 8 (l >> 4) + j], zero where that is outside A -- the A
 * fragment of v_mfma_f32_16x16x32_bf16 as 64 contiguous 16-byte vectors.  yolo_dense_operand_bytes(M, K, dtype) is its size; it is
 * written on the host when the parameters are prepared (yolo_amd/dense.py pack_operand).  A conv1x1 (Cout, Cin) is the matrix itself;
 * a conv3x3 (G, Cm, 3, 3) is the matrix (G, 9 * round_up(Cm, 32)) with column (3 ky + kx) * round_up(Cm, 32) + j = W[g][j][ky][kx].
 * Every entry validates before it launches: YOLO_EINVAL for a NULL pointer, a non-positive size or an unknown dtype, YOLO_EUNSUPPORTED
 * for a shape outside the stated limits and for a buffer of 2^31 bytes or more. */
long long yolo_dense_operand_bytes(int M, int K, int dtype);
/* One dense layer as one launch: a = max(0, x s1 + t1) over [0, Cin); m = W1 a (Cm channels); b = max(0, m s2 + t2) inside the image
 * and EXACTLY 0 outside (the 3x3 pads b, not m); y = conv3x3(W2, b) (G channels, raw: no BN, no activation) stored to channels
 * [Cin, Cin + G) of the same pixel.  Operands a, b and the weights are rounded once to `dtype`, sums are fp32 (bf16: v_mfma_f32_16x16x32_bf16,
 * f32: v_mfma_f32_16x16x4_f32).  Channels >= Cin of the last K-chunk are masked by a select; no byte outside [Cin, Cin + G) of a pixel is
 * written.  w1_image: operand image of (Cm, Cin); w2_image: of the (G, Cm, 3, 3) weights as above.
 * Supported: G % 4 == 0, G <= 32, Cm % 16 == 0, Cm <= 128, Cin >= 8, Cin + G <= Cs, Cs % 32 == 0, any H, W >= 1. */
int yolo_dense_layer_fwd(void* buf, const void* w1_image, const float* scale1, const float* bias1, const void* w2_image,
                         const float* scale2, const float* bias2, int N, int H, int W, int Cs, int Cin, int Cm, int G, int dtype,
                         void* stream);
/* Stem: Conv 7x7 s2 p3 without bias (w_oihw (F0,3,7,7) float32, unpacked) over the (N,3,H,W) float32 NCHW image + folded BN + ReLU +
 * MaxPool 3x3 s2 p1 -> channels [0, F0) of block 1's buffer (N,Hp,Wp,Cs), Hc = (H-1)/2+1, Hp = (Hc-1)/2+1.  A direct fp32
 * convolution on the vector pipe (K = 147), one rounding at the store.  F0 % 8 == 0, F0 <= 64, Cs % 32 == 0. */
int yolo_dense_stem_fwd(const float* x_nchw, const float* w_oihw, const float* scale, const float* bias, void* y, int N, int H, int W,
                        int F0, int Cs, int dtype, void* stream);
/* Transition: BN + ReLU + Conv 1x1 without bias C -> C/2 + AvgPool 2x2 s2, block buffer x (N,H,W,Cs_in) -> channels [0, C/2) of the
 * next block's buffer y (N,H/2,W/2,Cs_out); an odd last row / column is dropped.  Computed as pool-then-convolve (linear, a quarter of
 * the work): p = ((a00 + a01) + (a10 + a11)) * 0.25 in fp32, rounded once to `dtype`.  w_image: operand image of (C/2, C).  H, W >= 2. */
int yolo_dense_transition_fwd(const void* x, const void* w_image, const float* scale, const float* bias, void* y, int N, int H, int W,
                              int C, int Cs_in, int Cs_out, int dtype, void* stream);
/* The BN + ReLU after the last block, block buffer x (N,H,W,Cs) -> a dense tensor of Cp >= C channels per pixel, channels C..Cp-1 zero:
 * columns == 0: y (N,H,W,Cp), what a 3x3 yolo_conv_fwd reads (the LPD head); columns != 0: y (N,1,W,H*Cp), y[n][0][w][h*Cp + c] -- a
 * (H,1) convolution without padding (the OCR head, OCR/OCR.py:63) is then a 1x1 yolo_conv_fwd with Cin = H*Cp. */
int yolo_dense_bn_relu(const void* x, const float* scale, const float* bias, void* y, int N, int H, int W, int C, int Cs, int Cp,
                       int columns, int dtype, void* stream);
/* ---- DenseNet bodies, train-mode forward (csrc/dense_train.hip) --------------------------------------------------------------------
 * BatchNorm with the BATCH's statistics.  The four entries above are launched unchanged with (scale, bias) pairs folded from batch
 * statistics, so train and eval mode share their arithmetic; the entries here measure the statistics and fold them.  A block's feature
 * map is one buffer, a channel's mean and variance are fixed once it is written: every BN1 of a block folds the SAME per-channel
 * statistics with its own gamma and beta.  Only BN2's statistics (of the bottleneck m, never stored) and the stem's (of the raw 7x7
 * output) are recomputed.  No backward, no optimiser.
 * Every statistic is the mean and the BIASED variance over all pixels.  Reductions are deterministic: a block adds its values in double
 * in a fixed order and writes ONE partial row to `workspace`, a finishing launch of one block adds the rows in a fixed order (double),
 * var = max(Q / P - mean^2, 0) in double.  No atomics.  workspace: yolo_dense_stats_workspace_bytes(channels) bytes, 8-byte aligned,
 * channels = the number of channels the call measures; it needs NO zeroing and is left dirty (every row read was written by the same call).
 * A statistics entry makes two launches (partial rows, finish).  fold != NULL: the finishing launch also folds ONE BatchNorm of fold->C
 * channels from mean[0, C) / var[0, C) -- AFTER writing its own slice of them, so the BatchNorm may span channels measured by earlier
 * calls -- with yolo_fold_bn's arithmetic and padded layout (scale = gamma / sqrtf(var + eps), bias = beta - mean * scale, zeros up to
 * yolo_padded_channels(C)), and, where running_mean / running_var are given (both or neither), updates running = momentum * running +
 * (1 - momentum) * batch; running_var takes the biased variance, as yolo_bn_train_fwd states for Gluon.  0 <= momentum <= 1, eps > 0.
 * Validation as above: YOLO_EINVAL for a NULL pointer (fold may be NULL), a non-positive size, an unknown dtype or a malformed fold;
 * YOLO_EUNSUPPORTED for a shape outside the limits and a buffer of 2^31 bytes or more; nothing is launched on refusal. */
#define YOLO_DENSE_STATS_ROWS 256
typedef struct yolo_bn_batch_fold {
    const float* gamma; const float* beta;          /* C floats each */
    float* running_mean; float* running_var;        /* C floats each, or both NULL */
    float* scale; float* bias;                      /* yolo_padded_channels(C) floats each */
    int C; float eps; float momentum;
} yolo_bn_batch_fold;
long long yolo_dense_stats_workspace_bytes(int channels);
/* The fold alone (one launch): mean, var hold fold->C floats. */
int yolo_dense_bn_batch_fold(const float* mean, const float* var, const yolo_bn_batch_fold* fold, void* stream);
/* mean[0, Cm), var[0, Cm) of m = W1 a over the N*H*W pixels, a = round_dtype(max(0, x scale1 + bias1)) over channels [0, Cin) of the block
 * buffer: m is formed exactly as stage 1 of yolo_dense_layer_fwd forms it (the same operand image, channels >= Cin masked by a select, one
 * rounding, the same MFMA chain into fp32 accumulators) and is reduced from the accumulators without being stored.  fold: BN2 (C == Cm).
 * Supported: Cm % 16 == 0, Cm <= 128, Cin >= 8, Cin <= Cs, Cs % 32 == 0, any H, W >= 1.  buf is only read. */
int yolo_dense_bottleneck_stats(const void* buf, const void* w1_image, const float* scale1, const float* bias1, float* mean, float* var,
                                void* workspace, const yolo_bn_batch_fold* fold, int N, int H, int W, int Cs, int Cin, int Cm, int dtype,
                                void* stream);
/* mean[c0, c0 + n), var[c0, c0 + n) of channels [c0, c0 + n) of an (N,H,W,Cs) buffer, of the values AS STORED (what the next layer reads).
 * Any c0 >= 0, n >= 1 with c0 + n <= Cs.  No byte of buf and nothing outside [c0, c0 + n) of mean / var is written.  fold: any BatchNorm
 * over channels [0, C) of the same mean / var arrays (the next layer's BN1, a transition's or the final BN). */
int yolo_dense_channel_stats(const void* buf, float* mean, float* var, void* workspace, const yolo_bn_batch_fold* fold, int N, int H, int W,
                             int Cs, int c0, int n, int dtype, void* stream);
/* mean[0, F0), var[0, F0) of the stem's raw Conv 7x7 s2 p3 output (fp32, before BN) over N*Hc*Wc: per output value the products and the
 * order of accumulation are yolo_dense_stem_fwd's, so that entry run with the folded pair normalises what was measured.  fold: the stem's
 * BN (C == F0).  F0 % 8 == 0, F0 <= 64. */
int yolo_dense_stem_stats(const float* x_nchw, const float* w_oihw, float* mean, float* var, void* workspace, const yolo_bn_batch_fold* fold,
                          int N, int H, int W, int F0, void* stream);

/* OCR.predict / valid's reading rule (OCR/OCR.py:180-201) on the device (csrc/ocr.hip): logits (N,Wp,1+ncls) float32 ->
 * score (N,Wp) = 1 / (1 + expf(-logit 0)); column i is a PEAK iff s[i] > thr && s[i] > s[i+1] && s[i] > s[i-1] with s[-1] = s[Wp] = 0;
 * codes (N,Wp) = at a peak the first maximum of the ncls class logits (np.argmax of their softmax), -1 elsewhere; count (N) = peaks.
 * thr: 0.6 in predict, 0.2 in valid.  valid (N) bytes or NULL: a row with valid == 0 has no peaks (its scores are still written). */
int yolo_ocr_decode(const float* logits, const unsigned char* valid, float* score, int* codes, int* count, int N, int Wp, int ncls,
                    float thr, void* stream);

/* ---- OCR data, targets, losses and validation counts (csrc/ocr_data.hip) ---------------------------------------------------------
 * Every entry validates before it launches: YOLO_EINVAL for a NULL pointer (where NULL is not stated to be allowed), a non-positive
 * size or a misaligned pointer, YOLO_EUNSUPPORTED for a shape outside the stated limits.  Nothing is written on refusal.
 *
 * LPGenerator.render (yolo_modules/licence_plate_render/__init__.py:168-214) with the PIXELS made on the device: the OCR batch, a
 * plate resized, sheared, rotated, blurred by a wide Gaussian, noised, colour-jittered and pasted onto a background.  The host decides
 * (yolo_amd/render.py LPGenerator.draw_ocr_params) and hands over, per image, one row of YOLO_PLATE_ROW_WORDS words with the meaning
 * yolo_plate_render gives them -- words 16..24 carry the AFFINE map (resize, shear, rotate and paste composed on the host; m6 = m7 = 0,
 * m8 = 1), words 8..11 the paste rectangle (what PIL's tmp.paste covers; clipped to the canvas here whatever the row holds), words 25
 * and 26 are unused -- and one row of YOLO_OCR_TAP_WORDS words for the blur: word 0 T (int, taps per side, limited to
 * 0..YOLO_OCR_BLUR_TAPS here), words 1..T+1 the float32 weights w[0..T], w[0] the centre; the host normalises them to
 * w[0] + 2 (w[1] + .. + w[T]) = 1.  T = 0: no blur, the weights are not read.  The plates are yolo_plate_compose's, unchanged.
 * rows 8-byte, taps 4-byte, workspace 16-byte aligned, all ON THE DEVICE; bg (N,3,H,W) f32, out the same shape, dense.
 * The arithmetic, every operation in fp32, in this order, nothing fused (this is the definition; tests/ocr_render_ref.py restates it):
 *  S(j, i): yolo_plate_render's sample through m at the integer position (column j, row i), inside or outside the canvas.
 *  Inside the window  Hs(j, i') = sum over k = -T..T in ascending order of w[|k|] * S(j + k, i')   (the first term starts the sum)
 *                     P(j, i)   = sum over k = -T..T in ascending order of w[|k|] * Hs(j, i + k);  T = 0: P = S.
 *   The taps reach S outside the window and outside the canvas.  Outside the window P = 0 and nothing is sampled.
 *  Q(j, i) inside the window: s == 0: Q = P; otherwise yolo_plate_render's Philox / Irwin-Hall rule with the same key and counters
 *   (j, i, h, 0) on all four channels.  Outside the window Q = 0: the reference noises the plate image before it pastes it.
 *  yolo_ocr_plate_blur writes Q of the window's pixels to the workspace, and per 32 x 32 tile of the canvas (row-major tile index)
 *   the sum of Q_c, c of R, G, B, over the tile's window pixels, each converted to double and added in double in a fixed order; a
 *   tile outside the window, and every tile of a "no plate" image (yolo_plate_compose's rule), gets 0.  No atomics.  Workspace
 *   layout (yolo_ocr_plate_workspace_bytes(N, H, W) bytes, caller-owned): N * tiles * 3 doubles, padding to a multiple of 16 bytes,
 *   then (N,H,W,4) float32 Q of which only window pixels of images with a plate are written; no other byte is touched.
 *  yolo_ocr_plate_render: sum_c = the image's tile sums added in index order (double);  mu_c = (float)(sum_c / (double)(H*W)) -- the
 *   mean over the WHOLE canvas, Q = 0 outside the window;  k_c = ((D[c][0]*mu_0 + D[c][1]*mu_1) + D[c][2]*mu_2) + e_c;  per pixel
 *   of the window   fg_c = (((A[c][0]*Q_0 + A[c][1]*Q_1) + A[c][2]*Q_2) + k_c) / 255.f;   mask = Q_3 / 255.f
 *   out_c = min(max((bg_c * (1.f - mask)) / 255.f + fg_c * mask, 0), 1)                    (__init__.py:211; bg 0..255)
 *   bg_unit != 0 (bg already 0..1): the division by 255 of the first term is dropped.
 *  A pixel outside the window, and every pixel of a no-plate image: out_c = min(max(bg_c / 255.f, 0), 1) (bg_unit: of bg_c).
 *  out may alias bg: each thread reads its pixels before it writes them.
 * YOLO_EUNSUPPORTED: H * ceil(W / 4) beyond 2^31, more than 65535 tile rows.  16-byte bg loads and plane stores when W % 4 == 0 and
 * bg, out are 16-byte aligned, scalar ones otherwise.
 * Stream order: yolo_plate_compose, yolo_ocr_plate_blur, yolo_ocr_plate_render on the same rows and workspace. */
#define YOLO_OCR_BLUR_TAPS 24
#define YOLO_OCR_TAP_WORDS 32
long long yolo_ocr_plate_workspace_bytes(int N, int H, int W);
int yolo_ocr_plate_blur(const unsigned char* plates, const void* rows, const void* taps, void* workspace, int N, int H, int W,
                        void* stream);
int yolo_ocr_plate_render(const float* bg, const void* rows, const void* workspace, float* out, int N, int H, int W, int bg_unit,
                          void* stream);
/* loss_mask (OCR/OCR.py:77-100): labels (B,nobj,3) f32 [class, left, right] as fractions of the width, class < 0 (or NaN): no object;
 * order (B,nobj) int32 or NULL: the host's draw of nd.random.shuffle -- the labels of an image are visited as order[b][0], order[b][1],
 * ... (an entry outside 0..nobj-1 is passed over), NULL: in the given order.  score_y (B,Wp) f32, 0 where no label covers; class_y
 * (B,Wp) int32, -1 where no label covers.  For each label in that order, in fp32:
 *   left = round-half-away(L1 * Wp), right = round-half-away(L2 * Wp)        (limited to +-2^30)
 *   for columns i in [max(left, 0), min(right, Wp)):  score_y = 1 - |(i + 0.5) / Wp - (L1 + L2) / 2| / (L2 - L1),  class_y = (int)class
 * and a later label overwrites an earlier one: one thread per (image, column) keeps the last label that covers it.  Columns outside
 * [0, Wp) are DROPPED (the reference's container wraps a negative index to the far end and raises on one >= Wp: accidents).
 * YOLO_EUNSUPPORTED: B * Wp or B * nobj * 3 of 2^31 or more. */
int yolo_ocr_targets(const float* labels, const int* order, float* score_y, int* class_y, int B, int nobj, int Wp, void* stream);
/* The two losses of train_the (OCR/OCR.py:113-114, 264-265) and their gradient at the logits: logits (B,Wp,1+ncls) f32 as OCRNet.logits
 * returns them, z = column i's score logit, c_i its ncls class logits, y_i = score_y, k_i = min(max(class_y_i, 0), ncls - 1) (pick's
 * clip mode); losses (2,B) f32:
 *   losses[0][b] = score_w * mean_i( max(z, 0) - z * y + log1p(exp(-|z|)) )             LogisticLoss(label_format='binary')
 *   losses[1][b] = class_w * mean_i( y_i * (logsumexp(c_i) - c_i[k_i]) )                SoftmaxCrossEntropyLoss, sample weight score_y
 * (the reference: score_w = 0.1, class_w = 1.0).  logsumexp(c) = max c + log(sum exp(c - max c)): finite for logits of +-100.  Per
 * column the class terms are summed over a 64-lane butterfly, the columns of an image as four interleaved partial sums (column i in
 * sum i % 4, in column order) added in index order.  dlogits: the same shape as logits or NULL; the gradient of sum(losses), NOT
 * divided by the batch (yolo_loss_fwd_bwd's convention): score_w / Wp * (sigmoid(z) - y) and class_w / Wp * y * (softmax(c) - onehot(k)).
 * YOLO_EUNSUPPORTED: logits of 2^31 bytes or more. */
int yolo_ocr_loss_fwd_bwd(const float* logits, const float* score_y, const int* class_y, float* dlogits, float* losses, int B, int Wp,
                          int ncls, float score_w, float class_w, void* stream);
/* The counts of a validation step (OCR/OCR.py:301-343 reads the peaks and prints the text; this compares it with the labels): codes
 * (B,Wp) and count (B) as yolo_ocr_decode wrote them, labels (B,nobj,3), class_y (B,Wp) from yolo_ocr_targets, logits (B,Wp,1+ncls);
 * counts (B, YOLO_OCR_SCORE_WORDS) int32 per image:
 *   0 truth length: the labels with class >= 0 whose centre (L1 + L2) / 2 lies in [0, 1), read left to right (by centre; ties in label order)
 *   1 predicted length: the first count[b] non-negative codes in column order      2 the Levenshtein distance between the two texts
 *   3 exact match (0 / 1)      4 labelled columns (class_y >= 0)      5 those whose first maximum of the class logits equals class_y
 * One thread per image.  YOLO_EUNSUPPORTED: nobj > YOLO_OCR_SCORE_MAX_NOBJ, Wp > YOLO_OCR_SCORE_MAX_WP, logits of 2^31 bytes or more. */
#define YOLO_OCR_SCORE_WORDS 6
#define YOLO_OCR_SCORE_MAX_NOBJ 16
#define YOLO_OCR_SCORE_MAX_WP 64
int yolo_ocr_score(const int* codes, const int* count, const float* labels, const int* class_y, const float* logits, int* counts, int B,
                   int nobj, int Wp, int ncls, void* stream);

#ifdef __cplusplus
}
#endif
#endif
