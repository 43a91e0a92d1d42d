// The small kernels of the training step for gfx950: bias gradient, strided row gather, 2x dilation (stride-2 dgrad),
// up-sample/concat backward, gradient fan-in add, MXNet Adam.  One kernel text per operation serves the single-plane types and
// the split type (train_access.h).  Reference: car/YOLO.py:350-498 (_train_batch) + the mxnet/gluon operators it calls
// (SURVEY App. A.5, A.6).
#include "common.h"
#include "train_access.h"

// column sums: db[c] += sum_p dy[p*ps + c]   (bias gradient of YOLOOutput's conv)
// (split: rows of a dense split tensor or of a wider one with the same planes -- the lo plane round_up(C, 32) behind the hi plane)
template <typename T>
__global__ __launch_bounds__(256) void bias_grad_kernel(const T* __restrict__ dy, float* __restrict__ db, int C,
                                                        long long npix, long long ps, int pix_per_block) {
    const long long p0 = (long long)blockIdx.x * pix_per_block;
    const long long p1 = min(p0 + pix_per_block, npix);
    const int lo = dense_lo<T>(C);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float s = 0.f;
        for (long long p = p0; p < p1; ++p) s += load1s<T>(dy + p * ps + c, lo);
        atomicAdd(&db[c], s);
    }
}

extern "C" int yolo_bias_grad(const void* dy, float* db, long long npix, int C, long long pixel_stride, int dtype,
                              void* stream) {
    if (!dy || !db || npix <= 0 || C <= 0) return YOLO_EINVAL;
    const int ppb = 64;
    const unsigned nb = (unsigned)((npix + ppb - 1) / ppb);
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        const long long ps = pixel_stride ? pixel_stride : dense_ps<T>(C);
        if (IsSplit<T>::value && ps < dense_lo<T>(C) + C) return YOLO_EINVAL;     // (a split row holds its lo plane)
        YOLO_LAUNCH(bias_grad_kernel<T>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const T*)dy, db, C, npix, ps, ppb);
        YOLO_LAUNCH_CHECK();
        return YOLO_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// strided copy (rows of C floats, source row stride ps) -> dense (rows, Cpad) of `dtype`, zero padded
// (split: dst rows are dense split rows of Cpad channels, pixel stride 2 * round_up(Cpad, 32); the pad beyond Cpad is not written)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void gather_rows_kernel(const float* __restrict__ src, T* __restrict__ dst, int C, int Cpad,
                                   long long src_batch_stride, long long rows_per_batch, long long ps,
                                   long long total) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % Cpad);
    const long long row = i / Cpad;
    const long long b = row / rows_per_batch, r = row - b * rows_per_batch;
    store1s<T>(dst + dense_at<T>(i, row, c, Cpad), dense_lo<T>(Cpad), c < C ? src[b * src_batch_stride + r * ps + c] : 0.f);
}

extern "C" int yolo_gather_rows(const float* src, void* dst, int B, long long rows_per_batch, int C, int Cpad,
                                long long src_batch_stride, long long src_row_stride, int dtype, void* stream) {
    if (!src || !dst || B <= 0 || rows_per_batch <= 0 || C <= 0 || Cpad < C) return YOLO_EINVAL;
    const long long total = (long long)B * rows_per_batch * Cpad;
    const unsigned nb = (unsigned)((total + 255) / 256);
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        YOLO_LAUNCH(gather_rows_kernel<T>, dim3(nb), dim3(256), 0, (hipStream_t)stream, src, (T*)dst, C, Cpad, src_batch_stride,
                    rows_per_batch, src_row_stride, total);
        YOLO_LAUNCH_CHECK();
        return YOLO_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// 2x zero-dilation (stride-2 dgrad): D[n, 2y, 2x, :] = dy[n, y, x, :], zeros elsewhere; D is (N,H,W,C); C % 8 == 0
// (split: both planes of the C real channels are written, as stored in dy or zero; the pad channels are not)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void dilate2_kernel(const T* __restrict__ dy, T* __restrict__ d, int H, int W, int Ho, int Wo, int C8,
                               long long total8) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int c = (int)(i % C8);
    long long p = i / C8;
    const long long pix = p;
    const int xx = (int)(p % W); p /= W;
    const int yy = (int)(p % H);
    const long long n = p / H;
    const int lo = dense_lo<T>(C8 * 8);
    typename Moved8<T>::type v;
    zero8m(v);
    if (!(yy & 1) && !(xx & 1) && (yy >> 1) < Ho && (xx >> 1) < Wo) {
        const long long sp = (n * Ho + (yy >> 1)) * Wo + (xx >> 1);
        load8m(dy + dense_at<T>((sp * C8 + c) * 8, sp, c * 8, C8 * 8), lo, v);
    }
    store8m(d + dense_at<T>(i * 8, pix, c * 8, C8 * 8), lo, v);
}

extern "C" int yolo_dilate2x(const void* dy, void* d, int N, int H, int W, int Ho, int Wo, int C, int dtype,
                             void* stream) {
    if (!dy || !d || N <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || C <= 0) return YOLO_EINVAL;
    if (2 * Ho - 1 > H || 2 * Wo - 1 > W) return YOLO_EINVAL;     // dy pixel (i, j) lands on (2i, 2j): it must exist in the target
    if (C % 8) return YOLO_EUNSUPPORTED;
    const long long total8 = (long long)N * H * W * (C / 8);
    const unsigned nb = (unsigned)((total8 + 255) / 256);
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        YOLO_LAUNCH(dilate2_kernel<T>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (T*)d, H, W, Ho, Wo, C / 8, total8);
        YOLO_LAUNCH_CHECK();
        return YOLO_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// backward of 2x nearest up-sample + concat: d_up[n,y,x,:] (+)= sum of the 2x2 block of dcat[..., :C1];
// d_route (+)= dcat[..., C1:]
// (split: dense split dcat (C1 + C2 channels), dup (C1) and droute (C2); sums and accumulations in fp32, stored as pairs)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void upcat_bwd_kernel(const T* __restrict__ dcat, T* __restrict__ dup, T* __restrict__ droute, int H, int W,
                                 int C1, int C2, int acc_up, int acc_route, long long total_up, long long total_route) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int C = C1 + C2;
    if (i < total_up) {
        const int c = (int)(i % C1);
        long long p = i / C1;
        const long long pix = p;
        const int xx = (int)(p % (W / 2)); p /= (W / 2);
        const int yy = (int)(p % (H / 2));
        const long long n = p / (H / 2);
        float s = 0.f;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx)
                s += load1s<T>(dcat + ((n * H + 2 * yy + dy) * W + 2 * xx + dx) * dense_ps<T>(C) + c, dense_lo<T>(C));
        T* o = dup + dense_at<T>(i, pix, c, C1);
        const int lo = dense_lo<T>(C1);
        store1s<T>(o, lo, acc_up ? load1s<T>(o, lo) + s : s);
    } else if (i < total_up + total_route) {
        const long long j = i - total_up;
        const int c = (int)(j % C2);
        const long long p = j / C2;
        const float v = load1s<T>(dcat + p * dense_ps<T>(C) + C1 + c, dense_lo<T>(C));
        T* o = droute + dense_at<T>(j, p, c, C2);
        const int lo = dense_lo<T>(C2);
        store1s<T>(o, lo, acc_route ? load1s<T>(o, lo) + v : v);
    }
}

extern "C" int yolo_upsample2x_concat_bwd(const void* dcat, void* dup, void* droute, int N, int H, int W, int C1,
                                          int C2, int accumulate_up, int accumulate_route, int dtype, void* stream) {
    if (!dcat || !dup || !droute || N <= 0 || (H & 1) || (W & 1) || C1 <= 0 || C2 <= 0) return YOLO_EINVAL;
    const long long tu = (long long)N * (H / 2) * (W / 2) * C1, tr = (long long)N * H * W * C2;
    const unsigned nb = (unsigned)((tu + tr + 255) / 256);
    return dispatch_dtype<float, bf16_t, bf16x3_t>(dtype, [&](auto t) {
        using T = decltype(t);
        YOLO_LAUNCH(upcat_bwd_kernel<T>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const T*)dcat, (T*)dup, (T*)droute, H, W, C1,
                    C2, accumulate_up, accumulate_route, tu, tr);
        YOLO_LAUNCH_CHECK();
        return YOLO_OK;
    });
}

// y = a + b (elementwise, gradient fan-in) over `total` = pixels * C values of dense tensors.  A single-plane tensor is its `total`
// elements whatever C is (yolo_add passes 1); a split value's lo plane is round_up(C, 32) behind it, which an element count
// alone cannot locate: yolo_add_split takes the pixel count and C.
template <typename T>
__global__ void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, int C, long long total) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long p = i / C;
    const long long o = dense_at<T>(i, p, (int)(i - p * C), C);
    const int lo = dense_lo<T>(C);
    store1s<T>(y + o, lo, load1s<T>(a + o, lo) + load1s<T>(b + o, lo));
}
template <typename T>
static int add_launch(const void* a, const void* b, void* y, int C, long long total, void* stream) {
    YOLO_LAUNCH(add_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)a, (const T*)b,
                (T*)y, C, total);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
extern "C" int yolo_add(const void* a, const void* b, void* y, long long n, int dtype, void* stream) {
    if (!a || !b || !y || n <= 0) return YOLO_EINVAL;
    return dispatch_dtype<float, bf16_t>(dtype, [&](auto t) { return add_launch<decltype(t)>(a, b, y, 1, n, stream); });
}
extern "C" int yolo_add_split(const void* a, const void* b, void* y, long long npix, int C, int dtype, void* stream) {
    if (!a || !b || !y || npix <= 0 || C <= 0 || dtype != YOLO_BF16X3) return YOLO_EINVAL;
    return add_launch<bf16x3_t>(a, b, y, C, npix * C, stream);
}

// ------------------------------------------------------------------------------------------------
// MXNet Adam: g = rescale*grad; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// w -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)       (epsilon OUTSIDE the bias correction)
// ------------------------------------------------------------------------------------------------
// One element per thread ON PURPOSE: seven streams (four read, three written, 1.7 GB for Darknet-53) -- four elements per thread
// with 16-byte accesses were measured 10 % SLOWER (591 against 539 us on one box, round 3).
__device__ __forceinline__ void adam_one(float& w, float g, float& m, float& v, float lr_t, float b1, float b2, float eps, float rescale) {
    const float gr = g * rescale;
    const float mi = b1 * m + (1.f - b1) * gr;
    const float vi = b2 * v + (1.f - b2) * gr * gr;
    m = mi;
    v = vi;
    w = w - lr_t * mi / (sqrtf(vi) + eps);
}

template <bool DEV>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long long n, float lr_t, float b1, float b2, float eps,
                                                   float rescale_host, const float* __restrict__ gb) {
    // DEV: rescale = 1 / *gb, a float the caller's gradient exchange has just SUM-reduced over the ranks (each rank contributes its
    // shard size in a slot of the last gradient bucket) -- no collective of its own, no host read, no per-rank decision
    const float rescale = DEV ? 1.f / gb[0] : rescale_host;
    const long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (k < n) adam_one(w[k], g[k], m[k], v[k], lr_t, b1, b2, eps, rescale);
}

static int adam_launch(float* w, const float* grad, float* m, float* v, long long n, int t, float lr, float beta1, float beta2,
                       float eps, float rescale, const float* gb, void* stream) {
    const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t)));
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    if (gb) YOLO_LAUNCH(adam_kernel<true>, grid, dim3(256), 0, st, w, grad, m, v, n, lr_t, beta1, beta2, eps, 0.f, gb);
    else    YOLO_LAUNCH(adam_kernel<false>, grid, dim3(256), 0, st, w, grad, m, v, n, lr_t, beta1, beta2, eps, rescale, (const float*)nullptr);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

extern "C" int yolo_adam_step_dev(float* w, const float* grad, float* m, float* v, long long n, int t, float lr,
                                  float beta1, float beta2, float eps, const float* global_batch_dev, void* stream) {
    if (!w || !grad || !m || !v || !global_batch_dev || n <= 0 || t < 1) return YOLO_EINVAL;
    return adam_launch(w, grad, m, v, n, t, lr, beta1, beta2, eps, 0.f, global_batch_dev, stream);
}

extern "C" int yolo_adam_step(float* w, const float* grad, float* m, float* v, long long n, int t, float lr,
                              float beta1, float beta2, float eps, float rescale, void* stream) {
    if (!w || !grad || !m || !v || n <= 0 || t < 1) return YOLO_EINVAL;
    return adam_launch(w, grad, m, v, n, t, lr, beta1, beta2, eps, rescale, nullptr, stream);
}
