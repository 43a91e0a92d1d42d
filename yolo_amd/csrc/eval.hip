// Detection-quality evaluation for gfx950: matching of ranked detections to ground truth (PASCAL-VOC devkit semantics) and the
// reference's top-1 mean-IoU / azimuth arithmetic (car/YOLO.py:501-534 _valid_iou; yolo_cv.py:85-95 RadarProb.cls2ang).
// Compiled with -ffp-contract=off like detect.hip: the IoUs are bit-identical to the oracle's op-by-op fp32 evaluation.
// No global atomic anywhere: every output slot has exactly one writer, so results are reproducible run to run.
#include "common.h"
#include "iou.h"
#include <float.h>

constexpr int EVAL_MAX_OBJ = 512;       // ground truths per image staged in LDS
constexpr int EVAL_MAX_DET = 1024;      // kept detections per image (post_nms)
constexpr int EVAL_THREADS = 256;

// ---- yolo_eval_match ---------------------------------------------------------------------------
// One block per image.
//   1. the image's labels -> LDS as ltrb + class (-1: no object); gt_class written out.
//   2. every detection, independently: the eligible ground truth with the largest box_iou (first index among equals).
//   3. a detection whose IoU is above the threshold claims its ground truth: LDS atomicMin of the detection's rank per ground
//      truth -- the smallest rank (= highest score) wins, every later detection of that ground truth is a false positive.
__global__ __launch_bounds__(EVAL_THREADS) void eval_match_kernel(const float* __restrict__ rows, const int* __restrict__ kept,
                                                                  const int* __restrict__ kept_count,
                                                                  const float* __restrict__ labels, int nbox, int C, int cpb,
                                                                  int post_nms, int nobj, int label_cols, int class_aware,
                                                                  float iou_thresh, int* __restrict__ det_class,
                                                                  int* __restrict__ det_tp, int* __restrict__ det_gt,
                                                                  float* __restrict__ det_iou, int* __restrict__ gt_class) {
    __shared__ float4 gbox[EVAL_MAX_OBJ];
    __shared__ int gcls[EVAL_MAX_OBJ];
    __shared__ int claim[EVAL_MAX_OBJ];                  // lowest detection rank that matched this ground truth
    __shared__ int dgt[EVAL_MAX_DET];
    __shared__ float diou[EVAL_MAX_DET];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* lab = labels + (long long)b * nobj * label_cols;
    for (int g = tid; g < nobj; g += EVAL_THREADS) {
        const float* p = lab + (long long)g * label_cols;
        const float c = p[0], y = p[1], x = p[2], h = p[3], w = p[4];
        const int cls = c >= 0.f ? (class_aware ? (int)c : 0) : -1;           // (a NaN class is no object)
        gbox[g] = make_float4(x - w / 2.f, y - h / 2.f, x + w / 2.f, y + h / 2.f);
        gcls[g] = cls;
        claim[g] = 0x7fffffff;
        gt_class[(long long)b * nobj + g] = cls;
    }
    __syncthreads();
    int n = kept_count[b];
    n = n < 0 ? 0 : (n > post_nms ? post_nms : n);
    const long long ncand = (long long)nbox * cpb;
    const int* kp = kept + (long long)b * post_nms;
    const float* rw = rows + (long long)b * nbox * C;
    for (int d = tid; d < post_nms; d += EVAL_THREADS) {
        int best = -1;
        float biou = 0.f;
        const int id = d < n ? kp[d] : -1;
        if (id >= 0 && id < ncand) {
            const float* p = rw + (long long)(id / cpb) * C + 1;
            const float4 box = make_float4(p[0], p[1], p[2], p[3]);
            const int cls = class_aware ? id % cpb : 0;
            float top = -FLT_MAX;
            for (int g = 0; g < nobj; ++g) {
                if (gcls[g] < 0 || gcls[g] != cls) continue;
                const float v = box_iou(box, gbox[g]);
                if (v > top) { top = v; best = g; }      // strict: the first of equal IoUs stays; a NaN is never larger
            }
            if (best >= 0) biou = top;
            if (best >= 0 && biou > iou_thresh) atomicMin(&claim[best], d);
            det_class[(long long)b * post_nms + d] = cls;
        } else {
            det_class[(long long)b * post_nms + d] = -1;                        // pad slot / id out of range: nothing is read
            best = -2;
        }
        dgt[d] = best;
        diou[d] = biou;
    }
    __syncthreads();
    for (int d = tid; d < post_nms; d += EVAL_THREADS) {
        const int best = dgt[d];
        const float v = diou[d];
        const long long o = (long long)b * post_nms + d;
        if (best == -2) {
            det_tp[o] = -1; det_gt[o] = -1; det_iou[o] = 0.f;
        } else {
            det_tp[o] = (best >= 0 && v > iou_thresh && claim[best] == d) ? 1 : 0;
            det_gt[o] = best;
            det_iou[o] = v;
        }
    }
}

extern "C" int yolo_eval_match_supported(int nobj, int post_nms) {
    if (nobj <= 0 || post_nms <= 0) return YOLO_EINVAL;
    return (nobj <= EVAL_MAX_OBJ && post_nms <= EVAL_MAX_DET) ? 1 : 0;
}

extern "C" int yolo_eval_match(const float* rows, const int* kept, const int* kept_count, const float* labels, int B, int nbox,
                               int C, int cand_per_box, int post_nms, int nobj, int label_cols, int class_aware,
                               float iou_thresh, int* det_class, int* det_tp, int* det_gt, float* det_iou, int* gt_class,
                               void* stream) {
    if (!rows || !kept || !kept_count || !labels || !det_class || !det_tp || !det_gt || !det_iou || !gt_class) return YOLO_EINVAL;
    if (B <= 0 || nbox <= 0 || C < 5 || cand_per_box < 1 || post_nms < 1 || nobj < 1 || label_cols < 5) return YOLO_EINVAL;
    if (class_aware != 0 && class_aware != 1) return YOLO_EINVAL;
    if ((long long)nbox * cand_per_box > 0x7fffffffLL) return YOLO_EUNSUPPORTED;
    if (nobj > EVAL_MAX_OBJ || post_nms > EVAL_MAX_DET) return YOLO_EUNSUPPORTED;
    YOLO_LAUNCH(eval_match_kernel, dim3(B), dim3(EVAL_THREADS), 0, (hipStream_t)stream, rows, kept, kept_count, labels, nbox, C,
                cand_per_box, post_nms, nobj, label_cols, class_aware, iou_thresh, det_class, det_tp, det_gt, det_iou, gt_class);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// ---- yolo_eval_top1 ----------------------------------------------------------------------------
// RadarProb.cls2ang's sums (yolo_cv.py:85-94): p = softmax(cls logits), (cs, sn) = (sum cos_c p_c, sum sin_c p_c).  The one place
// this arithmetic lives: eval_top1_kernel and pose_top1_kernel return the same bits for the same row.
__device__ __forceinline__ void top1_direction(const float* cl, int ncls, const float* __restrict__ class_dirs, float& cs, float& sn) {
    float m = -FLT_MAX;
    for (int c = 0; c < ncls; ++c) m = fmaxf(m, cl[c]);
    float sum = 0.f;
    for (int c = 0; c < ncls; ++c) sum += expf(cl[c] - m);
    cs = 0.f;
    sn = 0.f;
    for (int c = 0; c < ncls; ++c) {
        const float pc = expf(cl[c] - m) / sum;
        cs += class_dirs[2 * c] * pc;
        sn += class_dirs[2 * c + 1] * pc;
    }
}

// One thread per image: pred row [score, y, x, h, w, rot, cls...] against object 0 of the image's labels.
//   iou      get_iou(mode 2) of the box rebuilt as car/YOLO.py:518-521 rebuilds it (l = x - w/2, t = y - h/2, r = x + w/2, b = y + h/2)
//   azimuth  atan2(sum sin_c p_c, sum cos_c p_c), p = softmax(cls logits): RadarProb.cls2ang, yolo_cv.py:85-95
//   radius   score * |(sum cos_c p_c, sum sin_c p_c)|
//   valid    label class >= 0 (an image without an object is left out of the mean; the reference scores it against a box of -1s)
__global__ __launch_bounds__(64) void eval_top1_kernel(const float* __restrict__ pred, const float* __restrict__ labels,
                                                       const float* __restrict__ class_dirs, float* __restrict__ out, int B, int C,
                                                       long long label_stride) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = pred + (long long)b * C;
    const float* t = labels + (long long)b * label_stride;
    const float y = p[1], x = p[2], h = p[3], w = p[4];
    const float4 box = make_float4(x - w / 2.f, y - h / 2.f, x + w / 2.f, y + h / 2.f);
    const float iou = get_iou_ref<2>(box, t[1], t[2], t[3], t[4]);
    float cs, sn;
    top1_direction(p + 6, C - 6, class_dirs, cs, sn);
    float4 o;
    o.x = iou;
    o.y = atan2f(sn, cs);
    o.z = p[0] * sqrtf(sn * sn + cs * cs);
    o.w = t[0] >= 0.f ? 1.f : 0.f;
    reinterpret_cast<float4*>(out)[b] = o;
}

extern "C" int yolo_eval_top1(const float* pred, const float* labels, const float* class_dirs, float* out, int B, int C, int nobj,
                              int label_cols, void* stream) {
    if (!pred || !labels || !class_dirs || !out) return YOLO_EINVAL;
    if (B <= 0 || C <= 6 || nobj < 1 || label_cols < 5) return YOLO_EINVAL;
    if ((reinterpret_cast<unsigned long long>(out) & 15ull) != 0) return YOLO_EINVAL;      // 16-byte rows
    YOLO_LAUNCH(eval_top1_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred, labels, class_dirs, out, B, C,
                (long long)nobj * label_cols);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}

// ---- yolo_pose_top1 ----------------------------------------------------------------------------
// The row Video.process publishes (car/video_node.py:235-255, car_and_LP/carLP_video_node.py:48-72), one thread per image:
//   azimuth, radius   eval_top1_kernel's, through top1_direction
//   class             the index of the largest class logit (strictly larger wins: the lowest index among equals, never a NaN)
//   depth             depth[b][(int)(Hd y)][(int)(Wd x)] (:239-241), -1 without a depth image (:243) or where the index leaves it
// rows_out may be pred itself: a thread has read its whole row (the logits above, column j just before it is stored) when it writes.
__global__ __launch_bounds__(64) void pose_top1_kernel(const float* pred, const float* __restrict__ class_dirs,
                                                       const float* __restrict__ depth, float* rows_out, float* __restrict__ pose,
                                                       int B, int C, int Hd, int Wd, int row5) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = pred + (long long)b * C;
    const int ncls = C - 6;
    float cs, sn;
    top1_direction(p + 6, ncls, class_dirs, cs, sn);
    const float azimuth = atan2f(sn, cs);
    const float radius = p[0] * sqrtf(sn * sn + cs * cs);
    int cls = 0;
    float top = -INFINITY;
    for (int c = 0; c < ncls; ++c) {
        const float v = p[6 + c];
        if (v > top) { top = v; cls = c; }
    }
    float dep = -1.f;
    if (depth) {
        const double dx = (double)Wd * (double)p[2], dy = (double)Hd * (double)p[1];
        // (false for a NaN or an infinity; the truncation toward zero makes (-1, 0) index 0)
        if (dx > -1.0 && dx < (double)Wd && dy > -1.0 && dy < (double)Hd)
            dep = depth[((long long)b * Hd + (int)dy) * Wd + (int)dx];
    }
    float4 o;
    o.x = azimuth;
    o.y = radius;
    o.z = dep;
    o.w = (float)cls;
    if (rows_out) {
        float* q = rows_out + (long long)b * C;
        const float five = row5 == 1 ? azimuth : dep;
        for (int j = 0; j < C; ++j) {
            const float v = p[j];
            q[j] = (j == 5 && row5 != 0) ? five : v;
        }
    }
    reinterpret_cast<float4*>(pose)[b] = o;
}

extern "C" int yolo_pose_top1(const float* pred, int B, int C, const float* class_dirs, const float* depth, int Hd, int Wd, int row5,
                              float* rows_out, float* pose, void* stream) {
    if (!pred || !class_dirs || !pose) return YOLO_EINVAL;
    if (B <= 0 || C <= 6 || row5 < 0 || row5 > 2) return YOLO_EINVAL;
    if (depth && (Hd < 1 || Wd < 1)) return YOLO_EINVAL;
    if ((reinterpret_cast<unsigned long long>(pose) & 15ull) != 0) return YOLO_EINVAL;     // 16-byte rows
    YOLO_LAUNCH(pose_top1_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred, class_dirs, depth, rows_out, pose, B, C,
                Hd, Wd, row5);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
