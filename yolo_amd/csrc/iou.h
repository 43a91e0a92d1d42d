// The two IoU definitions of the library as device functions, shared by detect.hip (get_iou, NMS) and eval.hip (evaluation).
// Units that include this are built with -ffp-contract=off (csrc/Makefile FP_EXACT): every operation below is one fp32 rounding.
#pragma once
#include <hip/hip_runtime.h>

// IoU of two ltrb boxes, max(0, .) intersections, no +1; 0 where the union is not positive (or NaN).
__device__ __forceinline__ float box_iou(const float4 a, const float4 b) {
    const float iw = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
    const float ih = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
    const float inter = iw * ih;
    const float ua = (a.z - a.x) * (a.w - a.y) + (b.z - b.x) * (b.w - b.y) - inter;
    return ua > 0.f ? inter / ua : 0.f;
}

// get_iou(predict, target, mode), yolo_gluon.py:127-168: p = one ltrb box, target = [c, t1, t2, t3, t4].
// MODE 2: target = [c, y, x, h, w] (the hot path: car/YOLO.py:403,525).  MODE 1 (the reference's default): target =
// [c, l, t, r, b] -- including its target_area = target[3] * target[4] (yolo_gluon.py:166), i.e. r2 * b2 in this mode.
// The quotient is the reference's undivided inter / (pa + ta - inter): no guard against an empty union.
template <int MODE>
__device__ __forceinline__ float get_iou_ref(const float4 p, float t1, float t2_, float t3, float t4) {
    float l2, t2, r2, b2;
    if (MODE == 1) { l2 = t1; t2 = t2_; r2 = t3; b2 = t4; }
    else { l2 = t2_ - t4 / 2.f; t2 = t1 - t3 / 2.f; r2 = t2_ + t4 / 2.f; b2 = t1 + t3 / 2.f; }
    const float iw = fmaxf(fminf(r2, p.z) - fmaxf(l2, p.x), 0.f);
    const float ih = fmaxf(fminf(b2, p.w) - fmaxf(t2, p.y), 0.f);
    const float inter = iw * ih;
    const float pa = (p.z - p.x) * (p.w - p.y);
    const float ta = t3 * t4;
    return inter / (pa + ta - inter);
}
