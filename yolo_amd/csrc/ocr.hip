// The reading end of the reference's OCR node: OCR.predict / OCR.valid (OCR/OCR.py:180-201) pick the plate text from the score
// columns of OCRDenseNet's output -- a sigmoid, a strict local-maximum rule along the plate, and the argmax of the class scores at
// each peak.  Here the logits are still on the device, so the rule runs there: one block per plate, no atomics.
#include "common.h"

__global__ __launch_bounds__(256) void ocr_decode_kernel(const float* logits, float* score, int* codes, int* count,
                                                         const unsigned char* valid, int Wp, int ncls, float thr) {
    const int n = blockIdx.x, C = 1 + ncls;
    const float* row = logits + (long long)n * Wp * C;
    const bool live = !valid || valid[n] != 0;
    int total = 0;
    for (int base = 0; base < Wp; base += 256) {                       // (uniform trip count: every thread reaches the barrier)
        const int i = base + threadIdx.x;
        int peak = 0;
        if (i < Wp) {
            const float s = 1.f / (1.f + expf(-row[(long long)i * C]));
            const float sl = i > 0 ? 1.f / (1.f + expf(-row[(long long)(i - 1) * C])) : 0.f;
            const float sr = i + 1 < Wp ? 1.f / (1.f + expf(-row[(long long)(i + 1) * C])) : 0.f;
            peak = live && s > thr && s > sr && s > sl;
            int code = -1;
            if (peak) {
                const float* cl = row + (long long)i * C + 1;
                float best = cl[0];
                code = 0;
                for (int k = 1; k < ncls; ++k)
                    if (cl[k] > best) { best = cl[k]; code = k; }       // the first maximum: np.argmax
            }
            score[(long long)n * Wp + i] = s;
            codes[(long long)n * Wp + i] = code;
        }
        total += __syncthreads_count(peak);
    }
    if (threadIdx.x == 0) count[n] = total;
}

extern "C" int yolo_ocr_decode(const float* logits, const unsigned char* valid, float* score, int* codes, int* count, int N, int Wp,
                               int ncls, float thr, void* stream) {
    if (!logits || !score || !codes || !count) return YOLO_EINVAL;
    if (N <= 0 || Wp <= 0 || ncls <= 0) return YOLO_EINVAL;
    if ((long long)N * Wp * (1 + ncls) * (long long)sizeof(float) >= (1LL << 31)) return YOLO_EUNSUPPORTED;      // logits of 2^31 bytes or more
    YOLO_LAUNCH(ocr_decode_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, logits, score, codes, count, valid, Wp, ncls, thr);
    YOLO_LAUNCH_CHECK();
    return YOLO_OK;
}
