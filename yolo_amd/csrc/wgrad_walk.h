// What wgrad_walk.hip offers to the weight-gradient entry points of wgrad.hip.  Both return YOLO_EUNSUPPORTED for a shape outside
// their domain (the caller then takes the register-staged kernels of wgrad.hip).
#pragma once
#include "common.h"

// the pipelined row-walk kernel of the 3x3 stride-1 layers (Cin, Cout multiples of 64); adds into dwt = dW as OIHW
int wgrad_walk_dispatch(const void* dy, const void* x, float* dwt, int N, int H, int W, int Cin, int Cout, long long ps,
                        int variant, hipStream_t st);
// the LDS-DMA GEMM of the 1x1 layers (Cin, Cout multiples of 128)
int wgrad_gemm_dispatch(const void* dy, const void* x, float* dw, long long P, int Cin, int Cout, long long ps, int variant,
                        hipStream_t st);
