// Split-operand GEMM of libjegal_hip (gemm_x3.hip), on the timed path: the fp16 contract modes run the ends of the JEGAL branches on it
// (option jegal_fp32_ends):
//   out[m][n] = act( sum_k A[m][k] * W[n][k] + bias[n] + res[m % res_mod][n] ),   A fp32, W = Wh + Wl (fp16 pair), out fp32,
// with A split into hi + lo fp16 IN THE LOADER and three MFMAs per fragment pair (Ah Wh + Ah Wl + Al Wh; the dropped Al Wl term is 2^-22
// of the product): fp32-grade products at 3/16 of the cost of the fp32 MFMA.  K % 256 == 0, N % 128 == 0, lda % 4 == 0.
#pragma once
#include "common.h"

struct GemmX3Args {
    const float* A;
    long lda;
    const f16* Wh;
    const f16* Wl;
    long ldw;
    int M, N, K;
    const float* bias;
    const float* res;
    long ldr;
    int res_mod;
    float* out;
    long ldc;
    int relu;
};
hipError_t launch_gemm_x3(const GemmX3Args& a, hipStream_t s);
