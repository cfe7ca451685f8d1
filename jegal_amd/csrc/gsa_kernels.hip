// Kernels of GestSync's audio stream (gfx950) that are not GEMMs: conv1 + BatchNorm + ReLU + max-pool from the mel windows, and the
// (2, 3) / stride (2, 2) max-pool in front of fc6.  Compiled once: no bf16 handle reaches them (jg_gestsync_audio_* refuse it), and the
// output type (fp16 for the 16-bit graph, fp32 for the audit graph) is a template argument.  Launchers: shared.h.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// conv1 (1 -> 64 channels, 3x3, stride 2, pad 1) + folded BatchNorm + ReLU + max-pool 3x3 / stride 2 of one 80 x 100 window per
// workgroup: (80, 100) -> conv (40, 50) -> pooled (19, 24), written [19][24][64] NHWC.  The pool never reads conv row 39 or conv
// column 49, so they are not computed -- and mel bands 78, 79 and steps 98, 99 of a window are never read.
//
// The window is staged once in LDS with a zero border above and to the left (the only padding the computed outputs touch), pitch 101
// floats: the time-major form writes it transposed, lane -> band, and 101 is odd.  A thread then owns ONE pooled position: the 7 x 7
// input patch under its 3 x 3 conv outputs sits in registers and is reused for all 64 channels, whose weights are wave-uniform and come
// through the scalar cache.  (Lane -> channel, the obvious NHWC mapping, reads LDS once per FMA: four waves' broadcast reads are four
// times what the LDS delivers per FMA issue slot.)  A position's 64 channels leave as eight (fp16) or sixteen (fp32) 16-byte stores
// that fill its own 128 / 256-byte row.
// Arithmetic: fp32 throughout; a conv output is the fmaf chain over the taps (kh, kw) in row-major order from 0, then + shift; weights
// w[c][kh * 3 + kw] carry the BatchNorm scale.  ReLU after the max (they commute).
//
// Two input forms, one body:
//   windows: src = x (N, 1, 80, 100), window n = block, value (band h, step w) = x[n][h][w]
//   clip:    src = mel (B, Tm, 80) time-major, window n = b * T + t reads mel row clamp(4 (t - 12) + w, 0, valid[b] - 1) of clip b:
//            the audio twin of the video path's +-12 frame edge pad by index clamping
constexpr int GSA_H = 80, GSA_W = 100, GSA_PITCH = 101;
constexpr int GSA_PH = 19, GSA_PW = 24, GSA_C = 64;

template <class OT>
__global__ __launch_bounds__(256) void gsa_conv1_pool_kernel(const float* __restrict__ src, int clip_form, int n0, int T, int Tm,
                                                             const int* __restrict__ valid, const float* __restrict__ w,
                                                             const float* __restrict__ shift, OT* __restrict__ out) {
    __shared__ float sX[(GSA_H + 1) * GSA_PITCH];
    const int tid = threadIdx.x;
    const long n = (long)n0 + blockIdx.x;
    for (int i = tid; i < GSA_PITCH; i += 256) sX[i] = 0.f;
    for (int i = tid; i <= GSA_H; i += 256) sX[i * GSA_PITCH] = 0.f;
    if (!clip_form) {
        const float* x = src + n * (GSA_H * GSA_W);
        for (int i = tid; i < GSA_H * GSA_W; i += 256) {
            const int hh = i / GSA_W, ww = i - hh * GSA_W;
            sX[(hh + 1) * GSA_PITCH + ww + 1] = x[i];
        }
    } else {
        const int b = (int)(n / T), t = (int)(n - (long)b * T);
        int vt = valid ? valid[b] : Tm;
        vt = vt < 1 ? 1 : (vt > Tm ? Tm : vt);
        const float* m = src + (long)b * Tm * GSA_H;
        const int r0 = 4 * (t - 12);
        for (int i = tid; i < GSA_H * GSA_W; i += 256) {
            const int ww = i / GSA_H, hh = i - ww * GSA_H;
            int row = r0 + ww;
            row = row < 0 ? 0 : (row > vt - 1 ? vt - 1 : row);
            sX[(hh + 1) * GSA_PITCH + ww + 1] = m[(long)row * GSA_H + hh];
        }
    }
    __syncthreads();
    OT* o = out + (long)blockIdx.x * (GSA_PH * GSA_PW * GSA_C);
    constexpr int V = 16 / sizeof(OT);                    // channels per 16-byte store
    typedef OT ovec __attribute__((ext_vector_type(V)));
    for (int p = tid; p < GSA_PH * GSA_PW; p += 256) {
        const int ph = p / GSA_PW, pw = p - ph * GSA_PW;
        float in[7][7];                                   // bordered rows 4 ph .. 4 ph + 6, columns 4 pw .. 4 pw + 6
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int c = 0; c < 7; ++c) in[r][c] = sX[(4 * ph + r) * GSA_PITCH + 4 * pw + c];
        for (int c0 = 0; c0 < GSA_C; c0 += V) {
            ovec v;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float* wc = w + (c0 + e) * 9;
                float mx = -INFINITY;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        float acc = 0.f;
#pragma unroll
                        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                            for (int kw = 0; kw < 3; ++kw) acc = __builtin_fmaf(in[2 * i + kh][2 * j + kw], wc[kh * 3 + kw], acc);
                        mx = fmaxf(mx, acc + shift[c0 + e]);
                    }
                v[e] = (OT)fmaxf(mx, 0.f);
            }
            *reinterpret_cast<ovec*>(o + (long)p * GSA_C + c0) = v;
        }
    }
}

hipError_t launch_gsa_conv1_pool(const float* src, int clip_form, int n0, int nwin, int T, int Tm, const int* valid, const float* w,
                                 const float* shift, void* out, int out32, hipStream_t s) {
    if (nwin <= 0) return hipSuccess;
    if (!src || !w || !shift || !out || n0 < 0 || (clip_form && (T <= 0 || Tm <= 0)) || (reinterpret_cast<uintptr_t>(out) & 15)) return hipErrorInvalidValue;
    const char* const form = clip_form ? "clip" : "windows";
    if (out32) {
        record_kernel("gsa_conv1_pool_kernel<float> %s", form);
        hipLaunchKernelGGL(gsa_conv1_pool_kernel<float>, dim3(nwin), dim3(256), 0, s, src, clip_form, n0, T, Tm, valid, w, shift, static_cast<float*>(out));
    } else {
        record_kernel("gsa_conv1_pool_kernel<f16> %s", form);
        hipLaunchKernelGGL(gsa_conv1_pool_kernel<f16>, dim3(nwin), dim3(256), 0, s, src, clip_form, n0, T, Tm, valid, w, shift, static_cast<f16*>(out));
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Max-pool, window (2, 3), stride (2, 2), no padding, NHWC: (N, H, W, C) -> (N, (H - 2) / 2 + 1, (W - 3) / 2 + 1, C); C % 8 == 0.
// A thread takes 16 bytes of channels of one output pixel.  Exact: the output is one of the six inputs.
template <class ET>
__global__ __launch_bounds__(256) void maxpool_2x3_s2_kernel(const ET* __restrict__ in, ET* __restrict__ out, int H, int W, int C, int OH, int OW,
                                                             long total) {
    constexpr int V = 16 / sizeof(ET);
    typedef ET evec __attribute__((ext_vector_type(V)));
    const int cv = C / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % cv);
        long r = i / cv;
        const int ow = (int)(r % OW);
        r /= OW;
        const int oh = (int)(r % OH);
        const long nimg = r / OH;
        const ET* p = in + ((nimg * H + 2 * oh) * W + 2 * ow) * C + c * V;
        evec m = *reinterpret_cast<const evec*>(p);
#pragma unroll
        for (int t = 1; t < 6; ++t) {
            const evec v = *reinterpret_cast<const evec*>(p + ((long)(t / 3) * W + t % 3) * C);
#pragma unroll
            for (int e = 0; e < V; ++e) m[e] = (float)v[e] > (float)m[e] ? v[e] : m[e];
        }
        *reinterpret_cast<evec*>(out + ((nimg * OH + oh) * OW + ow) * C + c * V) = m;
    }
}

hipError_t launch_maxpool_2x3_s2(const void* in, void* out, int N, int H, int W, int C, int f32, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    if (!in || !out || H < 2 || W < 3 || C <= 0 || C % 8 || ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15)) return hipErrorInvalidValue;
    const int OH = (H - 2) / 2 + 1, OW = (W - 3) / 2 + 1;
    const long total = (long)N * OH * OW * (C / (f32 ? 4 : 8));
    if (f32) {
        record_kernel("maxpool_2x3_s2_kernel<float>");
        hipLaunchKernelGGL(maxpool_2x3_s2_kernel<float>, dim3(grid_for(total)), dim3(256), 0, s, static_cast<const float*>(in), static_cast<float*>(out), H, W,
                           C, OH, OW, total);
    } else {
        record_kernel("maxpool_2x3_s2_kernel<f16>");
        hipLaunchKernelGGL(maxpool_2x3_s2_kernel<f16>, dim3(grid_for(total)), dim3(256), 0, s, static_cast<const f16*>(in), static_cast<f16*>(out), H, W, C, OH,
                           OW, total);
    }
    return hipGetLastError();
}
