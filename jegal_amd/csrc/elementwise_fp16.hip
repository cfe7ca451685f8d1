// fp16-only helper kernels (gfx950): compiled once; the host calls them un-dispatched, on paths a bf16 handle cannot take (the
// GestSync const chain and layer-0 qkv, calibration sums, the run-time correction).  Launchers: the fp16-only block of common.h.
#include "common.h"

// Projection of the positional rows through a Linear layer (layer-0 qkv by linearity, attention.hip): one wave per output.
__global__ __launch_bounds__(256) void pe_project_kernel(const float* __restrict__ pe, int S, const f16* __restrict__ Wh, const f16* __restrict__ Wl,
                                                         const float* __restrict__ bias, int N, int K, f16* __restrict__ out) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= S * N) return;
    const int j = o / N, n = o - j * N;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) {
        float w = (float)Wh[(long)n * K + k];
        if (Wl) w += (float)Wl[(long)n * K + k];
        acc += w * pe[(long)j * K + k];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) out[o] = (f16)(acc + (bias ? bias[n] : 0.f));
}

hipError_t launch_pe_project(const float* pe, int S, const f16* Wh, const f16* Wl, const float* bias, int N, int K, f16* out, hipStream_t s) {
    record_kernel("pe_project_kernel");
    hipLaunchKernelGGL(pe_project_kernel, dim3((unsigned)((S * N + 3) / 4)), dim3(256), 0, s, pe, S, Wh, Wl, bias, N, K, out);
    return hipGetLastError();
}

// out[pixel][c] = v[c]: an image whose every pixel is the same channel vector (the all-constant input of the const chain)
__global__ void broadcast_channels_kernel(const f16* __restrict__ v, int C, f16* __restrict__ out, long total) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) out[i] = v[i % C];
}
hipError_t launch_broadcast_channels(const f16* v, int C, f16* out, long pixels, hipStream_t s) {
    const long total = pixels * C;
    record_kernel("broadcast_channels_kernel");
    hipLaunchKernelGGL(broadcast_channels_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0, s, v, C, out, total);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Column sums of a row-major fp16 matrix (calibration pass of the bias-corrected precision mode):
// out[k] += sum_m A[m][k].  8 columns per thread, rows strided over blockIdx.y, one float atomic per
// (thread, column) at the end.  `out` is zeroed by the caller.
// Deterministic (no atomics): 64 row-strided partial sums per column go to `part` [gy][K], then one thread per column
// adds them to out[] in a fixed order.  out ACCUMULATES across calls (stream order), so a calibration batch may arrive
// in chunks and two handles calibrated on the same data end up with bit-identical bias corrections.
// stats ([M][2] mean, rstd; optional): the rows are normalised first -- what a Linear behind an IMPLICIT LayerNorm effectively sees.
__global__ void col_sum_kernel(const f16* __restrict__ A, long lda, int M, int K, float* __restrict__ part, const float* __restrict__ stats) {
    const int c8 = blockIdx.x * blockDim.x + threadIdx.x;
    if (c8 * 8 >= K) return;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int m = blockIdx.y; m < M; m += gridDim.y) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(A + (long)m * lda + c8 * 8);
        const float mu = stats ? stats[2 * (long)m] : 0.f, rs = stats ? stats[2 * (long)m + 1] : 1.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += ((float)v[e] - mu) * rs;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[(long)blockIdx.y * K + c8 * 8 + e] = acc[e];
}
__global__ void col_sum_finish_kernel(const float* __restrict__ part, int gy, int K, float* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    float s = 0.f;
    for (int y = 0; y < gy; ++y) s += part[(long)y * K + k];
    out[k] += s;
}

size_t col_sum_scratch_elems(int K) { return (size_t)64 * K; }

hipError_t launch_col_sum(const f16* A, long lda, int M, int K, float* scratch, float* out, hipStream_t s, const float* stats) {
    if (M <= 0 || K <= 0) return hipSuccess;
    if (K % 8) return hipErrorInvalidValue;      // eight columns per thread
    const int cols = K / 8;
    const int gy = M < 64 ? M : 64;
    record_kernel("col_sum_kernel+col_sum_finish_kernel");
    hipLaunchKernelGGL(col_sum_kernel, dim3((cols + 63) / 64, gy), dim3(64), 0, s, A, lda, M, K, scratch, stats);
    hipLaunchKernelGGL(col_sum_finish_kernel, dim3((K + 255) / 256), dim3(256), 0, s, scratch, gy, K, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Run-time weight-rounding correction (precision mode JG_PREC_FP16_RC).  A Linear that runs on single fp16
// weights wh = fp16(w) loses (w - wh) . x per output; its systematic part is lo . E[x], lo = fp16(w - wh).  JG_PREC_FP16_BC takes
// E[x] from a calibration pass; here it comes from the rows of the clip AT HAND, per GEMM call, so nothing depends on calibration
// data or on the other clips of the batch:
//     bias_clip[c][n] = bias[n] + sum_k lo[n][k] * mean_c[k],   mean_c = mean of a fixed sample of clip c's rows of A
// (rows r = 0 .. rpc-1 relative to the clip's first row; sample: every row when rpc < 1024, otherwise the 16-row runs
// (r >> 4) % 8 == 0 -- the error of a sampled mean is the row spread / sqrt(rows sampled), a few per cent of what the correction
// removes).  Two launches: column means per clip (one workgroup per clip and 128-column slab, fixed summation order), then the skinny
// product on the matrix cores.  Deterministic.
__device__ __forceinline__ int rc_rows_sampled(int rpc) {
    if (rpc < 1024) return rpc;
    int cnt = 0;
    for (int r0 = 0; r0 < rpc; r0 += 128) cnt += rpc - r0 < 16 ? rpc - r0 : 16;
    return cnt;
}
// valid (optional, device [nclips]): clip c's first valid[c] rows are its own (a batch padded to a common length: the rest is padding that
// must not enter the clip's statistics); the sample is then defined on the clip's OWN row count, exactly as if it were alone.
__global__ __launch_bounds__(256) void rc_col_mean_kernel(const f16* __restrict__ A, long lda, int tiled, int rpc_all, const int* __restrict__ valid, int K,
                                                          f16* __restrict__ mean) {
    __shared__ float red[32][8 * 8 + 1];
    const int clip = blockIdx.x, t = threadIdx.x;
    const int cg = t & 7, rl = t >> 3;                          // 8 column groups of 8 (a 64-column slab) x 32 row lanes
    const int n = blockIdx.y * 64 + cg * 8;
    int rpc = rpc_all;                                          // rows of this clip that count
    if (valid) rpc = valid[clip] < 1 ? 1 : (valid[clip] < rpc_all ? valid[clip] : rpc_all);
    const int step = rpc < 1024 ? 16 : 128;                     // 16-row runs: every one, or every eighth
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto row_ptr = [&](int r) -> const f16* {
        const long m = (long)clip * rpc_all + r;
        return tiled ? A + x16t_index(m, n) : A + m * lda + n;
    };
    // row lane rl takes row (rl & 15) of every second sampled run (runs of its parity rl >> 4); EIGHT loads in flight per thread (the
    // rows were just written with nontemporal stores: every load is an HBM round trip, and a 150-frame clip gives a thread 13 rows),
    // summed in a fixed order
    const int stride = 2 * step;
    int r = (rl & 15) + (rl >> 4) * step;
    for (; r + 7 * stride < rpc; r += 8 * stride) {
        f16x8 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f16x8*>(row_ptr(r + u * stride));
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[u][e];
    }
    {   // the tail: up to seven rows, again all in flight
        f16x8 v[7];
#pragma unroll
        for (int u = 0; u < 7; ++u) {
            const int ru = r + u * stride;
            v[u] = *reinterpret_cast<const f16x8*>(row_ptr(ru < rpc ? ru : 0));
        }
#pragma unroll
        for (int u = 0; u < 7; ++u)
            if (r + u * stride < rpc) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)v[u][e];
            }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl][cg * 8 + e] = acc[e];
    __syncthreads();
    if (t < 64) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 32; ++q) s += red[q][t];
        mean[(long)clip * K + blockIdx.y * 64 + t] = (f16)(s / (float)rc_rows_sampled(rpc));
    }
}
// out[c][n] = bias[n] + sum_k lo[n][k] * mean[c][k]: a 32-clip x 32-column tile per workgroup on v_mfma_f32_32x32x16 (A = the lo rows,
// B = the clip means as fp16 -- the mean's own rounding, 2^-12, scales a term that is 3e-4 of the output), the four waves split K and
// meet in LDS.  (The VALU form of this product -- a wave-wide reduction per clip and column -- took 17 us per Linear, twice the
// column means; rocprofv3, round 5.)
__global__ __launch_bounds__(256) void rc_gemv_kernel(const f16* __restrict__ mean16, const f16* __restrict__ lo, const float* __restrict__ bias,
                                                      int nclips, int N, int K, float* __restrict__ out) {
    __shared__ float red[3][16][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r31 = lane & 31, hh = lane >> 5;
    const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int cl = c0 + r31 < nclips ? c0 + r31 : nclips - 1;
    const int kq = K >> 2;                                       // this wave's share of K
    const f16* ap = lo + (long)(n0 + r31) * K + wave * kq + 8 * hh;
    const f16* bp = mean16 + (long)cl * K + wave * kq + 8 * hh;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k = 0; k < kq; k += 128) {           // kq is 128 or 512: eight k-steps' operands in flight at a time
        f16x8 a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a[u] = *reinterpret_cast<const f16x8*>(ap + k + 16 * u);
            b[u] = *reinterpret_cast<const f16x8*>(bp + k + 16 * u);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = JG_MFMA_32x32x16(a[u], b[u], acc);
    }
    if (wave) {
#pragma unroll
        for (int i = 0; i < 16; ++i) red[wave - 1][i][lane] = acc[i];
    }
    __syncthreads();
    if (wave == 0 && c0 + r31 < nclips) {
        // register i <-> column n0 + mfma32_row(i, hh), lane <-> clip
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int n = n0 + mfma32_row(i, hh);
            out[(long)(c0 + r31) * N + n] = (bias ? bias[n] : 0.f) + (((acc[i] + red[0][i][lane]) + red[1][i][lane]) + red[2][i][lane]);
        }
    }
}

size_t rc_scratch_elems(int nclips, int K) { return (size_t)nclips * K; }

hipError_t launch_rc_bias(const f16* A, long lda, int tiled, int nclips, int rpc, const int* valid_rows, const f16* lo, const float* bias, int N, int K,
                          float* scratch, float* out, hipStream_t s) {
    if (nclips <= 0 || rpc <= 0) return hipSuccess;
    if (!rc_bias_ok(N, K, tiled)) return hipErrorInvalidValue;
    f16* mean16 = reinterpret_cast<f16*>(scratch);
    record_kernel("rc_col_mean_kernel+rc_gemv_kernel");
    hipLaunchKernelGGL(rc_col_mean_kernel, dim3(nclips, K / 64), dim3(256), 0, s, A, lda, tiled, rpc, valid_rows, K, mean16);
    hipLaunchKernelGGL(rc_gemv_kernel, dim3(N / 32, (nclips + 31) / 32), dim3(256), 0, s, mean16, lo, bias, nclips, N, K, out);
    return hipGetLastError();
}
