// HBM-bound helper kernels (gfx950) that depend on the 16-bit operand type and that a bf16 handle launches (LAUNCH, engine.h): compiled
// twice, fp16 and -DJG_BF16 (common.h has the rule).  Layout changes, pooling, both LayerNorm flavours, means.  One wave (64 lanes)
// per row for the row reductions; 16-byte vector accesses wherever the layout allows (guide G13).
#include "common.h"

JG_NS_BEGIN

// ---------------------------------------------------------------------------------------------
// Temporal stacking for conv1 (v0 path): S[b][p][h][w][16] = {frame(p+dt)[h][w][c] : dt<5, c<3} + 0
// frame index = clamp(p + dt - pad, 0, T-1)  (edge padding of inference_embs.py:283; pad=0 for
// the raw-window path).  u8 sources are kept as exact integers (fp16 holds 0..255 exactly); the
// 1/255 is applied in fp32 in the conv1 epilogue.
template <typename SRC>
__global__ void stack_frames_kernel(const SRC* __restrict__ src, long sb, long st, long sh, long sw, long sc,
                                    int B, int T, int pad, int H, int W, f16* __restrict__ dst) {
    const int P = T + 2 * pad - 4;
    const long total = (long)B * P * H * W;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int w = idx % W;
        long r = idx / W;
        const int h = r % H;
        r /= H;
        const int p = r % P;
        const int b = r / P;
        f16 v[16];
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) {
            int f = p + dt - pad;
            f = f < 0 ? 0 : (f > T - 1 ? T - 1 : f);
            const SRC* s = src + b * sb + f * st + h * sh + w * sw;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[dt * 3 + c] = (f16)(float)s[c * sc];
        }
        v[15] = (f16)0.f;
        uint4* d = reinterpret_cast<uint4*>(dst + idx * 16);
        d[0] = *reinterpret_cast<uint4*>(&v[0]);
        d[1] = *reinterpret_cast<uint4*>(&v[8]);
    }
}

hipError_t launch_stack_frames(const void* src, int src_is_u8, long sb, long st, long sh, long sw, long sc,
                               int B, int T, int pad, int H, int W, f16* dst, hipStream_t s) {
    const long total = (long)B * (T + 2 * pad - 4) * H * W;
    const int grid = grid_for(total);
    if (src_is_u8) {
        record_kernel("stack_frames_kernel<uint8_t>");
        hipLaunchKernelGGL(stack_frames_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, (const uint8_t*)src, sb, st, sh, sw, sc, B, T, pad, H, W, dst);
    } else {
        record_kernel("stack_frames_kernel<float>");
        hipLaunchKernelGGL(stack_frames_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)src, sb, st, sh, sw, sc, B, T, pad, H, W, dst);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// MaxPool (1,3,3)/(1,2,2), no padding, NHWC fp16, 8 channels per thread (gestsync.py:42-45,74-77).
__global__ void maxpool_kernel(const f16* __restrict__ in, f16* __restrict__ out, int N, int H, int W, int C, int OH, int OW,
                               const int* __restrict__ s2, int in_op, const f16* __restrict__ const_in) {
    const bool skip = s2 && const_in;
    const int cv = C / 8;
    const long total = (long)N * OH * OW * cv;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c8 = idx % cv;
        long r = idx / cv;
        const int ow = r % OW;
        r /= OW;
        const int oh = r % OH;
        const int n = r / OH;
        const int rin = skip ? conv_skip_decode(s2[n], in_op) : 0;      // image n's producer left its first rin rows to the const image
        f16x8 m;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ih = oh * 2 + kh;
                const f16* img = ih < rin ? const_in : in + (long)n * H * W * C;
                const f16x8 v = *reinterpret_cast<const f16x8*>(img + ((long)ih * W + ow * 2 + kw) * C + c8 * 8);
                if (kh == 0 && kw == 0) m = v;
                else
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
            }
        *reinterpret_cast<f16x8*>(out + idx * 8) = m;
    }
}

hipError_t launch_maxpool3x3s2(const f16* in, f16* out, int N, int H, int W, int C, hipStream_t s, const int* s2, int in_op,
                               const f16* const_in) {
    const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    const long total = (long)N * OH * OW * (C / 8);
    const int grid = grid_for(total);
    record_kernel("maxpool_kernel");
    hipLaunchKernelGGL(maxpool_kernel, dim3(grid), dim3(256), 0, s, in, out, N, H, W, C, OH, OW, s2, in_op, const_in);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Window gather + positional encoding (gestsync.py:152, windowing of inference_embs.py:488-492):
// x[(b,i,j)][:] = conv[b][clamp(i+j-shift, 0, P-1)][:] + pe[j][:]   i < Twin, j < L.  conv is (B,P,D) fp32.
// shift/clamp: with edge padding the first 9 and last 9 padded-clip positions see five copies of the
// same frame, so the conv stack is only evaluated for the T+4 distinct positions (shift = 8).
__global__ void window_gather_kernel(const float* __restrict__ conv, const float* __restrict__ pe, int B, int P, int Twin,
                                     int L, int D, int shift, float* __restrict__ x32, f16* __restrict__ x16) {
    const int dv = D / 4;
    const long total = (long)B * Twin * L * dv;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int d4 = idx % dv;
        long r = idx / dv;
        const int j = r % L;
        r /= L;
        const int i = r % Twin;
        const int b = r / Twin;
        int pp = i + j - shift;
        pp = pp < 0 ? 0 : (pp > P - 1 ? P - 1 : pp);
        f32x4 v = *reinterpret_cast<const f32x4*>(conv + ((long)b * P + pp) * D + d4 * 4);
        v += *reinterpret_cast<const f32x4*>(pe + (long)j * D + d4 * 4);
        const f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
        *reinterpret_cast<f32x4*>(x32 + idx * 4) = v;
        if (x16) *reinterpret_cast<f16x4*>(x16 + idx * 4) = h;      // (nullptr: the fp32 audit path)
    }
}

// Tiled variant (token stream of the fused GEMM+LayerNorm kernel, layout in common.h): one wave per 16-row x 64-column
// block, lane = (column quad ng, row m15) exactly as in the LN epilogue of gemm_glds_kernel -- a lane holds columns
// 16q + 4ng .. +3 (q = 0..3) of its row, so every store instruction of the wave covers a contiguous 512 B (one per q).
// (The element-per-thread kernel above wrote 32-byte pieces 512 B apart: 67 us for the 155 MB of a 32-clip chunk.)
__global__ __launch_bounds__(256) void window_gather_tiled_kernel(const float* __restrict__ conv, const float* __restrict__ pe, int B, int P, int Twin,
                                                                  int L, int shift, f16* __restrict__ x16) {
    const long M = (long)B * Twin * L;
    const long nblk = ((M + 15) >> 4) * 8;
    const long blk = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (blk >= nblk) return;
    const int lane = threadIdx.x & 63, m15 = lane & 15, ng = lane >> 4;
    const long rb = blk >> 3;                       // 16-row block
    const int cb = (int)(blk & 7);                  // 64-column block
    long row = rb * 16 + m15;
    const bool live = row < M;
    row = live ? row : M - 1;
    // 32-bit index math (the launcher checks M < 2^31): 64-bit divisions by run-time values cost ~100 VALU instructions each and
    // made this store-bound kernel VALU-bound
    const unsigned r32 = (unsigned)row;
    const unsigned r2 = r32 / (unsigned)L;
    const int j = (int)(r32 - r2 * (unsigned)L);
    const unsigned b = r2 / (unsigned)Twin;
    const int i = (int)(r2 - b * (unsigned)Twin);
    int pp = i + j - shift;
    pp = pp < 0 ? 0 : (pp > P - 1 ? P - 1 : pp);
    const float* src = conv + ((long)b * P + pp) * 512 + cb * 64 + 4 * ng;
    const float* pes = pe + (long)j * 512 + cb * 64 + 4 * ng;
    f16* const dst = x16 + x16t_row_off(rb * 16 + m15) + x16t_col_off(cb * 64 + 4 * ng);      // + q * X16T_QUAD: the row's four column quads
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 v = *reinterpret_cast<const f32x4*>(src + 16 * q);
        v += *reinterpret_cast<const f32x4*>(pes + 16 * q);
        const f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
        if (live) __builtin_nontemporal_store(h, reinterpret_cast<f16x4*>(dst + q * X16T_QUAD));
    }
}

hipError_t launch_window_gather(const float* conv, const float* pe, int B, int P, int Twin, int L, int D, int shift, bool tiled,
                                float* x32, f16* x16, hipStream_t s) {
    if (tiled && D != 512) return hipErrorInvalidValue;
    if (P <= 0 || L <= 0 || Twin <= 0) return hipErrorInvalidValue;      // an empty clamp range; both kernels divide by L and Twin
    if (!tiled && D % 4) return hipErrorInvalidValue;                    // four columns per thread
    if (tiled) {
        if ((long)B * Twin * L >= (1L << 31)) return hipErrorInvalidValue;
        const long nblk = (((long)B * Twin * L + 15) >> 4) * 8;
        record_kernel("window_gather_tiled_kernel");
        hipLaunchKernelGGL(window_gather_tiled_kernel, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, s, conv, pe, B, P, Twin, L, shift, x16);
        return hipGetLastError();
    }
    const long total = (long)B * Twin * L * (D / 4);
    const int grid = grid_for(total);
    record_kernel("window_gather_kernel");
    hipLaunchKernelGGL(window_gather_kernel, dim3(grid), dim3(256), 0, s, conv, pe, B, P, Twin, L, D, shift, x32, x16);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// LayerNorm, one wave per row, fp32 statistics.
//   LN_STD       : nn.LayerNorm   (x-mean)/sqrt(var_biased+1e-5)*w+b          (gestsync.py:20, jegal.py:26)
//   LN_ANNOTATED : modules.py:32-35  w*(x-mean)/(std_unbiased+1e-6)+b
// D = 64*4*V (V = 2 for 512, 3 for 768).
template <int V>
__global__ void layernorm_kernel(const float* in, const float* __restrict__ w, const float* __restrict__ b,
                                 int rows, int flavour, int relu, float* out32, f16* __restrict__ out16) {
    constexpr int D = 256 * V;
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = in + row * D;
    f32x4 v[V];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        v[i] = *reinterpret_cast<const f32x4*>(x + (i * 64 + lane) * 4);
        sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(sum) * (1.f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        v[i] -= mean;
        sq += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    sq = wave_sum(sq);
    float inv;
    if (flavour == LN_STD) inv = 1.f / sqrtf(sq * (1.f / D) + 1e-5f);
    else inv = 1.f / (sqrtf(sq * (1.f / (D - 1))) + 1e-6f);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int col = (i * 64 + lane) * 4;
        const f32x4 ww = *reinterpret_cast<const f32x4*>(w + col);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(b + col);
        f32x4 y = v[i] * inv * ww + bb;
        if (relu) { y.x = fmaxf(y.x, 0.f); y.y = fmaxf(y.y, 0.f); y.z = fmaxf(y.z, 0.f); y.w = fmaxf(y.w, 0.f); }
        if (out32) *reinterpret_cast<f32x4*>(out32 + row * D + col) = y;
        if (out16) {
            f16x4 h = {(f16)y.x, (f16)y.y, (f16)y.z, (f16)y.w};
            *reinterpret_cast<f16x4*>(out16 + row * D + col) = h;
        }
    }
}

hipError_t launch_layernorm(const float* in, const float* w, const float* b, int rows, int D, int flavour,
                            int relu, float* out32, f16* out16, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    const int grid = (rows + 3) / 4;
    if (D == 512) {
        record_kernel("layernorm_kernel<2>");
        hipLaunchKernelGGL(layernorm_kernel<2>, dim3(grid), dim3(256), 0, s, in, w, b, rows, flavour, relu, out32, out16);
    } else if (D == 768) {
        record_kernel("layernorm_kernel<3>");
        hipLaunchKernelGGL(layernorm_kernel<3>, dim3(grid), dim3(256), 0, s, in, w, b, rows, flavour, relu, out32, out16);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Mean over groups of L consecutive rows (fp16 in, fp32 sum, fp16 out): the mean(-1) of
// inference_embs.py:511 moved in front of ff_vid.2 (it commutes with the Linear).
__global__ void group_mean_kernel(const f16* __restrict__ in, int groups, int L, int D, f16* __restrict__ out) {
    const int dv = D / 8;
    const long total = (long)groups * dv;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int d8 = idx % dv;
        const long g = idx / dv;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < L; ++j) {
            const f16x8 v = __builtin_nontemporal_load(reinterpret_cast<const f16x8*>(in + (g * L + j) * D + d8 * 8));      // read once
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
        }
        f16x8 o;
        const float inv = 1.f / L;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f16)(acc[e] * inv);
        *reinterpret_cast<f16x8*>(out + idx * 8) = o;
    }
}

hipError_t launch_group_mean(const f16* in, int groups, int L, int D, f16* out, hipStream_t s) {
    if (D % 8 || L <= 0) return hipErrorInvalidValue;      // eight columns per thread; the mean of no rows
    const long total = (long)groups * (D / 8);
    if (total <= 0) return hipSuccess;
    record_kernel("group_mean_kernel");
    hipLaunchKernelGGL(group_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, groups, L, D, out);
    return hipGetLastError();
}

__global__ void cast_kernel(const float* __restrict__ in, f16* __restrict__ out, long n4) {
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < n4; idx += (long)gridDim.x * blockDim.x) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(in + idx * 4);
        f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
        *reinterpret_cast<f16x4*>(out + idx * 4) = h;
    }
}

hipError_t launch_cast_f32_f16(const float* in, f16* out, long n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n % 4) return hipErrorInvalidValue;      // four elements per thread
    const long n4 = n / 4;
    const int grid = grid_for(n4);
    record_kernel("cast_kernel");
    hipLaunchKernelGGL(cast_kernel, dim3(grid), dim3(256), 0, s, in, out, n4);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// First audio conv (jegal.py:42, Conv2d(1,32,5,pad 2) + BN + ReLU) directly (round 3; rounds 1-2: an im2col kernel + a register-staged
// K = 32 GEMM, 0.24 ms of the 0.64 ms audio CNN at B = 64; now 0.10 ms): out[(b,t,f)][32] = relu(sum_taps x16 * w16 + bias), the same operands the GEMM saw (mel and the BN-folded weights
// rounded to the 16-bit operand type, fp32 accumulation; only the summation order differs).  One thread per output pixel: the
// 5 x 5 neighbourhood comes from a mel tile in LDS, the 25 x 32 weights are wave-uniform (fp32 copy in LDS, broadcast reads),
// 800 FMAs per pixel, one 64-byte NHWC store.  W2 modes carry the lo part of the weights in the same fp32 copy.
// valid (optional, [B]): clip b holds only valid[b] mel frames -- frames beyond are read as the zero padding the clip would see alone,
// and output rows beyond are written as zeros (the next layer's zero padding): see zero_tail_kernel.
__global__ __launch_bounds__(256) void audio_conv0_kernel(const float* __restrict__ mel, int B, int Tm, int F, const f16* __restrict__ wh,
                                                          const f16* __restrict__ wl, const float* __restrict__ bias, f16* __restrict__ out,
                                                          const int* __restrict__ valid) {
    constexpr int TR = 3, FW_MAX = 84;                   // 3 output rows x F (<= 80) per block: (TR + 4) x (F + 4) mel values staged
    __shared__ float sm[(TR + 4) * FW_MAX];
    __shared__ float sw[25 * 32];
    __shared__ float sb[32];
    const int tid = threadIdx.x;
    const int tiles_t = (Tm + TR - 1) / TR;
    const int b = blockIdx.x / tiles_t, t0 = (blockIdx.x - b * tiles_t) * TR;
    const int Tv = valid ? min(max(valid[b], 0), Tm) : Tm;
    for (int i = tid; i < 25 * 32; i += 256) {
        const int tap = i >> 5, oc = i & 31;
        sw[i] = (float)wh[oc * 32 + tap] + (wl ? (float)wl[oc * 32 + tap] : 0.f);
    }
    if (tid < 32) sb[tid] = bias[tid];
    const int FW = F + 4;
    for (int i = tid; i < (TR + 4) * FW; i += 256) {
        const int r = i / FW, c = i - r * FW;
        const int tt = t0 + r - 2, ff = c - 2;
        float x = 0.f;
        if (tt >= 0 && tt < Tv && ff >= 0 && ff < F) x = mel[((long)b * Tm + tt) * F + ff];
        sm[r * FW_MAX + c] = (float)(f16)x;             // the operand rounding of the GEMM path
    }
    __syncthreads();
    const int r = tid / F, f = tid - r * F;
    if (r >= TR || t0 + r >= Tm) return;
    uint4* d = reinterpret_cast<uint4*>(out + (((long)b * Tm + t0 + r) * F + f) * 32);
    if (t0 + r >= Tv) {                                  // beyond the clip's own frames: the next layer's zero padding
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    float acc[32];
#pragma unroll
    for (int oc = 0; oc < 32; ++oc) acc[oc] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 5; ++kh)
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) {
            const float x = sm[(r + kh) * FW_MAX + f + kw];
            const float* w = sw + (kh * 5 + kw) * 32;
#pragma unroll
            for (int oc = 0; oc < 32; ++oc) acc[oc] = __builtin_fmaf(x, w[oc], acc[oc]);
        }
    f16 o[32];
#pragma unroll
    for (int oc = 0; oc < 32; ++oc) o[oc] = (f16)fmaxf(acc[oc] + sb[oc], 0.f);
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = *reinterpret_cast<uint4*>(&o[q * 8]);
}

hipError_t launch_audio_conv0(const float* mel, int B, int Tm, int F, const f16* wh, const f16* wl, const float* bias, f16* out, const int* valid,
                              hipStream_t s) {
    if (B <= 0 || Tm <= 0) return hipSuccess;
    if (F < 1 || F > 80 || 3 * F > 256) return hipErrorInvalidValue;
    record_kernel("audio_conv0_kernel");
    hipLaunchKernelGGL(audio_conv0_kernel, dim3((unsigned)(B * ((Tm + 2) / 3))), dim3(256), 0, s, mel, B, Tm, F, wh, wl, bias, out, valid);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Per-clip valid lengths in a zero-padded audio batch (evaluation/extract_jegal_embs.py:141 runs batch_size = 1: a clip never
// sees another clip's length).  Layer outputs are NHWC [b][h][w][c] with h = time; a clip of valid[b] mel frames has
// len = valid[b] rows after the stride-1 layers and (len - 1) / 2 + 1 after each stride-2 layer (3x3, pad 1).  Rows h >= len of
// clip b are set to zero, which is exactly the zero padding the next conv layer would apply to the clip alone -- the rows
// h < len of every layer then do not depend on the batch's longest clip.  One block per (b, h) row.
__global__ __launch_bounds__(256) void zero_tail_kernel(f16* __restrict__ x, const int* __restrict__ valid, int halvings, int H, int row_vec) {
    const int b = blockIdx.x / H, hrow = blockIdx.x - b * H;
    int len = max(valid[b], 0);
    for (int i = 0; i < halvings; ++i) len = len > 0 ? (len - 1) / 2 + 1 : 0;
    if (hrow < len) return;
    uint4* p = reinterpret_cast<uint4*>(x) + (long)blockIdx.x * row_vec;
    for (int i = threadIdx.x; i < row_vec; i += 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

hipError_t launch_zero_tail(f16* x, const int* valid, int halvings, int B, int H, long row_elems, hipStream_t s) {
    if (B <= 0 || H <= 0 || !valid) return hipSuccess;
    if (row_elems % 8) return hipErrorInvalidValue;
    record_kernel("zero_tail_kernel");
    hipLaunchKernelGGL(zero_tail_kernel, dim3((unsigned)(B * H)), dim3(256), 0, s, x, valid, halvings, H, (int)(row_elems / 8));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Ragged word pooling (jegal.py:174-180,189-195): dst[seg.dst][col..col+D) = mean(seq[seg.start : seg.end]).
// seg = int32 triplets (start_row, end_row_exclusive, dst_row).  One wave per segment.
__global__ void segment_mean_kernel(const float* __restrict__ seq, int D, const int32_t* __restrict__ seg, int n,
                                    f16* __restrict__ dst16, float* __restrict__ dst32, int dst_ld, int dst_col) {
    const int lane = threadIdx.x & 63;
    const int sidx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (sidx >= n) return;
    const int s0 = seg[sidx * 3], s1 = seg[sidx * 3 + 1], dr = seg[sidx * 3 + 2];
    const float inv = 1.f / (float)(s1 - s0);
    for (int c = lane; c < D; c += 64) {
        float acc = 0.f;
        for (int r = s0; r < s1; ++r) acc += seq[(long)r * D + c];
        const float m = (s1 - s0 > 1) ? acc * inv : acc;
        if (dst16) dst16[(long)dr * dst_ld + dst_col + c] = (f16)m;
        if (dst32) dst32[(long)dr * dst_ld + dst_col + c] = m;
    }
}

hipError_t launch_segment_mean(const float* seq, int D, const int32_t* seg, int n, f16* dst16, float* dst32,
                               int dst_ld, int dst_col, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(segment_mean_kernel, dim3((n + 3) / 4), dim3(256), 0, s, seq, D, seg, n, dst16, dst32, dst_ld, dst_col);
    return hipGetLastError();
}

// Implicit-LayerNorm token stream (GemmArgs::ln_mode, common.h): xlmr_embed_kernel's embedding sum (elementwise_f32.hip), NOT normalised, as two fp16 planes
// (hi = fp16(x), lo = fp16(x - hi)) plus per row and 64-column block the (sum, sum of squares) that launch_ln_stats turns into the
// embedding LayerNorm's (mean, rstd).  One wave per token row; lane l holds columns 256 i + 4 l .. + 3: block = 4 i + l / 16.
__global__ __launch_bounds__(256) void xlmr_embed_planes_kernel(const int32_t* __restrict__ ids, int B, int L, int D, int pad_id, int vocab, int maxpos,
                                                                const float* __restrict__ word, const float* __restrict__ pos,
                                                                const float* __restrict__ type, f16* __restrict__ hi, f16* __restrict__ lo,
                                                                float* __restrict__ part) {
    const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (long)B * L) return;
    const int b = (int)(row / L), t = (int)(row - (long)b * L);
    int cnt = 0;
    for (int j = lane; j <= t; j += 64) cnt += ids[(long)b * L + j] != pad_id ? 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    int id = ids[row];
    int pid = id != pad_id ? pad_id + cnt : pad_id;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    pid = pid >= maxpos ? maxpos - 1 : pid;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(word + (long)id * D + c);
        const f32x4 p = *reinterpret_cast<const f32x4*>(pos + (long)pid * D + c);
        const f32x4 ty = *reinterpret_cast<const f32x4*>(type + c);
        const f32x4 v = (w + ty) + p;
        const f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
        const f16x4 l = {(f16)(v.x - (float)h.x), (f16)(v.y - (float)h.y), (f16)(v.z - (float)h.z), (f16)(v.w - (float)h.w)};
        *reinterpret_cast<f16x4*>(hi + row * D + c) = h;
        *reinterpret_cast<f16x4*>(lo + row * D + c) = l;
        float s1 = (v.x + v.y) + (v.z + v.w), s2 = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
            s1 += __shfl_xor(s1, d, 64);
            s2 += __shfl_xor(s2, d, 64);
        }
        if ((lane & 15) == 0) *reinterpret_cast<f32x2_t*>(part + ln_part_index(row, D >> 6, c >> 6)) = f32x2_t{s1, s2};
    }
}
hipError_t launch_xlmr_embed_planes(const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word, const float* pos,
                                    const float* type, f16* hi, f16* lo, float* part, hipStream_t s) {
    if (D % 256) return hipErrorInvalidValue;
    record_kernel("xlmr_embed_planes_kernel");
    hipLaunchKernelGGL(xlmr_embed_planes_kernel, dim3((unsigned)(((long)B * L + 3) / 4)), dim3(256), 0, s, ids, B, L, D, pad_id, vocab, maxpos, word, pos, type,
                       hi, lo, part);
    return hipGetLastError();
}
// out32 = nn.LayerNorm(hi + lo): the explicit LayerNorm that ends an implicit chain (two-pass statistics like layernorm_kernel)
template <int V>
__global__ void layernorm_planes_kernel(const f16* __restrict__ hi, const f16* __restrict__ lo, const float* __restrict__ w, const float* __restrict__ b,
                                        int rows, float* __restrict__ out32) {
    constexpr int D = 256 * V;
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    f32x4 v[V];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const f16x4 h = *reinterpret_cast<const f16x4*>(hi + row * D + (i * 64 + lane) * 4), l = *reinterpret_cast<const f16x4*>(lo + row * D + (i * 64 + lane) * 4);
        v[i] = f32x4{(float)h.x + (float)l.x, (float)h.y + (float)l.y, (float)h.z + (float)l.z, (float)h.w + (float)l.w};
        sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(sum) * (1.f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        v[i] -= mean;
        sq += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    const float inv = 1.f / sqrtf(wave_sum(sq) * (1.f / D) + 1e-5f);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int col = (i * 64 + lane) * 4;
        *reinterpret_cast<f32x4*>(out32 + row * D + col) = v[i] * inv * *reinterpret_cast<const f32x4*>(w + col) + *reinterpret_cast<const f32x4*>(b + col);
    }
}
hipError_t launch_layernorm_planes(const f16* hi, const f16* lo, const float* w, const float* b, int rows, int D, float* out32, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (D != 768) return hipErrorInvalidValue;
    record_kernel("layernorm_planes_kernel<3>");
    hipLaunchKernelGGL(layernorm_planes_kernel<3>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, hi, lo, w, b, rows, out32);
    return hipGetLastError();
}

JG_NS_END
