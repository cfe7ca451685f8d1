// Helper kernels (gfx950) with no 16-bit operand: compiled once, launchers declared in shared.h.  Layout changes, L2-normalise,
// the row movers of long gesture tracks, ragged means, the XLM-RoBERTa embedding sum and LayerNorm statistics, the log-mel and
// mask + resize front ends.
#include "common.h"

// (N, L, D) -> (N, D, L): the .transpose(1,2) of gestsync.py:156 for the drop-in forward_vid output.
__global__ void transpose_tokens_kernel(const float* __restrict__ in, int L, int D, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const long n = blockIdx.z;
    const int d0 = blockIdx.x * 32, l0 = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int l = l0 + r, d = d0 + threadIdx.x;
        tile[r][threadIdx.x] = (l < L && d < D) ? in[(n * L + l) * D + d] : 0.f;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int d = d0 + r, l = l0 + threadIdx.x;
        if (d < D && l < L) out[(n * D + d) * L + l] = tile[threadIdx.x][r];
    }
}

hipError_t launch_transpose_tokens(const float* in, int N, int L, int D, float* out, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    record_kernel("transpose_tokens_kernel");
    hipLaunchKernelGGL(transpose_tokens_kernel, dim3((D + 31) / 32, (L + 31) / 32, N), dim3(32, 8), 0, s, in, L, D, out);
    return hipGetLastError();
}

// F.normalize(p=2, dim=-1, eps=1e-12): x / max(||x||, eps)  (inference_embs.py:631,635). One wave per row.
__global__ void l2norm_kernel(const float* in, float* out, int rows, int D) {
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = in + row * D;
    float sq = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
        sq += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    const float nrm = fmaxf(sqrtf(wave_sum(sq)), 1e-12f);
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
        v.x /= nrm; v.y /= nrm; v.z /= nrm; v.w /= nrm;
        *reinterpret_cast<f32x4*>(out + row * D + c) = v;
    }
}

hipError_t launch_l2norm(const float* in, float* out, int rows, int D, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(l2norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, out, rows, D);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Long gesture tracks (jegal.hip, jegal_gesture_tracks_impl; the window rule: include/jegal_hip.h, jg_track_windows).  A window w of the
// table [n_windows][4] = (span first row, span length, core offset inside the span, core length) is encoded as a clip of span_max
// rows.  Both kernels are row movers: one wave per (window, span row), the window's table entry in one 16-byte scalar load, 16 bytes
// per lane and access (a 2 KB fp32 row of D = 512 is two accesses of the wave, each one contiguous KB), no LDS.
//   span_gather : x32[w][s] = p32[first_w + s] + pe[s] and mask[w][s] = 1 for s < len_w; zeros and 0 for the padding rows s >= len_w,
//                 which have to be WRITTEN: the encoder reads them as keys of weight exactly 0, and 0 * NaN is NaN (option ws_poison).
//   core_compact: out[first_w + s] = in[w][s] for the core rows coff_w <= s < coff_w + clen_w -- the cores partition the tracks, so
//                 every row of `out` is written exactly once, in track order.  Rows of row16 16-byte pieces, whatever the element type.
typedef int i32x4_t __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void span_gather_kernel(const float* __restrict__ p32, const float* __restrict__ pe, const i32x4_t* __restrict__ table,
                                                          unsigned rows, unsigned span_max, int D, float* __restrict__ x32, float* __restrict__ mask) {
    const unsigned r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));      // wave-uniform: the table entry is a scalar load
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const unsigned w = r / span_max, s = r - w * span_max;
    const i32x4_t e = table[w];
    const bool live = s < (unsigned)min(max(e.y, 0), (int)span_max);
    const float* src = p32 + ((long)e.x + s) * D;
    const float* pos = pe + (long)s * D;
    float* dst = x32 + (long)r * D;
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (live) v = *reinterpret_cast<const f32x4*>(src + c) + *reinterpret_cast<const f32x4*>(pos + c);
        *reinterpret_cast<f32x4*>(dst + c) = v;
    }
    if (lane == 0) mask[r] = live ? 1.f : 0.f;
}

hipError_t launch_span_gather(const float* p32, const float* pe, const int32_t* table, int n_windows, int span_max, int D, float* x32, float* mask,
                              hipStream_t s) {
    if (n_windows <= 0) return hipSuccess;
    if (span_max < 1 || D <= 0 || D % 4 || (long)n_windows * span_max >= (1L << 31)) return hipErrorInvalidValue;
    const unsigned rows = (unsigned)n_windows * (unsigned)span_max;
    record_kernel("span_gather_kernel");
    hipLaunchKernelGGL(span_gather_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, p32, pe, reinterpret_cast<const i32x4_t*>(table), rows,
                       (unsigned)span_max, D, x32, mask);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void core_compact_kernel(const uint4* __restrict__ in, const i32x4_t* __restrict__ table, unsigned rows, unsigned span_max,
                                                           int row16, uint4* __restrict__ out) {
    const unsigned r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (r >= rows) return;
    const unsigned w = r / span_max, s = r - w * span_max;
    const i32x4_t e = table[w];
    if ((int)s < e.z || (int)s >= e.z + e.w) return;                  // not a core row: some other window emits this frame
    const uint4* src = in + (long)r * row16;
    uint4* dst = out + ((long)e.x + s) * row16;
    for (int i = threadIdx.x & 63; i < row16; i += 64) dst[i] = src[i];
}

hipError_t launch_core_compact(const void* in, int elem_bytes, const int32_t* table, int n_windows, int span_max, int D, void* out, hipStream_t s) {
    if (n_windows <= 0) return hipSuccess;
    if (span_max < 1 || D <= 0 || (elem_bytes != 2 && elem_bytes != 4) || (long)D * elem_bytes % 16 || (long)n_windows * span_max >= (1L << 31))
        return hipErrorInvalidValue;
    const unsigned rows = (unsigned)n_windows * (unsigned)span_max;
    record_kernel("core_compact_kernel");
    hipLaunchKernelGGL(core_compact_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, static_cast<const uint4*>(in), reinterpret_cast<const i32x4_t*>(table),
                       rows, (unsigned)span_max, (int)((long)D * elem_bytes / 16), static_cast<uint4*>(out));
    return hipGetLastError();
}

// Test aid (option ws_poison, begin_pass): 0xff bytes -- fp16 / fp32 NaN -- over a workspace chunk
namespace {
__global__ void poison_kernel(uint4* __restrict__ p, size_t n16) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
}
}  // namespace

hipError_t launch_poison(void* p, size_t bytes, hipStream_t s) {
    if (!p || bytes < 16) return hipSuccess;
    hipLaunchKernelGGL(poison_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint4*>(p), bytes / 16);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// XLM-RoBERTa front end (third-party transformers.XLMRobertaModel, call site jegal.py:116-129).
// Embeddings: word[id] + position[pid] + token_type[0], pid = padding_idx + (number of non-pad tokens up to and including
// this one) for non-pad tokens and padding_idx for pads (create_position_ids_from_input_ids).  One wave per token row.
__global__ __launch_bounds__(256) void xlmr_embed_kernel(const int32_t* __restrict__ ids, int B, int L, int D, int pad_id, int vocab, int maxpos,
                                                         const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
                                                         float* __restrict__ out) {
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
        *reinterpret_cast<f32x4*>(out + row * D + c) = (w + ty) + p;       // HF: inputs_embeds + token_type_embeddings, then + position
    }
}
hipError_t launch_xlmr_embed(const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word, const float* pos,
                             const float* type, float* out, hipStream_t s) {
    if (D % 4) return hipErrorInvalidValue;
    record_kernel("xlmr_embed_kernel");
    hipLaunchKernelGGL(xlmr_embed_kernel, dim3((unsigned)(((long)B * L + 3) / 4)), dim3(256), 0, s, ids, B, L, D, pad_id, vocab, maxpos, word, pos, type, out);
    return hipGetLastError();
}
// (mean, rstd) of every row from its per-block partial sums, accumulated in double: var = E[x^2] - mean^2 (biased, nn.LayerNorm), eps 1e-5
__global__ void ln_stats_kernel(const float* __restrict__ part, int rows, int P, float* __restrict__ stats) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < P; ++p) {
        const f32x2_t v = *reinterpret_cast<const f32x2_t*>(part + ln_part_index(r, P, p));
        s1 += (double)v.x;
        s2 += (double)v.y;
    }
    const double inv_d = 1.0 / (double)(P * 64), mean = s1 * inv_d;
    double var = s2 * inv_d - mean * mean;
    var = var > 0.0 ? var : 0.0;
    *reinterpret_cast<f32x2_t*>(stats + 2 * (long)r) = f32x2_t{(float)mean, 1.f / sqrtf((float)var + 1e-5f)};
}
hipError_t launch_ln_stats(const float* part, int rows, int P, float* stats, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    record_kernel("ln_stats_kernel");
    hipLaunchKernelGGL(ln_stats_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, part, rows, P, stats);
    return hipGetLastError();
}
// int attention mask (1 = token, 0 = padding) -> the float key mask the attention kernels take
__global__ void mask_i32_f32_kernel(const int32_t* __restrict__ in, float* __restrict__ out, long n) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] != 0 ? 1.f : 0.f;
}
hipError_t launch_mask_i32_f32(const int32_t* in, float* out, long n, hipStream_t s) {
    record_kernel("mask_i32_f32_kernel");
    hipLaunchKernelGGL(mask_i32_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}

// Temporal mean of ragged (rows,D) blocks: out[i] = mean(x[offsets[i]:offsets[i+1]])
// (evaluate_retrieval.py:30-31, evaluate_asd.py:31,35).  One wave per (clip, 64-col group).
__global__ void ragged_mean_kernel(const float* __restrict__ x, const int32_t* __restrict__ off, int n, int D, float* __restrict__ out) {
    const int i = blockIdx.x;
    const int s0 = off[i], s1 = off[i + 1];
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float acc = 0.f;
        for (int r = s0; r < s1; ++r) acc += x[(long)r * D + c];
        out[(long)i * D + c] = acc / (float)(s1 - s0);
    }
}

hipError_t launch_ragged_mean(const float* x, const int32_t* offsets, int n, int D, float* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ragged_mean_kernel, dim3(n), dim3(256), 0, s, x, offsets, n, D, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Log-mel front-end (utils/audio_utils.py:28-66): torch.stft(n_fft 512, hop 160, hann(320) centred in the
// 512 window, center=True / reflect padding, onesided) -> drop the last frame -> |X| -> mel_basis (80x257) ->
// log(. + 1e-20).  One block per frame: the windowed 512-sample segment and a 512-entry twiddle table live in
// LDS, thread f computes bin f (and f+256) by direct DFT in fp32 (316 MFLOP per 150-frame clip: not worth an FFT),
// then threads 0..79 do the mel dot products.  n_samples >= 257 (jg_logmel refuses less): one reflection at either end then lands inside
// the signal, as torch.stft demands; the clamp below is never reached.
__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ wav, int n_samples, int n_frames,
                                                     const float* __restrict__ mel_basis, float* __restrict__ out) {
    __shared__ float seg[512];
    __shared__ float tc[512], ts[512];
    __shared__ float mag[257];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* x = wav + (long)b * n_samples;
    for (int n = tid; n < 512; n += 256) {
        float w = 0.f;
        if (n >= 96 && n < 416) w = 0.5f - 0.5f * cosf(6.283185307179586f * (float)(n - 96) / 320.f);
        int i = t * 160 + n - 256;
        if (i < 0) i = -i;
        if (i >= n_samples) i = 2 * (n_samples - 1) - i;
        i = i < 0 ? 0 : i;
        seg[n] = w * x[i];
        float sn, cs;
        sincosf(6.283185307179586f * (float)n / 512.f, &sn, &cs);
        tc[n] = cs;
        ts[n] = sn;
    }
    __syncthreads();
    for (int f = tid; f < 257; f += 256) {
        float re = 0.f, im = 0.f;
        int ph = 0;
        for (int n = 0; n < 512; ++n) {
            re += seg[n] * tc[ph];
            im -= seg[n] * ts[ph];
            ph = (ph + f) & 511;
        }
        mag[f] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    if (tid < 80) {
        const float* mb = mel_basis + tid * 257;
        float acc = 0.f;
        for (int f = 0; f < 257; ++f) acc += mb[f] * mag[f];
        out[((long)b * n_frames + t) * 80 + tid] = logf(acc + 1e-20f);
    }
}

hipError_t launch_logmel(const float* wav, int B, int n_samples, const float* mel_basis, float* out, hipStream_t s) {
    const int n_frames = n_samples / 160;      // 1 + n/160 STFT frames, last one dropped (audio_utils.py:46)
    if (B <= 0 || n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(logmel_kernel, dim3(n_frames, B), dim3(256), 0, s, wav, n_samples, n_frames, mel_basis, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Face-mask + resize pre-step (inference_embs.py:235-276): per frame
//   face found : cv2.rectangle(img,(0,0),(W,y2+15),0,-1) at SOURCE resolution, then cv2.resize(img,(480,270))
//   face None  : cv2.resize first, then cv2.rectangle(img,(0,0),(480,110),0,-1)
// as ONE uint8 -> uint8 kernel (mask_y[f] >= 0: last blanked source row; -1: the face-None case).
// cv2.resize default = INTER_LINEAR on 8-bit: restated from OpenCV's generic fixed-point path
// (modules/imgproc/src/resize.cpp: coefficients cvRound(w*2048) as short, horizontal pass in int,
// vertical pass ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2).  cv2 is not installed here and the
// pip wheels may dispatch to IPP: PARITY UNPINNED (oracle/jegal_oracle.py:mask_resize_frames is the same
// restatement in numpy).
// Packed source (offs != nullptr): the producer ships only the source rows BELOW each frame's mask -- frame f's rows
// row0 = max(mask_y[f] + 1, 0) .. H-1 start at src + offs[f]; the blanked rows are never read here, so they need not exist.
// A frame whose kept rows would end beyond `src_bytes` (bad metadata) is written as zeros instead of being read.
// The arithmetic, written once for the two kernels below (they differ in how they stage the source, and must stay bit-identical):
__device__ inline int mr_sat_short(float v) {
    int r = __float2int_rn(v);
    return r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
}
// output column dx -> source columns sx, min(sx + 1, W - 1) with weights a0, a1 (scale_x = W / 480 in double; all three fit a short
// when W <= 32767: the banded kernel keeps them in LDS as such)
__device__ __forceinline__ void mr_col_coef(int dx, double scale_x, int W, int& sx, int& a0, int& a1) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    sx = (int)floorf(fx);
    fx -= sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx + 1 >= W) { fx = 0.f; sx = W - 1; }
    a0 = mr_sat_short((1.f - fx) * 2048.f);
    a1 = mr_sat_short(fx * 2048.f);
}
// output row dy -> source rows y0, y1 (clamped to the frame) with weights b0, b1 (scale_y = H / 270 in double)
__device__ inline void mr_row_coef(int dy, double scale_y, int H, int& y0, int& y1, int& b0, int& b1) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= sy;
    b0 = mr_sat_short((1.f - fy) * 2048.f);
    b1 = mr_sat_short(fy * 2048.f);
    y0 = sy < 0 ? 0 : (sy < H ? sy : H - 1);
    y1 = sy + 1 < 0 ? 0 : (sy + 1 < H ? sy + 1 : H - 1);
}
// the 8-bit blend of the four neighbours (rows y0 / y1 x columns sx / x1)
__device__ __forceinline__ uint8_t mr_blend(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
    const int S0 = p00 * a0 + p01 * a1, S1 = p10 * a0 + p11 * a1;
    const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
// the first source row a frame keeps: the one below its mask (face found), or row 0 (face None: the blank rows are cut AFTER the resize)
// (a macro: as a function it is simplified on its own before it is inlined, and the banded kernel's scalar code comes out in another order)
#define MR_FIRST_ROW(my, H) ((my) >= 0 ? ((my) + 1 < (H) ? (my) + 1 : (H)) : 0)
// Packed source: the frame's kept rows row0 .. H-1 start at src + o.  Where its row 0 would be (the rows above row0 do not exist and are
// never read), and whether the metadata is bad (the kept rows would start in front of src or end beyond src_bytes)
__device__ __forceinline__ const uint8_t* mr_packed_base(const uint8_t* __restrict__ src, long long o, int H, int W, int row0, long long src_bytes, bool& bad) {
    bad = o < 0 || o + (long long)(H - row0) * W * 3 > src_bytes;
    return src + o - (long long)row0 * W * 3;
}

__global__ void mask_resize_kernel(const uint8_t* __restrict__ src, int T, int H, int W, const int* __restrict__ mask_y,
                                   uint8_t* __restrict__ dst, const long long* __restrict__ offs, long long src_bytes) {
    constexpr int OH = 270, OW = 480;
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= (long)T * OH * OW) return;
    const int dx = (int)(idx % OW);
    const int dy = (int)((idx / OW) % OH);
    const int f = (int)(idx / ((long)OW * OH));
    const int my = mask_y[f];
    uint8_t* o = dst + idx * 3;
    if (my < 0 && dy <= 110) {                 // face None: rows 0..110 of the RESIZED frame (rectangle corners inclusive)
        o[0] = o[1] = o[2] = 0;
        return;
    }
    int sx, a0, a1, y0, y1, b0, b1;
    mr_col_coef(dx, (double)W / OW, W, sx, a0, a1);
    mr_row_coef(dy, (double)H / OH, H, y0, y1, b0, b1);
    const int x1 = sx + 1 < W ? sx + 1 : W - 1;
    const uint8_t* fr = src + (long)f * H * W * 3;
    bool bad = false;
    if (offs) fr = mr_packed_base(src, offs[f], H, W, MR_FIRST_ROW(my, H), src_bytes, bad);
    const bool z0 = bad || (my >= 0 && y0 <= my), z1 = bad || (my >= 0 && y1 <= my);       // blanked source rows
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int p00 = z0 ? 0 : fr[((long)y0 * W + sx) * 3 + c], p01 = z0 ? 0 : fr[((long)y0 * W + x1) * 3 + c];
        const int p10 = z1 ? 0 : fr[((long)y1 * W + sx) * 3 + c], p11 = z1 ? 0 : fr[((long)y1 * W + x1) * 3 + c];
        o[c] = mr_blend(p00, p01, p10, p11, a0, a1, b0, b1);
    }
}

// The same arithmetic (the mr_* functions above), banded (round 4: the streamed source-resolution upload runs this kernel on the upload stream next to the
// compute, so its cost is CU time taken from the extraction): one workgroup = RB output rows of one frame.  The source rows the
// band touches are one contiguous byte span of the frame: staged into LDS with dword loads (the span's start is aligned down, a
// tail of < 4 bytes is loaded bytewise, nothing outside [src, src + src_bytes) is touched), the per-column (sx, a1) and per-row
// (y0, y1, b1) coefficients are computed once per workgroup -- in double / float exactly as in mask_resize_kernel -- and the
// output rows leave through LDS as whole 16-byte pieces (a row is 1440 B).  Results are bit-identical to mask_resize_kernel
// (tests/test_gpu_drivers.py::test_mask_resize_matches_oracle runs both).
constexpr int MR_RB = 6;                       // output rows per workgroup (270 = 45 bands)
constexpr int MR_SPAN_MAX = 40 * 1024;         // LDS bytes for the source span; larger sources take the per-pixel kernel
__global__ __launch_bounds__(256) void mask_resize_band_kernel(const uint8_t* __restrict__ src, int T, int H, int W, const int* __restrict__ mask_y,
                                                               uint8_t* __restrict__ dst, const long long* __restrict__ offs, long long src_bytes) {
    constexpr int OH = 270, OW = 480, RB = MR_RB;
    extern __shared__ __attribute__((aligned(16))) uint8_t mr_smem[];          // [orow RB*1440][span: sized by the launcher]
    uint8_t* const orow = mr_smem;
    uint8_t* const span = mr_smem + RB * OW * 3;
    __shared__ short cx_s[OW], cx_a[OW];       // source column, a1 (a0 from the same float, see below)
    __shared__ short cx_a0[OW];
    __shared__ int ry0[RB], ry1[RB], rb0[RB], rb1[RB];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / (OH / RB), band = blockIdx.x - f * (OH / RB);
    const int dy0 = band * RB;
    const int my = mask_y[f];
    uint4* out16 = reinterpret_cast<uint4*>(dst + ((long)f * OH + dy0) * (OW * 3));
    constexpr int OUT_V = RB * OW * 3 / 16;    // 540 16-byte pieces
    const double scale_x = (double)W / OW, scale_y = (double)H / OH;
    // per-row coefficients (every thread computes the band's first / last source row itself: wave-uniform, no barrier needed for them)
    int ylo, yhi, t0, t1, t2;
    mr_row_coef(dy0, scale_y, H, ylo, t0, t1, t2);
    mr_row_coef(dy0 + RB - 1, scale_y, H, t0, yhi, t1, t2);
    // rows the band READS: those the frame keeps
    const int row0 = MR_FIRST_ROW(my, H);
    const int rlo = ylo > row0 ? ylo : row0;
    const uint8_t* fr = src + (long)f * H * W * 3;
    bool bad = false;
    if (offs) fr = mr_packed_base(src, offs[f], H, W, row0, src_bytes, bad);
    const bool none = bad || rlo > yhi || (my < 0 && dy0 + RB - 1 <= 110);      // nothing of the source reaches this band
    if (none) {
        for (int i = tid; i < OUT_V; i += 256) out16[i] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    // ---- stage the span [rlo, yhi] of the frame
    const uint8_t* p_lo = fr + (long)rlo * W * 3;
    const long nbytes = (long)(yhi - rlo + 1) * W * 3;
    const int shift = (int)((uintptr_t)p_lo & 3);
    const uint8_t* p_al = p_lo - shift;                        // >= the allocation's start: allocations are at least 4-byte aligned
    const long nfull = (shift + nbytes) >> 2;                  // whole dwords inside [p_al, p_lo + nbytes)
    for (long i = tid; i < nfull; i += 256) reinterpret_cast<uint32_t*>(span)[i] = reinterpret_cast<const uint32_t*>(p_al)[i];
    for (long i = nfull * 4 + tid; i < shift + nbytes; i += 256) span[i] = p_al[i];
    for (int dx = tid; dx < OW; dx += 256) {
        int sx, a0, a1;
        mr_col_coef(dx, scale_x, W, sx, a0, a1);
        cx_s[dx] = (short)sx;
        cx_a0[dx] = (short)a0;
        cx_a[dx] = (short)a1;
    }
    if (tid < RB) mr_row_coef(dy0 + tid, scale_y, H, ry0[tid], ry1[tid], rb0[tid], rb1[tid]);
    __syncthreads();
    const int rowb = W * 3;
    for (int i = tid; i < RB * OW; i += 256) {
        const int r = i / OW, dx = i - r * OW;
        uint8_t* o = orow + i * 3;
        if (my < 0 && dy0 + r <= 110) {                       // face None: rows 0..110 of the RESIZED frame
            o[0] = o[1] = o[2] = 0;
            continue;
        }
        const int y0 = ry0[r], y1 = ry1[r], b0 = rb0[r], b1 = rb1[r];
        const int sx = cx_s[dx], a0 = cx_a0[dx], a1 = cx_a[dx];
        const int x1 = sx + 1 < W ? sx + 1 : W - 1;
        const bool z0 = my >= 0 && y0 <= my, z1 = my >= 0 && y1 <= my;
        const uint8_t* q0 = span + shift + (long)(y0 - rlo) * rowb;
        const uint8_t* q1 = span + shift + (long)(y1 - rlo) * rowb;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int p00 = z0 ? 0 : q0[sx * 3 + c], p01 = z0 ? 0 : q0[x1 * 3 + c];
            const int p10 = z1 ? 0 : q1[sx * 3 + c], p11 = z1 ? 0 : q1[x1 * 3 + c];
            o[c] = mr_blend(p00, p01, p10, p11, a0, a1, b0, b1);
        }
    }
    __syncthreads();
    for (int i = tid; i < OUT_V; i += 256) out16[i] = reinterpret_cast<const uint4*>(orow)[i];
}

hipError_t launch_mask_resize(const uint8_t* src, int T, int H, int W, const int* mask_y_dev, uint8_t* dst, hipStream_t s,
                              const long long* offs, long long src_bytes) {
    const long n = (long)T * 270 * 480;
    if (n <= 0) return hipSuccess;
    // source rows a band of MR_RB output rows can touch: (MR_RB - 1) * H / 270 + 3
    const long span_rows = (long)(MR_RB - 1) * H / 270 + 3;
    static const bool generic = getenv("JG_MASK_RESIZE_GENERIC") != nullptr;       // A/B and test switch
    // (the banded kernel stages dword-aligned spans: it may read up to 3 bytes in front of a row that does not start on a dword, which
    // is inside the buffer as long as the buffer itself starts on one)
    if (span_rows * W * 3 + 4 <= MR_SPAN_MAX && W <= 32767 && !generic && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        const size_t lds = (size_t)MR_RB * 480 * 3 + (((size_t)span_rows * W * 3 + 4 + 15) & ~(size_t)15);
        hipLaunchKernelGGL(mask_resize_band_kernel, dim3((unsigned)(T * (270 / MR_RB))), dim3(256), lds, s, src, T, H, W, mask_y_dev, dst, offs, src_bytes);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(mask_resize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, T, H, W, mask_y_dev, dst, offs, src_bytes);
    return hipGetLastError();
}

// ---- masked crops over PCIe in fewer bytes ------------------------------------------------------------------
// The reference blanks rows 0 .. y2+15 of every crop (inference_embs.py:264-270): ~40 % of the bytes of a batch are zeros the
// engine then skips.  A producer ships only the rows BELOW each frame's mask, packed back to back; this kernel rebuilds the
// dense (frames, 270, 480, 3) batch: frame f's rows >= row0[f] come from packed + offs[f], the rows above are zero.
// Bad metadata (row0 outside 0..270, an offset that is negative, not a multiple of 16, or whose rows end beyond packed_bytes) makes
// the frame come out all zero instead of reading out of bounds / misaligned (packed_bytes < 0: unknown size, offsets are trusted).
__global__ __launch_bounds__(256) void unpack_masked_kernel(const uint8_t* __restrict__ packed, const int* __restrict__ row0,
                                                            const long long* __restrict__ offs, uint8_t* __restrict__ dst, long long packed_bytes) {
    constexpr int ROW_B = 480 * 3, ROW_V = ROW_B / 16, ROWS = 30;          // 90 16-byte pieces per row, 30 rows per block (9 blocks per frame)
    const int f = blockIdx.x;
    const int r_begin = blockIdx.y * ROWS;
    int r0 = row0[f];
    const long long of = offs[f];
    if (r0 < 0 || r0 > 270 || of < 0 || (of & 15) || (packed_bytes >= 0 && of + (long long)(270 - r0) * ROW_B > packed_bytes)) r0 = 270;
    const uint8_t* src = packed + of;
    uint8_t* out = dst + (size_t)f * (270 * ROW_B);
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    for (int i = threadIdx.x; i < ROWS * ROW_V; i += 256) {
        const int r = r_begin + i / ROW_V, c = i % ROW_V;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r >= r0) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + (size_t)(r - r0) * ROW_B) + c);
        reinterpret_cast<u32x4*>(out + (size_t)r * ROW_B)[c] = v;
    }
}

hipError_t launch_unpack_masked(const uint8_t* packed, const int* row0, const long long* offs, int n_frames, uint8_t* dst, hipStream_t s,
                                long long packed_bytes) {
    if (n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_masked_kernel, dim3((unsigned)n_frames, 9), dim3(256), 0, s, packed, row0, offs, dst, packed_bytes);
    return hipGetLastError();
}

// ---- compaction maps of the conv layers behind conv1 (common.h: ConvGeom::rowmap, ConvRowMap) ----------------------------------
// Image (position) img computes rows >= s = conv_skip_decode(s2[img], op) of a layer's OH x OW output.  Step 1, one workgroup:
// exclusive prefix of the images' computed pixels per layer (base[img], *total).  Step 2, one workgroup per image: its computed
// pixels (one contiguous run of full indices per layer) go to their compacted place as rowmap_entry(full index, s2).
struct RowMapArgs {
    const int* s2;
    int NF, nl;
    ConvRowMap L[4];
};
__global__ __launch_bounds__(1024) void conv_rowmap_scan_kernel(RowMapArgs a) {
    __shared__ int part[4][1024];
    const int tid = threadIdx.x;
    const int per = (a.NF + 1023) / 1024;                  // consecutive images per thread
    const int i0 = tid * per, i1 = i0 + per < a.NF ? i0 + per : a.NF;
    int sum[4] = {0, 0, 0, 0};
    for (int i = i0; i < i1; ++i) {
        const int w = a.s2[i];
#pragma unroll
        for (int l = 0; l < 4; ++l) sum[l] += (a.L[l].OH - conv_skip_decode(w, a.L[l].op)) * a.L[l].OW;
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) part[l][tid] = sum[l];
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                   // Hillis-Steele inclusive scan, the four layers side by side
        int v[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) v[l] = tid >= d ? part[l][tid - d] : 0;
        __syncthreads();
#pragma unroll
        for (int l = 0; l < 4; ++l) part[l][tid] += v[l];
        __syncthreads();
    }
    int run[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) run[l] = part[l][tid] - sum[l];
    for (int i = i0; i < i1; ++i) {
        const int w = a.s2[i];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (l < a.nl) a.L[l].base[i] = run[l];
            run[l] += (a.L[l].OH - conv_skip_decode(w, a.L[l].op)) * a.L[l].OW;
        }
    }
    if (tid == 1023) {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (l < a.nl) { a.L[l].base[a.NF] = part[l][1023]; *a.L[l].total = part[l][1023]; }
    }
}
// one workgroup per image: its computed pixels of every layer, in order
__global__ __launch_bounds__(256) void conv_rowmap_fill_kernel(RowMapArgs a) {
    const int img = blockIdx.x;
    const int w = a.s2[img];
    for (int l = 0; l < a.nl; ++l) {
        const ConvRowMap& R = a.L[l];
        const int s = conv_skip_decode(w, R.op);
        const int n = (R.OH - s) * R.OW;                   // computed pixels of this image: full rows s*OW .. OH*OW - 1
        const int first = img * R.OH * R.OW + s * R.OW;
        int* dst = R.map + R.base[img];
        for (int i = threadIdx.x; i < n; i += 256) dst[i] = rowmap_entry(first + i, w);
    }
}

hipError_t launch_conv_rowmaps(const int* s2, int NF, const ConvRowMap* layers, int nlayers, hipStream_t s) {
    if (NF <= 0 || nlayers <= 0 || nlayers > 4) return hipErrorInvalidValue;
    RowMapArgs a;
    a.s2 = s2; a.NF = NF; a.nl = nlayers;
    for (int l = 0; l < 4; ++l) {
        a.L[l] = layers[l < nlayers ? l : nlayers - 1];
        if ((long)NF * a.L[l].OH * a.L[l].OW >= ROWMAP_MAX_ROWS) return hipErrorInvalidValue;      // the row index of a map entry
    }
    record_kernel("conv_rowmap_scan_kernel+conv_rowmap_fill_kernel");
    hipLaunchKernelGGL(conv_rowmap_scan_kernel, dim3(1), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(conv_rowmap_fill_kernel, dim3((unsigned)NF), dim3(256), 0, s, a);
    return hipGetLastError();
}
