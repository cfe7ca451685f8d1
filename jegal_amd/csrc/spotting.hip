// Word spotting and gesture-word attention matrices (gfx950), the latter on exact-fp32 MFMA.
#include "metric_parts.h"

// ---------------------------------------------------------------------------------------------
// Word spotting (evaluate_spotting.py:39-82): per clip A = softmax((G C^T)/temp, dim=1) over words
// with re-normalised rows; pred = first argmax_t A[t][w*], score = A[pred][w*].
// One block per clip, one wave per frame row; the W logits of a row go through a per-wave LDS line.
// Limits: W <= SPOT_MAX_W words and T <= SPOT_MAX_T frames per clip (LDS arrays), 0 <= target < W.  The offsets are device
// arrays, so the host cannot check them without a sync: a clip outside the limits gets pred = -1, score = NaN.
__global__ __launch_bounds__(256) void spot_kernel(const float* __restrict__ g, const float* __restrict__ c,
                                                   const int32_t* __restrict__ goff, const int32_t* __restrict__ coff,
                                                   const int32_t* __restrict__ target, int D, float temp,
                                                   int32_t* __restrict__ pred, float* __restrict__ score) {
    __shared__ float sCn[SPOT_MAX_W];        // 1/max(||c_w||, eps)
    __shared__ float sL[4][SPOT_MAX_W];      // per wave: the logits of the frame it is working on
    __shared__ float sA[SPOT_MAX_T];         // A[t][w*]
    const int clip = blockIdx.x;
    const int t0 = goff[clip], T = goff[clip + 1] - t0;
    const int w0 = coff[clip], W = coff[clip + 1] - w0;
    const int wt = target[clip];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (T <= 0 || T > SPOT_MAX_T || W <= 0 || W > SPOT_MAX_W || wt < 0 || wt >= W) {      // block-uniform
        if (threadIdx.x == 0) { pred[clip] = -1; score[clip] = __builtin_nanf(""); }
        return;
    }
    for (int w = wave; w < W; w += 4) {
        float sq = 0.f;
        for (int d = lane; d < D; d += 64) { const float v = c[(long)(w0 + w) * D + d]; sq += v * v; }
        sq = wave_sum(sq);
        if (lane == 0) sCn[w] = 1.f / fmaxf(sqrtf(sq), 1e-12f);
    }
    __syncthreads();
    float* L = sL[wave];
    for (int t = wave; t < T; t += 4) {
        const float* gr = g + (long)(t0 + t) * D;
        float sq = 0.f;
        for (int d = lane; d < D; d += 64) { const float v = gr[d]; sq += v * v; }
        const float gn = 1.f / fmaxf(sqrtf(wave_sum(sq)), 1e-12f);
        for (int w = 0; w < W; ++w) {
            const float* cr = c + (long)(w0 + w) * D;
            float dot = 0.f;
            for (int d = lane; d < D; d += 64) dot += (gr[d] * gn) * (cr[d] * sCn[w]);
            dot = wave_sum(dot) / temp;
            if (lane == 0) L[w] = dot;
        }
        wave_lds_sync();
        float mx = -INFINITY;
        for (int w = lane; w < W; w += 64) mx = fmaxf(mx, L[w]);
        mx = wmax(mx);
        float e = 0.f;
        for (int w = lane; w < W; w += 64) e += expf(L[w] - mx);
        const float den = wave_sum(e);
        const float a = expf(L[wt] - mx) / den;
        if (lane == 0) sA[t] = a;
        __builtin_amdgcn_wave_barrier();         // L is rewritten for the next frame
    }
    __syncthreads();
    if (wave == 0) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int t = lane; t < T; t += 64) {
            const float a = sA[t];
            if (a > best) { best = a; bi = t; }      // strided scan keeps the first index per lane
        }
        wave_best_first(best, bi);
        if (lane == 0) { pred[clip] = bi; score[clip] = best; }
    }
}

hipError_t launch_spot(const float* g, const float* c, const int32_t* goff, const int32_t* coff, const int32_t* target,
                       int n, int D, float temp, int32_t* pred, float* score, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(spot_kernel, dim3(n), dim3(256), 0, s, g, c, goff, coff, target, D, temp, pred, score);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Attention matrices (evaluate_spotting.py:39-57 with normalize, utils/plot_heatmap.py:34-59 without): per clip
// A = softmax((G C^T)/temp, dim=1)^T, shape (W, T), and for EVERY word its first arg-max frame and that probability
// (evaluate_spotting.py:72-73).  The logits run on v_mfma_f32_32x32x2_f32 as in sim_rank_kernel, content rows as the A operand and
// gesture rows as the B operand: a register of the 32x32 accumulator is one word x 32 consecutive frames per lane half, so a
// row of the (W, T) output leaves as 128-byte segments and the softmax over the words is a reduction over the lane's own
// registers plus one __shfl_xor(., 32).  A logit depends on its two rows alone (k-ordered fmaf chains of AM_KSPLIT terms summed
// in order, rows pre-scaled by 1 / max(||row||, 1e-12) when they are staged), so duplicate frames give bit-equal columns whatever
// tile they fall in.
//
// Grid = (clip, block of AM_FB frames).  Two forms = two instances, both launched over every clip (the host cannot see the word
// counts); a workgroup leaves at once when the clip belongs to the other one, so that the common form keeps its registers low:
//   W <= AM_REG_W: a wave owns 32 frames and all words (up to 4 accumulators); nothing is exchanged between waves.
//   wider:         the four waves share 32 frames at a time and deal the word tiles round-robin (up to 8 accumulators each);
//                  the per-frame max and sum cross the waves through 1 KB of LDS in a fixed order.
// The per-word arg-max is combined across waves and frame blocks by a 64-bit atomicMax on (probability bits, ~frame):
// order-independent, and on equal probabilities the smaller frame wins (np.argmax's first index).  attn_keys_init_kernel
// zeroes the keys of the clips inside the limits, attn_best_kernel decodes them (and marks the clips outside).
//
// The parts, each defined once and shared with the talk form below (jg_attn_talk), whose logits, softmax and keys therefore have the
// bits these kernels give the same rows:
//   am_row_scales                the staging factors of the content and gesture rows
//   am_stage, am_mfma, am_fold   one k chunk into LDS, its MFMAs, the cut of the k-ordered chains
//   am_reg_logits                the in-register form's k loop over those three: the logits of 128 words x the wave's 32 frames
//   am_softmax                   exp(x / temp - max) and its sum over the entries a mask admits
//   am_key_max                   a word's best frame among the wave's 32 into its key; argmax_key_decode reads a key back
// attn_matrix_kernel<false> = am_row_scales, am_reg_logits, am_finish<4, 1>; attn_matrix_kernel<true> = am_row_scales, then per frame
// tile its own k loop (8 k at a time over all words) and am_finish<8, 4>.  am_finish = am_softmax over the words that exist, the stores
// into the (W, T) matrix, am_key_max.
constexpr int AM_FB = 128;                   // frames per workgroup
constexpr int AM_REG_W = 128;                // widest clip of the in-register form
constexpr int AM_KEY_PITCH = SPOT_MAX_W;     // keys[clip][word]: the host cannot know sum W (the offsets are device arrays)

size_t attn_matrix_key_elems(int n_clips) { return (size_t)n_clips * AM_KEY_PITCH; }
// The arg-max key of a word: (fp32 bits of the probability << 32) | ~frame, so that a 64-bit max prefers the larger probability and then
// the smaller frame; 0 = no frame yet.
__device__ __forceinline__ unsigned long long argmax_key(float prob, unsigned frame) {
    return ((unsigned long long)__float_as_uint(prob) << 32) | (0xffffffffu - frame);
}
__device__ __forceinline__ int32_t argmax_key_frame(unsigned long long key) { return (int32_t)(0xffffffffu - (unsigned)key); }
__device__ __forceinline__ float argmax_key_prob(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }
// key -> best_frame[at] / best_score[at] (either may be null); no frame: -1 / NaN
__device__ __forceinline__ void argmax_key_decode(unsigned long long key, int32_t* __restrict__ best_frame, float* __restrict__ best_score,
                                                  long at) {
    if (best_frame) best_frame[at] = key ? argmax_key_frame(key) : -1;
    if (best_score) best_score[at] = key ? argmax_key_prob(key) : __builtin_nanf("");
}

__device__ __forceinline__ bool attn_clip_ok(int T, int W, int max_frames) {
    return T > 0 && T <= SPOT_MAX_T && T <= max_frames && W > 0 && W <= SPOT_MAX_W;
}

// sCn[w] / sGn[f] = the factor that content row w < nw / gesture row f < nf is staged with: 1 / max(||row||, 1e-12), or 1
__device__ __forceinline__ void am_row_scales(const float* __restrict__ crow, int nw, const float* __restrict__ grow, int nf, int D,
                                              int normalize, float* sCn, float* sGn, int lane, int wave) {
    for (int w = wave; w < nw; w += 4) {
        const float rn = normalize ? row_rnorm(crow + (long)w * D, D, lane) : 1.f;
        if (lane == 0) sCn[w] = rn;
    }
    for (int f = wave; f < nf; f += 4) {
        const float rn = normalize ? row_rnorm(grow + (long)f * D, D, lane) : 1.f;
        if (lane == 0) sGn[f] = rn;
    }
}

// rows r0, r0 + rstep, .. < npad of `rows`, columns k0 .. k0 + KC - 1, scaled by rinv[r], into dst[k][r] (pitch floats per k);
// rows >= nvalid are zero
template <int KC>
__device__ __forceinline__ void am_stage(const float* __restrict__ rows, int D, int k0, int nvalid, int npad, const float* rinv,
                                         float* dst, int pitch, int r0, int rstep) {
    for (int r = r0; r < npad; r += rstep) {
        const bool ok = r < nvalid;
        const float s = ok ? rinv[r] : 0.f;
        const float* src = rows + (long)r * D + k0;
#pragma unroll
        for (int q = 0; q < KC / 4; ++q) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(src + q * 4);
            float* d = dst + (q * 4) * pitch + r;
            d[0] = v.x * s; d[pitch] = v.y * s; d[2 * pitch] = v.z * s; d[3 * pitch] = v.w * s;
        }
    }
}

// KC k-steps of the wave's accumulators: accumulator i is word tile tbase + i * TSTEP against the 32 frames at column gcol of sG
template <int NT, int TSTEP, int KC, int CP, int GP>
__device__ __forceinline__ void am_mfma(const float* sC, const float* sG, int tbase, int ntile, int gcol, int lane, f32x16 (&acc)[NT]) {
#pragma unroll
    for (int kk = 0; kk < KC; kk += 2) {
        const int kr = kk + (lane >> 5);
        const float b = sG[kr * GP + gcol + (lane & 31)];
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (tbase + i * TSTEP < ntile) {
                const float a = sC[kr * CP + (tbase + i * TSTEP) * 32 + (lane & 31)];
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
            }
    }
}

// The k-ordered chain of an accumulator is cut every AM_KSPLIT terms: tot += acc in fp32, acc = 0.  Rounding errors of a chain grow
// with its length; four chains of 128 terms summed in order come out at 0.3-0.5 of one chain of 512 (CPU emulation against float64),
// which is what keeps the probabilities inside 4 x the blocked fp32 reference's own error.  An entry still depends on its two rows alone.
constexpr int AM_KSPLIT = 128;
template <int NT>
__device__ __forceinline__ void am_fold(f32x16 (&acc)[NT], f32x16 (&tot)[NT]) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) { tot[i][x] += acc[i][x]; acc[i][x] = 0.f; }
}

// The in-register form's logits: tot = <content row, gesture row> over all of D for the nw <= 128 words at crow against the wave's 32 of
// the nf <= 128 frames at grow.  sC / sG: 32 k of [k][word] / [k][frame] staging with pitches CP / GP.
template <int CP, int GP>
__device__ __forceinline__ void am_reg_logits(const float* __restrict__ crow, int nw, const float* __restrict__ grow, int nf, int D,
                                              const float* sCn, const float* sGn, float* sC, float* sG, int tid, f32x16 (&tot)[4]) {
    const int lane = tid & 63, wave = tid >> 6;
    const int ntile = (nw + 31) >> 5;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) { acc[i][x] = 0.f; tot[i][x] = 0.f; }
    const bool active = wave * 32 < nf;
    for (int k0 = 0; k0 < D; k0 += 32) {
        __syncthreads();
        if (tid < 128) am_stage<32>(crow, D, k0, nw, ntile * 32, sCn, sC, CP, tid, 128);
        else am_stage<32>(grow, D, k0, nf, (nf + 31) & ~31, sGn, sG, GP, tid - 128, 128);
        __syncthreads();
        if (active) am_mfma<4, 1, 32, CP, GP>(sC, sG, 0, ntile, wave * 32, lane, acc);
        if ((k0 + 32) % AM_KSPLIT == 0 || k0 + 32 == D) am_fold<4>(acc, tot);
    }
}

// The softmax over the words of the lane's frame as torch evaluates it, exp(x - max) / sum exp(x - max), up to the division:
// acc[i][x] <- in(i, x) ? exp(acc[i][x] / temp - max) : 0, returns the sum.  in(i, x): accumulator i, register x takes part; the same value
// at every call.  An entry outside adds exactly 0 to the sum and takes no part in the maximum.  Accumulator layout: frame = lane & 31,
// word = 32 tile + mfma32_row(x, lane >> 5).  TSTEP > 1: the four waves hold different words of the SAME frames, every wave of the
// workgroup makes this call, and max and sum cross the waves through sRed in a fixed order (TSTEP == 1 reads neither sRed nor wave).
template <int NT, int TSTEP, class In>
__device__ __forceinline__ float am_softmax(f32x16 (&acc)[NT], float temp, In in, float (*sRed)[4][32], int lane, int wave) {
    const int h = lane >> 5, l31 = lane & 31;
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            acc[i][x] = acc[i][x] / temp;
            if (in(i, x)) mx = fmaxf(mx, acc[i][x]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if constexpr (TSTEP > 1) {
        if (h == 0) sRed[0][wave][l31] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(sRed[0][0][l31], sRed[0][1][l31]), fmaxf(sRed[0][2][l31], sRed[0][3][l31]));
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const float e = in(i, x) ? expf(acc[i][x] - mx) : 0.f;
            acc[i][x] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32, 64);
    if constexpr (TSTEP > 1) {
        if (h == 0) sRed[1][wave][l31] = sum;
        __syncthreads();
        sum = ((sRed[1][0][l31] + sRed[1][1][l31]) + sRed[1][2][l31]) + sRed[1][3][l31];
    }
    return sum;
}

// A word's first frame with the largest probability among the wave's 32 (frame0 ..) into its key at `slot`: max over the lane half (lanes
// without `valid` count as -1), then the lowest lane that holds it.  Every lane of the wave makes the call with its own p of the same word;
// word_ok: the half's word exists.
__device__ __forceinline__ void am_key_max(unsigned long long* slot, float p, bool valid, bool word_ok, int frame0, int lane) {
    const int h = lane >> 5, l31 = lane & 31;
    float m = valid ? p : -1.f;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const unsigned long long bal = __ballot(valid && p == m);
    const unsigned mine = (unsigned)(bal >> (32 * h));
    if (l31 == 0 && word_ok && mine) atomicMax(slot, argmax_key(m, frame0 + __ffs(mine) - 1));
}

// The clip form's end for the wave's 32 frames (frame0 ..): the softmax over the clip's words, the stores into the (W, T) matrix and the
// arg-max keys.  Accumulator i is word tile tbase + i * TSTEP.
template <int NT, int TSTEP>
__device__ __forceinline__ void am_finish(f32x16 (&acc)[NT], int tbase, int W, int T, int frame0, float temp, float* __restrict__ Aclip,
                                          unsigned long long* __restrict__ kclip, float (*sRed)[4][32], int lane, int wave) {
    // Everything below that depends only on W, T and the lane is invariant in the wide form's frame-tile loop; hoisted out of it, the
    // word predicates and store offsets of 128 registers spill.  An empty asm keeps them inside.
    asm volatile("" : "+s"(W), "+s"(T));
    const int h = lane >> 5, l31 = lane & 31;
    const int frame = frame0 + l31;
    const bool fok = frame < T;
    const int wl = W - 4 * h - tbase * 32;           // accumulator i, register x holds a word of the clip iff roff(x) < wl - 32 i TSTEP
    const float sum = am_softmax<NT, TSTEP>(acc, temp, [&](int i, int x) { return mfma32_row(x, 0) < wl - i * TSTEP * 32; }, sRed, lane, wave);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int tile = tbase + i * TSTEP;
        if (tile * 32 < W) {                                         // wave-uniform: the tile holds a word
            const int word0 = tile * 32 + 4 * h;
            float* Arow = Aclip ? Aclip + ((long)word0 * T + frame) : nullptr;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int roff = mfma32_row(x, 0);
                const bool wok = roff < wl - i * TSTEP * 32;
                const float p = acc[i][x] / sum;
                if (Aclip && fok && wok) Arow[roff * T] = p;          // W T <= 2^23 elements per clip
                if (kclip) am_key_max(&kclip[word0 + roff], p, fok, wok, frame0, lane);
            }
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void attn_matrix_kernel(const float* __restrict__ g, const float* __restrict__ c,
                                                          const int32_t* __restrict__ goff, const int32_t* __restrict__ coff, int D,
                                                          int max_frames, float temp, int normalize, float* __restrict__ A,
                                                          const int64_t* __restrict__ aoff, unsigned long long* __restrict__ keys) {
    __shared__ float sC[8192];               // content chunk [k][word]: 32 x 128 (in-register form) or 8 x 1024 (wide form)
    __shared__ float sG[4096];               // gesture chunk [k][frame]: 32 x 128 or 8 x 32
    __shared__ float sCn[SPOT_MAX_W];        // 1 / max(||c_w||, eps), or 1
    __shared__ float sGn[AM_FB];
    __shared__ float sRed[2][4][32];         // wide form: per wave and frame, max and sum over the wave's words
    const int clip = blockIdx.x, f0 = blockIdx.y * AM_FB;
    const int t0 = goff[clip], T = goff[clip + 1] - t0;
    const int w0 = coff[clip], W = coff[clip + 1] - w0;
    if (!attn_clip_ok(T, W, max_frames) || f0 >= T || (W > AM_REG_W) != WIDE) return;          // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = T - f0 < AM_FB ? T - f0 : AM_FB;
    const float* crow = c + (long)w0 * D;
    const float* grow = g + (long)(t0 + f0) * D;
    am_row_scales(crow, W, grow, nf, D, normalize, sCn, sGn, lane, wave);
    float* Aclip = A ? A + aoff[clip] : nullptr;
    unsigned long long* kclip = keys ? keys + (size_t)clip * AM_KEY_PITCH : nullptr;

    if constexpr (!WIDE) {
        f32x16 tot[4];
        am_reg_logits<128, AM_FB>(crow, W, grow, nf, D, sCn, sGn, sC, sG, tid, tot);
        if (wave * 32 < nf) am_finish<4, 1>(tot, 0, W, T, f0 + wave * 32, temp, Aclip, kclip, sRed, lane, wave);
    } else {
        const int ntile = (W + 31) >> 5;
        for (int ft = 0; ft * 32 < nf; ++ft) {
            f32x16 acc[8], tot[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int x = 0; x < 16; ++x) { acc[i][x] = 0.f; tot[i][x] = 0.f; }
            const int nfr = nf - ft * 32 < 32 ? nf - ft * 32 : 32;
            for (int k0 = 0; k0 < D; k0 += 8) {
                __syncthreads();
                am_stage<8>(crow, D, k0, W, ntile * 32, sCn, sC, SPOT_MAX_W, tid, 256);
                am_stage<8>(grow + (long)ft * 32 * D, D, k0, nfr, 32, sGn + ft * 32, sG, 32, tid, 256);
                __syncthreads();
                am_mfma<8, 4, 8, SPOT_MAX_W, 32>(sC, sG, wave, ntile, 0, lane, acc);
                if ((k0 + 8) % AM_KSPLIT == 0 || k0 + 8 == D) am_fold<8>(acc, tot);
            }
            am_finish<8, 4>(tot, wave, W, T, f0 + ft * 32, temp, Aclip, kclip, sRed, lane, wave);
        }
    }
}

__global__ void attn_keys_init_kernel(const int32_t* __restrict__ goff, const int32_t* __restrict__ coff, int max_frames,
                                      unsigned long long* __restrict__ keys) {
    const int clip = blockIdx.x;
    const int T = goff[clip + 1] - goff[clip], W = coff[clip + 1] - coff[clip];
    if (!attn_clip_ok(T, W, max_frames)) return;
    for (int w = threadIdx.x; w < W; w += blockDim.x) keys[(size_t)clip * AM_KEY_PITCH + w] = 0ull;
}

// keys -> best_frame / best_score (either may be null); the words of a clip outside the limits read -1 / NaN
__global__ void attn_best_kernel(const int32_t* __restrict__ goff, const int32_t* __restrict__ coff, int max_frames,
                                 const unsigned long long* __restrict__ keys, int32_t* __restrict__ best_frame,
                                 float* __restrict__ best_score) {
    const int clip = blockIdx.x;
    const int T = goff[clip + 1] - goff[clip];
    const int w0 = coff[clip], W = coff[clip + 1] - w0;
    const bool ok = attn_clip_ok(T, W, max_frames);
    for (int w = threadIdx.x; w < W; w += blockDim.x)
        argmax_key_decode(ok ? keys[(size_t)clip * AM_KEY_PITCH + w] : 0ull, best_frame, best_score, w0 + w);
}

hipError_t launch_attn_matrix(const float* g, const float* c, const int32_t* goff, const int32_t* coff, int n, int D, int max_frames,
                              float temp, int normalize, float* A, const int64_t* aoff, unsigned long long* keys,
                              int32_t* best_frame, float* best_score, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (D <= 0 || D % 64 || max_frames < 1 || max_frames > SPOT_MAX_T || (A && !aoff) || (!A && !keys) ||
        ((best_frame || best_score) && !keys))
        return hipErrorInvalidValue;
    if (keys) hipLaunchKernelGGL(attn_keys_init_kernel, dim3(n), dim3(256), 0, s, goff, coff, max_frames, keys);
    const dim3 grid(n, (max_frames + AM_FB - 1) / AM_FB);
    hipLaunchKernelGGL(attn_matrix_kernel<false>, grid, dim3(256), 0, s, g, c, goff, coff, D, max_frames, temp, normalize, A, aoff, keys);
    hipLaunchKernelGGL(attn_matrix_kernel<true>, grid, dim3(256), 0, s, g, c, goff, coff, D, max_frames, temp, normalize, A, aoff, keys);
    if (keys) hipLaunchKernelGGL(attn_best_kernel, dim3(n), dim3(256), 0, s, goff, coff, max_frames, keys, best_frame, best_score);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The heat map along a whole talk (jg_attn_talk).  A track has T frame rows and W word rows in transcript order with inclusive frame
// bounds [start_w, end_w]; word w is IN REACH of frame f iff start_w - reach <= f <= end_w + reach, and
//   P[w][f] = exp(x_wf - m_f) / sum over the words in reach of f of exp(x_w'f - m_f),  x = <c_w, g_f> / temp,  m_f = the max over those words:
// every frame sees the words a clip of 2 reach + 1 frames centred on it would contain.
// Grid = (track, block of TALK_FB frames, aligned to the track's first frame); the block's CANDIDATES are the words in reach of any of
// its frames -- the bounds are non-decreasing, so they are one contiguous range [lo, hi) found by two binary searches on block-uniform
// values.  attn_talk_kernel = the two searches, am_row_scales and am_reg_logits with the candidates as the words (a wave owns 32 frames
// and all candidates), talk_finish.  talk_finish = am_softmax over the words in reach of the lane's frame, the stores into the band rows,
// am_key_max, and the frame's best word.  With every word in reach the mask is am_finish's, so the probabilities, best frames and best
// scores are jg_attn_matrix's bit for bit.
// A block with more than TALK_MAX_BLOCK_W candidates is UNDECIDED in all its frames.  attn_talk_fill_kernel writes the undecided values
// (NaN band, -1 / NaN frames, zero keys) everywhere first; the blocks overwrite what they decide; attn_talk_best_kernel decodes the keys.
constexpr int TALK_FB = 128;                 // frames per workgroup

// the track's rows and words, or false = the track is UNDECIDED as a whole (nothing of it is read)
__device__ __forceinline__ bool talk_track(int trk, const int32_t* __restrict__ goff, long n_rows, int max_frames,
                                           const int32_t* __restrict__ coff, int n_words, int& t0, int& T, int& w0, int& W) {
    t0 = goff[trk]; w0 = coff[trk];
    const long Tl = (long)goff[trk + 1] - t0, Wl = (long)coff[trk + 1] - w0;
    const bool ok = t0 >= 0 && Tl >= 0 && Tl <= max_frames && t0 + Tl <= n_rows && w0 >= 0 && Wl >= 0 && w0 + Wl <= n_words;
    T = ok ? (int)Tl : 0; W = ok ? (int)Wl : 0;
    return ok;
}
// the first w in [first, W) with v[w] + add >= bound, W when there is none (v non-decreasing; whatever v holds, the result is in [first, W])
__device__ __forceinline__ int talk_lower_bound(const int32_t* __restrict__ v, int first, int W, long add, long bound) {
    int a = first, b = W;
    while (a < b) {
        const int m = a + ((b - a) >> 1);
        if ((long)v[m] + add >= bound) b = m; else a = m + 1;
    }
    return a;
}

// The talk form's end for the wave's 32 frames (frame0 ..) against the block's NC candidates, entry (word, frame) taking part iff
// sLo[word] <= frame <= sHi[word] (an empty interval beyond the candidates).  bandw / kw / fw / fp: the outputs (any may be null) at
// the block's first candidate / the track's first frame; lo = the first candidate's index inside the track.
__device__ __forceinline__ void talk_finish(f32x16 (&acc)[4], int NC, int T, int frame0, float temp, const int* sLo, const int* sHi,
                                            float* __restrict__ bandw, int pitch, unsigned long long* __restrict__ kw,
                                            int32_t* __restrict__ fw, float* __restrict__ fp, int lo, int lane) {
    const int h = lane >> 5;
    const int frame = frame0 + (lane & 31);
    const bool fok = frame < T;
    unsigned in[4];                              // bit x of in[i]: accumulator i, register x is a word in reach of the lane's frame
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        in[i] = 0u;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int word = i * 32 + mfma32_row(x, 0) + 4 * h;
            if (fok && sLo[word] <= frame && frame <= sHi[word]) in[i] |= 1u << x;
        }
    }
    const float sum = am_softmax<4, 1>(acc, temp, [&](int i, int x) { return (in[i] >> x & 1) != 0; }, nullptr, lane, 0);
    float bp = -1.f;                             // the lane's best word so far: registers come in ascending word order, > keeps the first
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i * 32 < NC) {                                               // wave-uniform: the tile holds a candidate
            const int word0 = i * 32 + 4 * h;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int word = word0 + mfma32_row(x, 0);
                const bool inb = in[i] >> x & 1;
                const float p = acc[i][x] / sum;
                if (inb && p > bp) { bp = p; bi = word; }
                if (bandw && inb) {
                    const long j = (long)frame - sLo[word];                  // >= 0: the word is in reach
                    if (j < pitch) bandw[(long)word * pitch + j] = p;        // n_words * pitch < 2^31
                }
                if (kw) am_key_max(&kw[word], p, inb, word < NC, frame0, lane);
            }
        }
    }
    if (fw || fp) {
        wave_best_first<32>(bp, bi);                                     // the two halves hold different words of the same frame
        if (h == 0 && fok && bi != 0x7fffffff) {                         // (no word in reach: the frame keeps -1 / NaN)
            if (fw) fw[frame] = lo + bi;
            if (fp) fp[frame] = bp;
        }
    }
}

__global__ __launch_bounds__(256) void attn_talk_kernel(const float* __restrict__ g, const int32_t* __restrict__ goff, long n_rows,
                                                        int max_frames, const float* __restrict__ c, const int32_t* __restrict__ coff,
                                                        int n_words, const int32_t* __restrict__ wstart, const int32_t* __restrict__ wend,
                                                        int D, int reach, float temp, int normalize, float* __restrict__ band, int pitch,
                                                        unsigned long long* __restrict__ keys, int32_t* __restrict__ frame_word,
                                                        float* __restrict__ frame_prob) {
    __shared__ float sC[32 * TALK_MAX_BLOCK_W];      // content chunk [k][candidate]
    __shared__ float sG[32 * TALK_FB];               // gesture chunk [k][frame]
    __shared__ float sCn[TALK_MAX_BLOCK_W];          // 1 / max(||c_w||, eps), or 1
    __shared__ float sGn[TALK_FB];
    __shared__ int sLo[TALK_MAX_BLOCK_W], sHi[TALK_MAX_BLOCK_W];      // start - reach / end + reach per candidate; empty beyond them
    const int trk = blockIdx.x, f0 = blockIdx.y * TALK_FB;
    int t0, T, w0, W;
    if (!talk_track(trk, goff, n_rows, max_frames, coff, n_words, t0, T, w0, W) || f0 >= T) return;       // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = T - f0 < TALK_FB ? T - f0 : TALK_FB;
    // candidates [lo, hi): end_w + reach >= f0 and start_w - reach <= f0 + nf - 1; both searches stay inside the track's words
    const int lo = talk_lower_bound(wend + w0, 0, W, reach, f0);
    const int hi = talk_lower_bound(wstart + w0, lo, W, -(long)reach, (long)f0 + nf);
    const int NC = hi - lo;
    if (NC <= 0 || NC > TALK_MAX_BLOCK_W) return;                        // no word in reach of any frame | UNDECIDED
    const float* crow = c + (long)(w0 + lo) * D;
    const float* grow = g + (long)(t0 + f0) * D;
    am_row_scales(crow, NC, grow, nf, D, normalize, sCn, sGn, lane, wave);
    if (tid < TALK_MAX_BLOCK_W) {
        // clamped to int32: frames are < 2^20, so neither comparison changes, and a band index taken from a clamped bound is >= 2^31 - 1
        long a = 0x7fffffffL, b = -0x80000000L;
        if (tid < NC) { a = (long)wstart[w0 + lo + tid] - reach; b = (long)wend[w0 + lo + tid] + reach; }
        sLo[tid] = (int)(a < -0x7fffffffL ? -0x7fffffffL : a > 0x7fffffffL ? 0x7fffffffL : a);
        sHi[tid] = (int)(b < -0x80000000L ? -0x80000000L : b > 0x7fffffffL ? 0x7fffffffL : b);
    }
    f32x16 tot[4];
    am_reg_logits<TALK_MAX_BLOCK_W, TALK_FB>(crow, NC, grow, nf, D, sCn, sGn, sC, sG, tid, tot);
    if (wave * 32 < nf)
        talk_finish(tot, NC, T, f0 + wave * 32, temp, sLo, sHi, band ? band + (long)(w0 + lo) * pitch : nullptr, pitch,
                    keys ? keys + w0 + lo : nullptr, frame_word ? frame_word + t0 : nullptr, frame_prob ? frame_prob + t0 : nullptr, lo, lane);
}

// the undecided values, everywhere (each output may be null)
__global__ void attn_talk_fill_kernel(float* __restrict__ band, long band_elems, unsigned long long* __restrict__ keys, int n_words,
                                      int32_t* __restrict__ frame_word, float* __restrict__ frame_prob, long n_rows) {
    const long step = (long)gridDim.x * blockDim.x, first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const float nan = __builtin_nanf("");
    if (band)
        for (long e = first; e < band_elems; e += step) band[e] = nan;
    if (keys)
        for (long e = first; e < n_words; e += step) keys[e] = 0ull;
    for (long e = first; e < n_rows; e += step) {
        if (frame_word) frame_word[e] = -1;
        if (frame_prob) frame_prob[e] = nan;
    }
}

// keys -> best_frame / best_score (either may be null); a word without a decided frame reads -1 / NaN
__global__ void attn_talk_best_kernel(const unsigned long long* __restrict__ keys, int n_words, int32_t* __restrict__ best_frame,
                                      float* __restrict__ best_score) {
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (long)gridDim.x * blockDim.x)
        argmax_key_decode(keys[w], best_frame, best_score, w);
}

hipError_t launch_attn_talk(const float* g, const int32_t* goff, int n_tracks, long n_rows, int max_frames, const float* c,
                            const int32_t* coff, int n_words, const int32_t* wstart, const int32_t* wend, int D, int reach, float temp,
                            int normalize, float* band, int band_pitch, unsigned long long* keys, int32_t* best_frame, float* best_score,
                            int32_t* frame_word, float* frame_prob, hipStream_t s) {
    if (n_tracks <= 0) return hipSuccess;
    const long band_elems = band ? (long)n_words * band_pitch : 0;
    if (D <= 0 || D % 64 || max_frames < 1 || max_frames > TALK_MAX_T || reach < 0 || reach > TALK_MAX_REACH || n_rows < 0 || n_words < 0 ||
        !(temp > 0.f) || (band && (band_pitch < 1 || band_elems > 0x7fffffffL)) || ((best_frame || best_score) && !keys) ||
        (!band && !keys && !frame_word && !frame_prob))
        return hipErrorInvalidValue;
    record_kernel("attn_talk_fill_kernel+attn_talk_kernel+attn_talk_best_kernel");
    long most = band_elems > n_rows ? band_elems : n_rows;
    most = most > n_words ? most : n_words;
    if (most > 0)
        hipLaunchKernelGGL(attn_talk_fill_kernel, dim3(grid_for(most)), dim3(256), 0, s, band, band_elems, keys, n_words, frame_word, frame_prob,
                           n_rows);
    hipLaunchKernelGGL(attn_talk_kernel, dim3(n_tracks, (max_frames + TALK_FB - 1) / TALK_FB), dim3(256), 0, s, g, goff, n_rows, max_frames, c,
                       coff, n_words, wstart, wend, D, reach, temp, normalize, band, band_pitch, keys, frame_word, frame_prob);
    if (keys && n_words > 0)
        hipLaunchKernelGGL(attn_talk_best_kernel, dim3(grid_for(n_words)), dim3(256), 0, s, keys, n_words, best_frame, best_score);
    return hipGetLastError();
}
