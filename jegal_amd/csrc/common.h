// Per-build device/host declarations for libjegal_hip (gfx950 only): everything that depends on the 16-bit operand type.
//
// Two builds of the kernels live in the library: the default one with fp16 operands and, for precision mode JG_PREC_BF16, a
// second one of gemm.hip / attention.hip / elementwise.hip compiled with -DJG_BF16: there `f16` -- the 16-bit operand /
// activation type of every kernel -- is __bf16, the MFMA macros below name the bf16 instructions, and everything in this header
// sits in namespace bf.  engine.h includes this header twice and dispatches per handle (LAUNCH in engine.h).
// The rule: a launcher, kernel or struct exists in namespace bf if and only if it depends on the 16-bit operand type AND some
// call site dispatches it with LAUNCH.  Everything else exists once, in the global namespace: what has no 16-bit operand is
// declared in shared.h (kernels: elementwise_f32.hip), what only the fp16 paths reach in the block at the end of this header
// (kernels: elementwise_fp16.hip, conv1.hip).  A new kernel goes into a two-build unit only if a bf16 handle launches it.
#include "shared.h"

#if (defined(JG_BF16) && !defined(JG_COMMON_BF16_INCLUDED)) || (!defined(JG_BF16) && !defined(JG_COMMON_FP16_INCLUDED))
#undef JG_NS_BEGIN
#undef JG_NS_END
#undef JG_MFMA_16x16x32
#undef JG_MFMA_32x32x16
#ifdef JG_BF16
#define JG_COMMON_BF16_INCLUDED
#define JG_NS_BEGIN namespace bf {
#define JG_NS_END }
namespace bf {
typedef __bf16 f16;
#define JG_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define JG_MFMA_32x32x16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
#else
#define JG_COMMON_FP16_INCLUDED
#define JG_NS_BEGIN
#define JG_NS_END
typedef _Float16 f16;
#define JG_MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#define JG_MFMA_32x32x16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
#endif
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Geometry of an NHWC implicit-GEMM convolution (C must be a power of two >= 8).
struct ConvGeom {
    int H, W, C;          // input spatial size and channels
    int OH, OW;           // output spatial size
    int KH, KW, SH, SW, PH, PW;
    int cshift;           // log2(C)
    // K order of the taps: k = (p, c) with tap p -> (kh, kw) = taps byte p (kh << 4 | kw), or the natural
    // p = kh*KW + kw when tap_table == 0.  Strided layers list their taps by parity class (kh % SH, kw % SW):
    // consecutive taps of a class touch the same input pixels shifted by whole output positions, so the re-reads
    // of a k-loop hit the L2 instead of thrashing it (conv2: 25 taps, 4 classes of 9/6/6/4).  The packed weights
    // use the same order (linear.hip:make_conv).
    unsigned long long taps[4];
    int tap_table;
    // ---- position-independent leading rows (LDS-DMA conv kernels ONLY: gestsync.hip sets these for launches that take that path).
    // Behind conv1's zero-band skip (conv1.hip) the first rows of every layer's output do not depend on the position at all:
    // they are what the layer computes from an all-constant input image, and the engine keeps those images per weight load
    // ("const chain", gestsync.hip).  PER POSITION (image) p, conv2 leaves its first s2[p] output rows out and every deeper layer the
    // count conv_skip_decode(s2[p], op) derived from it; a consumer reads the input rows its producer left out from the const
    // image of its input instead.  The computed rows of a launch are COMPACTED: the kernel runs over m' = 0 .. *rows_total - 1 and
    //   rowmap[m'] = rowmap_entry(full output row = (img*OH + oh)*OW + ow, s2[img])      (shared.h)
    // gives it the pixel to compute, the row to store to and the image's count (launch_conv_rowmaps builds the maps on the
    // device from conv1_skip_mask_kernel's per-position counts; the host never sees a value, nothing synchronises).
    const int* rowmap;        // nullptr: every row is computed, m' = m
    const int* rows_total;    // device word: number of compacted rows of this launch (read at kernel start)
    int in_op;                // consumer side: input rows < conv_skip_decode(s2[img], in_op) were not computed by the producer ...
    const f16* const_in;      // ... and are read from this const image [H][W][C] of the input instead (nullptr: the input is complete)
};

#ifdef __HIPCC__
__device__ __forceinline__ void tap_decode(const ConvGeom& g, int p, int& kh, int& kw) {
    if (g.tap_table) {
        const unsigned long long w = p < 8 ? g.taps[0] : p < 16 ? g.taps[1] : p < 24 ? g.taps[2] : g.taps[3];
        const int code = (int)(w >> ((p & 7) * 8)) & 0xff;
        kh = code >> 4;
        kw = code & 15;
    } else {
        kh = p / g.KW;
        kw = p - kh * g.KW;
    }
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// One wave hands data to its own lanes through LDS (a per-wave scratch area): what its lanes wrote before this point is visible to what
// they read after it, and the compiler moves no access across it.  No workgroup barrier: the other waves are not involved.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

// out[m][n] = epi( sum_k A[m][k] * (Wh[n][k] + Wl[n][k]) )
// epi(v) = relu?( v*scale[n] + bias[n] + res[(m % res_mod)][n] )
struct GemmArgs {
    const f16* A;         // plain: row-major [M][lda]; conv: NHWC input
    long lda;
    ConvGeom g;
    const f16* Wh;        // [N][ldw] fp16 (hi part)
    const f16* Wl;        // [N][ldw] fp16 (lo part, W2 mode) or nullptr
    long ldw;
    int M, N, K;
    const float* scale;   // per-n or nullptr
    const float* bias;    // per-n or nullptr
    const float* res;     // fp32 residual or nullptr
    long ldr;
    int res_mod;          // residual row = m % res_mod (0: m)
    float* out32;         // optional fp32 output
    f16* out16;           // optional fp16 output
    long ldc;
    int relu;
    // fused LayerNorm epilogue (row-wide tiles only, N == 512): out32/out16 receive LN(acc*scale + bias + res)
    const float* ln_w;    // nullptr: no LayerNorm
    const float* ln_b;
    int ln_flavour;       // LN_STD / LN_ANNOTATED
    // Tiled token stream of the fused GestSync transformer (see below): with ln_w the residual comes from res16 and the
    // LayerNorm output goes to out16, both in the tiled order; a_tiled: the A operand of a plain GEMM (K == 512) is such
    // a tiled fp16 plane.
    const f16* res16;
    int a_tiled;
    // Implicit LayerNorm (XLM-RoBERTa's post-norm layers, xlmr.hip:xlmr_encode_folded): the token stream holds the UN-normalised rows
    // x = hi + lo (two fp16 planes; the hi plane is the next GEMM's A operand) and per row (mean, rstd) of x; LN(x) itself is never
    // materialised.  ln_mode 1 (consumer: the Linear behind the LayerNorm, weights pre-multiplied by gamma):
    //     out = rstd[m] * (acc - mean[m] * scale[n]) + bias[n]      scale = column sums of the folded weights, bias = b + W beta
    // ln_mode 2 (producer: the Linear whose output is added to LN(x_prev) and becomes the next x):
    //     v = acc + bias[n] + scale[n] * rstd[m] * (x_prev[m][n] - mean[m])     scale = gamma, bias = b + beta of that LayerNorm
    //     out16 / out_lo = hi / lo planes of v (in place over xres_hi / xres_lo is fine), stat_out[m][n / 64] = (sum, sum of squares) of
    //     the row's 64 columns n .. n + 63 (launch_ln_stats turns them into the next (mean, rstd))
    int ln_mode;
    const float* ln_stats;     // [M][2]: (mean, rstd) of the LayerNorm input rows (mode 1: of A's rows; mode 2: of x_prev's rows)
    const f16* xres_hi;        // mode 2: x_prev planes, row-major [M][ldc]
    const f16* xres_lo;
    f16* out_lo;               // mode 2: lo plane of the output
    float* stat_out;           // mode 2: [M][N / 64][2]
    // Per-clip bias (precision mode JG_PREC_FP16_RC, launch_rc_bias): row m takes bias_clip[min(m / rpc, nclips - 1)][n] instead of
    // bias[n].  LDS-DMA kernel only, through the fp16 row-transposing epilogue (out16 alone, no residual) or the LayerNorm-fused one;
    // the planner (gemm_plan.hip) rejects anything else -- there is no path that would quietly drop the correction.
    const float* bias_clip;    // [nclips][N] (the layer's bias already inside) or nullptr
    int rpc, nclips;
};

// (the tiled token stream x16t of the fused transformer -- GemmArgs::res16 / a_tiled -- has its layout in shared.h: x16t_index)
#ifdef __HIPCC__
typedef float f32x2_t __attribute__((ext_vector_type(2)));
#endif

// ---- launchers that both builds define (each returns hipGetLastError()) ------------------------------------------
// which instance a launch gets and which argument sets are accepted: plan_gemm (gemm_plan.h); a rejected set returns hipErrorInvalidValue
hipError_t launch_gemm(const GemmArgs& a, bool conv, const EngineOpts& o, hipStream_t s);
hipError_t launch_stack_frames(const void* src, int src_is_u8, long sb, long st, long sh, long sw, long sc,
                               int B, int T, int pad, int H, int W, f16* dst, hipStream_t s);
// s2 / in_op / const_in as in ConvGeom: input rows of image n below conv_skip_decode(s2[n], in_op) come from the const image
hipError_t launch_maxpool3x3s2(const f16* in, f16* out, int N, int H, int W, int C, hipStream_t s, const int* s2 = nullptr,
                               int in_op = 0, const f16* const_in = nullptr);
// tiled: x16 is the tiled token stream (D = 512; x32 unused); otherwise row-major x32 (+ x16 unless nullptr)
hipError_t launch_window_gather(const float* conv, const float* pe, int B, int P, int Twin, int L, int D, int shift, bool tiled,
                                float* x32, f16* x16, hipStream_t s);
hipError_t launch_layernorm(const float* in, const float* w, const float* b, int rows, int D, int flavour,
                            int relu, float* out32, f16* out16, hipStream_t s);
hipError_t launch_attention(const f16* qkv, const float* keymask, int B, int S, int H, int dk, f16* out, const EngineOpts& o, hipStream_t s);
// Window structure of the GestSync clip path for attention straight from per-position projections (attention.hip):
// token j of window (clip c, frame i) comes from conv position clamp(i + j - shift, 0, P - 1) of clip c.
struct AttnGather {
    const f16* pe_qkv;    // [S][3D]: W_qkv pe[j] + b
    int Twin, P, shift;   // windows per clip, conv positions per clip, window_gather's shift
};
hipError_t launch_group_mean(const f16* in, int groups, int L, int D, f16* out, hipStream_t s);
hipError_t launch_cast_f32_f16(const float* in, f16* out, long n, hipStream_t s);
// first audio conv (5x5, 1 -> 32 channels, BN folded, ReLU) straight from the mel frames: wh / wl = the packed [32][32] weights (k = tap)
// valid (optional, device [B]): per-clip number of valid mel frames in a zero-padded batch (see zero_tail_kernel, elementwise.hip)
hipError_t launch_audio_conv0(const float* mel, int B, int Tm, int F, const f16* wh, const f16* wl, const float* bias, f16* out, const int* valid,
                              hipStream_t s);
// NHWC [B][H][..row_elems..] fp16: rows h >= len_b of clip b set to zero, len_b = valid[b] halved (len-1)/2+1 `halvings` times
hipError_t launch_zero_tail(f16* x, const int* valid, int halvings, int B, int H, long row_elems, hipStream_t s);
hipError_t launch_segment_mean(const float* seq, int D, const int32_t* seg, int n, f16* dst16, float* dst32,
                               int dst_ld, int dst_col, hipStream_t s);
// implicit-LayerNorm token stream (GemmArgs::ln_mode): embeddings as un-normalised hi / lo planes + per-64-column (sum, sum of squares)
hipError_t launch_xlmr_embed_planes(const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word, const float* pos,
                                    const float* type, f16* hi, f16* lo, float* part, hipStream_t s);
// out32 = LayerNorm(hi + lo) (nn.LayerNorm, eps 1e-5), D = 768: the explicit LayerNorm at the end of the implicit chain
hipError_t launch_layernorm_planes(const f16* hi, const f16* lo, const float* w, const float* b, int rows, int D, float* out32, hipStream_t s);

#ifdef JG_BF16
}  // namespace bf
#else
// ---- fp16-only launchers: one definition, in the global namespace; the host calls them un-dispatched, on paths a bf16 handle
// cannot take (conv1.hip, elementwise_fp16.hip, launch_attention_gather in attention.hip).  The bf16 units do not see them.
// conv1 from u8 frames = three launches: launch_conv1_scan (zero bands -> skip masks, into zscratch: conv1_zmask_elems words),
// launch_conv1_direct (zscratch == nullptr: nothing is skipped), launch_conv1_edge_fix (pooled columns that straddle two strips)
hipError_t launch_conv1_scan(const uint8_t* src, int nclip, int T, int pad, const f16* Wd, float scale, unsigned* zscratch, hipStream_t s);
hipError_t launch_conv1_direct(const uint8_t* src, int nclip, int T, int pad, const f16* Wd, float scale,
                               f16* out_pooled, f16* edge, const unsigned* zscratch, bool fill_all, const EngineOpts& o, hipStream_t s);
hipError_t launch_conv1_edge_fix(f16* out_pooled, const f16* edge, long positions, hipStream_t s);
// the 64 per-channel values relu(bias) that conv1 produces over an all-zero patch, as the kernel rounds them (-> const chain)
hipError_t launch_conv1_zconst(const f16* Wd, float scale, f16* zconst, hipStream_t s);
hipError_t launch_attention_gather(const f16* qkv_pos, const AttnGather& g, int B, int S, int H, f16* out, hipStream_t s);
// pe_qkv[j][n] = sum_k W[n][k] pe[j][k] + bias[n]  (W = Wh (+ Wl), [N][K] fp16; pe [S][K] fp32): 21 x 1536 outputs
hipError_t launch_pe_project(const float* pe, int S, const f16* Wh, const f16* Wl, const float* bias, int N, int K, f16* out, hipStream_t s);
hipError_t launch_broadcast_channels(const f16* v, int C, f16* out, long pixels, hipStream_t s);
// stats != nullptr ([M][2] mean, rstd): sums of the NORMALISED rows (A[m][k] - mean[m]) * rstd[m] (calibration of an implicit-LayerNorm consumer)
hipError_t launch_col_sum(const f16* A, long lda, int M, int K, float* scratch, float* out, hipStream_t s, const float* stats = nullptr);
// JG_PREC_FP16_RC: out[c][n] = bias[n] + sum_k lo[n][k] * (mean over a fixed sample of clip c's rows of A[.][k]); clip c = rows c*rpc .. +rpc-1 of
// A (row-major [.][lda], or the tiled fp16 token plane when `tiled`: K == 512); scratch: rc_scratch_elems(nclips, K) floats
// valid_rows (optional, device [nclips]): rows of each clip that are its own (the rest of its rpc rows is batch padding)
hipError_t launch_rc_bias(const f16* A, long lda, int tiled, int nclips, int rpc, const int* valid_rows, const f16* lo, const float* bias, int N, int K,
                          float* scratch, float* out, hipStream_t s);
#endif
#endif  // this build's declarations
