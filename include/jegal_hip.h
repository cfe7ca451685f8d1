/* libjegal_hip -- C ABI of the MI355X-native JEGAL embedding-extraction engine.
 *
 * The reference (Sindhu-Hegde/jegal) has no FFI layer: its boundary for this path is the Python
 * method surface of two nn.Modules plus two on-disk formats.  Each entry
 * point below names the reference interface it replaces (file:line under the reference tree).
 * The Python facade in jegal_amd/ binds these with ctypes and re-creates the reference signatures
 * (GestSync.forward_vid, JEGAL.forward_inference, ...); INTEGRATION.md shows the binding.
 *
 * Conventions: opaque handle per GPU/process (not thread-safe), caller-owned buffers, every
 * function returns 0 on success or a negative code with jg_last_error() describing it, no
 * exceptions cross the boundary.  All data pointers are DEVICE pointers unless the parameter name
 * ends in _host.  Work is enqueued on the handle's HIP stream (jg_set_stream) and is asynchronous
 * unless stated; jg_sync waits for it.
 */
#ifndef JEGAL_HIP_H
#define JEGAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jg_handle jg_handle;

enum { JG_OK = 0, JG_ERR_ARG = -1, JG_ERR_HIP = -2, JG_ERR_STATE = -3, JG_ERR_WEIGHT = -4 };

/* dtype codes for jg_load_tensor / frame buffers */
enum { JG_F32 = 0, JG_F16 = 1, JG_I64 = 2, JG_U8 = 3 };

/* operand precision (DESIGN.md "precision"): fp32 accumulate / residual / LN / softmax in all modes */
enum {
    JG_PREC_FP16 = 0,     /* every GEMM/conv operand fp16 */
    JG_PREC_FP16_W2 = 1,  /* Linear weights carried as hi+lo fp16 pair (2 MFMAs) */
    JG_PREC_FP16_W2_ALL = 2, /* conv weights split as well */
    JG_PREC_FP16_BC = 3,  /* single fp16 weights on the gesture path, the systematic part of the weight
                             rounding error (w - fp16(w)).E[x] folded into the bias by a calibration pass run inside
                             jg_finalize_weights (built-in clips: validated on the seeded weights only) or by jg_calibrate_gesture on
                             the caller's clips; content-path Linears keep the hi+lo split.  Opt-in: ~3 % faster than the default */
    JG_PREC_BF16 = 4,     /* REPORTED mode (north_star names bf16): every weight and every 16-bit activation is bf16 and every
                             MFMA is a bf16 MFMA (v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16, the second build of the kernels,
                             namespace bf).  Same MFMA rate as fp16, 8 instead of 11 significant bits: the embeddings come out
                             at ~5e-3 of the reference, outside the 1e-3 contract -- which is why fp16 is the default
                             (tests/test_gpu_precision_uploads.py::test_precision_modes_report prints the measured errors side by
                             side).  conv1 runs as an implicit GEMM over stacked frames and the LayerNorms as separate kernels in
                             this mode (the fused u8 conv1 kernel and the fp16 + fp8 token stream are fp16 constructs). */
    JG_PREC_FP16_RC = 5,  /* DEFAULT (round 5).  Run-time corrected: as JG_PREC_FP16_BC, but the term (w - fp16(w)).E[x] of every GestSync transformer
                             Linear is rebuilt per GEMM call and per clip from a fixed sample of THAT clip's own input rows (two small
                             launches in front of the GEMM, a per-clip bias in its epilogue) -- no calibration pass, nothing depends on
                             calibration data or on the other clips of a batch.  The JEGAL branch and the content path run hi+lo.
                             What the CLI drivers select for a checkpoint they have never seen (jegal_amd/drivers.py). */
    JG_PREC_FP32 = 6      /* AUDIT mode (round 6; SURVEY 8b's precision list names BF16X3 / FP32: this is that exact mode).  Every GEMM /
                             convolution on v_mfma_f32_32x32x2_f32 with fp32 weights, fp32 activations end to end, fp32 softmax and
                             LayerNorm: the on-device stand-in for the reference's CPU path, which is fp32 (inference_embs.py:497: autocast
                             does nothing without CUDA).  ~2e-6 of the fp32 oracle instead of ~6e-4, ~50 clips/s instead of ~2 600: what
                             `python -m jegal_amd.drivers ... --audit` compares the default mode with on the caller's own clips and
                             checkpoint, where no oracle exists.  Option "audit_weights" (before jg_finalize_weights) keeps the fp32
                             matrices next to the fp16 ones in any mode, option "audit_stages" then moves single stages to fp32. */
};

/* ---- lifecycle ------------------------------------------------------------------------------ */
int jg_create(int device, jg_handle** out);
int jg_destroy(jg_handle* h);
const char* jg_last_error(jg_handle* h);
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the legacy default
 * stream.  Until this is called the handle uses a private non-blocking stream. */
int jg_set_stream(jg_handle* h, void* hip_stream);
int jg_set_precision(jg_handle* h, int mode);
/* clips (or 25-frame windows / 8) of the GestSync conv stack processed per pass; bounds the workspace (default 32: ~14 GB per lane
 * for 150-frame clips - fewer, larger launches are what the 288 GB of the part are for; lower it for long clips on a shared GPU) */
int jg_set_chunk(jg_handle* h, int clips_per_chunk);
/* tuning / A-B switches, per handle (all default to the fast setting; results stay within the parity tolerance either way):
 *   "conv1_direct"    1: fused u8 conv1+pool kernel, 0: temporal stack + implicit GEMM + pool kernel
 *   "conv1_zero_skip" 1: all-zero input bands (the face-mask rows) are skipped / run only the bias slots (bit-identical)
 *   "conv1_mfma16"    1: the fused conv1 kernel's MFMA waves run v_mfma_f32_16x16x32_f16 (0: 32x32x16, the round-1/2 form; the two
 *                     differ in fp32 summation order only)
 *   "conv2_row_skip"  1: conv2 .. conv5 do not compute the leading output rows of a POSITION that the zero-band scan proves to be
 *                     independent of the position (their whole window lies in conv1's constant region); consumers read them from
 *                     images computed once per weight load.  Per position: every position skips what its own five frames allow
 *                     (bit-identical)
 *   "qkv0_linear"     1: the first transformer layer's qkv projection runs over the T+4 distinct conv positions and the 21
 *                     positional rows (linearity of W(conv + pe) + b); the attention kernel gathers and sums the rows
 *   "edge_dedup"      1: evaluate only the T+4 distinct padded-clip positions
 *   "fuse_ln"         1: residual + LayerNorm fused into the GestSync projection GEMMs (tiled token stream)
 *   "attn_mfma"       1: MFMA attention kernels for S <= 160, dk = 64
 *   "gemm_glds", "gemm_big_tile", "gemm_small_tile", "gemm_tall_tile", "gemm_persistent", "gemm_counted",
 *   "gemm_stagger":   tile / pipeline choices of the LDS-DMA GEMM (tests/test_gpu_options_scale_multirank.py flips every one of them)
 *   "gemm_tile"       0: plain GEMMs pick their tile by a measured cost estimate; 1 / 2 / 3: force 128x128 / 256x128 / 256x256 (bit-identical)
 *   "dual_stream"     1: jg_extract_gesture and jg_gestsync_clip split a batch of >= 8 clips (and >= 256 frames in the smaller part) into two halves (option "dual_split": eighths of the batch on the first lane, default 4 since round 6; rounds 3-5: 3) and run the two parts concurrently on two internal
 *                     streams (own workspaces; the caller's stream is joined at entry and exit): one part's next kernel fills
 *                     the partly empty last round of the other's persistent kernels.  Bit-identical results.
 *   "num_cu"          workgroups a persistent kernel launches, 1..1024 (default: the device's CU count; experiment)
 *                     conv1_direct_kernel needs num_cu >= 8 or no more column strips (5 per position) than num_cu: it deals the strips out
 *                     per XCD (workgroup index & 7), and with fewer than 8 workgroups some XCD ranges would have nobody; such a
 *                     launch is rejected (JG_ERR_HIP, invalid value) instead of leaving pooled rows unwritten.
 *   "lane_walk_gemm", "lane_walk_conv", "lane_walk_lnf", "lane_walk_conv1" ("lane_walk": all four), 1..4: inside a two-lane batch a persistent
 *                     kernel of the family (plain GEMMs / conv GEMMs / the LayerNorm-fused GEMM / conv1_direct_kernel) launches
 *                     min(tiles, factor x num_cu) workgroups, so that each walks 1 / factor of the tiles and a CU can pass to the other
 *                     lane's next kernel whenever a workgroup exits.  Tile choice, cost estimates and admission keep using num_cu;
 *                     bit-identical results for every factor.  Handle defaults: plain GEMMs 4, the others 1 (measured:
 *                     tools/experiments/README.md); the planner's built-in default (jg_debug_gemm_plan) is 1.  One-stream batches: no effect.
 *   "debug_lanes"     1: jg_debug_gemm_check, jg_debug_conv_check and jg_debug_conv1_pool launch as inside a two-lane batch (tests)
 *   "lane_priority"   3 (default): the two lane streams are created with the device's highest stream priority; 0: normal priority (rounds 3-5);
 *                     1 / 2: only the second / first lane (a change drains and re-creates the lane streams).  HIP deals streams onto four hardware
 *                     queues PER PRIORITY LEVEL in creation order: normal-priority lanes can end up on one queue when the application owns
 *                     other streams, and then the "concurrent" halves run in turn (measured: 2 076 instead of 2 510 clips/s with five other
 *                     streams).  High-priority lanes only compete with the application's own high-priority streams.  (A host-streaming pipeline around the engine -- GestureStreamer's
 *                     H2D / D2H / compute streams -- in a process that owns further streams is the one measured case where 0 was faster:
 *                     tools/experiments/stream_queue_sweep.sh)
 *   "xlmr_lanes"      2 (default), 1 .. 4: jg_xlmr_encode runs a batch as that many equal parts on as many streams (the first two are the
 *                     lane streams of "dual_stream" / "lane_priority")
 *   "ws_poison"       1 (test aid, default 0): the workspace is filled with 0xff bytes (fp16/fp32 NaN) before every pass -- every entry
 *                     point that uses the workspace, every clip chunk of a long batch -- so a kernel that reads a row nobody wrote
 *                     (the row / band skips leave rows unwritten on purpose) shows up as NaN
 *   "jegal_fp32_ends" 1 (default): the two ends of the JEGAL gesture branch (proj_ip_rgb; final norm + proj_op_rgb + proj_op_align_gesture) and
 *                     of the content path (proj_op_text, fusion / align MLPs) keep fp32 activations and run on the split-operand GEMM
 *                     (three fp16 MFMAs per tile: fp32-grade products); 0: the round-5 arithmetic (fp16 activations, hi+lo weights).  DESIGN.md section 3.
 *                     "fp32-grade" holds for activation rows of rms >= ~2^-7 and |a| < 65520: below |a| ~ 2^-3 the lo half of the split is an fp16
 *                     subnormal with an absolute quantum of 2^-24.  At these call sites the activations have row rms 0.69 .. ~9 and |a| <= 42 over
 *                     the six synthetic weight families (tools/x3_operand_range.py, profiles/x3_operand_range.json); tests/test_gpu_kernels_fp64.py
 *                     holds the kernel to the fp32 bound for operand row rms 2^-6 / sqrt 3 .. 2^10 / sqrt 3
 *   "conv_round_diffuse" 1 (default; before jg_finalize_weights): conv weights are rounded to fp16 with error diffusion across the taps of each
 *                     (output channel, input slot) pair instead of round-to-nearest per weight (the pixel-independent part of the rounding error vanishes)
 *   "audit_jegal_parts" measurement only (needs audit_weights): parts of the fp16 JEGAL gesture branch on the fp32 kernels (1 input projection,
 *                     2 attention sub-layers, 4 feed-forward sub-layers, 8 final norm + output projections)
 *   "audit_weights"   1 (before jg_finalize_weights): the fp32 matrices are kept next to the packed fp16 ones (always in JG_PREC_FP32)
 *   "audit_stages"    mask of the stages that run on the fp32 audit kernels (needs audit_weights): 1 GestSync conv stack, 2 GestSync
 *                     transformer + ff_vid, 4 JEGAL gesture branch, 8 JEGAL content path (audio / text / fusion), 16 XLM-RoBERTa.  The
 *                     stage boundaries are fp32 tensors in every mode; this is how DESIGN.md section 3 decomposes the fp16 error by stage */
int jg_set_option(jg_handle* h, const char* name, int value);
int jg_sync(jg_handle* h);

/* ---- weights: replaces model.load_state_dict(sd) (inference_embs.py:92-119,
 *      evaluation/extract_jegal_embs.py:32-53).  `name` is the reference state_dict key with any
 *      "module." prefix already stripped; keys that no finalize consumes (lstm.*, logits_scale.*, fc.* of
 *      a GestSync checkpoint: no forward uses them) are accepted and ignored, missing keys of a model that
 *      is finalized make jg_finalize_weights fail (strict). ------------------------------------- */
int jg_load_tensor(jg_handle* h, const char* name, const void* data_host, const int64_t* shape_host, int ndim, int dtype);
/* which: bit 0 = GestSync (the video stream: net_vid, transformer, ff_vid), bit 1 = JEGAL, bit 2 = XLM-RoBERTa (keys of
 * transformers.XLMRobertaModel under the prefix "xlmr."), bit 3 (value 8) = GestSync's audio stream (net_aud.conv1..fc6 with bn1..6,
 * ff_aud.fc7 / bn7 / fc8; strict like the others and independent of bit 0: a checkpoint without audio keys still finalizes with 1 and
 * fails with 8).
 * Folds BatchNorm, packs k=(kh,kw,c), splits hi/lo.
 * Staged tensors: the ones this call consumed are dropped; tensors staged for a model that is finalized by a LATER call stay
 * (load everything, then finalize(1), finalize(2) works); keys no finalize consumes stay until jg_clear_staged_tensors.
 * JG_PREC_FP16_BC: the built-in calibration runs for the gesture models finalized by THIS call only (never for bit 2 alone);
 * bias corrections of the other model - e.g. from jg_calibrate_gesture on real clips - are kept.  Re-finalizing a model
 * discards ITS corrections: call jg_calibrate_gesture again after re-loading it. */
int jg_finalize_weights(jg_handle* h, int which);
/* Drop every staged host tensor (the lstm tensors of a GestSync checkpoint, tensors of a model never finalized -- e.g. net_aud.* when
 * bit 3 is not wanted). */
int jg_clear_staged_tensors(jg_handle* h);

/* Re-run the JG_PREC_FP16_BC calibration on caller-supplied clips (same layout as jg_gestsync_clip; device
 * pointer) instead of the built-in synthetic ones, e.g. a few real videos.  frames == NULL: built-in clips. */
int jg_calibrate_gesture(jg_handle* h, const void* frames, int frames_dtype, int B, int T);

/* ---- XLM-RoBERTa text front end ------------------------------------------------
 * Replaces `mroberta(input_ids, attention_mask=text_mask).last_hidden_state` of JEGAL.get_roberta_embeddings
 * (models/jegal.py:116-129; the reference runs transformers.XLMRobertaModel "xlm-roberta-base" on the CPU).  The tokenizer stays
 * on the host.  input_ids, attention_mask: (B, L) int32 on the device (attention_mask NULL = all ones); out (B, L, 768) fp32.
 * Third-party arithmetic: parity is pinned against transformers.XLMRobertaModel with seeded random weights
 * (tests/golden/xlmr.npz), not against the released checkpoint, which is not available offline. */
int jg_xlmr_encode(jg_handle* h, const int32_t* input_ids, const int32_t* attention_mask, int B, int L, float* out);
/* JG_PREC_FP16_BC and JG_PREC_FP16_RC (the default).  After jg_finalize_weights(h, 4) the XLM-RoBERTa Linears run with hi+lo fp16 weight pairs (calibration-free,
 * two MFMAs per fragment pair).  This call runs one pass over the CALLER's token ids (device (B,L) int32; attention_mask may be
 * NULL), records the input mean of every Linear and switches them to single fp16 weights with the systematic rounding term
 * (w - fp16(w)).E[x] folded into the bias (~1.5x faster encoder).  input_ids == NULL: built-in uniform-random ids -- validated on
 * seeded test weights only, NOT on the released xlm-roberta-base checkpoint (which is not available offline), hence never implicit. */
int jg_calibrate_xlmr(jg_handle* h, const int32_t* input_ids, const int32_t* attention_mask, int B, int L);

/* ---- GestSync (models/gestsync.py) ---------------------------------------------------------- */
/* Per-clip features: frames (B,T,270,480,3) u8 (JG_U8, the /255 of inference_embs.py:282 is applied
 * inside) or fp32 in [0,1] (JG_F32) -> edge-pad 12 (inference_embs.py:283) -> T windows of 25
 * (inference_embs.py:488-492) -> forward_vid -> mean(-1) (inference_embs.py:511) -> (B,T,1024) fp32.
 * The conv stack runs once over the padded clip (window de-duplication, exact). */
int jg_gestsync_clip(jg_handle* h, const void* frames, int frames_dtype, int B, int T, float* out_feats);
/* The same for a batch of clips of DIFFERENT lengths padded to T with copies of each clip's last frame (exact for the clip's own
 * frames: inference_embs.py:283 edge-pads with the last frame and window t only reaches frame t + 12; this is how
 * jegal_amd.drivers extract_gestsync_feats batches preprocess/extract_gestsync_feats.py:314-344, which runs one video at a time).
 * valid_frames_host (host [B], 1..T): frames of clip b that are its own.  JG_PREC_FP16_RC takes each clip's run-time correction from
 * its own rows only, so rows t < valid_frames[b] of clip b do not depend on T or on the other clips, and for clips of >= 49 frames
 * they are bit-identical to the clip run alone.  (A clip of fewer than 49 frames ALONE has fewer than 1 024 token rows and takes the
 * unfused hi+lo plan, in a padded batch the fused one: each within the 1e-3 contract of the reference, 5e-4 apart in the test -- not bit for bit.)  The
 * other modes ignore the lengths.  Rows t >= valid_frames[b] of the output are padding for the caller to strip. */
int jg_gestsync_clip_ragged(jg_handle* h, const void* frames, int frames_dtype, int B, int T, const int32_t* valid_frames_host, float* out_feats);
/* GestSync's audio stream (needs jg_finalize_weights bit 3; fp16 modes and JG_PREC_FP32 -- a JG_PREC_BF16 handle is refused with
 * JG_ERR_STATE).  All data pointers are device pointers.  Bad arguments (null buffers, non-positive sizes, valid_tm outside 1..Tm) return
 * JG_ERR_ARG before anything is enqueued; weights that were never finalized return JG_ERR_STATE.  Both use the workspace and run on the
 * handle's stream, asynchronously.
 * Drop-in for GestSync.forward_aud (gestsync.py:164-168): x (N,1,80,100) fp32 (mel band x 100 mel steps = 25 frames) -> out (N,1024) fp32. */
int jg_gestsync_audio_windows(jg_handle* h, const float* x, int N, float* out);
/* Per-clip form: mel (B,Tm,80) fp32, time-major as jg_logmel writes it -> out (B,T,1024): window t of clip b = mel rows
 * clamp(4(t-12) + w, 0, valid_tm[b] - 1), w = 0..99 -- the audio twin of the video path's +-12 frame edge pad; the windows are never
 * materialised.  valid_tm_host (host [B], 1..Tm; NULL: every clip fills its Tm rows): rows of clip b that are its own, so that a clip's
 * rows do not depend on a longer neighbour.
 * A window's embedding is a function of its own 8000 values: the two entries give bit-identical rows when called with the same number of
 * windows (N = B T) in the same order.  Across different N the GEMM planner may pick other kernel instances: only the parity contract
 * (1e-3 rel-L2 of the reference in the default mode) holds there. */
int jg_gestsync_audio_clip(jg_handle* h, const float* mel, int B, int Tm, int T, const int32_t* valid_tm_host, float* out);
/* Kernel check points of the audio stream: one production launch on caller buffers (jg_debug_last_kernel names it).
 * conv1 + BatchNorm + ReLU + 3x3/s2 max-pool: src as x above (clip_form 0; then T = 1, B = N, valid_host NULL) or as mel above
 * (clip_form 1), w [64][9] fp32 with the BatchNorm scale folded, shift [64] -> out [B T][19][24][64] fp16, or fp32 with out_f32.
 * max-pool window (2,3) stride (2,2): in (nimg,H,W,C) NHWC fp16 (f32: fp32) -> out (nimg,(H-2)/2+1,(W-3)/2+1,C); C % 8 == 0. */
int jg_debug_gsa_conv1_pool(jg_handle* h, const float* src, int clip_form, int B, int Tm, int T, const int32_t* valid_host, const float* w,
                            const float* shift, void* out, int out_f32);
int jg_debug_maxpool_2x3(jg_handle* h, const void* in, int nimg, int H, int W, int C, void* out, int f32);
/* Kernel-level check point: conv1+BN+ReLU+maxpool (gestsync.py:36-46) only.  frames (B,T,270,480,3) u8,
 * pad = temporal edge padding (12 for clips, 0 for a raw 25-frame window) -> out (B*(T+2*pad-4),43,78,64) fp16 NHWC. */
int jg_debug_conv1_pool(jg_handle* h, const void* frames_u8, int B, int T, int pad, void* out_f16);
/* Kernel check points (tests/test_gpu_kernels_fp64.py): each runs exactly ONE launch of a production launcher on caller operands.  The
 * handle's options (gemm_tile, gemm_small_tile, gemm_big_tile, gemm_persistent, num_cu, gemm_counted, gemm_stagger, gemm_glds, attn_mfma)
 * pick the kernel instance exactly as in production, and the handle's precision picks the build: under
 * JG_PREC_BF16 every 16-bit operand and output is bf16, otherwise fp16.  All pointers are device buffers the caller owns, leading
 * dimensions are in elements.  A shape or argument set the launcher rejects returns JG_ERR_ARG and launches nothing.  Asynchronous.
 * Linear GEMM (launch_gemm, GemmArgs in jegal_amd/csrc/common.h):
 *   out[m][n] = act( sum_k A[m][k] (Wh[n][k] + Wl[n][k]) * scale[n] + bias[n] + res[m % res_mod][n] ),  act: relu 0 none / 1 ReLU / 2 GELU;
 *   bias_clip [nclips][N]: row m takes bias_clip[min(m / rpc, nclips - 1)] instead of bias (fp16 out16 alone);
 *   ln_w != NULL: residual + LayerNorm fused (N = 512, M >= 1024): out16 = LN(acc + bias + res16) in the tiled token order;
 *     out16 may be res16 (the fused transformer runs it in place);
 *   ln_mode 1 / 2: the implicit-LayerNorm consumer / producer epilogues (ln_stats, xres_hi / xres_lo, out_lo, stat_out as in GemmArgs);
 *     with ln_mode 2, out16 / out_lo may be xres_hi / xres_lo (the token stream is updated in place);
 *   a_tiled != 0: A is the tiled token plane of jegal_amd/csrc/shared.h (x16t_index) instead of [M][lda]: K = 512, whole 128-row tiles,
 *     lda is not used for addressing, and the caller owns ceil(M / 128) * 65536 elements.  An fp16-build route (no bf16 handle reaches
 *     it): JG_ERR_STATE on a bf16 handle. */
typedef struct jg_gemm_check {
    const void* A; int64_t lda;                   /* [M][lda] 16-bit */
    const void* Wh; const void* Wl; int64_t ldw;  /* [N][ldw] 16-bit; Wl NULL: single weights */
    int M, N, K;
    const float* scale; const float* bias;        /* per n, or NULL */
    const float* bias_clip; int rpc, nclips;
    const float* res; int64_t ldr; int res_mod;   /* fp32 residual, row m % res_mod (0: m) */
    int relu;
    float* out32; void* out16; int64_t ldc;       /* either or both */
    const float* ln_w; const float* ln_b; const void* res16;
    int ln_mode; const float* ln_stats; const void* xres_hi; const void* xres_lo; void* out_lo; float* stat_out;
    int a_tiled;                                  /* A is the tiled token plane (above) */
} jg_gemm_check;
int jg_debug_gemm_check(jg_handle* h, const jg_gemm_check* c);
/* The GEMM planner's answer for an argument set, without a handle, a device or a launch: which kernel instance launch_gemm would run
 * (jegal_amd/csrc/gemm_plan.h).  Of `c` only the sizes and the null-ness of the pointers are read.  conv (optional): the launch is an
 * implicit-GEMM convolution of this geometry (rowmap / const_in: whether ConvGeom's pointers are set).  a_tiled: the A operand is the
 * tiled token plane (this parameter or c->a_tiled non-zero: the planner then plans exactly what jg_debug_gemm_check launches for c).  num_cu: compute units of the device; lanes_active: the launch is part of a two-lane batch.  opt_names / opt_values:
 * n_opts options as for jg_set_option ("gemm_*", "lane_walk*"; the built-in defaults otherwise, every walk factor 1).  name receives the instance as jg_debug_last_kernel reports it,
 * or "rejected" (launch_gemm would return an error and launch nothing; grid = lds = stagger = 0 then); grid = workgroups, lds = dynamic
 * LDS bytes, stagger = de-phasing delay in 10-ns ticks.  Returns JG_ERR_ARG for bad arguments or an unknown option. */
typedef struct jg_conv_shape { int H, W, C, KH, KW, PH, PW, tap_table, rowmap, const_in; } jg_conv_shape;
int jg_debug_gemm_plan(const jg_gemm_check* c, const jg_conv_shape* conv, int a_tiled, int num_cu, int lanes_active, const char* const* opt_names,
                       const int* opt_values, int n_opts, char* name, int name_len, int* grid, int* lds, int* stagger);
/* Which weights a packed layer's GEMM runs with (jegal_amd/csrc/weight_form.h), without a handle or a device.  precision: JG_PREC_*;
 * kind: 0 conv, 1 gesture-path Linear, 2 content-path Linear, 3 XLM-RoBERTa Linear; model: 1 GestSync, 2 JEGAL, 3 XLM-RoBERTa; keep32: the
 * layer also runs on the split-operand kernel.  form: 0 single, 1 hi+lo split, 2 single + calibrated bias, 3 single + per-clip run-time
 * bias; lo_kept: the lo matrix stays on the device; uncalibrated: the layer runs hi+lo until a calibration has been applied. */
int jg_debug_weight_form(int precision, int kind, int model, int keep32, int* form, int* lo_kept, int* uncalibrated);
/* ... and whether a GEMM on a layer of that form takes the lo operand: uncalibrated as above, calibrating: a calibration pass is in
 * progress, clip_bias: the call takes the per-clip bias (a run-time corrected layer runs hi+lo in every call that cannot). */
int jg_debug_gemm_runs_lo(int form, int uncalibrated, int calibrating, int clip_bias, int* lo);
/* The weight packing on caller arrays (jegal_amd/csrc/weight_pack.h: the functions every finalize runs before it uploads), without a
 * handle or a device.  16-bit values are uint16_t bit patterns.  JG_ERR_ARG for bad arguments, and then nothing is written.
 * Conv layer: w [O][I][KT][KH][KW], bias [O] and an optional eval BatchNorm (all four of bn_* or none) -> matrix [N][K] fp32 with
 *   k = t slot + kt I + c (t: the tap's place in the layer's order, by parity class with reorder when KH KW <= 32) and shift [N];
 *   N = max(O, Opad) and K = kpad > 0 ? kpad : KH KW slot must be passed as such; KT I <= slot, KH KW slot <= K. */
int jg_debug_pack_conv(const float* w, const float* bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, int O,
                       int I, int KT, int KH, int KW, int slot, int kpad, int Opad, int SH, int SW, int reorder, int N, int K, float* matrix, float* shift);
/* A layer's matrix w [N][K] and bias [N] packed under a rounding rule given as plain values: bf16 (single bf16 weights), form (as
 *   jg_debug_weight_form), keep_lo, diffuse_group (>= 0; error diffusion along k = tap group + slot where it applies).  ln_gamma / ln_beta [K]
 *   (both or neither): the layer is packed as the consumer of that LayerNorm, W diag(gamma) with b + W beta, and c1h / c1f [N] receive
 *   the column sums of the packed weights; add_beta [N] (optional): the producer's b + beta.  hi [N][K], bias_out [N]; lo [N][K] if and
 *   only if keep_lo; c1h / c1f if and only if ln_gamma; w32 [N][K] / b32 [N] (the fp32 matrix and bias as packed) if and only if device32
 *   or form 2, which keep them. */
int jg_debug_pack_round(const float* w, const float* bias, int N, int K, int bf16, int form, int keep_lo, int diffuse_group, const float* ln_gamma,
                        const float* ln_beta, const float* add_beta, int device32, uint16_t* hi, uint16_t* lo, float* bias_out, float* c1h, float* c1f,
                        float* w32, float* b32);
/* conv1's slot-major panel for the direct kernel from the packed matrix hi [64][784] and shift [64] -> panel [49][64][16]. */
int jg_debug_conv1_panel(const uint16_t* hi, const float* shift, uint16_t* panel);
/* The bias of a bias-corrected layer after a calibration: w32 [N][K], b32 [N], mu [K] = column sums of the input over `rows` rows -> bias [N]. */
int jg_debug_bias_correction(const float* w32, const float* b32, const float* mu, int64_t rows, int N, int K, float* bias);
/* Implicit-GEMM convolution (launch_gemm with conv = true; tests/test_gpu_conv_fp64.py): ONE conv launch on caller operands, the geometry
 * built by the function production uses (engine::geom), M = nimg * OH * OW output pixels.
 *   out[(img, oh, ow)][n] = relu?( sum_{t, c} in[img][oh SH - PH + kh_t][ow SW - PW + kw_t][c] (Wh + Wl)[n][t C + c] * scale[n] + bias[n] )
 * with the taps t in ConvGeom's order (reorder: by parity class when KH KW <= 32, jegal_amd/csrc/common.h), zero outside the image.
 * K must be KH KW C, C a power of two >= 8, relu 0 or 1 (the conv epilogues know ReLU only).
 * s2_host (host [nimg], optional; LDS-DMA instances only): the launch runs behind a row skip as conv layer `op` (0..3) of the GestSync
 * stack does -- image img leaves out its first conv_skip_decode(s2[img], op) output rows (they stay untouched) and runs over the
 * compacted row map that the production launch_conv_rowmaps builds in the handle's workspace in front of the GEMM; with const_in
 * ([H][W][C] 16-bit) its input rows below conv_skip_decode(s2[img], op - 1) are read from const_in instead of `in`.  Every s2 must lie in
 * 0..255 and leave its image at least one output row. */
typedef struct jg_conv_check {
    const void* in;                               /* NHWC 16-bit, [nimg][H][W][C] */
    int nimg, H, W, C, KH, KW, SH, SW, PH, PW, reorder;
    const void* Wh; const void* Wl; int64_t ldw;  /* [N][ldw] 16-bit, k = t C + c; Wl NULL: single weights */
    int N, K;
    const float* scale; const float* bias;        /* per n, or NULL */
    int relu;
    float* out32; void* out16; int64_t ldc;       /* [M][ldc], either or both */
    const int32_t* s2_host; int op; const void* const_in;
} jg_conv_check;
int jg_debug_conv_check(jg_handle* h, const jg_conv_check* c);
/* 3x3 / stride 2 max-pool, NHWC 16-bit (launch_maxpool3x3s2): in [nimg][H][W][C] -> out [nimg][(H-3)/2+1][(W-3)/2+1][C], C % 8 == 0, H, W >= 3.
 * s2_host (host [nimg]) with const_in ([H][W][C]): input rows of image img below conv_skip_decode(s2[img], in_op) (<= H) come from const_in. */
int jg_debug_maxpool(jg_handle* h, const void* in, int nimg, int H, int W, int C, const int32_t* s2_host, int in_op, const void* const_in, void* out);
/* The compaction maps of conv layers op = 0 .. nlayers-1 behind a row-skipping conv1 (launch_conv_rowmaps) from the per-image counts
 * s2_host (host [NF], each 0..255 with conv_skip_decode(s2, op) <= OH[op]).  Synchronises and copies to HOST buffers: map_host[l]
 * NF*OH[l]*OW[l] ints (the device buffer is filled with the caller's content of map_host[l] first: only the first total entries are
 * written), base_host[l] NF+1 ints, total_host[l] one int.  NF*OH*OW >= 2^24 or nlayers outside 1..4: JG_ERR_ARG. */
int jg_debug_conv_rowmaps(jg_handle* h, const int32_t* s2_host, int NF, const int* OH, const int* OW, int nlayers, int32_t* const* map_host,
                          int32_t* const* base_host, int32_t* total_host);
/* fp32 GEMM of the audit mode (launch_gemm32): out = act(A W^T * scale + bias + res[m % res_mod]), act 0 / 1 ReLU / 2 exact GELU. */
int jg_debug_gemm32(jg_handle* h, const float* A, int64_t lda, const float* W, int64_t ldw, int M, int N, int K, const float* scale,
                    const float* bias, const float* res, int64_t ldr, int res_mod, int act, float* out, int64_t ldc);
/* fp32 implicit-GEMM convolution of the audit mode (launch_gemm32 with conv = 1; tests/test_gpu_audit32_fp64.py): ONE launch, the geometry
 * built by engine::geom, M = nimg * OH * OW output pixels.
 *   out[(img, oh, ow)][n] = act( sum_{t, c} in[img][oh SH - PH + kh_t][ow SW - PW + kw_t][c] W[n][t C + c] * scale[n] + bias[n] )
 * in [nimg][H][W][C] fp32 NHWC, W [N][ldw] fp32 with the taps t in ConvGeom's order (as jg_debug_conv_check), scale / bias per n or NULL,
 * act 0 / 1 ReLU / 2 exact GELU, out [M][ldc].  C: any power of two >= 1 (the launcher's rule).  Refused up front: null pointers, sizes <= 0,
 * KH or KW > 15, ldw < KH KW C, ldc < N, a kernel larger than the padded image, M >= 2^31. */
int jg_debug_conv32(jg_handle* h, const float* in, int nimg, int H, int W, int C, int KH, int KW, int SH, int SW, int PH, int PW, int reorder,
                    const float* W_, int64_t ldw, int N, const float* scale, const float* bias, int act, float* out, int64_t ldc);
/* Split-operand GEMM (launch_gemm_x3, option jegal_fp32_ends): fp32 A, fp16 Wh + Wl, fp32 out = relu?(A W^T + bias + res[m % res_mod]).
 * fp16 weights in every precision mode.  K % 256 == 0, N % 128 == 0. */
int jg_debug_gemm_x3(jg_handle* h, const float* A, int64_t lda, const void* Wh, const void* Wl, int64_t ldw, int M, int N, int K,
                     const float* bias, const float* res, int64_t ldr, int res_mod, int relu, float* out, int64_t ldc);
/* softmax(q k^T / sqrt(dk), masked_fill(keymask == 0, -1e9)) v per (sequence, head) (launch_attention): qkv [B*S][3*H*dk] 16-bit (q | k | v),
 * keymask (B,S) fp32 or NULL, out [B*S][H*dk] 16-bit. */
int jg_debug_attention(jg_handle* h, const void* qkv, const float* keymask, int B, int S, int H, int dk, void* out);
/* The layer-0 gather form (launch_attention_gather, fp16 build only; dk = 64, S <= 32): token j of window b = (clip b / Twin, frame b % Twin)
 * is row clip * P + clamp(b % Twin + j - shift, 0, P - 1) of qkv_pos [.][3*H*64] plus row j of pe_qkv [S][3*H*64]. */
int jg_debug_attention_gather(jg_handle* h, const void* qkv_pos, const void* pe_qkv, int Twin, int P, int shift, int B, int S, int H, void* out);
/* fp32 attention of the audit mode (launch_attention32): as jg_debug_attention with fp32 qkv / out. */
int jg_debug_attention32(jg_handle* h, const float* qkv, const float* keymask, int B, int S, int H, int dk, float* out);
/* Check points of the element-wise and reduction launchers (jegal_amd/csrc/elementwise*.hip; tests/test_gpu_elementwise_fp64.py): ONE
 * production launch each on device buffers the caller owns, scratch included; "16-bit" is fp16 or, on a JG_PREC_BF16 handle, bf16.  Every
 * entry refuses with JG_ERR_ARG, before anything is enqueued, null pointers, sizes <= 0, a leading dimension below the row, pointers or
 * strides that break the kernel's 16-byte accesses and `valid` arrays that are not one entry per clip, as well as what the launcher
 * itself rejects.  valid_host arrays live on the HOST (n_valid entries; NULL with n_valid = 0 where optional) and are staged in the
 * handle's workspace.  pe_project, broadcast_channels, col_sum and rc_bias are fp16-build kernels: JG_ERR_STATE on a bf16 handle.
 *   stack_frames: dst [B][T+2pad-4][H][W][16] 16-bit = channels c < 3 of frames clamp(p + dt - pad, 0, T-1), dt < 5, channel 15 = 0;
 *     src u8 or fp32 with element strides sb / st / sh / sw / sc (>= 0), src_elems = elements the caller's source buffer holds.
 *   window_gather: x[(b,i,j)] = conv[b][clamp(i + j - shift, 0, P-1)] + pe[j], conv (B,P,D) fp32; row-major x32 (+ x16 unless NULL;
 *     D % 4 == 0), or tiled != 0: x16 alone as the tiled token plane of whole 128-row tiles (D = 512).
 *   layernorm: flavour 0 nn.LayerNorm (biased variance, eps 1e-5 inside the root), 1 the annotated form (unbiased std + 1e-6); D 512 or
 *     768; out32 and / or out16; out32 == in allowed.  layernorm_planes: out32 = nn.LayerNorm(hi + lo), D = 768.
 *   group_mean: out[g] = mean of rows g L .. g L + L - 1 of in [groups L][D] 16-bit (D % 8 == 0).  cast: n fp32 -> 16-bit, n % 4 == 0.
 *   audio_conv0: mel (B,Tm,F <= 80) fp32, wh / wl (or NULL) [32][32] 16-bit with k = 5 kh + kw < 25, bias [32] -> out (B,Tm,F,32) 16-bit =
 *     ReLU(5x5 conv, pad 2, of the mel rounded to 16 bits and read as zero from row valid[b] on) with rows t >= valid[b] zero.
 *   zero_tail: rows h >= len_b of x [B][H][row_elems] 16-bit zeroed, len_b = max(valid[b], 0) halved (len - 1) / 2 + 1 `halvings` times.
 *   xlmr_embed: out (B,L,D) = (word[id] + type) + pos[pid]; pid = pad_id + non-pad tokens up to and including t (pads: pad_id), clamped
 *     below maxpos; id clamped to 0 .. vocab-1; D % 4 == 0.  xlmr_embed_planes: the same values as hi = 16-bit(v), lo = 16-bit(v - hi) and
 *     part [B L][D / 64][2] = (sum, sum of squares) per 64 columns; D % 256 == 0.
 *   ln_stats: stats [rows][2] = (mean, 1 / sqrt(var + 1e-5)) from part [rows][P][2] (sums over 64 columns each).
 *   mask_i32_f32: out = in != 0.  transpose_tokens: (N,L,D) -> (N,D,L) fp32.
 *   pe_project: out [S][N] fp16 = sum_k (Wh + Wl)[n][k] pe[j][k] + bias[n], Wl / bias optional.  broadcast_channels: out[i] = v[i % C].
 *   col_sum: out[k] += sum_m A[m][k], or of (A[m][k] - stats[m][0]) stats[m][1]; A [M][lda] fp16, K % 8 == 0; scratch >= 64 K floats.
 *   rc_bias: out [nclips][N] = bias[n] + sum_k lo[n][k] mean_c[k], mean_c = fp16 mean of a fixed sample of the first clamp(valid[c], 1, rpc)
 *     rows of clip c (every row below 1024 rows, otherwise rows with (r >> 4) % 8 == 0); A row-major [nclips rpc][lda] or the tiled plane
 *     (K = 512), a_elems = elements the caller's A holds; K 512 or 2048, N % 32 == 0; scratch >= nclips K floats, and the fp16 means
 *     [nclips][K] are left at its start. */
int jg_debug_stack_frames(jg_handle* h, const void* src, int src_is_u8, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int64_t src_elems,
                          int B, int T, int pad, int H, int W, void* dst);
int jg_debug_window_gather(jg_handle* h, const float* conv, const float* pe, int B, int P, int Twin, int L, int D, int shift, int tiled, float* x32,
                           void* x16);
int jg_debug_layernorm(jg_handle* h, const float* in, const float* w, const float* b, int rows, int D, int flavour, int relu, float* out32, void* out16);
int jg_debug_layernorm_planes(jg_handle* h, const void* hi, const void* lo, const float* w, const float* b, int rows, int D, float* out32);
int jg_debug_group_mean(jg_handle* h, const void* in, int groups, int L, int D, void* out);
int jg_debug_cast(jg_handle* h, const float* in, void* out, int64_t n);
int jg_debug_audio_conv0(jg_handle* h, const float* mel, int B, int Tm, int F, const void* wh, const void* wl, const float* bias, void* out,
                         const int32_t* valid_host, int n_valid);
int jg_debug_zero_tail(jg_handle* h, void* x, const int32_t* valid_host, int n_valid, int halvings, int B, int H, int64_t row_elems);
int jg_debug_xlmr_embed(jg_handle* h, const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word, const float* pos,
                        const float* type, float* out);
int jg_debug_xlmr_embed_planes(jg_handle* h, const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word,
                               const float* pos, const float* type, void* hi, void* lo, float* part);
int jg_debug_ln_stats(jg_handle* h, const float* part, int rows, int P, float* stats);
int jg_debug_mask_i32_f32(jg_handle* h, const int32_t* in, float* out, int64_t n);
int jg_debug_transpose_tokens(jg_handle* h, const float* in, int N, int L, int D, float* out);
int jg_debug_pe_project(jg_handle* h, const float* pe, int S, const void* Wh, const void* Wl, const float* bias, int N, int K, void* out);
int jg_debug_broadcast_channels(jg_handle* h, const void* v, int C, void* out, int64_t pixels);
int jg_debug_col_sum(jg_handle* h, const void* A, int64_t lda, int M, int K, float* scratch, int64_t scratch_elems, float* out, const float* stats);
int jg_debug_rc_bias(jg_handle* h, const void* A, int64_t lda, int64_t a_elems, int tiled, int nclips, int rpc, const int32_t* valid_host, int n_valid,
                     const void* lo, const float* bias, int N, int K, float* scratch, int64_t scratch_elems, float* out);
/* The fp32 clones of the audit mode (jegal_amd/csrc/audit32.hip; tests/test_gpu_audit32_fp64.py): the same operations, arguments and
 * refusals as jg_debug_stack_frames / jg_debug_maxpool (without a row skip) / jg_debug_group_mean / jg_debug_zero_tail on fp32 tensors.
 * 16-byte aligned pointers; C % 4, D % 4, row_elems % 4 and L <= 0 are refused up front. */
int jg_debug_stack_frames32(jg_handle* h, const void* src, int src_is_u8, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int64_t src_elems,
                            int B, int T, int pad, int H, int W, float* dst);
int jg_debug_maxpool32(jg_handle* h, const float* in, int nimg, int H, int W, int C, float* out);
int jg_debug_group_mean32(jg_handle* h, const float* in, int groups, int L, int D, float* out);
int jg_debug_zero_tail32(jg_handle* h, float* x, const int32_t* valid_host, int n_valid, int halvings, int B, int H, int64_t row_elems);
/* Name of the kernel instance the last kernel check point on this handle launched, with its template arguments (e.g.
 * "gemm_glds_kernel<1,0,4,4,2,0,0,0,0>"; "a_kernel+b_kernel" for a launcher of two kernels).  The launcher itself writes the name, where
 * it picks the instance and directly in front of the launch; the check point only lends it the handle's slot.  A check point that makes
 * several launches (jg_debug_conv_check with s2_host, jg_debug_conv1_pool) reports the last one.  Empty after any error: a call the
 * check point or the launcher refused, or a HIP failure, never leaves an earlier call's name.  jg_debug_gemm / jg_debug_gemm_ex time
 * launches and leave the name alone.  Host only, no synchronisation. */
int jg_debug_last_kernel(jg_handle* h, char* buf, int len);
/* Check point for "conv2_row_skip": the MINIMUM over the positions of the last conv stack of the leading conv2 output rows that
 * were read from the const chain instead of computed (every position skips its own count: jg_debug_conv_rows);
 * 0: none, or the option is off.  The report describes the last conv stack of the LAST call on this handle: it reads 0 once another
 * workspace pass has begun (any later call that uses the workspace) or the stream was switched (jg_set_stream).  Synchronises the stream. */
int jg_debug_conv2_rowskip(jg_handle* h, int* rows);
/* Check point for the per-position form of it: computed[l] / full[l] = output pixels (rows of the implicit GEMM) that conv2 .. conv5
 * (l = 0..3) of the LAST conv stack computed / would compute without the skip (0 / 0: option off or path not taken).  The same
 * lifetime as jg_debug_conv2_rowskip: the last conv stack of the last call on this handle, 0 / 0 once another workspace pass has begun
 * or the stream was switched.  Synchronises. */
int jg_debug_conv_rows(jg_handle* h, int64_t* computed, int64_t* full);
/* Tuning aid: ms per launch of the production GEMM for a shape (mode bit0 hi+lo weights, bit1 fp32 residual in/out, bit2 ReLU). */
int jg_debug_gemm(jg_handle* h, int M, int N, int K, int mode, int iters, double* ms);
/* The same with caller-supplied fp16 operands a16 [M][K] / w16 [N][K] (device pointers; NULL: constant fill).  Constant operands
 * flatter any MFMA kernel (the chip holds a higher clock on them): tools/gemm_yardstick.py times random data on both sides. */
int jg_debug_gemm_ex(jg_handle* h, const void* a16, const void* w16, int M, int N, int K, int mode, int iters, double* ms);
/* Drop-in for GestSync.forward_vid(x, return_feats) (gestsync.py:148-162): x (N,3,25,270,480) fp32
 * -> out (N,1024,21) fp32, optional out_conv (N,512,21) fp32 (NULL to skip). */
int jg_gestsync_windows(jg_handle* h, const float* x, int N, float* out, float* out_conv);

/* Face-mask + resize pre-step, load_rgb_masked_frames (inference_embs.py:235-276) without the /255 and the edge pad
 * (those live in jg_gestsync_clip): src (T,H,W,3) uint8 device frames, mask_y (T) int32 DEVICE array -- per frame the
 * last source row blanked by cv2.rectangle(img,(0,0),(W,y2+15),0,-1) (face found: mask, then resize), or -1 when
 * mediapipe found no face (resize, then rows 0..110 of the result blanked) -> dst (T,270,480,3) uint8, ready for
 * jg_gestsync_clip.  cv2.resize(INTER_LINEAR, 8-bit) restated from OpenCV's generic fixed-point path; parity unpinned
 * (cv2 absent).  The keypoints themselves stay on the host (mediapipe). */
int jg_mask_resize(jg_handle* h, const uint8_t* src, int T, int H, int W, const int32_t* mask_y, uint8_t* dst);

/* Masked crops in fewer bytes (the host link, not the GPU, bounds a streamed extraction: DESIGN.md section 7): the reference blanks
 * rows 0..y2+15 of every crop (inference_embs.py:264-270), so a producer ships only the rows BELOW each frame's mask.
 * packed: those rows of all frames back to back (device), packed_bytes its size; row0 (n_frames) int32 device: first kept row of
 * each frame (0..270); offsets (n_frames) int64 device: byte offset of that row in `packed` (multiples of 16) -> dst
 * (n_frames,270,480,3) uint8 with the rows above row0 zero: exactly the crop load_rgb_masked_frames returns, ready for
 * jg_gestsync_clip / jg_extract_gesture.  Metadata is validated ON THE DEVICE (it lives there): a frame whose row0 is outside
 * 0..270 or whose offset is negative, not a multiple of 16 or runs past packed_bytes comes out all zero, nothing is read. */
int jg_unpack_masked(jg_handle* h, const uint8_t* packed, int64_t packed_bytes, const int32_t* row0, const int64_t* offsets, int n_frames, uint8_t* dst);
/* The same at SOURCE resolution: the reference decodes e.g. 228x314 / 294x294 crops and resizes them to 270x480 on the host
 * (inference_embs.py:255-276) -- shipping the decoder's frames moves up to 1.8x fewer bytes than shipping the resized crops, and the
 * rows the mask blanks (source rows 0..mask_y) need not cross the link at all.  packed: per frame f the source rows
 * max(mask_y[f]+1, 0) .. H-1 (mask_y = -1, no face: the whole frame), (H - row0) * W * 3 bytes starting at offsets[f];
 * -> dst (T,270,480,3) uint8 = jg_mask_resize of the full frames.  A frame whose rows would run past packed_bytes comes out zero. */
int jg_mask_resize_packed(jg_handle* h, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, int T, int H, int W,
                          const int32_t* mask_y, uint8_t* dst);

/* ---- JEGAL (models/jegal.py) ---------------------------------------------------------------- */
/* forward_gestures (jegal.py:78-92) [+ proj_op_align_gesture, jegal.py:381 when align != 0]:
 * feats (B,T,1024) fp32, mask (B,T) fp32 (1 valid / 0 pad) or NULL -> out (B,T,512) fp32. */
int jg_jegal_gestures(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out);
/* forward_audio (jegal.py:105-113): mel (B,Tm,80) fp32 -> out (B,Ta,256) fp32, Ta = jg_audio_len(Tm). */
int jg_jegal_audio(jg_handle* h, const float* mel, int B, int Tm, float* out);
int jg_audio_len(int Tm);
/* forward_audio on a zero-padded batch of clips of DIFFERENT lengths with the result each clip would give alone: the reference's
 * dataset driver runs batch_size = 1 (evaluation/extract_jegal_embs.py:141), and the conv stack's zero padding (jegal.py:41-63)
 * makes the last audio steps of a clip depend on what follows it in a padded batch.  valid_tm_host (B) int32 on the HOST: mel
 * frames clip b really holds (4..Tm; rows beyond must be present in `mel` but are never read as data).  Rows t < jg_audio_len(
 * valid_tm_host[b]) of out[b] equal jg_jegal_audio on the clip alone up to fp32 summation order; rows beyond are unspecified.
 * NULL = jg_jegal_audio. */
int jg_jegal_audio_ragged(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_tm_host, float* out);
/* wav2filterbanks (utils/audio_utils.py:28-66): wav (B,n_samples) fp32 (int16 scale, NOT normalised: audio_utils.py:20-25),
 * mel_basis (80,257) fp32 = librosa.filters.mel(sr=16000,n_fft=512,n_mels=80,fmin=0,fmax=8000) -> out (B, n_samples/160, 80) log-mel.
 * n_samples >= 257: the STFT reflects 256 samples at either end, which is undefined for a shorter signal (torch.stft raises);
 * fewer samples, or B <= 0, is JG_ERR_ARG and nothing is enqueued. */
int jg_logmel(jg_handle* h, const float* wav, int B, int n_samples, const float* mel_basis, float* out);
/* forward_text (jegal.py:95-103): states (B,L,768) fp32 (XLM-R last_hidden_state), mask (B,L) -> (B,L,256). */
int jg_jegal_text(jg_handle* h, const float* states, const float* mask, int B, int L, float* out);
/* word pooling (jegal.py:174-180,189-195,233-239): for each int32 triplet (start_row,end_row_excl,dst_row)
 * dst[dst_row][dst_col : dst_col+D] = mean(seq[start:end]).  seg is a DEVICE pointer. */
int jg_word_pool(jg_handle* h, const float* seq, int D, const int32_t* seg, int n_seg, float* dst, int dst_ld, int dst_col);
/* cat((audio,text),-1) -> proj_op_fusion_content -> proj_op_align_content (jegal.py:406-415):
 * fused (rows,512) fp32 (audio cols 0..255, text cols 256..511, zero-padded rows) -> out (rows,512). */
int jg_fuse_content(jg_handle* h, const float* fused, int rows, float* out);
/* F.normalize(p=2,dim=-1) (inference_embs.py:631,635; extract_jegal_embs.py:111,115); in == out allowed */
int jg_l2norm(jg_handle* h, const float* in, float* out, int rows, int D);
/* frames -> unit-norm gesture embedding (B,T,512) without leaving the device (the v-only path of
 * inference_embs.py:526-646): jg_gestsync_clip + jg_jegal_gestures(align=1) + jg_l2norm. */
int jg_extract_gesture(jg_handle* h, const void* frames, int frames_dtype, int B, int T, float* out_emb);

/* ---- gesture tracks of any length --------------------------------------------------------------
 * forward_gestures has a 500-row positional table (modules.py:136) and the reference fails beyond it; a longer track is encoded in
 * windows.  The window rule, for two integers win >= 1 and ctx >= 0 with win + 2 ctx <= 500 and a track of T frames:
 *   the track has ceil(T / win) windows; window j has the CORE [j win, min((j + 1) win, T)) and the SPAN
 *   [max(0, j win - ctx), min(T, (j + 1) win + ctx)).  The span is encoded as a clip of its own (positional row 0 = the first span frame,
 *   every span row a valid key, nothing else visible); the window emits the rows of its core alone.
 * The cores partition the track, so every frame is emitted exactly once: output row t of a track is row t - span_start of forward_gestures
 * (+ align MLP) on the span slice of the window whose core holds t.  A track with T <= win is one window whose span is the whole track:
 * exactly what forward_gestures defines for that clip.  No averaging over overlapping windows.
 *
 * jg_track_windows is that rule as a table, on the host: no handle, no device.  t_offsets_host [n_tracks + 1]: track i owns rows
 * t_offsets[i] .. t_offsets[i + 1] - 1 of the concatenated tracks (empty tracks allowed: no windows).  table_host [cap][4] receives per
 * window (span first row, span length, core offset inside the span, core length), rows global, windows ordered by track, then by j;
 * table_host == NULL only counts (cap ignored).  *n_windows = the number of windows, *span_max = the longest span (0 without windows).
 * Returns JG_ERR_ARG and writes nothing for n_tracks < 0, a null t_offsets_host (with n_tracks > 0), n_windows or span_max, win < 1,
 * ctx < 0, win + 2 ctx > 500, a negative or decreasing offset, more than INT32_MAX windows, or cap < the number of windows. */
int jg_track_windows(const int32_t* t_offsets_host, int n_tracks, int win, int ctx, int32_t* table_host, int cap, int* n_windows, int* span_max);
/* The gesture branch over tracks by that rule: feats (sum T, 1024) fp32 (device; GestSync features, the tracks back to back),
 * t_offsets_host [n_tracks + 1] on the HOST (they size the graph) with t_offsets[0] = 0 -> out (sum T, 512) fp32 (device), row for row;
 * align != 0 adds proj_op_align_gesture as for jg_jegal_gestures, normalize != 0 applies jg_l2norm to the rows of out in place.
 * The row-wise ends run once per track row, not once per window row (a row lies in up to (win + 2 ctx) / win spans): proj_ip_rgb on the
 * sum T rows, a gather into the padded (n_windows, span_max) batch with positional rows and key mask, the encoder, a compaction of the
 * core rows back into track order, proj_op_rgb (+ align) on sum T rows.
 * A track's rows are a function of that track, win and ctx alone: not of the other tracks or of the track's place among them.  In bits
 * this holds between calls with the same n_windows and span_max (the same tracks in another order give the same rows bit for bit);
 * between calls of other sizes the GEMM planner and the attention launcher may pick other kernel instances, and the rows agree within
 * the precision mode's contract (1e-3 rel-L2 of the reference in the default mode, 2e-5 in JG_PREC_FP32).
 * Every precision mode of jg_jegal_gestures, the fp32 audit stage included.  Uses the workspace (one pass), runs on the handle's stream,
 * asynchronous.  Workspace: 13 316 bytes per WINDOW row (n_windows * span_max of them) in the 16-bit modes, 20 484 in JG_PREC_FP32, and
 * 10 - 12 KB per track row; the defaults of the Python layer (win 120, ctx 50) make 1.83 window rows per track row.  Nothing is chunked inside the
 * call: a caller bounds a call -- its workspace and JG_TRACKS_MAX_WINDOW_ROWS -- by splitting at track boundaries, which changes no
 * row's definition.
 * JG_ERR_ARG before anything is enqueued: what jg_track_windows refuses, t_offsets[0] != 0, a null feats or out (with sum T > 0), more
 * than JG_TRACKS_MAX_WINDOW_ROWS window rows.  JG_ERR_STATE: JEGAL weights never finalized.  n_tracks == 0 or sum T == 0 returns JG_OK
 * and launches nothing. */
#define JG_TRACKS_MAX_WINDOW_ROWS 1048575      /* n_windows * span_max of one call: the widest activation is (window rows, 2048), and the
                                                  launchers index elements with 31 bits */
int jg_jegal_gesture_tracks(jg_handle* h, const float* feats, const int32_t* t_offsets_host, int n_tracks, int win, int ctx, int align,
                            int normalize, float* out);
/* Check points of its two row movers: ONE production launch each on device buffers the caller owns (jg_debug_last_kernel names it).
 * table_dev: [n_windows][4] int32 as jg_track_windows writes it, on the DEVICE, 16-byte aligned; the host cannot read it, so the caller
 * answers for first row + span length staying inside p32 / out and for spans of at most span_max rows.
 *   span_gather : p32 (rows, D) fp32, pe (>= span_max, D) fp32 -> x32 (n_windows, span_max, D): x32[w][s] = p32[first_w + s] + pe[s] for
 *                 s < len_w, zero beyond; mask (n_windows, span_max) fp32 = 1 / 0.  Every element of x32 and mask is written.
 *   core_compact: in (n_windows, span_max, D) elements of elem_bytes (2 or 4) -> out row first_w + s = in[w][s] for the core rows
 *                 coff_w <= s < coff_w + clen_w; nothing else of out is written.
 * JG_ERR_ARG before anything is enqueued: null pointers, n_windows or span_max < 1, span_gather's span_max > 500, D <= 0, D % 4, rows of
 * D elem_bytes that are no multiple of 16 bytes, n_windows * span_max >= 2^31, buffers not 16-byte aligned. */
int jg_debug_span_gather(jg_handle* h, const float* p32, const float* pe, const int32_t* table_dev, int n_windows, int span_max, int D, float* x32,
                         float* mask);
int jg_debug_core_compact(jg_handle* h, const void* in, int elem_bytes, const int32_t* table_dev, int n_windows, int span_max, int D, void* out);

/* ---- metrics (evaluation/evaluate_*.py) ----------------------------------------------------- */
/* temporal mean of ragged blocks (evaluate_retrieval.py:30-31): out[i] = mean(x[off[i]:off[i+1]]) */
int jg_pool_mean(jg_handle* h, const float* x, const int32_t* offsets, int n, int D, float* out);
/* evaluate_retrieval.py:38-65 on already-normalised rows: rank/ties of the diagonal per local row */
int jg_sim_rank(jg_handle* h, const float* e1, const float* e2, int n_local, int n_total, int row_offset, int D,
                int32_t* rank, int32_t* ties);
/* Retrieval itself, without the similarity matrix.  For each query row i, the k gallery rows with the largest s_ij = <queries[i], gallery[j]>
 * (rows as stored: the caller normalises, as for jg_sim_rank), best first.  idx / score: [n_queries][k], device.
 * s_ij is computed exactly as jg_sim_rank computes it (exact-fp32 MFMA, one k-ascending chain per element), so a score depends on its two
 * rows alone and is bit-identical to the value jg_sim_rank compares; -0.0 is treated (and returned) as +0.0.  The order is total: larger
 * score first, on equal scores the smaller gallery index first (np.argsort(-s, kind="stable")).  idx holds gallery_offset + j, score[i][r]
 * is s_ij bit for bit.  A NaN score is never selected; when fewer than k candidates exist (n_gallery < k, NaN scores) the remaining slots
 * are idx = -1, score = -inf.
 * merge == 0: idx and score are outputs only, their previous contents are never read.  merge != 0: idx and score hold the result of earlier
 * jg_sim_topk calls with the same queries and k for OTHER gallery rows (slots with idx < 0 are empty) and the call leaves the best k of the
 * union in the same total order -- a gallery cut into pieces, in any order, gives the bits of one call over the whole gallery (galleries
 * larger than device memory, gallery-sharded ranks).  If the index ranges gallery_offset .. gallery_offset + n_gallery - 1 of merged calls
 * overlap, or idx / score hold anything but such a result, the result is unspecified.
 * Limits: 1 <= k <= 128; D > 0, D % 64 == 0; n_queries >= 0, n_gallery >= 0; gallery_offset >= 0, gallery_offset + n_gallery <= INT32_MAX;
 * queries and gallery 16-byte aligned.  A violated limit or a null buffer returns JG_ERR_ARG before anything is enqueued.  n_queries == 0
 * returns JG_OK and launches nothing; n_gallery == 0 without merge fills -1 / -inf.  Nothing outside the n_queries * k entries of idx and
 * score is written; no workspace is used.  Asynchronous. */
int jg_sim_topk(jg_handle* h, const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k,
                int gallery_offset, int merge, int32_t* idx, float* score);
/* Grouped top-k: for this word or phrase, which clips gesture it, and at which frame.  The gallery rows (frame-level) are partitioned into
 * contiguous groups (a clip, or a fixed-length segment of a long track); a group scores as its best row; per query row the k best groups
 * are returned, each as the row that earned the score.  The n_queries x n_gallery matrix is never written.
 * Scores: s_ij = <queries[i], gallery[j]> exactly as jg_sim_topk and jg_sim_rank compute it (exact-fp32 MFMA, one k-ascending chain per
 * element, the same staging order): a score depends on its two rows alone and is bit-identical to theirs; -0.0 is treated (and returned)
 * as +0.0; a NaN score is never a candidate.
 * Groups: g_offsets [n_groups + 1], a DEVICE array; group g owns the local gallery rows g_offsets[g] .. g_offsets[g + 1] - 1 (0 ..
 * n_gallery), a contiguous non-decreasing partition, empty groups allowed.  Rows below g_offsets[0] or from g_offsets[n_groups] on belong
 * to no group and are never returned.  A group's champion is its row with the largest score, on equal scores the smallest row (the first
 * arg-max, np.argmax); a group without a non-NaN row has none.
 * Result: per query the k best champions in the total order "larger score first, then the smaller row" (= the smaller group); idx[i][r] =
 * gallery_offset + row, score[i][r] its score bit for bit; when fewer than k groups have a champion the remaining slots are idx = -1,
 * score = -inf.  No two returned rows of one call lie in the same group.  idx / score: [n_queries][k], device.
 * merge as for jg_sim_topk: with merge != 0, idx and score hold the result of earlier calls with the same queries and k for OTHER gallery
 * rows and the call leaves the best k of the union -- a gallery cut into pieces AT GROUP BOUNDARIES, in any order, gives the bits of one
 * call over the whole gallery.  A group split across calls, or overlapping row ranges, give an unspecified result.
 * Safety: the host cannot validate g_offsets, so the kernel never addresses the gallery through it: it walks the rows 0 .. n_gallery - 1 and
 * uses the offsets only to classify a row.  Offsets that are not a non-decreasing partition give an unspecified result, never a read
 * outside the two operands and g_offsets[0 .. n_groups], nor a write outside the n_queries * k entries of idx and score.
 * Limits as for jg_sim_topk: 1 <= k <= 128; D > 0, D % 64 == 0; n_queries, n_gallery, n_groups >= 0; gallery_offset >= 0, gallery_offset +
 * n_gallery <= INT32_MAX; queries and gallery 16-byte aligned.  A violated limit or a null buffer (g_offsets when n_groups > 0) returns
 * JG_ERR_ARG before anything is enqueued.  n_queries == 0 returns JG_OK and launches nothing; n_gallery == 0 or n_groups == 0 fills -1 /
 * -inf without merge and keeps the list with it.  No workspace is used.  Asynchronous. */
int jg_sim_topk_grouped(jg_handle* h, const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k,
                        const int32_t* g_offsets /* device, [n_groups + 1] */, int n_groups,
                        int gallery_offset, int merge, int32_t* idx, float* score);
/* Search of a corpus: jg_sim_topk (g_offsets == NULL, n_groups == 0) or jg_sim_topk_grouped (g_offsets != NULL) over a gallery that may be
 * stored in 16 bits and that every CU walks a part of.
 * Contract: let G32 be the gallery widened to fp32 (exact for fp16).  The call leaves in idx / score exactly what jg_sim_topk_grouped -- or
 * jg_sim_topk when g_offsets == NULL -- leaves for G32, bit for bit, for every value of `slices`, with and without merge.  Everything
 * those two entries document carries over: equal scores order by the smaller row, -0.0 counts as +0.0, a NaN score is never a candidate,
 * empty slots hold -1 / -inf, a group has at most one entry, gallery_offset and merge mean the same, nothing outside the n_queries * k
 * entries of idx and score is written, and g_offsets (a device array nobody has checked) is only read at 0 .. n_groups and only ever
 * compared with row numbers.
 * gallery: [n_gallery][D] rows of gallery_dtype, JG_F32 or JG_F16 (IEEE binary16; a 16-bit corpus is searched as stored: the scores are
 * exact fp32 chains over the stored values).
 * Slices: the gallery is cut into S slices of whole 64-row tiles, slice s = rows [s R, min((s + 1) R, n_gallery)), R % 64 == 0, none
 * empty.  One workgroup per (64 query rows, slice) walks its tiles as the plain entries walk all of them and writes its sorted list of k
 * candidate keys to the workspace; a second launch on the same stream seeds each row's list from idx / score (merge), passes the S k keys
 * of the row through the same insertion -- one entry per group when grouped -- and stores idx / score.  The k best champions of a set do
 * not depend on how the set is cut (a key is (score, row), totally ordered; the true champion of a group is the best row of the group in
 * its own slice and can miss that slice's list only when k other groups beat it there, so the group is not among the k best; a weaker part
 * of the group that survives in another slice is replaced by the champion in the reduction, or is beaten by the k groups that beat the
 * champion).  S == 1 is one launch straight into idx / score and uses no workspace.
 * slices: 0 = the library chooses (jg_debug_search_plan: one slice when the query blocks alone fill the device, else enough slices for
 * about two workgroups per CU, each of at least four tiles); > 0 = that many, at most one per tile.
 * Limits as for jg_sim_topk / jg_sim_topk_grouped, and 0 <= slices <= 1024 with lists of S n_queries k 8 bytes <= 64 MiB when S > 1.  A
 * violated limit, a null operand (g_offsets == NULL with n_groups != 0 included) or another gallery_dtype returns JG_ERR_ARG before
 * anything is enqueued.  n_queries == 0 returns JG_OK and launches nothing; n_gallery == 0, or g_offsets != NULL with n_groups == 0, fills
 * -1 / -inf without merge and keeps the list with it.  jg_debug_last_kernel names what the call launched ("a+b" for two launches).
 * Asynchronous. */
int jg_sim_search(jg_handle* h, const float* queries, int n_queries, const void* gallery, int gallery_dtype /* JG_F32 | JG_F16 */,
                  int n_gallery, int D, int k, const int32_t* g_offsets /* device [n_groups + 1], or NULL: ungrouped */, int n_groups,
                  int gallery_offset, int merge, int slices /* 0: the library chooses */, int32_t* idx, float* score);
/* The cut jg_sim_search makes on a device of num_cu CUs: no handle, no device.  slices_in as jg_sim_search's `slices`.  -> *slices = S,
 * *rows_per_slice = R, *ws_bytes = S n_queries k 8 (0 when S == 1: one slice writes no lists).  JG_ERR_ARG where jg_sim_search refuses
 * the counts (negative ones, k outside 1..128, slices_in > 1024, lists beyond 64 MiB). */
int jg_debug_search_plan(int n_queries, int n_gallery, int k, int num_cu, int slices_in, int* slices, int* rows_per_slice, int64_t* ws_bytes);
/* Coupling (late interaction, MaxSim): rank groups of gallery rows (clips of frames) for queries of several word rows, every word by its
 * best row in the group, without the (all words) x (all rows) matrix.
 * words [n_words][D] fp32; w_offsets_host [n_queries + 1], a HOST array: query q owns word rows w_offsets[q] .. w_offsets[q + 1] - 1.
 * gallery [n_gallery][D] of gallery_dtype (JG_F32 | JG_F16, as jg_sim_search); g_offsets [n_groups + 1], a DEVICE array with the meaning and
 * the safety rule of jg_sim_topk_grouped: read at 0 .. n_groups only, only ever compared with row numbers, the gallery is never addressed
 * through it; offsets that are no non-decreasing partition give an unspecified result, never an access outside the operands.
 * The score: s(w, t) = <words[w], gallery[t]> with the bits jg_sim_topk gives for the gallery widened to fp32; -0.0 counts as +0.0; a NaN s
 * is skipped.  m(w, g) = the max of the non-NaN s(w, t) over the rows of group g, none if there is no such row.  score(q, g): none if any
 * word of q has no m (NaN in `pair`, never a candidate); else the m(w, g) added in fp32 in ascending word order, one sequential chain,
 * divided by (float)W_q with a correctly rounded fp32 division.  A score depends on the rows of its query and its group only: not on
 * slices, tiles, k or what else is in the call.
 * idx / score [n_queries][k]: group_offset + g, best first: the larger score, on equal scores the smaller group; -1 / -inf where there are
 * fewer.  merge as for jg_sim_topk_grouped: pieces cut at group boundaries with disjoint group_offset ranges leave, in any order, the bits
 * of one call.
 * pair (optional, NULL to skip): the dense scores, GROUP-major: pair[g * pair_ld + q], pair_ld >= n_queries, g a local group of this call.
 * The entry first fills pair[g][0 .. n_queries) with NaN for every local group (a launch of its own on the handle's stream); the kernel
 * stores the pairs that have a score.  Nothing outside those entries and the n_queries * k entries of idx / score is written.
 * slices as for jg_sim_search (jg_debug_coupling_plan): a slice owns the groups that BEGIN in its rows and walks on until the last ends.
 * Limits: 1..64 word rows per query; 1 <= k <= 128; D > 0, D % 64 == 0; words and gallery 16-byte aligned; w_offsets_host[0] == 0 and
 * non-decreasing; counts >= 0; group_offset >= 0, group_offset + n_groups <= INT32_MAX; 0 <= slices <= 1024, the lists (S n_queries k 8
 * bytes) at most 64 MiB when S > 1.  A violated limit, a null buffer or another dtype returns JG_ERR_ARG before anything is enqueued or
 * written.  n_queries == 0 returns JG_OK and launches nothing; n_gallery == 0 or n_groups == 0 fills -1 / -inf without merge and keeps the
 * lists with it, pair stays NaN.  The two host tables go to this call's workspace pass.  jg_debug_last_kernel names the coupling launch
 * ("a+b" with the reduction of more than one slice; the NaN fill is not named).  Asynchronous. */
int jg_sim_coupling(jg_handle* h, const float* words, const int32_t* w_offsets_host, int n_queries, const void* gallery,
                    int gallery_dtype /* JG_F32 | JG_F16 */, int n_gallery, int D, int k, const int32_t* g_offsets /* device */, int n_groups,
                    int group_offset, int merge, int slices /* 0: the library chooses */, int32_t* idx, float* score,
                    float* pair /* optional */, int64_t pair_ld);
/* The plan jg_sim_coupling makes: no handle, no device.  Queries are packed in order into tiles of at most 64 word rows, never split;
 * tile_first_query (room for n_queries + 1) [i] = first query of tile i, [*n_tiles] = n_queries.  The cut is jg_debug_search_plan's with the
 * query tiles in place of the query blocks; *ws_bytes = S n_queries k 8 (0 when S == 1).  JG_ERR_ARG where jg_sim_coupling refuses. */
int jg_debug_coupling_plan(const int32_t* w_offsets_host, int n_queries, int n_gallery, int k, int num_cu, int slices_in,
                           int32_t* tile_first_query, int* n_tiles, int* slices, int* rows_per_slice, int64_t* ws_bytes);
/* Ordered coupling: jg_sim_coupling with the words of a query assigned to rows of the group IN WORD ORDER (speech is ordered, and a gesture
 * is time-locked to its word).  The parameter list, the operands and everything jg_sim_coupling documents carry over unchanged: the limits
 * and the refusals before anything is enqueued or written, the HOST w_offsets and the DEVICE g_offsets with their safety rule (read at 0 ..
 * n_groups only, only compared with row numbers), -0.0 as +0.0, idx = group_offset + g best first with ties to the smaller group and -1 /
 * -inf where there are fewer, merge at group boundaries, the optional group-major pair (NaN-filled first), slices and the lists in the
 * workspace (jg_debug_coupling_plan is the plan of this entry too), the two host tables, asynchronous execution.  Only the score differs.
 * With s(w, t) as for jg_sim_coupling, a query's words w_1 .. w_W, and t counting the rows of the group [a, b) clamped to 0 .. n_gallery
 * from a, T = b - a:
 *   M_0(t) = +0.0 for all t;  for i = 1 .. W:  E_i(t) = M_(i-1)(t) + s(w_i, t), one fp32 add, NaN when either operand is;
 *   M_i(t) = the max of the non-NaN E_i(t') over t' <= t, NaN when there is none;
 *   score(q, g) = M_W(T - 1) / (float)W, a correctly rounded fp32 division; none (NaN in pair, never a candidate) when M_W(T - 1) is NaN
 *   or the group has no row.
 * That is the best mean of s(w_i, t_i) over the assignments t_1 <= t_2 <= .. <= t_W -- one row may serve consecutive words, so a query
 * may have more words than the group has rows -- with the sum as one fp32 chain in word order and an exact max: a score depends on the
 * rows of its query and its group only.  With W = 1 it is jg_sim_topk_grouped's score bit for bit; it never exceeds jg_sim_coupling's (fp32
 * addition is monotone) and equals it bit for bit where the words' first arg-max rows are non-decreasing already.
 * jg_debug_last_kernel names the launch ("a+b" with the reduction of more than one slice; the NaN fill is not named). */
int jg_sim_ordered(jg_handle* h, const float* words, const int32_t* w_offsets_host, int n_queries, const void* gallery,
                   int gallery_dtype /* JG_F32 | JG_F16 */, int n_gallery, int D, int k, const int32_t* g_offsets /* device */, int n_groups,
                   int group_offset, int merge, int slices /* 0: the library chooses */, int32_t* idx, float* score,
                   float* pair /* optional */, int64_t pair_ld);
/* The rows behind a result of jg_sim_coupling (ordered == 0) or jg_sim_ordered (ordered != 0): for every returned (query, group) pair, the
 * row each word took.  words .. group_offset: the operands of that call (this piece's, for merged pieces).  idx [n_queries][k], device: its
 * result.  Slot (q, r) is handled iff group_offset <= idx[q][r] < group_offset + n_groups; a slot holding -1 or a group of another piece
 * is not, and its entries of frames and score stay exactly as they were: a caller of merged pieces initialises the two to -1 / NaN and
 * passes every piece with the final idx.
 * A handled slot: frames[(q k + r) frames_ld + i] = the call's local gallery row a + t_i of word i for i < W_q, -1 for W_q <= i < frames_ld;
 * score[q k + r] = the pair's score, bit for bit jg_sim_ordered's (ordered != 0) or jg_sim_coupling's (ordered == 0).
 *   ordered: t_W = the first arg-max of E_W over [0, T); t_i = the first arg-max of E_i over [0, t_(i+1)] for i = W - 1 .. 1; the rows are
 *   non-decreasing, and s at them, added in word order in fp32 and divided by W, is the score.
 *   unordered: t_i = the first arg-max row of s(w_i, .) in the group, where jg_sim_coupling's m(w_i, g) comes from.
 * A handled slot whose pair has no score, or whose group has more than 8192 rows (the limit of jg_spot and jg_attn_matrix), gets -1 in all
 * frames_ld entries and NaN.
 * One workgroup per slot recomputes the group's 64-row tiles for the query's words, keeps one bit per (word, row) -- did this row raise the
 * word's running max -- and backtracks through the bits.  g_offsets is read at the slot's group and the next only, and only clamped and
 * compared; idx is only compared.
 * Limits as for jg_sim_coupling (words per query, k, D, alignment, w_offsets_host, counts, group_offset, dtype) and frames_ld >= the longest
 * query; a violated limit or a null buffer returns JG_ERR_ARG before anything is enqueued or written.  n_queries == 0 returns JG_OK and
 * launches nothing.  Nothing outside the n_queries * k * frames_ld entries of frames and the n_queries * k entries of score is written.
 * The workspace pass holds the uploaded w_offsets only.  jg_debug_last_kernel names the launch.  Asynchronous. */
int jg_sim_align(jg_handle* h, const float* words, const int32_t* w_offsets_host, int n_queries, const void* gallery,
                 int gallery_dtype /* JG_F32 | JG_F16 */, int n_gallery, int D, const int32_t* g_offsets /* device */, int n_groups,
                 int group_offset, const int32_t* idx /* device, [n_queries][k] */, int k, int ordered, int32_t* frames, int frames_ld,
                 float* score);
/* The rows jg_sim_topk_grouped returns, back to (group, position inside the group), on the device: grp[e] = the group whose range holds
 * idx[e] - gallery_offset, pos[e] = the row's offset inside it; both -1 for idx[e] < 0 or a row in no group.  An element-wise binary
 * search over g_offsets (device, [n_groups + 1]); a caller of merged calls passes its global offsets with gallery_offset = 0.  n, n_groups,
 * gallery_offset >= 0; a null buffer (g_offsets when n_groups > 0) or a negative count returns JG_ERR_ARG; n == 0 launches nothing.
 * Only the n entries of grp and pos are written.  Asynchronous. */
int jg_group_of_rows(jg_handle* h, const int32_t* idx, int64_t n, const int32_t* g_offsets, int n_groups, int gallery_offset,
                     int32_t* grp, int32_t* pos);
/* evaluate_spotting.py:39-82: per clip first-argmax frame and its softmax score for word `target`.
 * Limits per clip: <= 1024 words, <= 8192 frames, 0 <= target < words.  The offsets are device arrays (no host sync to
 * validate them): a clip outside the limits gets pred = -1 and score = NaN instead of a result. */
int jg_spot(jg_handle* h, const float* gesture, const float* content, const int32_t* g_offsets, const int32_t* c_offsets,
            const int32_t* target, int n_clips, int D, float temp, int32_t* pred, float* score);
/* evaluate_spotting.py:39-57 (normalize = 1) / utils/plot_heatmap.py:34-59 (normalize = 0) for a ragged batch, and the arg-max of
 * evaluate_spotting.py:72-73 for EVERY word: per clip A_i = softmax((G_i C_i^T) / temp, dim=1)^T, fp32 row-major (W_i, T_i), written at
 * A + a_offsets[i] (device int64 ELEMENT offsets, caller-chosen, non-overlapping, gaps allowed; nothing outside the W_i * T_i elements
 * is written), and per word (in c_offsets order) best_frame = its first arg-max frame, best_score = A_i[w][best_frame] bit for bit.
 * normalize != 0: both operands' rows are F.normalize'd first (x / max(||x||, 1e-12)); 0: the rows as stored.  The logits run on
 * exact-fp32 MFMAs: an entry depends on its two rows alone, duplicate frames give bit-equal columns and ties go to the first frame.
 * Limits per clip as for jg_spot: 1..8192 frames, 1..1024 words; D % 64 == 0; max_frames (1..8192) >= the longest clip sizes the grid.
 * The offsets are device arrays: a clip outside the limits or longer than max_frames gets best_frame = -1 and best_score = NaN for
 * its words and nothing of its A is written; the other clips are computed normally.  Bad arguments (null operands, gesture / content
 * not 16-byte aligned, A without a_offsets, no output at all, max_frames, D, temp <= 0) return JG_ERR_ARG before anything is enqueued.
 * Workspace: with best_frame or best_score the call takes n_clips * 1024 64-bit arg-max keys (8 KB per clip whatever its word count:
 * the host cannot see the word counts; 32 MB for 4000 clips) from the handle's workspace; only the keys of existing words are touched.
 * Asynchronous. */
int jg_attn_matrix(jg_handle* h, const float* gesture, const float* content, const int32_t* g_offsets, const int32_t* c_offsets,
                   int n_clips, int D, int max_frames, float temp, int normalize,
                   float* A, const int64_t* a_offsets,          /* A may be NULL: no matrix is written (one pass over G, the spot-every-word mode) */
                   int32_t* best_frame, float* best_score);     /* [sum W], in c_offsets order; both may be NULL when A is not */
/* The gesture-word heat map along whole talks: jg_attn_matrix's softmax runs over the words of a clip of at most 220 frames, the length
 * the model was trained on; here every frame sees the words a clip of 2 reach + 1 frames centred on it would contain.  All pointers are
 * device pointers.
 *   gesture (n_rows, D) fp32: frame rows of n_tracks tracks, g_offsets [n_tracks + 1] their row offsets (T frames each);
 *   content (n_words, D) fp32: word rows, c_offsets [n_tracks + 1]: track i's words, in transcript order; word_start / word_end [n_words]:
 *     every word's inclusive frame bounds on ITS track's frame axis, non-decreasing along a track, start <= end.
 * Word w is IN REACH of frame f iff start_w - reach <= f <= end_w + reach.  For a frame f in 0..T-1 and a word w in reach of it
 *   P[w][f] = exp(x_wf - m_f) / sum over the words w' in reach of f of exp(x_w'f - m_f),  x_wf = <c_w, g_f> / temp,  m_f = max x_w'f over them;
 * normalize != 0: both rows F.normalize'd first, as in jg_attn_matrix.  With reach >= T every word is in reach of every frame and P is
 * jg_attn_matrix's A.
 * Outputs, each optional (NULL), at least one required; every element of each is written and nothing else is:
 *   band fp32 [n_words][band_pitch]: band[w][j] = P[w][f] for f = start_w - reach + j; NaN where f is outside 0..T-1, beyond end_w + reach,
 *     or undecided.  A word whose range is longer than band_pitch keeps its first band_pitch frames; its best_* still cover the whole range;
 *   best_frame int32 / best_score fp32 [n_words]: the first arg-max of P[w][.] over the word's decided frames (on the track's frame axis)
 *     and that probability, the band entry bit for bit; -1 / NaN when the word has none;
 *   frame_word int32 / frame_prob fp32 [n_rows]: the arg-max word of the frame, counted from the track's first word, the smaller index on
 *     ties, and its probability; -1 / NaN when no word is in reach, and in undecided frames.
 * The work is cut into blocks of 128 frames, aligned to the track's first frame; a block's candidates are the words in reach of any of its
 * frames (one contiguous range: the bounds are non-decreasing), and a block with more than 128 candidates is UNDECIDED in all its frames:
 * lower reach.  The logits run on exact-fp32 MFMAs and have the bits jg_attn_matrix gives the same two rows; for a track of at most 128
 * words with reach >= T, band entries, best_frame and best_score equal jg_attn_matrix's bit for bit.  Determinism: a track's results are
 * a function of its own rows, words and reach, not of the other tracks or of its place in the batch; duplicate frames give bit-equal columns.
 * Limits: tracks of 0..max_frames frames, max_frames 1..2^20 (it sizes the grid); reach 0..1024; n_words * band_pitch < 2^31; D % 64 == 0;
 * gesture / content 16-byte aligned.  A violated limit, a null operand, temp <= 0, band with band_pitch < 1 or no output at all returns
 * JG_ERR_ARG before anything is enqueued; n_tracks == 0 returns JG_OK and launches nothing.  The offsets and bounds are device arrays: a
 * track longer than max_frames, or with rows or words outside the arrays, is undecided as a whole, none of its rows is read, and the other
 * tracks are unaffected.  Bounds that are not non-decreasing, or start > end, give unspecified values for that track and no access outside
 * the operands (every index taken from the search is clamped to the track's words).  Words outside the track are legal and have no frames.
 * Workspace: with best_frame or best_score, n_words 64-bit arg-max keys.  Asynchronous, on the handle's stream. */
int jg_attn_talk(jg_handle* h, const float* gesture, const int32_t* g_offsets, int n_tracks, int64_t n_rows, int max_frames,
                 const float* content, const int32_t* c_offsets, int n_words, const int32_t* word_start, const int32_t* word_end,
                 int D, int reach, float temp, int normalize,
                 float* band, int band_pitch, int32_t* best_frame, float* best_score, int32_t* frame_word, float* frame_prob);
/* evaluate_asd.py:43-51,94-100: pred (n,3) = argmax over the first 2/4/6 candidates */
int jg_asd(jg_handle* h, const float* query, const float* cand, const int32_t* c_offsets, int n, int D, float temp, int32_t* pred);

/* ASD itself, per time window (the arithmetic of evaluate_asd.py:26-51, load_feats + get_similarity_cos, applied to the rows of a window):
 * which of a scene's candidate tracks gestures to the utterance, with what probability, and when.  All pointers are device pointers.
 *   gesture (sum T, D) fp32: frame-level rows of n_tracks tracks, g_offsets [n_tracks + 1] their row offsets;
 *   content (sum W, D) fp32: word-level rows of n_scenes utterances, c_offsets [n_scenes + 1]; word_start / word_end [sum W]: inclusive
 *     frame bounds of every word on the scene's frame axis (info["word_boundaries"]); both may be NULL when win == 0;
 *   trk [sum P], s_offsets [n_scenes + 1]: scene i's candidates are the tracks trk[s_offsets[i] : s_offsets[i + 1]] (indices into
 *     g_offsets); a track may be a candidate of many scenes and more than once in one.  Frame t of a scene is row t of each of its tracks;
 *   win, hop: window j covers frames lo = j hop .. hi = lo + win - 1; win == 0: one window over every frame and every word (clip-level ASD;
 *     hop ignored);  w_offsets [n_scenes + 1]: scene i owns pred rows w_offsets[i] .. w_offsets[i + 1] - 1 (n_win_i windows, the caller's
 *     choice);  p_offsets [n_scenes] int64: ELEMENT offset of the scene's (n_win_i, P_i) block in prob / cosv (caller-chosen, gaps allowed);
 *     max_windows >= every n_win_i sizes the grid.
 * Per window: q = mean of the content rows of the words with word_end >= lo and word_start <= hi; candidate p is PRESENT if its track has
 * a frame in [lo, hi], g_p = mean of those frames; cos_p = <q, g_p> / max(|q| |g_p|, 1e-8); prob = softmax(cos / temp) over the present
 * candidates, evaluated as exp(x - max) / sum; pred = first arg-max, an index into the scene's candidate list.  An absent candidate gets
 * prob 0 and cosv NaN.  A window without a word or without a present candidate is UNDECIDED: pred -1, its prob and cosv rows NaN.
 * Outputs: prob fp32 (n_win_i, P_i) row-major at p_offsets[i]; cosv the same layout, optional (NULL); pred int32 [w_offsets[n_scenes]].
 * Determinism: a window's cosv, prob and pred are a function of its own rows, added in ascending row order, and of nothing else -- not of
 * hop, of the window's place in its workgroup, of the scene's place in the batch or of the other scenes.  The same [lo, hi] reached through
 * different (hop, j) gives the same bits; win == 0 gives the bits of one window with win >= the longest track; a track listed twice gives
 * bit-equal columns and the tie goes to the first.
 * Limits per scene: 1..64 candidates, 1..1024 words, tracks of 1..8192 frames, 1..max_windows windows, trk entries inside 0..n_tracks-1.
 * The offsets are device arrays: a scene outside the limits is undecided in ALL of its windows, none of its rows is read, and the other
 * scenes are computed normally.  Bad arguments return JG_ERR_ARG before anything is enqueued: null operands, D <= 0, D % 64, D > 1024,
 * win < 0, win > 8192, hop < 1 with win > 0, temp <= 0, max_windows outside 1..8192, win > 0 without word bounds, gesture / content not
 * 16-byte aligned.  n_scenes == 0 returns JG_OK and launches nothing.  Nothing outside the described elements is written; no workspace
 * is used.  Asynchronous. */
int jg_asd_windows(jg_handle* h, const float* gesture, const int32_t* g_offsets, int n_tracks, const float* content, const int32_t* c_offsets,
                   const int32_t* word_start, const int32_t* word_end, const int32_t* trk, const int32_t* s_offsets, int n_scenes, int D,
                   int win, int hop, const int32_t* w_offsets, const int64_t* p_offsets, int max_windows, float temp,
                   float* prob, float* cosv /* may be NULL */, int32_t* pred);

/* Audio-visual offset and confidence per clip from the two streams of GestSync window embeddings (jg_gestsync_clip,
 * jg_gestsync_audio_clip); no counterpart in the reference tree, the SyncNet convention.  All pointers are device pointers.
 *   vid (sum Tv, D), aud (sum Ta, D) fp32 rows, used as stored; v_offsets / a_offsets [n_clips + 1]: clip i owns video rows
 *   v_offsets[i] .. v_offsets[i + 1] - 1 (Tv) and audio rows likewise (Ta; the two may differ).
 * For a shift d in -R .. R (R = max_shift) the pairs are (t, t + d) with 0 <= t < Tv and 0 <= t + d < Ta, n_d of them, and
 *   curve[d + R] = (1 / n_d) sum_t <v_t, a_{t+d}> / max(|v_t| |a_{t+d}|, 1e-8), summed in ascending t;  NaN when n_d < min_overlap;
 *   offset = the d of the first maximum in ascending d over the non-NaN entries (np.nanargmax);
 *   conf   = that maximum minus the median of the non-NaN entries (np.nanmedian).
 * Sign: offset d > 0 means that the audio row matching video row t is row t + d.
 * Outputs: curve fp32 [n_clips][2R + 1] (may be NULL), offset int32 [n_clips], conf fp32 [n_clips].
 * A clip's result is a function of its own rows: not of its place in the batch nor of n_clips.  The offsets are device arrays: a clip
 * with Tv or Ta outside 1..8192, or without a non-NaN shift, gets offset 0, conf NaN and a NaN curve row; nothing of it is read (in the
 * first case) and the other clips are computed normally.
 * Bad arguments return JG_ERR_ARG before anything is enqueued: null operands, D <= 0, D % 64, D > 1024, max_shift outside 0..64,
 * min_overlap < 1, vid / aud not 16-byte aligned, n_clips < 0.  n_clips == 0 returns JG_OK and launches nothing.  Nothing outside the
 * described elements is written; no workspace is used.  Asynchronous.
 * Cost: ONE workgroup (one CU) walks a clip's video rows in blocks of 32, in order -- that is what keeps the per-shift sums in
 * ascending t without scratch -- so the parallelism comes from n_clips.  A batch of many short clips is the intended use (4000 clips of
 * 150 rows, D = 1024, R = 15: 3.7 ms on MI355X); a single clip of 8192 rows is 256 blocks on one CU -- 16.6 ms at D = 1024, R = 15 and
 * 31 ms at R = 64, measured, while the rest of the device idles: jg_sync_offset_windows (below) spreads a long track over every CU,
 * takes tracks beyond 8192 rows and gives the same bits for one window over all rows. */
int jg_sync_offset(jg_handle* h, const float* vid, const int32_t* v_offsets, const float* aud, const int32_t* a_offsets,
                   int n_clips, int D, int max_shift, int min_overlap,
                   float* curve /* may be NULL */, int32_t* offset, float* conf);

/* The audio-visual offset as a function of time, of tracks of any length, and of several video tracks against one audio track.  All
 * pointers are device pointers.
 *   Clip i is video track i: rows v_offsets[i] .. v_offsets[i + 1] - 1 of vid (Tv of them; vid has n_vid_rows rows).  Its audio track is
 *   a_of[i], or track i when a_of is NULL (then n_aud must equal n_clips); audio track j owns rows a_offsets[j] .. a_offsets[j + 1] - 1 of
 *   aud (Ta).  Many clips may name the same audio track (which face is in sync with this audio) without copying it.
 * Band (the sync heat map): band[(v0 + t)][d + R] = <v_t, a_{t+d}> / max(|v_t| |a_{t+d}|, 1e-8) for d = -R .. R (R = max_shift), NaN where
 *   t + d is outside 0 .. Ta - 1; fp32 [n_vid_rows][2R + 1], indexed by the GLOBAL video row v0 + t.  Optional output: with band == NULL the
 *   same array (n_vid_rows (2R + 1) floats) is taken from the handle's workspace, and the results are the same bits.  A cosine has the bits
 *   jg_sync_offset computes for the same two rows, and depends on its two rows alone.
 * Windows: window j of clip i covers video rows lo = j hop .. hi = min(lo + win, Tv) - 1; win == 0: one window over all rows (hop ignored).
 *   Clip i owns the result rows w_offsets[i] .. w_offsets[i + 1] - 1, the number of windows being the caller's choice (to cover a track:
 *   Tv <= win ? 1 : ceil((Tv - win) / hop) + 1); max_windows >= every count sizes the grid.  For a shift d the pairs are (t, t + d) with
 *   lo <= t <= hi and 0 <= t + d < Ta, n_d of them; curve[d + R] = the sum of the band entries over those t in ascending t (with the
 *   compensation term jg_sync_offset uses) / n_d, NaN when n_d < min_overlap; offset and conf from the curve exactly as in jg_sync_offset.
 * Outputs: curve fp32 [w_offsets[n_clips]][2R + 1] (may be NULL), offset int32 and conf fp32 [w_offsets[n_clips]].
 * Determinism: a window's result is a function of its own rows -- not of hop, j, the clip's place in the batch or the other clips.  The same
 *   [lo, hi] reached through different (hop, j) gives the same bits; win == 0, or win >= Tv with j = 0, gives jg_sync_offset's bits for the
 *   same clip (Tv, Ta within that entry's limits, a_of NULL); clips that share a video row set and an audio track give bit-equal results.
 * Limits: tracks of 1..max_rows rows, max_rows 1..2^20; max_windows 1..2^20; max_shift, min_overlap, D and alignment as for jg_sync_offset;
 *   win >= 0, hop >= 1 when win > 0, n_vid_rows >= 0, n_vid_rows (2R + 1) < 2^40.  A violated limit or a null buffer returns JG_ERR_ARG
 *   before anything is enqueued; n_clips == 0 returns JG_OK and launches nothing.  The offsets are device arrays: a clip with Tv or Ta
 *   outside 1..max_rows, v0 + Tv > n_vid_rows, an a_of entry outside 0..n_aud-1, or more than max_windows windows is UNDECIDED in all its
 *   windows (offset 0, conf NaN, NaN curve rows): none of its rows is read, none of its band rows is written, the other clips are
 *   unaffected.  A window with lo >= Tv, or without a non-NaN shift, is undecided alone.  Nothing outside the described elements is written.
 * Cost: the band is computed once by a (clip, block of 32 rows) grid, so one long track uses every CU; the windows then read
 *   n_windows win (2R + 1) band entries -- hop = 1 with win = 8192 is the caller's choice -- each window's sum in order, so ONE window
 *   over a long track is a sequential walk (8192 rows: 0.3 ms).  For batches of short clips the band is an extra write and read (74 MB
 *   for 4000 clips of 150 rows at R = 15) and, with band == NULL, workspace: jg_sync_offset, which needs neither, remains the entry for
 *   those (measured on MI355X the two are within 20 % of each other there; one clip of 8192 rows: 0.42 ms here, 19.6 ms there).
 *   Asynchronous. */
int jg_sync_offset_windows(jg_handle* h,
        const float* vid, const int32_t* v_offsets, int n_clips, int64_t n_vid_rows, int max_rows,
        const float* aud, const int32_t* a_offsets, int n_aud, const int32_t* a_of /* device [n_clips] or NULL */,
        int D, int max_shift, int min_overlap, int win, int hop,
        const int32_t* w_offsets /* device [n_clips + 1] */, int max_windows,
        float* band /* may be NULL */, float* curve /* may be NULL */, int32_t* offset, float* conf);

/* ---- multi-GPU exchange.  The reference is single-process (its only parallelism is the --rank / --nshard file-list split of
 *      preprocess/extract_gestsync_feats.py:366-370); clips shard with no data-path collective, and the ONE exchange of the path is the
 *      gallery all-gather in front of the retrieval similarity matrix (+ a counter all-reduce for R@K / spotting / ASD).  These entries give a
 *      consumer of the C ABI that exchange on RCCL over xGMI without PyTorch: one communicator per handle (= per rank = per GPU), collectives
 *      enqueued on the handle's stream.  librccl.so is bound with dlopen at the first call (no link-time dependency).  jegal_amd/dist.py does
 *      the same through torch.distributed (backend "nccl" = RCCL). ---------------------------------------------------------------------- */
#define JG_COMM_ID_BYTES 128
/* rank 0: ncclGetUniqueId into a 128-byte host buffer, to be handed to every rank by the launcher (a file, MPI, a socket, torchrun's store) */
int jg_comm_get_unique_id(char* id128_host);
/* collective over all ranks: ncclCommInitRank on the handle's device */
int jg_comm_init(jg_handle* h, const char* id128_host, int rank, int world);
int jg_comm_destroy(jg_handle* h);
/* recv (world * bytes_per_rank bytes, device) = the ranks' send buffers (bytes_per_rank bytes each, device) in rank order */
int jg_allgather(jg_handle* h, const void* send, void* recv, int64_t bytes_per_rank);
/* in place sum over the ranks of n int64 counters (device) */
int jg_allreduce_sum_i64(jg_handle* h, int64_t* buf, int n);

/* ---- profiling: HIP-event timing per stage on the handle's stream -------------------------- */
enum { JG_ST_STACK = 0, JG_ST_CONV1, JG_ST_POOL, JG_ST_CONV, JG_ST_GEMM, JG_ST_ATTN, JG_ST_NORM, JG_ST_MISC, JG_ST_CONV1_AUX, JG_ST_COUNT };
/* on: 0 = off, 1 = every launch is bracketed by two events, 2 + stage = only the launches of that stage are (the other
 * launches of the step then run back to back, as in an unprofiled step) */
int jg_profile_enable(jg_handle* h, int on);
/* synchronises, then returns accumulated milliseconds and launch count of a stage since the last reset */
int jg_profile_get(jg_handle* h, int stage, double* ms, int64_t* launches);
int jg_profile_reset(jg_handle* h);
const char* jg_stage_name(int stage);
/* bytes currently held by the workspace arena */
int64_t jg_workspace_bytes(jg_handle* h);

#ifdef __cplusplus
}
#endif
#endif
