// Build-independent declarations of libjegal_hip (gfx950 only): everything that does not depend on the 16-bit operand type.
// Included once, global namespace, by both kernel builds (common.h includes it).  The rule of the two builds is in common.h:
// a kernel with no 16-bit operand is compiled once (elementwise_f32.hip, metrics.hip) and its launcher is declared here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>

// op 0: conv2 (the count itself); op 1: conv3 (3x3, stride 2, pad 1: rows whose window ends above s2); op 2: conv4 and op 3: conv5
// (3x3, vertical stride 1, pad 1: one row fewer each)
__host__ __device__ inline int conv_skip_decode(int w, int op) {
    const int s3 = w / 2;
    const int s = op == 0 ? w : s3 - (op - 1);
    return s > 0 ? s : 0;
}
// one layer of the compaction (launch_conv_rowmaps)
struct ConvRowMap {
    int OH, OW, op;           // output geometry of the layer and its conv_skip_decode op
    int* map;                 // [NF*OH*OW] (only the first *total entries are meaningful)
    int* base;                // [NF + 1] scratch: exclusive prefix of the images' computed rows
    int* total;               // device word
};
constexpr int CONV1_ZHDR_WORDS = 64;        // header of conv1's zero-scan scratch: 32 words of zconst, then ...
constexpr int CONV1_ROWSKIP_WORD = 32;      // ... the min over the launch's positions of conv2's position-independent leading rows (debug only)

enum { LN_STD = 0, LN_ANNOTATED = 1 };

// ---- per-handle engine state shared with the launchers ---------------------------------------------------------
// Tuning / A-B switches and the per-device resources a launch needs.  One instance per jg_handle (engine.h), passed to
// the launchers: two handles -- on one device or on two -- never see each other's settings.
struct EngineOpts {
    int device = 0;
    int num_cu = 256;
    const void* zeros = nullptr;         // 256-byte zero page on `device` (LDS-DMA source for padding taps / K tails)
    bool gemm_glds = true;               // LDS-DMA GEMM kernels (false: register-staged gemm_kernel everywhere)
    bool gemm_persistent = true;
    bool gemm_big_tile = true, gemm_small_tile = true, gemm_tall_tile = true;
    int gemm_tile = 0;                   // plain GEMMs: 0 = pick by the cost estimate (plan_gemm), 1 / 2 / 3 = force the 128x128 / 256x128 / 256x256 tile
    int gemm_counted = 1;                // counted s_waitcnt between a tile's epilogue stores and the next tile's first DMA
    int gemm_stagger = 0;                // 10-ns ticks per phase (0: default policy, -1: off)
    bool lanes_active = false;           // the launch is part of a two-lane batch (api.hip, run_in_lanes): the other lane's kernels already
                                         // spread the store bursts, the default de-phasing only costs time there (12.22 -> 12.16 ms per step)
    bool attn_mfma = true;
    bool conv1_zero_skip = true;
    bool conv1_mfma16 = true;            // conv1_direct_kernel's MFMA waves on 16x16x32 MFMAs (false: 32x32x16, the round-1/2 form)
    char* kname = nullptr;               // kernel check points (jg_debug_last_kernel): the launchers write the name of the instance they
                                         // launch here, with its template arguments (KNAME_LEN bytes; nullptr: not recorded)
};
constexpr int KNAME_LEN = 96;
// printf-style into kname (if any): host side of a launcher
template <class... T>
inline void record_kernel(char* kname, const char* fmt, T... v) {
    if (kname) snprintf(kname, KNAME_LEN, fmt, v...);
}
hipError_t engine_opts_init(EngineOpts& o, int device);      // queries the CU count, allocates the zero page (current device = `device`)
void engine_opts_release(EngineOpts& o);

// ---- launchers with one definition and no 16-bit type in their signature (each returns hipGetLastError()) ----------
// packed_bytes >= 0: frames whose metadata points outside [0, packed_bytes) or is misaligned come out zero instead of being read
hipError_t launch_unpack_masked(const uint8_t* packed, const int* row0, const long long* offs, int n_frames, uint8_t* dst, hipStream_t s,
                                long long packed_bytes = -1);
// offs != nullptr: packed source -- frame f's rows max(mask_y[f] + 1, 0) .. H-1 start at src + offs[f] (src_bytes = size of src)
hipError_t launch_mask_resize(const uint8_t* src, int T, int H, int W, const int* mask_y_dev, uint8_t* dst, hipStream_t s,
                              const long long* offs = nullptr, long long src_bytes = 0);
size_t conv1_zmask_elems(int nclip, int T);
const int* conv1_s2_counts(const unsigned* zscratch, int nclip, int T, int pad);     // [nclip*P] per position: conv2's position-independent leading rows
// compaction maps of the conv layers behind conv1 from the per-position counts s2 (NF positions = images)
hipError_t launch_conv_rowmaps(const int* s2, int NF, const ConvRowMap* layers, int nlayers, hipStream_t s);
size_t conv1_edge_elems(long positions);
hipError_t launch_transpose_tokens(const float* in, int N, int L, int D, float* out, hipStream_t s);
hipError_t launch_l2norm(const float* in, float* out, int rows, int D, hipStream_t s);
hipError_t launch_xlmr_embed(const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word, const float* pos,
                             const float* type, float* out, hipStream_t s);
// part [rows][P][2] (sum, sum of squares per 64-column block, P = D / 64) -> stats [rows][2] = (mean, 1 / sqrt(var_biased + 1e-5))
hipError_t launch_ln_stats(const float* part, int rows, int P, float* stats, hipStream_t s);
hipError_t launch_mask_i32_f32(const int32_t* in, float* out, long n, hipStream_t s);
hipError_t launch_logmel(const float* wav, int B, int n_samples, const float* mel_basis, float* out, hipStream_t s);
size_t col_sum_scratch_elems(int K);
size_t rc_scratch_elems(int nclips, int K);
// the shapes launch_rc_bias takes (its kernels' own limits; the GEMM that consumes the result has its rules in plan_gemm)
inline bool rc_bias_ok(int N, int K, int tiled) { return (K == 512 || K == 2048) && (!tiled || K == 512) && !(N & 31); }
hipError_t launch_ragged_mean(const float* x, const int32_t* offsets, int n, int D, float* out, hipStream_t s);
hipError_t launch_sim_rank(const float* e1, const float* e2, int n_local, int n_total, int row_offset, int D,
                           int32_t* rank, int32_t* ties, hipStream_t s);
hipError_t launch_spot(const float* g, const float* c, const int32_t* goff, const int32_t* coff, const int32_t* target,
                       int n, int D, float temp, int32_t* pred, float* score, hipStream_t s);
// A (optional; with aoff, int64 element offsets per clip) and / or best_frame / best_score (optional; they need keys: attn_matrix_key_elems(n)
// words of scratch).  A clip outside the limits (1..8192 frames, <= max_frames, 1..1024 words) is left out: its words read -1 / NaN
size_t attn_matrix_key_elems(int n_clips);
hipError_t launch_attn_matrix(const float* g, const float* c, const int32_t* goff, const int32_t* coff, int n, int D, int max_frames,
                              float temp, int normalize, float* A, const int64_t* aoff, unsigned long long* keys,
                              int32_t* best_frame, float* best_score, hipStream_t s);
hipError_t launch_asd(const float* q, const float* cand, const int32_t* coff, int n, int D, float temp,
                      int32_t* pred2, hipStream_t s);
