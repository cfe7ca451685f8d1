// Build-independent declarations of libjegal_hip (gfx950 only): everything that does not depend on the 16-bit operand type.
// Included once, global namespace, by both kernel builds (common.h includes it).  The rule of the two builds is in common.h:
// a kernel with no 16-bit operand is compiled once (elementwise_f32.hip and the metric units retrieval.hip, spotting.hip, asd.hip,
// sync_offset.hip) and its launcher is declared here, with every limit its entry refuses on beside it; so are the launchers of
// gsa_kernels.hip, whose output type (fp16 / fp32) is a run-time flag and which no bf16 handle reaches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include "conv1_panel.h"

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

// ---- layouts that a writer and a reader share -------------------------------------------------------------------
// Each is defined here once; the kernel (or host loop) that writes it and the ones that read it call the same function, and a
// static_assert pins it to points worked out by hand from the formula in its comment.  (In the register-tight kernels a function is
// written with the integer widths and the association of the address expression it stands for: see the overloads of x16t_row_off.)
//
// Tiled token plane x16t (N = 512 columns, row tiles of 128).  The residual stream of the fused transformer is one fp16 plane: in a
// post-norm transformer the LayerNorm output is rounded to fp16 as the next GEMM's operand anyway, and carrying the residual at that
// precision costs 1-5 % of the feature error (oracle/precision_families.py) for no extra bytes and no codec arithmetic.
// The plane is stored in the MFMA fragment order of the 128x512 LN kernel:
//   x16t element (m, n): R*65536 + (n>>6)*8192 + ((m&127)>>4)*1024 + ((n&63)>>4)*256 + (m&15)*16 + (n&15),  R = m>>7
//        (a wave's 8-byte accesses of one (j, i) block are one contiguous 512 B; a 64-wide k-tile of a 128-row
//         panel is one contiguous 16 KB -> the consumer GEMMs' LDS-DMA reads it with a_tiled addressing)
constexpr int X16T_TILE = 65536;            // 128 rows x 512 columns
constexpr int X16T_COLBLK = 8192;           // ... of which 128 rows x 64 columns (one k-tile of the consumer GEMMs)
constexpr int X16T_ROWBLK = 1024;           // ... of which 16 rows x 64 columns
constexpr int X16T_QUAD = 256;              // ... of which 16 rows x 16 columns, row-major (16 elements per row)
__host__ __device__ __forceinline__ constexpr long x16t_row_off(long m) { return (m >> 7) * X16T_TILE + ((m & 127) >> 4) * X16T_ROWBLK + (m & 15) * 16; }
__host__ __device__ __forceinline__ constexpr long x16t_row_off(int m) { return (long)(m >> 7) * X16T_TILE + ((m & 127) >> 4) * X16T_ROWBLK + (m & 15) * 16; }
__host__ __device__ __forceinline__ constexpr long x16t_col_off(int n) { return (long)(n >> 6) * X16T_COLBLK + ((n & 63) >> 4) * X16T_QUAD + (n & 15); }
__host__ __device__ __forceinline__ constexpr long x16t_index(long m, int n) { return x16t_row_off(m) + x16t_col_off(n); }
static_assert(x16t_index(0, 0) == 0 && x16t_index(1, 1) == 17 && x16t_index(16, 16) == 1024 + 256, "x16t: rows of 16 inside a quad, quads, row blocks");
static_assert(x16t_index(128, 64) == 65536 + 8192 && x16t_index(300, 500) == 2 * 65536 + 7 * 8192 + 2 * 1024 + 3 * 256 + 12 * 16 + 4, "x16t: tiles and column blocks");
static_assert(x16t_row_off(300) == x16t_row_off(300L), "x16t: the two widths agree");

// Entry of a compacted conv row map (ConvGeom::rowmap): the full output row (img*OH + oh)*OW + ow in the low 24 bits, the image's
// count s2 (conv2's position-independent leading rows) above them.
constexpr int ROWMAP_ROW_BITS = 24;
constexpr int ROWMAP_MAX_ROWS = 1 << ROWMAP_ROW_BITS;       // full output rows of a launch: row < ROWMAP_MAX_ROWS
constexpr int ROWMAP_MAX_S2 = 255;
__host__ __device__ __forceinline__ constexpr int rowmap_entry(int row, int s2) { return row | (s2 << ROWMAP_ROW_BITS); }
__host__ __device__ __forceinline__ constexpr int rowmap_row(int e) { return e & (ROWMAP_MAX_ROWS - 1); }
__host__ __device__ __forceinline__ constexpr int rowmap_s2(int e) { return (int)((unsigned)e >> ROWMAP_ROW_BITS); }
static_assert(rowmap_entry(5, 3) == 0x03000005 && rowmap_row(0x03000005) == 5 && rowmap_s2(0x03000005) == 3, "row map entry");
static_assert(rowmap_row(rowmap_entry(ROWMAP_MAX_ROWS - 1, ROWMAP_MAX_S2)) == 0xffffff && rowmap_s2(rowmap_entry(ROWMAP_MAX_ROWS - 1, ROWMAP_MAX_S2)) == 255,
              "row map entry: both limits survive the sign bit");

// Accumulator of a 32x32 MFMA: register i of the lane half `half` (lane >> 5) holds row (i&3) + 8*(i>>2) + 4*half of column lane & 31.
__host__ __device__ __forceinline__ constexpr int mfma32_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }
static_assert(mfma32_row(0, 0) == 0 && mfma32_row(5, 1) == 13 && mfma32_row(15, 1) == 31, "32x32 accumulator rows");

// LayerNorm partial sums part[row][nblk][2]: (sum, sum of squares) of the row's 64-column block blk, nblk = D / 64.
__host__ __device__ __forceinline__ constexpr long ln_part_index(long row, int nblk, int blk) { return 2 * (row * nblk + blk); }
static_assert(ln_part_index(0, 12, 1) == 2 && ln_part_index(3, 12, 5) == 82, "LayerNorm partial sums");

// conv1's weight panel Wd[slot][ch][16], conv1_wd_index and the CONV1_BIAS_* constants: conv1_panel.h (shared with the HIP-free packing unit)

// conv1's zero-scan scratch (launch_conv1_scan writes it; launch_conv1_direct and the conv stack behind it read it), in 32-bit words:
//   header of CONV1_ZHDR_WORDS: words 0..31 zconst (64 values of the 16-bit type: what conv1 gives over an all-zero patch), word
//   CONV1_ROWSKIP_WORD the min over the launch's positions of s2 (debug only); then the frame masks [nclip*T], the position masks
//   [nclip*P] and the per-position counts s2 [nclip*P] (conv2's position-independent leading rows), P = T + 2*pad - 4.
constexpr int CONV1_ZHDR_WORDS = 64;
constexpr int CONV1_ROWSKIP_WORD = 32;
constexpr int CONV1_SCAN_MAX_PAD = 12;      // the scratch is sized for this pad (conv1_zmask_elems)
struct Conv1Scan {
    unsigned* z;                            // the scratch (may be null when only the sizes are asked for)
    size_t frame_off, pos_off, s2_off, words;
    void* zconst() const { return z; }
    int* rowskip_min() const { return reinterpret_cast<int*>(z) + CONV1_ROWSKIP_WORD; }
    unsigned* frame_mask() const { return z + frame_off; }
    unsigned* pos_mask() const { return z + pos_off; }
    int* s2() const { return reinterpret_cast<int*>(z + s2_off); }
};
inline Conv1Scan conv1_scan_view(unsigned* zscratch, int nclip, int T, int pad) {
    Conv1Scan v;
    v.z = zscratch;
    v.frame_off = CONV1_ZHDR_WORDS;
    v.pos_off = v.frame_off + (size_t)nclip * T;
    v.s2_off = v.pos_off + (size_t)nclip * (T + 2 * pad - 4);
    v.words = v.s2_off + (size_t)nclip * (T + 2 * pad - 4);
    return v;
}

// blocks of 256 threads for a grid-stride loop over `total` items
inline int grid_for(long total) { return (int)((total + 255) / 256 < 65536 * 4 ? (total + 255) / 256 : 65536 * 4); }

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
    // Walk factors (options lane_walk_gemm / _conv / _lnf / _conv1, "lane_walk" = all four; 1..LANE_WALK_MAX): inside a two-lane batch a
    // persistent kernel of the family launches min(tiles, factor x num_cu) workgroups instead of num_cu, so that each walks 1/factor of
    // the tiles and a CU changes hands -- possibly to the other lane's next kernel -- whenever one exits.  Tile choice, cost estimates
    // and admission keep using num_cu; the work per tile does not depend on which workgroup runs it.  Built-in default 1 (the planner
    // as jg_debug_gemm_plan shows it); engine_opts_init sets the production values of a handle.
    enum { LW_GEMM = 0, LW_CONV = 1, LW_LNF = 2, LW_CONV1 = 3 };
    int lane_walk[4] = {1, 1, 1, 1};
    bool attn_mfma = true;
    bool conv1_zero_skip = true;
    bool conv1_mfma16 = true;            // conv1_direct_kernel's MFMA waves on 16x16x32 MFMAs (false: 32x32x16, the round-1/2 form)
};
constexpr int LANE_WALK_MAX = 4;

// ---- which kernel a launcher launched (jg_debug_last_kernel) ---------------------------------------------------
// Every launcher a kernel check point reaches calls record_kernel where it chooses its instance, directly in front of the launch and
// behind its last refusal: the name with its template arguments, or "a_kernel+b_kernel" for a launcher of two kernels.  The name goes to
// the calling thread's sink: KNAME_LEN bytes that a check point opens for the length of its call (engine.h: KernelNameScope; jg_sim_search opens one too) and
// nullptr, nothing recorded, everywhere else.  One sink per thread, defined once (gemm_plan.hip), for both kernel builds.
constexpr int KNAME_LEN = 96;
char*& kernel_name_sink();
template <class... T>
inline void record_kernel(const char* fmt, T... v) {
    if (char* const sink = kernel_name_sink()) snprintf(sink, KNAME_LEN, fmt, v...);
}
inline void record_kernel(const char* name) { record_kernel("%s", name); }
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
// Windows of long gesture tracks (elementwise_f32.hip; the rule: jg_track_windows).  table: device [n_windows][4] int32 = (span first row,
// span length, core offset inside the span, core length), 16-byte aligned.  span_gather: x32 (n_windows, span_max, D) = p32 rows + pe rows,
// zero beyond a span's length, mask (n_windows, span_max) = 1 / 0; pe needs span_max rows.  core_compact: the core rows of
// in (n_windows, span_max, D) elements of elem_bytes (2 or 4; D elem_bytes % 16 == 0) -> out row (span first row + s).
constexpr int TRACK_SPAN_MAX = 500;          // rows of JEGAL's positional table (modules.py:136): win + 2 ctx <= TRACK_SPAN_MAX
hipError_t launch_span_gather(const float* p32, const float* pe, const int32_t* table, int n_windows, int span_max, int D, float* x32, float* mask,
                              hipStream_t s);
hipError_t launch_core_compact(const void* in, int elem_bytes, const int32_t* table, int n_windows, int span_max, int D, void* out, hipStream_t s);
// Test aid (option ws_poison): fill with 0xff bytes (fp16 / fp32 NaN) by a kernel of our own on the stream -- NOT hipMemsetAsync: two 1-GiB
// hipMemsetAsync fills running concurrently on two streams were observed to overlap the kernels enqueued BEHIND them on their own stream
// (tools/experiments/xlmr_race/xl_poison_probe.py, round 6)
hipError_t launch_poison(void* p, size_t bytes, hipStream_t s);
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
// per query row the k <= SIM_TOPK_MAX_K best gallery rows (idx = gallery_offset + j, best first; -1 / -inf where there are fewer); merge:
// idx / score hold an earlier result for other gallery rows and the best k of the union are left.  No scratch.
constexpr int SIM_TOPK_MAX_K = 128;
hipError_t launch_sim_topk(const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k, int gallery_offset,
                           int merge, int32_t* idx, float* score, hipStream_t s);
// the same over groups of gallery rows (group g = local rows g_offsets[g] .. g_offsets[g + 1] - 1, device array of n_groups + 1 entries): per
// query row the k best groups, each as its best row (one row per group at most; rows in no group are never returned).  The offsets are
// only ever compared with row numbers: whatever they hold, nothing outside the operands is read.  No scratch.
hipError_t launch_sim_topk_grouped(const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k,
                                   const int32_t* g_offsets, int n_groups, int gallery_offset, int merge, int32_t* idx, float* score,
                                   hipStream_t s);
// jg_sim_search: either of the two above (g_offsets == nullptr: ungrouped) over a gallery of fp32 or fp16 rows cut into `slices` slices of
// slice_rows rows (whole 64-row tiles, none empty: a SimSearchPlan), one workgroup per query block and slice, and a second kernel that
// reduces the slices' lists (keys: slices x n_queries x k words of scratch, every one written) into idx / score.  slices == 1 is one
// launch straight into idx / score and needs no keys.  The bits do not depend on the cut.
constexpr int SIM_SEARCH_MAX_SLICES = 1024;  // slices of one call, asked for or chosen
constexpr int SIM_SEARCH_MAX_WS = 64 << 20;  // bytes of the slices' lists
constexpr int SIM_SEARCH_WG_PER_CU = 2;      // workgroups per CU the chosen cut aims at: what fits a CU's LDS at k <= 64
constexpr int SIM_SEARCH_MIN_TILES = 4;      // ... and the fewest tiles a chosen slice walks
struct SimSearchPlan {
    int slices, slice_rows;
    long long ws_bytes;                      // slices n_queries k 8: the lists; 0 with one slice, which writes none
};
// The cut of a call, a pure function (jg_debug_search_plan shows it).  slices_in == 0: as many slices as bring the launch to
// SIM_SEARCH_WG_PER_CU workgroups per CU -- one when the query blocks alone fill the device -- of at least SIM_SEARCH_MIN_TILES tiles, at
// most SIM_SEARCH_MAX_SLICES, with lists inside SIM_SEARCH_MAX_WS.  slices_in > 0: that many, at most one per tile.  The tiles are then
// dealt out evenly, which may leave fewer slices than asked for, none of them empty.  false: a count the entry refuses.
// (n_blocks workgroups per slice and lists of `list` bytes per slice: jg_sim_search's query blocks, jg_sim_coupling's query tiles)
inline bool sim_slice_cut(long long n_blocks, long long list, int n_gallery, int num_cu, int slices_in, SimSearchPlan& p) {
    const long long tiles = ((long long)n_gallery + 63) / 64, qblocks = n_blocks;
    long long s = slices_in;
    if (!slices_in) {
        s = qblocks >= num_cu || !qblocks ? 1 : ((long long)SIM_SEARCH_WG_PER_CU * num_cu + qblocks - 1) / qblocks;
        if (s > tiles / SIM_SEARCH_MIN_TILES) s = tiles / SIM_SEARCH_MIN_TILES;
        if (s > SIM_SEARCH_MAX_SLICES) s = SIM_SEARCH_MAX_SLICES;
        if (list && s > SIM_SEARCH_MAX_WS / list) s = SIM_SEARCH_MAX_WS / list;
    }
    if (s > tiles) s = tiles;
    if (s < 1) s = 1;
    const long long per = tiles ? (tiles + s - 1) / s : 1;       // tiles per slice
    s = tiles ? (tiles + per - 1) / per : 1;
    if (s > 1 && s * list > SIM_SEARCH_MAX_WS) return false;
    p.slices = (int)s;
    p.slice_rows = (int)(per * 64 < INT32_MAX ? per * 64 : INT32_MAX & ~63);
    p.ws_bytes = s > 1 ? s * list : 0;
    return true;
}
inline bool sim_search_plan(int n_queries, int n_gallery, int k, int num_cu, int slices_in, SimSearchPlan& p) {
    if (n_queries < 0 || n_gallery < 0 || k < 1 || k > SIM_TOPK_MAX_K || num_cu < 1 || slices_in < 0 || slices_in > SIM_SEARCH_MAX_SLICES)
        return false;
    return sim_slice_cut(((long long)n_queries + 63) / 64, (long long)n_queries * k * 8, n_gallery, num_cu, slices_in, p);
}
hipError_t launch_sim_search(const float* queries, const void* gallery, bool gallery_f16, int n_queries, int n_gallery, int D, int k,
                             const int32_t* g_offsets, int n_groups, int gallery_offset, int merge, int32_t* idx, float* score, int slices,
                             int slice_rows, unsigned long long* keys, hipStream_t s);
// jg_sim_coupling (late interaction): query q = word rows w_offsets[q] .. w_offsets[q + 1] - 1 (1 .. COUPLING_MAX_W of them), a group scores
// as the mean over the query's words of each word's best row in the group, per query the k best groups (retrieval.hip).
constexpr int COUPLING_MAX_W = 64;           // word rows of one query: a query lives in one 64-row tile
struct CouplingPlan {
    int n_tiles;                             // query tiles: whole queries in order, at most 64 word rows each
    SimSearchPlan cut;                       // sim_search_plan's rule with the query tiles in place of the query blocks
};
// The plan of a call, a pure host function (jg_debug_coupling_plan shows it).  Queries are packed in order into tiles of at most 64 word
// rows; a query is never split, one that does not fit the rest of a tile starts the next.  tile_first_query (n_queries + 1 entries of
// room): [i] = the first query of tile i, [n_tiles] = n_queries.  false: offsets or counts the entry refuses.
inline bool sim_coupling_plan(const int32_t* w_offsets, int n_queries, int n_gallery, int k, int num_cu, int slices_in, int32_t* tile_first_query,
                              CouplingPlan& p) {
    if (!w_offsets || !tile_first_query || n_queries < 0 || n_gallery < 0 || k < 1 || k > SIM_TOPK_MAX_K || num_cu < 1 || slices_in < 0 ||
        slices_in > SIM_SEARCH_MAX_SLICES || w_offsets[0] != 0)
        return false;
    int n_tiles = 0, used = 64;              // word rows in the open tile (64: none is open)
    for (int q = 0; q < n_queries; ++q) {
        const long long W = (long long)w_offsets[q + 1] - w_offsets[q];
        if (W < 1 || W > COUPLING_MAX_W) return false;
        if (used + W > 64) { tile_first_query[n_tiles++] = q; used = 0; }
        used += (int)W;
    }
    tile_first_query[n_tiles] = n_queries;
    p.n_tiles = n_tiles;
    return sim_slice_cut(n_tiles, (long long)n_queries * k * 8, n_gallery, num_cu, slices_in, p.cut);
}
// woff [n_queries + 1] and tfq [n_tiles + 1]: the two tables above on the device.  pair (optional) [n_groups][pair_ld]: only pairs with a
// score are stored (launch_coupling_fill first: NaN everywhere).  keys as for launch_sim_search.
hipError_t launch_coupling_fill(float* pair, long pair_ld, int n_queries, int n_groups, hipStream_t s);
hipError_t launch_sim_coupling(const float* words, const int32_t* woff, const int32_t* tfq, int n_tiles, const void* gallery, bool gallery_f16,
                               int n_queries, int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge,
                               int32_t* idx, float* score, float* pair, long pair_ld, int slices, int slice_rows, unsigned long long* keys,
                               hipStream_t s);
// jg_sim_ordered: launch_sim_coupling's arguments, plan and lists, with the words assigned to rows of the group in word order (retrieval.hip)
hipError_t launch_sim_ordered(const float* words, const int32_t* woff, const int32_t* tfq, int n_tiles, const void* gallery, bool gallery_f16,
                              int n_queries, int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge,
                              int32_t* idx, float* score, float* pair, long pair_ld, int slices, int slice_rows, unsigned long long* keys,
                              hipStream_t s);
// jg_sim_align: per slot of idx [n_queries][k] that names one of this call's groups, the row of every word (frames [n_queries k][frames_ld],
// -1 behind the query's words) and the pair's score, ordered or not; other slots are not written.  woff on the device, frames_ld >= the
// longest query (the entry checks it)
hipError_t launch_sim_align(const float* words, const int32_t* woff, const void* gallery, bool gallery_f16, int n_queries, int n_gallery, int D,
                            const int32_t* g_offsets, int n_groups, int group_offset, const int32_t* idx, int k, int ordered, int32_t* frames,
                            int frames_ld, float* score, hipStream_t s);
// grp / pos [n]: the group that holds row idx[e] - gallery_offset and the row's place inside it; -1 / -1 for idx[e] < 0 or a row in no group
hipError_t launch_group_of_rows(const int32_t* idx, long n, const int32_t* g_offsets, int n_groups, int gallery_offset, int32_t* grp,
                                int32_t* pos, hipStream_t s);
// per clip at most SPOT_MAX_W words and SPOT_MAX_T frames (spot, attention matrices and ASD windows size LDS arrays with them); a clip
// outside them, or with a target outside its words, gets pred = -1, score = NaN
constexpr int SPOT_MAX_W = 1024, SPOT_MAX_T = 8192;
hipError_t launch_spot(const float* g, const float* c, const int32_t* goff, const int32_t* coff, const int32_t* target,
                       int n, int D, float temp, int32_t* pred, float* score, hipStream_t s);
// A (optional; with aoff, int64 element offsets per clip) and / or best_frame / best_score (optional; they need keys: attn_matrix_key_elems(n)
// words of scratch).  A clip outside the limits (1..8192 frames, <= max_frames, 1..1024 words) is left out: its words read -1 / NaN
size_t attn_matrix_key_elems(int n_clips);
hipError_t launch_attn_matrix(const float* g, const float* c, const int32_t* goff, const int32_t* coff, int n, int D, int max_frames,
                              float temp, int normalize, float* A, const int64_t* aoff, unsigned long long* keys,
                              int32_t* best_frame, float* best_score, hipStream_t s);
// The heat map along whole talks (spotting.hip: attn_talk_kernel): track i = frame rows goff[i] .. goff[i + 1] - 1 of g (n_rows rows) and
// word rows coff[i] .. coff[i + 1] - 1 of c (n_words rows), wstart / wend [n_words] the words' inclusive bounds on the track's frame axis.
// band (optional) [n_words][band_pitch], best_* (optional; they need keys: n_words words of scratch) [n_words], frame_* (optional) [n_rows];
// every element of each is written.  A track outside the limits (0..max_frames frames and its words inside the arrays) is UNDECIDED as
// a whole, a block of TALK_FB frames with more than TALK_MAX_BLOCK_W words in reach in all its frames: NaN / -1.
constexpr int TALK_MAX_T = 1 << 20, TALK_MAX_REACH = 1024;
constexpr int TALK_MAX_BLOCK_W = 128;        // words in reach of a block of 128 frames: the in-register form of the attention matrix
hipError_t launch_attn_talk(const float* g, const int32_t* goff, int n_tracks, long n_rows, int max_frames, const float* c,
                            const int32_t* coff, int n_words, const int32_t* wstart, const int32_t* wend, int D, int reach, float temp,
                            int normalize, float* band, int band_pitch, unsigned long long* keys, int32_t* best_frame, float* best_score,
                            int32_t* frame_word, float* frame_prob, hipStream_t s);
hipError_t launch_asd(const float* q, const float* cand, const int32_t* coff, int n, int D, float temp,
                      int32_t* pred2, hipStream_t s);
// Audio-visual offset per clip (sync_offset.hip: sync_offset_kernel): mean cosine of the row pairs (t, t + d) for d = -R .. R -> curve
// (optional, [n][2R + 1]; NaN where fewer than min_overlap pairs exist), offset = first arg-max, conf = max - median.  A clip outside
// the limits (1..SYNC_MAX_T video and audio rows, one shift with enough pairs) gets offset 0, conf NaN, a NaN curve row.  No scratch.
constexpr int SYNC_MAX_R = 64, SYNC_MAX_T = 8192, SYNC_MAX_D = 1024;
hipError_t launch_sync_offset(const float* vid, const int32_t* voff, const float* aud, const int32_t* aoff, int n, int D, int R, int min_overlap,
                              float* curve, int32_t* offset, float* conf, hipStream_t s);
// The same over time (sync_offset.hip: sync_band_kernel + sync_windows_kernel): clip i = video track i against audio track a_of[i] (nullptr: i),
// window j of it = video rows j hop .. min(j hop + win, Tv) - 1 (win == 0: all rows) -> curve (optional) / offset / conf rows woff[i] + j.
// band [n_vid_rows][2R + 1] (required here: the caller's, or scratch of that size) receives every cosine once, NaN where the audio row does
// not exist.  A clip outside the limits (tracks of 1..max_rows rows inside the arrays, a_of inside 0..n_aud-1, 1..max_windows windows) gets
// offset 0, conf NaN and NaN curve rows in all of its windows and none of its band rows is written.
constexpr int SYNCW_MAX_T = 1 << 20, SYNCW_MAX_WINDOWS = 1 << 20;
constexpr int SYNCW_MAX_BAND_LOG2 = 40;      // n_vid_rows and the band's n_vid_rows (2R + 1) entries stay below 2^40
hipError_t launch_sync_offset_windows(const float* vid, const int32_t* voff, int n, long n_vid_rows, int max_rows, const float* aud,
                                      const int32_t* aoff, int n_aud, const int32_t* a_of, int D, int R, int min_overlap, int win, int hop,
                                      const int32_t* woff, int max_windows, float* band, float* curve, int32_t* offset, float* conf,
                                      hipStream_t s);
// GestSync's audio stream (gsa_kernels.hip).  conv1 + BatchNorm + ReLU + max-pool of windows n0 .. n0 + nwin - 1 -> out [nwin][19][24][64]
// (fp16, or fp32 with out32): clip_form 0: src = x (N, 1, 80, 100); 1: src = mel (B, Tm, 80), window n = b * T + t reads mel rows
// clamp(4 (t - 12) + 0..99, 0, valid[b] - 1) (valid: device [B] or nullptr = Tm).  w [64][9] (BatchNorm scale folded), shift [64]: fp32
hipError_t launch_gsa_conv1_pool(const float* src, int clip_form, int n0, int nwin, int T, int Tm, const int* valid, const float* w,
                                 const float* shift, void* out, int out32, hipStream_t s);
// NHWC max-pool, window (2, 3), stride (2, 2): (N, H, W, C) -> (N, (H - 2) / 2 + 1, (W - 3) / 2 + 1, C), fp16 or (f32) fp32 elements; C % 8 == 0
hipError_t launch_maxpool_2x3_s2(const void* in, void* out, int N, int H, int W, int C, int f32, hipStream_t s);
// ASD per time window (asd.hip: asd_windows_kernel): prob / cosv (optional) (n_win_i, P_i) at poff[i], pred [woff[n_scenes]].  A scene
// outside the limits (1..64 candidates, 1..1024 words, 1..max_windows windows, tracks of 1..8192 frames inside 0..n_tracks-1) gets
// pred = -1 and NaN rows in all of its windows.  No scratch.
constexpr int ASDW_MAX_D = 1024;
constexpr int ASDW_MAX_P = 64;               // candidates per scene: one lane each in the softmax
constexpr int ASDW_MAX_WIN = 8192;           // windows per scene, and frames per window
hipError_t launch_asd_windows(const float* g, const int32_t* goff, int n_tracks, const float* c, const int32_t* coff, const int32_t* wstart,
                              const int32_t* wend, const int32_t* trk, const int32_t* soff, int n_scenes, int D, int win, int hop,
                              const int32_t* woff, const int64_t* poff, int max_windows, float temp, float* prob, float* cosv,
                              int32_t* pred, hipStream_t s);
