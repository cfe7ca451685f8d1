// Retrieval kernels (gfx950): rank counting, top-k and grouped top-k on exact-fp32 MFMA -- in one walk or in slices over an fp32 or fp16
// gallery -- and the group of a returned row.
#include "metric_parts.h"

// ---------------------------------------------------------------------------------------------
// Retrieval (evaluate_retrieval.py:38-65).  For each local query row i (global index gi =
// row_offset + i):  d = <e1[i], e2[gi]>,  rank[i] = #{j : <e1[i],e2[j]> > d},
// ties[i] = #{j : <e1[i],e2[j]> == d} (includes j = gi).  The reference's `ind` entries for the row
// are rank .. rank+ties-1.  The N x N similarity matrix is never written to HBM.
//
// v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fmaf chain per element, so an element's value
// depends only on its two vectors -- duplicate gallery rows give bitwise-equal scores, i.e. exact
// ties like the reference.  Block = 4 waves = 64 query rows x 64 gallery rows per tile (each wave a
// 32x32 accumulator), K staged through LDS in 64-wide chunks stored [k][row] so the one-float
// fragment reads (lane -> row l&31, k l>>5) are bank-conflict free.
// The tile is written once (sim_tile) and so is an element's k order: a score has the same bits in jg_sim_rank, jg_sim_topk and
// jg_sim_topk_grouped, whatever tile of whichever call it falls in.

__global__ __launch_bounds__(256) void sim_rank_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                       int n_local, int n_total, int row_offset, int D,
                                                       int32_t* __restrict__ rank, int32_t* __restrict__ ties) {
    __shared__ float sA[64][64];   // [k][query row]
    __shared__ float sB[64][64];   // [k][gallery row]
    __shared__ float sDiag[64];
    __shared__ int sRank[64], sTies[64];

    const int tid = threadIdx.x, lane = tid & 63;
    const int i0 = blockIdx.x * 64;
    if (tid < 64) { sRank[tid] = 0; sTies[tid] = 0; }

    int cnt_gt[16], cnt_eq[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) { cnt_gt[x] = 0; cnt_eq[x] = 0; }

    const int ntiles = (n_total + 63) / 64;
    // tile -1 is the diagonal tile (gallery rows row_offset+i0 ..), then all gallery tiles.
    for (int tile = -1; tile < ntiles; ++tile) {
        const int j0 = tile < 0 ? row_offset + i0 : tile * 64;
        const f32x16 acc = sim_tile(e1, e2, i0, j0, n_local, n_total, D, sA, sB, tid);
        if (tile < 0) {
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int row = sim_tile_row(x, tid);
                if (row == sim_tile_col(tid)) sDiag[row] = acc[x];
            }
            __syncthreads();
        } else {
            const bool jok = j0 + sim_tile_col(tid) < n_total;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const float d = sDiag[sim_tile_row(x, tid)];
                cnt_gt[x] += (jok && acc[x] > d) ? 1 : 0;
                cnt_eq[x] += (jok && acc[x] == d) ? 1 : 0;
            }
        }
    }
    // reduce over the 32 lanes that share a row, then across the two column waves
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        int g = cnt_gt[x], e = cnt_eq[x];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { g += __shfl_xor(g, o, 64); e += __shfl_xor(e, o, 64); }
        if ((lane & 31) == 0) {
            atomicAdd(&sRank[sim_tile_row(x, tid)], g);
            atomicAdd(&sTies[sim_tile_row(x, tid)], e);
        }
    }
    __syncthreads();
    if (tid < 64 && i0 + tid < n_local) {
        rank[i0 + tid] = sRank[tid];
        ties[i0 + tid] = sTies[tid];
    }
}

hipError_t launch_sim_rank(const float* e1, const float* e2, int n_local, int n_total, int row_offset, int D,
                           int32_t* rank, int32_t* ties, hipStream_t s) {
    if (n_local <= 0) return hipSuccess;
    if (D % 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sim_rank_kernel, dim3((n_local + 63) / 64), dim3(256), 0, s, e1, e2, n_local, n_total, row_offset, D, rank, ties);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Top-k retrieval: for each query row the k gallery rows with the largest <q_i, g_j>, best first, without the similarity matrix.
// A candidate is the 64-bit key (order-preserving bits of the score << 32) | ~index:
// keys of distinct gallery rows are distinct and totally ordered (larger score first, then the smaller index), so "the k largest keys of
// a set" does not depend on the order of arrival, nor on how the gallery is cut into calls.  Key 0 = empty slot (no number has it).
//
// Per query row in LDS: LCAP >= k keys sorted descending (sL), the k-th of them as the threshold (sThr), and a queue of this tile's
// survivors (sQ, 64 slots = the tile's 64 columns, so it cannot overflow; it lies over the staging buffers, which are dead between the
// last MFMA of a tile and the staging of the next).  After every tile a wave takes 16 rows and inserts the queued keys of each one by one:
// the list lives in the wave's registers (position = lane, lane + 64), an insertion is one compare and a shift by one lane.
//
// Grouped top-k (GROUPED): the gallery rows are partitioned into contiguous groups (goff[g] .. goff[g + 1] - 1, local rows), a group
// scores as its best row (its champion: the largest key of its rows, so on equal scores the first row), and per query the k best champions
// are kept, each with its row.  What this adds is the invariant AT MOST ONE LIST ENTRY PER GROUP: an insertion first looks for the
// entry of the candidate's group; if that entry beats the candidate the candidate is dropped, else the entry is removed and the candidate
// inserted -- one pass, since the candidate lands at or before the entry it replaces: the positions behind that entry keep their keys.
// Entries only ever move towards the end of the list, and replacing an entry by a larger one can only raise the k-th key, so the
// threshold stays monotone: what is below a threshold that ever held is below the final k-th champion.
//
// Groups are contiguous, so "same group" is a range test on the row half of a key against the candidate's [goff[g], goff[g + 1]); the
// list needs no second array.  The range comes from a wave-uniform binary search over goff when the candidate is broadcast, and is kept
// for the candidates behind it: the queue of a tile holds 64 consecutive rows, mostly of one or two groups.  Entries seeded by merge lie
// outside this call's rows and never match.  goff is a device array that nobody has checked: it is only ever read at 0 .. n_groups
// (the search is bounded by n_groups, not by what it reads) and its values are only compared with row numbers, never used as addresses.
//
// Slices (jg_sim_search): the same walk over a part of the gallery's tiles per workgroup, the sorted lists written out as keys, and a second
// kernel that passes every slice's keys through the same insertion (sim_topk_reduce_kernel).  The k best keys of a set do not depend
// on how the set is cut; grouped, a group's true champion is the best row of the group in its own slice, so it misses that slice's list
// only if k other groups beat it there (the group is not in the result then), and a weaker part of the group that another slice kept is
// replaced by the champion in the reduction, or beaten by the k groups that beat the champion.
using u64 = unsigned long long;
__device__ __forceinline__ unsigned topk_ord(float s) {          // fp32 -> unsigned, order-preserving; -0.0 counts as +0.0
    const unsigned b = __float_as_uint(s);
    return b == 0x80000000u ? 0x80000000u : (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float topk_score(u64 key) {
    const unsigned o = (unsigned)(key >> 32);
    return key ? __uint_as_float((o & 0x80000000u) ? o ^ 0x80000000u : ~o) : -INFINITY;
}
__device__ __forceinline__ int32_t topk_index(u64 key) { return key ? (int32_t)(0xffffffffu - (unsigned)key) : -1; }
__device__ __forceinline__ u64 topk_key(float s, unsigned index) { return ((u64)topk_ord(s) << 32) | (0xffffffffu - index); }
__device__ __forceinline__ u64 topk_readlane(u64 v, int src) {   // src: wave-uniform
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, src), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// the group that holds local row j, and its rows [lo, hi), given goff[0] <= j < goff[n_groups] (else: some group and range)
__device__ __forceinline__ int group_range(const int32_t* __restrict__ goff, int n_groups, int j, int& lo, int& hi) {
    int a = 0, b = n_groups;
    lo = goff[0];
    hi = goff[n_groups];
    while (b - a > 1) {                                          // goff[a] <= j < goff[b]
        const int mid = (a + b) >> 1, v = goff[mid];
        if (v <= j) { a = mid; lo = v; } else { b = mid; hi = v; }
    }
    return a;
}

// the wave's 16 rows: queued keys into the sorted lists (GROUPED: one entry per group), new thresholds, queues emptied
template <int LCAP, bool GROUPED>
__device__ __forceinline__ void topk_flush(u64 (*sL)[LCAP], const u64 (*sQ)[64], int* sCnt, u64* sThr, int k, int wave, int lane,
                                           const int32_t* __restrict__ goff, int n_groups, unsigned gallery_offset) {
    unsigned first = 0u, len = 0u;                               // global rows first .. first + len - 1: the group searched last
    for (int rr = 0; rr < 16; ++rr) {
        const int row = wave * 16 + rr;
        const int n = __builtin_amdgcn_readfirstlane(sCnt[row]);
        if (n == 0) continue;
        const u64 cand = lane < n ? sQ[row][lane] : 0ull;
        u64 e0 = sL[row][lane], e1 = 0ull;
        if constexpr (LCAP == 128) e1 = sL[row][64 + lane];
        u64 kth = sThr[row];
        for (int i = 0; i < n; ++i) {
            const u64 c = topk_readlane(cand, i);
            // an earlier insertion of this tile has raised the threshold past it (GROUPED: below the k-th champion, its group's entry, if
            // any, beats it as well)
            if (c < kth) continue;
            int m = LCAP;                                        // GROUPED: the positions behind m keep their keys
            if constexpr (GROUPED) {
                const unsigned gi = 0xffffffffu - (unsigned)c;
                if (gi - first >= len) {
                    int lo, hi;
                    group_range(goff, n_groups, (int)(gi - gallery_offset), lo, hi);
                    first = gallery_offset + (unsigned)lo;
                    len = (unsigned)hi - (unsigned)lo;
                }
                // m: the position of the group's entry (the first one, should hostile offsets give several), LCAP when it has none
                const unsigned long long hit0 = __ballot(e0 != 0ull && 0xffffffffu - (unsigned)e0 - first < len);
                m = hit0 ? __builtin_ctzll(hit0) : LCAP;
                if constexpr (LCAP == 128) {
                    const unsigned long long hit1 = __ballot(e1 != 0ull && 0xffffffffu - (unsigned)e1 - first < len);
                    if (!hit0 && hit1) m = 64 + __builtin_ctzll(hit1);
                }
                if (m < LCAP && topk_readlane(m < 64 ? e0 : e1, m & 63) > c) continue;   // the group's champion stays
            }
            // up to m: position p keeps its key if that beats c, else it takes c if the key before it beats c, else the key before it
            // (GROUPED: the entry at m is below c, so it is the one that leaves)
            u64 p0 = __shfl_up(e0, 1, 64);
            if (lane == 0) p0 = ~0ull;
            if constexpr (LCAP == 128) {
                u64 p1 = __shfl_up(e1, 1, 64);
                const u64 last0 = topk_readlane(e0, 63);
                if (lane == 0) p1 = last0;
                e1 = ((GROUPED && 64 + lane > m) || e1 > c) ? e1 : (p1 > c ? c : p1);
            }
            e0 = ((GROUPED && lane > m) || e0 > c) ? e0 : (p0 > c ? c : p0);
            kth = topk_readlane(LCAP == 128 && k > 64 ? e1 : e0, (k - 1) & 63);
        }
        sL[row][lane] = e0;
        if constexpr (LCAP == 128) sL[row][64 + lane] = e1;
        if (lane == 0) { sThr[row] = kth; sCnt[row] = 0; }
    }
}

// the wave's 16 rows: the lists start empty, or (merge) from the caller's earlier result: sorted, empty slots (idx < 0) last
template <int LCAP>
__device__ __forceinline__ void topk_seed(u64 (*sL)[LCAP], int* sCnt, u64* sThr, int k, int wave, int lane, int i0, int n_queries, int merge,
                                          const int32_t* idx, const float* score) {
    for (int rr = 0; rr < 16; ++rr) {
        const int row = wave * 16 + rr;
        const long base = (long)(i0 + row) * k;
        u64 kth = 0ull;
#pragma unroll
        for (int p = lane; p < LCAP; p += 64) {
            u64 key = 0ull;
            if (merge && p < k && i0 + row < n_queries) {
                const int32_t j = idx[base + p];
                const float s = score[base + p];
                if (j >= 0 && s == s) key = topk_key(s, (unsigned)j);
            }
            sL[row][p] = key;
            if (p == k - 1) kth = key;
        }
        if (lane == ((k - 1) & 63)) sThr[row] = kth;
        if (lane == 0) sCnt[row] = 0;
    }
}
// ... and the lists to where they go: idx / score, each row as one contiguous run
template <int LCAP>
__device__ __forceinline__ void topk_store(const u64 (*sL)[LCAP], int k, int wave, int lane, int i0, int n_queries, int32_t* __restrict__ idx,
                                           float* __restrict__ score) {
    for (int rr = 0; rr < 16; ++rr) {
        const int row = wave * 16 + rr;
        if (i0 + row >= n_queries) break;
        const long base = (long)(i0 + row) * k;
        for (int p = lane; p < k; p += 64) {
            const u64 key = sL[row][p];
            idx[base + p] = topk_index(key);
            score[base + p] = topk_score(key);
        }
    }
}

// jg_sim_topk (GROUPED = false: goff and n_groups are not looked at), jg_sim_topk_grouped and the first kernel of jg_sim_search.
// GT: the gallery's element type (sim_tile).  Workgroup (x, y) walks the tiles of the gallery rows [y slice_rows, (y + 1) slice_rows) for
// the query rows 64 x ..; slice_rows is a multiple of 64, and one slice over all rows (gridDim.y == 1) is the walk of the two plain entries.
// keys == nullptr: the lists go to idx / score.  keys != nullptr (jg_sim_search with more than one slice; merge == 0): the sorted keys
// themselves go to keys[y][query row][0 .. k - 1], every slot written, 0 = empty, and idx / score are not touched.
template <class GT, int LCAP, bool GROUPED>
__global__ __launch_bounds__(256) void sim_topk_kernel(const float* __restrict__ e1, const GT* __restrict__ e2, int n_queries,
                                                       int n_gallery, int D, int k, const int32_t* __restrict__ goff, int n_groups,
                                                       int gallery_offset, int merge, int32_t* __restrict__ idx,
                                                       float* __restrict__ score, int slice_rows, u64* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) u64 sStage[64 * 64];       // staging (sA, sB) during a tile's k loop, the queues after it
    __shared__ u64 sL[64][LCAP];
    __shared__ u64 sThr[64];
    __shared__ int sCnt[64];
    float (*sA)[64] = reinterpret_cast<float (*)[64]>(sStage);         // [k][query row]
    float (*sB)[64] = sA + 64;                                         // [k][gallery row]
    u64 (*sQ)[64] = reinterpret_cast<u64 (*)[64]>(sStage);             // [query row][slot]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * 64;

    topk_seed<LCAP>(sL, sCnt, sThr, k, wave, lane, i0, n_queries, merge, idx, score);

    int grp_lo = 0, grp_hi = 0, ntiles = (n_gallery + 63) / 64;
    if constexpr (GROUPED) {
        // rows below goff[0] or from goff[n_groups] on belong to no group; without a group there is no candidate and no tile to walk
        grp_lo = n_groups > 0 ? goff[0] : 0;
        grp_hi = n_groups > 0 ? goff[n_groups] : 0;
        if (n_groups <= 0) ntiles = 0;
    }
    const int slice_tiles = slice_rows >> 6, tile0 = blockIdx.y * slice_tiles;
    if (ntiles - tile0 > slice_tiles) ntiles = tile0 + slice_tiles;
    for (int tile = tile0; tile < ntiles; ++tile) {
        const int j0 = tile * 64;
        const f32x16 acc = sim_tile(e1, e2, i0, j0, n_queries, n_gallery, D, sA, sB, tid);
        __syncthreads();                                         // the staging buffers become the queues
        const int j = j0 + sim_tile_col(tid);
        const bool jok = j < n_gallery && (!GROUPED || (j >= grp_lo && j < grp_hi));
        const unsigned gj = (unsigned)gallery_offset + (unsigned)j;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int row = sim_tile_row(x, tid);
            const u64 key = topk_key(acc[x], gj);
            if (jok && acc[x] == acc[x] && i0 + row < n_queries && key > sThr[row])      // a NaN is never a candidate
                sQ[row][atomicAdd(&sCnt[row], 1)] = key;
        }
        __syncthreads();
        topk_flush<LCAP, GROUPED>(sL, sQ, sCnt, sThr, k, wave, lane, goff, n_groups, (unsigned)gallery_offset);
    }
    // a wave stores the lists of the rows it seeded and flushed itself
    if (keys) {
        for (int rr = 0; rr < 16; ++rr) {
            const int row = wave * 16 + rr;
            if (i0 + row >= n_queries) break;
            const long base = ((long)blockIdx.y * n_queries + i0 + row) * k;
            for (int p = lane; p < k; p += 64) keys[base + p] = sL[row][p];
        }
    } else {
        topk_store<LCAP>(sL, k, wave, lane, i0, n_queries, idx, score);
    }
}

// The second kernel of jg_sim_search: the per-slice lists keys[n_slices][n_queries][k] (sim_topk_kernel) -> idx / score.  Organised as
// sim_topk_kernel's flush: a wave owns 16 query rows, seeds their lists as that kernel does (merge), streams the rows' n_slices k keys
// through topk_flush 64 at a time -- the queue's size; flat position e of a row is key e % k of slice e / k -- and stores the lists.  A key
// of a slice's list is a candidate like a tile's: GROUPED, the champion of a group that several slices hold a part of replaces the parts
// wherever they meet.  A wave touches the LDS rows of its own 16 query rows only: no barrier.  The next 64 keys are on their way while
// the current ones are inserted.
template <int LCAP, bool GROUPED>
__global__ __launch_bounds__(256) void sim_topk_reduce_kernel(const u64* __restrict__ keys, int n_slices, int n_queries, int k,
                                                              const int32_t* __restrict__ goff, int n_groups, int gallery_offset, int merge,
                                                              int32_t* __restrict__ idx, float* __restrict__ score) {
    __shared__ u64 sQ[64][64];
    __shared__ u64 sL[64][LCAP];
    __shared__ u64 sThr[64];
    __shared__ int sCnt[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * 64;
    topk_seed<LCAP>(sL, sCnt, sThr, k, wave, lane, i0, n_queries, merge, idx, score);

    const int per_row = n_slices * k;                                    // (at most 65535 slices of 128 keys: the launcher's limits)
    const long slice_pitch = (long)n_queries * k;
    auto fetch = [&](int e0, u64 (&v)[16]) {
        const int e = e0 + lane;
        const long at = e < per_row ? (e / k) * slice_pitch + e % k : -1;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int q = i0 + wave * 16 + rr;
            v[rr] = at >= 0 && q < n_queries ? keys[at + (long)q * k] : 0ull;
        }
    };
    u64 cur[16], nxt[16];
    fetch(0, nxt);
    for (int e0 = 0; e0 < per_row; e0 += 64) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) cur[rr] = nxt[rr];
        if (e0 + 64 < per_row) fetch(e0 + 64, nxt);
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int row = wave * 16 + rr;
            const bool in = cur[rr] > sThr[row];                         // (0, the empty slot, beats no threshold)
            const unsigned long long live = __ballot(in);
            if (in) sQ[row][__popcll(live & ((1ull << lane) - 1ull))] = cur[rr];
            if (lane == 0) sCnt[row] = __popcll(live);
        }
        topk_flush<LCAP, GROUPED>(sL, sQ, sCnt, sThr, k, wave, lane, goff, n_groups, (unsigned)gallery_offset);
    }
    topk_store<LCAP>(sL, k, wave, lane, i0, n_queries, idx, score);
}

template <class GT, bool GROUPED>
static hipError_t launch_topk(const float* queries, const GT* gallery, int n_queries, int n_gallery, int D, int k, const int32_t* g_offsets,
                              int n_groups, int gallery_offset, int merge, int32_t* idx, float* score, int slices, int slice_rows,
                              unsigned long long* keys, hipStream_t s) {
    if (n_queries <= 0) return hipSuccess;
    if (D <= 0 || D % 64 || k < 1 || k > SIM_TOPK_MAX_K || n_gallery < 0 || (GROUPED && (n_groups < 0 || (n_groups > 0 && !g_offsets))) ||
        gallery_offset < 0 || gallery_offset > INT32_MAX - n_gallery || slices < 1 || slices > 65535 || slice_rows < 64 || slice_rows % 64 ||
        (slices > 1 && (!keys || (long)(slices - 1) * slice_rows >= n_gallery)))
        return hipErrorInvalidValue;
    const char* const gt = sizeof(GT) == 2 ? "_Float16" : "float";
    const int L = k <= 64 ? 64 : 128, qblocks = (n_queries + 63) / 64;
    const auto kernel = k <= 64 ? sim_topk_kernel<GT, 64, GROUPED> : sim_topk_kernel<GT, 128, GROUPED>;
    if (slices == 1) {                               // one slice: its list is the result
        record_kernel("sim_topk_kernel<%s,%d,%d>", gt, L, (int)GROUPED);
        hipLaunchKernelGGL(kernel, dim3(qblocks), dim3(256), 0, s, queries, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups,
                           gallery_offset, merge, idx, score, slice_rows, (u64*)nullptr);
        return hipGetLastError();
    }
    // two launches on one stream: the kernel boundary is what makes the slices' lists visible to the reduction
    record_kernel("sim_topk_kernel<%s,%d,%d>+sim_topk_reduce_kernel<%d,%d>", gt, L, (int)GROUPED, L, (int)GROUPED);
    hipLaunchKernelGGL(kernel, dim3(qblocks, slices), dim3(256), 0, s, queries, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups,
                       gallery_offset, 0, idx, score, slice_rows, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const auto reduce = k <= 64 ? sim_topk_reduce_kernel<64, GROUPED> : sim_topk_reduce_kernel<128, GROUPED>;
    hipLaunchKernelGGL(reduce, dim3(qblocks), dim3(256), 0, s, keys, slices, n_queries, k, g_offsets, n_groups, gallery_offset, merge, idx, score);
    return hipGetLastError();
}
constexpr int ONE_SLICE = INT32_MAX & ~63;           // slice_rows of a walk over the whole gallery

hipError_t launch_sim_topk(const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k, int gallery_offset,
                           int merge, int32_t* idx, float* score, hipStream_t s) {
    return launch_topk<float, false>(queries, gallery, n_queries, n_gallery, D, k, nullptr, 0, gallery_offset, merge, idx, score, 1, ONE_SLICE,
                                     nullptr, s);
}

hipError_t launch_sim_topk_grouped(const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k,
                                   const int32_t* g_offsets, int n_groups, int gallery_offset, int merge, int32_t* idx, float* score,
                                   hipStream_t s) {
    return launch_topk<float, true>(queries, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups, gallery_offset, merge, idx, score, 1,
                                    ONE_SLICE, nullptr, s);
}

hipError_t launch_sim_search(const float* queries, const void* gallery, bool gallery_f16, int n_queries, int n_gallery, int D, int k,
                             const int32_t* g_offsets, int n_groups, int gallery_offset, int merge, int32_t* idx, float* score, int slices,
                             int slice_rows, unsigned long long* keys, hipStream_t s) {
    const float* const g32 = static_cast<const float*>(gallery);
    const _Float16* const g16 = static_cast<const _Float16*>(gallery);
#define SEARCH(GT, G, GROUPED) launch_topk<GT, GROUPED>(queries, G, n_queries, n_gallery, D, k, g_offsets, n_groups, gallery_offset, merge, idx, \
                                                        score, slices, slice_rows, keys, s)
    if (g_offsets) return gallery_f16 ? SEARCH(_Float16, g16, true) : SEARCH(float, g32, true);
    return gallery_f16 ? SEARCH(_Float16, g16, false) : SEARCH(float, g32, false);
#undef SEARCH
}

// ---------------------------------------------------------------------------------------------
// Coupling (late interaction, jg_sim_coupling): query q = word rows woff[q] .. woff[q + 1] - 1, group g = gallery rows goff[g] ..
// goff[g + 1] - 1; m(w, g) = the largest non-NaN <word w, row t> over the group's rows (-0.0 as +0.0), score(q, g) = (the m(w, g) added in
// word order, one fp32 chain) / W_q, and per query the k best groups.  A pair with a word that has no m has no score.  The max is exact and
// the chain's order is fixed, so a score depends on the rows of its query and its group alone, not on tiles, slices or the rest of the call.
//
// Workgroup (x, y): query tile x (tfq[x] .. tfq[x + 1] - 1: whole queries, at most 64 word rows together -- sim_coupling_plan) and the
// groups whose first row lies in slice y = [y slice_rows, (y + 1) slice_rows).  It walks the 64-row-aligned gallery tiles that hold a column
// of such a group, on past the slice's end until the last of them ends: a group is never split between workgroups, and the tiles are the
// same for every cut.  Inside a tile a group's columns are one segment [b, e): every thread masks its column, 5 shuffle / max steps leave a
// row's max over a wave's 32 columns in the row's first lane, the two column waves meet in sPart, and sRun keeps the max per word row while
// the group goes on into the next tile.  NaN stands for "none" throughout: fmaxf returns the other operand.  When a group ends, thread
// i < (queries of the tile) adds the maxima of query i's rows, divides, stores the pair and queues the key for topk_flush with "row" =
// query of the tile.  The segments of a tile are disjoint (`pos`: the first column not yet consumed, whatever the offsets hold) and only a
// group with a column queues a key, so at most 64 keys per query and tile: the queue cannot overflow.
// goff is only read at 0 .. n_groups and only compared with row numbers; hostile offsets give some result and nothing else.
__global__ void coupling_fill_kernel(float* __restrict__ pair, long pair_ld, int n_queries, int n_groups) {
    const long n = (long)n_queries * n_groups;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
        pair[(e / n_queries) * pair_ld + e % n_queries] = __uint_as_float(0x7fc00000u);
}

template <class GT, int LCAP>
__global__ __launch_bounds__(256) void sim_coupling_kernel(const float* __restrict__ words, const int32_t* __restrict__ woff,
                                                           const int32_t* __restrict__ tfq, const GT* __restrict__ gallery, int n_queries,
                                                           int n_gallery, int D, int k, const int32_t* __restrict__ goff, int n_groups,
                                                           int group_offset, int merge, int32_t* __restrict__ idx, float* __restrict__ score,
                                                           float* __restrict__ pair, long pair_ld, int slice_rows, u64* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) u64 sStage[64 * 64];       // staging (sA, sB) during a tile's k loop, the queues after it
    __shared__ u64 sL[64][LCAP];
    __shared__ u64 sThr[64];
    __shared__ int sCnt[64];
    __shared__ float sPart[2][64];                                     // a segment's max per word row, of either column wave
    __shared__ float sRun[64];                                         // the open group's max per word row so far
    __shared__ int sW[65];                                             // the tile's queries as word rows of the tile
    float (*sA)[64] = reinterpret_cast<float (*)[64]>(sStage);
    float (*sB)[64] = sA + 64;
    u64 (*sQ)[64] = reinterpret_cast<u64 (*)[64]>(sStage);             // [query of the tile][slot]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = tfq[blockIdx.x], q1 = tfq[blockIdx.x + 1], nq = q1 - q0;
    const int row0 = woff[q0], row1 = woff[q1];
    if (tid <= nq) sW[tid] = woff[q0 + tid] - row0;
    topk_seed<LCAP>(sL, sCnt, sThr, k, wave, lane, q0, q1, merge, idx, score);

    // the first group this slice owns (g, rows [lo, hi)); n_groups: none
    const long lim_lo = (long)blockIdx.y * slice_rows, lim_hi = lim_lo + slice_rows;
    int g = n_groups, lo = 0, hi = 0;
    if (n_groups > 0 && lim_lo < n_gallery) {
        if (lim_lo <= goff[0]) {
            g = 0; lo = goff[0]; hi = goff[1];
        } else if (lim_lo < goff[n_groups]) {
            g = group_range(goff, n_groups, (int)lim_lo, lo, hi);
            if (lo != lim_lo) { ++g; lo = hi; hi = g < n_groups ? goff[g + 1] : lo; }      // it began before the slice: another's
        }
    }
    auto next_group = [&] { ++g; lo = hi; if (g < n_groups) hi = goff[g + 1]; };
    auto flush = [&] {
        __syncthreads();
        topk_flush<LCAP, false>(sL, sQ, sCnt, sThr, k, wave, lane, nullptr, 0, 0u);
    };

    int pos = (int)(lim_lo < n_gallery ? lim_lo : n_gallery);      // columns below it are consumed (or another slice's)
    int j0 = -64;                                                    // the tile in acc: none yet
    bool queued = false;                                             // a group has ended in this tile
    f32x16 acc;
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[x] = 0.f;
    __syncthreads();                                                 // sW and the seeded lists
    for (;;) {
        // the next owned group with a column; a group without one has no score
        while (g < n_groups && lo < lim_hi && (hi < n_gallery ? hi : n_gallery) <= (lo > pos ? lo : pos)) next_group();
        if (g >= n_groups || lo >= lim_hi) break;
        int b = lo > pos ? lo : pos;
        const int e = hi < n_gallery ? hi : n_gallery;               // its columns [b, e), b < e
        bool first = true;
        for (;;) {                                                   // its segments, one per tile
            if (b >= (long)j0 + 64) {
                if (queued) { flush(); queued = false; }
                j0 = b & ~63;
                acc = sim_tile(words, gallery, row0, j0, row1, n_gallery, D, sA, sB, tid);
            }
            const int se = e < (long)j0 + 64 ? e : j0 + 64;                  // (long: the last tile of 2^31 - 1 rows ends past INT32_MAX)
            const long col = (long)j0 + sim_tile_col(tid);
            const bool in = col >= b && col < se;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                float v = in ? (acc[x] == 0.f ? 0.f : acc[x]) : __uint_as_float(0x7fc00000u);
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
                if ((lane & 31) == 0) sPart[wave >> 1][sim_tile_row(x, tid)] = v;
            }
            __syncthreads();
            if (tid < 64) {
                const float m = fmaxf(sPart[0][tid], sPart[1][tid]);
                sRun[tid] = first ? m : fmaxf(sRun[tid], m);
            }
            first = false;
            b = se;
            if (b >= e) break;
        }
        // the group has ended: query i of the tile, by thread i
        __syncthreads();
        if (tid < nq) {
            const int w0 = sW[tid], w1 = sW[tid + 1];
            float sum = 0.f;
            bool all = true;
            for (int r = w0; r < w1; ++r) {
                const float m = sRun[r];
                all = all && m == m;
                sum += m;
            }
            const float sc = __fdiv_rn(sum, (float)(w1 - w0));
            if (all) {
                if (pair) pair[(long)g * pair_ld + q0 + tid] = sc;
                const u64 key = topk_key(sc, (unsigned)group_offset + (unsigned)g);
                if (sc == sc && key > sThr[tid]) sQ[tid][sCnt[tid]++] = key;
            }
        }
        queued = true;
        pos = e;
        next_group();
    }
    if (queued) flush();
    // a wave stores the lists of the queries it seeded and flushed itself
    if (keys) {
        for (int rr = 0; rr < 16; ++rr) {
            const int row = wave * 16 + rr;
            if (row >= nq) break;
            const long base = ((long)blockIdx.y * n_queries + q0 + row) * k;
            for (int p = lane; p < k; p += 64) keys[base + p] = sL[row][p];
        }
    } else {
        topk_store<LCAP>(sL, k, wave, lane, q0, q1, idx, score);
    }
}

hipError_t launch_coupling_fill(float* pair, long pair_ld, int n_queries, int n_groups, hipStream_t s) {
    const long n = (long)n_queries * n_groups;
    if (n <= 0) return hipSuccess;
    if (!pair || pair_ld < n_queries) return hipErrorInvalidValue;
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(coupling_fill_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, pair, pair_ld, n_queries, n_groups);
    return hipGetLastError();
}

template <class GT>
static hipError_t launch_coupling(const float* words, const int32_t* woff, const int32_t* tfq, int n_tiles, const GT* gallery, int n_queries,
                                  int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge, int32_t* idx,
                                  float* score, float* pair, long pair_ld, int slices, int slice_rows, u64* keys, hipStream_t s) {
    const char* const gt = sizeof(GT) == 2 ? "_Float16" : "float";
    const int L = k <= 64 ? 64 : 128;
    const auto kernel = k <= 64 ? sim_coupling_kernel<GT, 64> : sim_coupling_kernel<GT, 128>;
    if (slices == 1) {
        record_kernel("sim_coupling_kernel<%s,%d>", gt, L);
        hipLaunchKernelGGL(kernel, dim3(n_tiles), dim3(256), 0, s, words, woff, tfq, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups,
                           group_offset, merge, idx, score, pair, pair_ld, slice_rows, (u64*)nullptr);
        return hipGetLastError();
    }
    record_kernel("sim_coupling_kernel<%s,%d>+sim_topk_reduce_kernel<%d,0>", gt, L, L);
    hipLaunchKernelGGL(kernel, dim3(n_tiles, slices), dim3(256), 0, s, words, woff, tfq, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups,
                       group_offset, 0, idx, score, pair, pair_ld, slice_rows, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const auto reduce = k <= 64 ? sim_topk_reduce_kernel<64, false> : sim_topk_reduce_kernel<128, false>;
    hipLaunchKernelGGL(reduce, dim3((n_queries + 63) / 64), dim3(256), 0, s, keys, slices, n_queries, k, (const int32_t*)nullptr, 0, group_offset,
                       merge, idx, score);
    return hipGetLastError();
}

hipError_t launch_sim_coupling(const float* words, const int32_t* woff, const int32_t* tfq, int n_tiles, const void* gallery, bool gallery_f16,
                               int n_queries, int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge,
                               int32_t* idx, float* score, float* pair, long pair_ld, int slices, int slice_rows, unsigned long long* keys,
                               hipStream_t s) {
    if (n_queries <= 0) return hipSuccess;
    if (!words || !woff || !tfq || n_tiles < 1 || n_tiles > n_queries || D <= 0 || D % 64 || k < 1 || k > SIM_TOPK_MAX_K || n_gallery < 0 ||
        n_groups < 0 || (n_groups > 0 && !g_offsets) || group_offset < 0 || group_offset > INT32_MAX - n_groups || (pair && pair_ld < n_queries) ||
        slices < 1 || slices > 65535 || slice_rows < 64 || slice_rows % 64 || (slices > 1 && (!keys || (long)(slices - 1) * slice_rows >= n_gallery)))
        return hipErrorInvalidValue;
    return gallery_f16 ? launch_coupling(words, woff, tfq, n_tiles, static_cast<const _Float16*>(gallery), n_queries, n_gallery, D, k, g_offsets,
                                         n_groups, group_offset, merge, idx, score, pair, pair_ld, slices, slice_rows, keys, s)
                       : launch_coupling(words, woff, tfq, n_tiles, static_cast<const float*>(gallery), n_queries, n_gallery, D, k, g_offsets,
                                         n_groups, group_offset, merge, idx, score, pair, pair_ld, slices, slice_rows, keys, s);
}

// ---------------------------------------------------------------------------------------------
// Ordered coupling (jg_sim_ordered): the queries, groups, tiles, slices and lists of jg_sim_coupling, with the words of a query assigned to
// frames of the group in word order.  With t counted from the group's first row and s(w, t) as above (-0.0 as +0.0):
//   M_0(t) = +0.0;  E_i(t) = M_{i-1}(t) + s(w_i, t) (one fp32 add, NaN if either is);  M_i(t) = the max of the non-NaN E_i(t'), t' <= t
// (NaN: none), and score(q, g) = M_W(T - 1) / W: the best mean of s(w_i, t_i) over t_1 <= t_2 <= .. <= t_W, the sum one fp32 chain in word
// order.  Nothing in it depends on where a tile or a slice ends, so the bits do not either.
//
// The walk is sim_coupling_kernel's, unchanged.  What differs is a segment (the columns [b, e) of a group inside a tile): the tile's scores
// go to LDS as sS[word row][column] once per tile, and every query of the tile is taken by one wave (query i by wave i & 3), lane = column.
// The wave runs down the query's word rows: one LDS value, one add, an inclusive fmax prefix scan over the 64 lanes with the lanes outside
// the segment as NaN (fmaxf returns the other operand), and an fmax with the word's carry sCarry[row] = M_i at the last column of the
// tiles before -- M_i is non-decreasing in t, so that one value stands for all of them.  Lane 63 of the result is the new carry.  A query's
// rows are touched by its own wave only; the barrier in front of a segment orders them against the tile's stores and against the threads
// that read the last carries when the group before ended.  NaN propagates by itself: a word without a value leaves M_i NaN everywhere, so
// every later E is NaN and so is M_W: the pair has no score.
__device__ __forceinline__ float wave_fmax_scan(float v, int lane) {     // inclusive, over the lanes 0 .. lane; NaN = none
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o, 64);
        if (lane >= o) v = fmaxf(v, u);
    }
    return v;
}
// the tile in acc -> sS[word row][column], -0.0 as +0.0
__device__ __forceinline__ void sim_tile_store(const f32x16& acc, float (*sS)[64], int tid) {
    const int col = sim_tile_col(tid);
#pragma unroll
    for (int x = 0; x < 16; ++x) sS[sim_tile_row(x, tid)][col] = acc[x] == 0.f ? 0.f : acc[x];
}

template <class GT, int LCAP>
__global__ __launch_bounds__(256) void sim_ordered_kernel(const float* __restrict__ words, const int32_t* __restrict__ woff,
                                                          const int32_t* __restrict__ tfq, const GT* __restrict__ gallery, int n_queries,
                                                          int n_gallery, int D, int k, const int32_t* __restrict__ goff, int n_groups,
                                                          int group_offset, int merge, int32_t* __restrict__ idx, float* __restrict__ score,
                                                          float* __restrict__ pair, long pair_ld, int slice_rows, u64* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) u64 sStage[64 * 64];       // staging (sA, sB) during a tile's k loop, the queues after it
    __shared__ u64 sL[64][LCAP];
    __shared__ u64 sThr[64];
    __shared__ int sCnt[64];
    __shared__ float sS[64][64];                                       // the tile's scores, [word row][column]
    __shared__ float sCarry[64];                                       // the open group's M_i at the last column so far, per word row
    __shared__ int sW[65];                                             // the tile's queries as word rows of the tile
    float (*sA)[64] = reinterpret_cast<float (*)[64]>(sStage);
    float (*sB)[64] = sA + 64;
    u64 (*sQ)[64] = reinterpret_cast<u64 (*)[64]>(sStage);             // [query of the tile][slot]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = tfq[blockIdx.x], q1 = tfq[blockIdx.x + 1], nq = q1 - q0;
    const int row0 = woff[q0], row1 = woff[q1];
    if (tid <= nq) sW[tid] = woff[q0 + tid] - row0;
    topk_seed<LCAP>(sL, sCnt, sThr, k, wave, lane, q0, q1, merge, idx, score);

    // the first group this slice owns (g, rows [lo, hi)); n_groups: none
    const long lim_lo = (long)blockIdx.y * slice_rows, lim_hi = lim_lo + slice_rows;
    int g = n_groups, lo = 0, hi = 0;
    if (n_groups > 0 && lim_lo < n_gallery) {
        if (lim_lo <= goff[0]) {
            g = 0; lo = goff[0]; hi = goff[1];
        } else if (lim_lo < goff[n_groups]) {
            g = group_range(goff, n_groups, (int)lim_lo, lo, hi);
            if (lo != lim_lo) { ++g; lo = hi; hi = g < n_groups ? goff[g + 1] : lo; }      // it began before the slice: another's
        }
    }
    auto next_group = [&] { ++g; lo = hi; if (g < n_groups) hi = goff[g + 1]; };
    auto flush = [&] {
        __syncthreads();
        topk_flush<LCAP, false>(sL, sQ, sCnt, sThr, k, wave, lane, nullptr, 0, 0u);
    };

    int pos = (int)(lim_lo < n_gallery ? lim_lo : n_gallery);      // columns below it are consumed (or another slice's)
    int j0 = -64;                                                    // the tile in sS: none yet
    bool queued = false;                                             // a group has ended in this tile
    __syncthreads();                                                 // sW and the seeded lists
    for (;;) {
        // the next owned group with a column; a group without one has no score
        while (g < n_groups && lo < lim_hi && (hi < n_gallery ? hi : n_gallery) <= (lo > pos ? lo : pos)) next_group();
        if (g >= n_groups || lo >= lim_hi) break;
        int b = lo > pos ? lo : pos;
        const int e = hi < n_gallery ? hi : n_gallery;               // its columns [b, e), b < e
        bool first = true;
        for (;;) {                                                   // its segments, one per tile
            if (b >= (long)j0 + 64) {
                if (queued) { flush(); queued = false; }
                j0 = b & ~63;
                // (the barriers inside sim_tile: every wave has finished the segments of the tile before, so sS may be written)
                const f32x16 acc = sim_tile(words, gallery, row0, j0, row1, n_gallery, D, sA, sB, tid);
                sim_tile_store(acc, sS, tid);
            }
            const int se = e < (long)j0 + 64 ? e : j0 + 64;                  // (long: the last tile of 2^31 - 1 rows ends past INT32_MAX)
            const long col = (long)j0 + lane;
            const bool in = col >= b && col < se;
            __syncthreads();                                         // sS is whole, and the carries of the group before have been read
            for (int i = wave; i < nq; i += 4) {
                float m = 0.f;                                       // M_0
                for (int r = sW[i]; r < sW[i + 1]; ++r) {
                    const float ev = in ? m + sS[r][lane] : __uint_as_float(0x7fc00000u);
                    m = wave_fmax_scan(ev, lane);
                    if (!first) m = fmaxf(m, sCarry[r]);
                    if (lane == 63) sCarry[r] = m;
                }
            }
            first = false;
            b = se;
            if (b >= e) break;
        }
        // the group has ended: query i of the tile, by thread i
        __syncthreads();
        if (tid < nq) {
            const int w0 = sW[tid], w1 = sW[tid + 1];
            const float m = sCarry[w1 - 1];                          // M_W(T - 1)
            const float sc = __fdiv_rn(m, (float)(w1 - w0));
            if (m == m) {
                if (pair) pair[(long)g * pair_ld + q0 + tid] = sc;
                const u64 key = topk_key(sc, (unsigned)group_offset + (unsigned)g);
                if (sc == sc && key > sThr[tid]) sQ[tid][sCnt[tid]++] = key;
            }
        }
        queued = true;
        pos = e;
        next_group();
    }
    if (queued) flush();
    // a wave stores the lists of the queries it seeded and flushed itself
    if (keys) {
        for (int rr = 0; rr < 16; ++rr) {
            const int row = wave * 16 + rr;
            if (row >= nq) break;
            const long base = ((long)blockIdx.y * n_queries + q0 + row) * k;
            for (int p = lane; p < k; p += 64) keys[base + p] = sL[row][p];
        }
    } else {
        topk_store<LCAP>(sL, k, wave, lane, q0, q1, idx, score);
    }
}

template <class GT>
static hipError_t launch_ordered(const float* words, const int32_t* woff, const int32_t* tfq, int n_tiles, const GT* gallery, int n_queries,
                                 int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge, int32_t* idx,
                                 float* score, float* pair, long pair_ld, int slices, int slice_rows, u64* keys, hipStream_t s) {
    const char* const gt = sizeof(GT) == 2 ? "_Float16" : "float";
    const int L = k <= 64 ? 64 : 128;
    const auto kernel = k <= 64 ? sim_ordered_kernel<GT, 64> : sim_ordered_kernel<GT, 128>;
    if (slices == 1) {
        record_kernel("sim_ordered_kernel<%s,%d>", gt, L);
        hipLaunchKernelGGL(kernel, dim3(n_tiles), dim3(256), 0, s, words, woff, tfq, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups,
                           group_offset, merge, idx, score, pair, pair_ld, slice_rows, (u64*)nullptr);
        return hipGetLastError();
    }
    record_kernel("sim_ordered_kernel<%s,%d>+sim_topk_reduce_kernel<%d,0>", gt, L, L);
    hipLaunchKernelGGL(kernel, dim3(n_tiles, slices), dim3(256), 0, s, words, woff, tfq, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups,
                       group_offset, 0, idx, score, pair, pair_ld, slice_rows, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const auto reduce = k <= 64 ? sim_topk_reduce_kernel<64, false> : sim_topk_reduce_kernel<128, false>;
    hipLaunchKernelGGL(reduce, dim3((n_queries + 63) / 64), dim3(256), 0, s, keys, slices, n_queries, k, (const int32_t*)nullptr, 0, group_offset,
                       merge, idx, score);
    return hipGetLastError();
}

hipError_t launch_sim_ordered(const float* words, const int32_t* woff, const int32_t* tfq, int n_tiles, const void* gallery, bool gallery_f16,
                              int n_queries, int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge,
                              int32_t* idx, float* score, float* pair, long pair_ld, int slices, int slice_rows, unsigned long long* keys,
                              hipStream_t s) {
    if (n_queries <= 0) return hipSuccess;
    if (!words || !woff || !tfq || n_tiles < 1 || n_tiles > n_queries || D <= 0 || D % 64 || k < 1 || k > SIM_TOPK_MAX_K || n_gallery < 0 ||
        n_groups < 0 || (n_groups > 0 && !g_offsets) || group_offset < 0 || group_offset > INT32_MAX - n_groups || (pair && pair_ld < n_queries) ||
        slices < 1 || slices > 65535 || slice_rows < 64 || slice_rows % 64 || (slices > 1 && (!keys || (long)(slices - 1) * slice_rows >= n_gallery)))
        return hipErrorInvalidValue;
    return gallery_f16 ? launch_ordered(words, woff, tfq, n_tiles, static_cast<const _Float16*>(gallery), n_queries, n_gallery, D, k, g_offsets,
                                        n_groups, group_offset, merge, idx, score, pair, pair_ld, slices, slice_rows, keys, s)
                       : launch_ordered(words, woff, tfq, n_tiles, static_cast<const float*>(gallery), n_queries, n_gallery, D, k, g_offsets,
                                        n_groups, group_offset, merge, idx, score, pair, pair_ld, slices, slice_rows, keys, s);
}

// ---------------------------------------------------------------------------------------------
// Alignment (jg_sim_align): which frame every word of a returned (query, group) pair took.  One workgroup per slot (q, r) of idx; a slot
// whose entry is not one of this call's groups is left alone.  The group's rows [a, b) (goff at the group and the next, clamped to the
// gallery) are walked in 64-row-aligned tiles through sim_tile with the query's word rows alone as the 64-row operand, and wave 0 runs the
// recurrence above per tile -- with M_{i-1} replaced by +0.0 when not ordered, which leaves E_i = s(w_i, .) and M_i the running max
// jg_sim_coupling takes.  Nothing of E is kept but one bit per cell: sBit[word][tile] = the ballot of "this column strictly raised the word's
// running max" (for a first value: "is not NaN").  The first arg-max of E_i over [0, c] is then the last set bit at or below c, so one wave
// backtracks from word W down to 1: ordered, the limit c of a word is the frame of the word after it; unordered, it is T - 1 for every
// word.  The score is M_W(T - 1) / W (ordered), or the M_i(T - 1) added in word order / W (unordered): the bits of the two scans.
constexpr int ALIGN_MAX_T = SPOT_MAX_T;                                // rows of a group that is aligned
constexpr int ALIGN_TILES = ALIGN_MAX_T / 64 + 1;                      // ... which lie in at most this many 64-row-aligned tiles

template <class GT>
__global__ __launch_bounds__(256) void sim_align_kernel(const float* __restrict__ words, const int32_t* __restrict__ woff,
                                                        const GT* __restrict__ gallery, int n_gallery, int D,
                                                        const int32_t* __restrict__ goff, int n_groups, int group_offset,
                                                        const int32_t* __restrict__ idx, int k, int ordered, int32_t* __restrict__ frames,
                                                        int frames_ld, float* __restrict__ score) {
    __shared__ __attribute__((aligned(16))) float sA[64][64];          // [k][word row]
    __shared__ __attribute__((aligned(16))) float sB[64][64];          // [k][gallery row]
    __shared__ float sS[64][64];                                       // the tile's scores, [word row][column]
    __shared__ u64 sBit[64][ALIGN_TILES];                              // [word row][tile]: the columns that raised the word's running max
    __shared__ float sCarry[64];                                       // M_i at the last column so far

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long slot = blockIdx.x;                                      // q k + r
    const int q = (int)(slot / k);
    const int32_t entry = idx[slot];
    const long gl = (long)entry - group_offset;
    if (entry < 0 || gl < 0 || gl >= n_groups) return;                 // -1, or another piece's group: not this call's slot
    const int g = (int)gl;
    const int w0 = woff[q], W = woff[q + 1] - w0;
    const int lo = goff[g], hi = goff[g + 1];
    const int a = lo > 0 ? lo : 0, b = hi < n_gallery ? hi : n_gallery;
    int32_t* const fr = frames + slot * frames_ld;
    const bool none = b <= a || (long)b - a > ALIGN_MAX_T;             // no row, or more rows than are aligned
    const int base = a & ~63;                                          // column c = gallery row base + c
    const int ntiles = none ? 0 : (int)(((long)b - base + 63) >> 6);

    if (tid < 64) sCarry[tid] = __uint_as_float(0x7fc00000u);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int j0 = base + tile * 64;
        const f32x16 acc = sim_tile(words, gallery, w0, j0, w0 + W, n_gallery, D, sA, sB, tid);
        sim_tile_store(acc, sS, tid);
        __syncthreads();
        if (wave == 0) {
            const long col = (long)j0 + lane;
            const bool in = col >= a && col < b;
            float m = 0.f;
            for (int i = 0; i < W; ++i) {
                const float ev = in ? (ordered ? m : 0.f) + sS[i][lane] : __uint_as_float(0x7fc00000u);
                const float incl = wave_fmax_scan(ev, lane);
                float before = __shfl_up(incl, 1, 64);               // the running max in front of this column
                const float carry = sCarry[i];
                before = lane == 0 ? carry : fmaxf(before, carry);
                const u64 raised = __ballot(ev == ev && !(ev <= before));
                m = fmaxf(incl, carry);
                if (lane == 63) sCarry[i] = m;
                if (lane == 0) sBit[i][tile] = raised;
            }
        }
        // (the next tile's sim_tile begins with a barrier: wave 0 has read sS before it is written again)
    }
    __syncthreads();
    if (wave != 0) return;
    // the score, the same in every lane
    float sum = 0.f;
    bool all = !none;
    if (ordered) {
        sum = sCarry[W - 1];
        all = all && sum == sum;
    } else {
        for (int i = 0; i < W; ++i) {
            const float m = sCarry[i];
            all = all && m == m;
            sum += m;
        }
    }
    // the backtrack: word i's frame = the last set bit of its row at or below `limit`
    int mine = -1;                                                     // lane i keeps the frame of word i
    int limit = all ? (int)((long)b - 1 - base) : -1;
    for (int i = W - 1; i >= 0 && all; --i) {
        int found = -1;
        const int lt = limit >> 6;
        for (int t0 = (lt >> 6) << 6; t0 >= 0 && found < 0; t0 -= 64) {
            const int t = t0 + lane;
            u64 bitsv = 0ull;
            if (t <= lt) {
                bitsv = sBit[i][t];
                if (t == lt) bitsv &= ~0ull >> (63 - (limit & 63));
            }
            const u64 any = __ballot(bitsv != 0ull);
            if (any) {
                const int src = 63 - __builtin_clzll(any);
                const u64 top = topk_readlane(bitsv, src);
                found = (t0 + src) * 64 + 63 - __builtin_clzll(top);
            }
        }
        if (found < 0) { all = false; break; }                         // (cannot be: a non-NaN M_i has a column that raised it)
        if (lane == i) mine = base + found;
        if (ordered) limit = found;
    }
    for (int i = lane; i < frames_ld; i += 64) fr[i] = all && i < W ? mine : -1;      // (W <= 64: word i is lane i's)
    if (lane == 0) score[slot] = all ? __fdiv_rn(sum, (float)W) : __uint_as_float(0x7fc00000u);
}

hipError_t launch_sim_align(const float* words, const int32_t* woff, const void* gallery, bool gallery_f16, int n_queries, int n_gallery, int D,
                            const int32_t* g_offsets, int n_groups, int group_offset, const int32_t* idx, int k, int ordered, int32_t* frames,
                            int frames_ld, float* score, hipStream_t s) {
    if (n_queries <= 0) return hipSuccess;
    if (!words || !woff || !gallery || !idx || !frames || !score || D <= 0 || D % 64 || k < 1 || k > SIM_TOPK_MAX_K || n_gallery < 0 ||
        n_groups < 0 || (n_groups > 0 && !g_offsets) || group_offset < 0 || group_offset > INT32_MAX - n_groups || frames_ld < 1 ||
        (long)n_queries * k > INT32_MAX)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((long)n_queries * k));
    if (gallery_f16) {
        record_kernel("sim_align_kernel<_Float16>");
        hipLaunchKernelGGL(sim_align_kernel<_Float16>, grid, dim3(256), 0, s, words, woff, static_cast<const _Float16*>(gallery), n_gallery, D,
                           g_offsets, n_groups, group_offset, idx, k, ordered, frames, frames_ld, score);
    } else {
        record_kernel("sim_align_kernel<float>");
        hipLaunchKernelGGL(sim_align_kernel<float>, grid, dim3(256), 0, s, words, woff, static_cast<const float*>(gallery), n_gallery, D,
                           g_offsets, n_groups, group_offset, idx, k, ordered, frames, frames_ld, score);
    }
    return hipGetLastError();
}

// rows (as jg_sim_topk_grouped returns them) -> group and position inside it: an element-wise binary search; -1 / -1 for idx < 0 or a row
// in no group.  Hostile offsets give some group and position, nothing else.
__global__ void group_of_rows_kernel(const int32_t* __restrict__ idx, long n, const int32_t* __restrict__ goff, int n_groups,
                                     int gallery_offset, int32_t* __restrict__ grp, int32_t* __restrict__ pos) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const long j = (long)idx[e] - gallery_offset;
        int g = -1, p = -1;
        if (idx[e] >= 0 && n_groups > 0 && j >= goff[0] && j < goff[n_groups]) {
            int lo, hi;
            g = group_range(goff, n_groups, (int)j, lo, hi);
            p = (int)(j - goff[g]);
        }
        grp[e] = g;
        pos[e] = p;
    }
}

hipError_t launch_group_of_rows(const int32_t* idx, long n, const int32_t* g_offsets, int n_groups, int gallery_offset, int32_t* grp,
                                int32_t* pos, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n_groups < 0 || (n_groups > 0 && !g_offsets)) return hipErrorInvalidValue;
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(group_of_rows_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, idx, n, g_offsets, n_groups,
                       gallery_offset, grp, pos);
    return hipGetLastError();
}
