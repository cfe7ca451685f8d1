// Metric kernels (gfx950): retrieval rank counting and gesture-word attention matrices on exact-fp32 MFMA, word spotting, ASD
// (the grade, and the speaker probabilities per time window).
#include "common.h"

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

// One 64 x 64 tile <e1[i0 ..], e2[j0 ..]> over all of D: the calling wave's 32 x 32 part of it.  sA / sB: [k][query row] / [k][gallery
// row] staging, 64 x 64 floats each; rows from n_rows / n_cols on are zero.  Begins with a barrier, so the buffers may hold anything that
// every wave has finished reading; the last chunk's reads are NOT fenced from what the caller writes there next.
__device__ __forceinline__ f32x16 sim_tile(const float* __restrict__ e1, const float* __restrict__ e2, int i0, int j0, int n_rows, int n_cols,
                                           int D, float (*sA)[64], float (*sB)[64], int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave & 1, wc = wave >> 1;
    const int r = tid & 63, kq = tid >> 6;
    f32x16 acc;
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[x] = 0.f;
    for (int k0 = 0; k0 < D; k0 += 64) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = kq * 16 + q * 4;
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = va;
            if (i0 + r < n_rows) va = *reinterpret_cast<const f32x4*>(e1 + (long)(i0 + r) * D + k0 + k);
            if (j0 + r < n_cols) vb = *reinterpret_cast<const f32x4*>(e2 + (long)(j0 + r) * D + k0 + k);
            sA[k][r] = va.x; sA[k + 1][r] = va.y; sA[k + 2][r] = va.z; sA[k + 3][r] = va.w;
            sB[k][r] = vb.x; sB[k + 1][r] = vb.y; sB[k + 2][r] = vb.z; sB[k + 3][r] = vb.w;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 64; kk += 2) {
            const float a = sA[kk + (lane >> 5)][wr * 32 + (lane & 31)];
            const float b = sB[kk + (lane >> 5)][wc * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    return acc;
}
// register x of sim_tile's result -> (query row, gallery column) inside the 64 x 64 tile; the column is the same for all 16
__device__ __forceinline__ int sim_tile_row(int x, int tid) { return ((tid >> 6) & 1) * 32 + mfma32_row(x, (tid & 63) >> 5); }
__device__ __forceinline__ int sim_tile_col(int tid) { return (tid >> 7) * 32 + (tid & 31); }

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

// jg_sim_topk (GROUPED = false: goff and n_groups are not looked at) and jg_sim_topk_grouped
template <int LCAP, bool GROUPED>
__global__ __launch_bounds__(256) void sim_topk_kernel(const float* __restrict__ e1, const float* __restrict__ e2, int n_queries,
                                                       int n_gallery, int D, int k, const int32_t* __restrict__ goff, int n_groups,
                                                       int gallery_offset, int merge, int32_t* __restrict__ idx,
                                                       float* __restrict__ score) {
    __shared__ __attribute__((aligned(16))) u64 sStage[64 * 64];       // staging (sA, sB) during a tile's k loop, the queues after it
    __shared__ u64 sL[64][LCAP];
    __shared__ u64 sThr[64];
    __shared__ int sCnt[64];
    float (*sA)[64] = reinterpret_cast<float (*)[64]>(sStage);         // [k][query row]
    float (*sB)[64] = sA + 64;                                         // [k][gallery row]
    u64 (*sQ)[64] = reinterpret_cast<u64 (*)[64]>(sStage);             // [query row][slot]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * 64;

    // the lists start empty, or (merge) from the caller's earlier result: sorted, empty slots (idx < 0) last
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

    int grp_lo = 0, grp_hi = 0, ntiles = (n_gallery + 63) / 64;
    if constexpr (GROUPED) {
        // rows below goff[0] or from goff[n_groups] on belong to no group; without a group there is no candidate and no tile to walk
        grp_lo = n_groups > 0 ? goff[0] : 0;
        grp_hi = n_groups > 0 ? goff[n_groups] : 0;
        if (n_groups <= 0) ntiles = 0;
    }
    for (int tile = 0; tile < ntiles; ++tile) {
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
    // a wave stores the lists of the rows it seeded and flushed itself, each row as one contiguous run
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

template <bool GROUPED>
static hipError_t launch_topk(const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k, const int32_t* g_offsets,
                              int n_groups, int gallery_offset, int merge, int32_t* idx, float* score, hipStream_t s) {
    if (n_queries <= 0) return hipSuccess;
    if (D <= 0 || D % 64 || k < 1 || k > SIM_TOPK_MAX_K || n_gallery < 0 || (GROUPED && (n_groups < 0 || (n_groups > 0 && !g_offsets))) ||
        gallery_offset < 0 || gallery_offset > INT32_MAX - n_gallery)
        return hipErrorInvalidValue;
    const auto kernel = k <= 64 ? sim_topk_kernel<64, GROUPED> : sim_topk_kernel<128, GROUPED>;
    hipLaunchKernelGGL(kernel, dim3((n_queries + 63) / 64), dim3(256), 0, s, queries, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups,
                       gallery_offset, merge, idx, score);
    return hipGetLastError();
}

hipError_t launch_sim_topk(const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k, int gallery_offset,
                           int merge, int32_t* idx, float* score, hipStream_t s) {
    return launch_topk<false>(queries, gallery, n_queries, n_gallery, D, k, nullptr, 0, gallery_offset, merge, idx, score, s);
}

hipError_t launch_sim_topk_grouped(const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k,
                                   const int32_t* g_offsets, int n_groups, int gallery_offset, int merge, int32_t* idx, float* score,
                                   hipStream_t s) {
    return launch_topk<true>(queries, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups, gallery_offset, merge, idx, score, s);
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

// ---------------------------------------------------------------------------------------------
// Word spotting (evaluate_spotting.py:39-82): per clip A = softmax((G C^T)/temp, dim=1) over words
// with re-normalised rows; pred = first argmax_t A[t][w*], score = A[pred][w*].
// One block per clip, one wave per frame row; the W logits of a row go through a per-wave LDS line.
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Limits: W <= SPOT_MAX_W words and T <= SPOT_MAX_T frames per clip (LDS arrays), 0 <= target < W.  The offsets are device
// arrays, so the host cannot check them without a sync: a clip outside the limits gets pred = -1, score = NaN.
constexpr int SPOT_MAX_W = 1024, SPOT_MAX_T = 8192;

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
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
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
constexpr int AM_FB = 128;                   // frames per workgroup
constexpr int AM_REG_W = 128;                // widest clip of the in-register form
constexpr int AM_KEY_PITCH = SPOT_MAX_W;     // keys[clip][word]: the host cannot know sum W (the offsets are device arrays)

size_t attn_matrix_key_elems(int n_clips) { return (size_t)n_clips * AM_KEY_PITCH; }
// The arg-max key of a word: (fp32 bits of the probability << 32) | ~frame, so that a 64-bit max prefers the larger probability and then
// the smaller frame; 0 = no frame yet.  (The pack is a macro: as a function, inlined or not, it changes the register allocation of both
// attn_matrix_kernel instances.)
#define ARGMAX_KEY(prob, frame) (((unsigned long long)__float_as_uint(prob) << 32) | (0xffffffffu - (frame)))
__device__ __forceinline__ int32_t argmax_key_frame(unsigned long long key) { return (int32_t)(0xffffffffu - (unsigned)key); }
__device__ __forceinline__ float argmax_key_prob(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }

__device__ __forceinline__ bool attn_clip_ok(int T, int W, int max_frames) {
    return T > 0 && T <= SPOT_MAX_T && T <= max_frames && W > 0 && W <= SPOT_MAX_W;
}

// F.normalize's 1 / max(||row||, 1e-12); the same bits in every lane
__device__ __forceinline__ float row_rnorm(const float* __restrict__ row, int D, int lane) {
    float sq = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + d);
        sq += v.x * v.x; sq += v.y * v.y; sq += v.z * v.z; sq += v.w * v.w;
    }
    return 1.f / fmaxf(sqrtf(wave_sum(sq)), 1e-12f);
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

// Softmax over the clip's words for the wave's 32 frames (frame0 ..), as torch evaluates it: exp(x - max) / sum exp(x - max); then the
// stores and the arg-max keys.  Accumulator layout: frame = lane & 31, word = 32 tile + mfma32_row(x, lane >> 5).
// TSTEP > 1: the four waves hold different words of the SAME frames and every wave of the workgroup makes this call.
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
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            acc[i][x] = acc[i][x] / temp;
            if (mfma32_row(x, 0) < wl - i * TSTEP * 32) mx = fmaxf(mx, acc[i][x]);
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
            const float e = mfma32_row(x, 0) < wl - i * TSTEP * 32 ? expf(acc[i][x] - mx) : 0.f;
            acc[i][x] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32, 64);
    if constexpr (TSTEP > 1) {
        if (h == 0) sRed[1][wave][l31] = sum;
        __syncthreads();
        sum = ((sRed[1][0][l31] + sRed[1][1][l31]) + sRed[1][2][l31]) + sRed[1][3][l31];
    }
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
                if (kclip) {
                    // first frame of the 32 with the largest probability: max over the lane half, then the lowest lane that holds it
                    float m = fok ? p : -1.f;
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
                    const unsigned long long bal = __ballot(fok && p == m);
                    const unsigned mine = (unsigned)(bal >> (32 * h));
                    if (l31 == 0 && wok && mine) {
                        const unsigned first = frame0 + __ffs(mine) - 1;
                        atomicMax(&kclip[word0 + roff], ARGMAX_KEY(m, first));
                    }
                }
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
    for (int w = wave; w < W; w += 4) {
        const float rn = normalize ? row_rnorm(crow + (long)w * D, D, lane) : 1.f;
        if (lane == 0) sCn[w] = rn;
    }
    for (int f = wave; f < nf; f += 4) {
        const float rn = normalize ? row_rnorm(grow + (long)f * D, D, lane) : 1.f;
        if (lane == 0) sGn[f] = rn;
    }
    float* Aclip = A ? A + aoff[clip] : nullptr;
    unsigned long long* kclip = keys ? keys + (size_t)clip * AM_KEY_PITCH : nullptr;
    const int ntile = (W + 31) >> 5;

    if constexpr (!WIDE) {
        f32x16 acc[4], tot[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int x = 0; x < 16; ++x) { acc[i][x] = 0.f; tot[i][x] = 0.f; }
        const bool active = wave * 32 < nf;
        for (int k0 = 0; k0 < D; k0 += 32) {
            __syncthreads();
            if (tid < 128) am_stage<32>(crow, D, k0, W, ntile * 32, sCn, sC, 128, tid, 128);
            else am_stage<32>(grow, D, k0, nf, (nf + 31) & ~31, sGn, sG, AM_FB, tid - 128, 128);
            __syncthreads();
            if (active) am_mfma<4, 1, 32, 128, AM_FB>(sC, sG, 0, ntile, wave * 32, lane, acc);
            if ((k0 + 32) % AM_KSPLIT == 0 || k0 + 32 == D) am_fold<4>(acc, tot);
        }
        if (active) am_finish<4, 1>(tot, 0, W, T, f0 + wave * 32, temp, Aclip, kclip, sRed, lane, wave);
    } else {
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
    for (int w = threadIdx.x; w < W; w += blockDim.x) {
        const unsigned long long key = ok ? keys[(size_t)clip * AM_KEY_PITCH + w] : 0ull;
        if (best_frame) best_frame[w0 + w] = key ? argmax_key_frame(key) : -1;
        if (best_score) best_score[w0 + w] = key ? argmax_key_prob(key) : __builtin_nanf("");
    }
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
// ASD (evaluate_asd.py:43-51,94-100): cosine(query content, candidate gestures) (eps 1e-8), softmax
// over the first P in {2,4,6} candidates, argmax.  softmax is monotonic -> argmax of the cosine.
// pred[q*3 + {0,1,2}] = first argmax over the first 2/4/6 candidates (or fewer if the query has fewer).
__global__ void asd_kernel(const float* __restrict__ q, const float* __restrict__ cand, const int32_t* __restrict__ coff,
                           int n, int D, float temp, int32_t* __restrict__ pred) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (qi >= n) return;
    const float* qr = q + (long)qi * D;
    float qs = 0.f;
    for (int d = lane; d < D; d += 64) qs += qr[d] * qr[d];
    const float qn = sqrtf(wave_sum(qs));
    const int c0 = coff[qi];
    int P = coff[qi + 1] - c0;
    P = P < 6 ? P : 6;
    float sim[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        sim[p] = -INFINITY;
        if (p < P) {
            const float* cr = cand + (long)(c0 + p) * D;
            float dot = 0.f, cs = 0.f;
            for (int d = lane; d < D; d += 64) { dot += qr[d] * cr[d]; cs += cr[d] * cr[d]; }
            dot = wave_sum(dot);
            const float cn = sqrtf(wave_sum(cs));
            sim[p] = dot / fmaxf(qn * cn, 1e-8f) / temp;
        }
    }
    // the reference takes np.argmax of softmax(sim[:P']) (evaluate_asd.py:47-49,96-100), P' = min(2|4|6, candidates):
    // the softmax is evaluated as torch does (exp(x - max) / sum) so that values it rounds together tie the same way
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int np = (2 * k + 2) < P ? (2 * k + 2) : P;
        float mx = -INFINITY;
#pragma unroll
        for (int p = 0; p < 6; ++p) if (p < np) mx = fmaxf(mx, sim[p]);
        float e[6], den = 0.f;
#pragma unroll
        for (int p = 0; p < 6; ++p) { e[p] = p < np ? expf(sim[p] - mx) : 0.f; den += e[p]; }
        float best = -INFINITY;
        int bi = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const float sc = e[p] / den;
            if (p < np && sc > best) { best = sc; bi = p; }
        }
        if (lane == 0) pred[qi * 3 + k] = np > 0 ? bi : -1;
    }
}

hipError_t launch_asd(const float* q, const float* cand, const int32_t* coff, int n, int D, float temp,
                      int32_t* pred2, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(asd_kernel, dim3((n + 3) / 4), dim3(256), 0, s, q, cand, coff, n, D, temp, pred2);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// ASD itself (evaluate_asd.py:26-51 per time window): which of a scene's candidate tracks gestures to the utterance, how sure, and when.
// Window j of a scene covers frames lo = j hop .. hi = lo + win - 1 (win == 0: one window over everything).  q = mean of the content rows
// of the words that touch [lo, hi], g_p = mean of candidate p's frames inside it, cos_p = <q, g_p> / max(|q| |g_p|, 1e-8) as in asd_kernel,
// prob = softmax(cos / temp) over the candidates that have a frame there, pred = first arg-max.
//
// The unit of work is one (window, candidate) pair, done by ONE wave: lane l owns columns 4 l .. 4 l + 3 of every 256-column chunk, adds the
// pair's rows in ascending row order into its own registers (16-byte loads, four rows in flight, the additions in row order), divides by
// the row count, and the two dot products cross the lanes through wave_sum's fixed butterfly.  So a pair's cosine is a function of its own
// rows alone: not of hop, of the window's place in the workgroup, of the scene's place in the batch or of which wave took the pair.  A
// workgroup owns ASDW_WB windows of a scene and deals their pairs to its four waves in contiguous runs; a wave forms q (same walk over the
// content rows) whenever its run enters a new window -- a window's q is formed by every wave whose run touches it, bit-equal, instead of crossing the
// waves through 64 KB of LDS at D = 1024.  The cosines meet in 4 KB of LDS; then one wave per window, lane = candidate, does the softmax as
// torch does (exp(x - max) / sum) and the stores.
//
// The offsets are device arrays: a scene outside the limits (1..64 candidates, 1..1024 words, 1..max_windows windows, every candidate an
// existing track of 1..8192 frames) gets pred = -1 and NaN rows in all of its windows and none of its rows is read.
constexpr int ASDW_WB = 16;                  // windows per workgroup
constexpr int ASDW_MAX_P = 64;               // candidates per scene: one lane each in the softmax
constexpr int ASDW_MAX_WIN = 8192;           // windows per scene, and frames per window

// acc[c] += rows r = 0 .. n - 1 with sel(r) (wave-uniform), in ascending r; lane l holds columns c 256 + 4 l .. + 3 (zero beyond D)
template <int NC, class Sel>
__device__ __forceinline__ void asdw_sum_rows(const float* __restrict__ rows, int n, int D, int lane, Sel sel, f32x4 (&acc)[NC]) {
    const float* p = rows + lane * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int r = 0;
    for (; r + 4 <= n; r += 4) {
        f32x4 v[4][NC];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < NC; ++c)
                v[u][c] = lane * 4 + c * 256 < D ? *reinterpret_cast<const f32x4*>(p + (long)(r + u) * D + c * 256) : zero;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (sel(r + u)) {
#pragma unroll
                for (int c = 0; c < NC; ++c) { acc[c].x += v[u][c].x; acc[c].y += v[u][c].y; acc[c].z += v[u][c].z; acc[c].w += v[u][c].w; }
            }
    }
    for (; r < n; ++r)
        if (sel(r)) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const f32x4 v = lane * 4 + c * 256 < D ? *reinterpret_cast<const f32x4*>(p + (long)r * D + c * 256) : zero;
                acc[c].x += v.x; acc[c].y += v.y; acc[c].z += v.z; acc[c].w += v.w;
            }
        }
}

// frames lo .. hi of window j; false: the window lies behind every possible frame
__device__ __forceinline__ bool asdw_window(int j, int win, int hop, int& lo, int& hi) {
    const long l = win ? (long)j * hop : 0;
    lo = (int)(l < SPOT_MAX_T ? l : SPOT_MAX_T);
    hi = win ? lo + win - 1 : SPOT_MAX_T - 1;
    return l < SPOT_MAX_T;
}

template <int NC>            // 256-column chunks per row: D <= 256 NC
__global__ __launch_bounds__(256) void asd_windows_kernel(const float* __restrict__ g, const int32_t* __restrict__ goff, int n_tracks,
                                                          const float* __restrict__ c, const int32_t* __restrict__ coff,
                                                          const int32_t* __restrict__ wstart, const int32_t* __restrict__ wend,
                                                          const int32_t* __restrict__ trk, const int32_t* __restrict__ soff,
                                                          const int32_t* __restrict__ woff, const int64_t* __restrict__ poff, int D, int win,
                                                          int hop, int max_windows, float temp, float* __restrict__ prob,
                                                          float* __restrict__ cosv, int32_t* __restrict__ pred) {
    __shared__ int sWs[SPOT_MAX_W], sWe[SPOT_MAX_W];     // the scene's word bounds
    __shared__ float sCos[ASDW_WB][ASDW_MAX_P];
    __shared__ int sHas[ASDW_WB];                        // the window has a word
    const int scene = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s0 = soff[scene], P = soff[scene + 1] - s0;
    const int w0 = coff[scene], W = coff[scene + 1] - w0;
    const int o0 = woff[scene], NW = woff[scene + 1] - o0;
    bool ok = s0 >= 0 && P >= 1 && P <= ASDW_MAX_P && w0 >= 0 && W >= 1 && W <= SPOT_MAX_W && o0 >= 0 && NW >= 1 && NW <= max_windows;
    int trow = 0, tlen = 0;                              // lane p: first row and frames of candidate p's track
    if (ok) {
        bool bad = false;
        if (lane < P) {
            const int t = trk[s0 + lane];
            bad = t < 0 || t >= n_tracks;
            if (!bad) {
                trow = goff[t];
                tlen = goff[t + 1] - trow;
                bad = trow < 0 || tlen < 1 || tlen > SPOT_MAX_T;
            }
        }
        ok = __ballot(bad) == 0ull;
    }
    const float nan = __builtin_nanf("");
    if (!ok) {                                           // block-uniform: every window of the scene is undecided, whatever their number
        if (o0 < 0 || NW < 1) return;
        const long nb = gridDim.y, first = (long)blockIdx.y * 256 + tid;
        for (long j = first; j < NW; j += nb * 256) pred[o0 + j] = -1;
        if (P >= 1) {
            const long base = poff[scene], ne = (long)NW * P;
            for (long e = first; e < ne; e += nb * 256) {
                prob[base + e] = nan;
                if (cosv) cosv[base + e] = nan;
            }
        }
        return;
    }
    const int j0 = blockIdx.y * ASDW_WB;
    if (j0 >= NW) return;
    const int nj = NW - j0 < ASDW_WB ? NW - j0 : ASDW_WB;
    if (win)
        for (int w = tid; w < W; w += 256) { sWs[w] = wstart[w0 + w]; sWe[w] = wend[w0 + w]; }
    __syncthreads();

    // this wave's run of (window, candidate) pairs
    const int items = nj * P;
    const int i_end = (wave + 1) * items / 4;
    int cur = -1, lo = 0, hi = 0, has = 0;
    float qn = 0.f;
    f32x4 q[NC];
    for (int i = wave * items / 4; i < i_end; ++i) {
        const int jj = i / P, p = __builtin_amdgcn_readfirstlane(i - jj * P);
        if (jj != cur) {
            cur = jj;
            has = 0;
            int first = 0, last = W - 1, cnt = W;
            const bool inside = asdw_window(j0 + jj, win, hop, lo, hi);
            if (win) {                                   // the words that touch [lo, hi]: their number, the first and the last
                first = -1; last = -1; cnt = 0;
                for (int k = 0; k < W; k += 64) {
                    const int w = k + lane;
                    const unsigned long long m = __ballot(w < W && sWe[w] >= lo && sWs[w] <= hi);
                    if (m) {
                        if (first < 0) first = k + __builtin_ctzll(m);
                        last = k + 63 - __builtin_clzll(m);
                        cnt += __builtin_popcountll(m);
                    }
                }
            }
#pragma unroll
            for (int x = 0; x < NC; ++x) q[x] = f32x4{0.f, 0.f, 0.f, 0.f};
            qn = 0.f;
            if (inside && cnt > 0) {
                has = 1;
                asdw_sum_rows<NC>(c + (long)(w0 + first) * D, last - first + 1, D, lane,
                                  [&](int r) { return win == 0 || (sWe[first + r] >= lo && sWs[first + r] <= hi); }, q);
                const float n = (float)cnt;
                float sq = 0.f;
#pragma unroll
                for (int x = 0; x < NC; ++x) {
                    q[x].x /= n; q[x].y /= n; q[x].z /= n; q[x].w /= n;
                    sq += q[x].x * q[x].x; sq += q[x].y * q[x].y; sq += q[x].z * q[x].z; sq += q[x].w * q[x].w;
                }
                qn = sqrtf(wave_sum(sq));
            }
            if (lane == 0) sHas[jj] = has;
        }
        const int tl = __builtin_amdgcn_readlane(tlen, p), tr = __builtin_amdgcn_readlane(trow, p);
        const int nr = (hi < tl - 1 ? hi : tl - 1) - lo + 1;
        float cs = 0.f;
        if (has && nr > 0) {
            f32x4 a[NC];
#pragma unroll
            for (int x = 0; x < NC; ++x) a[x] = f32x4{0.f, 0.f, 0.f, 0.f};
            asdw_sum_rows<NC>(g + (long)(tr + lo) * D, nr, D, lane, [](int) { return true; }, a);
            const float n = (float)nr;
            float dot = 0.f, sq = 0.f;
#pragma unroll
            for (int x = 0; x < NC; ++x) {
                a[x].x /= n; a[x].y /= n; a[x].z /= n; a[x].w /= n;
                dot += a[x].x * q[x].x; dot += a[x].y * q[x].y; dot += a[x].z * q[x].z; dot += a[x].w * q[x].w;
                sq += a[x].x * a[x].x; sq += a[x].y * a[x].y; sq += a[x].z * a[x].z; sq += a[x].w * a[x].w;
            }
            dot = wave_sum(dot);
            cs = dot / fmaxf(qn * sqrtf(wave_sum(sq)), 1e-8f);
        }
        if (lane == 0) sCos[jj][p] = cs;
    }
    __syncthreads();

    // one wave per window, lane = candidate
    for (int jj = wave; jj < nj; jj += 4) {
        const int j = j0 + jj;
        const bool inside = asdw_window(j, win, hop, lo, hi);
        const bool cand = lane < P;
        const bool present = cand && inside && (hi < tlen - 1 ? hi : tlen - 1) - lo + 1 > 0;
        const long row = poff[scene] + (long)j * P;
        if (!sHas[jj] || __ballot(present) == 0ull) {    // undecided
            if (cand) {
                prob[row + lane] = nan;
                if (cosv) cosv[row + lane] = nan;
            }
            if (lane == 0) pred[o0 + j] = -1;
            continue;
        }
        const float cs = cand ? sCos[jj][lane] : 0.f;
        const float x = cs / temp;
        const float mx = wmax(present ? x : -INFINITY);
        const float e = present ? expf(x - mx) : 0.f;
        const float pr = e / wave_sum(e);
        float best = present ? pr : -1.f;
        int bi = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (cand) {
            prob[row + lane] = pr;
            if (cosv) cosv[row + lane] = present ? cs : nan;
        }
        if (lane == 0) pred[o0 + j] = bi;
    }
}

hipError_t launch_asd_windows(const float* g, const int32_t* goff, int n_tracks, const float* c, const int32_t* coff, const int32_t* wstart,
                              const int32_t* wend, const int32_t* trk, const int32_t* soff, int n_scenes, int D, int win, int hop,
                              const int32_t* woff, const int64_t* poff, int max_windows, float temp, float* prob, float* cosv,
                              int32_t* pred, hipStream_t s) {
    if (n_scenes <= 0) return hipSuccess;
    if (D <= 0 || D % 64 || D > ASDW_MAX_D || n_tracks < 0 || win < 0 || win > ASDW_MAX_WIN || (win && (hop < 1 || !wstart || !wend)) ||
        max_windows < 1 || max_windows > ASDW_MAX_WIN || !(temp > 0.f))
        return hipErrorInvalidValue;
    const dim3 grid(n_scenes, (max_windows + ASDW_WB - 1) / ASDW_WB);
#define ASDW_LAUNCH(NC) hipLaunchKernelGGL(asd_windows_kernel<NC>, grid, dim3(256), 0, s, g, goff, n_tracks, c, coff, wstart, wend, trk, soff, \
                                           woff, poff, D, win, hop, max_windows, temp, prob, cosv, pred)
    if (D <= 256) ASDW_LAUNCH(1);
    else if (D <= 512) ASDW_LAUNCH(2);
    else ASDW_LAUNCH(4);
#undef ASDW_LAUNCH
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Audio-visual offset of a clip from its two streams of window embeddings (GestSync's use; the SyncNet convention).  Clip i owns video
// rows voff[i] .. voff[i + 1] - 1 (Tv) and audio rows aoff[i] .. (Ta).  For a shift d in -R .. R the pairs are (t, t + d) with
// 0 <= t < Tv, 0 <= t + d < Ta (n_d of them) and
//     curve[d + R] = (1 / n_d) sum_t <v_t, a_{t+d}> / max(||v_t|| ||a_{t+d}||, 1e-8)      (NaN when n_d < min_overlap)
// offset = the d of the first maximum over the non-NaN entries (np.nanargmax), conf = that maximum - their median (np.nanmedian).
//
// The band of dot products runs on v_mfma_f32_32x32x2_f32 with [k][row] staging, as sim_tile and attn_matrix_kernel: a block of 32
// video rows (B operand, column = lane & 31) against the 32 + 2R audio rows its band touches (A operand, NT tiles of 32).  The four
// waves split every 32-wide k chunk (eight k each, so all four are busy whatever R is) and their partial sums meet in LDS in wave
// order; a wave's chain is cut every SYNC_KSPLIT terms like attn_matrix_kernel's.  A dot product depends on its two rows alone.
// ONE workgroup walks its clip's row blocks in ascending order and thread d + R adds the block's cosines of shift d to its running sum
// in ascending t, with a compensation term (Kahan): the per-shift sum is the left-to-right sum over t whatever the clip's length -- at
// 150 rows and a cosine of 0.9 the plain fp32 sum's rounding is 3-4 x the error of everything else in the curve, with the compensation
// it disappears -- no partial sums of row blocks cross workgroups, and nothing but the outputs is written.  (A (clip, row block) grid needs
// scratch, which this call does not have, or floating-point atomics in arrival order; a clip is 5 blocks at 150 rows and the batch
// supplies the parallelism.  jg_sync_offset_windows below is that grid: it writes the cosines to a band in scratch and sums them there.)
constexpr int SYNC_KC = 32;                  // k per staged chunk
constexpr int SYNC_KSPLIT = 128;             // terms of one wave's fmaf chain before it is folded
static_assert((4 * SYNC_KSPLIT) % SYNC_KC == 0 && SYNC_KC % 8 == 0, "a wave takes a quarter of every chunk, two k per MFMA, and its chain is cut at whole chunks");

// ||row||; the same bits in every lane
__device__ __forceinline__ float row_norm(const float* __restrict__ row, int D, int lane) {
    float sq = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + d);
        sq += v.x * v.x; sq += v.y * v.y; sq += v.z * v.z; sq += v.w * v.w;
    }
    return sqrtf(wave_sum(sq));
}

// The parts jg_sync_offset and jg_sync_offset_windows are both built from: the cosines of one block of 32 video rows (sync_band_block), one
// step of a per-shift sum (sync_kahan_add), a shift's mean (sync_mean) and the decision over a curve (sync_decide).  A cosine, a sum and a
// decision have the same bits in both entries because they are the same code, fed the same values in the same order.
template <int NT>
struct SyncBandLds {
    static constexpr int NA = 32 * NT, BP = NA + 1;
    float V[SYNC_KC * 32];       // [k][video row]
    float A[SYNC_KC * NA];       // [k][audio row of the band]
    float red[4][16][64];        // one tile's accumulators, per wave
    float band[32 * BP];         // [video row][d + R]: the block's cosines
    float vn[32], an[NA];
};

// sm.band[i * BP + d + R] = cosine of video row vrows[i] (i < nv; the rows behind read as zero rows) and audio row arows[ja0 + R + i + d],
// for every d in -R .. R; an audio row outside 0 .. Ta - 1 reads as a zero row (cosine 0 by the 1e-8 floor: the callers leave those entries
// out).  All 256 threads call it; it begins with a barrier in front of its first LDS write that another thread may still read (V, A) and
// ends with one, so sm.band may be read at once and overwritten only behind the next call's first barrier.
template <int NT>
__device__ __forceinline__ void sync_band_block(SyncBandLds<NT>& sm, const float* __restrict__ vrows, int nv, const float* __restrict__ arows,
                                                int Ta, int ja0, int D, int R, int tid) {
    constexpr int NA = SyncBandLds<NT>::NA, BP = SyncBandLds<NT>::BP;
    const int lane = tid & 63, wave = tid >> 6;
    const int W = 2 * R + 1;
    const int nband = 32 + 2 * R;            // audio rows a block's band touches (<= NA)
    for (int r = wave; r < 32 + NA; r += 4) {
        float nr = 0.f;
        if (r < 32) {
            if (r < nv) nr = row_norm(vrows + (long)r * D, D, lane);
            if (lane == 0) sm.vn[r] = nr;
        } else {
            const int j = r - 32, a = ja0 + j;
            if (j < nband && a >= 0 && a < Ta) nr = row_norm(arows + (long)a * D, D, lane);
            if (lane == 0) sm.an[j] = nr;
        }
    }
    f32x16 acc[NT], tot[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) { acc[i][x] = 0.f; tot[i][x] = 0.f; }
    const int sr = tid & 31, sk = (tid >> 5) * 4;
    for (int k0 = 0; k0 < D; k0 += SYNC_KC) {
        __syncthreads();
        {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (sr < nv) v = *reinterpret_cast<const f32x4*>(vrows + (long)sr * D + k0 + sk);
            float* d = sm.V + sk * 32 + sr;
            d[0] = v.x; d[32] = v.y; d[64] = v.z; d[96] = v.w;
        }
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int j = u * 32 + sr, a = ja0 + j;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j < nband && a >= 0 && a < Ta) v = *reinterpret_cast<const f32x4*>(arows + (long)a * D + k0 + sk);
            float* d = sm.A + sk * NA + j;
            d[0] = v.x; d[NA] = v.y; d[2 * NA] = v.z; d[3 * NA] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < SYNC_KC / 4; kk += 2) {
            const int kr = wave * (SYNC_KC / 4) + kk + (lane >> 5);
            const float b = sm.V[kr * 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const float a = sm.A[kr * NA + i * 32 + (lane & 31)];
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
            }
        }
        if ((k0 + SYNC_KC) % (4 * SYNC_KSPLIT) == 0 || k0 + SYNC_KC == D) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int x = 0; x < 16; ++x) { tot[i][x] += acc[i][x]; acc[i][x] = 0.f; }
        }
    }
    // the waves' partial sums of one tile at a time, in wave order; register x of lane l: audio band column 32 n + mfma32_row(x, l >> 5),
    // video row l & 31
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        __syncthreads();
#pragma unroll
        for (int x = 0; x < 16; ++x) sm.red[wave][x][lane] = tot[n][x];
        __syncthreads();
        for (int e = tid; e < 1024; e += 256) {
            const int x = e >> 6, l = e & 63;
            const float dot = ((sm.red[0][x][l] + sm.red[1][x][l]) + sm.red[2][x][l]) + sm.red[3][x][l];
            const int i = l & 31, j = n * 32 + mfma32_row(x, l >> 5), dd = j - i;
            if (dd >= 0 && dd < W) sm.band[i * BP + dd] = dot / fmaxf(sm.vn[i] * sm.an[j], 1e-8f);
        }
    }
    __syncthreads();
}

// S += x with the compensation term Sc (Kahan)
__device__ __forceinline__ void sync_kahan_add(float& S, float& Sc, float x) {
    const float y = x - Sc, t = S + y;
    Sc = (t - S) - y;
    S = t;
}

// the curve entry of a shift whose cnt pairs sum to S
__device__ __forceinline__ float sync_mean(float S, int cnt, int min_overlap) {
    return cnt >= (min_overlap > 1 ? min_overlap : 1) ? S / (float)cnt : __builtin_nanf("");
}

// offset and conf of the curve sCurve[0 .. W - 1] (LDS, written by the threads k = 0 .. W - 1 of the group that calls with them; sMed: two
// words of the group's own).  Every thread of the workgroup calls it (two barriers); a thread with k >= W only waits.  out_offset == nullptr:
// the group has nothing to decide.
__device__ __forceinline__ void sync_decide(const float* sCurve, float* sMed, int W, int R, int k, int32_t* out_offset, float* out_conf) {
    __syncthreads();
    if (k < W) {                 // the median by rank: entry e is the (rank)-th smallest of the m non-NaN entries (ties by position)
        const float v = sCurve[k];
        int m = 0, rank = 0;
        for (int q = 0; q < W; ++q) {
            const float c = sCurve[q];
            m += c == c;
            rank += (c < v || (c == v && q < k)) ? 1 : 0;
        }
        if (v == v) {
            if (rank == (m - 1) / 2) sMed[0] = v;
            if (rank == m / 2) sMed[1] = v;
        }
    }
    __syncthreads();
    if (k == 0 && out_offset) {
        int best = -1;
        float mx = 0.f;
        for (int q = 0; q < W; ++q) {
            const float c = sCurve[q];
            if (c == c && (best < 0 || c > mx)) { best = q; mx = c; }
        }
        *out_offset = best < 0 ? 0 : best - R;
        *out_conf = best < 0 ? __builtin_nanf("") : mx - (sMed[0] + sMed[1]) * 0.5f;
    }
}

template <int NT>
__global__ __launch_bounds__(256) void sync_offset_kernel(const float* __restrict__ vid, const int32_t* __restrict__ voff,
                                                          const float* __restrict__ aud, const int32_t* __restrict__ aoff, int D, int R,
                                                          int min_overlap, float* __restrict__ curve, int32_t* __restrict__ offset,
                                                          float* __restrict__ conf) {
    constexpr int BP = SyncBandLds<NT>::BP;
    __shared__ SyncBandLds<NT> sm;
    __shared__ float sCurve[2 * SYNC_MAX_R + 1];
    __shared__ float sMed[2];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int v0 = voff[clip], Tv = voff[clip + 1] - v0;
    const int a0 = aoff[clip], Ta = aoff[clip + 1] - a0;
    const int W = 2 * R + 1;
    const float nan = __builtin_nanf("");
    if (Tv < 1 || Tv > SYNC_MAX_T || Ta < 1 || Ta > SYNC_MAX_T) {       // block-uniform: nothing of the clip is read
        if (curve && tid < W) curve[(long)clip * W + tid] = nan;
        if (tid == 0) { offset[clip] = 0; conf[clip] = nan; }
        return;
    }
    float S = 0.f, Sc = 0.f;                 // thread d + R: running sum of shift d and its compensation
    for (int t0 = 0; t0 < Tv; t0 += 32) {
        const int nv = Tv - t0 < 32 ? Tv - t0 : 32;
        sync_band_block<NT>(sm, vid + (long)(v0 + t0) * D, nv, aud + (long)a0 * D, Ta, t0 - R, D, R, tid);
        if (tid < W) {
            const int d = tid - R;
            for (int i = 0; i < nv; ++i) {
                const int a = t0 + i + d;
                if (a >= 0 && a < Ta) sync_kahan_add(S, Sc, sm.band[i * BP + tid]);
            }
        }
    }
    if (tid < W) {
        const int d = tid - R;
        const int lo = d < 0 ? -d : 0, hi = Tv < Ta - d ? Tv : Ta - d;
        const float v = sync_mean(S, hi - lo, min_overlap);
        sCurve[tid] = v;
        if (curve) curve[(long)clip * W + tid] = v;
    }
    sync_decide(sCurve, sMed, W, R, tid, offset + clip, conf + clip);
}

// ---- jg_sync_offset_windows: the band of cosines written once by a (clip, row block) grid, then a windowed reduction over it ----
// what both kernels decide alike: the clip's tracks and windows, or false = the clip is UNDECIDED in all its windows (nothing of it is read,
// none of its band rows is written).  o0 / NW are set in either case.
__device__ __forceinline__ bool syncw_clip(int clip, const int32_t* __restrict__ voff, long n_vid_rows, int max_rows,
                                           const int32_t* __restrict__ aoff, int n_aud, const int32_t* __restrict__ a_of,
                                           const int32_t* __restrict__ woff, int max_windows, int& v0, int& Tv, int& a0, int& Ta, int& o0,
                                           int& NW) {
    v0 = voff[clip]; Tv = voff[clip + 1] - v0;
    o0 = woff[clip]; NW = woff[clip + 1] - o0;
    a0 = 0; Ta = 0;
    const int at = a_of ? a_of[clip] : clip;
    if (at < 0 || at >= n_aud) return false;
    a0 = aoff[at]; Ta = aoff[at + 1] - a0;
    return v0 >= 0 && Tv >= 1 && Tv <= max_rows && (long)v0 + Tv <= n_vid_rows && a0 >= 0 && Ta >= 1 && Ta <= max_rows && o0 >= 0 &&
           NW >= 1 && NW <= max_windows;
}

// grid (clip, block of 32 video rows): band[(v0 + t)][d + R], NaN where audio row t + d does not exist
template <int NT>
__global__ __launch_bounds__(256) void sync_band_kernel(const float* __restrict__ vid, const int32_t* __restrict__ voff, long n_vid_rows,
                                                        int max_rows, const float* __restrict__ aud, const int32_t* __restrict__ aoff,
                                                        int n_aud, const int32_t* __restrict__ a_of, const int32_t* __restrict__ woff,
                                                        int max_windows, int D, int R, float* __restrict__ band) {
    constexpr int BP = SyncBandLds<NT>::BP;
    __shared__ SyncBandLds<NT> sm;
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int t0 = blockIdx.y * 32;
    int v0, Tv, a0, Ta, o0, NW;
    if (!syncw_clip(clip, voff, n_vid_rows, max_rows, aoff, n_aud, a_of, woff, max_windows, v0, Tv, a0, Ta, o0, NW) || t0 >= Tv) return;
    const int W = 2 * R + 1;
    const int nv = Tv - t0 < 32 ? Tv - t0 : 32;
    sync_band_block<NT>(sm, vid + (long)(v0 + t0) * D, nv, aud + (long)a0 * D, Ta, t0 - R, D, R, tid);
    // the block's nv x W entries are one contiguous piece of the band: consecutive threads store consecutive words (and read LDS words
    // that are consecutive but for the step at a row's end, BP being odd)
    float* out = band + (long)(v0 + t0) * W;
    const float nan = __builtin_nanf("");
    for (int e = tid; e < nv * W; e += 256) {
        const int i = e / W, k = e - i * W, a = t0 + i + k - R;
        out[e] = a >= 0 && a < Ta ? sm.band[i * BP + k] : nan;
    }
}

// grid (clip, chunk of 256 / G windows), G = the power of two >= 2R + 1: a group of G threads takes one window, thread k = d + R of it walks
// column d of the band over the window's rows in ascending t -- the values and the order of sync_offset_kernel's sum
constexpr int SYNCW_MAX_GROUPS = 8;
__global__ __launch_bounds__(256) void sync_windows_kernel(const int32_t* __restrict__ voff, long n_vid_rows, int max_rows,
                                                           const int32_t* __restrict__ aoff, int n_aud, const int32_t* __restrict__ a_of,
                                                           const int32_t* __restrict__ woff, int max_windows, int R, int min_overlap, int win,
                                                           int hop, int G, const float* __restrict__ band, float* __restrict__ curve,
                                                           int32_t* __restrict__ offset, float* __restrict__ conf) {
    __shared__ float sCurve[SYNCW_MAX_GROUPS][2 * SYNC_MAX_R + 1];
    __shared__ float sMed[SYNCW_MAX_GROUPS][2];
    const int clip = blockIdx.x, tid = threadIdx.x;
    const int W = 2 * R + 1, groups = 256 / G;
    const float nan = __builtin_nanf("");
    int v0, Tv, a0, Ta, o0, NW;
    if (!syncw_clip(clip, voff, n_vid_rows, max_rows, aoff, n_aud, a_of, woff, max_windows, v0, Tv, a0, Ta, o0, NW)) {
        if (o0 < 0 || NW < 1) return;                    // block-uniform: every window of the clip is undecided, whatever their number
        const long nb = gridDim.y, first = (long)blockIdx.y * 256 + tid;
        for (long j = first; j < NW; j += nb * 256) { offset[o0 + j] = 0; conf[o0 + j] = nan; }
        if (curve)
            for (long e = first; e < (long)NW * W; e += nb * 256) curve[(long)o0 * W + e] = nan;
        return;
    }
    const int grp = tid / G, k = tid - grp * G;
    // (block-uniform trip count: the grid's y covers max_windows up to the 65535 blocks a grid may have, the rest by striding)
    for (long jb = (long)blockIdx.y * groups; jb < NW; jb += (long)gridDim.y * groups) {
        const long j = jb + grp;                             // the group's window
        const bool mine = j < NW;
        if (mine && k < W) {
            const long l = win ? j * hop : 0;
            const int lo = (int)(l < Tv ? l : Tv);
            const int hi = (win && (long)lo + win < Tv ? lo + win : Tv) - 1;
            const int d = k - R;
            const int t_lo = lo > -d ? lo : -d, t_hi = hi < Ta - 1 - d ? hi : Ta - 1 - d;      // the rows t with audio row t + d
            float S = 0.f, Sc = 0.f;
            const int cnt = t_hi >= t_lo ? t_hi - t_lo + 1 : 0;
            const float* p = band + ((long)v0 + t_lo) * W + k;
            int left = cnt;
            for (; left >= 8; left -= 8, p += 8 * W) {       // eight loads in flight, added in order: the walk is bound by their latency
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = p[u * W];
#pragma unroll
                for (int u = 0; u < 8; ++u) sync_kahan_add(S, Sc, x[u]);
            }
            for (; left >= 4; left -= 4, p += 4 * W) {
                const float x0 = p[0], x1 = p[W], x2 = p[2 * W], x3 = p[3 * W];
                sync_kahan_add(S, Sc, x0); sync_kahan_add(S, Sc, x1); sync_kahan_add(S, Sc, x2); sync_kahan_add(S, Sc, x3);
            }
            for (; left > 0; --left, p += W) sync_kahan_add(S, Sc, p[0]);
            const float v = sync_mean(S, cnt, min_overlap);
            sCurve[grp][k] = v;
            if (curve) curve[(long)(o0 + j) * W + k] = v;
        }
        sync_decide(sCurve[grp], sMed[grp], W, R, mine ? k : W, mine ? offset + o0 + j : nullptr, mine ? conf + o0 + j : nullptr);
        __syncthreads();                                 // the curve and the medians are the next window's to overwrite
    }
}

hipError_t launch_sync_offset(const float* vid, const int32_t* voff, const float* aud, const int32_t* aoff, int n, int D, int R, int min_overlap,
                              float* curve, int32_t* offset, float* conf, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (D <= 0 || D % 64 || D > SYNC_MAX_D || R < 0 || R > SYNC_MAX_R || min_overlap < 1) return hipErrorInvalidValue;
    const int nt = (32 + 2 * R + 31) / 32;
#define SYNC_LAUNCH(NT) hipLaunchKernelGGL(sync_offset_kernel<NT>, dim3(n), dim3(256), 0, s, vid, voff, aud, aoff, D, R, min_overlap, curve, offset, conf)
    switch (nt) {
        case 1: SYNC_LAUNCH(1); break;
        case 2: SYNC_LAUNCH(2); break;
        case 3: SYNC_LAUNCH(3); break;
        case 4: SYNC_LAUNCH(4); break;
        default: SYNC_LAUNCH(5); break;
    }
#undef SYNC_LAUNCH
    return hipGetLastError();
}

hipError_t launch_sync_offset_windows(const float* vid, const int32_t* voff, int n, long n_vid_rows, int max_rows, const float* aud,
                                      const int32_t* aoff, int n_aud, const int32_t* a_of, int D, int R, int min_overlap, int win, int hop,
                                      const int32_t* woff, int max_windows, float* band, float* curve, int32_t* offset, float* conf,
                                      hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (D <= 0 || D % 64 || D > SYNC_MAX_D || R < 0 || R > SYNC_MAX_R || min_overlap < 1 || max_rows < 1 || max_rows > SYNCW_MAX_T ||
        max_windows < 1 || max_windows > SYNCW_MAX_WINDOWS || win < 0 || (win > 0 && hop < 1) || n_vid_rows < 0 || n_aud < 1 || !band)
        return hipErrorInvalidValue;
    const int nt = (32 + 2 * R + 31) / 32;
    const dim3 bgrid(n, (max_rows + 31) / 32);
#define SYNC_LAUNCH(NT) hipLaunchKernelGGL(sync_band_kernel<NT>, bgrid, dim3(256), 0, s, vid, voff, n_vid_rows, max_rows, aud, aoff, n_aud, a_of, \
                                           woff, max_windows, D, R, band)
    switch (nt) {
        case 1: SYNC_LAUNCH(1); break;
        case 2: SYNC_LAUNCH(2); break;
        case 3: SYNC_LAUNCH(3); break;
        case 4: SYNC_LAUNCH(4); break;
        default: SYNC_LAUNCH(5); break;
    }
#undef SYNC_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int G = 32;
    while (G < 2 * R + 1) G *= 2;
    const int groups = 256 / G, chunks = (max_windows + groups - 1) / groups;
    hipLaunchKernelGGL(sync_windows_kernel, dim3(n, chunks < 65535 ? chunks : 65535), dim3(256), 0, s, voff, n_vid_rows, max_rows, aoff,
                       n_aud, a_of, woff, max_windows, R, min_overlap, win, hop, G, band, curve, offset, conf);
    return hipGetLastError();
}
