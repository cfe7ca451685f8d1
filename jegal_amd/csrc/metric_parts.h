// Device parts that more than one family of metric kernels uses (retrieval.hip, spotting.hip, asd.hip, sync_offset.hip).
#pragma once
#include "common.h"

// One 64 x 64 tile <e1[i0 ..], e2[j0 ..]> over all of D: the calling wave's 32 x 32 part of it.  sA / sB: [k][query row] / [k][gallery
// row] staging, 64 x 64 floats each; rows from n_rows / n_cols on are zero.  Begins with a barrier, so the buffers may hold anything that
// every wave has finished reading; the last chunk's reads are NOT fenced from what the caller writes there next.
// GT: the element type of e2's rows as stored, float or _Float16 (sim_row4: widened on the way into sB, which is exact, so the MFMA chain
// and with it every bit of the result are those of the widened rows).
__device__ __forceinline__ f32x4 sim_row4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 sim_row4(const _Float16* p) {
    typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
    const h16x4 v = *reinterpret_cast<const h16x4*>(p);
    return f32x4{(float)v.x, (float)v.y, (float)v.z, (float)v.w};
}
template <class GT = float>
__device__ __forceinline__ f32x16 sim_tile(const float* __restrict__ e1, const GT* __restrict__ e2, int i0, int j0, int n_rows, int n_cols,
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
            if (j0 + r < n_cols) vb = sim_row4(e2 + (long)(j0 + r) * D + k0 + k);
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

// max over the wave's lanes
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// (best, bi) <- the pair with the larger `best`, on equal ones the lower index, among the lanes that differ from this one in the lane bits
// 32 .. LAST.  LAST = 1: over the wave, the same pair in every lane; LAST = 32: over the lane and its partner in the other half.
template <int LAST = 1>
__device__ __forceinline__ void wave_best_first(float& best, int& bi) {
#pragma unroll
    for (int o = 32; o >= LAST; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
}

// ||row||; the same bits in every lane
__device__ __forceinline__ float row_norm(const float* __restrict__ row, int D, int lane) {
    float sq = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + d);
        sq += v.x * v.x; sq += v.y * v.y; sq += v.z * v.z; sq += v.w * v.w;
    }
    return sqrtf(wave_sum(sq));
}
// F.normalize's 1 / max(||row||, 1e-12); the same bits in every lane
__device__ __forceinline__ float row_rnorm(const float* __restrict__ row, int D, int lane) { return 1.f / fmaxf(row_norm(row, D, lane), 1e-12f); }
