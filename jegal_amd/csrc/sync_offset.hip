// Audio-visual offset kernels (gfx950) on exact-fp32 MFMA: per clip, and over time.
#include "metric_parts.h"

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
