// ASD kernels (gfx950): the grade, and the speaker probabilities per time window.
#include "metric_parts.h"

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
        wave_best_first(best, bi);
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
