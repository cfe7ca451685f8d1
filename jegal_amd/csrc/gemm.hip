// MFMA fp16 GEMM / implicit-GEMM convolution for gfx950 (CDNA4).
//
//   out[m][n] = epi( sum_k A[m][k] * (Wh[n][k] + Wl[n][k]) ),   A, W both K-contiguous.
//
// * v_mfma_f32_16x16x32_f16, fp32 accumulate.  The WEIGHT tile is the MFMA "A" operand and the
//   activation tile the "B" operand, so a lane ends up with 4 consecutive n for one m and the
//   epilogue stores 16 B (fp32) / 8 B (fp16) per lane.
// * Workgroup = 4 waves, each wave a 64(m) x 64(n) sub-tile (4x4 MFMA tiles, 64 accumulator
//   VGPRs); block tile 128x128 (2x2 waves) or 256x64 (4x1 waves, for N <= 64 convolutions).
// * K-step 64: both operand tiles are staged through LDS in full 128-B rows (8 lanes x 16 B per
//   row -> whole cache lines from HBM/L2), XOR-swizzled (chunk ^= (row>>1)&7) so the
//   ds_read_b128 fragment reads of all four 16-lane groups are bank-conflict free.
// * Register-staged software pipeline: the global loads of tile t+1 are issued before the MFMAs
//   of tile t and written to LDS after them (guide T14).
// * W2 mode: the fp32 weight is carried as hi+lo fp16 pair (2 MFMAs per k-step) -- weight
//   rounding, not activation rounding, dominates the end-to-end error (precision).
// * CONV: the activation "row" m is an output pixel (img,oh,ow) of an NHWC tensor and
//   k = (kh,kw,c); out-of-image taps are zero-filled at staging time.
// * The parts, in file order: act4; gemm_kernel (register-staged); for the LDS-DMA kernel the tile context (TileCtx; the tile's sizes
//   and LDS layout are GldsTile in gemm_plan.h), load_scale_bias, the epilogue functions epi_ln_producer and epi_rows16 (plain instances), then
//   gemm_glds_kernel itself: persistent tile walk, per-lane loader state (setup / stage_begin / stage_piece), k loop, LayerNorm-fused
//   epilogue and the ladder that picks one of the other epilogues (what is still written out in the kernel body, and why: see there).
// * Host side (end of the file): launch_gemm asks the planner (gemm_plan.h / gemm_plan.hip) which instance a launch gets and
//   launches that entry of one table of thunks; no admission rule and no tile choice lives in this file.
#include "common.h"
#include "gemm_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#ifndef JG_LNF_JD
#define JG_LNF_JD 2            // LN-fused epilogue: 16-row block in front of which the next tile's first DMA is issued (experiments: 1 / 3 / 4)
#endif

JG_NS_BEGIN

// epilogue activation (GemmArgs::relu): 0 none, 1 ReLU, 2 exact GELU 0.5 v (1 + erf(v / sqrt 2)) (XLM-RoBERTa's intermediate layer;
// the conv instances are compiled with ReLU only)
__device__ __forceinline__ f32x4 act4(f32x4 v, int act) {
    if (act == 1) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    } else if (act == 2) {
        v.x = 0.5f * v.x * (1.f + erff(v.x * 0.70710678118654752f)); v.y = 0.5f * v.y * (1.f + erff(v.y * 0.70710678118654752f));
        v.z = 0.5f * v.z * (1.f + erff(v.z * 0.70710678118654752f)); v.w = 0.5f * v.w * (1.f + erff(v.w * 0.70710678118654752f));
    }
    return v;
}

template <int WM, int WN, bool CONV, bool W2>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs a) {
    constexpr int BM = 64 * WM, BN = 64 * WN, XR = BM / 32, WR = BN / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sX = smem;
    char* sWh = smem + BM * 128;
    char* sWl = sWh + BN * 128;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int n_tiles = (a.N + BN - 1) / BN;
    const int n0 = (blockIdx.x % n_tiles) * BN;
    const int m0 = (blockIdx.x / n_tiles) * BM;
    const int c = t & 7, r0 = t >> 3;

    long xbase[XR];
    int ih0[XR], iw0[XR];
    bool xok[XR];
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int m = m0 + r0 + 32 * i;
        xok[i] = m < a.M;
        if (CONV) {
            const int per = a.g.OH * a.g.OW;
            const int img = m / per, rem = m - img * per;
            const int oh = rem / a.g.OW, ow = rem - oh * a.g.OW;
            ih0[i] = oh * a.g.SH - a.g.PH;
            iw0[i] = ow * a.g.SW - a.g.PW;
            xbase[i] = (long)img * a.g.H * a.g.W * a.g.C;
        } else {
            ih0[i] = iw0[i] = 0;
            xbase[i] = (long)m * a.lda;
        }
    }
    long wbase[WR];
    bool wok[WR];
#pragma unroll
    for (int i = 0; i < WR; ++i) {
        const int n = n0 + r0 + 32 * i;
        wok[i] = n < a.N;
        wbase[i] = (long)n * a.ldw;
    }

    uint4 xr[XR], whr[WR], wlr[WR];
    const uint4 zero4 = make_uint4(0, 0, 0, 0);

    auto load_tile = [&](int kt) {
        const int k = kt * 64 + c * 8;
        const bool kok = k < a.K;
        int kh = 0, kw = 0, ci = 0;
        if (CONV) {
            ci = k & (a.g.C - 1);
            const int kp = k >> a.g.cshift;
            tap_decode(a.g, kp, kh, kw);
        }
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            uint4 v = zero4;
            if (xok[i] && kok) {
                if (CONV) {
                    const int ih = ih0[i] + kh, iw = iw0[i] + kw;
                    if ((unsigned)ih < (unsigned)a.g.H && (unsigned)iw < (unsigned)a.g.W)
                        v = *reinterpret_cast<const uint4*>(a.A + xbase[i] + ((long)ih * a.g.W + iw) * a.g.C + ci);
                } else {
                    v = *reinterpret_cast<const uint4*>(a.A + xbase[i] + k);
                }
            }
            xr[i] = v;
        }
#pragma unroll
        for (int i = 0; i < WR; ++i) {
            const bool ok = wok[i] && kok;
            whr[i] = ok ? *reinterpret_cast<const uint4*>(a.Wh + wbase[i] + k) : zero4;
            if (W2) wlr[i] = ok ? *reinterpret_cast<const uint4*>(a.Wl + wbase[i] + k) : zero4;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            const int r = r0 + 32 * i;
            *reinterpret_cast<uint4*>(sX + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = xr[i];
        }
#pragma unroll
        for (int i = 0; i < WR; ++i) {
            const int r = r0 + 32 * i;
            const int off = r * 128 + ((c ^ ((r >> 1) & 7)) << 4);
            *reinterpret_cast<uint4*>(sWh + off) = whr[i];
            if (W2) *reinterpret_cast<uint4*>(sWl + off) = wlr[i];
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (a.K + 63) / 64;
    const int frow = lane & 15, fq = lane >> 4;
    const int fsw = (frow >> 1) & 7;   // tile row bases are multiples of 16 -> swizzle depends on lane only

    load_tile(0);
    store_tile();
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int choff = ((kk * 4 + fq) ^ fsw) << 4;
            f16x8 wf[4], wl[4], xf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wn * 64 + i * 16 + frow;
                wf[i] = *reinterpret_cast<const f16x8*>(sWh + row * 128 + choff);
                if (W2) wl[i] = *reinterpret_cast<const f16x8*>(sWl + row * 128 + choff);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wm * 64 + j * 16 + frow;
                xf[j] = *reinterpret_cast<const f16x8*>(sX + row * 128 + choff);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = JG_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
                    if (W2) acc[i][j] = JG_MFMA_16x16x32(wl[i], xf[j], acc[i][j]);
                }
        }
        __syncthreads();
        if (kt + 1 < nk) {
            store_tile();
            __syncthreads();
        }
    }

    // ---- epilogue: lane holds D[n = 4*fq + r][m = frow] of each 16x16 tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + wn * 64 + i * 16 + fq * 4;
        if (n >= a.N) continue;
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
        if (a.scale) sc = *reinterpret_cast<const f32x4*>(a.scale + n);
        if (a.bias) bi = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + wm * 64 + j * 16 + frow;
            if (m >= a.M) continue;
            f32x4 v = acc[i][j] * sc + bi;
            if (a.res) {
                const int rr = a.res_mod ? (m % a.res_mod) : m;
                v += *reinterpret_cast<const f32x4*>(a.res + (long)rr * a.ldr + n);
            }
            v = act4(v, CONV ? (a.relu != 0) : a.relu);
            if (a.out32) *reinterpret_cast<f32x4*>(a.out32 + (long)m * a.ldc + n) = v;
            if (a.out16) {
                f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
                *reinterpret_cast<f16x4*>(a.out16 + (long)m * a.ldc + n) = h;
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------
// LDS-DMA variant for the plain (Linear) GEMMs, K % 64 == 0:  tile 256(m) x 128(n) x 64(k), 8 waves
// (4 x 2, each wave 64 x 64), both operand tiles brought in by global_load_lds_dwordx4 (no VGPR
// round trip, no ds_write), two LDS stages (activations 32 KB + weights 16 KB (+16 KB lo) each).
// The LDS image is lane-linear per wave-instruction (1 KB = 8 rows x 128 B), so the XOR swizzle is
// applied to the per-lane SOURCE address and again on the fragment read (guide rule 21).
// Rows beyond M / N are clamped to the last valid row (their results are never stored).
// Workgroups that share an activation row panel (the N tiles of one M tile) are remapped onto one
// XCD so the panel is fetched into that L2 once.
// Diagnostic build only (-DJG_CLOCK_STAMPS, see conv1.hip): wave 0 of every workgroup stamps both clocks around its persistent loop.
#if defined(JG_CLOCK_STAMPS) && !defined(JG_BF16)
__device__ unsigned long long jg_clock_stamps_gemm[2 * 1024];
extern "C" int jg_clock_read_gemm(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(jg_clock_stamps_gemm), sizeof(unsigned long long) * (n < 2048 ? n : 2048)) == hipSuccess ? 0 : 1;
}
#endif
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// What an epilogue knows about the tile at hand (gemm_glds_kernel fills it in per tile, behind the k loop); GldsTile (gemm_plan.h) is the
// compile-time half: the sizes and the offsets of the scratch in LDS stage 1.
struct TileCtx {
    const GemmArgs& a;
    char* smem;               // the two LDS stages
    int wave, lane;
    int frow, fq;             // the lane's place in a 16x16 MFMA tile: it holds D[n = 4*fq + r][m = frow]
    int wm, wn;               // the wave's place in the block tile
    int cm0, cn0;             // first row / column of the tile
    int nb, mb;               // first column / row of the lane (+ i*16 / + j*16 per MFMA tile)
    int Mrows;                // rows of the launch
    bool m_full;              // the tile has all its rows: no store needs a mask
};

// scale / bias of the lane's 4 x 4 columns nb + i*16 .. +3 (1 / 0 where the vector is absent)
__device__ __forceinline__ void load_scale_bias(const float* scale, const float* bias, int nb, f32x4 (&sc)[4], f32x4 (&bi)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sc[i] = f32x4{1.f, 1.f, 1.f, 1.f};
        bi[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (scale) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[i] = *reinterpret_cast<const f32x4*>(scale + nb + i * 16);
    }
    if (bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bi[i] = *reinterpret_cast<const f32x4*>(bias + nb + i * 16);
    }
}

// ---- epi_ln_producer (XE 2): implicit-LayerNorm producer: v = acc + bias + gamma * rstd[m] * (x_prev - mean[m]); v leaves as two fp16
// planes (hi = fp16(v), the next GEMM's A operand; lo = fp16(v - hi)) through the row-transposing scratch, one plane after
// the other, plus the (sum, sum of squares) of this wave's 64 columns per row.  The residual planes are read in
// fragment order (4 x 8 B per plane and 16-row block: one 128-B line per row over the four i), one block ahead.
// registers (the 256x256 instance holds 128 accumulators): the bias goes into the accumulators up front, the row
// statistics ride with the residual prefetch, and where LDS stage 1 has room for two scratch areas per wave the lo plane
// is written to its own area next to the hi plane instead of waiting in registers
template <bool W2, int MI, int WM, int WN>
__device__ __forceinline__ void epi_ln_producer(const TileCtx& c, f32x4 (&acc)[4][MI]) {
    constexpr GldsTile T = glds_tile(W2, MI, WM, WN);
    constexpr bool LO_LDS = T.LO_LDS;
    constexpr int TP16 = T.TP16;
    static_assert(T.PROD_END <= T.STAGE, "LDS stage 1 holds the producer epilogue's scratch and gamma");
    const GemmArgs& a = c.a;
    const int wave = c.wave, lane = c.lane, frow = c.frow, fq = c.fq, wn = c.wn, cn0 = c.cn0, nb = c.nb, mb = c.mb, Mrows = c.Mrows;
    const bool m_full = c.m_full;
    const int orow_m = c.cm0 + c.wm * (16 * MI) + (lane >> 3);
    char* tsc = c.smem + T.STAGE + wave * T.PROD_WAVE;
    char* tsl = LO_LDS ? tsc + T.PROD_WAVE / 2 : tsc;
    // gamma of this wave's 64 columns waits in LDS (256 B behind the transposing scratch; one ds_read_b128 per use)
    float* gsc = reinterpret_cast<float*>(c.smem + T.STAGE + T.PROD_GSC) + wave * 64;
    gsc[lane] = a.scale[cn0 + wn * 64 + lane];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 bi = *reinterpret_cast<const f32x4*>(a.bias + nb + i * 16);
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] += bi;
    }
    wave_lds_sync();
    f16x4 rh[2][4], rl[2][4];
    f32x2_t rst[2];
    auto ldres = [&](int j) __attribute__((always_inline)) {
        const int m = mb + j * 16 < Mrows ? mb + j * 16 : Mrows - 1;
        const long o = (long)m * a.ldc + nb;
        rst[j & 1] = *reinterpret_cast<const f32x2_t*>(a.ln_stats + 2 * (long)m);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rh[j & 1][i] = *reinterpret_cast<const f16x4*>(a.xres_hi + o + i * 16);
            rl[j & 1][i] = *reinterpret_cast<const f16x4*>(a.xres_lo + o + i * 16);
        }
    };
    ldres(0);
    const long ocol = cn0 + wn * 64 + (lane & 7) * 8;
    const int sblk = (cn0 >> 6) + wn, nblk = a.N >> 6;
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        if (j + 1 < MI) ldres(j + 1);
        float s1 = 0.f, s2 = 0.f;
        f16x4 lo4[LO_LDS ? 1 : 4];
        const float mu = rst[j & 1].x, rs = rst[j & 1].y;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f16x4 xh = rh[j & 1][i], xl = rl[j & 1][i];
            const f32x4 x = {(float)xh.x + (float)xl.x, (float)xh.y + (float)xl.y, (float)xh.z + (float)xl.z, (float)xh.w + (float)xl.w};
            const f32x4 v = acc[i][j] + *reinterpret_cast<const f32x4*>(gsc + i * 16 + fq * 4) * ((x - mu) * rs);
            s1 += (v.x + v.y) + (v.z + v.w);
            s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            const f16x4 hv = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
            const f16x4 lv = {(f16)(v.x - (float)hv.x), (f16)(v.y - (float)hv.y), (f16)(v.z - (float)hv.z), (f16)(v.w - (float)hv.w)};
            *reinterpret_cast<f16x4*>(tsc + frow * TP16 + i * 32 + fq * 8) = hv;
            if (LO_LDS) *reinterpret_cast<f16x4*>(tsl + frow * TP16 + i * 32 + fq * 8) = lv;
            else lo4[i] = lv;
        }
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            if (pl == 1 && LO_LDS) break;
            if (pl == 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<f16x4*>(tsc + frow * TP16 + i * 32 + fq * 8) = lo4[LO_LDS ? 0 : i];
            }
            wave_lds_sync();
            // (its own row store, not a helper shared with epi_rows16: the shared form cost the 128x128 single-weight instance 2 VGPRs)
#pragma unroll
            for (int q2 = 0; q2 < (LO_LDS ? 2 : 1); ++q2) {
                f16* const plane = (LO_LDS ? q2 : pl) ? a.out_lo : a.out16;
                const char* src = (LO_LDS && q2) ? tsl : tsc;
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const f16x8 o = *reinterpret_cast<const f16x8*>(src + (h2 * 8 + (lane >> 3)) * TP16 + (lane & 7) * 16);
                    const long orow = orow_m + j * 16 + h2 * 8;
                    if (m_full || orow < Mrows) *reinterpret_cast<f16x8*>(plane + orow * a.ldc + ocol) = o;
                }
            }
            wave_lds_sync();
        }
        s1 += __shfl_xor(s1, 16, 64);
        s2 += __shfl_xor(s2, 16, 64);
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (fq == 0 && (m_full || mb + j * 16 < Mrows))
            *reinterpret_cast<f32x2_t*>(a.stat_out + ln_part_index(mb + j * 16, nblk, sblk)) = f32x2_t{s1, s2};
    }
}

// ---- epi_rows16: fp16-only outputs (qkv, linear1, the conv layers) are transposed through LDS so that every store
// instruction writes 8 rows x 128 contiguous bytes.  In the MFMA fragment layout a store instruction covers
// 16 rows x 32 B, and the CU's write path retires those at ~17 GB/s: 8-9 us per 256x256 tile, as long as the
// whole k loop at K = 512 (tools/store_pattern.hip, profiles/r5_gemm_timeline.txt).  The scratch is this wave's
// slice of LDS stage 1, idle until the next tile's k-tile 1 is staged (after the barrier at the loop top);
// a wave's LDS instructions execute in order, so consecutive 16-row blocks reuse the same 2.3 KB.
// XE 1: the implicit-LayerNorm consumer form, with per-row (rstd, mean) factors.  Leaves 2 MI stores per lane in flight.
// Plain instances only: the conv instances keep their form of it in the kernel body (see the ladder there).
template <bool W2, int MI, int WM, int WN, int XE>
__device__ __forceinline__ void epi_rows16(const TileCtx& c, f32x4 (&acc)[4][MI]) {
    constexpr GldsTile T = glds_tile(W2, MI, WM, WN);
    constexpr int TP16 = T.TP16;
    static_assert(T.ROWS_END <= T.STAGE, "LDS stage 1 holds the row epilogue's scratch and its per-wave table");
    const GemmArgs& a = c.a;
    const int wave = c.wave, lane = c.lane, frow = c.frow, fq = c.fq, wn = c.wn, cm0 = c.cm0, cn0 = c.cn0, nb = c.nb, mb = c.mb, Mrows = c.Mrows;
    const int orow_m = cm0 + c.wm * (16 * MI) + (lane >> 3);
    char* tsc = c.smem + T.STAGE + wave * T.ROWS_WAVE;
    // per-clip bias (GemmArgs::bias_clip; plain instances): a tile inside one clip just takes that clip's vector; a tile that
    // meets a clip boundary (one in twelve at 3150 rows per clip) picks the vector per 16-row block and lane
    const float* bias_t = a.bias;
    bool straddle = false;
    if constexpr (XE == 0) {
        if (a.bias_clip) {
            const int c0 = cm0 / a.rpc;
            straddle = (cm0 + T.BM - 1) / a.rpc != c0;
            bias_t = a.bias_clip + (long)(c0 < a.nclips ? c0 : a.nclips - 1) * a.N;
        }
    }
    f32x4 sc[4], bi[4];
    load_scale_bias(XE == 1 ? nullptr : a.scale, bias_t, nb, sc, bi);
    f16* ocol = a.out16 + cn0 + wn * 64 + (lane & 7) * 8;
    // ln_mode 1: out = rstd[m] * (acc - mean[m] * c1[n]) + bias[n], c1 (column sums of the folded weights) in GemmArgs::scale
    float xrs[XE ? MI : 1], xrm[XE ? MI : 1];
    // (registers: c1 of this wave's 64 columns waits in LDS behind the transposing scratch instead of in `sc`)
    float* gsc = reinterpret_cast<float*>(c.smem + T.STAGE + T.ROWS_TAB) + wave * 64;
    if constexpr (XE == 1) {
        gsc[lane] = a.scale[cn0 + wn * 64 + lane];
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < MI; ++j) {
            const int m = mb + j * 16 < Mrows ? mb + j * 16 : Mrows - 1;
            const f32x2_t st = *reinterpret_cast<const f32x2_t*>(a.ln_stats + 2 * (long)m);
            xrs[j] = st.y;
            xrm[j] = st.x * st.y;
        }
    }
    auto store_rows = [&](auto masked_tag, auto straddle_tag) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        constexpr bool STRADDLE = decltype(straddle_tag)::value;
#pragma unroll
        for (int j = 0; j < MI; ++j) {
            const float* bj = nullptr;
            if constexpr (STRADDLE) {
                const int cj = (mb + j * 16) / a.rpc;
                bj = a.bias_clip + (long)(cj < a.nclips ? cj : a.nclips - 1) * a.N + nb;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f32x4 v;
                if constexpr (XE == 1) v = acc[i][j] * xrs[XE ? j : 0] + (bi[i] - *reinterpret_cast<const f32x4*>(gsc + i * 16 + fq * 4) * xrm[XE ? j : 0]);
                else if constexpr (STRADDLE) v = acc[i][j] * sc[i] + *reinterpret_cast<const f32x4*>(bj + i * 16);
                else v = acc[i][j] * sc[i] + bi[i];
                v = act4(v, a.relu);
                f16x4 hv = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
                *reinterpret_cast<f16x4*>(tsc + frow * TP16 + i * 32 + fq * 8) = hv;
            }
            wave_lds_sync();
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const f16x8 o = *reinterpret_cast<const f16x8*>(tsc + (h2 * 8 + (lane >> 3)) * TP16 + (lane & 7) * 16);
                const long orow = orow_m + j * 16 + h2 * 8;
                if (!MASKED || orow_m + j * 16 + h2 * 8 < Mrows) __builtin_nontemporal_store(o, reinterpret_cast<f16x8*>(ocol + orow * a.ldc));
            }
            wave_lds_sync();
        }
    };
    if constexpr (XE == 0) {
        if (straddle) {
            if (c.m_full) store_rows(std::false_type{}, std::true_type{}); else store_rows(std::true_type{}, std::true_type{});
        } else if (c.m_full) store_rows(std::false_type{}, std::false_type{}); else store_rows(std::true_type{}, std::false_type{});
    } else {
        if (c.m_full) store_rows(std::false_type{}, std::false_type{}); else store_rows(std::true_type{}, std::false_type{});
    }
}

// MI = 16-row MFMA tiles per wave along m (4: 64x64 wave tile, 8: 128x64); WM x WN waves.
//   <4,4,2>: 256x128 block tile (hi+lo weights fit two LDS stages);  <8,2,4>: 256x256 block tile for single-fp16
//   weights -- 1.5x fewer L2->LDS bytes per FLOP, which is what bounds the 256x128 kernel once the lo MFMAs are gone.
// LNF: row-wide 128x512 tile with the residual add and the LayerNorm in the epilogue (tiled fp16 token stream).
// SPR: plain GEMM -- the next k-tile's DMA pieces are spread over the MFMA schedule (K <= 1024 instances);
//      CONV -- the loader can read the producer's left-out leading rows from a const image (ConvGeom::in_op / const_in).
// Every CONV instance honours ConvGeom::rowmap on its output side (compacted row index, row_full()).
// XE:  plain GEMM instances that also know the implicit-LayerNorm epilogues (GemmArgs::ln_mode, common.h) -- their own
//      instantiations, so that the epilogue code and its registers never reach the instances of the gesture path.
//      XE = 1: consumer (ln_mode 1), XE = 2: producer (ln_mode 2); each is compiled with that one epilogue only (no residual, no
//      tiled operand, no generic path: launch_gemm checks the shapes), which is what keeps the 256x256 instance free of spills.
// C32: conv instance for C == 32 input channels (JEGAL's second audio conv, cnn.3: 32 -> 64 channels, jegal.py:45-47): a 64-wide k-tile
//      is then TWO taps x 32 channels, so a lane's tap depends on which half of the 128-B row its 16-B chunk sits in (one select per
//      piece); with WN = 1 (N = 64) every wave stages ONE weight piece.
template <bool W2, bool CONV, int MI, int WM, int WN, bool LNF = false, bool SPR = false, int XE = 0, bool C32 = false>
__global__ __launch_bounds__(512) void gemm_glds_kernel(GemmArgs a, int n_tiles, int total_tiles, const f16* zeros, int counted_ok) {
    static_assert(WM * WN == 8, "8 waves");
    static_assert(!C32 || (CONV && !SPR && !W2), "C32: plain conv instance, single fp16 weights");
    static_assert(!LNF || (WM == 1 && !W2), "fused LayerNorm needs a row-wide tile: all 8 waves side by side along n");
    static_assert(!XE || (!CONV && !LNF), "implicit-LayerNorm epilogues: plain GEMM instances only");
    constexpr GldsTile T = glds_tile(W2, MI, WM, WN);
    constexpr int BM = T.BM, BN = T.BN, XI = T.XI, WI = T.WI, XB = T.XB, WB = T.WB, STAGE = T.STAGE, NPIECE = T.NPIECE;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int G = gridDim.x;
    const int frow = lane & 15, fq = lane >> 4;
    const int fsw = (frow >> 1) & 7;
    const int lrow = lane >> 3, pc = lane & 7;

    // CONV with ConvGeom::rowmap: the kernel runs over the COMPACTED rows m' of the launch -- per image the output rows that
    // depend on the position (common.h) -- and rowmap[m'] gives the full output row (the pixel to compute, the row the epilogue
    // stores to) and the image's count s2 in the top byte.  Mrows replaces a.M.
    int Mrows = a.M;
    const int* rmap = nullptr;
    const float inv_per = CONV ? 1.0f / (float)(a.g.OH * a.g.OW) : 0.f, inv_ow = CONV ? 1.0f / (float)a.g.OW : 0.f;
    if constexpr (CONV) {
        if (a.g.rowmap) {
            rmap = a.g.rowmap;
            Mrows = __builtin_amdgcn_readfirstlane(*a.g.rows_total);
            total_tiles = ((Mrows + BM - 1) / BM) * n_tiles;
        }
    }
    // ConvGeom::in_op / const_in (conv instances with SPR, which has no other meaning for CONV: plan_gemm picks them when
    // const_in is set): input rows 0..rin-1 of an image were left out by the producer because they do not depend on the
    // position; the loader reads them from the const image of the input instead (same pixel, other base).  rin =
    // conv_skip_decode(s2[img], in_op) is per row (it rides in the low byte of xpix).
    // Its own instances: the compare + select per LDS-DMA piece cost the 256x256 conv kernel 5 % (conv4 / conv5: 580 -> 610 us)
    // when it was compiled into all of them.
    constexpr bool ROWCONST = CONV && SPR;
    const bool rowconst = ROWCONST && rmap && a.g.const_in;
    auto row_full = [&](int m) -> long {
        if (!CONV || !rmap) return m;
        return rowmap_row(rmap[m]);
    };

    // Persistent: one workgroup per CU walks rounds of G tiles.  Within a round the workgroups of one
    // XCD (b, b+8, ...) take consecutive tile ids, so the N tiles of an activation panel share an L2.
    auto tile_of = [&](int round) -> int {
        const int v0 = round * G;
        if (v0 >= total_tiles) return -1;
        const int cnt = total_tiles - v0 < G ? total_tiles - v0 : G;
        const int b = blockIdx.x;
        if (b >= cnt) return -1;
        const int q = cnt / 8, rr = cnt % 8, xcd = b % 8, loc = b / 8;
        return v0 + (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + loc;
    };

    // per-lane LDS-DMA source state of the current tile: wave-instruction i covers tile rows
    // (wave*R + i)*8 .. +8, lane -> (row, physical 16-B chunk); the XOR swizzle is applied to the SOURCE.
    // CONV: the activation row m is an output pixel; per k-tile every lane turns its chunk's
    // k = (kh,kw,c) into an NHWC address, or into `zeros` (a zero page) for padding taps and the K
    // tail -- LDS-DMA cannot predicate, but it can read zeros.
    // CONV requires C % 64 == 0 (launch_gemm sends other layers to gemm_kernel): a 64-wide k-tile is then 64 channels
    // of ONE tap, so (kh, kw, c0) are wave-uniform and simply advance with the k-tiles (stage() is always called for
    // kt = 0, 1, 2, ... of a tile); per lane only the pointer to its (pixel, chunk) at tap (0,0) -- possibly outside
    // the image for padded layers, dereferenced only when the tap lands inside -- and the pixel coordinates remain.
    // Register budget (the 128x512 and 512x128 instances sit at the 256-VGPR limit): the pixel coordinates of a conv row and
    // its image's const-row count share one register (ih << 20 | (iw & 0xfff) << 8 | rin), and the WI weight-row pointers are two base pointers (even / odd
    // 8-row piece: the swizzled chunk depends on the piece's parity only) plus a wave-uniform multiple of 16 rows.
    const f16* xsrc[XI];
    const f16* xalt[ROWCONST ? XI : 1];          // the same pixel in the const image of the input (ROWCONST)
    int xpix[XI];
    int tidx = 0, tc0 = 0;
    static_assert(WI % 2 == 0 || WI == 1, "weight pieces come in even/odd pairs (or one piece per wave: N = 64)");
    const f16* whb[2];
    const f16* wlb[2];
    int wchunk[2];
    int n0 = 0, m0 = 0;
    auto setup = [&](int bid) {
        n0 = (bid % n_tiles) * BN;
        m0 = (bid / n_tiles) * BM;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int row = (wave * XI + i) * 8 + lrow;
            const int c = pc ^ ((row >> 1) & 7);
            int m = m0 + row;
            m = m < Mrows ? m : Mrows - 1;
            if (CONV) {
                int s2 = 0;
                if (rmap) {
                    const int e = rmap[m];
                    m = rowmap_row(e);
                    s2 = rowmap_s2(e);
                }
                // m < 2^24 (launch_gemm): quotients from float reciprocals with a +-1 fix-up instead of two integer divisions
                // (8 pieces x 2 divisions per tile and lane, and their temporaries on top of 128 live accumulators)
                const int per = a.g.OH * a.g.OW;
                int img = (int)((float)m * inv_per);
                int rem = m - img * per;
                img += rem < 0 ? -1 : (rem >= per ? 1 : 0);
                rem += rem < 0 ? per : (rem >= per ? -per : 0);
                int oh = (int)((float)rem * inv_ow);
                int ow = rem - oh * a.g.OW;
                oh += ow < 0 ? -1 : (ow >= a.g.OW ? 1 : 0);
                ow += ow < 0 ? a.g.OW : (ow >= a.g.OW ? -a.g.OW : 0);
                const int ih = oh * a.g.SH - a.g.PH, iw = ow * a.g.SW - a.g.PW;
                const int rin = rowconst ? conv_skip_decode(s2, a.g.in_op) : 0;
                // C32: the low bit says which of the k-tile's two taps this lane's chunk belongs to (chunks 4-7 = the second tap)
                xpix[i] = (ih << 20) | ((iw & 0xfff) << 8) | (C32 ? (c >> 2) : rin);      // |ih|, |iw| < 2048 (checked by launch_gemm), rin <= 19
                xsrc[i] = a.A + (long)img * a.g.H * a.g.W * a.g.C + ((long)ih * a.g.W + iw) * a.g.C + (C32 ? (c & 3) * 8 : c * 8);
                if constexpr (ROWCONST) xalt[i] = a.g.const_in + ((long)ih * a.g.W + iw) * a.g.C + c * 8;
            } else {
                xpix[i] = 0;
                // (the chunk's column offset x16t_col_off(8 c), term by term: as one sum it changes the register allocation of every plain instance)
                xsrc[i] = (!XE && a.a_tiled) ? a.A + x16t_row_off(m) + (c >> 1) * X16T_QUAD + (c & 1) * 8
                                             : a.A + (long)m * a.lda + c * 8;
            }
        }
        // N % BN == 0 (launch_gemm sends anything else to gemm_kernel): no row clamp, piece i = base[i & 1] + (i >> 1) * 16 rows
#pragma unroll
        for (int par = 0; par < 2; ++par) {
            const int row = (wave * WI + par) * 8 + lrow;
            const int c = pc ^ ((row >> 1) & 7);
            const long off = (long)(n0 + row) * a.ldw + c * 8;
            whb[par] = a.Wh + off;
            wlb[par] = W2 ? a.Wl + off : nullptr;
            wchunk[par] = c;
        }
    };
    // One k-tile = NPIECE LDS-DMA instructions per wave (XI activation pieces, then WI weight pieces, then the lo
    // weights).  stage_begin() fixes the k-tile's wave-uniform part, stage_piece<P>() issues one instruction:
    // inside the k loop the pieces are spread over the MFMA schedule (an LDS-DMA issue costs ~60 cycles between
    // MFMAs but 100-185 in a burst of eight in front of them -- MI355X_MICROARCH.md -- and during that burst the
    // matrix pipe of every SIMD idles, because all waves leave the barrier together).
    int sk0 = 0;
    long stapoff = 0;
    int stkh = 0, stkw = 0;
    bool skin = true;
    long stapoff2 = 0;           // C32: the k-tile's second tap
    int stkh2 = 0, stkw2 = 0;
    bool skin2 = false;
    auto stage_begin = [&](int kt) __attribute__((always_inline)) {
        sk0 = kt * 64;
        if constexpr (C32) {
            tap_decode(a.g, 2 * kt, stkh, stkw);
            tap_decode(a.g, 2 * kt + 1, stkh2, stkw2);
            stapoff = ((long)stkh * a.g.W + stkw) * a.g.C;
            stapoff2 = ((long)stkh2 * a.g.W + stkw2) * a.g.C;
            skin = sk0 < a.K;
            skin2 = sk0 + 32 < a.K;
        } else if (CONV) {
            if (kt == 0) tidx = tc0 = 0;
            tap_decode(a.g, tidx, stkh, stkw);
            stapoff = ((long)stkh * a.g.W + stkw) * a.g.C + tc0;
            skin = sk0 < a.K;
            tc0 += 64;
            if (tc0 == a.g.C) {
                tc0 = 0;
                ++tidx;
            }
        }
    };
    auto stage_piece = [&](int p, int buf) __attribute__((always_inline)) {      // p is a compile-time constant at every call site (unrolled loops)
        char* base = smem + buf * STAGE;
        if (p < XI) {
            const int i = p;
            const f16* src;
            if constexpr (C32) {
                const bool hb = (xpix[i] & 1) != 0;
                const int ih = (xpix[i] >> 20) + (hb ? stkh2 : stkh), iw = ((xpix[i] << 12) >> 20) + (hb ? stkw2 : stkw);
                const bool ok = (hb ? skin2 : skin) && (unsigned)ih < (unsigned)a.g.H && (unsigned)iw < (unsigned)a.g.W;
                src = ok ? xsrc[i] + (hb ? stapoff2 : stapoff) : zeros;
            } else if (CONV) {
                const int ih = (xpix[i] >> 20) + stkh, iw = ((xpix[i] << 12) >> 20) + stkw;
                const bool ok = skin && (unsigned)ih < (unsigned)a.g.H && (unsigned)iw < (unsigned)a.g.W;
                src = ok ? xsrc[i] + stapoff : zeros;
                if (ROWCONST && ok && ih < (xpix[i] & 0xff)) src = xalt[i] + stapoff;
            } else {
                src = xsrc[i] + ((!XE && a.a_tiled) ? (long)sk0 * (X16T_COLBLK / 64) : (long)sk0);        // tiled plane: a 64-wide k-tile is X16T_COLBLK elements on
            }
            // LNF, long K (linear2: 413 MB of hidden activations read once by one tile each): nontemporal (aux = 2) so
            // the stream does not push the weights out of L2.  Measured: linear2+LN 282 -> 266 us; for out_proj (K = 512,
            // its input was written by the attention kernel just before) the same hint costs 10 %.
            if (LNF && a.K >= 1024) __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(base + (wave * XI + i) * 1024), 16, 0, 2);
            else __builtin_amdgcn_global_load_lds((glb_ptr_t)src, (lds_ptr_t)(base + (wave * XI + i) * 1024), 16, 0, 0);
        } else if (p < XI + WI) {
            const int i = p - XI;
            const bool kok = !CONV || (sk0 + wchunk[i & 1] * 8 < a.K);
            const f16* wsrc = whb[i & 1] + (long)(i >> 1) * 16 * a.ldw + sk0;
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(kok ? wsrc : zeros), (lds_ptr_t)(base + XB + (wave * WI + i) * 1024), 16, 0, 0);
        } else if (W2 && p < NPIECE) {
            const int i = p - XI - WI;
            const bool kok = !CONV || (sk0 + wchunk[i & 1] * 8 < a.K);
            const f16* wsrc = wlb[i & 1] + (long)(i >> 1) * 16 * a.ldw + sk0;
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(kok ? wsrc : zeros), (lds_ptr_t)(base + XB + WB + (wave * WI + i) * 1024), 16, 0, 0);
        }
    };
    auto stage = [&](int kt, int buf) __attribute__((always_inline)) {
        stage_begin(kt);
#pragma unroll
        for (int p = 0; p < NPIECE; ++p) stage_piece(p, buf);
    };

    const int nk = (a.K + 63) / 64;
    // conv launches carry no residual (launch_gemm rejects them): the conv instances are compiled without that path -- the
    // hoisted reciprocal of its `m % res_mod` alone cost the 512x128 instance a spilled register
    const float* const ares = (CONV || XE) ? nullptr : a.res;

    int round = 0;
    int bid = tile_of(0);
    if (bid < 0) return;
    setup(bid);
    stage(0, 0);
    if (const int stagger = counted_ok >> 8) {
        // De-phase the workgroups: left alone all CUs reach their epilogue together and the store burst of a
        // whole round (G tiles) hits HBM at once while the MFMA pipes wait for it.  The highest block ids get
        // the longest delay -- they are the ones that run one tile fewer in the last round.
        const int ph = (int)(((long)blockIdx.x * 4) / G);
        if (ph) {
            const unsigned long long t0 = wall_clock64();
            while (wall_clock64() - t0 < (unsigned long long)(ph * stagger)) __builtin_amdgcn_s_sleep(16);
        }
    }
    counted_ok &= 1;
    // LNF: the accumulators start from the residual.  The token stream is the tiled fp16 plane of common.h: its raw bits
    // are loaded one tile ahead (4 x 8 B per 16-row block and lane, every access a contiguous 512 B per wave instruction)
    // and expanded to fp32 right before the k loop.
    // The raw bits of a 16-row block (4 x 8 B of fp16 = 8 registers) are parked IN the 16 accumulator registers of that
    // block, which are dead between the block's stores and the next tile's k loop:
    //   acc[0][j] = {x16 i=0 (2 regs), x16 i=3 (2 regs)},  acc[1][j].xy = x16 i=1,  acc[2][j].xy = x16 i=2.
    // (As separate arrays hipcc spilled every loaded value to scratch right behind its load.)
    f32x4 acc[4][MI];
    auto x16t_off = [&](int tm0) -> long { return (long)(tm0 / BM) * X16T_TILE + (long)wn * X16T_COLBLK + frow * 16 + fq * 4; };     // + j * X16T_ROWBLK + i * X16T_QUAD
    auto asf = [](unsigned v) -> float { return __builtin_bit_cast(float, v); };
    auto load_stream = [&](int tm0, int j) __attribute__((always_inline)) {
        const f16* xp = a.res16 + x16t_off(tm0) + j * X16T_ROWBLK;
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        // read-once stream: nontemporal, so it does not push the weights out of L2
        const u32x2 r0 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(xp)), r1 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(xp + X16T_QUAD));
        const u32x2 r2 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(xp + 2 * X16T_QUAD)), r3 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(xp + 3 * X16T_QUAD));
        acc[0][j] = f32x4{asf(r0.x), asf(r0.y), asf(r3.x), asf(r3.y)};
        acc[1][j] = f32x4{asf(r1.x), asf(r1.y), 0.f, 0.f};
        acc[2][j] = f32x4{asf(r2.x), asf(r2.y), 0.f, 0.f};
    };
    if constexpr (LNF) {
#pragma unroll
        for (int j = 0; j < MI; ++j) load_stream(m0, j);
    }
    int pending = 0;           // the k-tile-0 DMA of this tile is older than exactly `pending` epilogue stores (0: unknown)
#if defined(JG_CLOCK_STAMPS) && !defined(JG_BF16)
    const unsigned long long ck0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
#endif
    while (true) {
        // The first k-tile of this tile was issued BEFORE the previous tile's epilogue stores, so it can be
        // retired with a counted wait that leaves those stores in flight: the store burst (and its HBM
        // latency) overlaps this tile's first MFMAs instead of idling the CU.
        switch (pending) {
            case 8: wait_vmcnt<8>(); break;
            case 16: wait_vmcnt<16>(); break;
            case 24: wait_vmcnt<24>(); break;
            case 32: wait_vmcnt<32>(); break;
            case 40: wait_vmcnt<40>(); break;
            case 48: wait_vmcnt<48>(); break;
            case 56: wait_vmcnt<56>(); break;
            default: wait_vmcnt<0>(); break;
        }
        __builtin_amdgcn_s_barrier();
        const int cn0 = n0, cm0 = m0;
        // interior: the fast epilogues apply.  A tile that is only partial along M (the last row tile: M = 4800 is 18.75 tiles of
        // 256 rows) takes them too, with its stores masked by row (m_full false): the generic per-element path below costs such a
        // tile ~8 us, which is what a one-round launch of the small-M GEMMs then takes (tools/gemm_tiles.py).
        const bool m_full = cm0 + BM <= Mrows;
        const bool interior = cn0 + BN <= a.N;
        const int nb = cn0 + wn * 64 + fq * 4;
        const int mb = cm0 + wm * (16 * MI) + frow;
        // spreading the DMA pieces over the MFMA schedule, measured: -16 % on the 128x512 LN kernel (K = 2048), -5 % on the
        // conv variants, -3 % on the 256x256 Linear tile at K = 512 (SPR instance: qkv, linear1) but +3 % at K = 2048 there
        constexpr bool SPREAD = LNF || CONV || SPR;
        constexpr bool PREFETCH_RES = MI <= 4;        // 128x64 wave tiles have no registers to spare for it

        f32x4 rs[4][PREFETCH_RES ? MI : 1];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < MI; ++j) {
                if (!LNF) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (PREFETCH_RES) rs[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }

        if constexpr (LNF) {
            // expand the parked fp16 bits of this tile into fp32 accumulators (from acc[3] down: 229 instead of 246 VGPRs)
            auto unpack = [](float lo, float hi) -> f32x4 {
                const f16x2 p = __builtin_bit_cast(f16x2, lo), q = __builtin_bit_cast(f16x2, hi);
                return f32x4{(float)p.x, (float)p.y, (float)q.x, (float)q.y};
            };
#pragma unroll
            for (int j = 0; j < MI; ++j) {
                const f32x4 a0 = acc[0][j], a1 = acc[1][j], a2 = acc[2][j];
                acc[3][j] = unpack(a0.z, a0.w);
                acc[2][j] = unpack(a2.x, a2.y);
                acc[1][j] = unpack(a1.x, a1.y);
                acc[0][j] = unpack(a0.x, a0.y);
            }
        }
        // LNF: this tile's bias row(s) / gamma / beta -- one element per thread (BN == 512 threads), loaded under the LAST k-tile's MFMAs
        // and parked in LDS right behind the loop (round 5: the loads used to sit between the loop and the first statistics barrier,
        // ~1 us of L2 latency per tile).  Per-clip bias (GemmArgs::bias_clip): a 128-row tile meets at most two clips when rpc >= 128
        // (launch_gemm checks); rows from csplit on take the second clip's vector.
        float pf_b0 = 0.f, pf_b1 = 0.f, pf_g = 0.f, pf_be = 0.f;
        int csplit = 0x7fffffff;
        for (int kt = 0; kt < nk; ++kt) {
            const bool pre = kt + 1 < nk;
            if constexpr (LNF) {
                if (kt == nk - 1) {
                    const float* b0 = a.bias;
                    const float* b1 = a.bias;
                    if (a.bias_clip) {
                        const int c0 = cm0 / a.rpc;
                        b0 = a.bias_clip + (long)(c0 < a.nclips ? c0 : a.nclips - 1) * BN;
                        b1 = a.bias_clip + (long)(c0 + 1 < a.nclips ? c0 + 1 : a.nclips - 1) * BN;
                        csplit = (c0 + 1) * a.rpc;
                    }
                    pf_b0 = b0 ? b0[t] : 0.f;
                    pf_b1 = b1 ? b1[t] : 0.f;
                    pf_g = a.ln_w[t];
                    pf_be = a.ln_b[t];
                }
            }
            if (pre) stage_begin(kt + 1);
            if (pre && !SPREAD) {
#pragma unroll
                for (int p = 0; p < NPIECE; ++p) stage_piece(p, (kt + 1) & 1);
            }
            if (PREFETCH_RES && kt == nk - 1 && interior && ares) {
                // residual prefetch: issued under the last k-tile's MFMAs, consumed in the epilogue
#pragma unroll
                for (int j = 0; j < (PREFETCH_RES ? MI : 1); ++j) {
                    const int m = mb + j * 16 < Mrows ? mb + j * 16 : Mrows - 1;      // rows past M: any valid row (their results are not stored)
                    const int rr = a.res_mod ? (m % a.res_mod) : m;
                    const float* rp = ares + (long)rr * a.ldr + nb;
#pragma unroll
                    for (int i = 0; i < 4; ++i) rs[i][j] = *reinterpret_cast<const f32x4*>(rp + i * 16);
                }
            }
            const char* sX = smem + (kt & 1) * STAGE;
            const char* sWh = sX + XB;
            const char* sWl = sWh + WB;
            // Fragment schedule pinned by hand: the 4 weight fragments of a k-step, then the activation fragments
            // two ahead of the MFMAs that use them.  Left to itself hipcc hoists all 12 reads of a k-step in
            // front of one s_waitcnt lgkmcnt(0), i.e. the MFMA pipe idles for a full LDS latency four times per
            // k-tile and 48 VGPRs of fragments are live (no room to overlap anything).
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int choff = ((kk * 4 + fq) ^ fsw) << 4;
                auto ldx = [&](int j) -> f16x8 {
                    return *reinterpret_cast<const f16x8*>(sX + (wm * (16 * MI) + j * 16 + frow) * 128 + choff);
                };
                f16x8 wf[4], wl[4], xq[3];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = wn * 64 + i * 16 + frow;
                    wf[i] = *reinterpret_cast<const f16x8*>(sWh + row * 128 + choff);
                    if (W2) wl[i] = *reinterpret_cast<const f16x8*>(sWl + row * 128 + choff);
                }
                xq[0] = ldx(0);
                xq[1] = ldx(1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < MI; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        acc[i][j] = JG_MFMA_16x16x32(wf[i], xq[j % 3], acc[i][j]);
                        if (W2) acc[i][j] = JG_MFMA_16x16x32(wl[i], xq[j % 3], acc[i][j]);
                    }
                    if (j + 2 < MI) xq[(j + 2) % 3] = ldx(j + 2);
                    if (SPREAD && pre) {
                        // this slot's share of the next k-tile's DMA pieces
                        constexpr int SLOTS = 2 * MI, PER = (NPIECE + SLOTS - 1) / SLOTS;
#pragma unroll
                        for (int u = 0; u < PER; ++u) stage_piece((kk * MI + j) * PER + u, (kt + 1) & 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();     // drains the LDS-DMA of tile kt+1 (vmcnt(0)) and fences the reads of tile kt
        }

        // fp16-only outputs (qkv, linear1, the conv layers) leave through the row-transposing epilogue (epi_rows16).  Every tile has room for
        // its scratch in LDS stage 1: the epilogue asserts it, so an instance with a smaller tile fails to build instead of falling back
        // to the fragment store.
        const bool rows16 = interior && a.out16 && !a.out32 && !ares && (a.ldc & 7) == 0;
        // ConvGeom::rowmap: the full output rows of this wave's 16*MI tile rows (epi_rows16 and the fragment store stay inside them) go
        // through a per-wave table in LDS -- 1-2 loads per lane, in front of the next tile's setup and OLDER than its first DMA,
        // so nothing in the epilogue waits for that DMA.  (Sixteen row indices per lane in registers spilled the 512x128 and
        // the ROWCONST instances, and so did two values kept live across setup().)  The table sits behind
        // the transposing epilogue's scratch in LDS stage 1 (GldsTile::ROWS_TAB), which is idle until the next tile's k-tile 1 is staged.
        constexpr int WROWS = 16 * MI;
        // (per-lane table addresses are recomputed from a laundered lane id per tile: hoisted out of the persistent loop as
        // invariants they cost the 512x128 instance four spilled registers)
        int lane_t = lane;
        if constexpr (CONV) asm volatile("" : "+v"(lane_t));
        int* rtab = reinterpret_cast<int*>(smem + STAGE + T.ROWS_TAB) + wave * 128;
        const bool use_rtab = CONV && rmap && interior;
        if constexpr (CONV) {
            if (use_rtab) {
                const int wrow0 = cm0 + wm * WROWS;
                // (rows past Mrows of an M-partial tile: clamped -- their stores are masked, but the read must stay inside the map)
                const int i0 = wrow0 + lane_t < Mrows ? wrow0 + lane_t : Mrows - 1, i1 = wrow0 + 64 + lane_t < Mrows ? wrow0 + 64 + lane_t : Mrows - 1;
                if (WROWS >= 64 || lane_t < WROWS) rtab[lane_t] = rowmap_row(rmap[i0]);
                if (WROWS > 64) rtab[64 + lane_t] = rowmap_row(rmap[i1]);
                wave_lds_sync();
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // next tile: issue its first k-tile now, BEFORE the epilogue's stores (LNF: inside its epilogue, see there)
        const int nbid = tile_of(++round);
        if (nbid >= 0) setup(nbid);
        __builtin_amdgcn_sched_barrier(0);
        if (nbid >= 0 && !LNF) stage(0, 0);
        __builtin_amdgcn_sched_barrier(0);       // keep the DMA older than the stores (the counted wait relies on it)

        if constexpr (LNF) {
            // ---- fused residual + LayerNorm epilogue (gestsync.py:20: LN(x + sublayer(x)), eps 1e-5).
            // The tile spans the whole row (BN == N == 512, wave wn owns columns wn*64..+63): row statistics are a
            // shuffle over the 4 lanes of a row inside the wave plus an 8-way exchange through LDS (stage 1 is idle
            // here).  Two-pass (mean, then centred variance) like nn.LayerNorm.
            // Input and output token stream: the tiled fp16 plane (common.h) in this kernel's own fragment
            // order, normally in place.  As soon as the 16-row block j of this tile has been stored, the raw bits of
            // block j of the NEXT tile are loaded (no spare registers are needed for a whole tile of residual, the
            // HBM latency hides behind the rest of the epilogue); that tile's first DMA goes in front of block JD and
            // is retired with a counted wait.  Whole 128-row tiles are written: the planes hold ceil(M/128)*128 rows.
            // bias / gamma / beta come from LDS (3 x 512 floats, re-staged per tile: the k loop owns the LDS).
            constexpr int JD = JG_LNF_JD;                                 // row block in front of which the next tile's DMA goes (default 2)
            static_assert(T.LN_END <= STAGE, "LDS stage 1 holds the LayerNorm epilogue's statistics and parameters");
            float* red = reinterpret_cast<float*>(smem + STAGE + T.LN_RED);        // [2][8 waves][BM rows]
            float* lnp = reinterpret_cast<float*>(smem + STAGE + T.LN_PAR);        // [4][BN]: bias, gamma, beta, bias of the tile's second clip
            static_assert(BN == 512, "one parked element per thread");
            lnp[t] = pf_b0;
            lnp[BN + t] = pf_g;
            lnp[2 * BN + t] = pf_be;
            lnp[3 * BN + t] = pf_b1;
            __syncthreads();
            const int ncol = wn * 64 + fq * 4;                            // + i*16: this lane's 4 columns of block i
            float rsum[MI];
#pragma unroll
            for (int j = 0; j < MI; ++j) {
                float sj = 0.f;
                const float* bsel = lnp + (cm0 + j * 16 + frow >= csplit ? 3 * BN : 0) + ncol;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v = acc[i][j] + *reinterpret_cast<const f32x4*>(bsel + i * 16);
                    acc[i][j] = v;
                    sj += (v.x + v.y) + (v.z + v.w);
                }
                sj += __shfl_xor(sj, 16, 64);
                sj += __shfl_xor(sj, 32, 64);
                rsum[j] = sj;
            }
            if (fq == 0) {
#pragma unroll
                for (int j = 0; j < MI; ++j) red[wn * BM + j * 16 + frow] = rsum[j];
            }
            __syncthreads();
            float rsq[MI];
#pragma unroll
            for (int j = 0; j < MI; ++j) {
                float tsum = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) tsum += red[w * BM + j * 16 + frow];
                const float mean = tsum * (1.f / BN);
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 d = acc[i][j] - mean;
                    acc[i][j] = d;
                    q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
                }
                q += __shfl_xor(q, 16, 64);
                q += __shfl_xor(q, 32, 64);
                rsq[j] = q;
            }
            if (fq == 0) {
#pragma unroll
                for (int j = 0; j < MI; ++j) red[(8 + wn) * BM + j * 16 + frow] = rsq[j];
            }
            __syncthreads();
            f16* o16 = a.out16 + x16t_off(cm0);
#pragma unroll
            for (int j = 0; j < MI; ++j) {
                if (j == JD) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (nbid >= 0) stage(0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                float tq = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) tq += red[(8 + w) * BM + j * 16 + frow];
                const float inv = a.ln_flavour == LN_STD ? 1.f / sqrtf(tq * (1.f / BN) + 1e-5f)
                                                         : 1.f / (sqrtf(tq * (1.f / (BN - 1))) + 1e-6f);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 y = acc[i][j] * inv * *reinterpret_cast<const f32x4*>(lnp + BN + ncol + i * 16) +
                                    *reinterpret_cast<const f32x4*>(lnp + 2 * BN + ncol + i * 16);
                    const f16x4 hv = {(f16)y.x, (f16)y.y, (f16)y.z, (f16)y.w};
                    *reinterpret_cast<f16x4*>(o16 + j * X16T_ROWBLK + i * X16T_QUAD) = hv;
                }
                if (nbid >= 0) load_stream(m0, j);                        // m0 is already the next tile's
            }
            if (nbid < 0) break;
            // the loop-top barrier fences red[] / lnp[] against the next tile's k-tile 1 (staged after it)
            pending = counted_ok ? (MI - JD) * 8 : 0;
            continue;
        }
        // ---- the other epilogues, one flat ladder: lane holds D[n = 4*fq + r][m = frow] of each 16x16 tile.  The XE instances are
        // compiled with their one epilogue (launch_gemm checks the shapes).  epi_ln_producer and epi_rows16 are functions above the
        // kernel.  Written out here, each because as a __forceinline__ function it cost instances registers (the figures per instance:
        // profiles/gemm_glds_split_isa.md): the fragment store and the generic path (VGPRs, one spill), the LayerNorm epilogue above
        // (16 VGPRs), the k loop (1 VGPR nearly everywhere, a peeled last iteration), and `pending` as one expression at the bottom.
        // Fragment store: ALL residual / scale / bias loads are issued first, then
        // the math, then all stores.  (Per-element `if (m < M) load` made hipcc branch around every load
        // and wait vmcnt(0) after each one: 16 serial HBM round trips per tile, 1/3 of the Linear time.)
        const TileCtx c = {a, smem, wave, lane, frow, fq, wm, wn, cm0, cn0, nb, mb, Mrows, m_full};
        if constexpr (XE == 2) {
            epi_ln_producer<W2, MI, WM, WN>(c, acc);
        } else if (XE == 1 || rows16) {
            if constexpr (!CONV) {
                epi_rows16<W2, MI, WM, WN, XE>(c, acc);
            } else {
                // the conv form of epi_rows16 (ReLU only, output rows through rtab), written out: as a call it cost three conv instances 1-2 SGPR spills
                static_assert(T.ROWS_END <= STAGE, "LDS stage 1 holds the row epilogue's scratch and its per-wave table");
                constexpr int TP16 = T.TP16;
                char* tsc = smem + STAGE + wave * T.ROWS_WAVE;
                const int orow_m = cm0 + wm * (16 * MI) + (lane >> 3);
                f32x4 sc[4], bi[4];
                load_scale_bias(a.scale, a.bias, nb, sc, bi);
                f16* ocol = a.out16 + cn0 + wn * 64 + (lane & 7) * 8;
                auto store_rows = [&](auto masked_tag) __attribute__((always_inline)) {
                    constexpr bool MASKED = decltype(masked_tag)::value;
#pragma unroll
                    for (int j = 0; j < MI; ++j) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            f32x4 v = acc[i][j] * sc[i] + bi[i];
                            v = act4(v, a.relu != 0);
                            f16x4 hv = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
                            *reinterpret_cast<f16x4*>(tsc + frow * TP16 + i * 32 + fq * 8) = hv;
                        }
                        wave_lds_sync();
#pragma unroll
                        for (int h2 = 0; h2 < 2; ++h2) {
                            const f16x8 o = *reinterpret_cast<const f16x8*>(tsc + (h2 * 8 + (lane >> 3)) * TP16 + (lane & 7) * 16);
                            const long orow = use_rtab ? rtab[j * 16 + h2 * 8 + (lane_t >> 3)] : orow_m + j * 16 + h2 * 8;
                            if (!MASKED || orow_m + j * 16 + h2 * 8 < Mrows) __builtin_nontemporal_store(o, reinterpret_cast<f16x8*>(ocol + orow * a.ldc));
                        }
                        wave_lds_sync();
                    }
                };
                if (m_full) store_rows(std::false_type{}); else store_rows(std::true_type{});
            }
        } else if (interior) {
            // (its own scale / bias block: with load_scale_bias hipcc laid the plain instances' store paths out with one more global store)
            f32x4 sc[4], bi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sc[i] = f32x4{1.f, 1.f, 1.f, 1.f};
                bi[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (a.scale) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sc[i] = *reinterpret_cast<const f32x4*>(a.scale + nb + i * 16);
            }
            if (a.bias) {
#pragma unroll
                for (int i = 0; i < 4; ++i) bi[i] = *reinterpret_cast<const f32x4*>(a.bias + nb + i * 16);
            }
            auto store_frag = [&](auto masked_tag) __attribute__((always_inline)) {
                constexpr bool MASKED = decltype(masked_tag)::value;
#pragma unroll
                for (int j = 0; j < MI; ++j) {
                    const long mo = (use_rtab ? (long)rtab[j * 16 + (lane_t & 15)] : (long)(mb + j * 16)) * a.ldc + nb;
                    f32x4 rj[4];
                    if (!PREFETCH_RES) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) rj[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (ares) {
                            const int m = !MASKED || mb + j * 16 < Mrows ? mb + j * 16 : Mrows - 1;
                            const int rr = a.res_mod ? (m % a.res_mod) : m;
                            const float* rp = ares + (long)rr * a.ldr + nb;
#pragma unroll
                            for (int i = 0; i < 4; ++i) rj[i] = *reinterpret_cast<const f32x4*>(rp + i * 16);
                        }
                    }
                    if (MASKED && mb + j * 16 >= Mrows) continue;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f32x4 v = acc[i][j] * sc[i] + bi[i] + (PREFETCH_RES ? rs[i][j] : rj[i]);
                        v = act4(v, CONV ? (a.relu != 0) : a.relu);
                        if (a.out32) *reinterpret_cast<f32x4*>(a.out32 + mo + i * 16) = v;
                        if (a.out16) {
                            f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
                            *reinterpret_cast<f16x4*>(a.out16 + mo + i * 16) = h;
                        }
                    }
                }
            };
            if (m_full) store_frag(std::false_type{}); else store_frag(std::true_type{});
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = cn0 + wn * 64 + i * 16 + fq * 4;
                if (n >= a.N) continue;
                f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
                if (a.scale) sc = *reinterpret_cast<const f32x4*>(a.scale + n);
                if (a.bias) bi = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
                for (int j = 0; j < MI; ++j) {
                    const int m = cm0 + wm * (16 * MI) + j * 16 + frow;
                    if (m >= Mrows) continue;
                    const long mf = row_full(m);
                    f32x4 v = acc[i][j] * sc + bi;
                    if (ares) {
                        const int rr = a.res_mod ? (m % a.res_mod) : m;
                        v += *reinterpret_cast<const f32x4*>(ares + (long)rr * a.ldr + n);
                    }
                    v = act4(v, CONV ? (a.relu != 0) : a.relu);
                    if (a.out32) *reinterpret_cast<f32x4*>(a.out32 + mf * a.ldc + n) = v;
                    if (a.out16) {
                        f16x4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
                        *reinterpret_cast<f16x4*>(a.out16 + mf * a.ldc + n) = h;
                    }
                }
            }
        }
        if (nbid < 0) break;
        pending = !(interior && m_full && counted_ok) || XE == 2 ? 0 : rows16 ? 2 * MI : (a.out32 ? 4 * MI : 0) + (a.out16 ? 4 * MI : 0);
    }
#if defined(JG_CLOCK_STAMPS) && !defined(JG_BF16)
    if (wave == 0 && lane == 0 && blockIdx.x < 1024) {
        jg_clock_stamps_gemm[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - ck0;
        jg_clock_stamps_gemm[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - rt0;
    }
#endif
}

// ---- host side: the launch thunks and launch_gemm.  Every tuning switch and per-device resource lives in the caller's EngineOpts
// (one per jg_handle): nothing here is process-global except the "dynamic LDS attribute set" flags, which are per (kernel instance,
// device).  The choice of the instance is the planner's (gemm_plan.hip).
constexpr int MAX_DEV = 64;

// One launch thunk per entry of the instance table (gemm_plan.h): it owns the instance's "dynamic LDS attribute set" flags and
// launches with the plan's figures.  Nothing is chosen here.
using GemmThunk = hipError_t (*)(const GemmArgs&, const GemmPlan&, const EngineOpts&, hipStream_t);

template <bool W2, bool CONV, int MI, int WM, int WN, bool LNF, bool SPR, int XE, bool C32>
static hipError_t run_glds(const GemmArgs& a, const GemmPlan& p, const EngineOpts& o, hipStream_t s) {
    static bool attr_set[MAX_DEV] = {};
    if (o.device < 0 || o.device >= MAX_DEV) return hipErrorInvalidDevice;
    if (!attr_set[o.device]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_glds_kernel<W2, CONV, MI, WM, WN, LNF, SPR, XE, C32>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
        attr_set[o.device] = true;
    }
    if (!o.zeros) return hipErrorInvalidValue;
    record_kernel(p.name);
    hipLaunchKernelGGL((gemm_glds_kernel<W2, CONV, MI, WM, WN, LNF, SPR, XE, C32>), dim3(p.grid), dim3(512), p.lds, s, a, p.n_tiles, p.total_tiles,
                       static_cast<const f16*>(o.zeros), o.gemm_counted | (p.stagger << 8));
    return hipGetLastError();
}

template <int WM, int WN, bool CONV, bool W2>
static hipError_t run_staged(const GemmArgs& a, const GemmPlan& p, const EngineOpts& o, hipStream_t s) {
    record_kernel(p.name);
    hipLaunchKernelGGL((gemm_kernel<WM, WN, CONV, W2>), dim3(p.grid), dim3(256), p.lds, s, a);
    return hipGetLastError();
}

static constexpr GemmThunk GEMM_THUNKS[] = {
#define X(W2, CONV, MI, WM, WN, LNF, SPR, XE, C32) run_glds<W2, CONV, MI, WM, WN, LNF, SPR, XE, C32>,
    JG_GEMM_GLDS_INSTANCES(X)
#undef X
#define X(WM, WN, CONV, W2) run_staged<WM, WN, CONV, W2>,
    JG_GEMM_STAGED_INSTANCES(X)
#undef X
};
static_assert(sizeof(GEMM_THUNKS) / sizeof(GEMM_THUNKS[0]) == GEMM_NUM_INSTANCES, "one thunk per table entry");

// shape of the arguments -> plan (gemm_plan.hip: every rule lives there) -> the table
hipError_t launch_gemm(const GemmArgs& a, bool conv, const EngineOpts& o, hipStream_t s) {
    if (a.M <= 0) return hipSuccess;
    const GemmPlan p = plan_gemm(gemm_shape(a, conv), o);
    if (!p.ok()) return hipErrorInvalidValue;
    return GEMM_THUNKS[p.instance](a, p, o, s);
}

JG_NS_END
