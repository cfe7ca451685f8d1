// Self-attention for short sequences (gfx950).  softmax(q k^T / sqrt(dk) [masked_fill(mask==0,-1e9)]) v
//   gestsync.py:20-21 (nn.MultiheadAttention, S = 21, no mask), modules.py:61-75 (S = T <= 500 or
//   L text tokens, key-padding mask).  Attention is < 5 % of the path's FLOPs and HBM-bound (it reads the
//   packed qkv rows once and writes the context rows once), so every kernel is organised around the
//   memory and LDS pipes.  Reading order of this file:
//     attn_kernel<DK>        option attn_mfma = 0 only (A/B, tests): VALU kernel, one lane per
//                            query row, K/V rows in LDS read as wave-wide broadcasts, v_dot2_f32_f16, online softmax
//                            over blocks of 8 keys, fp32 state.  For S <= 32 one wave carries floor(64/S) (sequence, head) pairs.
//     the parts of the MFMA kernels, each written once: the accumulator layout (mfma32_row), the loads and the LDS images
//                            (load16, stage_row, stage_vt, stage_kv, stage_mask, operand_frag, load_q_operand), the score
//                            tile and its masking (score_tile, mask_scale_tile, exp_sum_tile), P.V from the score
//                            accumulators (split_hi_lo + pv_mfma = pv_step) and the output path (store_rows).
//     the three MFMA kernels as compositions of them; launch_attention() picks one:
//     attn_mfma_s32_kernel   S <= 32, dk = 64, no mask (the GestSync windows, S = 21): one wave per (window, head),
//                            all three operands through the wave's own LDS slice, one score tile.
//     attn_mfma_kernel<NB>   S <= 160, dk = 64, optional key mask (JEGAL gesture encoder at the dataset's clip lengths):
//                            one workgroup per (clip, head), K and V^T staged in LDS once, one wave per 32 queries.
//     attn_mfma_flash_kernel<DK>  everything else (dk = 64 with S > 160: long clips, XLM-RoBERTa at L > 160; dk = 96: the text
//                            encoder): key chunks of 128 through LDS, online softmax.
#include "common.h"

JG_NS_BEGIN

template <int DK>
__global__ __launch_bounds__(256) void attn_kernel(const f16* __restrict__ qkv, const float* __restrict__ keymask,
                                                   int B, int S, int H, int G, f16* __restrict__ out) {
    constexpr int NV = DK / 8;            // 16-byte vectors per head row
    __shared__ __attribute__((aligned(16))) f16 sK[64 * DK];
    __shared__ __attribute__((aligned(16))) f16 sV[64 * DK];
    __shared__ float sM[64];

    const int D = H * DK;
    const long ld = 3L * D;
    const int tid = threadIdx.x;
    const bool small = G > 1 || blockDim.x == 64;
    const long npairs = (long)B * H;

    long pair;            // (b,h) of this lane's query
    int qi;               // query index inside the sequence
    int kbase;            // first LDS row of this lane's keys (small mode)
    bool active;
    if (small) {
        const int g = tid / S;
        pair = (long)blockIdx.x * G + g;
        qi = tid - g * S;
        kbase = g * S;
        active = g < G && pair < npairs;
    } else {
        pair = blockIdx.x;
        qi = blockIdx.y * blockDim.x + tid;
        kbase = 0;
        active = qi < S;
    }
    const int b = active ? (int)(pair / H) : 0, h = active ? (int)(pair % H) : 0;

    f16x2 q[DK / 2];
    float o[DK];
#pragma unroll
    for (int d = 0; d < DK; ++d) o[d] = 0.f;
    if (active) {
        const f16* qp = qkv + ((long)b * S + qi) * ld + h * DK;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const f16x8 t8 = *reinterpret_cast<const f16x8*>(qp + v * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) q[v * 4 + e] = f16x2{t8[2 * e], t8[2 * e + 1]};
        }
    } else {
#pragma unroll
        for (int d = 0; d < DK / 2; ++d) q[d] = f16x2{(f16)0.f, (f16)0.f};
    }
    const float scale = 1.0f / sqrtf((float)DK);
    float mrun = -INFINITY, lrun = 0.f;

    const int nchunks = small ? 1 : (S + 63) / 64;
    for (int ch = 0; ch < nchunks; ++ch) {
        // ---- stage K/V rows (and their mask) of this chunk
        const int rows = small ? G * S : min(64, S - ch * 64);
        __syncthreads();
        for (int idx = tid; idx < rows * NV; idx += blockDim.x) {
            const int r = idx / NV, v = idx - r * NV;
            long p2;
            int j;
            if (small) { const int g = r / S; p2 = (long)blockIdx.x * G + g; j = r - g * S; }
            else { p2 = pair; j = ch * 64 + r; }
            uint4 kk = make_uint4(0, 0, 0, 0), vv = kk;
            if (p2 < npairs) {
                const int b2 = (int)(p2 / H), h2 = (int)(p2 % H);
                const f16* base = qkv + ((long)b2 * S + j) * ld + h2 * DK + v * 8;
                kk = *reinterpret_cast<const uint4*>(base + D);
                vv = *reinterpret_cast<const uint4*>(base + 2 * D);
            }
            *reinterpret_cast<uint4*>(&sK[r * DK + v * 8]) = kk;
            *reinterpret_cast<uint4*>(&sV[r * DK + v * 8]) = vv;
        }
        for (int r = tid; r < rows; r += blockDim.x) {
            long p2;
            int j;
            if (small) { const int g = r / S; p2 = (long)blockIdx.x * G + g; j = r - g * S; }
            else { p2 = pair; j = ch * 64 + r; }
            float mk = 1.f;
            if (keymask && p2 < npairs) mk = keymask[(p2 / H) * S + j];
            sM[r] = mk;
        }
        __syncthreads();

        const int nkeys = small ? S : rows;
        for (int j0 = 0; j0 < nkeys; j0 += 8) {
            float sc[8];
            float bmax = -INFINITY;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u;
                float acc = 0.f;
                if (j < nkeys) {
                    const f16* kr = &sK[(kbase + j) * DK];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const f16x8 k8 = *reinterpret_cast<const f16x8*>(kr + v * 8);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#ifdef JG_BF16
                            acc = __builtin_fmaf((float)q[v * 4 + e].x, (float)k8[2 * e], __builtin_fmaf((float)q[v * 4 + e].y, (float)k8[2 * e + 1], acc));
#else
                            acc = __builtin_amdgcn_fdot2(q[v * 4 + e], f16x2{k8[2 * e], k8[2 * e + 1]}, acc, false);
#endif
                    }
                    acc *= scale;
                    if (sM[kbase + j] == 0.f) acc = -1e9f;
                } else {
                    acc = -INFINITY;
                }
                sc[u] = acc;
                bmax = fmaxf(bmax, acc);
            }
            const float mnew = fmaxf(mrun, bmax);
            const float alpha = __expf(mrun - mnew);     // first block: exp(-inf) = 0
            lrun *= alpha;
#pragma unroll
            for (int d = 0; d < DK; ++d) o[d] *= alpha;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u;
                if (j < nkeys) {
                    const float p = __expf(sc[u] - mnew);
                    lrun += p;
                    const f16* vr = &sV[(kbase + j) * DK];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const f16x8 v8 = *reinterpret_cast<const f16x8*>(vr + v * 8);
#pragma unroll
                        for (int e = 0; e < 8; ++e) o[v * 8 + e] += p * (float)v8[e];
                    }
                }
            }
            mrun = mnew;
        }
    }
    if (active) {
        const float inv = 1.f / lrun;
        f16* op = out + ((long)b * S + qi) * D + h * DK;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            f16x8 t8;
#pragma unroll
            for (int e = 0; e < 8; ++e) t8[e] = (f16)(o[v * 8 + e] * inv);
            *reinterpret_cast<f16x8*>(op + v * 8) = t8;
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Parts of the MFMA kernels.  All three compute, on v_mfma_f32_32x32x16 tiles,
//   S^T = K Q^T   (keys x queries): K rows are the A operand, Q rows the B operand (lane = row, 16 B = 8 consecutive d);
//   softmax over the keys of a query = over the accumulator registers of a lane and its partner lane+32;
//   O^T = V^T P^T (d x queries): P^T is ALREADY in B-operand order in the S^T accumulators (pv_step), V^T comes from a
//                 transposed copy of the head's V rows in LDS, read in the same key order;
//   and transpose the output tile back through LDS so the stores are whole rows (store_rows).
// A lane is (r31 = lane & 31, hh = lane >> 5): r31 is the row of an operand and the column (the query) of an accumulator
// tile, hh the half of a k-step's 16 values it holds.  Rows beyond S are clamped on load (finite values), masked to -inf as
// keys and never stored as queries.

// THE accumulator layout of the 32x32x16 tile: register i of a lane in half hh holds row mfma32_row(i, hh) of the lane's column --
// a key of a score tile, a d of an output block.  Registers 4g .. 4g+3 are the four consecutive rows from mfma32_row(4g, hh).

template <int N>
__device__ __forceinline__ void zero_tiles(f32x16 (&t)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) t[n][i] = 0.f;
}

// 16 bytes (8 d) of a q / k / v row.  NT = nontemporal: for a stream that its kernel reads exactly once (the kernels say why).
template <bool NT>
__device__ __forceinline__ f16x8 load16(const f16* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const f16x8*>(p));
    else return *reinterpret_cast<const f16x8*>(p);
}

// One 16-byte chunk of a K, Q or output row in a row-major LDS image.
template <int PITCH>
__device__ __forceinline__ f16x8* row_chunk(char* img, int row, int part) { return reinterpret_cast<f16x8*>(img + row * PITCH + part * 16); }
template <int PITCH>
__device__ __forceinline__ void stage_row(char* img, int row, int part, f16x8 v) { *row_chunk<PITCH>(img, row, part) = v; }
// One 16-byte chunk of V row `row` into the transposed image [d][key] (pv_step reads four consecutive keys of a d).
template <int PITCH>
__device__ __forceinline__ void stage_vt(char* sVt, int row, int part, f16x8 v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) *reinterpret_cast<f16*>(sVt + (part * 8 + e) * PITCH + row * 2) = v[e];
}
// The K and V chunks of one row (src = its q chunk) from global memory into the two images.
template <bool NT, int K_PITCH, int VT_PITCH>
__device__ __forceinline__ void stage_kv(const f16* src, int D, char* sK, char* sVt, int row, int part) {
    const f16x8 kk = load16<NT>(src + D);
    const f16x8 vv = load16<NT>(src + 2 * D);
    stage_row<K_PITCH>(sK, row, part, kk);
    stage_vt<VT_PITCH>(sVt, row, part, vv);
}
// The mask row of keys k0 .. k0 + n - 1 for mask_scale_tile: the key mask's value (1 without a mask), -1 beyond S.
__device__ __forceinline__ void stage_mask(float* sM, int n, const float* keymask, long b, int k0, int S, int tid, int NT) {
    for (int j = tid; j < n; j += NT) sM[j] = k0 + j < S ? (keymask ? keymask[b * S + k0 + j] : 1.f) : -1.f;
}

// A or B operand of k-step s (d = 16s + 8hh ..) from row `row` of a row-major LDS image / of a Q row in global memory.
template <int PITCH>
__device__ __forceinline__ f16x8 operand_frag(const char* img, int row, int s, int hh) {
    return *reinterpret_cast<const f16x8*>(img + row * PITCH + (16 * s + 8 * hh) * 2);
}
template <int KS>
__device__ __forceinline__ void load_q_operand(f16x8 (&qB)[KS], const f16* qrow, int hh) {
#pragma unroll
    for (int s = 0; s < KS; ++s) qB[s] = *reinterpret_cast<const f16x8*>(qrow + 16 * s + 8 * hh);
}

// One score tile: keys 32kb .. 32kb+31 of the K image x this wave's 32 queries.
template <int KS, int PITCH>
__device__ __forceinline__ f32x16 score_tile(const char* sK, int kb, const f16x8 (&qB)[KS], int r31, int hh) {
    f32x16 sc;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[i] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) sc = JG_MFMA_32x32x16(operand_frag<PITCH>(sK, 32 * kb + r31, s, hh), qB[s], sc);
    return sc;
}
// Scale a score tile and apply its mask row sMt (stage_mask): < 0 (beyond S) -> -inf, == 0 -> -1e9 (masked_fill(mask == 0, -1e9),
// modules.py:66-67); mx = running max.
__device__ __forceinline__ void mask_scale_tile(f32x16& sc, const float* sMt, int hh, float scale, float& mx) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 mk = *reinterpret_cast<const f32x4*>(&sMt[mfma32_row(4 * g, hh)]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = sc[4 * g + e] * scale;
            v = mk[e] < 0.f ? -INFINITY : (mk[e] == 0.f ? -1e9f : v);
            sc[4 * g + e] = v;
            mx = fmaxf(mx, v);
        }
    }
}
// sc = exp(sc - mx) (exp(-inf) = 0 for the keys beyond S), sum += its registers.
__device__ __forceinline__ void exp_sum_tile(f32x16& sc, float mx, float& sum) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        sc[i] = __expf(sc[i] - mx);
        sum += sc[i];
    }
}

// O^T += V^T P^T, one k-step (s = 0, 1: 16 keys) of a tile of probabilities at a time.  The operand trick: registers 8s .. 8s+7
// of a lane ARE the B fragment of k-step s (lane = query), in the permuted key order mfma32_row(8s + j, hh).
// split_hi_lo: that fragment as 16-bit hi + lo (two MFMAs per block of 32 d): the probabilities keep fp32 accuracy, as in the
// VALU kernel, and the matrix pipe has nothing else to do.  NORM: times inv = 1 / sum first (kernels that know the sum by now).
template <bool NORM>
__device__ __forceinline__ void split_hi_lo(const f32x16& sc, int s, f16x8& pH, f16x8& pL, float inv = 0.f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float pv = NORM ? sc[8 * s + j] * inv : sc[8 * s + j];
        const f16 hi = (f16)pv;
        pH[j] = hi;
        pL[j] = (f16)(pv - (float)hi);
    }
}
// pv_mfma: the two MFMAs of one block of 32 d (row = this lane's d).  V^T is read in the fragment's key order: four keys from
// key0 + mfma32_row(8s, hh) and the four 8 further on (mfma32_row(8s + 4, hh)); key0 = the tile's first key in the V^T image.
template <int PITCH>
__device__ __forceinline__ void pv_mfma(f16x8 pH, f16x8 pL, int s, const char* sVt, int key0, int row, int hh, f32x16& o) {
    const char* vp = sVt + row * PITCH + (key0 + mfma32_row(8 * s, hh)) * 2;
    const f16x4 v0 = *reinterpret_cast<const f16x4*>(vp), v1 = *reinterpret_cast<const f16x4*>(vp + 16);
    const f16x8 vA = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    o = JG_MFMA_32x32x16(vA, pH, o);
    o = JG_MFMA_32x32x16(vA, pL, o);
}
// pv_step: both, for the NBLK blocks of a head.
template <int NBLK, int PITCH, bool NORM>
__device__ __forceinline__ void pv_step(const f32x16& sc, int s, const char* sVt, int key0, int r31, int hh, f32x16 (&o)[NBLK], float inv = 0.f) {
    f16x8 pH, pL;
    split_hi_lo<NORM>(sc, s, pH, pL, inv);
#pragma unroll
    for (int blk = 0; blk < NBLK; ++blk) pv_mfma<PITCH>(pH, pL, s, sVt, key0, r31 + 32 * blk, hh, o[blk]);
}

// Output path: the accumulator blocks o (register i of block blk <-> d = 32 blk + mfma32_row(i, hh), lane <-> query) -> [query][d]
// 16-bit rows in the wave's LDS slice sO -> whole-row stores to obase[row][..] for the rows with q0 + row < S.  PASS blocks
// (32 PASS columns) go through the slice at a time; NORM folds inv = 1 / sum into the conversion; rows >= OR do not exist in
// the slice (OR = 32: all do).  The wave's LDS operations execute in order; the wave_lds_sync()s keep the compiler to it.
template <int NBLK, int PASS, int PITCH, int OR, bool NORM>
__device__ __forceinline__ void store_rows(const f32x16 (&o)[NBLK], char* sO, f16* obase, int D, int q0, int S, int lane, float inv = 0.f) {
    const int r31 = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int b0 = 0; b0 < NBLK; b0 += PASS) {
#pragma unroll
        for (int blk = 0; blk < PASS; ++blk)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f16x4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (f16)(NORM ? o[b0 + blk][4 * g + e] * inv : o[b0 + blk][4 * g + e]);
                if (OR == 32 || r31 < OR) *reinterpret_cast<f16x4*>(sO + r31 * PITCH + (32 * blk + mfma32_row(4 * g, hh)) * 2) = hv;
            }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 2 * PASS; ++r) {
            const int c = lane + 64 * r, row = c / (4 * PASS), part = c % (4 * PASS);
            if (q0 + row < S) *reinterpret_cast<f16x8*>(obase + (long)row * D + 32 * b0 + part * 8) = *row_chunk<PITCH>(sO, row, part);
        }
        if (PASS < NBLK) wave_lds_sync();           // the next pass overwrites the slice
    }
}


// ---------------------------------------------------------------------------------------------
// MFMA kernel for the GestSync layers: S <= 32 keys, dk = 64, no mask (keys are masked by key < S: one score tile, no mask
// row).  One wave per (sequence, head) pair, four independent waves per workgroup (no workgroup barrier); 1 / sum goes into
// the probabilities before the hi + lo split.
// GATHER (layer 0 of the GestSync transformer, AttnGather in common.h): token j of window (clip c, frame i) is
//   x = conv[c][clamp(i + j - shift)] + pe[j],  so its projection is  W x + b = (W conv[c][p]) + (W pe[j] + b):
// `qkv` then holds ONE projected row per distinct conv position ([clip][P][3D], 154 rows per clip instead of 3150) and
// `g.pe_qkv` the 21 projected positional rows incl. the bias; the operand rows are gathered and summed here.  The windows
// of a clip re-read the same 154 rows, so the blocks are dealt to the XCDs in contiguous ranges (whole clips per L2).
// OR = rows of the K / Q / output image in LDS, >= S: 24 for the GestSync windows (S = 21) -- 8064 B per wave, five
// workgroups (20 waves) per CU, which is also what the 96 VGPRs allow; the kernel is bound by its per-wave latency chain
// (load -> LDS -> MFMA -> softmax -> LDS -> MFMA -> LDS -> store), so the number of waves in flight is what counts.
template <bool GATHER, int OR>
__global__ __launch_bounds__(256, 5) void attn_mfma_s32_kernel(const f16* __restrict__ qkv, int npairs, int S, int H, f16* __restrict__ out, AttnGather g) {
    constexpr int DK = 64, VT_PITCH = 72, O_PITCH = 144;
    __shared__ __attribute__((aligned(16))) char smem[4 * (64 * VT_PITCH + OR * O_PITCH)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int wg = blockIdx.x;
    if (GATHER) {
        const int per = ((int)gridDim.x + 7) >> 3;
        wg = (wg & 7) * per + (wg >> 3);
    }
    const int pair = wg * 4 + wave;
    if (pair >= npairs) return;
    char* sVt = smem + wave * (64 * VT_PITCH + OR * O_PITCH);
    const int r31o = (lane & 31) < OR ? (lane & 31) : OR - 1;       // rows >= OR only exist as clamped copies (masked keys, unused queries)
    char* sO = sVt + 64 * VT_PITCH;
    const int b = pair / H, head = pair - b * H;
    const int D = H * DK;
    const long ld = 3L * D;
    const f16* base = qkv + (GATHER ? 0L : (long)b * S * ld) + head * DK;
    const int r31 = lane & 31, hh = lane >> 5;
    // GATHER: source row of token j
    int gc = 0, gi = 0;
    if (GATHER) { gc = b / g.Twin; gi = b - gc * g.Twin - g.shift; }
    auto src_row = [&](int j) -> long {
        if (!GATHER) return j;
        int p = gi + j;
        p = p < 0 ? 0 : (p > g.P - 1 ? g.P - 1 : p);
        return (long)gc * g.P + p;
    };

    // ---- operand loads.  Every row's 128-byte q, k and v slices are read by 8 lanes x 16 B (8 cache lines per load
    // instruction; with lane = row and 16 B per lane a load touches 32 lines and the kernel ends up bound by the CU's
    // address/tag path, not by HBM), and all three operands go through LDS: K, then Q, row-major in the buffer that later
    // holds the output tile (a wave's LDS operations execute in order), V transposed.
    // Not GATHER: read exactly once, by this wave: nontemporal keeps the 310 MB stream from evicting what the other kernels of
    // the step (and the other lane) keep in L2 -- attention stage 0.517 -> 0.472 ms per step.  GATHER re-reads its rows: plain.
    f16x8 qq[4], kk[4], vv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = lane + 64 * r, row = c >> 3, part = c & 7;
        const int rc = row < S ? row : S - 1;
        const f16* p = base + src_row(rc) * ld + part * 8;
        qq[r] = load16<!GATHER>(p);
        kk[r] = load16<!GATHER>(p + D);
        vv[r] = load16<!GATHER>(p + 2 * D);
    }
    if (GATHER) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = lane + 64 * r, row = c >> 3, part = c & 7;
            const int rc = row < S ? row : S - 1;
            const f16* p = g.pe_qkv + (long)rc * ld + head * DK + part * 8;
            qq[r] += load16<false>(p);
            kk[r] += load16<false>(p + D);
            vv[r] += load16<false>(p + 2 * D);
        }
    }
    f16x8 kA[4], qB[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = lane + 64 * r, row = c >> 3, part = c & 7;
        if (OR == 32 || row < OR) stage_row<O_PITCH>(sO, row, part, kk[r]);
        stage_vt<VT_PITCH>(sVt, row, part, vv[r]);
    }
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 4; ++s) kA[s] = operand_frag<O_PITCH>(sO, r31o, s, hh);
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = lane + 64 * r, row = c >> 3, part = c & 7;
        if (OR == 32 || row < OR) stage_row<O_PITCH>(sO, row, part, qq[r]);
    }
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 4; ++s) qB[s] = operand_frag<O_PITCH>(sO, r31o, s, hh);

    // ---- S^T = K Q^T (K from registers: Q has taken its place in the image)
    f32x16 sc;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[i] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) sc = JG_MFMA_32x32x16(kA[s], qB[s], sc);

    // ---- softmax over the keys
    const float scale = 0.125f;                       // 1/sqrt(64)
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        sc[i] = mfma32_row(i, hh) < S ? sc[i] * scale : -INFINITY;
        mx = fmaxf(mx, sc[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
    exp_sum_tile(sc, mx, sum);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;

    // the two halves of pv_step, apart: both k-steps are split before the wave_lds_sync() and the MFMAs go block by block --
    // as one pv_step per k-step behind it, the <false, 24> instance needs 66 VGPRs instead of 60
    f16x8 pH[2], pL[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) split_hi_lo<true>(sc, s, pH[s], pL[s], inv);

    // ---- O^T = V^T P^T, then rows
    wave_lds_sync();
    f32x16 o[2];
    zero_tiles(o);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int s = 0; s < 2; ++s) pv_mfma<VT_PITCH>(pH[s], pL[s], s, sVt, 0, r31 + 32 * blk, hh, o[blk]);
    store_rows<2, 2, O_PITCH, OR, false>(o, sO, out + (long)b * S * D + head * DK, D, 0, S, lane);
}


// ---------------------------------------------------------------------------------------------
// MFMA kernel for S <= 160 (JEGAL gesture encoder: S = T = 150 frames), dk = 64, optional key mask.
// One workgroup per (sequence, head) pair, one wave per block of 32 queries (NB = ceil(S/32) waves).  K (row-major)
// and V (transposed) of the head are staged in LDS once per pair, nontemporal (each row is read once, by this workgroup);
// every wave computes its 32 x S score block into NB accumulator tiles, softmaxes over its registers and its partner
// lane, and puts 1 / sum into the probabilities before the hi + lo split.
template <int NB>
__global__ __launch_bounds__(64 * NB) void attn_mfma_kernel(const f16* __restrict__ qkv, const float* __restrict__ keymask,
                                                            int S, int H, f16* __restrict__ out) {
    constexpr int DK = 64, SP = 32 * NB, K_PITCH = 144, VT_PITCH = SP * 2 + 8, O_PITCH = 144, NT = 64 * NB;
    __shared__ __attribute__((aligned(16))) char sK[SP * K_PITCH];
    __shared__ __attribute__((aligned(16))) char sVt[64 * VT_PITCH];
    __shared__ __attribute__((aligned(16))) float sM[SP];
    static_assert(K_PITCH == O_PITCH, "the output tiles reuse the K image");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pair = blockIdx.x;
    const int b = pair / H, head = pair - b * H;
    const int D = H * DK;
    const long ld = 3L * D;
    const f16* base = qkv + (long)b * S * ld + head * DK;
    const int r31 = lane & 31, hh = lane >> 5;

    // ---- stage K, V^T and the mask row; this wave's queries: B operand straight from global memory
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = tid + NT * r, row = c >> 3, part = c & 7;          // SP rows x 8 chunks = 4 * NT
        const int rc = row < S ? row : S - 1;
        stage_kv<true, K_PITCH, VT_PITCH>(base + (long)rc * ld + part * 8, D, sK, sVt, row, part);
    }
    stage_mask(sM, SP, keymask, b, 0, S, tid, NT);
    const int q0 = 32 * wave;
    const int qr = q0 + r31 < S ? q0 + r31 : S - 1;
    f16x8 qB[4];
    load_q_operand(qB, base + (long)qr * ld, hh);
    __syncthreads();

    // ---- scores: NB tiles of 32 keys x 32 queries, softmax over all of them
    f32x16 sc[NB];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) sc[kb] = score_tile<4, K_PITCH>(sK, kb, qB, r31, hh);
    const float scale = 0.125f;
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) mask_scale_tile(sc[kb], sM + 32 * kb, hh, scale, mx);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) exp_sum_tile(sc[kb], mx, sum);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;

    // ---- O^T = V^T P^T
    f32x16 o[2];
    zero_tiles(o);
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s) pv_step<2, VT_PITCH, true>(sc[kb], s, sVt, 32 * kb, r31, hh, o, inv);
    // ---- rows, through this wave's slice of the K image: every wave is done with K
    __syncthreads();
    store_rows<2, 2, O_PITCH, 32, false>(o, sK + wave * (32 * O_PITCH), out + ((long)b * S + q0) * D + head * DK, D, q0, S, lane);
}

// ---------------------------------------------------------------------------------------------
// MFMA kernel for every other instance: dk = 64 with 160 < S (JEGAL clips of 161..500 frames, XLM-RoBERTa at L > 160) and
// dk = 96 at any S (JEGAL text encoder: d = 768, h = 8, jegal.py:35-38), optional key mask.  One workgroup per (sequence,
// head, group of up to 256 queries), one wave per 32 queries; the keys go by in chunks of 128: K and V^T of a chunk are
// staged in LDS once per workgroup (plain loads: the other query groups of the pair read the rows again), every wave
// computes its 32 x 128 score block, updates its ONLINE softmax state (running max and sum per query = per lane pair,
// fp32) and accumulates O^T += V^T P^T with unnormalised probabilities.  The 1 / sum normalisation happens once, in fp32, in
// the output path, which takes 32 columns at a time.  Score tiles entirely beyond S are skipped.
template <int DK>
__global__ __launch_bounds__(512) void attn_mfma_flash_kernel(const f16* __restrict__ qkv, const float* __restrict__ keymask, int S, int H,
                                                              f16* __restrict__ out) {
    constexpr int KC = 128, NV = DK / 8, KS = DK / 16, NBLK = DK / 32;
    constexpr int K_PITCH = DK * 2 + 16, VT_PITCH = KC * 2 + 8, O_PITCH = 80;
    constexpr int K_BYTES = KC * K_PITCH > 8 * 32 * O_PITCH ? KC * K_PITCH : 8 * 32 * O_PITCH;      // the output slices of eight waves alias the K image
    __shared__ __attribute__((aligned(16))) char sK[K_BYTES];
    __shared__ __attribute__((aligned(16))) char sVt[DK * VT_PITCH];
    __shared__ __attribute__((aligned(16))) float sM[KC];
    const int tid = threadIdx.x, lane = tid & 63, NT = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pair = blockIdx.x;
    const int b = pair / H, head = pair - b * H;
    const int D = H * DK;
    const long ld = 3L * D;
    const f16* base = qkv + (long)b * S * ld + head * DK;
    const int r31 = lane & 31, hh = lane >> 5;
    const int q0 = 256 * blockIdx.y + 32 * wave;
    const bool wave_on = q0 < S;                                    // (waves past the last query still help with the staging)
    const int qr = q0 + r31 < S ? q0 + r31 : S - 1;
    f16x8 qB[KS];
    load_q_operand(qB, base + (long)qr * ld, hh);
    f32x16 o[NBLK];
    zero_tiles(o);
    float mrun = -INFINITY, lrun = 0.f;
    const float scale = DK == 64 ? 0.125f : 0.10206207261596575f;   // 1 / sqrt(dk)

    for (int k0 = 0; k0 < S; k0 += KC) {
        __syncthreads();                                            // every wave is done with the previous chunk
        for (int idx = tid; idx < KC * NV; idx += NT) {
            const int row = idx / NV, part = idx - row * NV;
            const int rc = k0 + row < S ? k0 + row : S - 1;
            stage_kv<false, K_PITCH, VT_PITCH>(base + (long)rc * ld + part * 8, D, sK, sVt, row, part);
        }
        stage_mask(sM, KC, keymask, b, k0, S, tid, NT);
        __syncthreads();
        if (!wave_on) continue;
        const int ntile = (S - k0 + 31) / 32 < KC / 32 ? (S - k0 + 31) / 32 : KC / 32;      // tiles of this chunk that hold a key
        f32x16 sc[KC / 32];
        float cm = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KC / 32; ++kb) {
            if (kb >= ntile) break;
            sc[kb] = score_tile<KS, K_PITCH>(sK, kb, qB, r31, hh);
            mask_scale_tile(sc[kb], sM + 32 * kb, hh, scale, cm);
        }
        cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
        const float mnew = fmaxf(mrun, cm);                         // finite: the chunk holds at least one key < S
        const float alpha = __expf(mrun - mnew);                    // first chunk: exp(-inf) = 0
        mrun = mnew;
        lrun *= alpha;
#pragma unroll
        for (int blk = 0; blk < NBLK; ++blk)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[blk][i] *= alpha;
#pragma unroll
        for (int kb = 0; kb < KC / 32; ++kb) {
            if (kb >= ntile) break;
            exp_sum_tile(sc[kb], mnew, lrun);
#pragma unroll
            for (int s = 0; s < 2; ++s) pv_step<NBLK, VT_PITCH, false>(sc[kb], s, sVt, 32 * kb, r31, hh, o);
        }
    }
    // ---- normalise and rows, through this wave's slice of the K image
    __syncthreads();
    if (!wave_on) return;
    const float inv = 1.f / (lrun + __shfl_xor(lrun, 32, 64));
    store_rows<NBLK, 1, O_PITCH, 32, true>(o, sK + wave * (32 * O_PITCH), out + ((long)b * S + q0) * D + head * DK, D, q0, S, lane, inv);
}

template <int DK>
static hipError_t launch_attn_flash(const f16* qkv, const float* keymask, long npairs, int S, int H, f16* out, hipStream_t s) {
    const int nq = S < 256 ? S : 256;
    record_kernel("attn_mfma_flash_kernel<%d>", DK);
    hipLaunchKernelGGL((attn_mfma_flash_kernel<DK>), dim3((unsigned)npairs, (unsigned)((S + 255) / 256)), dim3(64 * ((nq + 31) / 32)), 0, s, qkv, keymask, S, H, out);
    return hipGetLastError();
}

template <int NB>
static hipError_t launch_attn_mfma(const f16* qkv, const float* keymask, long npairs, int S, int H, f16* out, hipStream_t s) {
    record_kernel("attn_mfma_kernel<%d>", NB);
    hipLaunchKernelGGL((attn_mfma_kernel<NB>), dim3((unsigned)npairs), dim3(64 * NB), 0, s, qkv, keymask, S, H, out);
    return hipGetLastError();
}

// The attn_mfma_s32_kernel instance for S <= 32: OR = 24 where the sequence fits, four pairs per workgroup; the gather form
// rounds the grid up to whole rounds of the eight XCDs (its block -> XCD deal).
template <bool GATHER>
static hipError_t launch_attn_s32(const f16* qkv, const AttnGather& g, long npairs, int S, int H, f16* out, hipStream_t s) {
    unsigned blocks = (unsigned)((npairs + 3) / 4);
    if (GATHER) blocks = (blocks + 7) / 8 * 8;
    const bool or24 = S <= 24;
    const auto kernel = or24 ? attn_mfma_s32_kernel<GATHER, 24> : attn_mfma_s32_kernel<GATHER, 32>;
    record_kernel("attn_mfma_s32_kernel<%d,%d>", (int)GATHER, or24 ? 24 : 32);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, qkv, (int)npairs, S, H, out, g);
    return hipGetLastError();
}

#ifndef JG_BF16      // fp16 only (declared in common.h's fp16-only block): a bf16 handle never has the tiled token stream this path needs
// Layer-0 attention of the GestSync transformer from per-position projections (see attn_mfma_s32_kernel<true>):
// B = windows (nclip * g.Twin), S <= 32 tokens, dk = 64.
hipError_t launch_attention_gather(const f16* qkv_pos, const AttnGather& g, int B, int S, int H, f16* out, hipStream_t s) {
    if (B <= 0 || S <= 0) return hipSuccess;
    const long npairs = (long)B * H;
    if (S > 32 || npairs >= (1L << 31) || g.Twin <= 0 || g.P <= 0 || !g.pe_qkv) return hipErrorInvalidValue;
    return launch_attn_s32<true>(qkv_pos, g, npairs, S, H, out, s);
}
#endif

hipError_t launch_attention(const f16* qkv, const float* keymask, int B, int S, int H, int dk, f16* out, const EngineOpts& o, hipStream_t s) {
    if (B <= 0 || S <= 0) return hipSuccess;
    const long npairs = (long)B * H;
    if (o.attn_mfma && S <= 32 && dk == 64 && !keymask && npairs < (1L << 31))
        return launch_attn_s32<false>(qkv, AttnGather{}, npairs, S, H, out, s);
    if (o.attn_mfma && S <= 160 && dk == 64 && npairs < (1L << 31)) {      // S <= 32 with a key mask: one query block
        static constexpr decltype(&launch_attn_mfma<1>) by_nb[5] = {launch_attn_mfma<1>, launch_attn_mfma<2>, launch_attn_mfma<3>, launch_attn_mfma<4>,
                                                                    launch_attn_mfma<5>};
        return by_nb[(S + 31) / 32 - 1](qkv, keymask, npairs, S, H, out, s);
    }
    // everything else on the matrix cores too: dk = 64 beyond 160 keys, dk = 96 (text encoder) at any length
    if (o.attn_mfma && npairs < (1L << 31) && (dk == 64 || dk == 96)) {
        if (dk == 64) return launch_attn_flash<64>(qkv, keymask, npairs, S, H, out, s);
        if (dk == 96) return launch_attn_flash<96>(qkv, keymask, npairs, S, H, out, s);
    }
    // option attn_mfma = 0 (A/B and tests): the VALU kernel
    dim3 grid, block;
    int G = 1;
    if (S <= 32) {
        G = 64 / S;
        grid = dim3((unsigned)((npairs + G - 1) / G));
        block = dim3(64);
    } else {
        grid = dim3((unsigned)npairs, (S + 255) / 256);
        block = dim3(256);
    }
    if (dk == 64) {
        record_kernel("attn_kernel<64>");
        hipLaunchKernelGGL(attn_kernel<64>, grid, block, 0, s, qkv, keymask, B, S, H, G, out);
    } else if (dk == 96) {
        record_kernel("attn_kernel<96>");
        hipLaunchKernelGGL(attn_kernel<96>, grid, block, 0, s, qkv, keymask, B, S, H, G, out);
    } else return hipErrorInvalidValue;
    return hipGetLastError();
}

JG_NS_END
