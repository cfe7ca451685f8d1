// libjegal_hip: the GEMM planner (gemm_plan.h) -- every admission rule and every tile choice of launch_gemm -- and the EngineOpts
// it reads (engine_opts_set / init / release), and the per-thread sink of record_kernel.  Host code only, one copy for both kernel builds.
#include "gemm_plan.h"

#include <algorithm>
#include <cstring>

namespace {

struct Tile { int mi, wm, wn; };      // wave tile 16 mi x 64 (LDS-DMA kernels) or 64 x 64 (register-staged), wm x wn waves

// The table entry with these template arguments and its launch figures for this shape ("rejected" if the library has no such kernel)
GemmPlan instance(const GemmShape& a, const EngineOpts& o, bool glds, bool w2, Tile t, bool spr = false, int xe = 0, bool c32 = false, bool lnf = false) {
    const int key[10] = {glds, w2, a.conv, t.mi, t.wm, t.wn, lnf, spr, xe, c32};
    GemmPlan p;
    for (int i = 0; i < GEMM_NUM_INSTANCES && p.instance < 0; ++i)
        if (std::equal(key, key + 10, GEMM_INSTANCES[i].key)) p.instance = i;
    if (p.instance < 0) return p;
    p.name = GEMM_INSTANCES[p.instance].name;
    const int bm = (glds ? 16 * t.mi : 64) * t.wm, bn = 64 * t.wn;
    const long tiles = ((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn);
    p.n_tiles = (a.N + bn - 1) / bn; p.total_tiles = (int)tiles;
    p.lds = glds ? glds_tile(w2, t.mi, t.wm, t.wn).lds() : (size_t)(bm + bn * (w2 ? 2 : 1)) * 128;      // register-staged: one stage
    p.grid = (unsigned)tiles;                                             // register-staged: one workgroup per tile
    if (!glds) return p;
    // Persistent: num_cu workgroups walk the tiles in rounds; inside a two-lane batch lane_walk x num_cu of them (shared.h), each with
    // 1/lane_walk of the rounds.  tile_of (gemm.hip) deals the tiles over any grid; no workgroup waits for another.
    const int walk = !o.lanes_active ? 1 : o.lane_walk[lnf ? EngineOpts::LW_LNF : a.conv ? EngineOpts::LW_CONV : EngineOpts::LW_GEMM];
    if ((lnf || o.gemm_persistent) && tiles > o.num_cu) p.grid = (unsigned)std::min(tiles, (long)walk * o.num_cu);
    // De-phasing the workgroups (4 phases, 2 us apart; the last phase falls on the workgroups that run one tile fewer):
    // once the outputs were nontemporal the epilogues became HBM-write-burst bound (every CU stores its 128 KB at the
    // same moment) and spreading them pays: qkv 157 -> 146 us.  Only for long plain GEMMs (>= 4 rounds); the LN-fused
    // and conv kernels and short launches measured neutral or slower.  Option gemm_stagger: ticks of 10 ns, -1 = off.
    // Round 3: the delay only pays when the last round is less than half full - the highest block ids, delayed longest, then run one
    // tile fewer (ff0, 3.08 rounds: 79 -> 75 us; N = 1024, 6.16 rounds: 129 -> 117 us; qkv 9.23: 175 -> 170; with a nearly full last
    // round it costs 2-3 %), short launches included (round 2: >= 4 rounds).  Inside the two-lane batches the plain GEMMs stay
    // un-staggered: the other lane's kernels already spread the store bursts and the delay only costs (+0.8 % per step measured).
    // LN-fused, round 3: in that kernel every workgroup reaches its store / reload phase at the same moment and that phase is an HBM
    // burst (100 MB per round in ~10 us) while the k loops leave HBM idle.  Four start phases spread it; the delay is free when the
    // last round is less than half full, because the highest block ids - the ones delayed longest - run one tile fewer: out_proj
    // 108 -> 94 us, linear2 265 -> 256 us at M = 100 800 (3.08 rounds), 52 -> 48 us at 1.15 rounds; with a nearly full last round it
    // costs what it delays (1.92 rounds: 58 -> 61 us), so it is off there -- and it stays on inside the two-lane batches.
    // With more workgroups than CUs (lane_walk) there is no de-phasing: the kernel's phase is blockIdx.x * 4 / grid, which takes all
    // workgroups to start together, and "the last phase runs one tile fewer" is an argument about resident workgroups.  The later
    // workgroups start whenever a CU frees, which spreads the bursts by itself.
    const bool pays = tiles > o.num_cu && 2 * (tiles % o.num_cu) < o.num_cu && p.grid <= (unsigned)o.num_cu;
    const int auto_stagger = !pays ? 0 : lnf ? (a.K <= 1024 ? 500 : 1400) : (!a.conv && !o.lanes_active ? 300 : 0);
    p.stagger = o.gemm_stagger < 0 ? 0 : o.gemm_stagger > 0 ? o.gemm_stagger : auto_stagger;
    return p;
}
GemmPlan glds(const GemmShape& a, const EngineOpts& o, bool w2, Tile t, bool spr = false, int xe = 0, bool c32 = false) {
    return instance(a, o, true, w2, t, spr, xe, c32);
}
GemmPlan staged(const GemmShape& a, const EngineOpts& o, int wm, int wn) { return instance(a, o, false, a.w2, {4, wm, wn}); }

bool ln_fusable(const GemmShape& a) {
    return !a.w2 && a.N == 512 && a.K % 64 == 0 && a.M >= GEMM_LN_FUSED_MIN_ROWS && a.lda % 8 == 0 && a.ldw % 8 == 0 && !a.relu && !a.scale &&
           !a.res && !a.out32 && a.res16 && a.out16 && !a.a_tiled;
}

// the tile of a launch that reaches the LDS-DMA kernel
GemmPlan plan_glds(const GemmShape& a, const EngineOpts& o) {
    const bool w2 = a.w2;
    // small problems (the JEGAL branch: M = B*T = 4800 tokens) would leave most CUs idle with 256-row tiles:
    // 128x128 tiles (32x64 wave tiles) give 4x the workgroups
    const long tiles256 = (long)((a.M + 255) / 256) * ((a.N + 127) / 128);
    const long tiles_big = (long)((a.M + 255) / 256) * ((a.N + 255) / 256);        // 256x256 tiles: fewer than CUs -> under-filled
    if (a.conv) {
        const bool after_skip = a.rowmap && a.const_in;      // consumer of a row-skipping producer: the instances whose loader can read the const image
        if (o.gemm_small_tile && (tiles256 < 200 || tiles_big < 224)) return glds(a, o, w2, {2, 4, 2}, after_skip);
        if (!w2 && o.gemm_big_tile && a.N >= 256 && a.N % 256 == 0) return glds(a, o, false, {8, 2, 4}, after_skip);
        // N = 128 (conv2): 512x128 block tile, the whole 160 KiB of LDS -- the activation side dominates the
        // L2->LDS traffic there, a taller tile halves the weight re-reads per activation byte
        if (!w2 && !after_skip && o.gemm_tall_tile && a.N == 128 && a.M >= 512 * 256) return glds(a, o, false, {8, 4, 2});
        return glds(a, o, w2, {4, 4, 2}, after_skip);
    }
    // Plain GEMMs: pick the tile by a cost estimate, rounds of one tile per CU x (k-tiles x time per k-tile + epilogue), with
    // the per-tile figures measured on the box (tools/gemm_tiles.py; us, L2-resident operands): bigger tiles move fewer
    // bytes per FLOP through the CU's LDS-DMA path but fill fewer CUs / leave emptier last rounds.  Every instance
    // accumulates k in the same order, so the choice never changes a bit of the result.  (Round 2 took the 128x128 tile
    // whenever fewer than 224 of the 256x256 tiles existed: M = 4800 x N = 2048 ran three rounds of small tiles instead of
    // one round of 152 big ones, and XLM-R's N = 768 layers likewise.)
    const int nk = (a.K + 63) / 64;
    auto est = [&](int bm, int bn, double kt_us, double epi_us) {
        const long tiles = (long)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn);
        return (double)((tiles + o.num_cu - 1) / o.num_cu) * (nk * kt_us + epi_us);
    };
    const bool spr = a.K <= 1024;      // 256x256, short k loops: spread DMA issue
    if (a.ln_mode) {
        // implicit-LayerNorm epilogues (XE instances): single fp16 weights -> 256x256 or 128x128, hi+lo -> 256x128 or 128x128, by the
        // same cost estimate
        const int xe = a.ln_mode == 1 ? 1 : 2;
        if (w2) {
            if (est(128, 128, 1.25, 1.0) < est(256, 128, 1.6, 1.6) && o.gemm_tile != 2) return glds(a, o, true, {2, 4, 2}, false, xe);
            return glds(a, o, true, {4, 4, 2}, false, xe);
        }
        const bool big_ok = a.N % 256 == 0;
        if (!big_ok || (est(128, 128, 0.95, 1.0) < est(256, 256, 1.45, 2.7) && o.gemm_tile != 3) || o.gemm_tile == 1)
            return glds(a, o, false, {2, 4, 2}, false, xe);
        return glds(a, o, false, {8, 2, 4}, spr, xe);
    }
    const bool can_big = !w2 && o.gemm_big_tile && a.N >= 256 && a.N % 256 == 0;
    const double e_small = o.gemm_small_tile ? est(128, 128, w2 ? 1.25 : 0.95, 1.0) : 1e30;
    const double e_mid = est(256, 128, w2 ? 1.6 : 1.2, 1.6);
    const double e_big = can_big ? est(256, 256, 1.45, 2.7) : 1e30;
    int pick = e_big <= e_mid && e_big <= e_small ? 3 : (e_mid <= e_small ? 2 : 1);
    if (o.gemm_tile >= 1 && o.gemm_tile <= 3 && (o.gemm_tile != 3 || can_big)) pick = o.gemm_tile;
    if (pick == 1) return glds(a, o, w2, {2, 4, 2});
    if (pick == 3 && !w2) return glds(a, o, false, {8, 2, 4}, spr);
    return glds(a, o, w2, {4, 4, 2});
}

}  // namespace

GemmPlan plan_gemm(const GemmShape& a, const EngineOpts& o) {
    const GemmPlan rejected;
    if (a.ln_w) {
        if (a.conv || !ln_fusable(a) || (a.bias_clip && (a.rpc < GEMM_LN_CLIP_MIN_RPC || a.nclips <= 0))) return rejected;
        return instance(a, o, true, false, {8, 1, 8}, false, 0, false, true);      // 128x512 tiles, always persistent
    }
    const bool narrow = a.N <= 64;
    if (a.bias_clip) {
        // per-clip bias: only the LDS-DMA kernel's fp16 row epilogue knows it (the LayerNorm-fused route returned above); the minimum
        // rows per clip keep a tile within two clips' reach of the straddle path's per-block lookup.  Anything else is refused:
        // there is no path that would quietly drop the correction.
        const bool ok = !a.conv && !a.ln_mode && o.gemm_glds && a.rpc >= GEMM_CLIP_MIN_RPC && a.nclips > 0 && a.K % 64 == 0 && a.M >= GEMM_GLDS_MIN_ROWS &&
                        a.lda % 8 == 0 && a.ldw % 8 == 0 && a.N % 128 == 0 && a.out16 && !a.out32 && !a.res && (a.ldc & 7) == 0 && !narrow;
        if (!ok) return rejected;
    }
    if (a.ln_mode) {
        // implicit LayerNorm: LDS-DMA instances with the fast epilogues only (whole tiles along n, 16-byte rows); anything else is a
        // caller error -- there is no slow path that would quietly ignore the statistics
        const bool shape_ok = !a.conv && o.gemm_glds && a.K % 64 == 0 && a.M >= GEMM_GLDS_MIN_ROWS && a.lda % 8 == 0 && a.ldw % 8 == 0 && a.N % 128 == 0 &&
                              a.ldc % 8 == 0;
        const bool mode1_ok = a.ln_mode == 1 && a.ln_stats && a.scale && a.bias && a.out16 && !a.out32 && !a.res;
        const bool mode2_ok = a.ln_mode == 2 && a.ln_stats && a.scale && a.bias && a.out16 && a.out_lo && a.xres_hi && a.xres_lo && a.stat_out &&
                              !a.out32 && !a.res && !a.relu;
        if (!shape_ok || !(mode1_ok || mode2_ok) || a.ln_w || a.a_tiled) return rejected;
        return plan_glds(a, o);
    }
    // the tiled token plane as A operand: LDS-DMA kernel only
    if (a.a_tiled && (a.conv || narrow || !o.gemm_glds || a.K != 512 || a.M < GEMM_GLDS_MIN_ROWS || a.N % 128)) return rejected;
    if (a.conv) {
        if (a.res) return rejected;          // the conv instances are compiled without the residual path
        // as for the plain GEMMs below: 4 columns per lane in every store, 16-byte pieces of the weight rows in every loader
        if (a.N % 4 || a.ldc % 4 || a.ldw % 8) return rejected;
        const bool coords_ok = a.H + a.PH < 2048 && a.W + a.PW < 2048 && a.M < ROWMAP_MAX_ROWS;      // packed pixel coordinates / rowmap entries
        // C = 32 -> N = 64 (the second audio conv): its own LDS-DMA instance, 256x64 tiles (round 5; before: the register-staged kernel)
        if (o.gemm_glds && !a.w2 && a.N == 64 && a.C == 32 && a.K % 32 == 0 && a.K == a.KH * a.KW * 32 && !a.tap_table && !a.rowmap &&
            a.M >= GEMM_GLDS_CONV_MIN_ROWS && coords_ok && a.out16 && !a.out32 && (a.ldc & 7) == 0 && (a.ldw & 7) == 0)
            return glds(a, o, false, {2, 8, 1}, false, 0, true);
        if (narrow) return a.rowmap ? rejected : staged(a, o, 4, 1);      // (a row map: as below)
        if (o.gemm_glds && a.M >= GEMM_GLDS_CONV_MIN_ROWS && a.C % 64 == 0 && a.N % 128 == 0 && coords_ok) return plan_glds(a, o);
        if (a.rowmap) return rejected;          // only the LDS-DMA kernel knows the compaction
        return staged(a, o, 2, 2);
    }
    // every epilogue stores 4 columns per lane (16 / 8 bytes) and reads the residual the same way; the register-staged kernel below
    // also loads A and W in 8-element (16-byte) pieces and only masks whole pieces against K: anything else would read columns >= K
    if (a.N % 4 || a.ldc % 4 || (a.res && a.ldr % 4)) return rejected;
    const bool staged_ok = a.K % 8 == 0 && a.lda % 8 == 0 && a.ldw % 8 == 0;
    if (narrow) return staged_ok ? staged(a, o, 4, 1) : rejected;
    if (o.gemm_glds && a.K % 64 == 0 && a.M >= GEMM_GLDS_MIN_ROWS && a.lda % 8 == 0 && a.ldw % 8 == 0 && a.N % 128 == 0) return plan_glds(a, o);
    return staged_ok ? staged(a, o, 2, 2) : rejected;
}

bool engine_opts_set(EngineOpts& o, const char* name, int value) {
    if (!std::strcmp(name, "conv1_mfma16")) o.conv1_mfma16 = value != 0;
    else if (!std::strcmp(name, "conv1_zero_skip")) o.conv1_zero_skip = value != 0;
    else if (!std::strcmp(name, "attn_mfma")) o.attn_mfma = value != 0;
    else if (!std::strcmp(name, "gemm_glds")) o.gemm_glds = value != 0;
    else if (!std::strcmp(name, "gemm_tall_tile")) o.gemm_tall_tile = value != 0;
    else if (!std::strcmp(name, "gemm_small_tile")) o.gemm_small_tile = value != 0;
    else if (!std::strcmp(name, "gemm_big_tile")) o.gemm_big_tile = value != 0;
    else if (!std::strcmp(name, "gemm_tile")) o.gemm_tile = value;
    else if (!std::strcmp(name, "gemm_counted")) o.gemm_counted = value != 0;
    else if (!std::strcmp(name, "gemm_persistent")) o.gemm_persistent = value != 0;
    else if (!std::strcmp(name, "gemm_stagger")) o.gemm_stagger = value;
    else if (!std::strncmp(name, "lane_walk", 9)) {
        static const char* const family[4] = {"_gemm", "_conv", "_lnf", "_conv1"};
        if (value < 1 || value > LANE_WALK_MAX) return false;
        bool known = !name[9];                                            // "lane_walk": every family
        for (int f = 0; f < 4; ++f)
            if (!name[9] || !std::strcmp(name + 9, family[f])) { o.lane_walk[f] = value; known = true; }
        return known;
    }
    else return false;
    return true;
}

hipError_t engine_opts_init(EngineOpts& o, int device) {
    o.device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return e;
    o.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // production walk factors (shared.h; measurements: tools/experiments/README.md, "Lane walk"): the plain GEMMs of a two-lane batch
    // launch four workgroups per CU; the conv GEMMs, the LayerNorm-fused kernel and conv1 measured neutral or slower and stay at one
    o.lane_walk[EngineOpts::LW_GEMM] = 4;
    void* z = nullptr;
    e = hipMalloc(&z, 256);                  // zero page on THIS device: LDS-DMA cannot predicate, but it can read zeros
    if (e != hipSuccess) return e;
    e = hipMemset(z, 0, 256);
    if (e != hipSuccess) return e;
    o.zeros = z;
    return hipSuccess;
}

void engine_opts_release(EngineOpts& o) {
    if (o.zeros) (void)hipFree(const_cast<void*>(o.zeros));
    o.zeros = nullptr;
}

// where record_kernel (shared.h) writes on this thread: a check point's name slot while its call runs, nullptr otherwise
char*& kernel_name_sink() {
    static thread_local char* sink = nullptr;
    return sink;
}
