// The GEMM launch policy of libjegal_hip: which kernel instance a launch gets and which argument sets the GEMM accepts.
//
// plan_gemm() (gemm_plan.hip) is the ONE place that decides.  launch_gemm (gemm.hip) derives a GemmShape from its GemmArgs, asks, and
// launches the instance the plan names; the host units ask the same function before they commit to a form (linear.hip: the run-time
// corrected form of a call; gestsync.hip: the fused transformer plan and the row-skipping conv chain), and jg_debug_gemm_plan
// (checks.hip) shows the answer on a machine without a GPU.  The choice does not depend on the 16-bit operand type, so this header
// is included once and is not part of the fp16 / bf16 double include of common.h: there is one planner in the library.
#pragma once
#include "shared.h"      // EngineOpts

// ---- the instance table: every gemm_glds_kernel / gemm_kernel instantiation the library holds per build, each exactly once.
// gemm_glds_kernel<W2, CONV, MI, WM, WN, LNF, SPR, XE, C32> (LDS-DMA; block tile 16 MI WM x 64 WN) ...
#define JG_GEMM_GLDS_INSTANCES(X)                                                                                                  \
    /* plain Linear: 128x128, 256x128 (single / hi+lo weights), 256x256 (SPR: K <= 1024) */                                        \
    X(0, 0, 2, 4, 2, 0, 0, 0, 0) X(1, 0, 2, 4, 2, 0, 0, 0, 0) X(0, 0, 4, 4, 2, 0, 0, 0, 0) X(1, 0, 4, 4, 2, 0, 0, 0, 0)            \
    X(0, 0, 8, 2, 4, 0, 1, 0, 0) X(0, 0, 8, 2, 4, 0, 0, 0, 0)                                                                      \
    /* residual + LayerNorm fused, 128x512: the whole LDS */                                                                       \
    X(0, 0, 8, 1, 8, 1, 0, 0, 0)                                                                                                   \
    /* implicit-LayerNorm consumer (XE = 1) and producer (XE = 2) epilogues */                                                     \
    X(0, 0, 2, 4, 2, 0, 0, 1, 0) X(1, 0, 2, 4, 2, 0, 0, 1, 0) X(1, 0, 4, 4, 2, 0, 0, 1, 0) X(0, 0, 8, 2, 4, 0, 1, 1, 0)            \
    X(0, 0, 8, 2, 4, 0, 0, 1, 0)                                                                                                   \
    X(0, 0, 2, 4, 2, 0, 0, 2, 0) X(1, 0, 2, 4, 2, 0, 0, 2, 0) X(1, 0, 4, 4, 2, 0, 0, 2, 0) X(0, 0, 8, 2, 4, 0, 1, 2, 0)            \
    X(0, 0, 8, 2, 4, 0, 0, 2, 0)                                                                                                   \
    /* conv: 128x128, 256x128, 256x256, the tall 512x128 tile (conv2) and the C = 32 instance (256x64) */                          \
    X(0, 1, 2, 4, 2, 0, 0, 0, 0) X(1, 1, 2, 4, 2, 0, 0, 0, 0) X(0, 1, 4, 4, 2, 0, 0, 0, 0) X(1, 1, 4, 4, 2, 0, 0, 0, 0)            \
    X(0, 1, 8, 2, 4, 0, 0, 0, 0) X(0, 1, 8, 4, 2, 0, 0, 0, 0) X(0, 1, 2, 8, 1, 0, 0, 0, 1)                                         \
    /* conv behind a row-skipping producer (SPR: the loader reads ConvGeom::const_in) */                                           \
    X(0, 1, 2, 4, 2, 0, 1, 0, 0) X(1, 1, 2, 4, 2, 0, 1, 0, 0) X(0, 1, 4, 4, 2, 0, 1, 0, 0) X(1, 1, 4, 4, 2, 0, 1, 0, 0)            \
    X(0, 1, 8, 2, 4, 0, 1, 0, 0)
// ... and gemm_kernel<WM, WN, CONV, W2> (register-staged; block tile 64 WM x 64 WN)
#define JG_GEMM_STAGED_INSTANCES(X)                                                                                                \
    X(4, 1, 0, 0) X(4, 1, 0, 1) X(2, 2, 0, 0) X(2, 2, 0, 1) X(4, 1, 1, 0) X(4, 1, 1, 1) X(2, 2, 1, 0) X(2, 2, 1, 1)

struct GemmInstance {
    const char* name;       // what the instance's launch thunk (gemm.hip) hands to record_kernel: jg_debug_last_kernel reads exactly this
    int key[10];            // {LDS-DMA kernel (512 threads) or register-staged (256), W2, CONV, MI, WM, WN, LNF, SPR, XE, C32}
};
constexpr GemmInstance GEMM_INSTANCES[] = {
#define X(W2, CONV, MI, WM, WN, LNF, SPR, XE, C32) \
    {"gemm_glds_kernel<" #W2 "," #CONV "," #MI "," #WM "," #WN "," #LNF "," #SPR "," #XE "," #C32 ">", {1, W2, CONV, MI, WM, WN, LNF, SPR, XE, C32}},
    JG_GEMM_GLDS_INSTANCES(X)
#undef X
#define X(WM, WN, CONV, W2) {"gemm_kernel<" #WM "," #WN "," #CONV "," #W2 ">", {0, W2, CONV, 4, WM, WN, 0, 0, 0, 0}},
    JG_GEMM_STAGED_INSTANCES(X)
#undef X
};
constexpr int GEMM_NUM_INSTANCES = sizeof(GEMM_INSTANCES) / sizeof(GEMM_INSTANCES[0]);

// ---- the LDS-DMA tile of gemm_glds_kernel<W2, CONV, MI, WM, WN, ...>: its sizes and the layout of the scratch that the epilogues keep
// in LDS stage 1 (idle from the end of a tile's k loop until the next tile's k-tile 1 is staged).  One definition for the kernel, its
// epilogues (gemm.hip: each one that keeps scratch there asserts that its areas fit in STAGE) and the planner (GemmPlan::lds).  A new
// epilogue that needs scratch adds its offsets and its *_END here.
struct GldsTile {
    int BM, BN;             // block tile: 16 MI WM rows (m) x 64 WN columns (n); k-step 64 = one 128-B row per tile row
    int XI, WI;             // LDS-DMA instructions (8 rows each) per wave and k-tile: activations, weights (hi; as many again for lo)
    int XB, WB;             // bytes of a stage's activation tile / of one weight tile
    int STAGE;              // bytes of one of the two stages: activations, hi weights (, lo weights)
    int NPIECE;             // LDS-DMA instructions per wave and k-tile in all
    int TP16;               // row pitch of the row-transposing scratch: 16-B aligned, 36 banks -> conflict-free b64 writes
    // byte offsets from the start of stage 1
    int ROWS_WAVE;          // epi_rows16: 16 rows x TP16 of transposing scratch per wave, from offset 0 ...
    int ROWS_TAB;           // ... and behind the 8 waves' scratch the per-wave tables: 128 output rows (ConvGeom::rowmap; the fragment store reads
    int ROWS_END;           //     them too) or 64 column factors (XE 1)
    bool LO_LDS;            // epi_ln_producer: room for a second scratch area per wave (the lo plane, PROD_WAVE / 2 behind the hi plane)?
    int PROD_WAVE;          // its transposing scratch per wave, from offset 0 ...
    int PROD_GSC, PROD_END; // ... and gamma of each wave's 64 columns behind it
    int LN_RED, LN_PAR, LN_END;      // LayerNorm-fused epilogue: row statistics [2][8 waves][BM], then [4][BN] bias / gamma / beta / second clip's bias
    constexpr size_t lds() const { return 2 * (size_t)STAGE; }      // double-buffered; 128x512 LN-fused = 160 KiB, the whole LDS
};
constexpr GldsTile glds_tile(bool w2, int mi, int wm, int wn) {
    GldsTile t = {};
    t.BM = 16 * mi * wm; t.BN = 64 * wn;
    t.XI = t.BM / 64; t.WI = t.BN / 64;
    t.XB = t.BM * 128; t.WB = t.BN * 128;
    t.STAGE = t.XB + t.WB * (w2 ? 2 : 1);
    t.NPIECE = t.XI + t.WI * (w2 ? 2 : 1);
    t.TP16 = 144;
    t.ROWS_WAVE = 16 * t.TP16;
    t.ROWS_TAB = 8 * t.ROWS_WAVE;
    t.ROWS_END = t.ROWS_TAB + 8 * 128 * 4;
    t.LO_LDS = t.STAGE / 8 >= 32 * t.TP16;
    t.PROD_WAVE = (t.LO_LDS ? 32 : 16) * t.TP16;
    t.PROD_GSC = 8 * t.PROD_WAVE;
    t.PROD_END = t.PROD_GSC + 8 * 64 * 4;
    t.LN_RED = 0;
    t.LN_PAR = 2 * 8 * t.BM * 4;
    t.LN_END = t.LN_PAR + 4 * t.BN * 4;
    return t;
}

// ---- minimum row counts of the routes (the planner's own rules use them; the host pads or asks, it does not restate them)
constexpr int GEMM_GLDS_MIN_ROWS = 128;         // a Linear launch reaches the LDS-DMA kernel from this many rows (shorter batches: pad with zero rows)
constexpr int GEMM_GLDS_CONV_MIN_ROWS = 256;    // ... and a conv launch from this many output pixels
constexpr int GEMM_LN_FUSED_MIN_ROWS = 1024;    // residual + LayerNorm fused (row-wide 128x512 tiles)
constexpr int GEMM_CLIP_MIN_RPC = 256;          // per-clip bias through the fp16 row epilogue: rows per clip (a tile stays within two clips' reach)
constexpr int GEMM_LN_CLIP_MIN_RPC = 128;       // ... through the LayerNorm-fused epilogue (128-row tiles)

// Everything the choice depends on and nothing it does not: sizes, which operands / outputs are present, plain values.  No pointers.
struct GemmShape {
    long M;
    int N, K;
    long lda, ldw, ldc, ldr;
    bool w2;                                    // lo weights present
    bool out16, out32, res, scale, bias, bias_clip, ln_w, res16, a_tiled;
    bool ln_stats, xres_hi, xres_lo, out_lo, stat_out;      // ln_mode 2's planes and the statistics
    int relu, ln_mode, rpc, nclips;
    bool conv;                                  // implicit-GEMM convolution: the geometry below counts
    int H, W, C, KH, KW, PH, PW, tap_table;
    bool rowmap, const_in;

    template <class Geom>
    void set_geom(const Geom& g) {
        conv = true;
        H = g.H; W = g.W; C = g.C; KH = g.KH; KW = g.KW; PH = g.PH; PW = g.PW; tap_table = g.tap_table;
        rowmap = g.rowmap != nullptr; const_in = g.const_in != nullptr;
    }
};

// The shape of a GemmArgs (either build's)
template <class Args>
inline GemmShape gemm_shape(const Args& a, bool conv) {
    GemmShape s = {};
    s.M = a.M; s.N = a.N; s.K = a.K; s.lda = a.lda; s.ldw = a.ldw; s.ldc = a.ldc; s.ldr = a.ldr;
    s.w2 = a.Wl != nullptr;
    s.out16 = a.out16 != nullptr; s.out32 = a.out32 != nullptr; s.res = a.res != nullptr; s.scale = a.scale != nullptr;
    s.bias = a.bias != nullptr; s.bias_clip = a.bias_clip != nullptr; s.ln_w = a.ln_w != nullptr; s.res16 = a.res16 != nullptr;
    s.a_tiled = a.a_tiled != 0;
    s.ln_stats = a.ln_stats != nullptr; s.xres_hi = a.xres_hi != nullptr; s.xres_lo = a.xres_lo != nullptr; s.out_lo = a.out_lo != nullptr;
    s.stat_out = a.stat_out != nullptr;
    s.relu = a.relu; s.ln_mode = a.ln_mode; s.rpc = a.rpc; s.nclips = a.nclips;
    if (conv) s.set_geom(a.g);
    return s;
}

// The verdict: rejected (instance < 0: launch_gemm returns hipErrorInvalidValue and launches nothing), or one entry of GEMM_INSTANCES
// with its launch figures.
struct GemmPlan {
    int instance = -1;
    const char* name = "rejected";              // GEMM_INSTANCES[instance].name: jg_debug_gemm_plan shows it, the launch thunk records it
    unsigned grid = 0;
    size_t lds = 0;
    int n_tiles = 0, total_tiles = 0;           // tiles along n / in all (the LDS-DMA kernels' arguments)
    int stagger = 0;                            // de-phasing delay in 10-ns ticks per phase (LDS-DMA kernels; 0: none)
    bool ok() const { return instance >= 0; }
    bool glds() const { return instance >= 0 && GEMM_INSTANCES[instance].key[0]; }
};

// Pure: no HIP call, dereferences nothing, keeps no state.  Reads the gemm_* options, num_cu, lanes_active and lane_walk of `o`.
GemmPlan plan_gemm(const GemmShape& s, const EngineOpts& o);

// The EngineOpts half of jg_set_option ("gemm_*", "lane_walk*", "attn_mfma", "conv1_mfma16", "conv1_zero_skip"): true if `name` is one of them
// (and, for a walk factor, the value is in 1..LANE_WALK_MAX)
bool engine_opts_set(EngineOpts& o, const char* name, int value);
