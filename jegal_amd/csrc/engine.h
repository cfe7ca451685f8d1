// libjegal_hip host side: the handle, the packed model state and the helpers the host units share (api.hip, linear.hip,
// gestsync.hip, gestsync_audio.hip, jegal.hip, xlmr.hip, checks.hip).  Host code only; the kernel units do not include it.
#pragma once
#include "common.h"
#define JG_BF16                  // the bf16 build's declarations (namespace bf): the dispatched launchers, f16 = __bf16
#include "common.h"
#undef JG_BF16
#include "gemm_plan.h"
#include "weight_pack.h"      // (and weight_form.h)
#include "../../include/jegal_hip.h"
#include "audit32.h"
#include "gemm_x3.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <vector>

namespace engine {

// ---- dispatch between the two kernel builds.  LAUNCH(h, launch_x, args...) calls launch_x of the fp16 build or bf::launch_x of
// the bf16 build (precision mode JG_PREC_BF16): same argument lists, the 16-bit pointers and the structs that carry them are
// layout-identical in both builds and simply re-typed.  Only launchers that depend on the 16-bit type AND run on a bf16 handle
// exist in both builds and go through LAUNCH (the rule: common.h); every other launcher exists once and is called plainly.
[[maybe_unused]] inline const bf::f16* to_bf(const f16* p) { return reinterpret_cast<const bf::f16*>(p); }
inline bf::f16* to_bf(f16* p) { return reinterpret_cast<bf::f16*>(p); }
inline const bf::GemmArgs& to_bf(const GemmArgs& a) { return reinterpret_cast<const bf::GemmArgs&>(a); }
static_assert(sizeof(bf::GemmArgs) == sizeof(GemmArgs), "the two builds share their argument struct");
template <class T> inline T to_bf(T v) { return v; }
template <class F, class G, class... A>
inline hipError_t dispatch_build(bool bf16, F f, G g, A... a) { return bf16 ? g(to_bf(a)...) : f(a...); }
#define LAUNCH(h, fn, ...) engine::dispatch_build((h)->bf16, fn, bf::fn, __VA_ARGS__)

struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
    mutable bool used = false;      // consumed by a finalize (find / need): erased when that finalize is done
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct BiasCalib;
struct Lin {            // packed Linear / folded conv:  [N][K] fp16 hi (+lo), fp32 bias.  Read-only once packed, but for `uncalibrated`
    f16* wh = nullptr;
    f16* lo = nullptr;          // the lo half, or nullptr when it is not kept (lo_kept).  Whether a GEMM runs with it: run_lo() below
    float* bias = nullptr;
    int N = 0, K = 0;
    WeightForm form = WF_SINGLE;        // which weights the layer's GEMM runs with (weight_form.h)
    bool uncalibrated = false;          // starts_uncalibrated: hi+lo until apply_bias_corrections (jg_calibrate_xlmr) clears it
    BiasCalib* cal = nullptr;           // WF_BIAS_CORRECTED: the layer's calibration record (owned by Model::bc)
    // Linear behind an IMPLICIT LayerNorm (GemmArgs::ln_mode 1): wh / lo / BiasCalib::w32 hold W . diag(gamma), bias / BiasCalib::b32 hold b + W beta, and
    // c1h / c1f [N] the column sums of the packed weights -- of `wh` alone (single-fp16 runs: the GEMM then is exactly
    // sum_k wh[n][k] (x[k] - mean) rstd, and the bias correction covers the lo part) and of wh + lo (hi+lo runs)
    float* c1h = nullptr;
    float* c1f = nullptr;
    // fp32 audit path (JG_PREC_FP32 / option audit_weights; audit32.hip): the fp32 matrix [N][K] as packed (BatchNorm folded, same k order as
    // wh) and the layer's own fp32 bias (`bias` above may carry a calibration's correction)
    float* w32d = nullptr;
    float* b32d = nullptr;
};
// What a calibration pass records for one bias-corrected layer and what apply_bias_corrections needs to fold it into the layer's bias
struct BiasCalib {
    Lin* layer = nullptr;
    float* mu = nullptr;        // device [K]: column sums of the A operand seen during calibration
    long mu_rows = 0;
    std::vector<float> w32, b32;        // the matrix and the bias as packed, fp32
};
struct LNp { float* w = nullptr; float* b = nullptr; };

struct EncLayer { Lin qkv, out, ff1, ff2; LNp n1, n2; };

struct Arena {          // stream-ordered bump allocator over persistent chunks
    struct Chunk { char* p; size_t cap; };
    std::vector<Chunk> chunks;
    size_t cur = 0, off = 0;
    void reset() { cur = 0; off = 0; }     // begin_pass, and nobody else: what else a pass's beginning means is decided there
    unsigned long tick = 0;         // jg_set_stream: when this arena was last parked (least recently used goes first)
    size_t total() const { size_t t = 0; for (auto& c : chunks) t += c.cap; return t; }
    void* alloc(size_t bytes, hipError_t* err) {
        bytes = (bytes + 255) & ~size_t(255);
        while (cur < chunks.size()) {
            if (off + bytes <= chunks[cur].cap) { void* r = chunks[cur].p + off; off += bytes; return r; }
            ++cur; off = 0;
        }
        size_t cap = bytes > (size_t(1) << 30) ? bytes : (size_t(1) << 30);
        char* p = nullptr;
        hipError_t e = hipMalloc(&p, cap);
        if (e != hipSuccess) { *err = e; return nullptr; }
        chunks.push_back({p, cap});
        cur = chunks.size() - 1; off = bytes;
        return p;
    }
    void release() { for (auto& c : chunks) (void)hipFree(c.p); chunks.clear(); cur = off = 0; }
};

// What the last conv stack on this handle did (jg_debug_conv2_rowskip, jg_debug_conv_rows).  The two device words lie in the workspace of
// the pass that ran the stack, so the report lives exactly as long as that pass: gs_conv_stack fills it, begin_pass and a switch of
// streams (jg_set_stream) clear it.
struct ConvReport {
    const int* rowskip = nullptr;       // device word: min over the stack's positions of conv2's row skip
    const int* totals = nullptr;        // device [4]: rows conv2 .. conv5 computed
    long full[4] = {0, 0, 0, 0};        // ... of these many
    void clear() { *this = ConvReport(); }
};

struct ProfRec { int stage; hipEvent_t e0, e1; };

// What each model's finalize owns besides its layers (the drivers reload the state_dict on every command: drop_model)
struct Model {
    int id = 0;                    // 1 GestSync, 2 JEGAL, 3 XLM-RoBERTa: bit id - 1 of a `which` / `models` mask
    bool ready = false;
    std::vector<void*> allocs;     // device weights and the buffers derived from them (walloc)
    std::deque<BiasCalib> bc;      // calibration records of the bias-corrected layers (a deque: Lin::cal points into it)
};

struct GestSyncModel {
    Model m{1};
    Lin c1, c2, c3, c4, c5, fc6, ff0, ff2;
    EncLayer layers[6];
    float* pe = nullptr;
    // const chain: what conv2 / conv3 / conv4 compute from an all-constant pooled image (relu(bias1) everywhere) -- the rows of
    // their outputs that the zero-band skip makes position-independent are read from here (ConvGeom::const_in); 4 copies each
    f16 *c2C = nullptr, *c3C = nullptr, *c4C = nullptr, *c5C = nullptr;
    float* c1_scale255 = nullptr;
    f16* c1_direct = nullptr;      // conv1 weights, slot-major [49][64][16] for the direct kernel
    f16* qpe = nullptr;            // [21][1536]: layer-0 W_qkv pe[j] + b (Qkv0); recomputed when weights or bias corrections change
    bool qpe_valid = false;
};

// GestSync's audio stream (net_aud + ff_aud, gestsync.py:89-146,346-361; gestsync_audio.hip): `which` bit 3, a model of its own beside
// the video stream -- either can be finalized without the other.  Weight forms as a GestSync model (id 1)
struct GestSyncAudioModel {
    Model m{1};
    float* c1w = nullptr;          // conv1 [64][9] fp32, BatchNorm scale folded (gsa_conv1_pool_kernel)
    float* c1shift = nullptr;      // [64]
    Lin c2, c3, c4, c5, fc6, fc7, fc8;      // channels padded to powers of two: 192 -> 256 (c2 out, c3 in), 384 -> 512 (c3 out, c4 in)
};

struct JegalModel {
    Model m{2};
    Lin ip0, ip3, op_rgb, al_g0, al_g2, fu0, fu2, al_c0, al_c2, op_text, op_audio;
    Lin a0, a3, a6, a9, a12, a15;  // audio CNN
    LNp ip_ln, rgb_norm, text_norm;
    float* rgb_pe = nullptr;
    EncLayer rgb_layers[6], text_layers[3];
};

// XLM-RoBERTa text front end (third-party transformers.XLMRobertaModel, call site jegal.py:116-129)
struct XlmrModel {
    Model m{3};
    int vocab = 0, maxpos = 0;
    float *word = nullptr, *pos = nullptr, *type = nullptr;
    LNp emb_ln;
    std::vector<EncLayer> layers;
    bool folded = false;           // packed for the implicit-LayerNorm pass (option xlmr_fold at finalize, xlmr_encode_folded)
};

}  // namespace engine

struct jg_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    std::string err;
    int precision = JG_PREC_FP16_RC;      // the calibration-free mode (round 5; rounds 1-4: JG_PREC_FP16_BC)
    bool bf16 = false;             // precision == JG_PREC_BF16: every launcher comes from the bf16 build (namespace bf)
    bool calib = false;            // calibration pass in progress (bias-corrected layers run hi+lo and record input means: runs_with_lo, gemm())
    int chunk = 32;                // clips per GestSync pass: ~14 GB of workspace per lane at 150 frames; 288 GB of HBM make the whole BASELINE batch one pass
    bool fuse_ln = true;           // residual + LayerNorm in the GEMM epilogue (GestSync post-norm layers)
    bool edge_dedup = true;        // skip the 16 duplicated edge positions of a padded clip
    bool conv1_direct = true;      // fused u8 conv1 kernel (false: stack_frames + implicit GEMM)
    bool qkv0_linear = true;       // layer-0 qkv projection over the distinct conv positions + gather in the attention kernel
    bool ws_poison = false;        // option "ws_poison": fill the workspace with 0xff before every pass (begin_pass; tests)
    bool conv2_row_skip = true;    // conv2 leaves out the leading output rows that the zero-band scan proves to be copies of one row
    engine::ConvReport conv_report;
    std::map<std::string, engine::HostTensor> host;
    EngineOpts opts;               // per-handle tuning switches + per-device resources (shared.h)
    char kname[KNAME_LEN] = {0};   // jg_debug_last_kernel: what the launcher of the last kernel check point's last launch recorded (record_kernel,
                                   // shared.h; the slot is that sink while a check point runs, checks.hip); "" after a refusal or a failure
    engine::Arena ws;
    bool prof = false;
    int prof_only = -1;            // >= 0: only this stage is bracketed with events (jg_profile_enable(h, 2 + stage))
    std::vector<engine::ProfRec> recs;
    double prof_ms[JG_ST_COUNT] = {0};
    int64_t prof_n[JG_ST_COUNT] = {0};

    engine::GestSyncModel gs;
    engine::GestSyncAudioModel gsa;
    engine::JegalModel jg;
    engine::XlmrModel xl;
    // implicit LayerNorm (option "xlmr_fold", read when the XLM-R weights are finalized): the 25 LayerNorms of a pass are never
    // materialised -- see xlmr_encode_folded
    bool xl_fold_opt = true;
    float* feats = nullptr;
    size_t feats_cap = 0;
    // Small host -> device uploads that a call enqueues on its stream (per-clip lengths): a ring of PINNED staging slots, each guarded by
    // an event recorded behind its copy, so a slot is re-used only once that copy has run (pageable vectors kept "alive for
    // seven more parts" relied on the runtime staging pageable copies synchronously and on no caller enqueueing more than eight parts ahead)
    struct StageSlot { int32_t* host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; };
    StageSlot stage_ring[16];
    unsigned stage_next = 0;
    // jg_extract_gesture on two lanes (option "dual_stream"): the batch is split in two (dual_split) and the parts run concurrently on two
    // internal streams with their own workspaces, so that one part's next kernel fills the partly empty last round of the
    // other's (persistent kernels run in rounds of one tile per CU: 788 LayerNorm tiles on 256 CUs are 3.08 rounds)
    bool dual_stream = true;
    bool debug_lanes = false;      // option "debug_lanes": the one-launch check points (checks.hip) launch as inside a two-lane batch (EngineOpts::lanes_active)
    int dual_split = 4;            // the first lane gets dual_split/8 of the batch.  Round 6: equal halves (rounds 3-5: 3/8; with the run-time correction's
                                   // small launches and the split-operand GEMMs in the mix the sweep reads 12.77 ms at 12:20, 12.57 at 14:18, 12.53-12.61 at 16:16,
                                   // 12.57-12.66 at 17:15 / 18:14, 12.66-12.73 at 20:12 -- tools/experiments/README.md)
    std::map<hipStream_t, engine::Arena> ws_parked;      // arenas of the other streams this handle has been bound to (jg_set_stream)
    static constexpr int MAX_LANES = 4;
    hipStream_t lane_stream[MAX_LANES] = {};
    engine::Arena lane_ws[MAX_LANES];
    hipEvent_t lane_ev[MAX_LANES + 1] = {};      // [0]: the caller's stream at entry, [1 + l]: end of lane l
    // fp32 audit path (audit32.hip).  audit_weights: finalize also keeps every matrix in fp32 (always in JG_PREC_FP32); audit_stages: which
    // stages of the path run in fp32 (bit 0 conv stack, 1 GestSync transformer + ff_vid, 2 JEGAL gesture branch, 3 JEGAL content path,
    // 4 XLM-RoBERTa; JG_PREC_FP32 = all of them) -- the stage boundaries are fp32 tensors in every mode, so stages can be mixed
    // round 6: the two ends of the JEGAL gesture branch -- proj_ip_rgb and final norm + proj_op_rgb + the align MLP, five
    // small GEMMs that carry two thirds of the branch's fp16 error -- run on the fp32 kernel in the fp16 contract modes
    bool jegal_fp32_ends = true;
    bool conv_round_diffuse = true;      // conv weights rounded with per-channel error diffusion across the taps (round_matrix, weight_pack.h)
    bool audit_weights = false;
    int audit_stages = 0;
    // diagnosis inside the fp16 JEGAL gesture branch (option "audit_jegal_parts", needs audit_weights): 1 input projection, 2 attention
    // sub-layers, 4 feed-forward sub-layers, 8 final norm + output / align projections run on the fp32 kernels (the residual stream
    // between them is fp32 in every mode)
    int audit_jegal_parts = 0;
    void* comm = nullptr;          // ncclComm_t of this rank (jg_comm_init) or nullptr
    int comm_rank = 0, comm_world = 1;
    // option "xlmr_lanes": jg_xlmr_encode runs a batch as this many equal parts (1..4) on as many streams (default 2).  Round 6 ran it with 1 for
    // a while: with two parts in flight the implicit-LayerNorm pass returned ~1e-2 errors on some sequences of one part in 10-40 % of the runs.
    // Root cause (tools/experiments/xlmr_race/, tools/experiments/pk_opsel_mfma/repro.hip): on this GPU a v_pk_fma_f32 whose low half selects
    // the HIGH register of its second operand (op_sel:[0,1,0], the consumer epilogue's `acc * rstd`) reads that operand as 0 in lanes 48-63
    // while waves of another kernel issue MFMAs on the same SIMD.  The library is built without packed-fp32 instructions since (Makefile, NOPK).
    int xl_lanes = 2;
    // option "lane_priority": 0 = lane streams of normal priority; 1 / 2 = lane 1 / lane 0 of high priority; 3 = both
    // (default since round 6).  The runtime deals streams onto hardware queues per PRIORITY LEVEL (four queues each, in creation order): with
    // normal priority the two lanes can land on ONE queue and then run in turn -- measured with five other streams in the application:
    // 2 076 instead of 2 510 clips/s (tools/experiments/lane_queue_sweep.sh) -- high-priority lanes get queues of their own whatever the
    // application's normal-priority streams are doing (2 503-2 526 clips/s with 0 / 1 / 2 / 3 / 5 / 8 other streams)
    int lane_priority = 3;
};

namespace engine {

#define JG_FAIL(h, code, ...) do { char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__); (h)->err = _b; return (code); } while (0)
#define HIPCHK(h, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) JG_FAIL(h, JG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); } while (0)
#define RET(expr) do { int _r = (expr); if (_r != JG_OK) return _r; } while (0)

// Every entry point runs on the handle's device whatever the caller's current device is, and restores it afterwards:
// workspace allocations, kernel launches and hipFuncSetAttribute all act on the CURRENT device.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// the handle's name slot, emptied, as this thread's record_kernel sink (shared.h) until the scope ends: the kernel check points
// (checks.hip: ENTER_CHECK) and jg_sim_search, whose launch depends on a plan
struct KernelNameScope {
    char* const prev = kernel_name_sink();
    explicit KernelNameScope(char* slot) { slot[0] = 0; kernel_name_sink() = slot; }
    ~KernelNameScope() { kernel_name_sink() = prev; }
    KernelNameScope(const KernelNameScope&) = delete;
};
#define ENTER(h) if (!(h)) return JG_ERR_ARG; engine::DeviceGuard _dg((h)->device); if (!_dg.ok) JG_FAIL(h, JG_ERR_HIP, "hipSetDevice(%d) failed", (h)->device)

// env JG_DEBUG_SYNC, read once per process: synchronise (and report) after every launch
inline bool debug_sync() {
    static const bool on = getenv("JG_DEBUG_SYNC") != nullptr;
    return on;
}

// run a launcher under optional event timing
template <class F>
int timed(jg_handle* h, int stage, F&& f) {
    ProfRec r{stage, nullptr, nullptr};
    const bool prof = h->prof && (h->prof_only < 0 || h->prof_only == stage);
    if (prof) {
        HIPCHK(h, hipEventCreate(&r.e0));
        HIPCHK(h, hipEventCreate(&r.e1));
        HIPCHK(h, hipEventRecord(r.e0, h->stream));
    }
    hipError_t e = f();
    if (e != hipSuccess) JG_FAIL(h, JG_ERR_HIP, "kernel launch failed (stage %s): %s", jg_stage_name(stage), hipGetErrorString(e));
    if (debug_sync()) {                          // fault hunting (env JG_DEBUG_SYNC): name the launch a memory fault belongs to
        static long n = 0;
        std::fprintf(stderr, "[jg] launch %ld (stage %s) ...", ++n, jg_stage_name(stage));
        e = hipStreamSynchronize(h->stream);
        std::fprintf(stderr, " %s\n", e == hipSuccess ? "done" : hipGetErrorString(e));
        if (e != hipSuccess) JG_FAIL(h, JG_ERR_HIP, "launch %ld (stage %s) failed at its synchronisation: %s", n, jg_stage_name(stage), hipGetErrorString(e));
    }
    if (prof) {
        HIPCHK(h, hipEventRecord(r.e1, h->stream));
        h->recs.push_back(r);
    }
    return JG_OK;
}

template <class T>
int walloc(jg_handle* h, Model& m, size_t n, T** out) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, n * sizeof(T) + 256));
    m.allocs.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return JG_OK;
}

template <class T>
int upload(jg_handle* h, Model& m, const std::vector<T>& v, T** out) {
    RET(walloc<T>(h, m, v.size(), out));
    HIPCHK(h, hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return JG_OK;
}

// 16-bit values as the packing leaves them (weight_pack.h: bit containers) -> device operands of the handle's 16-bit type
inline int upload(jg_handle* h, Model& m, const std::vector<uint16_t>& bits, f16** out) {
    RET(walloc<f16>(h, m, bits.size(), out));
    HIPCHK(h, hipMemcpy(*out, bits.data(), bits.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return JG_OK;
}

// Re-finalizing a model (the drivers reload the state_dict on every command) frees that model's previous device
// weights and drops its bias-corrected layers first.
template <class M>
void drop_model(jg_handle* h, M& model) {
    (void)hipStreamSynchronize(h->stream);
    for (void* p : model.m.allocs) (void)hipFree(p);
    model = M();
}

template <class T>
int wsalloc(jg_handle* h, size_t n, T** out) {
    hipError_t e = hipSuccess;
    void* p = h->ws.alloc(n * sizeof(T), &e);
    if (!p) JG_FAIL(h, JG_ERR_HIP, "workspace allocation of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    *out = reinterpret_cast<T*>(p);
    return JG_OK;
}

// Where a workspace pass begins, and the only place: the arena is handed out from its start again, so what pointed into it is void (the
// conv report), and with option ws_poison every chunk is filled with 0xff (fp16 / fp32 NaN) on the handle's stream, in front of the pass's
// kernels -- whatever one of them reads without having written it is NaN, not the previous identical run's value.  The stages of
// one call share one pass (jg_extract_gesture: the JEGAL stage allocates behind the last GestSync chunk's buffers).
inline int begin_pass(jg_handle* h) {
    h->ws.reset();
    h->conv_report.clear();
    if (h->ws_poison)
        for (auto& c : h->ws.chunks) HIPCHK(h, launch_poison(c.p, c.cap, h->stream));
    return JG_OK;
}

// Row-map chain set-up (ConvGeom::rowmap, launch_conv_rowmaps): rm[l], l < n, becomes the compaction map of a conv layer with OH[l] x OW[l]
// outputs per image and conv_skip_decode op op0 + l over NF images -- map, base and the layer's word of one block of totals (rm[0].total)
// come from the workspace.  g (optional, [n]): the layers' geometries, patched to run compacted and to read the rows their producer
// left out from const_in[l].
inline int rowmap_chain(jg_handle* h, long NF, int n, const int* OH, const int* OW, int op0, ConvRowMap* rm, ConvGeom* g = nullptr,
                        const f16* const* const_in = nullptr) {
    int* totals;
    RET(wsalloc(h, (size_t)64, &totals));
    for (int l = 0; l < n; ++l) {
        rm[l].OH = OH[l]; rm[l].OW = OW[l]; rm[l].op = op0 + l;
        RET(wsalloc(h, (size_t)NF * OH[l] * OW[l], &rm[l].map));
        RET(wsalloc(h, (size_t)NF + 1, &rm[l].base));
        rm[l].total = totals + l;
        if (g) {
            g[l].rowmap = rm[l].map; g[l].rows_total = rm[l].total;
            g[l].in_op = rm[l].op - 1; g[l].const_in = const_in ? const_in[l] : nullptr;
        }
    }
    return JG_OK;
}

constexpr int FH = 270, FW = 480;
inline size_t pad128(size_t rows) { return (rows + 127) / 128 * 128; }

// fp32 audit stages (audit32.hip, JG_PREC_FP32 and option audit_stages on a handle finalized with audit_weights)
enum { AUD_CONV = 1, AUD_GS = 2, AUD_JG = 4, AUD_CONTENT = 8, AUD_XLMR = 16, AUD_ALL = 31 };
inline int audit_mask(const jg_handle* h) { return h->precision == JG_PREC_FP32 ? AUD_ALL : h->audit_stages; }

// The lo operand a GEMM on layer L runs with on this handle, or nullptr (weight_form.h, runs_with_lo).  clip_bias: the call takes the
// per-clip bias of a run-time corrected layer
inline const f16* run_lo(const jg_handle* h, const Lin& L, bool clip_bias) {
    return runs_with_lo(L.form, L.uncalibrated, h->calib, clip_bias) ? L.lo : nullptr;
}

// ------------------------------------------------------------------------------------ GEMM calls (linear.hip)
struct Epi {
    const float* scale = nullptr;
    const float* res = nullptr;
    long ldr = 0;
    int res_mod = 0;
    float* out32 = nullptr;
    f16* out16 = nullptr;
    long ldc = 0;
    int relu = 0;
    const LNp* ln = nullptr;      // fused residual + LayerNorm epilogue (when the GEMM can: plan_gemm, gemm_plan.hip)
    int ln_flavour = LN_STD;
    // tiled token stream of the fused GestSync transformer (common.h): residual in / LayerNorm out planes, tiled A operand
    const f16* res16 = nullptr;
    int a_tiled = 0;
    int no_bias = 0;              // the layer's bias is applied elsewhere (layer-0 qkv by linearity: it rides in the projected PE rows)
    // implicit LayerNorm (GemmArgs::ln_mode): ln_stats = (mean, rstd) of the LayerNorm's input rows.  Mode 1: the layer is a folded
    // consumer (Lin::c1h / c1f).  Mode 2: x_hi / x_lo = the token stream's planes (residual in, new rows out, in place),
    // ln_gamma = that LayerNorm's weight (its bias is already part of the layer's packed bias), stat_out = the new rows' partial sums.
    int ln_mode = 0;
    const float* ln_stats = nullptr;
    f16* x_hi = nullptr;
    f16* x_lo = nullptr;
    const float* ln_gamma = nullptr;
    float* stat_out = nullptr;
    int calib_rows = 0;           // calibration pass: only the first calib_rows rows of A are real (0: all M) -- short XLM-R batches are padded to 128 rows
    // JG_PREC_FP16_RC: the M rows are rc_clips clips of rc_rpc rows each (0: no clip structure -> a run-time corrected layer runs hi+lo)
    int rc_rpc = 0, rc_clips = 0;
    const int* rc_valid = nullptr;    // device [rc_clips]: rows of each clip that are its own (jg_gestsync_clip_ragged) or nullptr
};

struct Epi32 {
    const float* res = nullptr;
    long ldr = 0;
    int res_mod = 0;
    int act = 0;          // 0 none, 1 ReLU, 2 exact GELU
};

int gemm(jg_handle* h, int stage, const f16* A, long lda, int M, const Lin& L, const Epi& e, const ConvGeom* g = nullptr);
int gemm32(jg_handle* h, int stage, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e = Epi32(), const ConvGeom* g = nullptr);
int gemm_x3(jg_handle* h, int stage, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e = Epi32());
ConvGeom geom(int H, int W, int C, int KH, int KW, int SH, int SW, int PH, int PW, bool reorder = false);

// ------------------------------------------------------------------------------------ the arithmetic of a model graph (linear.hip)
// A model graph is written once, templated on the element type T of its activations, and takes its arithmetic as a value: Arith<f16> is
// the handle's 16-bit build (gemm() and LAUNCH: fp16, or bf16 on a bf16 handle), Arith<float> the fp32 kernels -- the fp32 MFMA of the
// audit path (gemm32) or, x3, the split operands on the fp16 matrix cores (gemm_x3: the ends of the JEGAL branches in the fp16 contract
// modes).  The residual stream between sub-layers is fp32 in every arithmetic.  One overload per primitive and arithmetic; stage tags:
// a linear layer is JG_ST_CONV with a geometry and JG_ST_GEMM without, the others are what their names say.
template <class T> struct Arith {};
template <> struct Arith<float> { bool x3 = false; };
using A16 = Arith<f16>;
using A32 = Arith<float>;
// out = act(A W^T + b), T activations (act: 0 none, 1 ReLU, 2 exact GELU)
int linear(jg_handle* h, A16 ar, const f16* A, long lda, int M, const Lin& L, f16* out, int act = 0, const ConvGeom* g = nullptr);
int linear(jg_handle* h, A32 ar, const float* A, long lda, int M, const Lin& L, float* out, int act = 0, const ConvGeom* g = nullptr);
// out32 = A W^T + b + res[m % res_mod]: into the fp32 stream (res and out32 may be the same rows) or a stage's fp32 output
int linear_to32(jg_handle* h, A16 ar, const f16* A, long lda, int M, const Lin& L, float* out32, const float* res = nullptr, long ldr = 0, int res_mod = 0);
int linear_to32(jg_handle* h, A32 ar, const float* A, long lda, int M, const Lin& L, float* out32, const float* res = nullptr, long ldr = 0, int res_mod = 0);
// LayerNorm of fp32 rows in ONE launch: the next GEMM's operand `copy` and, optionally, fp32 rows `out32`.  T = float: the operand IS
// the fp32 rows -- the launch writes out32 when given, else copy
int layernorm(jg_handle* h, A16 ar, const float* x, const LNp& ln, int M, int D, int flavour, int relu, f16* copy, float* out32 = nullptr);
int layernorm(jg_handle* h, A32 ar, const float* x, const LNp& ln, int M, int D, int flavour, int relu, float* copy, float* out32 = nullptr);
int attention(jg_handle* h, A16 ar, const f16* qkv, const float* mask, int B, int S, int H, int dk, f16* out);
int attention(jg_handle* h, A32 ar, const float* qkv, const float* mask, int B, int S, int H, int dk, float* out);
// rows beyond each clip's own extent of an NHWC tensor [B][H][row_elems] set to zero (launch_zero_tail); valid == nullptr: nothing to do
int zero_tail(jg_handle* h, A16 ar, f16* x, const int* valid, int halvings, int B, int H, long row_elems);
int zero_tail(jg_handle* h, A32 ar, float* x, const int* valid, int halvings, int B, int H, long row_elems);
// cnn.0 + BatchNorm + ReLU of the audio CNN from fp32 mel frames (B, Tm, F), rows beyond valid[b] zero on both sides of the layer
int audio_conv0(jg_handle* h, A16 ar, const float* mel, int B, int Tm, int F, const Lin& L, const ConvGeom& g, const int* valid, f16* out);
int audio_conv0(jg_handle* h, A32 ar, const float* mel, int B, int Tm, int F, const Lin& L, const ConvGeom& g, const int* valid, float* out);
// a stage's fp32 input of n elements as the arithmetic's operand: a 16-bit copy in the workspace, or the rows themselves
int operand(jg_handle* h, A16 ar, const float* x, long n, const f16** out);
int operand(jg_handle* h, A32 ar, const float* x, long n, const float** out);

// One post-norm layer, x = LN(x + f(x)) (GestSync's unfused plan, XLM-RoBERTa unfolded; torch.nn.TransformerEncoderLayer / the BERT
// layer): x32 the fp32 stream, x its operand copy (T = float: x32 itself), t32 the projections' fp32 output (may be x32: in place);
// the last LayerNorm's fp32 rows go to `out`.  act: the feed-forward activation (1 ReLU, 2 exact GELU).
template <class T>
int post_norm_layer(jg_handle* h, Arith<T> ar, const EncLayer& L, float* x32, T* x, float* t32, T* qkv, T* att, T* hid, const float* mask, int B,
                    int S, int H, int D, int Dff, int act, float* out) {
    const int M = B * S;
    RET(linear(h, ar, x, D, M, L.qkv, qkv));
    RET(attention(h, ar, qkv, mask, B, S, H, D / H, att));
    RET(linear_to32(h, ar, att, D, M, L.out, t32, x32, D));
    RET(layernorm(h, ar, t32, L.n1, M, D, LN_STD, 0, x, x32));
    RET(linear(h, ar, x, D, M, L.ff1, hid, act));
    RET(linear_to32(h, ar, hid, Dff, M, L.ff2, t32, x32, D));
    return layernorm(h, ar, t32, L.n2, M, D, LN_STD, 0, x, out);
}

// ------------------------------------------------------------------------------------ weight packing (linear.hip)
// (layer kinds LK_* and the form each gets under the handle's mode: weight_form.h)
const HostTensor* find(jg_handle* h, const std::string& name);
int need(jg_handle* h, const std::string& name, int64_t numel, const HostTensor** out);
// the one upload step of a packed layer (weight_pack.h): allocations, copies, the Lin, the calibration record
int upload_layer(jg_handle* h, Model& m, PackedLayer&& p, Lin* L);
int pack_matrix(jg_handle* h, Model& m, const std::vector<float>& w, const std::vector<float>& bias, int N, int K, int kind, Lin* L,
                bool ln_consumer = false, bool keep32 = false);
int make_linear(jg_handle* h, Model& m, const std::string& wname, const std::string& bname, int N, int K, Lin* L, int kind = LK_GESTURE, bool keep32 = false);
int make_ln(jg_handle* h, Model& m, const std::string& wname, const std::string& bname, int D, LNp* p);
// Opad > O: output channels O .. Opad - 1 are added with zero weights and zero shift (relu(0) = 0 for whoever reads them)
int make_conv(jg_handle* h, Model& m, const std::string& conv, const std::string& bn, int O, int I, int KT, int KH, int KW,
              int slot, int kpad, Lin* L, int SH = 1, int SW = 1, bool reorder = false, int Opad = 0, int kind = LK_CONV);
// the two halves of make_conv for whoever needs the host result: the folded fp32 matrix and shift alone (GestSync's audio conv1), and
// the packed layer before its upload (GestSync's conv1: the direct kernel's panel is built from it)
int fold_conv(jg_handle* h, const std::string& conv, const std::string& bn, const ConvPack& c, std::vector<float>* p, std::vector<float>* shift);
int pack_conv(jg_handle* h, int model_id, const std::string& conv, const std::string& bn, const ConvPack& c, int kind, PackedLayer* out);
int make_annotated_layer(jg_handle* h, Model& m, const std::string& p, int D, int Dff, EncLayer* L, int kind);
int calibrate_gesture(jg_handle* h, const void* frames, int dtype, int B, int T, int models);
int calibrate_xlmr(jg_handle* h, const int32_t* ids_dev, const int32_t* mask_dev, int B, int L);

// ------------------------------------------------------------------------------------ models (gestsync.hip, gestsync_audio.hip, jegal.hip, xlmr.hip)
int finalize_gestsync(jg_handle* h);
int gs_conv1_stage(jg_handle* h, const void* src, int src_u8, long sb, long st, long sh, long sw, long sc, int nclip, int T, int pad,
                   f16* pooled, bool fill_all, unsigned** zscr);
int gestsync_clip_impl(jg_handle* h, const void* frames, int dtype, int B, int T, float* out_feats, const int32_t* valid_host = nullptr);
int gestsync_windows_impl(jg_handle* h, const float* x, int N, float* out, float* out_conv);
int finalize_gestsync_audio(jg_handle* h);
// src: x (N, 1, 80, 100) (clip_form 0: B = N, T = 1) or mel (B, Tm, 80) (clip_form 1) -> out (B * T, 1024)
int gestsync_audio_impl(jg_handle* h, const float* src, int clip_form, int B, int Tm, int T, const int32_t* valid_host, float* out);
int finalize_jegal(jg_handle* h);
int jegal_gestures_impl(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out);
int plan_track_windows(const int32_t* off, int n_tracks, int win, int ctx, int32_t* table, int cap, int* n_windows, int* span_max);
int jegal_gesture_tracks_impl(jg_handle* h, const float* feats, const int32_t* table_host, int n_windows, int span_max, int rows, int align, float* out);
int jegal_audio_impl(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_host, float* out);
int jegal_text_impl(jg_handle* h, const float* states, const float* mask, int B, int L, float* out);
int fuse_content_impl(jg_handle* h, const float* fused, int rows, float* out);
int finalize_xlmr(jg_handle* h);
int xlmr_encode_impl(jg_handle* h, const int32_t* ids, const int32_t* amask, int B, int L, float* out);

// n int32 values from the host into `dst` (device) on the handle's stream, through the pinned staging ring (api.hip)
int upload_i32_async(jg_handle* h, const int32_t* src, size_t n, int32_t* dst);

}  // namespace engine
