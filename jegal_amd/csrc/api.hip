// libjegal_hip: handle, weight packing and the host-side orchestration of the HIP kernels behind
// the C ABI of include/jegal_hip.h.  Host code only (no kernels here).
#include "common.h"
#define JG_BF16                  // the bf16 build's declarations (namespace bf): same launchers, f16 = __bf16
#include "common.h"
#undef JG_BF16
#include "../../include/jegal_hip.h"
#include "audit32.h"

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

// ---- dispatch between the two kernel builds.  LAUNCH(h, launch_x, args...) calls launch_x of the fp16 build or bf::launch_x of
// the bf16 build (precision mode JG_PREC_BF16): same argument lists, the 16-bit pointers and the structs that carry them are
// layout-identical in both builds and simply re-typed.
[[maybe_unused]] inline const bf::f16* to_bf(const f16* p) { return reinterpret_cast<const bf::f16*>(p); }
inline bf::f16* to_bf(f16* p) { return reinterpret_cast<bf::f16*>(p); }
inline const bf::GemmArgs& to_bf(const GemmArgs& a) { return reinterpret_cast<const bf::GemmArgs&>(a); }
inline const bf::EngineOpts& to_bf(const EngineOpts& o) { return reinterpret_cast<const bf::EngineOpts&>(o); }
static_assert(sizeof(bf::GemmArgs) == sizeof(GemmArgs) && sizeof(bf::EngineOpts) == sizeof(EngineOpts), "the two builds share their argument structs");
template <class T> inline T to_bf(T v) { return v; }
template <class F, class G, class... A>
inline hipError_t dispatch_build(bool bf16, F f, G g, A... a) { return bf16 ? g(to_bf(a)...) : f(a...); }
#define LAUNCH(h, fn, ...) dispatch_build((h)->bf16, fn, bf::fn, __VA_ARGS__)

// fp32 -> bf16 bits, round to nearest even (host side of the weight packing)
inline uint16_t bf16_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
    mutable bool used = false;      // consumed by a finalize (find / need): erased when that finalize is done
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct Lin {            // packed Linear / folded conv:  [N][K] fp16 hi (+lo), fp32 bias
    f16* wh = nullptr;
    f16* wl = nullptr;          // lo part used at run time (W2 modes) or nullptr
    float* bias = nullptr;
    int N = 0, K = 0;
    // bias-corrected mode (JG_PREC_FP16_BC): run-time weights are the single fp16 `wh`; the systematic part of
    // the weight-rounding error, (w - fp16(w)) . E[x], is folded into `bias` after a calibration pass that runs
    // with hi+lo weights (wl_calib) and records the per-channel mean of this layer's input (mu).
    bool bc = false;
    // run-time corrected mode (JG_PREC_FP16_RC; GestSync transformer Linears): single fp16 `wh` + a per-clip bias built from the clip's own
    // rows and the lo part (`wl_calib`), see gemm(); wherever that epilogue is not available the GEMM runs hi+lo instead
    bool rc = false;
    bool bc_pending = false;    // LK_XLMR: no calibration yet -- the run-time GEMM keeps using hi+lo (wl == wl_calib); jg_calibrate_xlmr clears it
    f16* wl_calib = nullptr;
    float* mu = nullptr;        // device [K]: column sums of the A operand seen during calibration
    long mu_rows = 0;
    int model = 0;              // 1 GestSync, 2 JEGAL (which finalize owns this layer)
    std::vector<float> w32, b32;
    // Linear behind an IMPLICIT LayerNorm (GemmArgs::ln_mode 1): w32 / wh / wl hold W . diag(gamma), b32 / bias hold b + W beta, and
    // c1h / c1f [N] the column sums of the packed weights -- of `wh` alone (single-fp16 runs: the GEMM then is exactly
    // sum_k wh[n][k] (x[k] - mean) rstd, and the bias correction covers the lo part) and of wh + lo (hi+lo runs)
    float* c1h = nullptr;
    float* c1f = nullptr;
    // fp32 audit path (JG_PREC_FP32 / option audit_weights; audit32.hip): the fp32 matrix [N][K] as packed (BatchNorm folded, same k order as
    // wh) and the layer's own fp32 bias (`bias` above may carry a calibration's correction)
    float* w32d = nullptr;
    float* b32d = nullptr;
};
struct LNp { float* w = nullptr; float* b = nullptr; };

struct EncLayer { Lin qkv, out, ff1, ff2; LNp n1, n2; };

struct Arena {          // stream-ordered bump allocator over persistent chunks
    struct Chunk { char* p; size_t cap; };
    std::vector<Chunk> chunks;
    size_t cur = 0, off = 0;
    void reset() { cur = 0; off = 0; }
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
    void release() { for (auto& c : chunks) (void)hipFree(c.p); chunks.clear(); reset(); }
};

struct ProfRec { int stage; hipEvent_t e0, e1; };

// ---- RCCL, bound at run time (jg_comm_* / jg_allgather / jg_allreduce_sum_i64): the library has no link-time dependency on librccl -- a
// single-GPU consumer never loads it; inside a PyTorch process dlopen returns the copy torch already mapped (same SONAME).
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void* id) = nullptr;
    void* CommInitRank = nullptr;      // takes ncclUniqueId BY VALUE: cast at the call site (jg_comm_init)
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
struct NcclId { char internal[128]; };          // layout of ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES)
inline Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            x.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (x.lib) break;
        }
        if (!x.lib) return x;
        x.GetUniqueId = reinterpret_cast<int (*)(void*)>(dlsym(x.lib, "ncclGetUniqueId"));
        x.CommInitRank = dlsym(x.lib, "ncclCommInitRank");
        x.AllGather = reinterpret_cast<int (*)(const void*, void*, size_t, int, void*, hipStream_t)>(dlsym(x.lib, "ncclAllGather"));
        x.AllReduce = reinterpret_cast<int (*)(const void*, void*, size_t, int, int, void*, hipStream_t)>(dlsym(x.lib, "ncclAllReduce"));
        x.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(x.lib, "ncclCommDestroy"));
        x.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(x.lib, "ncclGetErrorString"));
        x.ok = x.GetUniqueId && x.CommInitRank && x.AllGather && x.AllReduce && x.CommDestroy;
        return x;
    }();
    return r;
}

}  // namespace

struct jg_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    std::string err;
    int precision = JG_PREC_FP16_RC;      // the calibration-free mode (round 5; rounds 1-4: JG_PREC_FP16_BC)
    bool bf16 = false;             // precision == JG_PREC_BF16: every launcher comes from the bf16 build (namespace bf)
    bool calib = false;            // calibration pass in progress (bc layers use hi+lo and record input means)
    bool gs_calibrated = false, jg_calibrated = false;
    std::vector<Lin*> bc_layers;   // bias-corrected layers of both models (entries of a model are dropped on its re-finalize)
    int chunk = 32;                // clips per GestSync pass: ~14 GB of workspace per lane at 150 frames; 288 GB of HBM make the whole BASELINE batch one pass
    bool fuse_ln = true;           // residual + LayerNorm in the GEMM epilogue (GestSync post-norm layers)
    bool edge_dedup = true;        // skip the 16 duplicated edge positions of a padded clip
    bool conv1_direct = true;      // fused u8 conv1 kernel (false: stack_frames + implicit GEMM)
    f16* gs_qpe = nullptr;         // [21][1536]: layer-0 W_qkv pe[j] + b (Qkv0); recomputed when weights or bias corrections change
    bool gs_qpe_valid = false;
    bool qkv0_linear = true;       // layer-0 qkv projection over the distinct conv positions + gather in the attention kernel
    bool ws_poison = false;        // option "ws_poison": fill the workspace with 0xff before every clip chunk (tests)
    bool conv2_row_skip = true;    // conv2 leaves out the leading output rows that the zero-band scan proves to be copies of one row
    const int* last_rowskip = nullptr;   // device word: min over the last conv stack's positions of conv2's row skip (jg_debug_conv2_rowskip)
    const int* last_conv_totals = nullptr;   // device [4]: rows conv2 .. conv5 of the last conv stack computed (jg_debug_conv_rows)
    long last_conv_full[4] = {0, 0, 0, 0};   // ... of these many
    std::map<std::string, HostTensor> host;
    std::vector<void*> wallocs_gs, wallocs_jg;   // device weights of the GestSync / JEGAL model (freed on re-finalize)
    std::vector<void*>* wallocs = &wallocs_gs;   // list the model being finalized allocates into
    int cur_model = 1;
    EngineOpts opts;               // per-handle tuning switches + per-device resources (common.h)
    char kname[KNAME_LEN] = {0};   // instance the last kernel check point launched (jg_debug_last_kernel)
    Arena ws;
    bool prof = false;
    int prof_only = -1;            // >= 0: only this stage is bracketed with events (jg_profile_enable(h, 2 + stage))
    std::vector<ProfRec> recs;
    double prof_ms[JG_ST_COUNT] = {0};
    int64_t prof_n[JG_ST_COUNT] = {0};

    // GestSync
    bool gs_ready = false;
    Lin c1, c2, c3, c4, c5, fc6, ff0, ff2;
    // const chain: what conv2 / conv3 / conv4 compute from an all-constant pooled image (relu(bias1) everywhere) -- the rows of
    // their outputs that the zero-band skip makes position-independent are read from here (ConvGeom::const_in); 4 copies each
    f16 *gs_c2C = nullptr, *gs_c3C = nullptr, *gs_c4C = nullptr, *gs_c5C = nullptr;
    float* c1_scale255 = nullptr;
    f16* c1_direct = nullptr;      // conv1 weights, slot-major [49][64][16] for the direct kernel
    float* gs_pe = nullptr;
    EncLayer gs_layers[6];
    // JEGAL
    bool jg_ready = false;
    Lin ip0, ip3, op_rgb, al_g0, al_g2, fu0, fu2, al_c0, al_c2, op_text, op_audio;
    LNp ip_ln, rgb_norm, text_norm;
    float* rgb_pe = nullptr;
    EncLayer rgb_layers[6], text_layers[3];
    // XLM-RoBERTa text front end (third-party transformers.XLMRobertaModel, call site jegal.py:116-129)
    bool xl_ready = false;
    int xl_layers_n = 0, xl_vocab = 0, xl_maxpos = 0;
    float *xl_word = nullptr, *xl_pos = nullptr, *xl_type = nullptr;
    LNp xl_emb_ln;
    std::vector<EncLayer> xl_layers;
    // implicit LayerNorm (option "xlmr_fold", read when the XLM-R weights are finalized): the 25 LayerNorms of a pass are never
    // materialised -- see xlmr_encode_folded
    bool xl_fold_opt = true, xl_folded = false;
    std::vector<void*> wallocs_xl;
    Lin a0, a3, a6, a9, a12, a15;
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
    int dual_split = 4;            // the first lane gets dual_split/8 of the batch.  Round 6: equal halves (rounds 3-5: 3/8; with the run-time correction's
                                   // small launches and the split-operand GEMMs in the mix the sweep reads 12.77 ms at 12:20, 12.57 at 14:18, 12.53-12.61 at 16:16,
                                   // 12.57-12.66 at 17:15 / 18:14, 12.66-12.73 at 20:12 -- tools/experiments/README.md)
    std::map<hipStream_t, Arena> ws_parked;      // arenas of the other streams this handle has been bound to (jg_set_stream)
    static constexpr int MAX_LANES = 4;
    hipStream_t lane_stream[MAX_LANES] = {};
    Arena lane_ws[MAX_LANES];
    hipEvent_t lane_ev[MAX_LANES + 1] = {};      // [0]: the caller's stream at entry, [1 + l]: end of lane l
    // fp32 audit path (audit32.hip).  audit_weights: finalize also keeps every matrix in fp32 (always in JG_PREC_FP32); audit_stages: which
    // stages of the path run in fp32 (bit 0 conv stack, 1 GestSync transformer + ff_vid, 2 JEGAL gesture branch, 3 JEGAL content path,
    // 4 XLM-RoBERTa; JG_PREC_FP32 = all of them) -- the stage boundaries are fp32 tensors in every mode, so stages can be mixed
    // round 6: the two ends of the JEGAL gesture branch -- proj_ip_rgb and final norm + proj_op_rgb + the align MLP, five
    // small GEMMs that carry two thirds of the branch's fp16 error -- run on the fp32 kernel in the fp16 contract modes
    bool jegal_fp32_ends = true;
    bool conv_round_diffuse = true;      // conv weights rounded with per-channel error diffusion across the taps (pack_matrix)
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

namespace {

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
#define ENTER(h) if (!(h)) return JG_ERR_ARG; DeviceGuard _dg((h)->device); if (!_dg.ok) JG_FAIL(h, JG_ERR_HIP, "hipSetDevice(%d) failed", (h)->device)

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
int walloc(jg_handle* h, size_t n, T** out) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, n * sizeof(T) + 256));
    h->wallocs->push_back(p);
    *out = reinterpret_cast<T*>(p);
    return JG_OK;
}

template <class T>
int upload(jg_handle* h, const std::vector<T>& v, T** out) {
    RET(walloc<T>(h, v.size(), out));
    HIPCHK(h, hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return JG_OK;
}

template <class T>
int wsalloc(jg_handle* h, size_t n, T** out) {
    hipError_t e = hipSuccess;
    void* p = h->ws.alloc(n * sizeof(T), &e);
    if (!p) JG_FAIL(h, JG_ERR_HIP, "workspace allocation of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    *out = reinterpret_cast<T*>(p);
    return JG_OK;
}

// n int32 values from the host into `dst` (device) on the handle's stream, through the pinned staging ring (jg_handle::stage_ring)
int upload_i32_async(jg_handle* h, const int32_t* src, size_t n, int32_t* dst) {
    jg_handle::StageSlot& sl = h->stage_ring[h->stage_next++ & 15];
    if (sl.pending) { HIPCHK(h, hipEventSynchronize(sl.ev)); sl.pending = false; }
    if (!sl.ev) HIPCHK(h, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.cap < n) {
        if (sl.host) HIPCHK(h, hipHostFree(sl.host));
        sl.host = nullptr; sl.cap = 0;
        const size_t cap = n < 256 ? 256 : n;
        HIPCHK(h, hipHostMalloc(reinterpret_cast<void**>(&sl.host), cap * sizeof(int32_t), hipHostMallocDefault));
        sl.cap = cap;
    }
    std::memcpy(sl.host, src, n * sizeof(int32_t));
    HIPCHK(h, hipMemcpyAsync(dst, sl.host, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(sl.ev, h->stream));
    sl.pending = true;
    return JG_OK;
}

const HostTensor* find(jg_handle* h, const std::string& name) {
    auto it = h->host.find(name);
    if (it == h->host.end()) return nullptr;
    it->second.used = true;
    return &it->second;
}

int need(jg_handle* h, const std::string& name, int64_t numel, const HostTensor** out) {
    const HostTensor* t = find(h, name);
    if (!t) JG_FAIL(h, JG_ERR_WEIGHT, "missing weight '%s' (strict load)", name.c_str());
    if (t->numel() != numel) JG_FAIL(h, JG_ERR_WEIGHT, "weight '%s' has %lld elements, expected %lld", name.c_str(), (long long)t->numel(), (long long)numel);
    *out = t;
    return JG_OK;
}

// [N][K] fp32 -> device fp16 hi (+lo)
// layer kinds: which precision treatment a matrix gets under the handle's mode
enum { LK_CONV = 0, LK_GESTURE = 1, LK_CONTENT = 2, LK_XLMR = 3 };      // LK_XLMR: bias-corrected like the gesture path (calibrated on token ids)

// keep32: the layer also runs on the fp32 kernel in the fp16 modes (the two ends of the JEGAL gesture branch, option jegal_fp32_ends)
// diffuse_group > 0 (conv layers, option conv_round_diffuse): fp16 rounding with ERROR DIFFUSION along the taps of one (output channel,
// input slot) pair -- k = tap * diffuse_group + slot -- instead of round-to-nearest per weight: the residuals w - fp16(w) of a
// channel's taps then sum to less than half an ulp, so the part of the weight-rounding error that is the same for every output pixel,
// sum_k (w - fp16(w))[k] E[x_k] = sum_slot E[x_slot] sum_taps (w - fp16(w)), vanishes wherever the input statistics do not depend on the
// tap (everywhere but at the image border); the price is a per-weight residual of up to one ulp instead of half an ulp in the part
// that averages out over pixels.  No calibration, no run-time cost (measured with tools/precision_floor.py).
int pack_matrix(jg_handle* h, const std::vector<float>& w, const std::vector<float>& bias, int N, int K, int kind, Lin* L, bool ln_consumer = false,
                bool keep32 = false, int diffuse_group = 0) {
    const int mode = h->precision;
    // JG_PREC_FP16_RC: GestSync's Linears (model 1) are run-time corrected; the JEGAL gesture branch (M = B*T rows: launch-bound, a
    // 256-row tile meets several clips) and the content path keep hi+lo; XLM-RoBERTa as in JG_PREC_FP16_BC (hi+lo until calibrated)
    const bool rcm = mode == JG_PREC_FP16_RC;
    const bool rc = rcm && kind == LK_GESTURE && h->cur_model == 1;
    const bool bc = (mode == JG_PREC_FP16_BC && (kind == LK_GESTURE || kind == LK_XLMR)) || (rcm && kind == LK_XLMR);
    const bool split = kind == LK_CONV ? mode == JG_PREC_FP16_W2_ALL
                                       : (mode == JG_PREC_FP16_W2 || mode == JG_PREC_FP16_W2_ALL || (mode == JG_PREC_FP16_BC && kind == LK_CONTENT) ||
                                          (rcm && !rc && kind != LK_XLMR));
    std::vector<f16> hi((size_t)N * K), lo;
    const bool want_lo = split || bc || rc || keep32;
    if (want_lo) lo.resize((size_t)N * K);
    if (h->bf16) {                       // JG_PREC_BF16: single bf16 weights (the 16-bit container is re-typed by the bf16 build)
        for (size_t i = 0; i < hi.size(); ++i) {
            const uint16_t b = bf16_bits(w[i]);
            std::memcpy(&hi[i], &b, 2);
        }
    } else if (diffuse_group > 0 && K % diffuse_group == 0 && !(split || bc || rc)) {
        const int taps = K / diffuse_group;
        for (int n = 0; n < N; ++n)
            for (int sl = 0; sl < diffuse_group; ++sl) {
                double carry = 0.0;
                for (int t = 0; t < taps; ++t) {
                    const size_t i = (size_t)n * K + (size_t)t * diffuse_group + sl;
                    if (w[i] == 0.f) { hi[i] = (f16)0.f; continue; }        // padding slots stay exactly zero
                    const double v = (double)w[i] + carry;
                    const f16 a = (f16)(float)v;
                    hi[i] = a;
                    carry = v - (double)(float)a;
                }
            }
    } else {
        for (size_t i = 0; i < hi.size(); ++i) {
            const f16 a = (f16)w[i];
            hi[i] = a;
            if (want_lo) lo[i] = (f16)(w[i] - (float)a);
        }
    }
    L->N = N; L->K = K;
    L->model = h->cur_model;
    L->c1h = L->c1f = nullptr;
    if (ln_consumer) {            // column sums of the weights AS PACKED (Lin::c1h / c1f)
        std::vector<float> c1h(N), c1f(N);
        for (int n = 0; n < N; ++n) {
            double sh = 0.0, sl = 0.0;
            for (int k = 0; k < K; ++k) {
                const size_t i = (size_t)n * K + k;
                if (h->bf16) {
                    uint16_t b;
                    std::memcpy(&b, &hi[i], 2);
                    const uint32_t u = (uint32_t)b << 16;
                    float f;
                    std::memcpy(&f, &u, 4);
                    sh += (double)f;
                } else {
                    sh += (double)(float)hi[i];
                    if (!lo.empty()) sl += (double)(float)lo[i];
                }
            }
            c1h[n] = (float)sh;
            c1f[n] = (float)(sh + sl);
        }
        RET(upload(h, c1h, &L->c1h));
        RET(upload(h, c1f, &L->c1f));
    }
    RET(upload(h, hi, &L->wh));
    L->wl = nullptr;
    if (split) RET(upload(h, lo, &L->wl));
    RET(upload(h, bias, &L->bias));
    L->w32d = L->b32d = nullptr;
    if (h->audit_weights || h->precision == JG_PREC_FP32 || keep32) {
        RET(upload(h, w, &L->w32d));
        RET(upload(h, bias, &L->b32d));
    }
    L->bc = bc;
    L->rc = rc;
    L->bc_pending = false;
    if (rc) RET(upload(h, lo, &L->wl_calib));
    if (keep32 && !split && !bc && !rc) RET(upload(h, lo, &L->wl_calib));      // the lo half for the split-operand kernel (gemm_x3)
    if (bc) {
        RET(upload(h, lo, &L->wl_calib));
        RET(walloc<float>(h, (size_t)K, &L->mu));
        L->w32 = w;
        L->b32 = bias;
        h->bc_layers.push_back(L);
        // XLM-RoBERTa: calibration-free hi+lo until jg_calibrate_xlmr has seen the caller's token ids (the released checkpoint has
        // strong outlier activation dimensions; bias corrections recorded on made-up ids were never validated for it)
        if (kind == LK_XLMR) { L->wl = L->wl_calib; L->bc_pending = true; }
    }
    return JG_OK;
}

int make_linear(jg_handle* h, const std::string& wname, const std::string& bname, int N, int K, Lin* L, int kind = LK_GESTURE, bool keep32 = false) {
    const HostTensor *w, *b;
    RET(need(h, wname, (int64_t)N * K, &w));
    RET(need(h, bname, N, &b));
    return pack_matrix(h, w->v, b->v, N, K, kind, L, false, keep32);
}

int make_ln(jg_handle* h, const std::string& wname, const std::string& bname, int D, LNp* p) {
    const HostTensor *w, *b;
    RET(need(h, wname, D, &w));
    RET(need(h, bname, D, &b));
    RET(upload(h, w->v, &p->w));
    RET(upload(h, b->v, &p->b));
    return JG_OK;
}

// conv weight [O][I][KT][KH][KW] (+ optional eval BatchNorm) -> [O][Kpad] with k = ((kh*KW+kw)*slot + (kt*I + c)),
// slot = channels per (kh,kw) position after padding (16 for conv1's 5x3 temporal stack, I otherwise).
// Tap order of a conv layer's K axis: natural (kh, kw) or, for strided layers run with `reorder`, grouped by
// parity class (kh % SH, kw % SW) -- see ConvGeom::taps.  Used by BOTH the weight packing and the geometry.
std::vector<std::pair<int, int>> tap_order(int KH, int KW, int SH, int SW, bool reorder) {
    std::vector<std::pair<int, int>> t;
    if (!reorder || KH * KW > 32) {
        for (int kh = 0; kh < KH; ++kh)
            for (int kw = 0; kw < KW; ++kw) t.push_back({kh, kw});
        return t;
    }
    for (int ph = 0; ph < SH; ++ph)
        for (int pw = 0; pw < SW; ++pw)
            for (int kh = ph; kh < KH; kh += SH)
                for (int kw = pw; kw < KW; kw += SW) t.push_back({kh, kw});
    return t;
}

int make_conv(jg_handle* h, const std::string& conv, const std::string& bn, int O, int I, int KT, int KH, int KW,
              int slot, int kpad, Lin* L, int SH = 1, int SW = 1, bool reorder = false) {
    const HostTensor *w, *b;
    RET(need(h, conv + ".weight", (int64_t)O * I * KT * KH * KW, &w));
    RET(need(h, conv + ".bias", O, &b));
    std::vector<float> s(O, 1.f), shift(b->v);
    if (!bn.empty()) {
        const HostTensor *g, *be, *mu, *var;
        RET(need(h, bn + ".weight", O, &g));
        RET(need(h, bn + ".bias", O, &be));
        RET(need(h, bn + ".running_mean", O, &mu));
        RET(need(h, bn + ".running_var", O, &var));
        for (int o = 0; o < O; ++o) {
            s[o] = g->v[o] / std::sqrt(var->v[o] + 1e-5f);
            shift[o] = (b->v[o] - mu->v[o]) * s[o] + be->v[o];
        }
    }
    const int K = kpad > 0 ? kpad : KH * KW * slot;
    std::vector<float> p((size_t)O * K, 0.f);
    const auto order = tap_order(KH, KW, SH, SW, reorder);
    for (int o = 0; o < O; ++o)
        for (int c = 0; c < I; ++c)
            for (int kt = 0; kt < KT; ++kt)
                for (size_t t = 0; t < order.size(); ++t) {
                    const int kh = order[t].first, kw = order[t].second;
                    const float v = w->v[((((size_t)o * I + c) * KT + kt) * KH + kh) * KW + kw] * s[o];
                    p[(size_t)o * K + t * slot + kt * I + c] = v;
                }
    return pack_matrix(h, p, shift, O, K, LK_CONV, L, false, false, h->conv_round_diffuse ? slot : 0);
}

int make_annotated_layer(jg_handle* h, const std::string& p, int D, int Dff, EncLayer* L, int kind) {
    // pack linears.0/1/2 (q,k,v) into one [3D][D] projection (modules.py:108-110)
    std::vector<float> w((size_t)3 * D * D), b((size_t)3 * D);
    for (int i = 0; i < 3; ++i) {
        const HostTensor *wi, *bi;
        RET(need(h, p + ".self_attn.linears." + std::to_string(i) + ".weight", (int64_t)D * D, &wi));
        RET(need(h, p + ".self_attn.linears." + std::to_string(i) + ".bias", D, &bi));
        std::memcpy(&w[(size_t)i * D * D], wi->v.data(), sizeof(float) * D * D);
        std::memcpy(&b[(size_t)i * D], bi->v.data(), sizeof(float) * D);
    }
    RET(pack_matrix(h, w, b, 3 * D, D, kind, &L->qkv));
    RET(make_linear(h, p + ".self_attn.linears.3.weight", p + ".self_attn.linears.3.bias", D, D, &L->out, kind));
    RET(make_linear(h, p + ".feed_forward.w_1.weight", p + ".feed_forward.w_1.bias", Dff, D, &L->ff1, kind));
    RET(make_linear(h, p + ".feed_forward.w_2.weight", p + ".feed_forward.w_2.bias", D, Dff, &L->ff2, kind));
    RET(make_ln(h, p + ".sublayer.0.norm.a_2", p + ".sublayer.0.norm.b_2", D, &L->n1));
    RET(make_ln(h, p + ".sublayer.1.norm.a_2", p + ".sublayer.1.norm.b_2", D, &L->n2));
    return JG_OK;
}

// Re-finalizing a model (the drivers reload the state_dict on every command) frees that model's previous device
// weights and drops its bias-corrected layers from the calibration list first.
void drop_model(jg_handle* h, std::vector<void*>& allocs, int model) {
    (void)hipStreamSynchronize(h->stream);
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    std::vector<Lin*> keep;
    for (Lin* L : h->bc_layers)
        if (L->model != model) keep.push_back(L);
    h->bc_layers.swap(keep);
    h->cur_model = model;
}

int finalize_gestsync(jg_handle* h) {
    h->gs_ready = false;
    h->gs_calibrated = false;
    drop_model(h, h->wallocs_gs, 1);
    h->c1 = h->c2 = h->c3 = h->c4 = h->c5 = h->fc6 = h->ff0 = h->ff2 = Lin();
    for (auto& L : h->gs_layers) L = EncLayer();
    h->wallocs = &h->wallocs_gs;
    RET(make_conv(h, "net_vid.conv1", "net_vid.bn1", 64, 3, 5, 7, 7, 16, 0, &h->c1));
    // conv2..conv5: taps grouped by stride parity class (ConvGeom::taps); gs_conv_stack builds the same geometry
    RET(make_conv(h, "net_vid.conv2", "net_vid.bn2", 128, 64, 1, 5, 5, 64, 0, &h->c2, 2, 2, true));
    RET(make_conv(h, "net_vid.conv3", "net_vid.bn3", 256, 128, 1, 3, 3, 128, 0, &h->c3, 2, 2, true));
    RET(make_conv(h, "net_vid.conv4", "net_vid.bn4", 256, 256, 1, 3, 3, 256, 0, &h->c4, 1, 2, true));
    RET(make_conv(h, "net_vid.conv5", "net_vid.bn5", 256, 256, 1, 3, 3, 256, 0, &h->c5, 1, 1, true));
    RET(make_conv(h, "net_vid.fc6", "net_vid.bn6", 512, 256, 1, 4, 4, 256, 0, &h->fc6));
    RET(upload(h, std::vector<float>(64, 1.0f / 255.0f), &h->c1_scale255));
    if (!h->bf16) {   // slot-major copy of the packed conv1 panel for conv1_direct_kernel: Wd[s][o][e] = W[o][s*16+e]
        std::vector<f16> hostw((size_t)64 * 784), wd((size_t)49 * 64 * 16);
        HIPCHK(h, hipMemcpy(hostw.data(), h->c1.wh, hostw.size() * sizeof(f16), hipMemcpyDeviceToHost));
        for (int s = 0; s < 49; ++s)
            for (int o = 0; o < 64; ++o)
                for (int e = 0; e < 16; ++e) wd[((size_t)s * 64 + o) * 16 + e] = hostw[(size_t)o * 784 + s * 16 + e];
        // bias lane: the kernel sets element 15 of every pixel slot to 1.0; shift*255 as hi+lo fp16 pair
        std::vector<float> shift(64);
        HIPCHK(h, hipMemcpy(shift.data(), h->c1.bias, 64 * sizeof(float), hipMemcpyDeviceToHost));
        for (int o = 0; o < 64; ++o) {
            const float v = shift[o] * 255.0f;
            const f16 hi = (f16)v;
            wd[((size_t)0 * 64 + o) * 16 + 15] = hi;
            wd[((size_t)1 * 64 + o) * 16 + 15] = (f16)(v - (float)hi);
        }
        RET(upload(h, wd, &h->c1_direct));
    }
    RET(make_linear(h, "ff_vid.0.weight", "ff_vid.0.bias", 512, 512, &h->ff0));
    RET(make_linear(h, "ff_vid.2.weight", "ff_vid.2.bias", 1024, 512, &h->ff2));
    const HostTensor* pe;
    RET(need(h, "pos_encoder.pe", 50 * 512, &pe));
    RET(upload(h, pe->v, &h->gs_pe));
    for (int l = 0; l < 6; ++l) {
        const std::string p = "transformer_encoder.layers." + std::to_string(l);
        EncLayer* L = &h->gs_layers[l];
        RET(make_linear(h, p + ".self_attn.in_proj_weight", p + ".self_attn.in_proj_bias", 1536, 512, &L->qkv));
        RET(make_linear(h, p + ".self_attn.out_proj.weight", p + ".self_attn.out_proj.bias", 512, 512, &L->out));
        RET(make_linear(h, p + ".linear1.weight", p + ".linear1.bias", 2048, 512, &L->ff1));
        RET(make_linear(h, p + ".linear2.weight", p + ".linear2.bias", 512, 2048, &L->ff2));
        RET(make_ln(h, p + ".norm1.weight", p + ".norm1.bias", 512, &L->n1));
        RET(make_ln(h, p + ".norm2.weight", p + ".norm2.bias", 512, &L->n2));
    }
    h->gs_ready = true;
    return JG_OK;
}

int finalize_jegal(jg_handle* h) {
    h->jg_ready = false;
    h->jg_calibrated = false;
    drop_model(h, h->wallocs_jg, 2);
    h->ip0 = h->ip3 = h->op_rgb = h->al_g0 = h->al_g2 = h->fu0 = h->fu2 = h->al_c0 = h->al_c2 = h->op_text = h->op_audio = Lin();
    h->a0 = h->a3 = h->a6 = h->a9 = h->a12 = h->a15 = Lin();
    for (auto& L : h->rgb_layers) L = EncLayer();
    for (auto& L : h->text_layers) L = EncLayer();
    h->wallocs = &h->wallocs_jg;
    // The input projection keeps hi+lo weights in the bias-corrected mode too: the zero-padded rows of a ragged batch
    // (dataset.py:336-340) reach it as x = 0 exactly, where a bias correction (w - fp16(w)).E[x] would be pure error -- the
    // reference computes those rows as well (callers strip them).  Two small GEMMs of the 50 in the branch.
    RET(make_linear(h, "proj_ip_rgb.0.weight", "proj_ip_rgb.0.bias", 512, 1024, &h->ip0, LK_CONTENT, true));
    RET(make_ln(h, "proj_ip_rgb.1.weight", "proj_ip_rgb.1.bias", 512, &h->ip_ln));
    RET(make_linear(h, "proj_ip_rgb.3.weight", "proj_ip_rgb.3.bias", 512, 512, &h->ip3, LK_CONTENT, true));
    const HostTensor* pe;
    RET(need(h, "position_rgb.pe", 500 * 512, &pe));
    RET(upload(h, pe->v, &h->rgb_pe));
    for (int l = 0; l < 6; ++l) RET(make_annotated_layer(h, "encoder_rgb.layers." + std::to_string(l), 512, 2048, &h->rgb_layers[l], LK_GESTURE));
    RET(make_ln(h, "encoder_rgb.norm.a_2", "encoder_rgb.norm.b_2", 512, &h->rgb_norm));
    RET(make_linear(h, "proj_op_rgb.weight", "proj_op_rgb.bias", 512, 512, &h->op_rgb, LK_GESTURE, true));
    for (int l = 0; l < 3; ++l) RET(make_annotated_layer(h, "encoder_text.layers." + std::to_string(l), 768, 3072, &h->text_layers[l], LK_CONTENT));
    RET(make_ln(h, "encoder_text.norm.a_2", "encoder_text.norm.b_2", 768, &h->text_norm));
    RET(make_linear(h, "proj_op_text.weight", "proj_op_text.bias", 256, 768, &h->op_text, LK_CONTENT));
    RET(make_conv(h, "cnn.0", "cnn.1", 32, 1, 1, 5, 5, 1, 32, &h->a0));
    RET(make_conv(h, "cnn.3", "cnn.4", 64, 32, 1, 3, 3, 32, 0, &h->a3));
    RET(make_conv(h, "cnn.6", "cnn.7", 128, 64, 1, 3, 3, 64, 0, &h->a6));
    RET(make_conv(h, "cnn.9", "cnn.10", 256, 128, 1, 3, 3, 128, 0, &h->a9));
    RET(make_conv(h, "cnn.12", "cnn.13", 256, 256, 1, 3, 3, 256, 0, &h->a12));
    RET(make_conv(h, "cnn.15", "", 256, 256, 1, 1, 1, 256, 0, &h->a15));
    RET(make_linear(h, "proj_op_audio.weight", "proj_op_audio.bias", 256, 256, &h->op_audio, LK_CONTENT));
    RET(make_linear(h, "proj_op_fusion_content.0.weight", "proj_op_fusion_content.0.bias", 512, 512, &h->fu0, LK_CONTENT));
    RET(make_linear(h, "proj_op_fusion_content.2.weight", "proj_op_fusion_content.2.bias", 512, 512, &h->fu2, LK_CONTENT));
    RET(make_linear(h, "proj_op_align_gesture.0.weight", "proj_op_align_gesture.0.bias", 512, 512, &h->al_g0, LK_GESTURE, true));
    RET(make_linear(h, "proj_op_align_gesture.2.weight", "proj_op_align_gesture.2.bias", 512, 512, &h->al_g2, LK_GESTURE, true));
    RET(make_linear(h, "proj_op_align_content.0.weight", "proj_op_align_content.0.bias", 512, 512, &h->al_c0, LK_CONTENT));
    RET(make_linear(h, "proj_op_align_content.2.weight", "proj_op_align_content.2.bias", 512, 512, &h->al_c2, LK_CONTENT));
    h->jg_ready = true;
    return JG_OK;
}

// ------------------------------------------------------------------------------------ GEMM helpers
struct Epi {
    const float* scale = nullptr;
    const float* res = nullptr;
    long ldr = 0;
    int res_mod = 0;
    float* out32 = nullptr;
    f16* out16 = nullptr;
    long ldc = 0;
    int relu = 0;
    const LNp* ln = nullptr;      // fused residual + LayerNorm epilogue (when the GEMM can: see gemm_ln_fusable)
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

int gemm(jg_handle* h, int stage, const f16* A, long lda, int M, const Lin& L, const Epi& e, const ConvGeom* g = nullptr) {
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda;
    if (g) a.g = *g;
    a.Wh = L.wh; a.Wl = (h->calib && L.bc) ? L.wl_calib : L.wl; a.ldw = L.K;
    const bool conv = g != nullptr;
    if (L.rc) {
        // run-time correction: bias_clip = bias + lo . (mean of a sample of the clip's own rows), two small launches in front of the GEMM;
        // only the LDS-DMA kernel's fp16-row and LayerNorm-fused epilogues take it (launch_gemm), everything else runs hi+lo
        const bool ln_fused = e.ln && e.res16;
        const bool rows16 = e.out16 && !e.out32 && !e.res && !e.ln;
        const bool can = !conv && !e.ln_mode && !e.no_bias && h->opts.gemm_glds && e.rc_rpc >= 256 && e.rc_clips > 0 && (long)e.rc_rpc * e.rc_clips == M &&
                         M >= 1024 && (L.K == 512 || L.K == 2048) && L.N % 128 == 0 && (ln_fused || rows16) && (!e.a_tiled || L.K == 512);
        if (can) {
            float *scr, *bc;
            RET(wsalloc(h, rc_scratch_elems(e.rc_clips, L.K), &scr));
            RET(wsalloc(h, (size_t)e.rc_clips * L.N, &bc));
            RET(timed(h, JG_ST_GEMM, [&] { return launch_rc_bias(A, lda, e.a_tiled, e.rc_clips, e.rc_rpc, e.rc_valid, L.wl_calib, L.bias, L.N, L.K, scr, bc, h->stream); }));
            a.bias_clip = bc; a.rpc = e.rc_rpc; a.nclips = e.rc_clips;
        } else {
            a.Wl = L.wl_calib;
        }
    }
    a.M = M; a.N = L.N; a.K = L.K;
    a.scale = e.scale; a.bias = e.no_bias ? nullptr : L.bias;
    a.res = e.res; a.ldr = e.ldr; a.res_mod = e.res_mod;
    a.out32 = e.out32; a.out16 = e.out16; a.ldc = e.ldc ? e.ldc : L.N;
    a.relu = e.relu;
    if (e.ln) { a.ln_w = e.ln->w; a.ln_b = e.ln->b; a.ln_flavour = e.ln_flavour; }
    a.res16 = e.res16; a.a_tiled = e.a_tiled;
    if (e.ln_mode == 1) {
        if (!L.c1h || !L.c1f) JG_FAIL(h, JG_ERR_STATE, "implicit LayerNorm on a layer that was not packed for it");
        a.ln_mode = 1; a.ln_stats = e.ln_stats; a.scale = a.Wl ? L.c1f : L.c1h;
    } else if (e.ln_mode == 2) {
        a.ln_mode = 2; a.ln_stats = e.ln_stats; a.scale = e.ln_gamma;
        a.xres_hi = e.x_hi; a.xres_lo = e.x_lo; a.out16 = e.x_hi; a.out_lo = e.x_lo; a.stat_out = e.stat_out;
    }
    if (h->calib && L.bc && !conv) {
        // column sums ACCUMULATE over every call of a calibration pass (chunks of a large calibration batch, the six
        // layers' shared shapes are separate Lin objects): calibrate_impl zeroes mu / mu_rows once at its start
        Lin& Lm = const_cast<Lin&>(L);
        float* part;
        RET(wsalloc(h, col_sum_scratch_elems(L.K), &part));
        // (a folded consumer's effective input is the NORMALISED row: the correction term is (w' - fp16(w')) . E[(x - mean) rstd])
        // (padding rows behind the caller's tokens would be averaged into E[x]: ADVICE r4)
        const int rows = e.calib_rows > 0 && e.calib_rows < M ? e.calib_rows : M;
        RET(timed(h, JG_ST_MISC, [&] { return launch_col_sum(A, lda, rows, L.K, part, Lm.mu, h->stream, e.ln_mode == 1 ? e.ln_stats : nullptr); }));
        Lm.mu_rows += rows;
    }
    return timed(h, stage, [&] { return LAUNCH(h, launch_gemm, a, conv, h->opts, h->stream); });
}

ConvGeom geom(int H, int W, int C, int KH, int KW, int SH, int SW, int PH, int PW, bool reorder = false) {
    ConvGeom g;
    g.taps[0] = g.taps[1] = g.taps[2] = g.taps[3] = 0;
    g.tap_table = 0;
    if (reorder && KH * KW <= 32) {
        const auto order = tap_order(KH, KW, SH, SW, true);
        for (size_t t = 0; t < order.size(); ++t)
            g.taps[t >> 3] |= (unsigned long long)((order[t].first << 4) | order[t].second) << ((t & 7) * 8);
        g.tap_table = 1;
    }
    g.H = H; g.W = W; g.C = C; g.KH = KH; g.KW = KW; g.SH = SH; g.SW = SW; g.PH = PH; g.PW = PW;
    g.OH = (H + 2 * PH - KH) / SH + 1;
    g.OW = (W + 2 * PW - KW) / SW + 1;
    g.cshift = 0;
    while ((1 << g.cshift) < C) ++g.cshift;
    g.rowmap = nullptr; g.rows_total = nullptr;
    g.in_op = 0;
    g.const_in = nullptr;
    return g;
}

// ------------------------------------------------------------------------------------ GestSync
constexpr int FH = 270, FW = 480;

// conv1 + max-pool straight from u8 frames: zero-band scan (stage "conv1_aux"), the fused kernel (stage "conv1": the
// path's dominant kernel, timed alone), strip-seam fix-up (stage "conv1_aux")
// fill_all = false: the caller's conv2 honours the row skip the scan leaves in zscr, so the pooled rows it never reads stay unwritten
int conv1_from_frames(jg_handle* h, const uint8_t* src, int nclip, int T, int pad, f16* pooled, f16* edge, unsigned* zscr, bool fill_all) {
    const bool scan = h->opts.conv1_zero_skip;
    if (debug_sync()) {
        const long NFd = (long)nclip * (T + 2 * pad - 4);
        std::fprintf(stderr, "[jg] conv1: src %p..%p pooled %p..%p edge %p..%p zscr %p..%p fill_all %d\n", (const void*)src,
                     (const void*)(src + (size_t)nclip * T * FH * FW * 3), (void*)pooled, (void*)(pooled + (size_t)NFd * 43 * 78 * 64), (void*)edge,
                     (void*)(edge + conv1_edge_elems(NFd)), (void*)zscr, (void*)(zscr + conv1_zmask_elems(nclip, T)), (int)fill_all);
    }
    if (scan) RET(timed(h, JG_ST_CONV1_AUX, [&] { return launch_conv1_scan(src, nclip, T, pad, h->c1_direct, 1.0f / 255.0f, zscr, h->stream); }));
    RET(timed(h, JG_ST_CONV1, [&] { return launch_conv1_direct(src, nclip, T, pad, h->c1_direct, 1.0f / 255.0f, pooled, edge,
                                                               scan ? zscr : nullptr, fill_all, h->opts, h->stream); }));
    return timed(h, JG_ST_CONV1_AUX, [&] { return launch_conv1_edge_fix(pooled, edge, (long)nclip * (T + 2 * pad - 4), h->stream); });
}

// conv stack over `nclip` temporal volumes -> conv_out (nclip*P, 512) fp32, P = T + 2*pad - 4
// conv16 (optional): fp16 copy of conv_out, the A operand of the per-position qkv projection (gs_transformer, Qkv0)
int gs_conv_stack(jg_handle* h, const void* src, int src_u8, long sb, long st, long sh, long sw, long sc,
                  int nclip, int T, int pad, float* conv_out, f16* conv16 = nullptr) {
    const int P = T + 2 * pad - 4;
    const long NF = (long)nclip * P;
    f16 *S, *o1, *p1, *o2, *o3, *o4, *o5, *p5;
    const int* s2pos = nullptr;          // per-position row-skip counts (direct path with conv2_row_skip)
    h->last_rowskip = nullptr;
    h->last_conv_totals = nullptr;
    const ConvGeom g1 = geom(FH, FW, 16, 7, 7, 3, 3, 0, 0);            // 88 x 158
    ConvGeom g2 = geom(43, 78, 64, 5, 5, 2, 2, 0, 0, true);            // 20 x 37   (taps in parity-class order, as packed)
    ConvGeom g3 = geom(20, 37, 128, 3, 3, 2, 2, 1, 1, true);           // 10 x 19
    ConvGeom g4 = geom(10, 19, 256, 3, 3, 1, 2, 1, 1, true);           // 10 x 10
    ConvGeom g5 = geom(10, 10, 256, 3, 3, 1, 1, 1, 1, true);           // 10 x 10
    RET(wsalloc(h, (size_t)NF * 43 * 78 * 64, &p1));
    RET(wsalloc(h, (size_t)NF * 20 * 37 * 128, &o2));
    RET(wsalloc(h, (size_t)NF * 10 * 19 * 256, &o3));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o4));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o5));
    RET(wsalloc(h, (size_t)NF * 4 * 4 * 256, &p5));
    Epi e;
    e.relu = 1;
    // (the direct kernel feeds u8 pixels to the MFMA as fp16 subnormals: fp16 build only; JG_PREC_BF16 stacks the frames and runs
    // conv1 as an implicit GEMM)
    const bool direct = src_u8 && sc == 1 && sw == 3 && sh == (long)FW * 3 && st == (long)FH * FW * 3 && sb == (long)T * st && h->conv1_direct && !h->bf16;
    if (direct) {
        // u8 HWC video: conv1 + max-pool straight from the frames; neither the temporal stack nor the
        // pre-pool tensor exists in HBM
        f16* edge;
        unsigned* zscr;
        RET(wsalloc(h, conv1_edge_elems(NF), &edge));
        RET(wsalloc(h, conv1_zmask_elems(nclip, T), &zscr));
        // Position-independent leading rows (common.h, ConvGeom::rowmap): the zero-band scan leaves every position's count s2 in
        // zscr; conv2 .. conv5 leave those rows out PER POSITION (compacted row maps built on the device) and conv3 .. conv5 and the
        // last max-pool read them from the const chain.  Only the LDS-DMA conv kernel knows how, so every layer of the chain must
        // take that path.
        const bool rowskip = h->opts.conv1_zero_skip && h->conv2_row_skip && h->opts.gemm_glds && h->gs_c2C && NF * 10 * 10 >= 256 &&
                             NF * 20 * 37 < (1L << 24);
        RET(conv1_from_frames(h, static_cast<const uint8_t*>(src), nclip, T, pad, p1, edge, zscr, !rowskip));
        if (rowskip) {
            s2pos = conv1_s2_counts(zscr, nclip, T, pad);
            ConvGeom* gs[4] = {&g2, &g3, &g4, &g5};
            const f16* cin[4] = {nullptr, h->gs_c2C, h->gs_c3C, h->gs_c4C};
            ConvRowMap rm[4];
            int* totals;
            RET(wsalloc(h, (size_t)64, &totals));
            for (int l = 0; l < 4; ++l) {
                rm[l].OH = gs[l]->OH; rm[l].OW = gs[l]->OW; rm[l].op = l;
                RET(wsalloc(h, (size_t)NF * gs[l]->OH * gs[l]->OW, &rm[l].map));
                RET(wsalloc(h, (size_t)NF + 1, &rm[l].base));
                rm[l].total = totals + l;
                gs[l]->rowmap = rm[l].map; gs[l]->rows_total = rm[l].total;
                gs[l]->in_op = l - 1; gs[l]->const_in = cin[l];
                h->last_conv_full[l] = NF * gs[l]->OH * gs[l]->OW;
            }
            RET(timed(h, JG_ST_CONV1_AUX, [&] { return launch_conv_rowmaps(s2pos, (int)NF, rm, 4, h->stream); }));
            h->last_conv_totals = totals;
            h->last_rowskip = reinterpret_cast<const int*>(zscr) + CONV1_ROWSKIP_WORD;
        }
    } else {
        RET(wsalloc(h, (size_t)NF * 88 * 158 * 64, &o1));
        RET(wsalloc(h, (size_t)NF * FH * FW * 16, &S));
        RET(timed(h, JG_ST_STACK, [&] { return LAUNCH(h, launch_stack_frames, src, src_u8, sb, st, sh, sw, sc, nclip, T, pad, FH, FW, S, h->stream); }));
        e.scale = src_u8 ? h->c1_scale255 : nullptr;
        e.out16 = o1;
        RET(gemm(h, JG_ST_CONV1, S, 0, (int)(NF * 88 * 158), h->c1, e, &g1));
        RET(timed(h, JG_ST_POOL, [&] { return LAUNCH(h, launch_maxpool3x3s2, o1, p1, (int)NF, 88, 158, 64, h->stream, nullptr, 0, nullptr); }));
    }
    e.scale = nullptr;
    e.out16 = o2; RET(gemm(h, JG_ST_CONV, p1, 0, (int)(NF * 20 * 37), h->c2, e, &g2));
    e.out16 = o3; RET(gemm(h, JG_ST_CONV, o2, 0, (int)(NF * 10 * 19), h->c3, e, &g3));
    e.out16 = o4; RET(gemm(h, JG_ST_CONV, o3, 0, (int)(NF * 10 * 10), h->c4, e, &g4));
    e.out16 = o5; RET(gemm(h, JG_ST_CONV, o4, 0, (int)(NF * 10 * 10), h->c5, e, &g5));
    RET(timed(h, JG_ST_POOL, [&] { return LAUNCH(h, launch_maxpool3x3s2, o5, p5, (int)NF, 10, 10, 256, h->stream, s2pos, 3, h->gs_c5C); }));
    e.out16 = conv16; e.out32 = conv_out;
    RET(gemm(h, JG_ST_CONV, p5, 4096, (int)NF, h->fc6, e));
    return JG_OK;
}

// Const chain (ConvGeom::rowskip): conv2 .. conv5 of an all-constant pooled image -- relu(bias1) in every pixel, which is
// what conv1 + max-pool produce wherever the frames are blanked.  Computed once per weight load with the run-time kernels
// (same MFMA sequence per output element, so the rows are bit-identical to what the layers would compute per position);
// 4 copies per layer so that every launch has the 256 rows the LDS-DMA kernel needs.
int gs_build_const_chain(jg_handle* h) {
    h->gs_c2C = h->gs_c3C = h->gs_c4C = h->gs_c5C = nullptr;
    if (!h->opts.gemm_glds || h->bf16) return JG_OK;      // the chain starts from conv1_direct's constant (fp16 build only)
    constexpr int NC = 4;
    f16 *zc, *poolC, *c2C, *c3C, *c4C, *c5C;
    h->wallocs = &h->wallocs_gs;
    RET(walloc(h, (size_t)64, &zc));
    RET(walloc(h, (size_t)NC * 43 * 78 * 64, &poolC));
    RET(walloc(h, (size_t)NC * 20 * 37 * 128, &c2C));
    RET(walloc(h, (size_t)NC * 10 * 19 * 256, &c3C));
    RET(walloc(h, (size_t)NC * 10 * 10 * 256, &c4C));
    RET(walloc(h, (size_t)NC * 10 * 10 * 256, &c5C));
    HIPCHK(h, launch_conv1_zconst(h->c1_direct, 1.0f / 255.0f, zc, h->stream));
    HIPCHK(h, launch_broadcast_channels(zc, 64, poolC, (long)NC * 43 * 78, h->stream));
    const ConvGeom g2 = geom(43, 78, 64, 5, 5, 2, 2, 0, 0, true);
    const ConvGeom g3 = geom(20, 37, 128, 3, 3, 2, 2, 1, 1, true);
    const ConvGeom g4 = geom(10, 19, 256, 3, 3, 1, 2, 1, 1, true);
    const ConvGeom g5 = geom(10, 10, 256, 3, 3, 1, 1, 1, 1, true);
    Epi e;
    e.relu = 1;
    e.out16 = c2C; RET(gemm(h, JG_ST_CONV, poolC, 0, NC * 20 * 37, h->c2, e, &g2));
    e.out16 = c3C; RET(gemm(h, JG_ST_CONV, c2C, 0, NC * 10 * 19, h->c3, e, &g3));
    e.out16 = c4C; RET(gemm(h, JG_ST_CONV, c3C, 0, NC * 10 * 10, h->c4, e, &g4));
    e.out16 = c5C; RET(gemm(h, JG_ST_CONV, c4C, 0, NC * 10 * 10, h->c5, e, &g5));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->gs_c2C = c2C; h->gs_c3C = c3C; h->gs_c4C = c4C; h->gs_c5C = c5C;
    return JG_OK;
}

// post-norm transformer (gestsync.py:20-21) in place on x32/x16, M = nseq*21 tokens
// Whether the whole GestSync transformer of M tokens runs with residual+LayerNorm fused into the projection GEMMs.
// All twelve projections must qualify (single-fp16 weights, not the calibration pass): the fused kernel keeps the
// fp32 residual stream in its own tiled order (gemm.hip), so fused and unfused layers cannot be mixed.
// rows_per_clip: rows of one clip in the launch (T * 21 on the clip path; 0: no clip structure, e.g. forward_vid windows).  In the
// run-time corrected mode the LayerNorm-fused projections exist with the per-clip bias only (there is no hi+lo instance of that
// kernel), and the per-clip bias needs rows_per_clip >= 256 (gemm(): `can`): shorter clips (T <= 12) and launches without clip structure
// take the unfused plan, whose GEMMs run hi+lo (such batches used to fail with hipErrorInvalidValue).
bool gs_fused_plan(const jg_handle* h, int M, int rows_per_clip) {
    if (!h->fuse_ln || !h->opts.gemm_glds || h->calib || M < 1024 || h->bf16) return false;     // (the token stream is fp16)      // the tiled token stream is read by LDS-DMA only
    if (h->precision == JG_PREC_FP16_RC && rows_per_clip < 256) return false;
    for (int l = 0; l < 6; ++l)
        if (h->gs_layers[l].out.wl || h->gs_layers[l].ff2.wl) return false;
    return true;
}
inline size_t pad128(size_t rows) { return (rows + 127) / 128 * 128; }

// x32/x16 hold pad128(M) rows.  With `tiled` (gs_fused_plan) the token stream is the tiled fp16 plane x16 alone (x32 is not
// used); otherwise fp32 rows + fp16 rows.
// Layer 0's qkv projection by linearity (clip path): token j of window (clip c, frame i) is conv[c][clamp(i+j-shift)] + pe[j],
// so W x + b = W conv[c][p] + (W pe[j] + b).  The projection then runs over the nclip*P distinct conv positions (154 per clip
// instead of 150 * 21 tokens) plus the 21 positional rows, and the attention kernel gathers and sums the operand rows
// (attention.hip, attn_mfma_s32_kernel<true>): no 310 MB qkv tensor for layer 0.
struct Qkv0 {
    const f16* conv16;    // [nclip*P][512]
    int nclip, P, Twin, shift;
};

// rc_clips > 0: the rows are rc_clips clips of M / rc_clips rows each (the clip path; JG_PREC_FP16_RC's per-clip corrections)
int gs_transformer(jg_handle* h, float* x32, f16* x16, int nseq, int S, bool tiled, const Qkv0* q0 = nullptr, int rc_clips = 0, const int* rc_valid = nullptr) {
    const int M = nseq * S;
    const int rc_rpc = rc_clips > 0 && tiled ? M / rc_clips : 0;
    if (!rc_rpc) rc_clips = 0;
    f16 *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)M * 1536, &qkv));
    RET(wsalloc(h, (size_t)M * 512, &att));
    RET(wsalloc(h, (size_t)M * 2048, &hid));
    for (int l = 0; l < 6; ++l) {
        const EncLayer& L = h->gs_layers[l];
        if (l == 0 && q0) {
            f16* qpos;
            RET(wsalloc(h, (size_t)q0->nclip * q0->P * 1536, &qpos));
            if (!h->gs_qpe) HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->gs_qpe), (size_t)32 * 1536 * sizeof(f16)));
            f16* qpe = h->gs_qpe;
            Epi e;
            e.out16 = qpos; e.no_bias = 1;
            RET(gemm(h, JG_ST_GEMM, q0->conv16, 512, q0->nclip * q0->P, L.qkv, e));
            if (!h->gs_qpe_valid) {
                RET(timed(h, JG_ST_GEMM, [&] { return launch_pe_project(h->gs_pe, S, L.qkv.wh, L.qkv.rc ? L.qkv.wl_calib : L.qkv.wl, L.qkv.bias, 1536, 512, qpe, h->stream); }));
                HIPCHK(h, hipStreamSynchronize(h->stream));      // once per weight load: later calls may come on another stream
                h->gs_qpe_valid = true;
            }
            const AttnGather ag = {qpe, q0->Twin, q0->P, q0->shift};
            RET(timed(h, JG_ST_ATTN, [&] { return launch_attention_gather(qpos, ag, nseq, S, 8, att, h->stream); }));
        } else {
            Epi e;
            e.out16 = qkv; e.a_tiled = tiled; e.rc_rpc = rc_rpc; e.rc_clips = rc_clips; e.rc_valid = rc_valid;
            RET(gemm(h, JG_ST_GEMM, x16, 512, M, L.qkv, e));
            RET(timed(h, JG_ST_ATTN, [&] { return LAUNCH(h, launch_attention, qkv, nullptr, nseq, S, 8, 64, att, h->opts, h->stream); }));
        }
        // out_proj / linear2 with the residual add and the post-norm LayerNorm fused into the epilogue (row-wide
        // 128x512 tiles, tiled fp16 token stream) when gs_fused_plan() says so; otherwise GEMM + LayerNorm kernel.
        auto proj_ln = [&](const f16* A, long lda, const Lin& W, const LNp& ln) -> int {
            Epi r;
            if (tiled) {
                r.res16 = x16; r.out16 = x16; r.ln = &ln; r.ln_flavour = LN_STD;
                r.rc_rpc = rc_rpc; r.rc_clips = rc_clips; r.rc_valid = rc_valid;
                return gemm(h, JG_ST_GEMM, A, lda, M, W, r);
            }
            r.res = x32; r.ldr = 512; r.out32 = x32;
            RET(gemm(h, JG_ST_GEMM, A, lda, M, W, r));
            return timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, x32, ln.w, ln.b, M, 512, LN_STD, 0, x32, x16, h->stream); });
        };
        RET(proj_ln(att, 512, L.out, L.n1));
        Epi f;
        f.relu = 1; f.out16 = hid; f.a_tiled = tiled; f.rc_rpc = rc_rpc; f.rc_clips = rc_clips; f.rc_valid = rc_valid;
        RET(gemm(h, JG_ST_GEMM, x16, 512, M, L.ff1, f));
        RET(proj_ln(hid, 2048, L.ff2, L.n2));
    }
    return JG_OK;
}

// ------------------------------------------------------------------------------------ fp32 audit path (audit32.hip)
// JG_PREC_FP32 (and option audit_stages on a handle finalized with audit_weights): the same stages as above on fp32 weights and fp32
// activations, exact-fp32 MFMAs, fp32 softmax / LayerNorm.  The reference's CPU path is fp32 (inference_embs.py:497 -- autocast does nothing
// without CUDA): this is the on-device stand-in for it, what the fp16 modes are audited against on a checkpoint the parity tests never saw.
// Straightforward on purpose (no window de-duplication tricks beyond the distinct conv positions, no fused epilogues beyond bias /
// residual / activation, the mean(-1) AFTER ff_vid.2 as in inference_embs.py:511); ~40-60 clips/s.
enum { AUD_CONV = 1, AUD_GS = 2, AUD_JG = 4, AUD_CONTENT = 8, AUD_XLMR = 16, AUD_ALL = 31 };
inline int audit_mask(const jg_handle* h) { return h->precision == JG_PREC_FP32 ? AUD_ALL : h->audit_stages; }

struct Epi32 {
    const float* res = nullptr;
    long ldr = 0;
    int res_mod = 0;
    int act = 0;          // 0 none, 1 ReLU, 2 exact GELU
};

int gemm32(jg_handle* h, int stage, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e = Epi32(), const ConvGeom* g = nullptr) {
    if (!L.w32d || !L.b32d)
        JG_FAIL(h, JG_ERR_STATE, "fp32 audit weights missing: select JG_PREC_FP32 or set option audit_weights=1 before jg_finalize_weights");
    Gemm32Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda;
    if (g) { a.g = *g; a.conv = 1; }
    a.W = L.w32d; a.ldw = L.K;
    a.M = M; a.N = L.N; a.K = L.K;
    a.bias = L.b32d;
    a.res = e.res; a.ldr = e.ldr; a.res_mod = e.res_mod;
    a.out = out; a.ldc = L.N;
    a.act = e.act;
    return timed(h, stage, [&] { return launch_gemm32(a, h->stream); });
}

// The same product on the fp16 matrix cores with split operands (audit32.h, GemmX3Args): A fp32, W = hi + lo, three MFMAs per fragment pair
int gemm_x3(jg_handle* h, int stage, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e = Epi32()) {
    const f16* lo = L.wl ? L.wl : L.wl_calib;
    if (!L.wh || !lo) JG_FAIL(h, JG_ERR_STATE, "split-operand GEMM on a layer that was packed without its lo half");
    GemmX3Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.Wh = L.wh; a.Wl = lo; a.ldw = L.K;
    a.M = M; a.N = L.N; a.K = L.K;
    a.bias = L.b32d ? L.b32d : L.bias;
    a.res = e.res; a.ldr = e.ldr; a.res_mod = e.res_mod;
    a.out = out; a.ldc = L.N;
    a.relu = e.act == 1;
    if (e.act > 1) JG_FAIL(h, JG_ERR_ARG, "gemm_x3: ReLU only");
    return timed(h, stage, [&] { return launch_gemm_x3(a, h->stream); });
}

// conv stack over `nclip` temporal volumes -> conv_out (nclip*P, 512) fp32 (gestsync.py:34-87,308-325: conv + BatchNorm(eval, folded) + ReLU, two max-pools)
int gs_conv_stack32(jg_handle* h, const void* src, int src_u8, long sb, long st, long sh, long sw, long sc, int nclip, int T, int pad, float* conv_out) {
    const int P = T + 2 * pad - 4;
    const long NF = (long)nclip * P;
    if (NF * 88 * 158 >= (1L << 31)) JG_FAIL(h, JG_ERR_ARG, "fp32 conv stack: too many positions in one pass (lower jg_set_chunk)");
    const ConvGeom g1 = geom(FH, FW, 16, 7, 7, 3, 3, 0, 0);
    const ConvGeom g2 = geom(43, 78, 64, 5, 5, 2, 2, 0, 0, true);       // (tap order as packed: make_conv(..., reorder = true))
    const ConvGeom g3 = geom(20, 37, 128, 3, 3, 2, 2, 1, 1, true);
    const ConvGeom g4 = geom(10, 19, 256, 3, 3, 1, 2, 1, 1, true);
    const ConvGeom g5 = geom(10, 10, 256, 3, 3, 1, 1, 1, 1, true);
    float *S, *o1, *p1, *o2, *o3, *o4, *o5, *p5;
    RET(wsalloc(h, (size_t)NF * FH * FW * 16, &S));
    RET(wsalloc(h, (size_t)NF * 88 * 158 * 64, &o1));
    RET(wsalloc(h, (size_t)NF * 43 * 78 * 64, &p1));
    RET(wsalloc(h, (size_t)NF * 20 * 37 * 128, &o2));
    RET(wsalloc(h, (size_t)NF * 10 * 19 * 256, &o3));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o4));
    RET(wsalloc(h, (size_t)NF * 10 * 10 * 256, &o5));
    RET(wsalloc(h, (size_t)NF * 4 * 4 * 256, &p5));
    RET(timed(h, JG_ST_STACK, [&] { return launch_stack_frames32(src, src_u8, sb, st, sh, sw, sc, nclip, T, pad, FH, FW, S, h->stream); }));
    Epi32 e;
    e.act = 1;
    RET(gemm32(h, JG_ST_CONV1, S, 0, (int)(NF * 88 * 158), h->c1, o1, e, &g1));
    RET(timed(h, JG_ST_POOL, [&] { return launch_maxpool3x3s2_32(o1, p1, (int)NF, 88, 158, 64, h->stream); }));
    RET(gemm32(h, JG_ST_CONV, p1, 0, (int)(NF * 20 * 37), h->c2, o2, e, &g2));
    RET(gemm32(h, JG_ST_CONV, o2, 0, (int)(NF * 10 * 19), h->c3, o3, e, &g3));
    RET(gemm32(h, JG_ST_CONV, o3, 0, (int)(NF * 10 * 10), h->c4, o4, e, &g4));
    RET(gemm32(h, JG_ST_CONV, o4, 0, (int)(NF * 10 * 10), h->c5, o5, e, &g5));
    RET(timed(h, JG_ST_POOL, [&] { return launch_maxpool3x3s2_32(o5, p5, (int)NF, 10, 10, 256, h->stream); }));
    return gemm32(h, JG_ST_CONV, p5, 4096, (int)NF, h->fc6, conv_out, e);
}

// post-norm transformer (gestsync.py:19-21) in place on x32, M = nseq * S tokens
int gs_transformer32(jg_handle* h, float* x32, int nseq, int S) {
    const int M = nseq * S;
    float *qkv, *att, *hid, *t;
    RET(wsalloc(h, (size_t)M * 1536, &qkv));
    RET(wsalloc(h, (size_t)M * 512, &att));
    RET(wsalloc(h, (size_t)M * 2048, &hid));
    RET(wsalloc(h, (size_t)M * 512, &t));
    Epi32 r; r.res = x32; r.ldr = 512;
    Epi32 f; f.act = 1;
    for (int l = 0; l < 6; ++l) {
        const EncLayer& L = h->gs_layers[l];
        RET(gemm32(h, JG_ST_GEMM, x32, 512, M, L.qkv, qkv));
        RET(timed(h, JG_ST_ATTN, [&] { return launch_attention32(qkv, nullptr, nseq, S, 8, 64, att, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, att, 512, M, L.out, t, r));
        RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(t, L.n1.w, L.n1.b, M, 512, LN_STD, 0, x32, nullptr, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, x32, 512, M, L.ff1, hid, f));
        RET(gemm32(h, JG_ST_GEMM, hid, 2048, M, L.ff2, t, r));
        RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(t, L.n2.w, L.n2.b, M, 512, LN_STD, 0, x32, nullptr, h->stream); }));
    }
    return JG_OK;
}

// windows + PE + transformer + ff_vid + mean(-1) of the clip path: conv (nb*P, 512) fp32 -> out_feats (nb*T, 1024)
int gs_clip_tail32(jg_handle* h, const float* conv, int nb, int P, int T, int shift, float* out_feats) {
    const int S = 21, nseq = nb * T, M = nseq * S;
    float *x32, *hid, *full;
    RET(wsalloc(h, (size_t)M * 512, &x32));
    RET(timed(h, JG_ST_MISC, [&] { return launch_window_gather(conv, h->gs_pe, nb, P, T, S, 512, shift, 0, x32, nullptr, h->stream); }));
    RET(gs_transformer32(h, x32, nseq, S));
    RET(wsalloc(h, (size_t)M * 512, &hid));
    RET(wsalloc(h, (size_t)M * 1024, &full));
    Epi32 f; f.act = 1;
    RET(gemm32(h, JG_ST_GEMM, x32, 512, M, h->ff0, hid, f));
    RET(gemm32(h, JG_ST_GEMM, hid, 512, M, h->ff2, full));
    return timed(h, JG_ST_MISC, [&] { return launch_group_mean32(full, nseq, S, 1024, out_feats, h->stream); });
}

// pre-norm encoder (modules.py:11-59) in place on x32; the final norm's output goes to n32
int annotated_encoder32(jg_handle* h, const EncLayer* layers, int nl, const LNp& fin, float* x32, float* n32, const float* mask, int B, int S, int D, int Dff) {
    const int M = B * S, H = 8, dk = D / H;
    float *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)M * 3 * D, &qkv));
    RET(wsalloc(h, (size_t)M * D, &att));
    RET(wsalloc(h, (size_t)M * Dff, &hid));
    Epi32 r; r.res = x32; r.ldr = D;
    Epi32 f; f.act = 1;
    for (int l = 0; l < nl; ++l) {
        const EncLayer& L = layers[l];
        RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(x32, L.n1.w, L.n1.b, M, D, LN_ANNOTATED, 0, n32, nullptr, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, n32, D, M, L.qkv, qkv));
        RET(timed(h, JG_ST_ATTN, [&] { return launch_attention32(qkv, mask, B, S, H, dk, att, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, att, D, M, L.out, x32, r));
        RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(x32, L.n2.w, L.n2.b, M, D, LN_ANNOTATED, 0, n32, nullptr, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, n32, D, M, L.ff1, hid, f));
        RET(gemm32(h, JG_ST_GEMM, hid, Dff, M, L.ff2, x32, r));
    }
    return timed(h, JG_ST_NORM, [&] { return launch_layernorm(x32, fin.w, fin.b, M, D, LN_ANNOTATED, 0, n32, nullptr, h->stream); });
}

// ONE sub-layer of a pre-norm encoder layer on the fp32 kernels, in place on the fp32 residual stream (which = 1: x += out(attn(qkv(LN1 x))),
// 2: x += ff2(relu(ff1(LN2 x)))); scratch: M * (D + 3 D + D + Dff) floats.  (Diagnosis: annotated_encoder's `parts`.)
int encoder_sublayers32(jg_handle* h, const EncLayer& L, int which, float* x32, float* scratch, const float* mask, int B, int S, int D, int Dff) {
    const int M = B * S, H = 8, dk = D / H;
    float* n32 = scratch;
    float* qkv = n32 + (size_t)M * D;
    float* att = qkv + (size_t)M * 3 * D;
    float* hid = att + (size_t)M * D;
    Epi32 r; r.res = x32; r.ldr = D;
    if (which == 1) {
        RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(x32, L.n1.w, L.n1.b, M, D, LN_ANNOTATED, 0, n32, nullptr, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, n32, D, M, L.qkv, qkv));
        RET(timed(h, JG_ST_ATTN, [&] { return launch_attention32(qkv, mask, B, S, H, dk, att, h->stream); }));
        return gemm32(h, JG_ST_GEMM, att, D, M, L.out, x32, r);
    }
    Epi32 f; f.act = 1;
    RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(x32, L.n2.w, L.n2.b, M, D, LN_ANNOTATED, 0, n32, nullptr, h->stream); }));
    RET(gemm32(h, JG_ST_GEMM, n32, D, M, L.ff1, hid, f));
    return gemm32(h, JG_ST_GEMM, hid, Dff, M, L.ff2, x32, r);
}

// proj_ip_rgb + positional rows (jegal.py:25-28,84-85) on the fp32 kernels: feats (M,1024) -> x32 (M,512); t32: (M,512) scratch
// x3: on the fp16 matrix cores with split operands (gemm_x3: the fp16 modes' production path) instead of the fp32 MFMA (audit)
int jegal_input32(jg_handle* h, const float* feats, int M, int T, float* t32, float* x32, bool x3 = false) {
    auto G = [&](const float* A, long lda, const Lin& L, float* out, const Epi32& e) {
        return x3 ? gemm_x3(h, JG_ST_GEMM, A, lda, M, L, out, e) : gemm32(h, JG_ST_GEMM, A, lda, M, L, out, e);
    };
    float* t2;
    RET(wsalloc(h, (size_t)M * 512, &t2));
    RET(G(feats, 1024, h->ip0, t32, Epi32()));
    RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(t32, h->ip_ln.w, h->ip_ln.b, M, 512, LN_STD, 1, t2, nullptr, h->stream); }));
    Epi32 p; p.res = h->rgb_pe; p.ldr = 512; p.res_mod = T;
    return G(t2, 512, h->ip3, x32, p);
}

// proj_op_rgb (+ proj_op_align_gesture) on the fp32 kernels from the final norm's fp32 output
int jegal_tail32(jg_handle* h, const float* n32, int M, int align, float* out, bool x3 = false) {
    auto G = [&](const float* A, const Lin& L, float* o, const Epi32& e) {
        return x3 ? gemm_x3(h, JG_ST_GEMM, A, 512, M, L, o, e) : gemm32(h, JG_ST_GEMM, A, 512, M, L, o, e);
    };
    if (!align) return G(n32, h->op_rgb, out, Epi32());
    float *g32, *a32;
    RET(wsalloc(h, (size_t)M * 512, &g32));
    RET(wsalloc(h, (size_t)M * 512, &a32));
    RET(G(n32, h->op_rgb, g32, Epi32()));
    Epi32 f; f.act = 1;
    RET(G(g32, h->al_g0, a32, f));
    return G(a32, h->al_g2, out, Epi32());
}

int jegal_gestures_impl32(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out) {
    const int M = B * T;
    float *t32, *x32, *n32;
    RET(wsalloc(h, (size_t)M * 512, &t32));
    RET(wsalloc(h, (size_t)M * 512, &x32));
    RET(wsalloc(h, (size_t)M * 512, &n32));
    RET(jegal_input32(h, feats, M, T, t32, x32, false));
    RET(annotated_encoder32(h, h->rgb_layers, 6, h->rgb_norm, x32, n32, mask, B, T, 512, 2048));
    return jegal_tail32(h, n32, M, align, out, false);
}

int jegal_audio_impl32(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_host, float* out) {
    const int F = 80;
    const ConvGeom g0 = geom(Tm, F, 1, 5, 5, 1, 1, 2, 2);
    const ConvGeom g3 = geom(Tm, F, 32, 3, 3, 2, 2, 1, 1);
    const ConvGeom g6 = geom(g3.OH, g3.OW, 64, 3, 3, 2, 2, 1, 1);
    const ConvGeom g9 = geom(g6.OH, g6.OW, 128, 3, 3, 1, 3, 1, 1);
    const ConvGeom g12 = geom(g9.OH, g9.OW, 256, 3, 3, 1, 3, 1, 1);
    const ConvGeom g15 = geom(g12.OH, g12.OW, 256, 1, 1, 1, 3, 0, 0);
    if (g15.OW != 1) JG_FAIL(h, JG_ERR_ARG, "audio CNN must reduce 80 mel bands to 1");
    int* valid = nullptr;
    if (valid_host) {
        bool ragged = false;
        for (int b = 0; b < B; ++b) {
            if (valid_host[b] < 4 || valid_host[b] > Tm) JG_FAIL(h, JG_ERR_ARG, "valid_tm[%d] = %d outside 4..Tm = %d", b, valid_host[b], Tm);
            ragged |= valid_host[b] != Tm;
        }
        if (ragged) {
            RET(wsalloc(h, (size_t)B, &valid));
            RET(upload_i32_async(h, valid_host, (size_t)B, valid));
        }
    }
    float *m0, *c0, *c3, *c6, *c9, *c12, *c15;
    RET(wsalloc(h, (size_t)B * Tm * F, &m0));
    RET(wsalloc(h, (size_t)B * Tm * F * 32, &c0));
    RET(wsalloc(h, (size_t)B * g3.OH * g3.OW * 64, &c3));
    RET(wsalloc(h, (size_t)B * g6.OH * g6.OW * 128, &c6));
    RET(wsalloc(h, (size_t)B * g9.OH * g9.OW * 256, &c9));
    RET(wsalloc(h, (size_t)B * g12.OH * g12.OW * 256, &c12));
    RET(wsalloc(h, (size_t)B * g15.OH * 256, &c15));
    // every layer's rows beyond a clip's own extent are zero: the padding the clip would see alone (jegal_audio_impl)
    auto tail = [&](float* x, int halvings, int H, long row_elems) -> int {
        if (!valid) return JG_OK;
        return timed(h, JG_ST_MISC, [&] { return launch_zero_tail32(x, valid, halvings, B, H, row_elems, h->stream); });
    };
    const float* mel_in = mel;
    if (valid) {
        HIPCHK(h, hipMemcpyAsync(m0, mel, (size_t)B * Tm * F * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        RET(tail(m0, 0, Tm, F));
        mel_in = m0;
    }
    Epi32 e; e.act = 1;
    RET(gemm32(h, JG_ST_CONV, mel_in, 0, B * Tm * F, h->a0, c0, e, &g0));
    RET(tail(c0, 0, Tm, (long)F * 32));
    RET(gemm32(h, JG_ST_CONV, c0, 0, B * g3.OH * g3.OW, h->a3, c3, e, &g3));
    RET(tail(c3, 1, g3.OH, (long)g3.OW * 64));
    RET(gemm32(h, JG_ST_CONV, c3, 0, B * g6.OH * g6.OW, h->a6, c6, e, &g6));
    RET(tail(c6, 2, g6.OH, (long)g6.OW * 128));
    RET(gemm32(h, JG_ST_CONV, c6, 0, B * g9.OH * g9.OW, h->a9, c9, e, &g9));
    RET(tail(c9, 2, g9.OH, (long)g9.OW * 256));
    RET(gemm32(h, JG_ST_CONV, c9, 0, B * g12.OH * g12.OW, h->a12, c12, e, &g12));
    RET(gemm32(h, JG_ST_CONV, c12, 0, B * g15.OH, h->a15, c15, Epi32(), &g15));
    return gemm32(h, JG_ST_GEMM, c15, 256, B * g15.OH, h->op_audio, out);
}

int jegal_text_impl32(jg_handle* h, const float* states, const float* mask, int B, int L, float* out) {
    const int M = B * L;
    float *x32, *n32;
    RET(wsalloc(h, (size_t)M * 768, &x32));
    RET(wsalloc(h, (size_t)M * 768, &n32));
    HIPCHK(h, hipMemcpyAsync(x32, states, (size_t)M * 768 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    RET(annotated_encoder32(h, h->text_layers, 3, h->text_norm, x32, n32, mask, B, L, 768, 3072));
    return gemm32(h, JG_ST_GEMM, n32, 768, M, h->op_text, out);
}

int fuse_content_impl32(jg_handle* h, const float* fused, int rows, float* out) {
    float *a32, *b32;
    RET(wsalloc(h, (size_t)rows * 512, &a32));
    RET(wsalloc(h, (size_t)rows * 512, &b32));
    Epi32 r; r.act = 1;
    RET(gemm32(h, JG_ST_GEMM, fused, 512, rows, h->fu0, a32, r));
    RET(gemm32(h, JG_ST_GEMM, a32, 512, rows, h->fu2, b32));
    RET(gemm32(h, JG_ST_GEMM, b32, 512, rows, h->al_c0, a32, r));
    return gemm32(h, JG_ST_GEMM, a32, 512, rows, h->al_c2, out);
}

// XLMRobertaModel.forward (explicit LayerNorms, un-folded matrices: finalize_xlmr packs them that way when audit weights are kept)
int xlmr_encode_impl32(jg_handle* h, const int32_t* ids, const int32_t* amask, int B, int L, float* out) {
    if (h->xl_folded) JG_FAIL(h, JG_ERR_STATE, "the XLM-RoBERTa weights were packed for the implicit-LayerNorm pass: finalize them with audit weights for the fp32 path");
    constexpr int D = 768, DFF = 3072, H = 12;
    const int M = B * L;
    float *x32, *t32, *qkv, *att, *hid, *mk = nullptr;
    RET(wsalloc(h, (size_t)M * D, &x32));
    RET(wsalloc(h, (size_t)M * D, &t32));
    RET(wsalloc(h, (size_t)M * 3 * D, &qkv));
    RET(wsalloc(h, (size_t)M * D, &att));
    RET(wsalloc(h, (size_t)M * DFF, &hid));
    if (amask) {
        RET(wsalloc(h, (size_t)M, &mk));
        RET(timed(h, JG_ST_MISC, [&] { return launch_mask_i32_f32(amask, mk, M, h->stream); }));
    }
    RET(timed(h, JG_ST_MISC, [&] { return launch_xlmr_embed(ids, B, L, D, 1, h->xl_vocab, h->xl_maxpos, h->xl_word, h->xl_pos, h->xl_type, t32, h->stream); }));
    RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(t32, h->xl_emb_ln.w, h->xl_emb_ln.b, M, D, LN_STD, 0, x32, nullptr, h->stream); }));
    Epi32 r; r.res = x32; r.ldr = D;
    Epi32 f; f.act = 2;
    for (int l = 0; l < h->xl_layers_n; ++l) {
        const EncLayer& Ly = h->xl_layers[l];
        const bool last = l + 1 == h->xl_layers_n;
        RET(gemm32(h, JG_ST_GEMM, x32, D, M, Ly.qkv, qkv));
        RET(timed(h, JG_ST_ATTN, [&] { return launch_attention32(qkv, mk, B, L, H, 64, att, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, att, D, M, Ly.out, t32, r));
        RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(t32, Ly.n1.w, Ly.n1.b, M, D, LN_STD, 0, x32, nullptr, h->stream); }));
        RET(gemm32(h, JG_ST_GEMM, x32, D, M, Ly.ff1, hid, f));
        RET(gemm32(h, JG_ST_GEMM, hid, DFF, M, Ly.ff2, t32, r));
        RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(t32, Ly.n2.w, Ly.n2.b, M, D, LN_STD, 0, last ? out : x32, nullptr, h->stream); }));
    }
    return JG_OK;
}

// valid_host (optional, host [B]): clip b's first valid_host[b] frames are its own, the rest of its T frames is batch padding (copies of its
// last frame, jg_gestsync_clip_ragged): only the run-time corrected mode looks at it -- a clip's statistics come from its own rows
int gestsync_clip_impl(jg_handle* h, const void* frames, int dtype, int B, int T, float* out_feats, const int32_t* valid_host = nullptr) {
    if (!h->gs_ready) JG_FAIL(h, JG_ERR_STATE, "GestSync weights not finalized");
    if (B <= 0 || T <= 0) JG_FAIL(h, JG_ERR_ARG, "B and T must be positive");
    if (dtype != JG_U8 && dtype != JG_F32) JG_FAIL(h, JG_ERR_ARG, "frames dtype must be JG_U8 or JG_F32");
    // Edge padding 12 (inference_embs.py:283) gives T+20 conv positions, but positions 0..8 and
    // T+11..T+19 each see five copies of one frame: evaluate the T+4 distinct ones (== padding 4) and
    // let the window gather clamp.  Bit-identical to evaluating all T+20.
    const int PAD = h->edge_dedup ? 4 : 12;
    const int P = T + 2 * PAD - 4, S = 21;
    const size_t esz = dtype == JG_U8 ? 1 : 4;
    const long sw = 3, sh = (long)FW * 3, st = (long)FH * FW * 3, sb = (long)T * st;
    // fp32 audit stages (audit_mask): the conv stack and / or the transformer + ff_vid of this call run on the fp32 kernels; a pass of the
    // fp32 conv stack holds 2.1 GB per 150-frame clip, so its passes are two clips
    const int am = audit_mask(h);
    const int chunk = (am & AUD_CONV) ? std::min(h->chunk, 2) : h->chunk;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        h->ws.reset();
        if (h->ws_poison)                       // test aid: whatever a kernel reads without having written it is NaN
            for (auto& c : h->ws.chunks) HIPCHK(h, launch_poison(c.p, c.cap, h->stream));
        float* conv;
        RET(wsalloc(h, (size_t)nb * P * 512, &conv));
        const char* src = reinterpret_cast<const char*>(frames) + (size_t)b0 * sb * esz;
        const int nseq = nb * T, M = nseq * S;
        if (am & AUD_GS) {
            if (am & AUD_CONV) RET(gs_conv_stack32(h, src, dtype == JG_U8, sb, st, sh, sw, 1, nb, T, PAD, conv));
            else RET(gs_conv_stack(h, src, dtype == JG_U8, sb, st, sh, sw, 1, nb, T, PAD, conv));
            RET(gs_clip_tail32(h, conv, nb, P, T, 12 - PAD, out_feats + (size_t)b0 * T * 1024));
            continue;
        }
        float* x32; f16 *x16, *hid, *mean16, *conv16 = nullptr;
        const bool tiled = gs_fused_plan(h, M, T * S);
        int* rc_valid = nullptr;
        if (valid_host && tiled && h->precision == JG_PREC_FP16_RC) {
            std::vector<int32_t> hv(nb);
            for (int b = 0; b < nb; ++b) hv[b] = valid_host[b0 + b] * S;              // rows = frames x 21 tokens
            RET(wsalloc(h, (size_t)nb, &rc_valid));
            RET(upload_i32_async(h, hv.data(), (size_t)nb, rc_valid));
        }
        // layer-0 qkv from the distinct conv positions: worth it when the windows overlap (T > 1) and the MFMA attention runs
        const bool lin0 = tiled && h->qkv0_linear && h->opts.attn_mfma && T > 1;
        if (lin0) RET(wsalloc(h, (size_t)nb * P * 512, &conv16));
        if (am & AUD_CONV) {
            RET(gs_conv_stack32(h, src, dtype == JG_U8, sb, st, sh, sw, 1, nb, T, PAD, conv));
            if (conv16) RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_cast_f32_f16, (const float*)conv, conv16, (long)nb * P * 512, h->stream); }));
        } else {
            RET(gs_conv_stack(h, src, dtype == JG_U8, sb, st, sh, sw, 1, nb, T, PAD, conv, conv16));
        }
        RET(wsalloc(h, pad128(M) * 512, &x32));
        RET(wsalloc(h, pad128(M) * 512, &x16));
        RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_window_gather, conv, h->gs_pe, nb, P, T, S, 512, 12 - PAD, tiled, x32, x16, h->stream); }));
        const Qkv0 q0 = {conv16, nb, P, T, 12 - PAD};
        RET(gs_transformer(h, x32, x16, nseq, S, tiled, lin0 ? &q0 : nullptr, nb, rc_valid));
        RET(wsalloc(h, (size_t)M * 512, &hid));
        RET(wsalloc(h, (size_t)nseq * 512, &mean16));
        Epi f; f.relu = 1; f.out16 = hid; f.a_tiled = tiled;
        if (tiled) { f.rc_rpc = T * S; f.rc_clips = nb; f.rc_valid = rc_valid; }
        RET(gemm(h, JG_ST_GEMM, x16, 512, M, h->ff0, f));
        RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_group_mean, hid, nseq, S, 512, mean16, h->stream); }));
        Epi o; o.out32 = out_feats + (size_t)b0 * T * 1024;
        RET(gemm(h, JG_ST_GEMM, mean16, 512, nseq, h->ff2, o));
    }
    return JG_OK;
}

int gestsync_windows_impl(jg_handle* h, const float* x, int N, float* out, float* out_conv) {
    if (!h->gs_ready) JG_FAIL(h, JG_ERR_STATE, "GestSync weights not finalized");
    if (N <= 0) JG_FAIL(h, JG_ERR_ARG, "N must be positive");
    const int S = 21;
    const long sw = 1, sh = FW, st = (long)FH * FW, sc = 25 * st, sb = 3 * sc;
    const int am = audit_mask(h);
    const int wchunk = (am & AUD_CONV) ? 16 : std::max(1, h->chunk * 8);      // (fp32 conv stack: 0.26 GB per window)
    for (int n0 = 0; n0 < N; n0 += wchunk) {
        const int nb = std::min(wchunk, N - n0);
        h->ws.reset();
        float* conv;
        RET(wsalloc(h, (size_t)nb * S * 512, &conv));
        if (am & AUD_CONV) RET(gs_conv_stack32(h, x + (size_t)n0 * sb, 0, sb, st, sh, sw, sc, nb, 25, 0, conv));
        else RET(gs_conv_stack(h, x + (size_t)n0 * sb, 0, sb, st, sh, sw, sc, nb, 25, 0, conv));
        if (out_conv)
            RET(timed(h, JG_ST_MISC, [&] { return launch_transpose_tokens(conv, nb, S, 512, out_conv + (size_t)n0 * 512 * S, h->stream); }));
        const int M = nb * S;
        if (am & AUD_GS) {
            float *x32a, *hida, *fulla;
            RET(wsalloc(h, (size_t)M * 512, &x32a));
            RET(timed(h, JG_ST_MISC, [&] { return launch_window_gather(conv, h->gs_pe, nb, S, 1, S, 512, 0, 0, x32a, nullptr, h->stream); }));
            RET(gs_transformer32(h, x32a, nb, S));
            RET(wsalloc(h, (size_t)M * 512, &hida));
            RET(wsalloc(h, (size_t)M * 1024, &fulla));
            Epi32 fa; fa.act = 1;
            RET(gemm32(h, JG_ST_GEMM, x32a, 512, M, h->ff0, hida, fa));
            RET(gemm32(h, JG_ST_GEMM, hida, 512, M, h->ff2, fulla));
            RET(timed(h, JG_ST_MISC, [&] { return launch_transpose_tokens(fulla, nb, S, 1024, out + (size_t)n0 * 1024 * S, h->stream); }));
            continue;
        }
        float *x32, *full; f16 *x16, *hid;
        const bool tiled = gs_fused_plan(h, M, 0);
        RET(wsalloc(h, pad128(M) * 512, &x32));
        RET(wsalloc(h, pad128(M) * 512, &x16));
        RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_window_gather, conv, h->gs_pe, nb, S, 1, S, 512, 0, tiled, x32, x16, h->stream); }));
        RET(gs_transformer(h, x32, x16, nb, S, tiled));
        RET(wsalloc(h, (size_t)M * 512, &hid));
        RET(wsalloc(h, (size_t)M * 1024, &full));
        Epi f; f.relu = 1; f.out16 = hid; f.a_tiled = tiled;
        RET(gemm(h, JG_ST_GEMM, x16, 512, M, h->ff0, f));
        Epi o; o.out32 = full;
        RET(gemm(h, JG_ST_GEMM, hid, 512, M, h->ff2, o));
        RET(timed(h, JG_ST_MISC, [&] { return launch_transpose_tokens(full, nb, S, 1024, out + (size_t)n0 * 1024 * S, h->stream); }));
    }
    return JG_OK;
}

// ------------------------------------------------------------------------------------ JEGAL
// pre-norm encoder (modules.py:11-59) in place on x32; returns final-norm output in n16
// parts (diagnosis, option audit_jegal_parts): bit 1 = the attention sub-layers, bit 2 = the feed-forward sub-layers run on the fp32 audit
// kernels (encoder_sublayers32, with the audit path above)
int annotated_encoder(jg_handle* h, const EncLayer* layers, int nl, const LNp& fin, float* x32, f16* n16,
                      const float* mask, int B, int S, int D, int Dff, int parts = 0, float* n32_out = nullptr) {
    const int M = B * S, H = 8, dk = D / H;
    f16 *qkv, *att, *hid;
    float* scr32 = nullptr;
    RET(wsalloc(h, (size_t)M * 3 * D, &qkv));
    RET(wsalloc(h, (size_t)M * D, &att));
    RET(wsalloc(h, (size_t)M * Dff, &hid));
    if (parts & 6) RET(wsalloc(h, (size_t)M * (D + 3 * D + D + Dff), &scr32));
    for (int l = 0; l < nl; ++l) {
        const EncLayer& L = layers[l];
        Epi r; r.res = x32; r.ldr = D; r.out32 = x32;
        if (parts & 2) {
            RET(encoder_sublayers32(h, L, 1, x32, scr32, mask, B, S, D, Dff));
        } else {
            RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, x32, L.n1.w, L.n1.b, M, D, LN_ANNOTATED, 0, nullptr, n16, h->stream); }));
            Epi e; e.out16 = qkv;
            RET(gemm(h, JG_ST_GEMM, n16, D, M, L.qkv, e));
            RET(timed(h, JG_ST_ATTN, [&] { return LAUNCH(h, launch_attention, qkv, mask, B, S, H, dk, att, h->opts, h->stream); }));
            RET(gemm(h, JG_ST_GEMM, att, D, M, L.out, r));
        }
        if (parts & 4) {
            RET(encoder_sublayers32(h, L, 2, x32, scr32, mask, B, S, D, Dff));
        } else {
            RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, x32, L.n2.w, L.n2.b, M, D, LN_ANNOTATED, 0, nullptr, n16, h->stream); }));
            Epi f; f.relu = 1; f.out16 = hid;
            RET(gemm(h, JG_ST_GEMM, n16, D, M, L.ff1, f));
            RET(gemm(h, JG_ST_GEMM, hid, Dff, M, L.ff2, r));
        }
    }
    RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, x32, fin.w, fin.b, M, D, LN_ANNOTATED, 0, n32_out, n16, h->stream); }));
    return JG_OK;
}

int jegal_gestures_impl(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out) {
    if (!h->jg_ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || T <= 0 || T > 500) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and 0 < T <= 500 (PE table, modules.py:136)");
    if (audit_mask(h) & AUD_JG) return jegal_gestures_impl32(h, feats, mask, B, T, align, out);
    const int M = B * T;
    // the branch's two ends on the fp32 kernel (option jegal_fp32_ends; not in the plain-fp16 / bf16 reported modes, not while calibrating)
    const bool ends32 = h->jegal_fp32_ends && !h->calib && h->precision != JG_PREC_FP16 && h->precision != JG_PREC_BF16 && h->ip0.b32d && h->al_g2.b32d;
    const int parts = h->audit_jegal_parts | (ends32 ? 9 : 0);
    const bool ends_x3 = ends32 && !(h->audit_jegal_parts & 9);          // production: split operands on the fp16 matrix cores; diagnosis: fp32 MFMA
    f16 *f16in, *t16, *n16, *g16, *a16;
    float *t32, *x32, *n32 = nullptr;
    RET(wsalloc(h, (size_t)M * 1024, &f16in));
    RET(wsalloc(h, (size_t)M * 512, &t32));
    RET(wsalloc(h, (size_t)M * 512, &t16));
    RET(wsalloc(h, (size_t)M * 512, &x32));
    RET(wsalloc(h, (size_t)M * 512, &n16));
    if (parts & 8) RET(wsalloc(h, (size_t)M * 512, &n32));
    if (parts & 1) {
        RET(jegal_input32(h, feats, M, T, t32, x32, ends_x3));
    } else {
        RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_cast_f32_f16, feats, f16in, (long)M * 1024, h->stream); }));
        Epi e; e.out32 = t32;
        RET(gemm(h, JG_ST_GEMM, f16in, 1024, M, h->ip0, e));
        RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, t32, h->ip_ln.w, h->ip_ln.b, M, 512, LN_STD, 1, nullptr, t16, h->stream); }));
        Epi p; p.res = h->rgb_pe; p.ldr = 512; p.res_mod = T; p.out32 = x32;
        RET(gemm(h, JG_ST_GEMM, t16, 512, M, h->ip3, p));
    }
    RET(annotated_encoder(h, h->rgb_layers, 6, h->rgb_norm, x32, n16, mask, B, T, 512, 2048, parts, n32));
    if (parts & 8) return jegal_tail32(h, n32, M, align, out, ends_x3);
    if (!align) {
        Epi o; o.out32 = out;
        return gemm(h, JG_ST_GEMM, n16, 512, M, h->op_rgb, o);
    }
    RET(wsalloc(h, (size_t)M * 512, &g16));
    RET(wsalloc(h, (size_t)M * 512, &a16));
    Epi o1; o1.out16 = g16;
    RET(gemm(h, JG_ST_GEMM, n16, 512, M, h->op_rgb, o1));
    Epi o2; o2.relu = 1; o2.out16 = a16;
    RET(gemm(h, JG_ST_GEMM, g16, 512, M, h->al_g0, o2));
    Epi o3; o3.out32 = out;
    return gemm(h, JG_ST_GEMM, a16, 512, M, h->al_g2, o3);
}


// ------------------------------------------------------------------------------------ bias-corrected precision
// Weight rounding (w -> fp16) leaves an error (w - fp16(w)) . x per output that is the SAME for every token,
// so it does not average out downstream; its dominant part is (w - fp16(w)) . E[x].  A calibration pass runs the
// gesture path with hi+lo weights on a small batch, records E[x] of every Linear input, and folds that term into the
// bias.  Run-time GEMMs then use single fp16 weights (half the MFMAs and LDS traffic of the hi+lo split) at the split's
// accuracy (oracle/precision_probe.py).
int apply_bias_corrections(jg_handle* h, int models) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<float> mu;
    for (Lin* L : h->bc_layers) {
        if (L->mu_rows <= 0) continue;
        if (!((models >> (L->model - 1)) & 1)) { L->mu_rows = 0; continue; }
        mu.resize(L->K);
        HIPCHK(h, hipMemcpy(mu.data(), L->mu, sizeof(float) * L->K, hipMemcpyDeviceToHost));
        std::vector<float> nb(L->N);
        const double inv = 1.0 / (double)L->mu_rows;
        for (int n = 0; n < L->N; ++n) {
            double c = 0.0;
            const float* wr = &L->w32[(size_t)n * L->K];
            for (int k = 0; k < L->K; ++k) c += (double)(wr[k] - (float)(f16)wr[k]) * ((double)mu[k] * inv);
            nb[n] = L->b32[n] + (float)c;
        }
        HIPCHK(h, hipMemcpy(L->bias, nb.data(), sizeof(float) * L->N, hipMemcpyHostToDevice));
        L->mu_rows = 0;
        if (L->bc_pending) { L->wl = nullptr; L->bc_pending = false; }      // calibrated: single fp16 + corrected bias from here on
    }
    h->gs_qpe_valid = false;          // the projected positional rows carry layer 0's qkv bias
    return JG_OK;
}

int xlmr_encode_impl(jg_handle* h, const int32_t* ids, const int32_t* amask, int B, int L, float* out);

// Bias corrections of the XLM-RoBERTa layers (JG_PREC_FP16_BC): one pass with hi+lo weights over token ids records every Linear's
// input means; the run-time GEMMs then switch from hi+lo to single fp16 + corrected bias.  ids_dev / mask_dev (B, L): the CALLER's
// tokens (device); ids_dev == nullptr: built-in ids, uniform over the vocabulary, no padding (E[x] behind a LayerNorm is mostly
// its beta and the mean of the position / type embeddings -- true for the seeded test weights, unvalidated for the released
// checkpoint, which is why nothing calls this implicitly).
int calibrate_xlmr(jg_handle* h, const int32_t* ids_dev, const int32_t* mask_dev, int B, int L) {
    if (!h->xl_ready) JG_FAIL(h, JG_ERR_STATE, "XLM-RoBERTa weights not finalized");
    int32_t* dids = nullptr;
    if (!ids_dev) {
        B = 8; L = 64;
        std::vector<int32_t> ids((size_t)B * L);
        uint32_t x = 0xC0FFEE11u;
        for (auto& v : ids) {
            x ^= x << 13; x ^= x >> 17; x ^= x << 5;
            v = 3 + (int32_t)(x % (uint32_t)(h->xl_vocab > 3 ? h->xl_vocab - 3 : 1));
        }
        for (int b = 0; b < B; ++b) { ids[(size_t)b * L] = 0; ids[(size_t)b * L + L - 1] = 2; }       // <s> ... </s>
        HIPCHK(h, hipMalloc(&dids, ids.size() * sizeof(int32_t)));
        if (hipMemcpy(dids, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dids); JG_FAIL(h, JG_ERR_HIP, "hipMemcpy failed"); }
        ids_dev = dids;
        mask_dev = nullptr;
    }
    float* out = nullptr;
    if (hipMalloc(&out, (size_t)B * L * 768 * sizeof(float)) != hipSuccess) { if (dids) (void)hipFree(dids); JG_FAIL(h, JG_ERR_HIP, "hipMalloc failed"); }
    int rc = JG_OK;
    for (Lin* Ly : h->bc_layers) {
        if (Ly->model != 3) continue;
        if (hipMemsetAsync(Ly->mu, 0, sizeof(float) * Ly->K, h->stream) != hipSuccess) rc = JG_ERR_HIP;
        Ly->mu_rows = 0;
    }
    if (rc == JG_OK) {
        h->calib = true;
        h->ws.reset();
        rc = xlmr_encode_impl(h, ids_dev, mask_dev, B, L, out);
        h->calib = false;
    }
    if (rc == JG_OK) rc = apply_bias_corrections(h, 4);
    (void)hipStreamSynchronize(h->stream);
    if (dids) (void)hipFree(dids);
    (void)hipFree(out);
    return rc;
}

// frames == nullptr: built-in deterministic calibration clips (uniform u8 noise, rows 0..109 zeroed like the
// face-mask rectangle), so results do not depend on what the engine happens to see first.
// models: bit 0 GestSync, bit 1 JEGAL -- only the bias-corrected layers of these models receive new corrections (the pass
// itself always runs the whole gesture path: JEGAL's input means depend on GestSync's output)
int calibrate_impl(jg_handle* h, const void* frames, int dtype, int B, int T, int models) {
    if (h->bc_layers.empty()) return JG_OK;
    void* own = nullptr;
    if (!frames) {
        B = 4; T = 16; dtype = JG_U8;
        const size_t n = (size_t)B * T * FH * FW * 3;
        std::vector<uint8_t> host(n);
        uint32_t x = 0x9E3779B9u;
        for (size_t i = 0; i < n; ++i) {
            x ^= x << 13; x ^= x >> 17; x ^= x << 5;
            host[i] = (uint8_t)(x >> 24);
        }
        for (int f = 0; f < B * T; ++f) std::memset(&host[(size_t)f * FH * FW * 3], 0, (size_t)110 * FW * 3);
        HIPCHK(h, hipMalloc(&own, n));
        HIPCHK(h, hipMemcpy(own, host.data(), n, hipMemcpyHostToDevice));
        frames = own;
    }
    float *feats = nullptr, *emb = nullptr;
    HIPCHK(h, hipMalloc(&feats, (size_t)B * T * 1024 * sizeof(float)));
    HIPCHK(h, hipMalloc(&emb, (size_t)B * T * 512 * sizeof(float)));
    for (Lin* L : h->bc_layers) {
        if (hipMemsetAsync(L->mu, 0, sizeof(float) * L->K, h->stream) != hipSuccess) { (void)hipFree(feats); (void)hipFree(emb); if (own) (void)hipFree(own); JG_FAIL(h, JG_ERR_HIP, "hipMemsetAsync(mu) failed"); }
        L->mu_rows = 0;
    }
    h->calib = true;
    int rc = JG_OK;
    if (h->gs_ready) {
        rc = gestsync_clip_impl(h, frames, dtype, B, T, feats);
    } else {
        std::vector<float> hf((size_t)B * T * 1024);          // no GestSync loaded: standard-normal stand-in features
        uint32_t x = 0x2545F491u;
        for (auto& v : hf) {
            float s = 0.f;
            for (int i = 0; i < 12; ++i) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; s += (float)(x >> 8) * (1.0f / 16777216.0f); }
            v = s - 6.0f;
        }
        if (hipMemcpy(feats, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = JG_ERR_HIP;
    }
    if (rc == JG_OK && h->jg_ready) {
        h->ws.reset();
        rc = jegal_gestures_impl(h, feats, nullptr, B, T, 1, emb);
    }
    h->calib = false;
    if (rc == JG_OK) rc = apply_bias_corrections(h, models);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(feats);
    (void)hipFree(emb);
    if (own) (void)hipFree(own);
    return rc;
}

int audio_len(int Tm) {
    const int h1 = (Tm + 2 - 3) / 2 + 1;
    return (h1 + 2 - 3) / 2 + 1;
}

// valid_host (optional, host [B]): clip b holds valid_host[b] mel frames, the rest of its Tm rows is batch padding.  Every layer's
// rows beyond the clip's own extent are zeroed (launch_zero_tail), i.e. each clip sees the zero padding it would see alone -- the
// reference's dataset driver runs one clip per step (extract_jegal_embs.py:141), so its result never depends on a longer neighbour.
int jegal_audio_impl(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_host, float* out) {
    if (!h->jg_ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || Tm < 4) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and Tm >= 4");
    if (audit_mask(h) & AUD_CONTENT) return jegal_audio_impl32(h, mel, B, Tm, valid_host, out);
    const int F = 80;
    const ConvGeom g3 = geom(Tm, F, 32, 3, 3, 2, 2, 1, 1);
    const ConvGeom g6 = geom(g3.OH, g3.OW, 64, 3, 3, 2, 2, 1, 1);
    const ConvGeom g9 = geom(g6.OH, g6.OW, 128, 3, 3, 1, 3, 1, 1);
    const ConvGeom g12 = geom(g9.OH, g9.OW, 256, 3, 3, 1, 3, 1, 1);
    const ConvGeom g15 = geom(g12.OH, g12.OW, 256, 1, 1, 1, 3, 0, 0);
    if (g15.OW != 1) JG_FAIL(h, JG_ERR_ARG, "audio CNN must reduce 80 mel bands to 1");
    int* valid = nullptr;
    if (valid_host) {
        bool ragged = false;
        for (int b = 0; b < B; ++b) {
            if (valid_host[b] < 4 || valid_host[b] > Tm) JG_FAIL(h, JG_ERR_ARG, "valid_tm[%d] = %d outside 4..Tm = %d", b, valid_host[b], Tm);
            ragged |= valid_host[b] != Tm;
        }
        if (ragged) {
            RET(wsalloc(h, (size_t)B, &valid));
            RET(upload_i32_async(h, valid_host, (size_t)B, valid));
        }
    }
    f16 *c0, *c3, *c6, *c9, *c12, *c15;
    const long M0 = (long)B * Tm * F;
    RET(wsalloc(h, (size_t)M0 * 32, &c0));
    RET(wsalloc(h, (size_t)B * g3.OH * g3.OW * 64, &c3));
    RET(wsalloc(h, (size_t)B * g6.OH * g6.OW * 128, &c6));
    RET(wsalloc(h, (size_t)B * g9.OH * g9.OW * 256, &c9));
    RET(wsalloc(h, (size_t)B * g12.OH * g12.OW * 256, &c12));
    RET(wsalloc(h, (size_t)B * g15.OH * 256, &c15));
    auto tail = [&](f16* x, int halvings, const ConvGeom& g, int C) -> int {
        if (!valid) return JG_OK;
        return timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_zero_tail, x, (const int*)valid, halvings, B, g.OH, (long)g.OW * C, h->stream); });
    };
    // cnn.0 + BN + ReLU straight from the mel frames (round 2: im2col + a K = 32 GEMM on the register-staged kernel)
    RET(timed(h, JG_ST_CONV, [&] { return LAUNCH(h, launch_audio_conv0, mel, B, Tm, F, h->a0.wh, h->a0.wl, h->a0.bias, c0, (const int*)valid, h->stream); }));
    Epi e; e.relu = 1;
    e.out16 = c3; RET(gemm(h, JG_ST_CONV, c0, 0, B * g3.OH * g3.OW, h->a3, e, &g3));
    RET(tail(c3, 1, g3, 64));
    e.out16 = c6; RET(gemm(h, JG_ST_CONV, c3, 0, B * g6.OH * g6.OW, h->a6, e, &g6));
    RET(tail(c6, 2, g6, 128));
    e.out16 = c9; RET(gemm(h, JG_ST_CONV, c6, 0, B * g9.OH * g9.OW, h->a9, e, &g9));
    RET(tail(c9, 2, g9, 256));
    e.out16 = c12; RET(gemm(h, JG_ST_CONV, c9, 0, B * g12.OH * g12.OW, h->a12, e, &g12));
    e.relu = 0;      // (cnn.15 is 1x1: rows of c12 beyond a clip's extent only reach output rows beyond it, which callers strip)
    e.out16 = c15; RET(gemm(h, JG_ST_CONV, c12, 0, B * g15.OH, h->a15, e, &g15));
    Epi o; o.out32 = out;
    return gemm(h, JG_ST_GEMM, c15, 256, B * g15.OH, h->op_audio, o);
}

int jegal_text_impl(jg_handle* h, const float* states, const float* mask, int B, int L, float* out) {
    if (!h->jg_ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || L <= 0) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and L > 0");
    if (audit_mask(h) & AUD_CONTENT) return jegal_text_impl32(h, states, mask, B, L, out);
    const int M = B * L;
    float* x32; f16* n16;
    RET(wsalloc(h, (size_t)M * 768, &x32));
    RET(wsalloc(h, (size_t)M * 768, &n16));
    HIPCHK(h, hipMemcpyAsync(x32, states, (size_t)M * 768 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    const bool x3 = h->jegal_fp32_ends && !h->calib && h->precision != JG_PREC_FP16 && h->precision != JG_PREC_BF16 && h->op_text.wl;
    float* n32 = nullptr;
    if (x3) RET(wsalloc(h, (size_t)M * 768, &n32));
    RET(annotated_encoder(h, h->text_layers, 3, h->text_norm, x32, n16, mask, B, L, 768, 3072, 0, n32));
    if (x3) return gemm_x3(h, JG_ST_GEMM, n32, 768, M, h->op_text, out);      // proj_op_text from the final norm's fp32 rows (round 6)
    Epi o; o.out32 = out;
    return gemm(h, JG_ST_GEMM, n16, 768, M, h->op_text, o);
}

// ------------------------------------------------------------------------------------ XLM-RoBERTa (text front end)
// State-dict keys: those of transformers.XLMRobertaModel (add_pooling_layer irrelevant) under the prefix "xlmr.":
// xlmr.embeddings.{word,position,token_type}_embeddings.weight, xlmr.embeddings.LayerNorm.{weight,bias},
// xlmr.encoder.layer.<i>.attention.self.{query,key,value}.{weight,bias}, .attention.output.{dense,LayerNorm}.*,
// .intermediate.dense.*, .output.{dense,LayerNorm}.*.  The number of layers is the number present; hidden size 768,
// 12 heads of 64, intermediate 3072 (xlm-roberta-base); the vocabulary and position table sizes come from the tensors.
int finalize_xlmr(jg_handle* h) {
    h->xl_ready = false;
    drop_model(h, h->wallocs_xl, 3);          // frees the previous weights, drops its bias-corrected layers from the calibration list
    h->xl_layers.clear();
    h->wallocs = &h->wallocs_xl;
    constexpr int D = 768, DFF = 3072;
    const HostTensor* t = find(h, "xlmr.embeddings.word_embeddings.weight");
    if (!t || t->numel() % D) JG_FAIL(h, JG_ERR_WEIGHT, "missing or malformed 'xlmr.embeddings.word_embeddings.weight'");
    h->xl_vocab = (int)(t->numel() / D);
    RET(upload(h, t->v, &h->xl_word));
    t = find(h, "xlmr.embeddings.position_embeddings.weight");
    if (!t || t->numel() % D) JG_FAIL(h, JG_ERR_WEIGHT, "missing or malformed 'xlmr.embeddings.position_embeddings.weight'");
    h->xl_maxpos = (int)(t->numel() / D);
    RET(upload(h, t->v, &h->xl_pos));
    RET(need(h, "xlmr.embeddings.token_type_embeddings.weight", D, &t));
    RET(upload(h, t->v, &h->xl_type));
    RET(make_ln(h, "xlmr.embeddings.LayerNorm.weight", "xlmr.embeddings.LayerNorm.bias", D, &h->xl_emb_ln));
    // Implicit LayerNorm (xlmr_encode_folded): the Linear BEHIND a LayerNorm(gamma, beta) is packed as W diag(gamma) with bias
    // b + W beta (fold_consumer), the Linear whose output is ADDED to that LayerNorm's output takes beta into its bias (the
    // gamma (x - mean) rstd part is recomputed from the un-normalised stream in its epilogue).
    // (the implicit-LayerNorm epilogues exist in the LDS-DMA kernel only; the fp32 audit path runs the explicit LayerNorms on the
    // un-folded matrices, so audit weights switch the folding off)
    const bool fold = h->xl_fold_opt && h->opts.gemm_glds && !h->audit_weights && h->precision != JG_PREC_FP32;
    const HostTensor *pg, *pb;          // the LayerNorm in front of the current sub-layer
    RET(need(h, "xlmr.embeddings.LayerNorm.weight", D, &pg));
    RET(need(h, "xlmr.embeddings.LayerNorm.bias", D, &pb));
    auto fold_consumer = [](std::vector<float>& w, std::vector<float>& b, int N, int K, const std::vector<float>& g, const std::vector<float>& be) {
        for (int n = 0; n < N; ++n) {
            double acc = 0.0;
            float* wr = &w[(size_t)n * K];
            for (int k = 0; k < K; ++k) {
                acc += (double)wr[k] * (double)be[k];
                wr[k] *= g[k];
            }
            b[n] = (float)((double)b[n] + acc);
        }
    };
    auto make_producer = [&](const std::string& wname, const std::string& bname, int N, int K, const std::vector<float>& be, Lin* Lo) -> int {
        const HostTensor *w, *b;
        RET(need(h, wname, (int64_t)N * K, &w));
        RET(need(h, bname, N, &b));
        std::vector<float> bb = b->v;
        for (int n = 0; n < N; ++n) bb[n] += be[n];
        return pack_matrix(h, w->v, bb, N, K, LK_XLMR, Lo);
    };
    int nl = 0;
    while (find(h, "xlmr.encoder.layer." + std::to_string(nl) + ".attention.self.query.weight")) ++nl;
    if (nl == 0) JG_FAIL(h, JG_ERR_WEIGHT, "no 'xlmr.encoder.layer.*' weights");
    h->xl_layers.resize(nl);
    for (int l = 0; l < nl; ++l) {
        const std::string p = "xlmr.encoder.layer." + std::to_string(l);
        EncLayer* L = &h->xl_layers[l];
        std::vector<float> w((size_t)3 * D * D), b((size_t)3 * D);
        const char* names[3] = {"query", "key", "value"};
        for (int i = 0; i < 3; ++i) {
            const HostTensor *wi, *bi;
            RET(need(h, p + ".attention.self." + names[i] + ".weight", (int64_t)D * D, &wi));
            RET(need(h, p + ".attention.self." + names[i] + ".bias", D, &bi));
            std::memcpy(&w[(size_t)i * D * D], wi->v.data(), sizeof(float) * D * D);
            std::memcpy(&b[(size_t)i * D], bi->v.data(), sizeof(float) * D);
        }
        if (!fold) {
            RET(pack_matrix(h, w, b, 3 * D, D, LK_XLMR, &L->qkv));
            RET(make_linear(h, p + ".attention.output.dense.weight", p + ".attention.output.dense.bias", D, D, &L->out, LK_XLMR));
            RET(make_ln(h, p + ".attention.output.LayerNorm.weight", p + ".attention.output.LayerNorm.bias", D, &L->n1));
            RET(make_linear(h, p + ".intermediate.dense.weight", p + ".intermediate.dense.bias", DFF, D, &L->ff1, LK_XLMR));
            RET(make_linear(h, p + ".output.dense.weight", p + ".output.dense.bias", D, DFF, &L->ff2, LK_XLMR));
            RET(make_ln(h, p + ".output.LayerNorm.weight", p + ".output.LayerNorm.bias", D, &L->n2));
            continue;
        }
        fold_consumer(w, b, 3 * D, D, pg->v, pb->v);
        RET(pack_matrix(h, w, b, 3 * D, D, LK_XLMR, &L->qkv, true));
        RET(make_producer(p + ".attention.output.dense.weight", p + ".attention.output.dense.bias", D, D, pb->v, &L->out));
        RET(make_ln(h, p + ".attention.output.LayerNorm.weight", p + ".attention.output.LayerNorm.bias", D, &L->n1));
        RET(need(h, p + ".attention.output.LayerNorm.weight", D, &pg));
        RET(need(h, p + ".attention.output.LayerNorm.bias", D, &pb));
        {
            const HostTensor *w1, *b1;
            RET(need(h, p + ".intermediate.dense.weight", (int64_t)DFF * D, &w1));
            RET(need(h, p + ".intermediate.dense.bias", DFF, &b1));
            std::vector<float> wf = w1->v, bf1 = b1->v;
            fold_consumer(wf, bf1, DFF, D, pg->v, pb->v);
            RET(pack_matrix(h, wf, bf1, DFF, D, LK_XLMR, &L->ff1, true));
        }
        RET(make_producer(p + ".output.dense.weight", p + ".output.dense.bias", D, DFF, pb->v, &L->ff2));
        RET(make_ln(h, p + ".output.LayerNorm.weight", p + ".output.LayerNorm.bias", D, &L->n2));
        RET(need(h, p + ".output.LayerNorm.weight", D, &pg));
        RET(need(h, p + ".output.LayerNorm.bias", D, &pb));
    }
    h->xl_layers_n = nl;
    h->xl_folded = fold;
    h->xl_ready = true;
    return JG_OK;
}

// XLMRobertaModel.forward(input_ids, attention_mask).last_hidden_state: post-norm BERT layers (LayerNorm eps 1e-5, exact GELU),
// the key padding mask of attention_mask, position ids from the non-pad tokens (padding_idx = 1).
// The same forward pass with IMPLICIT LayerNorms (option xlmr_fold, default): post-norm layers x' = LN(x + f(x)) are carried as the
// UN-normalised sums x (two fp16 planes hi + lo; hi is the next GEMM's A operand) plus (mean, rstd) per row.  A Linear behind a
// LayerNorm runs on x with W diag(gamma) and finishes rstd (acc - mean c1) + (b + W beta) in its epilogue; a Linear whose output is
// added to LN(x) recomputes gamma (x - mean) rstd + beta from the planes there, writes the new planes in place and the per-64-column
// (sum, sum of squares) of the new rows; launch_ln_stats (one thread per row) makes the next (mean, rstd).  Per pass: 25 LayerNorm
// launches over fp32 rows (10 % of the time, 18 B per element and sub-layer through HBM) become 24 x 3 us and 8 B per element.
int xlmr_encode_folded(jg_handle* h, const int32_t* ids, const int32_t* amask, int B, int L, float* out) {
    constexpr int D = 768, DFF = 3072, H = 12, P = D / 64;
    const int M = B * L;
    const int Mp = M < 128 ? 128 : M;             // the LDS-DMA GEMMs want >= 128 rows: short batches carry zero rows behind the tokens
    float *part, *stats, *mk = nullptr;
    f16 *xh, *xl, *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)Mp * D, &xh));
    RET(wsalloc(h, (size_t)Mp * D, &xl));
    RET(wsalloc(h, (size_t)Mp * P * 2, &part));
    RET(wsalloc(h, (size_t)Mp * 2, &stats));
    RET(wsalloc(h, (size_t)Mp * 3 * D, &qkv));
    RET(wsalloc(h, (size_t)Mp * D, &att));
    RET(wsalloc(h, (size_t)Mp * DFF, &hid));
    if (Mp > M) {
        HIPCHK(h, hipMemsetAsync(xh + (size_t)M * D, 0, (size_t)(Mp - M) * D * sizeof(f16), h->stream));
        HIPCHK(h, hipMemsetAsync(xl + (size_t)M * D, 0, (size_t)(Mp - M) * D * sizeof(f16), h->stream));
        HIPCHK(h, hipMemsetAsync(part + (size_t)M * P * 2, 0, (size_t)(Mp - M) * P * 2 * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(att + (size_t)M * D, 0, (size_t)(Mp - M) * D * sizeof(f16), h->stream));
    }
    if (amask) {
        RET(wsalloc(h, (size_t)M, &mk));
        RET(timed(h, JG_ST_MISC, [&] { return launch_mask_i32_f32(amask, mk, M, h->stream); }));
    }
    RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_xlmr_embed_planes, ids, B, L, D, 1, h->xl_vocab, h->xl_maxpos, h->xl_word, h->xl_pos, h->xl_type, xh, xl, part, h->stream); }));
    auto ln_stats = [&]() { return timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_ln_stats, part, Mp, P, stats, h->stream); }); };
    RET(ln_stats());
    const LNp* prev = &h->xl_emb_ln;
    for (int l = 0; l < h->xl_layers_n; ++l) {
        const EncLayer& Ly = h->xl_layers[l];
        Epi q; q.out16 = qkv; q.ln_mode = 1; q.ln_stats = stats; q.calib_rows = M;
        RET(gemm(h, JG_ST_GEMM, xh, D, Mp, Ly.qkv, q));
        RET(timed(h, JG_ST_ATTN, [&] { return LAUNCH(h, launch_attention, qkv, mk, B, L, H, 64, att, h->opts, h->stream); }));
        Epi o; o.ln_mode = 2; o.ln_stats = stats; o.x_hi = xh; o.x_lo = xl; o.ln_gamma = prev->w; o.stat_out = part; o.calib_rows = M;
        RET(gemm(h, JG_ST_GEMM, att, D, Mp, Ly.out, o));
        RET(ln_stats());
        Epi f; f.relu = 2; f.out16 = hid; f.ln_mode = 1; f.ln_stats = stats; f.calib_rows = M;
        RET(gemm(h, JG_ST_GEMM, xh, D, Mp, Ly.ff1, f));
        o.ln_gamma = Ly.n1.w;
        RET(gemm(h, JG_ST_GEMM, hid, DFF, Mp, Ly.ff2, o));
        if (l + 1 < h->xl_layers_n) RET(ln_stats());
        prev = &Ly.n2;
    }
    return timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm_planes, xh, xl, prev->w, prev->b, M, D, out, h->stream); });
}

int xlmr_encode_impl(jg_handle* h, const int32_t* ids, const int32_t* amask, int B, int L, float* out) {
    if (!h->xl_ready) JG_FAIL(h, JG_ERR_STATE, "XLM-RoBERTa weights not finalized (jg_finalize_weights(h, 4))");
    if (B <= 0 || L <= 0 || L > h->xl_maxpos - 2) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and 0 < L <= %d", h->xl_maxpos - 2);
    if (audit_mask(h) & AUD_XLMR) return xlmr_encode_impl32(h, ids, amask, B, L, out);
    if (h->xl_folded && !h->opts.gemm_glds)
        JG_FAIL(h, JG_ERR_STATE, "the XLM-RoBERTa weights were packed for the implicit-LayerNorm pass, which needs the LDS-DMA GEMM: set option "
                                 "gemm_glds=0 (or xlmr_fold=0) BEFORE jg_finalize_weights(h, 4)");
    if (h->xl_folded) return xlmr_encode_folded(h, ids, amask, B, L, out);
    constexpr int D = 768, DFF = 3072, H = 12;
    const int M = B * L;
    float *x32, *t32, *mk = nullptr;
    f16 *x16, *qkv, *att, *hid;
    RET(wsalloc(h, (size_t)M * D, &x32));
    RET(wsalloc(h, (size_t)M * D, &x16));
    RET(wsalloc(h, (size_t)M * D, &t32));
    RET(wsalloc(h, (size_t)M * 3 * D, &qkv));
    RET(wsalloc(h, (size_t)M * D, &att));
    RET(wsalloc(h, (size_t)M * DFF, &hid));
    if (amask) {
        RET(wsalloc(h, (size_t)M, &mk));
        RET(timed(h, JG_ST_MISC, [&] { return launch_mask_i32_f32(amask, mk, M, h->stream); }));
    }
    RET(timed(h, JG_ST_MISC, [&] { return launch_xlmr_embed(ids, B, L, D, 1, h->xl_vocab, h->xl_maxpos, h->xl_word, h->xl_pos, h->xl_type, t32, h->stream); }));
    RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, t32, h->xl_emb_ln.w, h->xl_emb_ln.b, M, D, LN_STD, 0, x32, x16, h->stream); }));
    for (int l = 0; l < h->xl_layers_n; ++l) {
        const EncLayer& Ly = h->xl_layers[l];
        const bool last = l + 1 == h->xl_layers_n;
        Epi e; e.out16 = qkv;
        RET(gemm(h, JG_ST_GEMM, x16, D, M, Ly.qkv, e));
        RET(timed(h, JG_ST_ATTN, [&] { return LAUNCH(h, launch_attention, qkv, mk, B, L, H, 64, att, h->opts, h->stream); }));
        Epi r; r.res = x32; r.ldr = D; r.out32 = t32;
        RET(gemm(h, JG_ST_GEMM, att, D, M, Ly.out, r));
        RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, t32, Ly.n1.w, Ly.n1.b, M, D, LN_STD, 0, x32, x16, h->stream); }));
        Epi f; f.relu = 2; f.out16 = hid;             // exact GELU in the GEMM epilogue (round 2: fp32 M x 3072 out + a separate kernel)
        RET(gemm(h, JG_ST_GEMM, x16, D, M, Ly.ff1, f));
        RET(gemm(h, JG_ST_GEMM, hid, DFF, M, Ly.ff2, r));
        RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, t32, Ly.n2.w, Ly.n2.b, M, D, LN_STD, 0, last ? out : x32, x16, h->stream); }));
    }
    return JG_OK;
}

int fuse_content_impl(jg_handle* h, const float* fused, int rows, float* out) {
    if (!h->jg_ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (rows <= 0) JG_FAIL(h, JG_ERR_ARG, "rows must be positive");
    if (audit_mask(h) & AUD_CONTENT) return fuse_content_impl32(h, fused, rows, out);
    // round 6: like the gesture branch's ends, the content path's last four GEMMs keep fp32 activations and run on the split-operand
    // kernel (fp32-grade products on the fp16 matrix cores; a few hundred rows: the cost is a launch either way)
    if (h->jegal_fp32_ends && !h->calib && h->precision != JG_PREC_FP16 && h->precision != JG_PREC_BF16 && h->fu0.wl && h->fu2.wl && h->al_c0.wl && h->al_c2.wl) {
        float *a32, *b32;
        RET(wsalloc(h, (size_t)rows * 512, &a32));
        RET(wsalloc(h, (size_t)rows * 512, &b32));
        Epi32 r; r.act = 1;
        RET(gemm_x3(h, JG_ST_GEMM, fused, 512, rows, h->fu0, a32, r));
        RET(gemm_x3(h, JG_ST_GEMM, a32, 512, rows, h->fu2, b32));
        RET(gemm_x3(h, JG_ST_GEMM, b32, 512, rows, h->al_c0, a32, r));
        return gemm_x3(h, JG_ST_GEMM, a32, 512, rows, h->al_c2, out);
    }
    f16 *x16, *a16, *b16;
    RET(wsalloc(h, (size_t)rows * 512, &x16));
    RET(wsalloc(h, (size_t)rows * 512, &a16));
    RET(wsalloc(h, (size_t)rows * 512, &b16));
    RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_cast_f32_f16, fused, x16, (long)rows * 512, h->stream); }));
    Epi r; r.relu = 1; r.out16 = a16;
    RET(gemm(h, JG_ST_GEMM, x16, 512, rows, h->fu0, r));
    Epi p; p.out16 = b16;
    RET(gemm(h, JG_ST_GEMM, a16, 512, rows, h->fu2, p));
    RET(gemm(h, JG_ST_GEMM, b16, 512, rows, h->al_c0, r));
    Epi o; o.out32 = out;
    return gemm(h, JG_ST_GEMM, a16, 512, rows, h->al_c2, o);
}

// Run a batch of B independent items (clips, token sequences) as parts on the lane streams (option "dual_stream", jg_handle::lane_*):
// run_part(b0, nb) enqueues one part on h->stream / h->ws, which are the current lane's while it is called.  Entry: the lane streams
// wait for the caller's stream; exit: the caller's stream waits for every lane.  Small batches run as one part on the caller's stream.
template <class F>
int run_in_lanes(jg_handle* h, int B, int T, F&& run_part, int equal_lanes = 0) {
    // equal_lanes = 0: two lanes, the first gets dual_split eighths of the batch (the gesture path); n > 0: n equal parts.
    // (small parts would fall below the LDS-DMA GEMM's 128-row minimum in the JEGAL branch and take the register-staged kernel,
    // whose summation order differs in the last bit: keep every part in the regime of the whole batch)
    const int nl = equal_lanes ? equal_lanes : 2;
    int start[jg_handle::MAX_LANES + 1];
    start[0] = 0;
    for (int l = 1; l <= nl; ++l) start[l] = equal_lanes ? (int)((long)B * l / nl) : (l == 1 ? (B * h->dual_split + 4) / 8 : B);
    int smallest = B;
    for (int l = 0; l < nl; ++l) smallest = std::min(smallest, start[l + 1] - start[l]);
    if (!h->dual_stream || h->calib || nl < 2 || B < 8 || (long)smallest * T < 256 || audit_mask(h)) return run_part(0, B);
    for (int l = 0; l < nl; ++l)
        if (!h->lane_stream[l]) {
            const bool high = l < 2 && (h->lane_priority >> (l == 1 ? 0 : 1) & 1);
            int least = 0, greatest = 0;
            if (high && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least &&
                hipStreamCreateWithPriority(&h->lane_stream[l], hipStreamNonBlocking, greatest) == hipSuccess) {
                // a lane of the high-priority queue pool
            } else {
                (void)hipGetLastError();          // no priority levels on this device / runtime: a normal-priority lane
                h->lane_stream[l] = nullptr;
                HIPCHK(h, hipStreamCreateWithFlags(&h->lane_stream[l], hipStreamNonBlocking));
            }
        }
    for (int e = 0; e < nl + 1; ++e)
        if (!h->lane_ev[e]) HIPCHK(h, hipEventCreateWithFlags(&h->lane_ev[e], hipEventDisableTiming));
    hipStream_t user = h->stream;
    HIPCHK(h, hipEventRecord(h->lane_ev[0], user));
    int rc = JG_OK;
    for (int l = 0; l < nl && rc == JG_OK; ++l) {
        if (hipStreamWaitEvent(h->lane_stream[l], h->lane_ev[0], 0) != hipSuccess) { rc = JG_ERR_HIP; break; }
        h->stream = h->lane_stream[l];
        std::swap(h->ws, h->lane_ws[l]);
        h->opts.lanes_active = true;
        rc = run_part(start[l], start[l + 1] - start[l]);
        h->opts.lanes_active = false;
        std::swap(h->ws, h->lane_ws[l]);
        h->stream = user;
        // the join is unconditional: when run_part failed half way, the kernels it did enqueue on the lane still read the caller's
        // frames / write its output, and the caller's stream must stay ordered behind them (it may free both right after the error)
        if (hipEventRecord(h->lane_ev[1 + l], h->lane_stream[l]) != hipSuccess || hipStreamWaitEvent(user, h->lane_ev[1 + l], 0) != hipSuccess) {
            (void)hipStreamSynchronize(h->lane_stream[l]);
            if (rc == JG_OK) rc = JG_ERR_HIP;
        }
    }
    if (rc == JG_ERR_HIP && h->err.empty()) h->err = "lane stream / event call failed";
    return rc;
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

const char* jg_stage_name(int s) {
    static const char* n[] = {"stack_frames", "conv1", "maxpool", "conv2-fc6+audio_cnn", "gemm", "attention", "layernorm", "misc", "conv1_aux"};
    return (s >= 0 && s < JG_ST_COUNT) ? n[s] : "?";
}

int jg_create(int device, jg_handle** out) {
    if (!out) return JG_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return JG_ERR_HIP;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess) return JG_ERR_HIP;
    jg_handle* h = new jg_handle();
    h->device = device;
    int rc = JG_OK;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) rc = JG_ERR_HIP;
    if (rc == JG_OK && engine_opts_init(h->opts, device) != hipSuccess) rc = JG_ERR_HIP;
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    if (rc != JG_OK) { if (h->own_stream) (void)hipStreamDestroy(h->own_stream); delete h; return rc; }
    h->stream = h->own_stream;
    *out = h;
    return JG_OK;
}

int jg_destroy(jg_handle* h) {
    if (!h) return JG_OK;
    {
        DeviceGuard dg(h->device);
        (void)hipDeviceSynchronize();
        for (auto& r : h->recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        for (void* p : h->wallocs_gs) (void)hipFree(p);
        for (void* p : h->wallocs_jg) (void)hipFree(p);
        for (void* p : h->wallocs_xl) (void)hipFree(p);
        if (h->feats) (void)hipFree(h->feats);
        if (h->gs_qpe) (void)hipFree(h->gs_qpe);
        h->ws.release();
        for (auto& kv : h->ws_parked) kv.second.release();
        for (int l = 0; l < jg_handle::MAX_LANES; ++l) { h->lane_ws[l].release(); if (h->lane_stream[l]) (void)hipStreamDestroy(h->lane_stream[l]); }
        for (int e = 0; e < jg_handle::MAX_LANES + 1; ++e) if (h->lane_ev[e]) (void)hipEventDestroy(h->lane_ev[e]);
        engine_opts_release(h->opts);
        if (h->comm && rccl().ok) (void)rccl().CommDestroy(h->comm);
        for (auto& sl : h->stage_ring) { if (sl.ev) (void)hipEventDestroy(sl.ev); if (sl.host) (void)hipHostFree(sl.host); }
        if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    }
    delete h;
    return JG_OK;
}
const char* jg_last_error(jg_handle* h) { return h ? h->err.c_str() : "null handle"; }

// The workspace arena is stream-ordered (every entry point resets and re-uses it), so it belongs to ONE stream: a handle that is
// driven from several streams -- e.g. JEGAL.forward_inference runs the content path on a side stream beside the gesture encoder --
// keeps one arena per stream and switches with the stream.  (Before round 4 two calls on two un-synchronised streams shared one arena.)
int jg_set_stream(jg_handle* h, void* s) {
    if (!h) return JG_ERR_ARG;
    hipStream_t ns = reinterpret_cast<hipStream_t>(s);   // NULL is the legacy default stream, used as such
    if (ns != h->stream) {
        static unsigned long tick = 0;
        h->ws.tick = ++tick;
        std::swap(h->ws, h->ws_parked[h->stream]);       // park the current arena under its stream ...
        std::swap(h->ws, h->ws_parked[ns]);              // ... and take the new stream's (empty the first time)
        h->ws_parked.erase(ns);
        // A caller cycling through many streams (a fresh torch.cuda.Stream per batch): at most 6 parked arenas (>= 1 GiB each, INTEGRATION.md
        // section 6) -- the LEAST RECENTLY used one goes, alone.  Its stream may no longer exist, so the device is synchronised rather
        // than the stream (hipFree would wait for the device anyway); the debug pointers into a released arena are dropped with it.
        while (h->ws_parked.size() > 6) {
            auto lru = h->ws_parked.begin();
            for (auto it = h->ws_parked.begin(); it != h->ws_parked.end(); ++it)
                if (it->second.tick < lru->second.tick) lru = it;
            DeviceGuard dg(h->device);
            (void)hipDeviceSynchronize();
            lru->second.release();
            h->ws_parked.erase(lru);
            h->last_rowskip = nullptr;                   // (they may point into the arena that was just released)
            h->last_conv_totals = nullptr;
        }
        h->stream = ns;
    }
    return JG_OK;
}

int jg_set_precision(jg_handle* h, int mode) {
    if (!h) return JG_ERR_ARG;
    if (mode < JG_PREC_FP16 || mode > JG_PREC_FP32) JG_FAIL(h, JG_ERR_ARG, "unknown precision mode %d", mode);
    if ((h->gs_ready || h->jg_ready || h->xl_ready) && mode != h->precision) JG_FAIL(h, JG_ERR_STATE, "set the precision before jg_finalize_weights");
    h->precision = mode;
    h->bf16 = mode == JG_PREC_BF16;
    return JG_OK;
}

int jg_set_chunk(jg_handle* h, int c) {
    if (!h) return JG_ERR_ARG;
    if (c < 1) JG_FAIL(h, JG_ERR_ARG, "clips_per_chunk must be >= 1");
    h->chunk = c;
    return JG_OK;
}

int jg_set_option(jg_handle* h, const char* name, int value) {
    if (!h || !name) return JG_ERR_ARG;
    EngineOpts& o = h->opts;
    if (!std::strcmp(name, "conv1_direct")) { h->conv1_direct = value != 0; return JG_OK; }
    if (!std::strcmp(name, "fuse_ln")) { h->fuse_ln = value != 0; return JG_OK; }
    if (!std::strcmp(name, "edge_dedup")) { h->edge_dedup = value != 0; return JG_OK; }
    if (!std::strcmp(name, "conv1_mfma16")) { o.conv1_mfma16 = value != 0; return JG_OK; }
    if (!std::strcmp(name, "conv1_zero_skip")) { o.conv1_zero_skip = value != 0; return JG_OK; }
    if (!std::strcmp(name, "conv2_row_skip")) { h->conv2_row_skip = value != 0; return JG_OK; }
    if (!std::strcmp(name, "ws_poison")) { h->ws_poison = value != 0; return JG_OK; }
    if (!std::strcmp(name, "jegal_fp32_ends")) { h->jegal_fp32_ends = value != 0; return JG_OK; }
    if (!std::strcmp(name, "conv_round_diffuse")) {
        if (h->gs_ready || h->jg_ready) JG_FAIL(h, JG_ERR_STATE, "set conv_round_diffuse before jg_finalize_weights");
        h->conv_round_diffuse = value != 0;
        return JG_OK;
    }
    if (!std::strcmp(name, "audit_weights")) {
        if (h->gs_ready || h->jg_ready || h->xl_ready) JG_FAIL(h, JG_ERR_STATE, "set audit_weights before jg_finalize_weights");
        h->audit_weights = value != 0;
        return JG_OK;
    }
    if (!std::strcmp(name, "audit_jegal_parts")) {
        if (value < 0 || value > 15) JG_FAIL(h, JG_ERR_ARG, "audit_jegal_parts is a mask of 4 bits");
        if (value && !h->audit_weights && h->precision != JG_PREC_FP32) JG_FAIL(h, JG_ERR_STATE, "audit_jegal_parts needs option audit_weights=1 set before jg_finalize_weights");
        h->audit_jegal_parts = value;
        return JG_OK;
    }
    if (!std::strcmp(name, "audit_stages")) {
        if (value < 0 || value > 31) JG_FAIL(h, JG_ERR_ARG, "audit_stages is a mask of 5 bits");
        if (value && !h->audit_weights && h->precision != JG_PREC_FP32) JG_FAIL(h, JG_ERR_STATE, "audit_stages needs option audit_weights=1 set before jg_finalize_weights");
        h->audit_stages = value;
        return JG_OK;
    }
    if (!std::strcmp(name, "dual_stream")) { h->dual_stream = value != 0; return JG_OK; }
    if (!std::strcmp(name, "num_cu")) {          // experiments: persistent kernels of this handle launch this many workgroups (<= the device's CUs)
        if (value < 8 || value > 1024) JG_FAIL(h, JG_ERR_ARG, "num_cu out of range");
        o.num_cu = value;
        return JG_OK;
    }
    if (!std::strcmp(name, "xlmr_lanes")) {
        if (value < 1 || value > jg_handle::MAX_LANES) JG_FAIL(h, JG_ERR_ARG, "xlmr_lanes must be 1..%d", jg_handle::MAX_LANES);
        h->xl_lanes = value;
        return JG_OK;
    }
    if (!std::strcmp(name, "xlmr_fold")) { h->xl_fold_opt = value != 0; return JG_OK; }       // takes effect at the next jg_finalize_weights(h, 4)
    if (!std::strcmp(name, "lane_priority")) {
        if (value < 0 || value > 3) JG_FAIL(h, JG_ERR_ARG, "lane_priority must be 0..3");
        if (value != h->lane_priority) {
            // the lane streams are re-created (lazily, by the next two-lane call) with the new priority: drain and drop the old ones
            DeviceGuard dg(h->device);
            for (int l = 0; l < 2; ++l)
                if (h->lane_stream[l]) {
                    HIPCHK(h, hipStreamSynchronize(h->lane_stream[l]));
                    HIPCHK(h, hipStreamDestroy(h->lane_stream[l]));
                    h->lane_stream[l] = nullptr;
                }
            h->lane_priority = value;
        }
        return JG_OK;
    }
    if (!std::strcmp(name, "dual_split")) {
        if (value < 1 || value > 7) JG_FAIL(h, JG_ERR_ARG, "dual_split must be 1..7 (eighths of the batch on the first lane)");
        h->dual_split = value;
        return JG_OK;
    }
    if (!std::strcmp(name, "qkv0_linear")) { h->qkv0_linear = value != 0; return JG_OK; }
    if (!std::strcmp(name, "attn_mfma")) { o.attn_mfma = value != 0; return JG_OK; }
    if (!std::strcmp(name, "gemm_glds")) { o.gemm_glds = value != 0; return JG_OK; }
    if (!std::strcmp(name, "gemm_tall_tile")) { o.gemm_tall_tile = value != 0; return JG_OK; }
    if (!std::strcmp(name, "gemm_small_tile")) { o.gemm_small_tile = value != 0; return JG_OK; }
    if (!std::strcmp(name, "gemm_big_tile")) { o.gemm_big_tile = value != 0; return JG_OK; }
    if (!std::strcmp(name, "gemm_tile")) { o.gemm_tile = value; return JG_OK; }
    if (!std::strcmp(name, "gemm_counted")) { o.gemm_counted = value != 0; return JG_OK; }
    if (!std::strcmp(name, "gemm_persistent")) { o.gemm_persistent = value != 0; return JG_OK; }
    if (!std::strcmp(name, "gemm_stagger")) { o.gemm_stagger = value; return JG_OK; }
    JG_FAIL(h, JG_ERR_ARG, "unknown option '%s'", name);
}

int jg_debug_conv2_rowskip(jg_handle* h, int* rows) {
    ENTER(h);
    if (!rows) JG_FAIL(h, JG_ERR_ARG, "rows is NULL");
    *rows = 0;
    if (!h->last_rowskip) return JG_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(rows, h->last_rowskip, sizeof(int), hipMemcpyDeviceToHost));
    return JG_OK;
}

int jg_debug_conv_rows(jg_handle* h, int64_t* computed, int64_t* full) {
    ENTER(h);
    if (!computed || !full) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    for (int l = 0; l < 4; ++l) computed[l] = full[l] = 0;
    if (!h->last_conv_totals) return JG_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int t[4];
    HIPCHK(h, hipMemcpy(t, h->last_conv_totals, sizeof(t), hipMemcpyDeviceToHost));
    for (int l = 0; l < 4; ++l) { computed[l] = t[l]; full[l] = h->last_conv_full[l]; }
    return JG_OK;
}

int jg_sync(jg_handle* h) {
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return JG_OK;
}

int jg_load_tensor(jg_handle* h, const char* name, const void* data, const int64_t* shape, int ndim, int dtype) {
    if (!h) return JG_ERR_ARG;
    if (!name || !data || ndim < 0 || (ndim > 0 && !shape)) JG_FAIL(h, JG_ERR_ARG, "jg_load_tensor: bad arguments");
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    const int64_t n = t.numel();
    t.v.resize((size_t)n);
    switch (dtype) {
        case JG_F32: std::memcpy(t.v.data(), data, sizeof(float) * n); break;
        case JG_F16: { const f16* p = static_cast<const f16*>(data); for (int64_t i = 0; i < n; ++i) t.v[i] = (float)p[i]; } break;
        case JG_I64: { const int64_t* p = static_cast<const int64_t*>(data); for (int64_t i = 0; i < n; ++i) t.v[i] = (float)p[i]; } break;
        default: JG_FAIL(h, JG_ERR_ARG, "jg_load_tensor(%s): unsupported dtype %d", name, dtype);
    }
    std::string key(name);
    if (key.rfind("module.", 0) == 0) key = key.substr(7);     // inference_embs.py:113-114
    h->host[key] = std::move(t);
    return JG_OK;
}

int jg_finalize_weights(jg_handle* h, int which) {
    ENTER(h);
    h->gs_qpe_valid = false;
    if (which & 1) { RET(finalize_gestsync(h)); RET(gs_build_const_chain(h)); }
    if (which & 2) RET(finalize_jegal(h));
    if (which & 4) RET(finalize_xlmr(h));
    // The fp32 host copies this finalize consumed are no longer needed (packed device weights + the w32/b32 of the
    // bias-corrected layers carry everything).  Tensors staged for a model that is finalized LATER stay staged; what no
    // finalize consumes (the unused audio/LSTM tensors of gestsync.py:23-32) stays until jg_clear_staged_tensors / jg_destroy.
    for (auto it = h->host.begin(); it != h->host.end();) it = it->second.used ? h->host.erase(it) : std::next(it);
    // Built-in calibration only for the gesture models finalized by THIS call (XLM-R has no bias-corrected layers): the bias
    // corrections of the other model -- possibly from jg_calibrate_gesture on real clips -- are left as they are.
    if (h->precision == JG_PREC_FP16_BC && (which & 3)) RET(calibrate_impl(h, nullptr, JG_U8, 0, 0, which & 3));
    // XLM-RoBERTa is NOT calibrated implicitly: its Linears run hi+lo (calibration-free) until jg_calibrate_xlmr is called
    return JG_OK;
}

int jg_clear_staged_tensors(jg_handle* h) {
    if (!h) return JG_ERR_ARG;
    h->host.clear();
    return JG_OK;
}

int jg_calibrate_gesture(jg_handle* h, const void* frames, int dtype, int B, int T) {
    ENTER(h);
    if (h->precision != JG_PREC_FP16_BC) JG_FAIL(h, JG_ERR_STATE, "calibration only applies to JG_PREC_FP16_BC");
    if (frames && (B <= 0 || T <= 0 || (dtype != JG_U8 && dtype != JG_F32))) JG_FAIL(h, JG_ERR_ARG, "bad calibration batch");
    return calibrate_impl(h, frames, dtype, B, T, 3);
}

int jg_calibrate_xlmr(jg_handle* h, const int32_t* input_ids, const int32_t* attention_mask, int B, int L) {
    ENTER(h);
    if (h->precision != JG_PREC_FP16_BC && h->precision != JG_PREC_FP16_RC) JG_FAIL(h, JG_ERR_STATE, "calibration only applies to JG_PREC_FP16_BC / JG_PREC_FP16_RC");
    if (input_ids && (B <= 0 || L <= 0)) JG_FAIL(h, JG_ERR_ARG, "bad calibration batch");
    return calibrate_xlmr(h, input_ids, attention_mask, B, L);
}

int jg_gestsync_clip(jg_handle* h, const void* frames, int dtype, int B, int T, float* out) {
    ENTER(h);
    if (!frames || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (B <= 0 || T <= 0 || (dtype != JG_U8 && dtype != JG_F32)) return gestsync_clip_impl(h, frames, dtype, B, T, out);      // reports the error
    const size_t esz = dtype == JG_U8 ? 1 : 4;
    return run_in_lanes(h, B, T, [&](int b0, int nb) -> int {
        return gestsync_clip_impl(h, reinterpret_cast<const char*>(frames) + (size_t)b0 * T * FH * FW * 3 * esz, dtype, nb, T,
                                  out + (size_t)b0 * T * 1024);
    });
}

int jg_gestsync_clip_ragged(jg_handle* h, const void* frames, int dtype, int B, int T, const int32_t* valid_frames_host, float* out) {
    ENTER(h);
    if (!frames || !out || !valid_frames_host) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (B <= 0 || T <= 0 || (dtype != JG_U8 && dtype != JG_F32)) return gestsync_clip_impl(h, frames, dtype, B, T, out);      // reports the error
    for (int b = 0; b < B; ++b)
        if (valid_frames_host[b] < 1 || valid_frames_host[b] > T) JG_FAIL(h, JG_ERR_ARG, "valid_frames[%d] = %d outside 1..T = %d", b, valid_frames_host[b], T);
    const size_t esz = dtype == JG_U8 ? 1 : 4;
    return run_in_lanes(h, B, T, [&](int b0, int nb) -> int {
        return gestsync_clip_impl(h, reinterpret_cast<const char*>(frames) + (size_t)b0 * T * FH * FW * 3 * esz, dtype, nb, T,
                                  out + (size_t)b0 * T * 1024, valid_frames_host + b0);
    });
}

int jg_debug_conv1_pool(jg_handle* h, const void* frames_u8, int B, int T, int pad, void* out_f16) {
    ENTER(h);
    if (!h->gs_ready) JG_FAIL(h, JG_ERR_STATE, "GestSync weights not finalized");
    if (!frames_u8 || !out_f16 || B <= 0 || pad < 0 || pad > 12 || T + 2 * pad < 5)      // conv1's skip-mask area is sized for pad <= 12
        JG_FAIL(h, JG_ERR_ARG, "bad arguments (need 0 <= pad <= 12 and T + 2*pad >= 5)");
    h->ws.reset();
    const int P = T + 2 * pad - 4;
    const long NF = (long)B * P;
    if (h->conv1_direct && !h->bf16) {
        f16* edge;
        unsigned* zscr;
        RET(wsalloc(h, conv1_edge_elems(NF), &edge));
        RET(wsalloc(h, conv1_zmask_elems(B, T), &zscr));
        return conv1_from_frames(h, static_cast<const uint8_t*>(frames_u8), B, T, pad, static_cast<f16*>(out_f16), edge, zscr, true);
    }
    f16 *o1, *S;
    RET(wsalloc(h, (size_t)NF * 88 * 158 * 64, &o1));
    RET(wsalloc(h, (size_t)NF * FH * FW * 16, &S));
    const long sw = 3, sh = (long)FW * 3, st = (long)FH * FW * 3, sb = (long)T * st;
    RET(timed(h, JG_ST_STACK, [&] { return LAUNCH(h, launch_stack_frames, frames_u8, 1, sb, st, sh, sw, 1, B, T, pad, FH, FW, S, h->stream); }));
    const ConvGeom g1 = geom(FH, FW, 16, 7, 7, 3, 3, 0, 0);
    Epi e; e.relu = 1; e.scale = h->c1_scale255; e.out16 = o1;
    RET(gemm(h, JG_ST_CONV1, S, 0, (int)(NF * 88 * 158), h->c1, e, &g1));
    return timed(h, JG_ST_POOL, [&] { return LAUNCH(h, launch_maxpool3x3s2, o1, static_cast<f16*>(out_f16), (int)NF, 88, 158, 64, h->stream, nullptr, 0, nullptr); });
}

// Tuning aid: time `iters` launches of the production GEMM on garbage operands of a given shape.
// mode bit 0: hi+lo weights, bit 1: fp32 residual in/out (else fp16 out), bit 2: ReLU.  Returns ms per launch in *ms.
int jg_debug_gemm(jg_handle* h, int M, int N, int K, int mode, int iters, double* ms) {
    return jg_debug_gemm_ex(h, nullptr, nullptr, M, N, K, mode, iters, ms);
}

// a16 / w16: caller-supplied fp16 operands ([M][K] and [N][K], e.g. random data: constant operands let the chip hold a higher
// clock than real data does, MI355X_MICROARCH.md "DVFS give-back"); NULL: constant fill
int jg_debug_gemm_ex(jg_handle* h, const void* a16, const void* w16, int M, int N, int K, int mode, int iters, double* ms) {
    if (!h || !ms || M <= 0 || N <= 0 || K <= 0 || iters <= 0) return JG_ERR_ARG;
    ENTER(h);
    h->ws.reset();
    f16 *A, *Wh, *Wl, *o16;
    float *bias, *x32;
    RET(wsalloc(h, (size_t)M * K, &A));
    RET(wsalloc(h, (size_t)N * K, &Wh));
    RET(wsalloc(h, (size_t)N * K, &Wl));
    RET(wsalloc(h, pad128(M) * N, &o16));
    RET(wsalloc(h, pad128(M) * N, &x32));
    RET(wsalloc(h, (size_t)N, &bias));
    if (a16) HIPCHK(h, hipMemcpyAsync(A, a16, (size_t)M * K * 2, hipMemcpyDeviceToDevice, h->stream));
    else HIPCHK(h, hipMemsetAsync(A, 0x3c, (size_t)M * K * 2, h->stream));
    if (w16) HIPCHK(h, hipMemcpyAsync(Wh, w16, (size_t)N * K * 2, hipMemcpyDeviceToDevice, h->stream));
    else HIPCHK(h, hipMemsetAsync(Wh, 0x2c, (size_t)N * K * 2, h->stream));
    HIPCHK(h, hipMemsetAsync(Wl, 0x1c, (size_t)N * K * 2, h->stream));
    HIPCHK(h, hipMemsetAsync(bias, 0, (size_t)N * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(x32, 0, (size_t)M * N * 4, h->stream));
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = K; a.Wh = Wh; a.Wl = (mode & 1) ? Wl : nullptr; a.ldw = K;
    a.M = M; a.N = N; a.K = K; a.bias = bias; a.ldc = N; a.relu = (mode >> 2) & 1;
    if (mode & 2) { a.res = x32; a.ldr = N; a.out32 = x32; } else { a.out16 = o16; }
    if (mode & 8) {      // residual + LayerNorm fused (N = 512): gamma/beta = the zero bias vector, timing only
        a.res = nullptr; a.out32 = nullptr;
        a.res16 = o16; a.out16 = o16;
        a.ln_w = bias; a.ln_b = bias; a.ln_flavour = LN_STD;
    }
    if (mode & 48) {     // implicit LayerNorm, timing only: 16 = consumer (ln_mode 1), 32 = producer (ln_mode 2); statistics / planes = the scratch buffers
        float* stats;
        RET(wsalloc(h, (size_t)pad128(M) * 2, &stats));
        HIPCHK(h, hipMemsetAsync(stats, 0, (size_t)M * 2 * 4, h->stream));
        a.res = nullptr; a.out32 = nullptr; a.scale = bias; a.ln_stats = stats;
        if (mode & 16) { a.ln_mode = 1; a.out16 = o16; }
        else {
            f16* lo;
            float* part;
            RET(wsalloc(h, pad128(M) * N, &lo));
            RET(wsalloc(h, (size_t)pad128(M) * (N / 64) * 2, &part));
            a.ln_mode = 2; a.relu = 0; a.xres_hi = o16; a.xres_lo = lo; a.out16 = o16; a.out_lo = lo; a.stat_out = part;
        }
    }
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    HIPCHK(h, LAUNCH(h, launch_gemm, a, false, h->opts, h->stream));
    HIPCHK(h, hipEventRecord(e0, h->stream));
    for (int i = 0; i < iters; ++i) HIPCHK(h, LAUNCH(h, launch_gemm, a, false, h->opts, h->stream));
    HIPCHK(h, hipEventRecord(e1, h->stream));
    HIPCHK(h, hipEventSynchronize(e1));
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms = t / iters;
    return JG_OK;
}

// ---- kernel check points: one launch of a production launcher on the caller's operands, with the handle's options (which pick
// the instance exactly as in production) and the handle's build (fp16 or bf16).  The launcher's own shape rules decide what is
// valid: its hipErrorInvalidValue comes back as JG_ERR_ARG, and nothing was launched then.
// (They live here rather than in a translation unit of their own because they need the handle's internals -- options, stream, build
// switch, error slot -- and the LAUNCH dispatch between the fp16 and bf16 builds, all private to this file.)
namespace {
// options of the handle + the name slot the launchers write
void check_opts(jg_handle* h, EngineOpts& o) {
    o = h->opts;
    o.kname = h->kname;
}
int check_result(jg_handle* h, hipError_t e, const char* what) {
    if (e == hipErrorInvalidValue) JG_FAIL(h, JG_ERR_ARG, "%s: the launcher rejects this shape / argument set", what);
    if (e != hipSuccess) JG_FAIL(h, JG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return JG_OK;
}
}  // namespace

int jg_debug_gemm_check(jg_handle* h, const jg_gemm_check* c) {
    ENTER(h);
    h->kname[0] = 0;
    if (!c || !c->A || !c->Wh || c->M <= 0 || c->N <= 0 || c->K <= 0 || c->lda < c->K || c->ldw < c->K || (!c->out32 && !c->out16) ||
        ((c->out32 || (c->out16 && !c->ln_w)) && c->ldc < c->N) || (c->res && (c->ldr < c->N || c->res_mod < 0)) ||
        (c->bias_clip && (c->rpc <= 0 || c->nclips <= 0)) || c->relu < 0 || c->relu > 2 || c->ln_mode < 0 || c->ln_mode > 2)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_gemm_check: bad arguments");
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.A = static_cast<const f16*>(c->A); a.lda = c->lda;
    a.Wh = static_cast<const f16*>(c->Wh); a.Wl = static_cast<const f16*>(c->Wl); a.ldw = c->ldw;
    a.M = c->M; a.N = c->N; a.K = c->K;
    a.scale = c->scale; a.bias = c->bias;
    a.bias_clip = c->bias_clip; a.rpc = c->rpc; a.nclips = c->nclips;
    a.res = c->res; a.ldr = c->ldr; a.res_mod = c->res_mod; a.relu = c->relu;
    a.out32 = c->out32; a.out16 = static_cast<f16*>(c->out16); a.ldc = c->ldc;
    a.ln_w = c->ln_w; a.ln_b = c->ln_b; a.ln_flavour = LN_STD;
    a.res16 = static_cast<const f16*>(c->res16);
    a.ln_mode = c->ln_mode; a.ln_stats = c->ln_stats;
    a.xres_hi = static_cast<const f16*>(c->xres_hi); a.xres_lo = static_cast<const f16*>(c->xres_lo);
    a.out_lo = static_cast<f16*>(c->out_lo); a.stat_out = c->stat_out;
    EngineOpts o;
    check_opts(h, o);
    return check_result(h, LAUNCH(h, launch_gemm, a, false, o, h->stream), "launch_gemm");
}

int jg_debug_gemm32(jg_handle* h, const float* A, int64_t lda, const float* W, int64_t ldw, int M, int N, int K, const float* scale,
                    const float* bias, const float* res, int64_t ldr, int res_mod, int act, float* out, int64_t ldc) {
    ENTER(h);
    h->kname[0] = 0;
    if (!A || !W || !out || M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || (res && (ldr < N || res_mod < 0)) || act < 0 || act > 2)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_gemm32: bad arguments");
    Gemm32Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
    a.scale = scale; a.bias = bias; a.res = res; a.ldr = ldr; a.res_mod = res_mod; a.out = out; a.ldc = ldc; a.act = act;
    return check_result(h, launch_gemm32(a, h->stream, h->kname), "launch_gemm32");
}

int jg_debug_gemm_x3(jg_handle* h, const float* A, int64_t lda, const void* Wh, const void* Wl, int64_t ldw, int M, int N, int K,
                     const float* bias, const float* res, int64_t ldr, int res_mod, int relu, float* out, int64_t ldc) {
    ENTER(h);
    h->kname[0] = 0;
    if (!A || !Wh || !Wl || !out || M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || (res && (ldr < N || res_mod < 0)) ||
        relu < 0 || relu > 1)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_gemm_x3: bad arguments");
    GemmX3Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.Wh = static_cast<const f16*>(Wh); a.Wl = static_cast<const f16*>(Wl); a.ldw = ldw; a.M = M; a.N = N; a.K = K;
    a.bias = bias; a.res = res; a.ldr = ldr; a.res_mod = res_mod; a.out = out; a.ldc = ldc; a.relu = relu;
    return check_result(h, launch_gemm_x3(a, h->stream, h->kname), "launch_gemm_x3");
}

int jg_debug_attention(jg_handle* h, const void* qkv, const float* keymask, int B, int S, int H, int dk, void* out) {
    ENTER(h);
    h->kname[0] = 0;
    if (!qkv || !out || B <= 0 || S <= 0 || H <= 0 || (dk != 64 && dk != 96)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_attention: bad arguments");
    EngineOpts o;
    check_opts(h, o);
    return check_result(h, LAUNCH(h, launch_attention, static_cast<const f16*>(qkv), keymask, B, S, H, dk, static_cast<f16*>(out), o, h->stream),
                        "launch_attention");
}

int jg_debug_attention_gather(jg_handle* h, const void* qkv_pos, const void* pe_qkv, int Twin, int P, int shift, int B, int S, int H, void* out) {
    ENTER(h);
    h->kname[0] = 0;
    if (!qkv_pos || !pe_qkv || !out || B <= 0 || S <= 0 || H <= 0 || Twin <= 0 || P <= 0 || B % Twin)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_attention_gather: bad arguments (B must be a multiple of Twin)");
    if (h->bf16) JG_FAIL(h, JG_ERR_STATE, "jg_debug_attention_gather: the gather form is an fp16-build kernel (the clip path's layer 0)");
    const AttnGather g{static_cast<const f16*>(pe_qkv), Twin, P, shift};
    return check_result(h, launch_attention_gather(static_cast<const f16*>(qkv_pos), g, B, S, H, static_cast<f16*>(out), h->stream, h->kname),
                        "launch_attention_gather");
}

int jg_debug_attention32(jg_handle* h, const float* qkv, const float* keymask, int B, int S, int H, int dk, float* out) {
    ENTER(h);
    h->kname[0] = 0;
    if (!qkv || !out || B <= 0 || S <= 0 || H <= 0) JG_FAIL(h, JG_ERR_ARG, "jg_debug_attention32: bad arguments");
    return check_result(h, launch_attention32(qkv, keymask, B, S, H, dk, out, h->stream, h->kname), "launch_attention32");
}

int jg_debug_last_kernel(jg_handle* h, char* buf, int len) {
    if (!h || !buf || len <= 0) return JG_ERR_ARG;
    snprintf(buf, (size_t)len, "%s", h->kname);
    return JG_OK;
}

int jg_gestsync_windows(jg_handle* h, const float* x, int N, float* out, float* out_conv) {
    ENTER(h);
    if (!x || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return gestsync_windows_impl(h, x, N, out, out_conv);
}

int jg_jegal_gestures(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out) {
    ENTER(h);
    if (!feats || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    h->ws.reset();
    return jegal_gestures_impl(h, feats, mask, B, T, align, out);
}

int jg_audio_len(int Tm) { return audio_len(Tm); }

int jg_jegal_audio(jg_handle* h, const float* mel, int B, int Tm, float* out) {
    ENTER(h);
    if (!mel || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    h->ws.reset();
    return jegal_audio_impl(h, mel, B, Tm, nullptr, out);
}

int jg_jegal_audio_ragged(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_tm_host, float* out) {
    ENTER(h);
    if (!mel || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    h->ws.reset();
    return jegal_audio_impl(h, mel, B, Tm, valid_tm_host, out);
}

int jg_mask_resize(jg_handle* h, const uint8_t* src, int T, int H, int W, const int32_t* mask_y, uint8_t* dst) {
    ENTER(h);
    if (!src || !mask_y || !dst || T <= 0 || H <= 0 || W <= 0) JG_FAIL(h, JG_ERR_ARG, "bad mask_resize arguments");
    return timed(h, JG_ST_MISC, [&] { return launch_mask_resize(src, T, H, W, mask_y, dst, h->stream); });
}

int jg_unpack_masked(jg_handle* h, const uint8_t* packed, int64_t packed_bytes, const int32_t* row0, const int64_t* offsets, int n_frames, uint8_t* dst) {
    ENTER(h);
    if (!packed || !row0 || !offsets || !dst || n_frames <= 0 || packed_bytes < 0) JG_FAIL(h, JG_ERR_ARG, "bad unpack_masked arguments");
    static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
    return timed(h, JG_ST_MISC, [&] { return launch_unpack_masked(packed, row0, reinterpret_cast<const long long*>(offsets), n_frames, dst, h->stream,
                                                                   (long long)packed_bytes); });
}

int jg_mask_resize_packed(jg_handle* h, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, int T, int H, int W,
                          const int32_t* mask_y, uint8_t* dst) {
    ENTER(h);
    if (!packed || !offsets || !mask_y || !dst || T <= 0 || H <= 0 || W <= 0 || packed_bytes < 0) JG_FAIL(h, JG_ERR_ARG, "bad mask_resize_packed arguments");
    return timed(h, JG_ST_MISC, [&] { return launch_mask_resize(packed, T, H, W, mask_y, dst, h->stream, reinterpret_cast<const long long*>(offsets),
                                                                 (long long)packed_bytes); });
}

int jg_logmel(jg_handle* h, const float* wav, int B, int n_samples, const float* mel_basis, float* out) {
    ENTER(h);
    if (!wav || !mel_basis || !out || B <= 0 || n_samples < 160) JG_FAIL(h, JG_ERR_ARG, "bad logmel arguments");
    return timed(h, JG_ST_MISC, [&] { return launch_logmel(wav, B, n_samples, mel_basis, out, h->stream); });
}

int jg_jegal_text(jg_handle* h, const float* states, const float* mask, int B, int L, float* out) {
    ENTER(h);
    if (!states || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    h->ws.reset();
    return jegal_text_impl(h, states, mask, B, L, out);
}

int jg_xlmr_encode(jg_handle* h, const int32_t* input_ids, const int32_t* attention_mask, int B, int L, float* out) {
    ENTER(h);
    if (!input_ids || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    // Option xlmr_lanes > 1 (experiment, see jg_handle::xl_lanes): sequences are independent, and at B * L = 16 384 tokens the N = 768
    // GEMMs are single rounds of 192 tiles on 256 CUs and qkv is 2.25 rounds -- two half batches on two streams let one lane's
    // kernels start on the CUs the other's last round leaves idle.
    auto run_part = [&](int b0, int nb) -> int {
        h->ws.reset();
        if (h->ws_poison)                       // test aid: whatever a kernel reads without having written it is NaN
            for (auto& c : h->ws.chunks) HIPCHK(h, launch_poison(c.p, c.cap, h->stream));
        return xlmr_encode_impl(h, input_ids + (size_t)b0 * L, attention_mask ? attention_mask + (size_t)b0 * L : nullptr, nb, L,
                                out + (size_t)b0 * L * 768);
    };
    return run_in_lanes(h, B, L, run_part, h->xl_lanes);      // equal parts: every token costs the same (two lanes: 3:5 587, 4:4 606 TFLOP/s)
}

int jg_word_pool(jg_handle* h, const float* seq, int D, const int32_t* seg, int n, float* dst, int dst_ld, int dst_col) {
    ENTER(h);
    if (!seq || !seg || !dst) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_segment_mean, seq, D, seg, n, nullptr, dst, dst_ld, dst_col, h->stream); });
}

int jg_fuse_content(jg_handle* h, const float* fused, int rows, float* out) {
    ENTER(h);
    if (!fused || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    h->ws.reset();
    return fuse_content_impl(h, fused, rows, out);
}

int jg_l2norm(jg_handle* h, const float* in, float* out, int rows, int D) {
    ENTER(h);
    if (!in || !out || D % 4) JG_FAIL(h, JG_ERR_ARG, "bad l2norm arguments");
    return timed(h, JG_ST_MISC, [&] { return launch_l2norm(in, out, rows, D, h->stream); });
}

int jg_extract_gesture(jg_handle* h, const void* frames, int dtype, int B, int T, float* out_emb) {
    ENTER(h);
    if (!frames || !out_emb) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (B <= 0 || T <= 0) JG_FAIL(h, JG_ERR_ARG, "B and T must be positive");
    if (T > 500) JG_FAIL(h, JG_ERR_ARG, "T must be <= 500");
    if (dtype != JG_U8 && dtype != JG_F32) JG_FAIL(h, JG_ERR_ARG, "frames dtype must be JG_U8 or JG_F32");
    if (!h->gs_ready || !h->jg_ready) JG_FAIL(h, JG_ERR_STATE, "GestSync and JEGAL weights must both be finalized");
    // the (B,T,1024) GestSync features stay on the device in a buffer owned by the handle
    const size_t need_b = (size_t)B * T * 1024 * sizeof(float);
    if (need_b > h->feats_cap) {
        if (h->feats) { HIPCHK(h, hipDeviceSynchronize()); HIPCHK(h, hipFree(h->feats)); h->feats = nullptr; h->feats_cap = 0; }
        HIPCHK(h, hipMalloc(&h->feats, need_b));
        h->feats_cap = need_b;
    }
    auto run_part = [&](int b0, int nb) -> int {
        const size_t esz = dtype == JG_U8 ? 1 : 4;
        const char* fr = reinterpret_cast<const char*>(frames) + (size_t)b0 * T * FH * FW * 3 * esz;
        float* feats = h->feats + (size_t)b0 * T * 1024;
        float* emb = out_emb + (size_t)b0 * T * 512;
        RET(gestsync_clip_impl(h, fr, dtype, nb, T, feats));
        h->ws.reset();
        RET(jegal_gestures_impl(h, feats, nullptr, nb, T, 1, emb));
        return timed(h, JG_ST_MISC, [&] { return launch_l2norm(emb, emb, nb * T, 512, h->stream); });
    };
    return run_in_lanes(h, B, T, run_part);
}

int jg_pool_mean(jg_handle* h, const float* x, const int32_t* off, int n, int D, float* out) {
    ENTER(h);
    if (!x || !off || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return timed(h, JG_ST_MISC, [&] { return launch_ragged_mean(x, off, n, D, out, h->stream); });
}

int jg_sim_rank(jg_handle* h, const float* e1, const float* e2, int n_local, int n_total, int row_offset, int D,
                int32_t* rank, int32_t* ties) {
    ENTER(h);
    if (!e1 || !e2 || !rank || !ties) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (D % 64 || row_offset < 0 || row_offset + n_local > n_total) JG_FAIL(h, JG_ERR_ARG, "bad sim_rank geometry");
    return timed(h, JG_ST_MISC, [&] { return launch_sim_rank(e1, e2, n_local, n_total, row_offset, D, rank, ties, h->stream); });
}

int jg_spot(jg_handle* h, const float* g, const float* c, const int32_t* goff, const int32_t* coff, const int32_t* target,
            int n, int D, float temp, int32_t* pred, float* score) {
    ENTER(h);
    if (!g || !c || !goff || !coff || !target || !pred || !score) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return timed(h, JG_ST_MISC, [&] { return launch_spot(g, c, goff, coff, target, n, D, temp, pred, score, h->stream); });
}

int jg_asd(jg_handle* h, const float* q, const float* cand, const int32_t* coff, int n, int D, float temp, int32_t* pred) {
    ENTER(h);
    if (!q || !cand || !coff || !pred) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return timed(h, JG_ST_MISC, [&] { return launch_asd(q, cand, coff, n, D, temp, pred, h->stream); });
}

// ---- multi-GPU exchange on RCCL: one communicator per handle = per rank = per GPU
int jg_comm_get_unique_id(char* id128_host) {
    if (!id128_host) return JG_ERR_ARG;
    if (!rccl().ok) return JG_ERR_STATE;
    NcclId id;
    if (rccl().GetUniqueId(&id) != 0) return JG_ERR_HIP;
    std::memcpy(id128_host, id.internal, sizeof(id.internal));
    return JG_OK;
}

int jg_comm_init(jg_handle* h, const char* id128_host, int rank, int world) {
    ENTER(h);
    if (!id128_host || world < 1 || rank < 0 || rank >= world) JG_FAIL(h, JG_ERR_ARG, "bad communicator arguments");
    if (!rccl().ok) JG_FAIL(h, JG_ERR_STATE, "librccl.so could not be loaded (%s)", dlerror() ? dlerror() : "symbols missing");
    if (h->comm) { (void)rccl().CommDestroy(h->comm); h->comm = nullptr; }
    NcclId id;
    std::memcpy(id.internal, id128_host, sizeof(id.internal));
    typedef int (*init_t)(void**, int, NcclId, int);          // ncclCommInitRank(ncclComm_t*, int nranks, ncclUniqueId commId, int rank)
    const int rc = reinterpret_cast<init_t>(rccl().CommInitRank)(&h->comm, world, id, rank);
    if (rc != 0) { h->comm = nullptr; JG_FAIL(h, JG_ERR_HIP, "ncclCommInitRank failed: %s", rccl().GetErrorString ? rccl().GetErrorString(rc) : "?"); }
    h->comm_rank = rank; h->comm_world = world;
    return JG_OK;
}

int jg_comm_destroy(jg_handle* h) {
    ENTER(h);
    if (h->comm && rccl().ok) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        (void)rccl().CommDestroy(h->comm);
    }
    h->comm = nullptr; h->comm_rank = 0; h->comm_world = 1;
    return JG_OK;
}

int jg_allgather(jg_handle* h, const void* send, void* recv, int64_t bytes_per_rank) {
    ENTER(h);
    if (!send || !recv || bytes_per_rank < 0) JG_FAIL(h, JG_ERR_ARG, "bad allgather arguments");
    if (!h->comm) JG_FAIL(h, JG_ERR_STATE, "jg_allgather before jg_comm_init");
    const int rc = rccl().AllGather(send, recv, (size_t)bytes_per_rank, /* ncclInt8 */ 0, h->comm, h->stream);
    if (rc != 0) JG_FAIL(h, JG_ERR_HIP, "ncclAllGather failed: %s", rccl().GetErrorString ? rccl().GetErrorString(rc) : "?");
    return JG_OK;
}

int jg_allreduce_sum_i64(jg_handle* h, int64_t* buf, int n) {
    ENTER(h);
    if (!buf || n < 0) JG_FAIL(h, JG_ERR_ARG, "bad allreduce arguments");
    if (!h->comm) JG_FAIL(h, JG_ERR_STATE, "jg_allreduce_sum_i64 before jg_comm_init");
    const int rc = rccl().AllReduce(buf, buf, (size_t)n, /* ncclInt64 */ 4, /* ncclSum */ 0, h->comm, h->stream);
    if (rc != 0) JG_FAIL(h, JG_ERR_HIP, "ncclAllReduce failed: %s", rccl().GetErrorString ? rccl().GetErrorString(rc) : "?");
    return JG_OK;
}

int jg_profile_enable(jg_handle* h, int on) {
    if (!h) return JG_ERR_ARG;
    if (on < 0 || on - 2 >= JG_ST_COUNT) JG_FAIL(h, JG_ERR_ARG, "bad stage");      // validated before anything changes
    h->prof = on != 0;
    h->prof_only = on >= 2 ? on - 2 : -1;
    return JG_OK;
}

static int prof_collect(jg_handle* h) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (auto& r : h->recs) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, r.e0, r.e1));
        h->prof_ms[r.stage] += ms;
        h->prof_n[r.stage] += 1;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    h->recs.clear();
    return JG_OK;
}

int jg_profile_get(jg_handle* h, int stage, double* ms, int64_t* launches) {
    ENTER(h);
    if (stage < 0 || stage >= JG_ST_COUNT) JG_FAIL(h, JG_ERR_ARG, "bad stage");
    RET(prof_collect(h));
    if (ms) *ms = h->prof_ms[stage];
    if (launches) *launches = h->prof_n[stage];
    return JG_OK;
}

int jg_profile_reset(jg_handle* h) {
    ENTER(h);
    RET(prof_collect(h));
    for (int i = 0; i < JG_ST_COUNT; ++i) { h->prof_ms[i] = 0; h->prof_n[i] = 0; }
    return JG_OK;
}

int64_t jg_workspace_bytes(jg_handle* h) {
    if (!h) return 0;
    size_t t = h->ws.total();
    for (int l = 0; l < jg_handle::MAX_LANES; ++l) t += h->lane_ws[l].total();
    for (auto& kv : h->ws_parked) t += kv.second.total();
    return (int64_t)t;
}

}  // extern "C"
