// libjegal_hip: the C ABI of include/jegal_hip.h -- handle lifecycle, setters, the compute entry points (the models live in
// gestsync.hip, jegal.hip and xlmr.hip), two-lane scheduling, the RCCL binding and profiling.  Host code only (no kernels here).
#include "engine.h"

#include <dlfcn.h>

using namespace engine;

namespace {

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

// jg_gestsync_clip (valid == nullptr) and jg_gestsync_clip_ragged
int gestsync_clip_entry(jg_handle* h, const void* frames, int dtype, int B, int T, const int32_t* valid, float* out) {
    ENTER(h);
    if (!frames || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (B <= 0 || T <= 0 || (dtype != JG_U8 && dtype != JG_F32)) return gestsync_clip_impl(h, frames, dtype, B, T, out);      // reports the error
    for (int b = 0; valid && b < B; ++b)
        if (valid[b] < 1 || valid[b] > T) JG_FAIL(h, JG_ERR_ARG, "valid_frames[%d] = %d outside 1..T = %d", b, valid[b], T);
    const size_t esz = dtype == JG_U8 ? 1 : 4;
    return run_in_lanes(h, B, T, [&](int b0, int nb) -> int {
        return gestsync_clip_impl(h, reinterpret_cast<const char*>(frames) + (size_t)b0 * T * FH * FW * 3 * esz, dtype, nb, T,
                                  out + (size_t)b0 * T * 1024, valid ? valid + b0 : nullptr);
    });
}

}  // namespace

int engine::upload_i32_async(jg_handle* h, const int32_t* src, size_t n, int32_t* dst) {
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

// what a metric entry ends in: one launch on the handle's stream, timed as the MISC stage -- launcher(args..., h->stream)
template <class F, class... A>
static int misc_launch(jg_handle* h, F launcher, A... args) { return timed(h, JG_ST_MISC, [&] { return launcher(args..., h->stream); }); }

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
        for (Model* m : {&h->gs.m, &h->gsa.m, &h->jg.m, &h->xl.m})
            for (void* p : m->allocs) (void)hipFree(p);
        if (h->feats) (void)hipFree(h->feats);
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

// The workspace arena is stream-ordered (every entry point begins a pass at its start: begin_pass), so it belongs to ONE stream: a handle that is
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
        // than the stream (hipFree would wait for the device anyway).
        while (h->ws_parked.size() > 6) {
            auto lru = h->ws_parked.begin();
            for (auto it = h->ws_parked.begin(); it != h->ws_parked.end(); ++it)
                if (it->second.tick < lru->second.tick) lru = it;
            DeviceGuard dg(h->device);
            (void)hipDeviceSynchronize();
            lru->second.release();
            h->ws_parked.erase(lru);
        }
        h->stream = ns;
        h->conv_report.clear();                          // it described a pass of the arena that was just parked (or released)
    }
    return JG_OK;
}

int jg_set_precision(jg_handle* h, int mode) {
    if (!h) return JG_ERR_ARG;
    if (mode < JG_PREC_FP16 || mode > JG_PREC_FP32) JG_FAIL(h, JG_ERR_ARG, "unknown precision mode %d", mode);
    if ((h->gs.m.ready || h->gsa.m.ready || h->jg.m.ready || h->xl.m.ready) && mode != h->precision) JG_FAIL(h, JG_ERR_STATE, "set the precision before jg_finalize_weights");
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
    if (!std::strncmp(name, "lane_walk", 9) && (value < 1 || value > LANE_WALK_MAX)) JG_FAIL(h, JG_ERR_ARG, "%s must be 1..%d", name, LANE_WALK_MAX);
    if (engine_opts_set(o, name, value)) return JG_OK;      // the launchers' own switches (gemm_*, lane_walk*, attn_mfma, conv1_mfma16, conv1_zero_skip)
    if (!std::strcmp(name, "conv1_direct")) { h->conv1_direct = value != 0; return JG_OK; }
    if (!std::strcmp(name, "fuse_ln")) { h->fuse_ln = value != 0; return JG_OK; }
    if (!std::strcmp(name, "edge_dedup")) { h->edge_dedup = value != 0; return JG_OK; }
    if (!std::strcmp(name, "conv2_row_skip")) { h->conv2_row_skip = value != 0; return JG_OK; }
    if (!std::strcmp(name, "ws_poison")) { h->ws_poison = value != 0; return JG_OK; }
    if (!std::strcmp(name, "jegal_fp32_ends")) { h->jegal_fp32_ends = value != 0; return JG_OK; }
    if (!std::strcmp(name, "conv_round_diffuse")) {
        if (h->gs.m.ready || h->gsa.m.ready || h->jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "set conv_round_diffuse before jg_finalize_weights");
        h->conv_round_diffuse = value != 0;
        return JG_OK;
    }
    if (!std::strcmp(name, "audit_weights")) {
        if (h->gs.m.ready || h->gsa.m.ready || h->jg.m.ready || h->xl.m.ready) JG_FAIL(h, JG_ERR_STATE, "set audit_weights before jg_finalize_weights");
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
    if (!std::strcmp(name, "debug_lanes")) { h->debug_lanes = value != 0; return JG_OK; }
    if (!std::strcmp(name, "num_cu")) {          // experiments: persistent kernels of this handle launch this many workgroups (<= the device's CUs)
        if (value < 1 || value > 1024) JG_FAIL(h, JG_ERR_ARG, "num_cu out of range");      // (1, 2: many rounds per workgroup on a handful of tiles, tests/test_gpu_conv_fp64.py)
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
    JG_FAIL(h, JG_ERR_ARG, "unknown option '%s'", name);
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
    h->gs.qpe_valid = false;
    if (which & 1) RET(finalize_gestsync(h));
    if (which & 2) RET(finalize_jegal(h));
    if (which & 4) RET(finalize_xlmr(h));
    if (which & 8) RET(finalize_gestsync_audio(h));
    // The fp32 host copies this finalize consumed are no longer needed (packed device weights + the w32 / b32 of the
    // bias-corrected layers' calibration records carry everything).  Tensors staged for a model that is finalized LATER stay staged; what no
    // finalize consumes (the LSTM / logits_scale / fc tensors of gestsync.py:23-32, which no forward uses) stays until jg_clear_staged_tensors / jg_destroy.
    for (auto it = h->host.begin(); it != h->host.end();) it = it->second.used ? h->host.erase(it) : std::next(it);
    // Built-in calibration only for the gesture models finalized by THIS call (XLM-R has no bias-corrected layers): the bias
    // corrections of the other model -- possibly from jg_calibrate_gesture on real clips -- are left as they are.
    if (h->precision == JG_PREC_FP16_BC && (which & 3)) RET(calibrate_gesture(h, nullptr, JG_U8, 0, 0, which & 3));
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
    return calibrate_gesture(h, frames, dtype, B, T, 3);
}

int jg_calibrate_xlmr(jg_handle* h, const int32_t* input_ids, const int32_t* attention_mask, int B, int L) {
    ENTER(h);
    if (h->precision != JG_PREC_FP16_BC && h->precision != JG_PREC_FP16_RC) JG_FAIL(h, JG_ERR_STATE, "calibration only applies to JG_PREC_FP16_BC / JG_PREC_FP16_RC");
    if (input_ids && (B <= 0 || L <= 0)) JG_FAIL(h, JG_ERR_ARG, "bad calibration batch");
    return calibrate_xlmr(h, input_ids, attention_mask, B, L);
}

int jg_gestsync_clip(jg_handle* h, const void* frames, int dtype, int B, int T, float* out) { return gestsync_clip_entry(h, frames, dtype, B, T, nullptr, out); }

int jg_gestsync_clip_ragged(jg_handle* h, const void* frames, int dtype, int B, int T, const int32_t* valid_frames_host, float* out) {
    if (h && !valid_frames_host) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return gestsync_clip_entry(h, frames, dtype, B, T, valid_frames_host, out);
}

int jg_gestsync_windows(jg_handle* h, const float* x, int N, float* out, float* out_conv) {
    ENTER(h);
    if (!x || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return gestsync_windows_impl(h, x, N, out, out_conv);
}

int jg_gestsync_audio_windows(jg_handle* h, const float* x, int N, float* out) {
    ENTER(h);
    if (!x || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return gestsync_audio_impl(h, x, 0, N, 0, 1, nullptr, out);
}

int jg_gestsync_audio_clip(jg_handle* h, const float* mel, int B, int Tm, int T, const int32_t* valid_tm_host, float* out) {
    ENTER(h);
    if (!mel || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return gestsync_audio_impl(h, mel, 1, B, Tm, T, valid_tm_host, out);
}

int jg_jegal_gestures(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out) {
    ENTER(h);
    if (!feats || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    RET(begin_pass(h));
    return jegal_gestures_impl(h, feats, mask, B, T, align, out);
}

int jg_track_windows(const int32_t* t_offsets_host, int n_tracks, int win, int ctx, int32_t* table_host, int cap, int* n_windows, int* span_max) {
    return plan_track_windows(t_offsets_host, n_tracks, win, ctx, table_host, cap, n_windows, span_max);
}

int jg_jegal_gesture_tracks(jg_handle* h, const float* feats, const int32_t* t_offsets_host, int n_tracks, int win, int ctx, int align, int normalize,
                            float* out) {
    ENTER(h);
    int nw = 0, span_max = 0;
    if (plan_track_windows(t_offsets_host, n_tracks, win, ctx, nullptr, 0, &nw, &span_max) != JG_OK)
        JG_FAIL(h, JG_ERR_ARG, "bad tracks: need n_tracks >= 0, non-decreasing offsets >= 0, win >= 1, ctx >= 0, win + 2 ctx <= %d", TRACK_SPAN_MAX);
    if (n_tracks > 0 && t_offsets_host[0] != 0) JG_FAIL(h, JG_ERR_ARG, "t_offsets[0] must be 0: feats and out hold the tracks' rows alone");
    const int rows = n_tracks > 0 ? t_offsets_host[n_tracks] : 0;
    if (rows == 0) return JG_OK;
    if (!feats || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if ((long)nw * span_max > JG_TRACKS_MAX_WINDOW_ROWS)
        JG_FAIL(h, JG_ERR_ARG, "%d windows of %d rows: more than %d window rows in one call (split at track boundaries)", nw, span_max, JG_TRACKS_MAX_WINDOW_ROWS);
    if (!h->jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    std::vector<int32_t> table((size_t)nw * 4);
    if (plan_track_windows(t_offsets_host, n_tracks, win, ctx, table.data(), nw, &nw, &span_max) != JG_OK) JG_FAIL(h, JG_ERR_ARG, "window table");
    RET(begin_pass(h));
    RET(jegal_gesture_tracks_impl(h, feats, table.data(), nw, span_max, rows, align, out));
    if (!normalize) return JG_OK;
    return timed(h, JG_ST_MISC, [&] { return launch_l2norm(out, out, rows, 512, h->stream); });
}

int jg_audio_len(int Tm) {
    const int h1 = (Tm + 2 - 3) / 2 + 1;
    return (h1 + 2 - 3) / 2 + 1;
}

int jg_jegal_audio(jg_handle* h, const float* mel, int B, int Tm, float* out) { return jg_jegal_audio_ragged(h, mel, B, Tm, nullptr, out); }

int jg_jegal_audio_ragged(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_tm_host, float* out) {
    ENTER(h);
    if (!mel || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    RET(begin_pass(h));
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
    if (!wav || !mel_basis || !out || B <= 0) JG_FAIL(h, JG_ERR_ARG, "bad logmel arguments");
    if (n_samples < 257) JG_FAIL(h, JG_ERR_ARG, "reflect padding needs more than 256 samples");
    return timed(h, JG_ST_MISC, [&] { return launch_logmel(wav, B, n_samples, mel_basis, out, h->stream); });
}

int jg_jegal_text(jg_handle* h, const float* states, const float* mask, int B, int L, float* out) {
    ENTER(h);
    if (!states || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    RET(begin_pass(h));
    return jegal_text_impl(h, states, mask, B, L, out);
}

int jg_xlmr_encode(jg_handle* h, const int32_t* input_ids, const int32_t* attention_mask, int B, int L, float* out) {
    ENTER(h);
    if (!input_ids || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    // Option xlmr_lanes > 1 (experiment, see jg_handle::xl_lanes): sequences are independent, and at B * L = 16 384 tokens the N = 768
    // GEMMs are single rounds of 192 tiles on 256 CUs and qkv is 2.25 rounds -- two half batches on two streams let one lane's
    // kernels start on the CUs the other's last round leaves idle.
    auto run_part = [&](int b0, int nb) -> int {
        RET(begin_pass(h));
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
    RET(begin_pass(h));
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
    if (!h->gs.m.ready || !h->jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "GestSync and JEGAL weights must both be finalized");
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
        // one pass for both stages: gestsync_clip_impl begins it, the JEGAL stage goes on allocating behind the last chunk's buffers
        RET(gestsync_clip_impl(h, fr, dtype, nb, T, feats));
        RET(jegal_gestures_impl(h, feats, nullptr, nb, T, 1, emb));
        return timed(h, JG_ST_MISC, [&] { return launch_l2norm(emb, emb, nb * T, 512, h->stream); });
    };
    return run_in_lanes(h, B, T, run_part);
}

// ---- the metric entries
int jg_pool_mean(jg_handle* h, const float* x, const int32_t* off, int n, int D, float* out) {
    ENTER(h);
    if (!x || !off || !out) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return misc_launch(h, launch_ragged_mean, x, off, n, D, out);
}

int jg_sim_rank(jg_handle* h, const float* e1, const float* e2, int n_local, int n_total, int row_offset, int D,
                int32_t* rank, int32_t* ties) {
    ENTER(h);
    if (!e1 || !e2 || !rank || !ties) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (D % 64 || row_offset < 0 || row_offset + n_local > n_total) JG_FAIL(h, JG_ERR_ARG, "bad sim_rank geometry");
    return misc_launch(h, launch_sim_rank, e1, e2, n_local, n_total, row_offset, D, rank, ties);
}

// The checks that several entries make, each written once.  Two row operands (`names` for the message): D a positive multiple of 64, at
// most max_D where the entry has a maximum (0: none), both 16-byte aligned
static int row_pair_check(jg_handle* h, const char* names, const float* a, const float* b, int D, int max_D = 0) {
    if (max_D && (D <= 0 || D % 64 || D > max_D)) JG_FAIL(h, JG_ERR_ARG, "D must be a positive multiple of 64, at most %d", max_D);
    if (D <= 0 || D % 64) JG_FAIL(h, JG_ERR_ARG, "D must be a positive multiple of 64");
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) JG_FAIL(h, JG_ERR_ARG, "%s must be 16-byte aligned", names);
    return JG_OK;
}
static int shift_check(jg_handle* h, int max_shift, int min_overlap) {
    if (max_shift < 0 || max_shift > SYNC_MAX_R) JG_FAIL(h, JG_ERR_ARG, "max_shift must be 0..%d", SYNC_MAX_R);
    if (min_overlap < 1) JG_FAIL(h, JG_ERR_ARG, "min_overlap must be >= 1");
    return JG_OK;
}
// the arguments jg_sim_topk and jg_sim_topk_grouped share (`entry` names the caller in the geometry message; n_groups: 0 for the former)
static int sim_topk_check(jg_handle* h, const char* entry, const float* queries, const float* gallery, int n_queries, int n_gallery, int D,
                          int k, int n_groups, int gallery_offset) {
    if (k < 1 || k > SIM_TOPK_MAX_K) JG_FAIL(h, JG_ERR_ARG, "k must be 1..%d", SIM_TOPK_MAX_K);
    if (n_queries < 0 || n_gallery < 0 || n_groups < 0 || gallery_offset < 0 || gallery_offset > INT32_MAX - n_gallery)
        JG_FAIL(h, JG_ERR_ARG, "bad %s geometry (counts and gallery_offset >= 0, gallery_offset + n_gallery <= INT32_MAX)", entry);
    return row_pair_check(h, "queries / gallery", queries, gallery, D);
}

int jg_sim_topk(jg_handle* h, const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k,
                int gallery_offset, int merge, int32_t* idx, float* score) {
    ENTER(h);
    if (!queries || !gallery || !idx || !score) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    RET(sim_topk_check(h, "sim_topk", queries, gallery, n_queries, n_gallery, D, k, 0, gallery_offset));
    if (n_queries == 0) return JG_OK;
    return misc_launch(h, launch_sim_topk, queries, gallery, n_queries, n_gallery, D, k, gallery_offset, merge, idx, score);
}

int jg_sim_topk_grouped(jg_handle* h, const float* queries, const float* gallery, int n_queries, int n_gallery, int D, int k,
                        const int32_t* g_offsets, int n_groups, int gallery_offset, int merge, int32_t* idx, float* score) {
    ENTER(h);
    if (!queries || !gallery || !idx || !score || (n_groups > 0 && !g_offsets)) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    RET(sim_topk_check(h, "sim_topk_grouped", queries, gallery, n_queries, n_gallery, D, k, n_groups, gallery_offset));
    if (n_queries == 0) return JG_OK;
    return misc_launch(h, launch_sim_topk_grouped, queries, gallery, n_queries, n_gallery, D, k, g_offsets, n_groups, gallery_offset, merge, idx,
                       score);
}

int jg_sim_search(jg_handle* h, const float* queries, int n_queries, const void* gallery, int gallery_dtype, int n_gallery, int D, int k,
                  const int32_t* g_offsets, int n_groups, int gallery_offset, int merge, int slices, int32_t* idx, float* score) {
    if (!h) return JG_ERR_ARG;
    const KernelNameScope kn(h->kname);          // the launch depends on the plan: jg_debug_last_kernel shows which one it was
    ENTER(h);
    if (!queries || !gallery || !idx || !score) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (!g_offsets && n_groups != 0) JG_FAIL(h, JG_ERR_ARG, "g_offsets == NULL means ungrouped: n_groups must be 0");
    if (gallery_dtype != JG_F32 && gallery_dtype != JG_F16) JG_FAIL(h, JG_ERR_ARG, "gallery_dtype must be JG_F32 or JG_F16");
    RET(sim_topk_check(h, "sim_search", queries, static_cast<const float*>(gallery), n_queries, n_gallery, D, k, n_groups, gallery_offset));
    // no gallery row, or grouped without a group: no tile to walk; one launch seeds and stores the lists as the plain entries do
    const bool no_rows = n_gallery == 0 || (g_offsets && n_groups == 0);
    SimSearchPlan plan;
    if (!sim_search_plan(n_queries, no_rows ? 0 : n_gallery, k, h->opts.num_cu, slices, plan))
        JG_FAIL(h, JG_ERR_ARG, "slices must be 0 (the library chooses) .. %d, and the slices' lists (slices x n_queries x k x 8 bytes) at most %d bytes",
                SIM_SEARCH_MAX_SLICES, SIM_SEARCH_MAX_WS);
    if (n_queries == 0) return JG_OK;
    unsigned long long* keys = nullptr;          // the slices' lists: scratch of this call, one pass
    if (plan.slices > 1) {
        RET(begin_pass(h));
        RET(wsalloc(h, (size_t)(plan.ws_bytes / 8), &keys));
    }
    const int rc = misc_launch(h, launch_sim_search, queries, gallery, gallery_dtype == JG_F16, n_queries, n_gallery, D, k, g_offsets, n_groups,
                               gallery_offset, merge, idx, score, plan.slices, plan.slice_rows, keys);
    if (rc != JG_OK) h->kname[0] = 0;            // (a failure may come from behind the launcher's record)
    return rc;
}

// jg_sim_coupling and jg_sim_ordered: one entry, two launchers with one signature (`entry` names the caller in the geometry message)
using CouplingLauncher = decltype(&launch_sim_coupling);
static int coupling_entry(jg_handle* h, const char* entry, CouplingLauncher launcher, const float* words, const int32_t* w_offsets_host,
                          int n_queries, const void* gallery, int gallery_dtype, int n_gallery, int D, int k, const int32_t* g_offsets,
                          int n_groups, int group_offset, int merge, int slices, int32_t* idx, float* score, float* pair, int64_t pair_ld) {
    if (!h) return JG_ERR_ARG;
    const KernelNameScope kn(h->kname);          // the launch depends on the plan, as in jg_sim_search
    ENTER(h);
    if (!words || !w_offsets_host || !gallery || !idx || !score || (n_groups > 0 && !g_offsets)) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (gallery_dtype != JG_F32 && gallery_dtype != JG_F16) JG_FAIL(h, JG_ERR_ARG, "gallery_dtype must be JG_F32 or JG_F16");
    // (the check of the top-k entries, with the groups as what group_offset numbers)
    RET(sim_topk_check(h, entry, words, static_cast<const float*>(gallery), n_queries, n_gallery, D, k, n_groups, 0));
    if (group_offset < 0 || group_offset > INT32_MAX - n_groups) JG_FAIL(h, JG_ERR_ARG, "group_offset >= 0, group_offset + n_groups <= INT32_MAX");
    if (pair && (pair_ld < n_queries || (reinterpret_cast<uintptr_t>(pair) & 3))) JG_FAIL(h, JG_ERR_ARG, "pair needs pair_ld >= n_queries");
    const bool no_rows = n_gallery == 0 || n_groups == 0;
    std::vector<int32_t> tables((size_t)n_queries * 2 + 2);      // w_offsets [n_queries + 1], then tile_first_query [n_tiles + 1]
    int32_t* const tfq_host = tables.data() + n_queries + 1;
    CouplingPlan plan;
    if (!sim_coupling_plan(w_offsets_host, n_queries, no_rows ? 0 : n_gallery, k, h->opts.num_cu, slices, tfq_host, plan))
        JG_FAIL(h, JG_ERR_ARG, "w_offsets must start at 0 and give every query 1..%d word rows; slices must be 0 (the library chooses) .. %d, and "
                "the slices' lists (slices x n_queries x k x 8 bytes) at most %d bytes", COUPLING_MAX_W, SIM_SEARCH_MAX_SLICES, SIM_SEARCH_MAX_WS);
    if (n_queries == 0) return JG_OK;
    std::memcpy(tables.data(), w_offsets_host, ((size_t)n_queries + 1) * sizeof(int32_t));
    RET(begin_pass(h));
    int32_t* tables_dev = nullptr;
    unsigned long long* keys = nullptr;
    RET(wsalloc(h, tables.size(), &tables_dev));
    if (plan.cut.slices > 1) RET(wsalloc(h, (size_t)(plan.cut.ws_bytes / 8), &keys));
    RET(upload_i32_async(h, tables.data(), (size_t)n_queries + 1 + plan.n_tiles + 1, tables_dev));
    if (pair) RET(misc_launch(h, launch_coupling_fill, pair, (long)pair_ld, n_queries, n_groups));
    const int rc = misc_launch(h, launcher, words, tables_dev, tables_dev + n_queries + 1, plan.n_tiles, gallery, gallery_dtype == JG_F16,
                               n_queries, n_gallery, D, k, g_offsets, n_groups, group_offset, merge, idx, score, pair, (long)pair_ld,
                               plan.cut.slices, plan.cut.slice_rows, keys);
    if (rc != JG_OK) h->kname[0] = 0;
    return rc;
}

int jg_sim_coupling(jg_handle* h, const float* words, const int32_t* w_offsets_host, int n_queries, const void* gallery, int gallery_dtype,
                    int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge, int slices, int32_t* idx,
                    float* score, float* pair, int64_t pair_ld) {
    return coupling_entry(h, "sim_coupling", launch_sim_coupling, words, w_offsets_host, n_queries, gallery, gallery_dtype, n_gallery, D, k,
                          g_offsets, n_groups, group_offset, merge, slices, idx, score, pair, pair_ld);
}

int jg_sim_ordered(jg_handle* h, const float* words, const int32_t* w_offsets_host, int n_queries, const void* gallery, int gallery_dtype,
                   int n_gallery, int D, int k, const int32_t* g_offsets, int n_groups, int group_offset, int merge, int slices, int32_t* idx,
                   float* score, float* pair, int64_t pair_ld) {
    return coupling_entry(h, "sim_ordered", launch_sim_ordered, words, w_offsets_host, n_queries, gallery, gallery_dtype, n_gallery, D, k,
                          g_offsets, n_groups, group_offset, merge, slices, idx, score, pair, pair_ld);
}

int jg_sim_align(jg_handle* h, const float* words, const int32_t* w_offsets_host, int n_queries, const void* gallery, int gallery_dtype,
                 int n_gallery, int D, const int32_t* g_offsets, int n_groups, int group_offset, const int32_t* idx, int k, int ordered,
                 int32_t* frames, int frames_ld, float* score) {
    if (!h) return JG_ERR_ARG;
    const KernelNameScope kn(h->kname);
    ENTER(h);
    if (!words || !w_offsets_host || !gallery || !idx || !frames || !score || (n_groups > 0 && !g_offsets)) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (gallery_dtype != JG_F32 && gallery_dtype != JG_F16) JG_FAIL(h, JG_ERR_ARG, "gallery_dtype must be JG_F32 or JG_F16");
    RET(sim_topk_check(h, "sim_align", words, static_cast<const float*>(gallery), n_queries, n_gallery, D, k, n_groups, 0));
    if (group_offset < 0 || group_offset > INT32_MAX - n_groups) JG_FAIL(h, JG_ERR_ARG, "group_offset >= 0, group_offset + n_groups <= INT32_MAX");
    // the word offsets as jg_sim_coupling takes them: its plan is the check (one slice: no lists to size)
    std::vector<int32_t> tfq((size_t)n_queries + 1);
    CouplingPlan plan;
    if (!sim_coupling_plan(w_offsets_host, n_queries, 0, k, h->opts.num_cu, 1, tfq.data(), plan))
        JG_FAIL(h, JG_ERR_ARG, "w_offsets must start at 0 and give every query 1..%d word rows", COUPLING_MAX_W);
    int longest = 0;
    for (int q = 0; q < n_queries; ++q) longest = std::max(longest, (int)(w_offsets_host[q + 1] - w_offsets_host[q]));
    if (frames_ld < longest || frames_ld < 1) JG_FAIL(h, JG_ERR_ARG, "frames_ld must hold the longest query (%d word rows)", longest);
    if ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(score) | reinterpret_cast<uintptr_t>(idx)) & 3)
        JG_FAIL(h, JG_ERR_ARG, "idx, frames and score must be 4-byte aligned");
    if (n_queries == 0) return JG_OK;
    RET(begin_pass(h));
    int32_t* woff_dev = nullptr;
    RET(wsalloc(h, (size_t)n_queries + 1, &woff_dev));
    RET(upload_i32_async(h, w_offsets_host, (size_t)n_queries + 1, woff_dev));
    const int rc = misc_launch(h, launch_sim_align, words, woff_dev, gallery, gallery_dtype == JG_F16, n_queries, n_gallery, D, g_offsets, n_groups,
                               group_offset, idx, k, ordered, frames, frames_ld, score);
    if (rc != JG_OK) h->kname[0] = 0;
    return rc;
}

int jg_group_of_rows(jg_handle* h, const int32_t* idx, int64_t n, const int32_t* g_offsets, int n_groups, int gallery_offset,
                     int32_t* grp, int32_t* pos) {
    ENTER(h);
    if (!idx || !grp || !pos || (n_groups > 0 && !g_offsets)) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (n < 0 || n_groups < 0 || gallery_offset < 0) JG_FAIL(h, JG_ERR_ARG, "n, n_groups and gallery_offset must be >= 0");
    if (n == 0) return JG_OK;
    return misc_launch(h, launch_group_of_rows, idx, (long)n, g_offsets, n_groups, gallery_offset, grp, pos);
}

int jg_spot(jg_handle* h, const float* g, const float* c, const int32_t* goff, const int32_t* coff, const int32_t* target,
            int n, int D, float temp, int32_t* pred, float* score) {
    ENTER(h);
    if (!g || !c || !goff || !coff || !target || !pred || !score) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return misc_launch(h, launch_spot, g, c, goff, coff, target, n, D, temp, pred, score);
}

int jg_attn_matrix(jg_handle* h, const float* g, const float* c, const int32_t* goff, const int32_t* coff, int n, int D, int max_frames,
                   float temp, int normalize, float* A, const int64_t* aoff, int32_t* best_frame, float* best_score) {
    ENTER(h);
    if (!g || !c || !goff || !coff) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (A && !aoff) JG_FAIL(h, JG_ERR_ARG, "A needs a_offsets");
    if (!A && !best_frame && !best_score) JG_FAIL(h, JG_ERR_ARG, "no output: A, best_frame and best_score are all NULL");
    if (n < 0 || max_frames < 1 || max_frames > SPOT_MAX_T) JG_FAIL(h, JG_ERR_ARG, "max_frames must be 1..%d (and n_clips >= 0)", SPOT_MAX_T);
    if (!(temp > 0.f)) JG_FAIL(h, JG_ERR_ARG, "temp must be positive");
    RET(row_pair_check(h, "gesture / content", g, c, D));
    if (n == 0) return JG_OK;
    unsigned long long* keys = nullptr;          // per-word arg-max keys, combined across the frame blocks of a clip
    RET(begin_pass(h));
    if (best_frame || best_score) RET(wsalloc(h, attn_matrix_key_elems(n), &keys));
    return misc_launch(h, launch_attn_matrix, g, c, goff, coff, n, D, max_frames, temp, normalize, A, aoff, keys, best_frame, best_score);
}

int jg_attn_talk(jg_handle* h, const float* gesture, const int32_t* g_offsets, int n_tracks, int64_t n_rows, int max_frames,
                 const float* content, const int32_t* c_offsets, int n_words, const int32_t* word_start, const int32_t* word_end, int D,
                 int reach, float temp, int normalize, float* band, int band_pitch, int32_t* best_frame, float* best_score,
                 int32_t* frame_word, float* frame_prob) {
    ENTER(h);
    if (!gesture || !g_offsets || !content || !c_offsets || !word_start || !word_end) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (!band && !best_frame && !best_score && !frame_word && !frame_prob)
        JG_FAIL(h, JG_ERR_ARG, "no output: band, best_frame, best_score, frame_word and frame_prob are all NULL");
    if (n_tracks < 0 || n_rows < 0 || n_rows > INT32_MAX || n_words < 0) JG_FAIL(h, JG_ERR_ARG, "n_tracks, n_rows (int32) and n_words must be >= 0");
    if (max_frames < 1 || max_frames > TALK_MAX_T) JG_FAIL(h, JG_ERR_ARG, "max_frames must be 1..%d", TALK_MAX_T);
    if (reach < 0 || reach > TALK_MAX_REACH) JG_FAIL(h, JG_ERR_ARG, "reach must be 0..%d", TALK_MAX_REACH);
    if (!(temp > 0.f)) JG_FAIL(h, JG_ERR_ARG, "temp must be positive");
    if (band && (band_pitch < 1 || (int64_t)n_words * band_pitch > INT32_MAX))
        JG_FAIL(h, JG_ERR_ARG, "band needs band_pitch >= 1 and n_words x band_pitch < 2^31");
    RET(row_pair_check(h, "gesture / content", gesture, content, D));
    if (n_tracks == 0) return JG_OK;
    unsigned long long* keys = nullptr;          // per-word arg-max keys, combined across the frame blocks of a track
    if (best_frame || best_score) {
        RET(begin_pass(h));
        RET(wsalloc(h, (size_t)(n_words > 0 ? n_words : 1), &keys));
    }
    return misc_launch(h, launch_attn_talk, gesture, g_offsets, n_tracks, (long)n_rows, max_frames, content, c_offsets, n_words, word_start, word_end,
                       D, reach, temp, normalize, band, band_pitch, keys, best_frame, best_score, frame_word, frame_prob);
}

int jg_sync_offset(jg_handle* h, const float* vid, const int32_t* v_offsets, const float* aud, const int32_t* a_offsets, int n_clips, int D,
                   int max_shift, int min_overlap, float* curve, int32_t* offset, float* conf) {
    ENTER(h);
    if (!vid || !v_offsets || !aud || !a_offsets || !offset || !conf) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (n_clips < 0) JG_FAIL(h, JG_ERR_ARG, "n_clips must be >= 0");
    RET(shift_check(h, max_shift, min_overlap));
    RET(row_pair_check(h, "vid / aud", vid, aud, D, SYNC_MAX_D));
    if (n_clips == 0) return JG_OK;
    return misc_launch(h, launch_sync_offset, vid, v_offsets, aud, a_offsets, n_clips, D, max_shift, min_overlap, curve, offset, conf);
}

int jg_sync_offset_windows(jg_handle* h, const float* vid, const int32_t* v_offsets, int n_clips, int64_t n_vid_rows, int max_rows,
                           const float* aud, const int32_t* a_offsets, int n_aud, const int32_t* a_of, int D, int max_shift, int min_overlap,
                           int win, int hop, const int32_t* w_offsets, int max_windows, float* band, float* curve, int32_t* offset,
                           float* conf) {
    ENTER(h);
    if (!vid || !v_offsets || !aud || !a_offsets || !w_offsets || !offset || !conf) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (n_clips < 0 || n_aud < 0 || n_vid_rows < 0) JG_FAIL(h, JG_ERR_ARG, "n_clips, n_aud and n_vid_rows must be >= 0");
    if (!a_of && n_aud != n_clips) JG_FAIL(h, JG_ERR_ARG, "without a_of clip i takes audio track i: n_aud must equal n_clips");
    RET(shift_check(h, max_shift, min_overlap));
    if (max_rows < 1 || max_rows > SYNCW_MAX_T) JG_FAIL(h, JG_ERR_ARG, "max_rows must be 1..%d", SYNCW_MAX_T);
    if (max_windows < 1 || max_windows > SYNCW_MAX_WINDOWS) JG_FAIL(h, JG_ERR_ARG, "max_windows must be 1..%d", SYNCW_MAX_WINDOWS);
    if (win < 0 || (win > 0 && hop < 1)) JG_FAIL(h, JG_ERR_ARG, "win must be >= 0 (0: one window over all rows) and hop >= 1");
    const int64_t band_max = (int64_t)1 << SYNCW_MAX_BAND_LOG2, band_elems = n_vid_rows * (2 * max_shift + 1);
    if (n_vid_rows >= band_max || band_elems >= band_max) JG_FAIL(h, JG_ERR_ARG, "the band (n_vid_rows x (2 max_shift + 1)) must stay below 2^%d entries", SYNCW_MAX_BAND_LOG2);
    RET(row_pair_check(h, "vid / aud", vid, aud, D, SYNC_MAX_D));
    if (n_clips == 0) return JG_OK;
    if (n_aud == 0) JG_FAIL(h, JG_ERR_ARG, "clips need an audio track: n_aud must be >= 1");
    if (!band) {                 // the band is scratch of this call: one pass, like jg_attn_matrix's keys
        RET(begin_pass(h));
        RET(wsalloc(h, (size_t)(band_elems > 0 ? band_elems : 1), &band));
    }
    return misc_launch(h, launch_sync_offset_windows, vid, v_offsets, n_clips, (long)n_vid_rows, max_rows, aud, a_offsets, n_aud, a_of, D, max_shift,
                       min_overlap, win, hop, w_offsets, max_windows, band, curve, offset, conf);
}

int jg_asd(jg_handle* h, const float* q, const float* cand, const int32_t* coff, int n, int D, float temp, int32_t* pred) {
    ENTER(h);
    if (!q || !cand || !coff || !pred) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    return misc_launch(h, launch_asd, q, cand, coff, n, D, temp, pred);
}

int jg_asd_windows(jg_handle* h, const float* gesture, const int32_t* g_offsets, int n_tracks, const float* content, const int32_t* c_offsets,
                   const int32_t* word_start, const int32_t* word_end, const int32_t* trk, const int32_t* s_offsets, int n_scenes, int D,
                   int win, int hop, const int32_t* w_offsets, const int64_t* p_offsets, int max_windows, float temp, float* prob,
                   float* cosv, int32_t* pred) {
    ENTER(h);
    if (!gesture || !g_offsets || !content || !c_offsets || !trk || !s_offsets || !w_offsets || !p_offsets || !prob || !pred)
        JG_FAIL(h, JG_ERR_ARG, "null buffer");
    if (n_scenes < 0 || n_tracks < 0) JG_FAIL(h, JG_ERR_ARG, "n_scenes and n_tracks must be >= 0");
    if (win < 0 || win > ASDW_MAX_WIN) JG_FAIL(h, JG_ERR_ARG, "win must be 0 (one window over everything) or 1..%d frames", ASDW_MAX_WIN);
    if (win > 0 && hop < 1) JG_FAIL(h, JG_ERR_ARG, "hop must be >= 1");
    if (win > 0 && (!word_start || !word_end)) JG_FAIL(h, JG_ERR_ARG, "windows need word_start and word_end");
    if (!(temp > 0.f)) JG_FAIL(h, JG_ERR_ARG, "temp must be positive");
    if (max_windows < 1 || max_windows > ASDW_MAX_WIN) JG_FAIL(h, JG_ERR_ARG, "max_windows must be 1..%d", ASDW_MAX_WIN);
    RET(row_pair_check(h, "gesture / content", gesture, content, D, ASDW_MAX_D));
    if (n_scenes == 0) return JG_OK;
    return misc_launch(h, launch_asd_windows, gesture, g_offsets, n_tracks, content, c_offsets, word_start, word_end, trk, s_offsets, n_scenes, D, win,
                       hop, w_offsets, p_offsets, max_windows, temp, prob, cosv, pred);
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
