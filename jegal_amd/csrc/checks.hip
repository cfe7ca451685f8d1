// libjegal_hip: the jg_debug_* entry points -- kernel check points, GEMM timing, what the last conv stack did.  Host code only.
#include "engine.h"

using namespace engine;

// ---- kernel check points: one launch of a production launcher on the caller's operands, with the handle's options (which pick
// the instance exactly as in production) and the handle's build (fp16 or bf16).  The launcher's own shape rules decide what is
// valid: its hipErrorInvalidValue comes back as JG_ERR_ARG, and nothing was launched then.  (Handle internals and LAUNCH: engine.h.)
// Which instance ran is the launcher's word, not this file's: a check point begins with ENTER_CHECK, which makes the handle's name slot
// the sink of record_kernel (shared.h) for the length of the call, and the launcher writes the name where it picks the instance.  No
// kernel is named here.  A check point of several launches reports the last one; one that is refused, here or by the launcher, or that
// fails reports "" (check_result).  jg_debug_gemm / jg_debug_gemm_ex only time launches and open no sink.
// jg_debug_gemm_plan asks the GEMM planner (gemm_plan.h) the same question without a handle, a device or a launch, and
// jg_debug_weight_form / jg_debug_gemm_runs_lo show which weights a layer's GEMM runs with (weight_form.h) in the same way.
namespace {
#define ENTER_CHECK(h) if (!(h)) return JG_ERR_ARG; const KernelNameScope _kn((h)->kname); ENTER(h)
// option debug_lanes: the handle's options read as inside a two-lane batch (EngineOpts::lanes_active) until the check point returns.
// Only the check points whose launchers read the flag take it: launch_gemm (plan_gemm) and, through gs_conv1_stage, launch_conv1_direct.
struct DebugLanes {
    jg_handle* const h;
    explicit DebugLanes(jg_handle* h_) : h(h_) { h->opts.lanes_active = h->debug_lanes; }
    ~DebugLanes() { h->opts.lanes_active = false; }
    DebugLanes(const DebugLanes&) = delete;
};
int check_result(jg_handle* h, hipError_t e, const char* what) {
    if (e != hipSuccess) h->kname[0] = 0;       // a refusal comes from in front of the launcher's record, a HIP failure may come from behind it
    if (e == hipErrorInvalidValue) JG_FAIL(h, JG_ERR_ARG, "%s: the launcher rejects this shape / argument set", what);
    if (e != hipSuccess) JG_FAIL(h, JG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return JG_OK;
}
// the GemmArgs of a jg_gemm_check
GemmArgs gemm_check_args(const jg_gemm_check* c) {
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
    a.a_tiled = c->a_tiled != 0;
    return a;
}
bool al(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
// a host [n] int32 array as the device array the launchers take, in the handle's workspace (as jg_debug_maxpool does for s2)
int upload_valid(jg_handle* h, const int32_t* host, int n, int32_t** dev) {
    RET(begin_pass(h));
    RET(wsalloc(h, (size_t)n, dev));
    return upload_i32_async(h, host, (size_t)n, *dev);
}
#define FP16_ONLY(h, name) \
    if ((h)->bf16) JG_FAIL(h, JG_ERR_STATE, name ": an fp16-build kernel (no bf16 handle reaches its launcher)")
}  // namespace

extern "C" {

int jg_debug_conv2_rowskip(jg_handle* h, int* rows) {
    ENTER(h);
    if (!rows) JG_FAIL(h, JG_ERR_ARG, "rows is NULL");
    *rows = 0;
    if (!h->conv_report.rowskip) return JG_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(rows, h->conv_report.rowskip, sizeof(int), hipMemcpyDeviceToHost));
    return JG_OK;
}

int jg_debug_conv_rows(jg_handle* h, int64_t* computed, int64_t* full) {
    ENTER(h);
    if (!computed || !full) JG_FAIL(h, JG_ERR_ARG, "null buffer");
    for (int l = 0; l < 4; ++l) computed[l] = full[l] = 0;
    if (!h->conv_report.totals) return JG_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int t[4];
    HIPCHK(h, hipMemcpy(t, h->conv_report.totals, sizeof(t), hipMemcpyDeviceToHost));
    for (int l = 0; l < 4; ++l) { computed[l] = t[l]; full[l] = h->conv_report.full[l]; }
    return JG_OK;
}

int jg_debug_conv1_pool(jg_handle* h, const void* frames_u8, int B, int T, int pad, void* out_f16) {
    ENTER_CHECK(h);
    if (!h->gs.m.ready) JG_FAIL(h, JG_ERR_STATE, "GestSync weights not finalized");
    if (!frames_u8 || !out_f16 || B <= 0 || pad < 0 || pad > 12 || T + 2 * pad < 5)      // conv1's skip-mask area is sized for pad <= 12
        JG_FAIL(h, JG_ERR_ARG, "bad arguments (need 0 <= pad <= 12 and T + 2*pad >= 5)");
    RET(begin_pass(h));
    const long sw = 3, sh = (long)FW * 3, st = (long)FH * FW * 3, sb = (long)T * st;
    unsigned* zscr;
    const DebugLanes lanes(h);
    const int rc = gs_conv1_stage(h, frames_u8, 1, sb, st, sh, sw, 1, B, T, pad, static_cast<f16*>(out_f16), true, &zscr);
    if (rc != JG_OK) h->kname[0] = 0;
    return rc;
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
    RET(begin_pass(h));
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

int jg_debug_gemm_check(jg_handle* h, const jg_gemm_check* c) {
    ENTER_CHECK(h);
    if (!c || !c->A || !c->Wh || c->M <= 0 || c->N <= 0 || c->K <= 0 || c->lda < c->K || c->ldw < c->K || (!c->out32 && !c->out16) ||
        ((c->out32 || (c->out16 && !c->ln_w)) && c->ldc < c->N) || (c->res && (c->ldr < c->N || c->res_mod < 0)) ||
        (c->bias_clip && (c->rpc <= 0 || c->nclips <= 0)) || c->relu < 0 || c->relu > 2 || c->ln_mode < 0 || c->ln_mode > 2)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_gemm_check: bad arguments");
    if (c->a_tiled) { FP16_ONLY(h, "jg_debug_gemm_check with a_tiled"); }
    const GemmArgs a = gemm_check_args(c);
    const DebugLanes lanes(h);
    return check_result(h, LAUNCH(h, launch_gemm, a, false, h->opts, h->stream), "launch_gemm");
}

// One conv launch of launch_gemm.  With s2_host the launch runs as layer `op` of the row-skipping chain does in gs_conv_stack: the production
// launch_conv_rowmaps builds the layer's compacted map in the workspace in front of the GEMM.  The planner is asked before anything is
// enqueued, so a rejected argument set launches nothing at all.
int jg_debug_conv_check(jg_handle* h, const jg_conv_check* c) {
    ENTER_CHECK(h);
    if (!c || !c->in || !c->Wh || c->nimg <= 0 || c->H <= 0 || c->W <= 0 || c->C < 8 || (c->C & (c->C - 1)) || c->KH <= 0 || c->KW <= 0 || c->KH > 15 ||
        c->KW > 15 || c->SH <= 0 || c->SW <= 0 || c->PH < 0 || c->PW < 0 || c->H + 2 * c->PH < c->KH || c->W + 2 * c->PW < c->KW || c->N <= 0 ||
        (long)c->KH * c->KW * c->C != c->K || c->ldw < c->K || (!c->out32 && !c->out16) || c->ldc < c->N || c->relu < 0 || c->relu > 1 || c->op < 0 ||
        c->op > 3 || (c->const_in && (!c->s2_host || c->op == 0)))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv_check: bad arguments (K = KH KW C, C a power of two >= 8, relu 0 / 1, op 0..3, const_in needs s2_host and op >= 1)");
    ConvGeom g = geom(c->H, c->W, c->C, c->KH, c->KW, c->SH, c->SW, c->PH, c->PW, c->reorder != 0);
    const long M = (long)c->nimg * g.OH * g.OW;
    if (M >= (1L << 31)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv_check: too many output pixels");
    if (c->s2_host) {
        for (int i = 0; i < c->nimg; ++i)
            if (c->s2_host[i] < 0 || c->s2_host[i] > ROWMAP_MAX_S2 || conv_skip_decode(c->s2_host[i], c->op) >= g.OH)
                JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv_check: s2[%d] = %d outside 0..255 or leaves image %d no output row", i, c->s2_host[i], i);
    }
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.A = static_cast<const f16*>(c->in);
    a.Wh = static_cast<const f16*>(c->Wh); a.Wl = static_cast<const f16*>(c->Wl); a.ldw = c->ldw;
    a.M = (int)M; a.N = c->N; a.K = c->K;
    a.scale = c->scale; a.bias = c->bias; a.relu = c->relu;
    a.out32 = c->out32; a.out16 = static_cast<f16*>(c->out16); a.ldc = c->ldc;
    const DebugLanes lanes(h);
    if (c->s2_host) {
        GemmShape q = gemm_shape(a, false);
        q.set_geom(g);
        q.rowmap = true; q.const_in = c->const_in != nullptr;
        if (!plan_gemm(q, h->opts).ok()) JG_FAIL(h, JG_ERR_ARG, "launch_gemm: the launcher rejects this shape / argument set");
        RET(begin_pass(h));
        int32_t* s2;
        ConvRowMap rm;
        const f16* const cin = static_cast<const f16*>(c->const_in);
        RET(wsalloc(h, (size_t)c->nimg, &s2));
        RET(rowmap_chain(h, c->nimg, 1, &g.OH, &g.OW, c->op, &rm, &g, &cin));
        RET(upload_i32_async(h, c->s2_host, (size_t)c->nimg, s2));
        RET(check_result(h, launch_conv_rowmaps(s2, c->nimg, &rm, 1, h->stream), "launch_conv_rowmaps"));
    }
    a.g = g;
    return check_result(h, LAUNCH(h, launch_gemm, a, true, h->opts, h->stream), "launch_gemm");
}

int jg_debug_maxpool(jg_handle* h, const void* in, int nimg, int H, int W, int C, const int32_t* s2_host, int in_op, const void* const_in, void* out) {
    ENTER_CHECK(h);
    if (!in || !out || nimg <= 0 || H < 3 || W < 3 || C <= 0 || C % 8 || (s2_host != nullptr) != (const_in != nullptr) || in_op < 0 || in_op > 3)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_maxpool: bad arguments (C %% 8 == 0, H, W >= 3, s2_host and const_in together, in_op 0..3)");
    int32_t* s2 = nullptr;
    if (s2_host) {
        for (int i = 0; i < nimg; ++i)
            if (s2_host[i] < 0 || s2_host[i] > ROWMAP_MAX_S2 || conv_skip_decode(s2_host[i], in_op) > H)
                JG_FAIL(h, JG_ERR_ARG, "jg_debug_maxpool: s2[%d] = %d outside 0..255 or past the image's %d rows", i, s2_host[i], H);
        RET(begin_pass(h));
        RET(wsalloc(h, (size_t)nimg, &s2));
        RET(upload_i32_async(h, s2_host, (size_t)nimg, s2));
    }
    return check_result(h, LAUNCH(h, launch_maxpool3x3s2, static_cast<const f16*>(in), static_cast<f16*>(out), nimg, H, W, C, h->stream,
                                  static_cast<const int*>(s2), in_op, static_cast<const f16*>(const_in)), "launch_maxpool3x3s2");
}

int jg_debug_gsa_conv1_pool(jg_handle* h, const float* src, int clip_form, int B, int Tm, int T, const int32_t* valid_host, const float* w,
                            const float* shift, void* out, int out_f32) {
    ENTER_CHECK(h);
    if (!src || !w || !shift || !out || B <= 0 || T <= 0 || (clip_form && Tm <= 0) || (!clip_form && (T != 1 || valid_host)) || !al(out, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_gsa_conv1_pool: bad arguments (window form: T = 1 and no valid_host)");
    for (int b = 0; valid_host && b < B; ++b)
        if (valid_host[b] < 1 || valid_host[b] > Tm) JG_FAIL(h, JG_ERR_ARG, "jg_debug_gsa_conv1_pool: valid[%d] = %d outside 1..Tm = %d", b, valid_host[b], Tm);
    int32_t* valid = nullptr;
    if (valid_host) RET(upload_valid(h, valid_host, B, &valid));
    return check_result(h, launch_gsa_conv1_pool(src, clip_form, 0, B * T, T, Tm, valid, w, shift, out, out_f32, h->stream), "launch_gsa_conv1_pool");
}

int jg_debug_maxpool_2x3(jg_handle* h, const void* in, int nimg, int H, int W, int C, void* out, int f32) {
    ENTER_CHECK(h);
    if (!in || !out || nimg <= 0) JG_FAIL(h, JG_ERR_ARG, "jg_debug_maxpool_2x3: bad arguments");
    return check_result(h, launch_maxpool_2x3_s2(in, out, nimg, H, W, C, f32, h->stream), "launch_maxpool_2x3_s2");
}

int jg_debug_conv_rowmaps(jg_handle* h, const int32_t* s2_host, int NF, const int* OH, const int* OW, int nlayers, int32_t* const* map_host,
                          int32_t* const* base_host, int32_t* total_host) {
    ENTER_CHECK(h);
    if (!s2_host || !OH || !OW || !map_host || !base_host || !total_host || NF <= 0) JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv_rowmaps: bad arguments");
    if (nlayers < 1 || nlayers > 4) JG_FAIL(h, JG_ERR_ARG, "launch_conv_rowmaps: the launcher rejects this shape / argument set");
    for (int l = 0; l < nlayers; ++l) {
        if (OH[l] <= 0 || OW[l] <= 0 || !map_host[l] || !base_host[l]) JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv_rowmaps: bad layer %d", l);
        for (int i = 0; i < NF; ++i)
            if (s2_host[i] < 0 || s2_host[i] > ROWMAP_MAX_S2 || conv_skip_decode(s2_host[i], l) > OH[l])
                JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv_rowmaps: s2[%d] = %d outside 0..255 or past layer %d's %d rows", i, s2_host[i], l, OH[l]);
    }
    RET(begin_pass(h));
    int32_t* s2;
    ConvRowMap rm[4];
    RET(wsalloc(h, (size_t)NF, &s2));
    RET(rowmap_chain(h, NF, nlayers, OH, OW, 0, rm));
    RET(upload_i32_async(h, s2_host, (size_t)NF, s2));
    for (int l = 0; l < nlayers; ++l)      // the caller's fill: the launch writes the first *total entries only (on the stream: behind the pass's poison)
        HIPCHK(h, hipMemcpyAsync(rm[l].map, map_host[l], (size_t)NF * OH[l] * OW[l] * sizeof(int), hipMemcpyHostToDevice, h->stream));
    RET(check_result(h, launch_conv_rowmaps(s2, NF, rm, nlayers, h->stream), "launch_conv_rowmaps"));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int l = 0; l < nlayers; ++l) {
        HIPCHK(h, hipMemcpy(map_host[l], rm[l].map, (size_t)NF * OH[l] * OW[l] * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(base_host[l], rm[l].base, ((size_t)NF + 1) * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(total_host + l, rm[l].total, sizeof(int), hipMemcpyDeviceToHost));
    }
    return JG_OK;
}

int jg_debug_gemm_plan(const jg_gemm_check* c, const jg_conv_shape* conv, int a_tiled, int num_cu, int lanes_active, const char* const* opt_names,
                       const int* opt_values, int n_opts, char* name, int name_len, int* grid, int* lds, int* stagger) {
    if (!c || c->M <= 0 || c->N <= 0 || c->K <= 0 || num_cu <= 0 || n_opts < 0 || (n_opts && (!opt_names || !opt_values)) || !name || name_len <= 0 ||
        !grid || !lds || !stagger)
        return JG_ERR_ARG;
    GemmShape s = gemm_shape(gemm_check_args(c), false);
    s.a_tiled = a_tiled != 0 || c->a_tiled != 0;
    if (conv) {
        s.conv = true;
        s.H = conv->H; s.W = conv->W; s.C = conv->C; s.KH = conv->KH; s.KW = conv->KW; s.PH = conv->PH; s.PW = conv->PW;
        s.tap_table = conv->tap_table; s.rowmap = conv->rowmap != 0; s.const_in = conv->const_in != 0;
    }
    EngineOpts o;
    o.num_cu = num_cu;
    o.lanes_active = lanes_active != 0;
    for (int i = 0; i < n_opts; ++i)
        if (!opt_names[i] || !engine_opts_set(o, opt_names[i], opt_values[i])) return JG_ERR_ARG;
    const GemmPlan p = plan_gemm(s, o);
    snprintf(name, (size_t)name_len, "%s", p.name);
    *grid = (int)p.grid; *lds = (int)p.lds; *stagger = p.stagger;
    return JG_OK;
}

int jg_debug_weight_form(int precision, int kind, int model, int keep32, int* form, int* lo_kept_out, int* uncalibrated) {
    if (precision < JG_PREC_FP16 || precision > JG_PREC_FP32 || kind < LK_CONV || kind > LK_XLMR || model < 1 || model > 3 || !form || !lo_kept_out ||
        !uncalibrated)
        return JG_ERR_ARG;
    const WeightForm f = weight_form(precision, kind, model);
    *form = f; *lo_kept_out = lo_kept(f, keep32 != 0); *uncalibrated = starts_uncalibrated(f, kind);
    return JG_OK;
}

int jg_debug_gemm_runs_lo(int form, int uncalibrated, int calibrating, int clip_bias, int* lo) {
    if (form < WF_SINGLE || form > WF_RUNTIME_CORRECTED || !lo) return JG_ERR_ARG;
    *lo = runs_with_lo((WeightForm)form, uncalibrated != 0, calibrating != 0, clip_bias != 0);
    return JG_OK;
}

// ---- the weight packing on caller arrays (weight_pack.h): no handle, no device; nothing is written unless every argument is good
int jg_debug_pack_conv(const float* w, const float* bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, int O,
                       int I, int KT, int KH, int KW, int slot, int kpad, int Opad, int SH, int SW, int reorder, int N, int K, float* matrix, float* shift) {
    const bool bn = bn_gamma || bn_beta || bn_mean || bn_var;
    if (!w || !bias || (bn && !(bn_gamma && bn_beta && bn_mean && bn_var)) || !matrix || !shift) return JG_ERR_ARG;
    if (O <= 0 || I <= 0 || KT <= 0 || KH <= 0 || KW <= 0 || slot <= 0 || kpad < 0 || Opad < 0 || SH <= 0 || SW <= 0) return JG_ERR_ARG;
    if ((long)KH * KW > 4096 || (long)KT * I > slot || (long)KH * KW * slot > (1L << 24)) return JG_ERR_ARG;
    const ConvPack c = {O, I, KT, KH, KW, slot, kpad, Opad, SH, SW, reorder != 0};
    if (N != conv_pack_N(c) || K != conv_pack_K(c) || KH * KW * slot > K) return JG_ERR_ARG;
    std::vector<float> s(O, 1.f), sh(bias, bias + O);
    if (bn) bn_fold(bias, bn_gamma, bn_beta, bn_mean, bn_var, O, s.data(), sh.data());
    sh.resize(N, 0.f);
    const std::vector<float> p = conv_matrix(w, s.data(), c);
    std::memcpy(matrix, p.data(), p.size() * sizeof(float));
    std::memcpy(shift, sh.data(), sh.size() * sizeof(float));
    return JG_OK;
}

int jg_debug_pack_round(const float* w, const float* bias, int N, int K, int bf16, int form, int keep_lo, int diffuse_group, const float* ln_gamma,
                        const float* ln_beta, const float* add_beta, int device32, uint16_t* hi, uint16_t* lo, float* bias_out, float* c1h, float* c1f,
                        float* w32, float* b32) {
    const bool consumer = ln_gamma || ln_beta;
    if (!w || !bias || N <= 0 || K <= 0 || form < WF_SINGLE || form > WF_RUNTIME_CORRECTED || diffuse_group < 0 || !hi || !bias_out) return JG_ERR_ARG;
    if ((keep_lo != 0) != (lo != nullptr) || (consumer && !(ln_gamma && ln_beta)) || consumer != (c1h != nullptr) || consumer != (c1f != nullptr))
        return JG_ERR_ARG;
    const bool keeps32 = device32 != 0 || form == WF_BIAS_CORRECTED;
    if (keeps32 != (w32 != nullptr) || keeps32 != (b32 != nullptr)) return JG_ERR_ARG;
    std::vector<float> wv(w, w + (size_t)N * K), bv(bias, bias + N);
    if (consumer) fold_ln_consumer(wv.data(), bv.data(), N, K, ln_gamma, ln_beta);
    if (add_beta) fold_ln_producer(bv.data(), N, add_beta);
    const RoundRule rule = {bf16 != 0, (WeightForm)form, keep_lo != 0, diffuse_group};
    const PackedLayer p = pack_layer(wv.data(), bv.data(), N, K, rule, false, consumer, device32 != 0);
    std::memcpy(hi, p.hi.data(), p.hi.size() * 2);
    if (lo) std::memcpy(lo, p.lo.data(), p.lo.size() * 2);
    std::memcpy(bias_out, p.bias.data(), (size_t)N * sizeof(float));
    if (consumer) {
        std::memcpy(c1h, p.c1h.data(), (size_t)N * sizeof(float));
        std::memcpy(c1f, p.c1f.data(), (size_t)N * sizeof(float));
    }
    if (keeps32) {
        std::memcpy(w32, p.w32.data(), p.w32.size() * sizeof(float));
        std::memcpy(b32, p.b32.data(), (size_t)N * sizeof(float));
    }
    return JG_OK;
}

int jg_debug_conv1_panel(const uint16_t* hi, const float* shift, uint16_t* panel) {
    if (!hi || !shift || !panel) return JG_ERR_ARG;
    const std::vector<uint16_t> wd = conv1_direct_panel(hi, shift);
    std::memcpy(panel, wd.data(), wd.size() * 2);
    return JG_OK;
}

int jg_debug_bias_correction(const float* w32, const float* b32, const float* mu, int64_t rows, int N, int K, float* bias) {
    if (!w32 || !b32 || !mu || rows <= 0 || N <= 0 || K <= 0 || !bias) return JG_ERR_ARG;
    bias_correction(w32, b32, mu, (long)rows, N, K, bias);
    return JG_OK;
}

int jg_debug_gemm32(jg_handle* h, const float* A, int64_t lda, const float* W, int64_t ldw, int M, int N, int K, const float* scale,
                    const float* bias, const float* res, int64_t ldr, int res_mod, int act, float* out, int64_t ldc) {
    ENTER_CHECK(h);
    if (!A || !W || !out || M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || (res && (ldr < N || res_mod < 0)) || act < 0 || act > 2)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_gemm32: bad arguments");
    Gemm32Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
    a.scale = scale; a.bias = bias; a.res = res; a.ldr = ldr; a.res_mod = res_mod; a.out = out; a.ldc = ldc; a.act = act;
    return check_result(h, launch_gemm32(a, h->stream), "launch_gemm32");
}

// The conv form of launch_gemm32 (the fp32 implicit GEMM of the audit mode; tests/test_gpu_audit32_fp64.py).  C is any power of two >= 1 --
// the launcher's own rule, so another C comes back through check_result; everything else that could leave the caller's buffers is refused here.
int jg_debug_conv32(jg_handle* h, const float* in, int nimg, int H, int W, int C, int KH, int KW, int SH, int SW, int PH, int PW, int reorder,
                    const float* Wt, int64_t ldw, int N, const float* scale, const float* bias, int act, float* out, int64_t ldc) {
    ENTER_CHECK(h);
    if (!in || !Wt || !out || nimg <= 0 || H <= 0 || W <= 0 || C <= 0 || KH <= 0 || KW <= 0 || KH > 15 || KW > 15 || SH <= 0 || SW <= 0 || PH < 0 ||
        PW < 0 || H + 2 * PH < KH || W + 2 * PW < KW || N <= 0 || (long)KH * KW * C >= (1L << 31) || ldw < (long)KH * KW * C || ldc < N || act < 0 ||
        act > 2)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv32: bad arguments (KH, KW <= 15, the kernel inside the padded image, ldw >= KH KW C, ldc >= N, act 0..2)");
    const ConvGeom g = geom(H, W, C, KH, KW, SH, SW, PH, PW, reorder != 0);
    const long M = (long)nimg * g.OH * g.OW;
    if (M >= (1L << 31)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_conv32: too many output pixels");
    Gemm32Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = in; a.g = g; a.conv = 1; a.W = Wt; a.ldw = ldw; a.M = (int)M; a.N = N; a.K = KH * KW * C;
    a.scale = scale; a.bias = bias; a.out = out; a.ldc = ldc; a.act = act;
    return check_result(h, launch_gemm32(a, h->stream), "launch_gemm32");
}

int jg_debug_gemm_x3(jg_handle* h, const float* A, int64_t lda, const void* Wh, const void* Wl, int64_t ldw, int M, int N, int K,
                     const float* bias, const float* res, int64_t ldr, int res_mod, int relu, float* out, int64_t ldc) {
    ENTER_CHECK(h);
    if (!A || !Wh || !Wl || !out || M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || (res && (ldr < N || res_mod < 0)) ||
        relu < 0 || relu > 1)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_gemm_x3: bad arguments");
    GemmX3Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.Wh = static_cast<const f16*>(Wh); a.Wl = static_cast<const f16*>(Wl); a.ldw = ldw; a.M = M; a.N = N; a.K = K;
    a.bias = bias; a.res = res; a.ldr = ldr; a.res_mod = res_mod; a.out = out; a.ldc = ldc; a.relu = relu;
    return check_result(h, launch_gemm_x3(a, h->stream), "launch_gemm_x3");
}

int jg_debug_attention(jg_handle* h, const void* qkv, const float* keymask, int B, int S, int H, int dk, void* out) {
    ENTER_CHECK(h);
    if (!qkv || !out || B <= 0 || S <= 0 || H <= 0 || (dk != 64 && dk != 96)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_attention: bad arguments");
    return check_result(h, LAUNCH(h, launch_attention, static_cast<const f16*>(qkv), keymask, B, S, H, dk, static_cast<f16*>(out), h->opts, h->stream),
                        "launch_attention");
}

int jg_debug_attention_gather(jg_handle* h, const void* qkv_pos, const void* pe_qkv, int Twin, int P, int shift, int B, int S, int H, void* out) {
    ENTER_CHECK(h);
    if (!qkv_pos || !pe_qkv || !out || B <= 0 || S <= 0 || H <= 0 || Twin <= 0 || P <= 0 || B % Twin)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_attention_gather: bad arguments (B must be a multiple of Twin)");
    if (h->bf16) JG_FAIL(h, JG_ERR_STATE, "jg_debug_attention_gather: the gather form is an fp16-build kernel (the clip path's layer 0)");
    const AttnGather g{static_cast<const f16*>(pe_qkv), Twin, P, shift};
    return check_result(h, launch_attention_gather(static_cast<const f16*>(qkv_pos), g, B, S, H, static_cast<f16*>(out), h->stream),
                        "launch_attention_gather");
}

int jg_debug_attention32(jg_handle* h, const float* qkv, const float* keymask, int B, int S, int H, int dk, float* out) {
    ENTER_CHECK(h);
    if (!qkv || !out || B <= 0 || S <= 0 || H <= 0) JG_FAIL(h, JG_ERR_ARG, "jg_debug_attention32: bad arguments");
    return check_result(h, launch_attention32(qkv, keymask, B, S, H, dk, out, h->stream), "launch_attention32");
}

// ---- the element-wise and reduction launchers (elementwise.hip, elementwise_f32.hip, elementwise_fp16.hip; tests/test_gpu_elementwise_fp64.py).
// Each check point refuses up front whatever could make its kernel touch memory outside the caller's buffers (null pointers, sizes <= 0,
// a leading dimension below the row, a pointer or stride that breaks the kernel's 16-byte accesses, a `valid` array of the wrong
// length); the shape rules the launcher itself carries come back through check_result.  Nothing is enqueued in either case.
int jg_debug_stack_frames(jg_handle* h, const void* src, int src_is_u8, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int64_t src_elems,
                          int B, int T, int pad, int H, int W, void* dst) {
    ENTER_CHECK(h);
    if (!src || !dst || B <= 0 || T <= 0 || H <= 0 || W <= 0 || pad < 0 || T + 2 * pad < 5 || sb < 0 || st < 0 || sh < 0 || sw < 0 || sc < 0 ||
        (src_is_u8 != 0 && src_is_u8 != 1) || !al(dst, 16) || (!src_is_u8 && !al(src, 4)) ||
        (B - 1) * sb + (T - 1) * st + (H - 1) * sh + (W - 1) * sw + 2 * sc >= src_elems)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_stack_frames: bad arguments (T + 2 pad >= 5, strides >= 0 and inside src_elems, dst 16-byte aligned)");
    return check_result(h, LAUNCH(h, launch_stack_frames, src, src_is_u8, (long)sb, (long)st, (long)sh, (long)sw, (long)sc, B, T, pad, H, W,
                                  static_cast<f16*>(dst), h->stream), "launch_stack_frames");
}

int jg_debug_window_gather(jg_handle* h, const float* conv, const float* pe, int B, int P, int Twin, int L, int D, int shift, int tiled, float* x32,
                           void* x16) {
    ENTER_CHECK(h);
    if (!conv || !pe || B <= 0 || D <= 0 || shift < 0 || (tiled ? !x16 : !x32) || !al(conv, 16) || !al(pe, 16) || !al(x32, 16) || !al(x16, 8))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_window_gather: bad arguments (tiled: x16, row-major: x32; 16-byte aligned fp32 rows)");
    return check_result(h, LAUNCH(h, launch_window_gather, conv, pe, B, P, Twin, L, D, shift, tiled != 0, x32, static_cast<f16*>(x16), h->stream),
                        "launch_window_gather");
}

int jg_debug_layernorm(jg_handle* h, const float* in, const float* w, const float* b, int rows, int D, int flavour, int relu, float* out32, void* out16) {
    ENTER_CHECK(h);
    if (!in || !w || !b || rows <= 0 || D <= 0 || (!out32 && !out16) || (flavour != LN_STD && flavour != LN_ANNOTATED) || relu < 0 || relu > 1 ||
        !al(in, 16) || !al(w, 16) || !al(b, 16) || !al(out32, 16) || !al(out16, 8))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_layernorm: bad arguments (flavour 0 / 1, relu 0 / 1, out32 and / or out16, 16-byte aligned rows)");
    return check_result(h, LAUNCH(h, launch_layernorm, in, w, b, rows, D, flavour, relu, out32, static_cast<f16*>(out16), h->stream), "launch_layernorm");
}

int jg_debug_layernorm_planes(jg_handle* h, const void* hi, const void* lo, const float* w, const float* b, int rows, int D, float* out32) {
    ENTER_CHECK(h);
    if (!hi || !lo || !w || !b || !out32 || rows <= 0 || D <= 0 || !al(hi, 8) || !al(lo, 8) || !al(w, 16) || !al(b, 16) || !al(out32, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_layernorm_planes: bad arguments");
    return check_result(h, LAUNCH(h, launch_layernorm_planes, static_cast<const f16*>(hi), static_cast<const f16*>(lo), w, b, rows, D, out32, h->stream),
                        "launch_layernorm_planes");
}

int jg_debug_group_mean(jg_handle* h, const void* in, int groups, int L, int D, void* out) {
    ENTER_CHECK(h);
    if (!in || !out || groups <= 0 || D <= 0 || !al(in, 16) || !al(out, 16)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_group_mean: bad arguments");
    return check_result(h, LAUNCH(h, launch_group_mean, static_cast<const f16*>(in), groups, L, D, static_cast<f16*>(out), h->stream), "launch_group_mean");
}

int jg_debug_cast(jg_handle* h, const float* in, void* out, int64_t n) {
    ENTER_CHECK(h);
    if (!in || !out || n <= 0 || !al(in, 16) || !al(out, 8)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_cast: bad arguments");
    return check_result(h, LAUNCH(h, launch_cast_f32_f16, in, static_cast<f16*>(out), (long)n, h->stream), "launch_cast_f32_f16");
}

int jg_debug_audio_conv0(jg_handle* h, const float* mel, int B, int Tm, int F, const void* wh, const void* wl, const float* bias, void* out,
                         const int32_t* valid_host, int n_valid) {
    ENTER_CHECK(h);
    if (!mel || !wh || !bias || !out || B <= 0 || Tm <= 0 || F <= 0 || !al(out, 16) || (valid_host ? n_valid != B : n_valid != 0))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_audio_conv0: bad arguments (valid_host: one entry per clip)");
    if (F > 80) JG_FAIL(h, JG_ERR_ARG, "launch_audio_conv0: the launcher rejects this shape / argument set");      // before the upload: nothing enqueued
    int32_t* valid = nullptr;
    if (valid_host) RET(upload_valid(h, valid_host, B, &valid));
    return check_result(h, LAUNCH(h, launch_audio_conv0, mel, B, Tm, F, static_cast<const f16*>(wh), static_cast<const f16*>(wl), bias,
                                  static_cast<f16*>(out), static_cast<const int*>(valid), h->stream), "launch_audio_conv0");
}

int jg_debug_zero_tail(jg_handle* h, void* x, const int32_t* valid_host, int n_valid, int halvings, int B, int H, int64_t row_elems) {
    ENTER_CHECK(h);
    if (!x || !valid_host || B <= 0 || H <= 0 || n_valid != B || halvings < 0 || halvings > 30 || row_elems <= 0 || !al(x, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_zero_tail: bad arguments (valid_host: one entry per clip)");
    if (row_elems % 8) JG_FAIL(h, JG_ERR_ARG, "launch_zero_tail: the launcher rejects this shape / argument set");     // before the upload: nothing enqueued
    int32_t* valid;
    RET(upload_valid(h, valid_host, B, &valid));
    return check_result(h, LAUNCH(h, launch_zero_tail, static_cast<f16*>(x), static_cast<const int*>(valid), halvings, B, H, (long)row_elems, h->stream),
                        "launch_zero_tail");
}

// ---- the fp32 clones of the audit mode (audit32.hip; tests/test_gpu_audit32_fp64.py): the 16-bit entries' arguments and refusals, with the
// 16-byte rules of the fp32 kernels (C % 4, D % 4, row_elems % 4) refused up front as well
int jg_debug_stack_frames32(jg_handle* h, const void* src, int src_is_u8, int64_t sb, int64_t st, int64_t sh, int64_t sw, int64_t sc, int64_t src_elems,
                            int B, int T, int pad, int H, int W, float* dst) {
    ENTER_CHECK(h);
    if (!src || !dst || B <= 0 || T <= 0 || H <= 0 || W <= 0 || pad < 0 || T + 2 * pad < 5 || sb < 0 || st < 0 || sh < 0 || sw < 0 || sc < 0 ||
        (src_is_u8 != 0 && src_is_u8 != 1) || !al(dst, 16) || (!src_is_u8 && !al(src, 4)) ||
        (B - 1) * sb + (T - 1) * st + (H - 1) * sh + (W - 1) * sw + 2 * sc >= src_elems)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_stack_frames32: bad arguments (T + 2 pad >= 5, strides >= 0 and inside src_elems, dst 16-byte aligned)");
    return check_result(h, launch_stack_frames32(src, src_is_u8, (long)sb, (long)st, (long)sh, (long)sw, (long)sc, B, T, pad, H, W, dst, h->stream),
                        "launch_stack_frames32");
}

int jg_debug_maxpool32(jg_handle* h, const float* in, int nimg, int H, int W, int C, float* out) {
    ENTER_CHECK(h);
    if (!in || !out || nimg <= 0 || H < 3 || W < 3 || C <= 0 || C % 4 || !al(in, 16) || !al(out, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_maxpool32: bad arguments (C %% 4 == 0, H, W >= 3, 16-byte aligned images)");
    return check_result(h, launch_maxpool3x3s2_32(in, out, nimg, H, W, C, h->stream), "launch_maxpool3x3s2_32");
}

int jg_debug_group_mean32(jg_handle* h, const float* in, int groups, int L, int D, float* out) {
    ENTER_CHECK(h);
    if (!in || !out || groups <= 0 || L <= 0 || D <= 0 || D % 4 || !al(in, 16) || !al(out, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_group_mean32: bad arguments (L > 0, D %% 4 == 0, 16-byte aligned rows)");
    return check_result(h, launch_group_mean32(in, groups, L, D, out, h->stream), "launch_group_mean32");
}

int jg_debug_zero_tail32(jg_handle* h, float* x, const int32_t* valid_host, int n_valid, int halvings, int B, int H, int64_t row_elems) {
    ENTER_CHECK(h);
    if (!x || !valid_host || B <= 0 || H <= 0 || n_valid != B || halvings < 0 || halvings > 30 || row_elems <= 0 || row_elems % 4 || !al(x, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_zero_tail32: bad arguments (valid_host: one entry per clip; row_elems %% 4 == 0)");
    int32_t* valid;
    RET(upload_valid(h, valid_host, B, &valid));
    return check_result(h, launch_zero_tail32(x, static_cast<const int*>(valid), halvings, B, H, (long)row_elems, h->stream), "launch_zero_tail32");
}

int jg_debug_xlmr_embed(jg_handle* h, const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word, const float* pos,
                        const float* type, float* out) {
    ENTER_CHECK(h);
    if (!ids || !word || !pos || !type || !out || B <= 0 || L <= 0 || D <= 0 || vocab <= 0 || maxpos <= 0 || pad_id < 0 || pad_id >= maxpos ||
        !al(word, 16) || !al(pos, 16) || !al(type, 16) || !al(out, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_xlmr_embed: bad arguments (0 <= pad_id < maxpos)");
    return check_result(h, launch_xlmr_embed(ids, B, L, D, pad_id, vocab, maxpos, word, pos, type, out, h->stream), "launch_xlmr_embed");
}

int jg_debug_xlmr_embed_planes(jg_handle* h, const int32_t* ids, int B, int L, int D, int pad_id, int vocab, int maxpos, const float* word,
                               const float* pos, const float* type, void* hi, void* lo, float* part) {
    ENTER_CHECK(h);
    if (!ids || !word || !pos || !type || !hi || !lo || !part || B <= 0 || L <= 0 || D <= 0 || vocab <= 0 || maxpos <= 0 || pad_id < 0 || pad_id >= maxpos ||
        !al(word, 16) || !al(pos, 16) || !al(type, 16) || !al(hi, 8) || !al(lo, 8) || !al(part, 8))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_xlmr_embed_planes: bad arguments (0 <= pad_id < maxpos)");
    return check_result(h, LAUNCH(h, launch_xlmr_embed_planes, ids, B, L, D, pad_id, vocab, maxpos, word, pos, type, static_cast<f16*>(hi),
                                  static_cast<f16*>(lo), part, h->stream), "launch_xlmr_embed_planes");
}

int jg_debug_ln_stats(jg_handle* h, const float* part, int rows, int P, float* stats) {
    ENTER_CHECK(h);
    if (!part || !stats || rows <= 0 || P <= 0 || !al(part, 8) || !al(stats, 8)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_ln_stats: bad arguments");
    return check_result(h, launch_ln_stats(part, rows, P, stats, h->stream), "launch_ln_stats");
}

int jg_debug_mask_i32_f32(jg_handle* h, const int32_t* in, float* out, int64_t n) {
    ENTER_CHECK(h);
    if (!in || !out || n <= 0) JG_FAIL(h, JG_ERR_ARG, "jg_debug_mask_i32_f32: bad arguments");
    return check_result(h, launch_mask_i32_f32(in, out, (long)n, h->stream), "launch_mask_i32_f32");
}

int jg_debug_transpose_tokens(jg_handle* h, const float* in, int N, int L, int D, float* out) {
    ENTER_CHECK(h);
    if (!in || !out || N <= 0 || L <= 0 || D <= 0 || N > 65535 || (L + 31) / 32 > 65535)
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_transpose_tokens: bad arguments (N and L / 32 are grid dimensions: <= 65535)");
    return check_result(h, launch_transpose_tokens(in, N, L, D, out, h->stream), "launch_transpose_tokens");
}

int jg_debug_pe_project(jg_handle* h, const float* pe, int S, const void* Wh, const void* Wl, const float* bias, int N, int K, void* out) {
    ENTER_CHECK(h);
    if (!pe || !Wh || !out || S <= 0 || N <= 0 || K <= 0 || (long)S * N >= (1L << 31)) JG_FAIL(h, JG_ERR_ARG, "jg_debug_pe_project: bad arguments");
    FP16_ONLY(h, "jg_debug_pe_project");
    return check_result(h, launch_pe_project(pe, S, static_cast<const f16*>(Wh), static_cast<const f16*>(Wl), bias, N, K, static_cast<f16*>(out), h->stream),
                        "launch_pe_project");
}

int jg_debug_broadcast_channels(jg_handle* h, const void* v, int C, void* out, int64_t pixels) {
    ENTER_CHECK(h);
    if (!v || !out || C <= 0 || pixels <= 0) JG_FAIL(h, JG_ERR_ARG, "jg_debug_broadcast_channels: bad arguments");
    FP16_ONLY(h, "jg_debug_broadcast_channels");
    return check_result(h, launch_broadcast_channels(static_cast<const f16*>(v), C, static_cast<f16*>(out), (long)pixels, h->stream),
                        "launch_broadcast_channels");
}

int jg_debug_col_sum(jg_handle* h, const void* A, int64_t lda, int M, int K, float* scratch, int64_t scratch_elems, float* out, const float* stats) {
    ENTER_CHECK(h);
    if (!A || !scratch || !out || M <= 0 || K <= 0 || lda < K || lda % 8 || !al(A, 16) || scratch_elems < (int64_t)col_sum_scratch_elems(K))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_col_sum: bad arguments (lda >= K, lda %% 8 == 0, A 16-byte aligned, scratch of 64 K floats)");
    FP16_ONLY(h, "jg_debug_col_sum");
    return check_result(h, launch_col_sum(static_cast<const f16*>(A), (long)lda, M, K, scratch, out, h->stream, stats), "launch_col_sum");
}

int jg_debug_rc_bias(jg_handle* h, const void* A, int64_t lda, int64_t a_elems, int tiled, int nclips, int rpc, const int32_t* valid_host, int n_valid,
                     const void* lo, const float* bias, int N, int K, float* scratch, int64_t scratch_elems, float* out) {
    ENTER_CHECK(h);
    if (!A || !lo || !scratch || !out || nclips <= 0 || rpc <= 0 || N <= 0 || K <= 0 || !al(A, 16) || !al(lo, 16) || !al(scratch, 16) ||
        (valid_host ? n_valid != nclips : n_valid != 0) || (long)nclips * rpc >= (1L << 31) || scratch_elems < (int64_t)rc_scratch_elems(nclips, K))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_rc_bias: bad arguments (valid_host: one entry per clip; scratch of nclips K floats)");
    const long rows = (long)nclips * rpc;
    if (tiled ? (long)pad128(rows) * K > a_elems : (lda < K || lda % 8 || (rows - 1) * lda + K > a_elems))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_rc_bias: A too small for nclips rpc rows (tiled: whole 128-row tiles), or lda < K / lda %% 8 != 0");
    FP16_ONLY(h, "jg_debug_rc_bias");
    if (!rc_bias_ok(N, K, tiled)) JG_FAIL(h, JG_ERR_ARG, "launch_rc_bias: the launcher rejects this shape / argument set");      // before the upload: nothing enqueued
    int32_t* valid = nullptr;
    if (valid_host) RET(upload_valid(h, valid_host, nclips, &valid));
    return check_result(h, launch_rc_bias(static_cast<const f16*>(A), (long)lda, tiled, nclips, rpc, static_cast<const int*>(valid),
                                          static_cast<const f16*>(lo), bias, N, K, scratch, out, h->stream), "launch_rc_bias");
}

int jg_debug_span_gather(jg_handle* h, const float* p32, const float* pe, const int32_t* table_dev, int n_windows, int span_max, int D, float* x32,
                         float* mask) {
    ENTER_CHECK(h);
    if (!p32 || !pe || !table_dev || !x32 || !mask || n_windows < 1 || span_max < 1 || span_max > TRACK_SPAN_MAX || D <= 0 || !al(p32, 16) ||
        !al(pe, 16) || !al(table_dev, 16) || !al(x32, 16) || !al(mask, 4))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_span_gather: bad arguments (span_max 1..%d, 16-byte aligned fp32 rows and table)", TRACK_SPAN_MAX);
    return check_result(h, launch_span_gather(p32, pe, table_dev, n_windows, span_max, D, x32, mask, h->stream), "launch_span_gather");
}

int jg_debug_core_compact(jg_handle* h, const void* in, int elem_bytes, const int32_t* table_dev, int n_windows, int span_max, int D, void* out) {
    ENTER_CHECK(h);
    if (!in || !table_dev || !out || n_windows < 1 || span_max < 1 || D <= 0 || D % 4 || !al(in, 16) || !al(table_dev, 16) || !al(out, 16))
        JG_FAIL(h, JG_ERR_ARG, "jg_debug_core_compact: bad arguments (D %% 4 == 0, 16-byte aligned rows and table)");
    return check_result(h, launch_core_compact(in, elem_bytes, table_dev, n_windows, span_max, D, out, h->stream), "launch_core_compact");
}

int jg_debug_search_plan(int n_queries, int n_gallery, int k, int num_cu, int slices_in, int* slices, int* rows_per_slice, int64_t* ws_bytes) {
    SimSearchPlan p;
    if (!slices || !rows_per_slice || !ws_bytes || !sim_search_plan(n_queries, n_gallery, k, num_cu, slices_in, p)) return JG_ERR_ARG;
    *slices = p.slices;
    *rows_per_slice = p.slice_rows;
    *ws_bytes = p.ws_bytes;
    return JG_OK;
}

int jg_debug_coupling_plan(const int32_t* w_offsets_host, int n_queries, int n_gallery, int k, int num_cu, int slices_in, int32_t* tile_first_query,
                           int* n_tiles, int* slices, int* rows_per_slice, int64_t* ws_bytes) {
    CouplingPlan p;
    if (!n_tiles || !slices || !rows_per_slice || !ws_bytes ||
        !sim_coupling_plan(w_offsets_host, n_queries, n_gallery, k, num_cu, slices_in, tile_first_query, p))
        return JG_ERR_ARG;
    *n_tiles = p.n_tiles;
    *slices = p.cut.slices;
    *rows_per_slice = p.cut.slice_rows;
    *ws_bytes = p.cut.ws_bytes;
    return JG_OK;
}

int jg_debug_last_kernel(jg_handle* h, char* buf, int len) {
    if (!h || !buf || len <= 0) return JG_ERR_ARG;
    snprintf(buf, (size_t)len, "%s", h->kname);
    return JG_OK;
}

}  // extern "C"
