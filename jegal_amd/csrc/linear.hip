// libjegal_hip: weight packing, the host side of every GEMM call, bias corrections and the calibration passes.  Host code only.
#include "engine.h"

namespace engine {

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

// The one upload step: everything device-side of a packed layer -- its allocations and copies into model `m`, the Lin, and the
// calibration record of a bias-corrected layer, which takes the fp32 copies
int upload_layer(jg_handle* h, Model& m, PackedLayer&& p, Lin* L) {
    L->N = p.N; L->K = p.K;
    L->c1h = L->c1f = nullptr;
    if (!p.c1h.empty()) {
        RET(upload(h, m, p.c1h, &L->c1h));
        RET(upload(h, m, p.c1f, &L->c1f));
    }
    RET(upload(h, m, p.hi, &L->wh));
    RET(upload(h, m, p.bias, &L->bias));
    L->w32d = L->b32d = nullptr;
    if (p.device32) {
        RET(upload(h, m, p.w32, &L->w32d));
        RET(upload(h, m, p.b32, &L->b32d));
    }
    L->lo = nullptr;
    if (!p.lo.empty()) RET(upload(h, m, p.lo, &L->lo));       // for the form's own GEMMs and / or the split-operand kernel (gemm_x3, keep32)
    L->form = p.form;
    L->uncalibrated = p.uncalibrated;
    L->cal = nullptr;
    if (p.form == WF_BIAS_CORRECTED) {
        float* mu;
        RET(walloc<float>(h, m, (size_t)p.K, &mu));
        m.bc.push_back({L, mu, 0, std::move(p.w32), std::move(p.b32)});
        L->cal = &m.bc.back();
    }
    return JG_OK;
}

// The handle's policy for one matrix as plain values (weight_form.h, the options), then the arithmetic (weight_pack.h).
// keep32: the layer also runs on the fp32 kernel in the fp16 modes (the two ends of the JEGAL gesture branch, option jegal_fp32_ends)
static PackedLayer pack_host(const jg_handle* h, int model_id, const float* w, const float* bias, int N, int K, int kind, bool ln_consumer, bool keep32,
                             int diffuse_group) {
    const WeightForm form = weight_form(h->precision, kind, model_id);
    const RoundRule rule = {h->bf16, form, lo_kept(form, keep32), diffuse_group};
    return pack_layer(w, bias, N, K, rule, starts_uncalibrated(form, kind), ln_consumer, h->audit_weights || h->precision == JG_PREC_FP32 || keep32);
}

// [N][K] fp32 -> device 16-bit hi (+lo), allocated into model `m`
int pack_matrix(jg_handle* h, Model& m, const std::vector<float>& w, const std::vector<float>& bias, int N, int K, int kind, Lin* L, bool ln_consumer,
                bool keep32) {
    return upload_layer(h, m, pack_host(h, m.id, w.data(), bias.data(), N, K, kind, ln_consumer, keep32, 0), L);
}

int make_linear(jg_handle* h, Model& m, const std::string& wname, const std::string& bname, int N, int K, Lin* L, int kind, bool keep32) {
    const HostTensor *w, *b;
    RET(need(h, wname, (int64_t)N * K, &w));
    RET(need(h, bname, N, &b));
    return pack_matrix(h, m, w->v, b->v, N, K, kind, L, false, keep32);
}

int make_ln(jg_handle* h, Model& m, const std::string& wname, const std::string& bname, int D, LNp* p) {
    const HostTensor *w, *b;
    RET(need(h, wname, D, &w));
    RET(need(h, bname, D, &b));
    RET(upload(h, m, w->v, &p->w));
    RET(upload(h, m, b->v, &p->b));
    return JG_OK;
}

// conv weight [O][I][KT][KH][KW] (+ optional eval BatchNorm `bn`, "" for none) -> the folded matrix [N][K] and shift [N] (conv_matrix,
// weight_pack.h)
int fold_conv(jg_handle* h, const std::string& conv, const std::string& bn, const ConvPack& c, std::vector<float>* p, std::vector<float>* shift) {
    const HostTensor *w, *b;
    RET(need(h, conv + ".weight", (int64_t)c.O * c.I * c.KT * c.KH * c.KW, &w));
    RET(need(h, conv + ".bias", c.O, &b));
    std::vector<float> s(c.O, 1.f);
    *shift = b->v;
    if (!bn.empty()) {
        const HostTensor *g, *be, *mu, *var;
        RET(need(h, bn + ".weight", c.O, &g));
        RET(need(h, bn + ".bias", c.O, &be));
        RET(need(h, bn + ".running_mean", c.O, &mu));
        RET(need(h, bn + ".running_var", c.O, &var));
        bn_fold(b->v.data(), g->v.data(), be->v.data(), mu->v.data(), var->v.data(), c.O, s.data(), shift->data());
    }
    shift->resize(conv_pack_N(c), 0.f);
    *p = conv_matrix(w->v.data(), s.data(), c);
    return JG_OK;
}

int pack_conv(jg_handle* h, int model_id, const std::string& conv, const std::string& bn, const ConvPack& c, int kind, PackedLayer* out) {
    std::vector<float> p, shift;
    RET(fold_conv(h, conv, bn, c, &p, &shift));
    *out = pack_host(h, model_id, p.data(), shift.data(), conv_pack_N(c), conv_pack_K(c), kind, false, false, h->conv_round_diffuse ? c.slot : 0);
    return JG_OK;
}

int make_conv(jg_handle* h, Model& m, const std::string& conv, const std::string& bn, int O, int I, int KT, int KH, int KW,
              int slot, int kpad, Lin* L, int SH, int SW, bool reorder, int Opad, int kind) {
    PackedLayer p;
    RET(pack_conv(h, m.id, conv, bn, {O, I, KT, KH, KW, slot, kpad, Opad, SH, SW, reorder}, kind, &p));
    return upload_layer(h, m, std::move(p), L);
}

int make_annotated_layer(jg_handle* h, Model& m, const std::string& p, int D, int Dff, EncLayer* L, int kind) {
    // pack linears.0/1/2 (q,k,v) into one [3D][D] projection (modules.py:108-110)
    std::vector<float> w((size_t)3 * D * D), b((size_t)3 * D);
    for (int i = 0; i < 3; ++i) {
        const HostTensor *wi, *bi;
        RET(need(h, p + ".self_attn.linears." + std::to_string(i) + ".weight", (int64_t)D * D, &wi));
        RET(need(h, p + ".self_attn.linears." + std::to_string(i) + ".bias", D, &bi));
        std::memcpy(&w[(size_t)i * D * D], wi->v.data(), sizeof(float) * D * D);
        std::memcpy(&b[(size_t)i * D], bi->v.data(), sizeof(float) * D);
    }
    RET(pack_matrix(h, m, w, b, 3 * D, D, kind, &L->qkv));
    RET(make_linear(h, m, p + ".self_attn.linears.3.weight", p + ".self_attn.linears.3.bias", D, D, &L->out, kind));
    RET(make_linear(h, m, p + ".feed_forward.w_1.weight", p + ".feed_forward.w_1.bias", Dff, D, &L->ff1, kind));
    RET(make_linear(h, m, p + ".feed_forward.w_2.weight", p + ".feed_forward.w_2.bias", D, Dff, &L->ff2, kind));
    RET(make_ln(h, m, p + ".sublayer.0.norm.a_2", p + ".sublayer.0.norm.b_2", D, &L->n1));
    RET(make_ln(h, m, p + ".sublayer.1.norm.a_2", p + ".sublayer.1.norm.b_2", D, &L->n2));
    return JG_OK;
}

// ------------------------------------------------------------------------------------ GEMM calls
int gemm(jg_handle* h, int stage, const f16* A, long lda, int M, const Lin& L, const Epi& e, const ConvGeom* g) {
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda;
    if (g) a.g = *g;
    a.Wh = L.wh; a.Wl = run_lo(h, L, true); a.ldw = L.K;      // (a run-time corrected layer: the per-clip-bias form, unless that is refused below)
    const bool conv = g != nullptr;
    a.M = M; a.N = L.N; a.K = L.K;
    a.scale = e.scale; a.bias = e.no_bias ? nullptr : L.bias;
    a.res = e.res; a.ldr = e.ldr; a.res_mod = e.res_mod;
    a.out32 = e.out32; a.out16 = e.out16; a.ldc = e.ldc ? e.ldc : L.N;
    a.relu = e.relu;
    if (e.ln) { a.ln_w = e.ln->w; a.ln_b = e.ln->b; a.ln_flavour = e.ln_flavour; }
    a.res16 = e.res16; a.a_tiled = e.a_tiled;
    if (e.ln_mode == 1) {
        if (!L.c1h || !L.c1f) JG_FAIL(h, JG_ERR_STATE, "implicit LayerNorm on a layer that was not packed for it");
        a.ln_mode = 1; a.ln_stats = e.ln_stats; a.scale = L.c1h;
    } else if (e.ln_mode == 2) {
        a.ln_mode = 2; a.ln_stats = e.ln_stats; a.scale = e.ln_gamma;
        a.xres_hi = e.x_hi; a.xres_lo = e.x_lo; a.out16 = e.x_hi; a.out_lo = e.x_lo; a.stat_out = e.stat_out;
    }
    if (L.form == WF_RUNTIME_CORRECTED) {
        // run-time correction: bias_clip = bias + lo . (mean of a sample of the clip's own rows), two small launches in front of the GEMM.
        // Whether the GEMM takes the corrected form of this call (per-clip bias, single fp16 weights) is the planner's answer for that
        // form; everything else runs hi+lo.  Particular to this call site: the clips must tile the rows, the layer's bias rides in the
        // per-clip vector, and launches of fewer than 1024 rows stay hi+lo (stricter than the planner's own minimum for the two
        // non-fused GEMMs).  Decided before the scratch buffers are allocated: a refused call leaves the workspace layout alone.
        GemmShape q = gemm_shape(a, conv);
        q.bias_clip = true; q.rpc = e.rc_rpc; q.nclips = e.rc_clips;
        const bool can = !e.no_bias && (long)e.rc_rpc * e.rc_clips == M && M >= 1024 && rc_bias_ok(L.N, L.K, e.a_tiled) && plan_gemm(q, h->opts).ok();
        if (can) {
            float *scr, *bc;
            RET(wsalloc(h, rc_scratch_elems(e.rc_clips, L.K), &scr));
            RET(wsalloc(h, (size_t)e.rc_clips * L.N, &bc));
            RET(timed(h, JG_ST_GEMM, [&] { return launch_rc_bias(A, lda, e.a_tiled, e.rc_clips, e.rc_rpc, e.rc_valid, L.lo, L.bias, L.N, L.K, scr, bc, h->stream); }));
            a.bias_clip = bc; a.rpc = e.rc_rpc; a.nclips = e.rc_clips;
        } else {
            a.Wl = run_lo(h, L, false);
        }
    }
    if (a.ln_mode == 1 && a.Wl) a.scale = L.c1f;      // column sums of the weights the GEMM runs with (Lin::c1h / c1f)
    if (h->calib && L.cal && !conv) {
        // column sums ACCUMULATE in the layer's record over every call of a calibration pass (chunks of a large calibration batch, the
        // six layers' shared shapes are separate Lin objects): calibration_pass zeroes mu / mu_rows once at its start
        float* part;
        RET(wsalloc(h, col_sum_scratch_elems(L.K), &part));
        // (a folded consumer's effective input is the NORMALISED row: the correction term is (w' - fp16(w')) . E[(x - mean) rstd])
        // (padding rows behind the caller's tokens would be averaged into E[x]: ADVICE r4)
        const int rows = e.calib_rows > 0 && e.calib_rows < M ? e.calib_rows : M;
        RET(timed(h, JG_ST_MISC, [&] { return launch_col_sum(A, lda, rows, L.K, part, L.cal->mu, h->stream, e.ln_mode == 1 ? e.ln_stats : nullptr); }));
        L.cal->mu_rows += rows;
    }
    return timed(h, stage, [&] { return LAUNCH(h, launch_gemm, a, conv, h->opts, h->stream); });
}

ConvGeom geom(int H, int W, int C, int KH, int KW, int SH, int SW, int PH, int PW, bool reorder) {
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

int gemm32(jg_handle* h, int stage, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e, const ConvGeom* g) {
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

// The same product on the fp16 matrix cores with split operands (gemm_x3.h, GemmX3Args): A fp32, W = hi + lo, three MFMAs per fragment pair
int gemm_x3(jg_handle* h, int stage, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e) {
    if (!L.wh || !L.lo) JG_FAIL(h, JG_ERR_STATE, "split-operand GEMM on a layer that was packed without its lo half");
    GemmX3Args a;
    std::memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.Wh = L.wh; a.Wl = L.lo; a.ldw = L.K;
    a.M = M; a.N = L.N; a.K = L.K;
    a.bias = L.b32d ? L.b32d : L.bias;
    a.res = e.res; a.ldr = e.ldr; a.res_mod = e.res_mod;
    a.out = out; a.ldc = L.N;
    a.relu = e.act == 1;
    if (e.act > 1) JG_FAIL(h, JG_ERR_ARG, "gemm_x3: ReLU only");
    return timed(h, stage, [&] { return launch_gemm_x3(a, h->stream); });
}

// ------------------------------------------------------------------------------------ the primitives of the two arithmetics (engine.h)
static int gemm_a32(jg_handle* h, A32 ar, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e, const ConvGeom* g = nullptr) {
    if (!ar.x3) return gemm32(h, g ? JG_ST_CONV : JG_ST_GEMM, A, lda, M, L, out, e, g);
    if (g) JG_FAIL(h, JG_ERR_ARG, "gemm_x3: no convolutions");
    return gemm_x3(h, JG_ST_GEMM, A, lda, M, L, out, e);
}
int linear(jg_handle* h, A16, const f16* A, long lda, int M, const Lin& L, f16* out, int act, const ConvGeom* g) {
    Epi e; e.out16 = out; e.relu = act;
    return gemm(h, g ? JG_ST_CONV : JG_ST_GEMM, A, lda, M, L, e, g);
}
int linear(jg_handle* h, A32 ar, const float* A, long lda, int M, const Lin& L, float* out, int act, const ConvGeom* g) {
    Epi32 e; e.act = act;
    return gemm_a32(h, ar, A, lda, M, L, out, e, g);
}
int linear_to32(jg_handle* h, A16, const f16* A, long lda, int M, const Lin& L, float* out32, const float* res, long ldr, int res_mod) {
    Epi e; e.out32 = out32; e.res = res; e.ldr = ldr; e.res_mod = res_mod;
    return gemm(h, JG_ST_GEMM, A, lda, M, L, e);
}
int linear_to32(jg_handle* h, A32 ar, const float* A, long lda, int M, const Lin& L, float* out32, const float* res, long ldr, int res_mod) {
    Epi32 e; e.res = res; e.ldr = ldr; e.res_mod = res_mod;
    return gemm_a32(h, ar, A, lda, M, L, out32, e);
}
int layernorm(jg_handle* h, A16, const float* x, const LNp& ln, int M, int D, int flavour, int relu, f16* copy, float* out32) {
    return timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, x, ln.w, ln.b, M, D, flavour, relu, out32, copy, h->stream); });
}
int layernorm(jg_handle* h, A32, const float* x, const LNp& ln, int M, int D, int flavour, int relu, float* copy, float* out32) {
    return timed(h, JG_ST_NORM, [&] { return launch_layernorm(x, ln.w, ln.b, M, D, flavour, relu, out32 ? out32 : copy, nullptr, h->stream); });
}
int attention(jg_handle* h, A16, const f16* qkv, const float* mask, int B, int S, int H, int dk, f16* out) {
    return timed(h, JG_ST_ATTN, [&] { return LAUNCH(h, launch_attention, qkv, mask, B, S, H, dk, out, h->opts, h->stream); });
}
int attention(jg_handle* h, A32, const float* qkv, const float* mask, int B, int S, int H, int dk, float* out) {
    return timed(h, JG_ST_ATTN, [&] { return launch_attention32(qkv, mask, B, S, H, dk, out, h->stream); });
}
int zero_tail(jg_handle* h, A16, f16* x, const int* valid, int halvings, int B, int H, long row_elems) {
    if (!valid) return JG_OK;
    return timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_zero_tail, x, valid, halvings, B, H, row_elems, h->stream); });
}
int zero_tail(jg_handle* h, A32, float* x, const int* valid, int halvings, int B, int H, long row_elems) {
    if (!valid) return JG_OK;
    return timed(h, JG_ST_MISC, [&] { return launch_zero_tail32(x, valid, halvings, B, H, row_elems, h->stream); });
}
// 16-bit: one fused kernel straight from the mel frames, which zeroes the ragged tails itself (round 2: im2col + a K = 32 GEMM)
int audio_conv0(jg_handle* h, A16, const float* mel, int B, int Tm, int F, const Lin& L, const ConvGeom&, const int* valid, f16* out) {
    return timed(h, JG_ST_CONV, [&] { return LAUNCH(h, launch_audio_conv0, mel, B, Tm, F, L.wh, run_lo(h, L, false), L.bias, out, valid, h->stream); });
}
// fp32: the implicit-GEMM convolution, between a zero-tailed copy of a ragged batch's frames and the zero tail of its output
int audio_conv0(jg_handle* h, A32 ar, const float* mel, int B, int Tm, int F, const Lin& L, const ConvGeom& g, const int* valid, float* out) {
    if (valid) {
        float* m0;
        RET(wsalloc(h, (size_t)B * Tm * F, &m0));
        HIPCHK(h, hipMemcpyAsync(m0, mel, (size_t)B * Tm * F * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        RET(zero_tail(h, ar, m0, valid, 0, B, Tm, F));
        mel = m0;
    }
    RET(linear(h, ar, mel, 0, B * Tm * F, L, out, 1, &g));
    return zero_tail(h, ar, out, valid, 0, B, Tm, (long)F * L.N);
}
int operand(jg_handle* h, A16, const float* x, long n, const f16** out) {
    f16* x16;
    RET(wsalloc(h, (size_t)n, &x16));
    *out = x16;
    return timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_cast_f32_f16, x, x16, n, h->stream); });
}
int operand(jg_handle*, A32, const float* x, long, const float** out) { *out = x; return JG_OK; }

// ------------------------------------------------------------------------------------ bias-corrected precision
// Weight rounding (w -> fp16) leaves an error (w - fp16(w)) . x per output that is the SAME for every token,
// so it does not average out downstream; its dominant part is (w - fp16(w)) . E[x].  A calibration pass runs the
// gesture path with hi+lo weights on a small batch, records E[x] of every Linear input, and folds that term into the
// bias.  Run-time GEMMs then use single fp16 weights (half the MFMAs and LDS traffic of the hi+lo split) at the split's
// accuracy (oracle/precision_probe.py).
static int apply_bias_corrections(jg_handle* h, int models) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<float> mu;
    for (Model* m : {&h->gs.m, &h->jg.m, &h->xl.m})
        for (BiasCalib& c : m->bc) {
            Lin* L = c.layer;
            if (c.mu_rows <= 0) continue;
            if (!((models >> (m->id - 1)) & 1)) { c.mu_rows = 0; continue; }
            mu.resize(L->K);
            HIPCHK(h, hipMemcpy(mu.data(), c.mu, sizeof(float) * L->K, hipMemcpyDeviceToHost));
            std::vector<float> nb(L->N);
            bias_correction(c.w32.data(), c.b32.data(), mu.data(), c.mu_rows, L->N, L->K, nb.data());
            HIPCHK(h, hipMemcpy(L->bias, nb.data(), sizeof(float) * L->N, hipMemcpyHostToDevice));
            c.mu_rows = 0;
            L->uncalibrated = false;          // calibrated: single fp16 + corrected bias from here on
        }
    h->gs.qpe_valid = false;          // the projected positional rows carry layer 0's qkv bias
    return JG_OK;
}

// One calibration pass: zero the input means of the bias-corrected layers of `record` (a models mask), run `pass(bufs)` with hi+lo weights
// while they are recorded, fold the corrections of the layers of `apply` into their biases.  `bufs` (device buffers) are freed on every path.
template <class F>
static int calibration_pass(jg_handle* h, int record, int apply, F&& pass) {
    std::vector<void*> bufs;
    int rc = JG_OK;
    for (Model* m : {&h->gs.m, &h->jg.m, &h->xl.m}) {
        if (!((record >> (m->id - 1)) & 1)) continue;
        for (BiasCalib& c : m->bc) {
            if (hipMemsetAsync(c.mu, 0, sizeof(float) * c.layer->K, h->stream) != hipSuccess) rc = JG_ERR_HIP;
            c.mu_rows = 0;
        }
    }
    if (rc != JG_OK) h->err = "hipMemsetAsync(mu) failed";
    if (rc == JG_OK) { h->calib = true; rc = pass(bufs); h->calib = false; }
    if (rc == JG_OK) rc = apply_bias_corrections(h, apply);
    (void)hipStreamSynchronize(h->stream);
    for (void* p : bufs) (void)hipFree(p);
    return rc;
}

// frames == nullptr: built-in deterministic calibration clips (uniform u8 noise, rows 0..109 zeroed like the
// face-mask rectangle), so results do not depend on what the engine happens to see first.
// models: bit 0 GestSync, bit 1 JEGAL -- only the bias-corrected layers of these models receive new corrections (the pass
// itself always runs the whole gesture path: JEGAL's input means depend on GestSync's output)
int calibrate_gesture(jg_handle* h, const void* frames, int dtype, int B, int T, int models) {
    if (h->gs.m.bc.empty() && h->jg.m.bc.empty()) return JG_OK;
    return calibration_pass(h, 3, models, [&](std::vector<void*>& bufs) -> int {
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
            void* own = nullptr;
            HIPCHK(h, hipMalloc(&own, n));
            bufs.push_back(own);
            HIPCHK(h, hipMemcpy(own, host.data(), n, hipMemcpyHostToDevice));
            frames = own;
        }
        float *feats = nullptr, *emb = nullptr;
        HIPCHK(h, hipMalloc(&feats, (size_t)B * T * 1024 * sizeof(float)));
        bufs.push_back(feats);
        HIPCHK(h, hipMalloc(&emb, (size_t)B * T * 512 * sizeof(float)));
        bufs.push_back(emb);
        if (h->gs.m.ready) {
            RET(gestsync_clip_impl(h, frames, dtype, B, T, feats));
        } else {
            std::vector<float> hf((size_t)B * T * 1024);          // no GestSync loaded: standard-normal stand-in features
            uint32_t x = 0x2545F491u;
            for (auto& v : hf) {
                float s = 0.f;
                for (int i = 0; i < 12; ++i) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; s += (float)(x >> 8) * (1.0f / 16777216.0f); }
                v = s - 6.0f;
            }
            if (hipMemcpy(feats, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return JG_ERR_HIP;
        }
        if (!h->jg.m.ready) return JG_OK;
        RET(begin_pass(h));
        return jegal_gestures_impl(h, feats, nullptr, B, T, 1, emb);
    });
}

// Bias corrections of the XLM-RoBERTa layers (JG_PREC_FP16_BC): one pass with hi+lo weights over token ids records every Linear's
// input means; the run-time GEMMs then switch from hi+lo to single fp16 + corrected bias.  ids_dev / mask_dev (B, L): the CALLER's
// tokens (device); ids_dev == nullptr: built-in ids, uniform over the vocabulary, no padding (E[x] behind a LayerNorm is mostly
// its beta and the mean of the position / type embeddings -- true for the seeded test weights, unvalidated for the released
// checkpoint, which is why nothing calls this implicitly).
int calibrate_xlmr(jg_handle* h, const int32_t* ids_dev, const int32_t* mask_dev, int B, int L) {
    if (!h->xl.m.ready) JG_FAIL(h, JG_ERR_STATE, "XLM-RoBERTa weights not finalized");
    return calibration_pass(h, 4, 4, [&](std::vector<void*>& bufs) -> int {
        if (!ids_dev) {
            B = 8; L = 64;
            std::vector<int32_t> ids((size_t)B * L);
            uint32_t x = 0xC0FFEE11u;
            for (auto& v : ids) {
                x ^= x << 13; x ^= x >> 17; x ^= x << 5;
                v = 3 + (int32_t)(x % (uint32_t)(h->xl.vocab > 3 ? h->xl.vocab - 3 : 1));
            }
            for (int b = 0; b < B; ++b) { ids[(size_t)b * L] = 0; ids[(size_t)b * L + L - 1] = 2; }       // <s> ... </s>
            int32_t* dids = nullptr;
            HIPCHK(h, hipMalloc(&dids, ids.size() * sizeof(int32_t)));
            bufs.push_back(dids);
            if (hipMemcpy(dids, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) JG_FAIL(h, JG_ERR_HIP, "hipMemcpy failed");
            ids_dev = dids;
            mask_dev = nullptr;
        }
        float* out = nullptr;
        if (hipMalloc(&out, (size_t)B * L * 768 * sizeof(float)) != hipSuccess) JG_FAIL(h, JG_ERR_HIP, "hipMalloc failed");
        bufs.push_back(out);
        RET(begin_pass(h));
        return xlmr_encode_impl(h, ids_dev, mask_dev, B, L, out);
    });
}

}  // namespace engine
