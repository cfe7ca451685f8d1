// libjegal_hip: JEGAL -- finalize, encoders, gesture branch, audio CNN, text encoder, content fusion, fp16 and fp32 (audit) forms.  Host code only.
#include "engine.h"

namespace engine {

int finalize_jegal(jg_handle* h) {
    drop_model(h, h->jg);
    JegalModel& jg = h->jg;
    Model& m = jg.m;
    // The input projection keeps hi+lo weights in the bias-corrected mode too: the zero-padded rows of a ragged batch
    // (dataset.py:336-340) reach it as x = 0 exactly, where a bias correction (w - fp16(w)).E[x] would be pure error -- the
    // reference computes those rows as well (callers strip them).  Two small GEMMs of the 50 in the branch.
    RET(make_linear(h, m, "proj_ip_rgb.0.weight", "proj_ip_rgb.0.bias", 512, 1024, &jg.ip0, LK_CONTENT, true));
    RET(make_ln(h, m, "proj_ip_rgb.1.weight", "proj_ip_rgb.1.bias", 512, &jg.ip_ln));
    RET(make_linear(h, m, "proj_ip_rgb.3.weight", "proj_ip_rgb.3.bias", 512, 512, &jg.ip3, LK_CONTENT, true));
    const HostTensor* pe;
    RET(need(h, "position_rgb.pe", 500 * 512, &pe));
    RET(upload(h, m, pe->v, &jg.rgb_pe));
    for (int l = 0; l < 6; ++l) RET(make_annotated_layer(h, m, "encoder_rgb.layers." + std::to_string(l), 512, 2048, &jg.rgb_layers[l], LK_GESTURE));
    RET(make_ln(h, m, "encoder_rgb.norm.a_2", "encoder_rgb.norm.b_2", 512, &jg.rgb_norm));
    RET(make_linear(h, m, "proj_op_rgb.weight", "proj_op_rgb.bias", 512, 512, &jg.op_rgb, LK_GESTURE, true));
    for (int l = 0; l < 3; ++l) RET(make_annotated_layer(h, m, "encoder_text.layers." + std::to_string(l), 768, 3072, &jg.text_layers[l], LK_CONTENT));
    RET(make_ln(h, m, "encoder_text.norm.a_2", "encoder_text.norm.b_2", 768, &jg.text_norm));
    RET(make_linear(h, m, "proj_op_text.weight", "proj_op_text.bias", 256, 768, &jg.op_text, LK_CONTENT));
    RET(make_conv(h, m, "cnn.0", "cnn.1", 32, 1, 1, 5, 5, 1, 32, &jg.a0));
    RET(make_conv(h, m, "cnn.3", "cnn.4", 64, 32, 1, 3, 3, 32, 0, &jg.a3));
    RET(make_conv(h, m, "cnn.6", "cnn.7", 128, 64, 1, 3, 3, 64, 0, &jg.a6));
    RET(make_conv(h, m, "cnn.9", "cnn.10", 256, 128, 1, 3, 3, 128, 0, &jg.a9));
    RET(make_conv(h, m, "cnn.12", "cnn.13", 256, 256, 1, 3, 3, 256, 0, &jg.a12));
    RET(make_conv(h, m, "cnn.15", "", 256, 256, 1, 1, 1, 256, 0, &jg.a15));
    RET(make_linear(h, m, "proj_op_audio.weight", "proj_op_audio.bias", 256, 256, &jg.op_audio, LK_CONTENT));
    RET(make_linear(h, m, "proj_op_fusion_content.0.weight", "proj_op_fusion_content.0.bias", 512, 512, &jg.fu0, LK_CONTENT));
    RET(make_linear(h, m, "proj_op_fusion_content.2.weight", "proj_op_fusion_content.2.bias", 512, 512, &jg.fu2, LK_CONTENT));
    RET(make_linear(h, m, "proj_op_align_gesture.0.weight", "proj_op_align_gesture.0.bias", 512, 512, &jg.al_g0, LK_GESTURE, true));
    RET(make_linear(h, m, "proj_op_align_gesture.2.weight", "proj_op_align_gesture.2.bias", 512, 512, &jg.al_g2, LK_GESTURE, true));
    RET(make_linear(h, m, "proj_op_align_content.0.weight", "proj_op_align_content.0.bias", 512, 512, &jg.al_c0, LK_CONTENT));
    RET(make_linear(h, m, "proj_op_align_content.2.weight", "proj_op_align_content.2.bias", 512, 512, &jg.al_c2, LK_CONTENT));
    m.ready = true;
    return JG_OK;
}

// Option jegal_fp32_ends: these ends of a JEGAL path keep fp32 activations and run on gemm_x3 -- not in the plain-fp16
// / bf16 reported modes, not while calibrating, and only where every one of them keeps its lo half on the device (lo_kept, weight_form.h)
static bool split_ends(const jg_handle* h, std::initializer_list<const Lin*> ends) {
    if (!h->jegal_fp32_ends || h->calib || h->precision == JG_PREC_FP16 || h->precision == JG_PREC_BF16) return false;
    for (const Lin* L : ends) if (!L->lo) return false;
    return true;
}

// ------------------------------------------------------------------------------------ fp32 audit path (audit32.hip)
// ONE sub-layer of a pre-norm encoder layer on the fp32 kernels, in place on the fp32 residual stream (which = 1: x += out(attn(qkv(LN1 x))),
// 2: x += ff2(relu(ff1(LN2 x)))); scratch: M * (D + 3 D + D + Dff) floats.  (annotated_encoder32, and annotated_encoder's `parts`.)
static int encoder_sublayers32(jg_handle* h, const EncLayer& L, int which, float* x32, float* scratch, const float* mask, int B, int S, int D, int Dff) {
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

// pre-norm encoder (modules.py:11-59) in place on x32; the final norm's output goes to n32
static int annotated_encoder32(jg_handle* h, const EncLayer* layers, int nl, const LNp& fin, float* x32, float* n32, const float* mask, int B, int S,
                               int D, int Dff) {
    const int M = B * S;
    float* scr;
    RET(wsalloc(h, (size_t)M * (D + 3 * D + D + Dff), &scr));
    for (int l = 0; l < nl; ++l) {
        RET(encoder_sublayers32(h, layers[l], 1, x32, scr, mask, B, S, D, Dff));
        RET(encoder_sublayers32(h, layers[l], 2, x32, scr, mask, B, S, D, Dff));
    }
    return timed(h, JG_ST_NORM, [&] { return launch_layernorm(x32, fin.w, fin.b, M, D, LN_ANNOTATED, 0, n32, nullptr, h->stream); });
}

// a GEMM on fp32 activations: the fp32 MFMA (audit) or, x3, the split operands on the fp16 matrix cores (gemm_x3: the fp16 modes' ends)
static int gemm_f32(jg_handle* h, bool x3, const float* A, long lda, int M, const Lin& L, float* out, const Epi32& e = Epi32()) {
    return x3 ? gemm_x3(h, JG_ST_GEMM, A, lda, M, L, out, e) : gemm32(h, JG_ST_GEMM, A, lda, M, L, out, e);
}

// proj_ip_rgb + positional rows (jegal.py:25-28,84-85) on the fp32 kernels: feats (M,1024) -> x32 (M,512); t32: (M,512) scratch
// x3: on the fp16 matrix cores with split operands (gemm_x3: the fp16 modes' production path) instead of the fp32 MFMA (audit)
static int jegal_input32(jg_handle* h, const float* feats, int M, int T, float* t32, float* x32, bool x3) {
    const JegalModel& jg = h->jg;
    float* t2;
    RET(wsalloc(h, (size_t)M * 512, &t2));
    RET(gemm_f32(h, x3, feats, 1024, M, jg.ip0, t32));
    RET(timed(h, JG_ST_NORM, [&] { return launch_layernorm(t32, jg.ip_ln.w, jg.ip_ln.b, M, 512, LN_STD, 1, t2, nullptr, h->stream); }));
    Epi32 p; p.res = jg.rgb_pe; p.ldr = 512; p.res_mod = T;
    return gemm_f32(h, x3, t2, 512, M, jg.ip3, x32, p);
}

// proj_op_rgb (+ proj_op_align_gesture) on the fp32 kernels from the final norm's fp32 output
static int jegal_tail32(jg_handle* h, const float* n32, int M, int align, float* out, bool x3) {
    const JegalModel& jg = h->jg;
    if (!align) return gemm_f32(h, x3, n32, 512, M, jg.op_rgb, out);
    float *g32, *a32;
    RET(wsalloc(h, (size_t)M * 512, &g32));
    RET(wsalloc(h, (size_t)M * 512, &a32));
    RET(gemm_f32(h, x3, n32, 512, M, jg.op_rgb, g32));
    Epi32 f; f.act = 1;
    RET(gemm_f32(h, x3, g32, 512, M, jg.al_g0, a32, f));
    return gemm_f32(h, x3, a32, 512, M, jg.al_g2, out);
}

static int jegal_gestures_impl32(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out) {
    const int M = B * T;
    float *t32, *x32, *n32;
    RET(wsalloc(h, (size_t)M * 512, &t32));
    RET(wsalloc(h, (size_t)M * 512, &x32));
    RET(wsalloc(h, (size_t)M * 512, &n32));
    RET(jegal_input32(h, feats, M, T, t32, x32, false));
    RET(annotated_encoder32(h, h->jg.rgb_layers, 6, h->jg.rgb_norm, x32, n32, mask, B, T, 512, 2048));
    return jegal_tail32(h, n32, M, align, out, false);
}

// The audio CNN of a batch: geometry of cnn.0 .. cnn.15 and the per-clip lengths.  valid_host (optional, host [B]): clip b holds
// valid_host[b] mel frames; a ragged batch gets them on the device in `valid` (nullptr when every clip fills its Tm rows).
struct AudioGeom { ConvGeom g0, g3, g6, g9, g12, g15; int* valid = nullptr; };
static int audio_setup(jg_handle* h, int B, int Tm, const int32_t* valid_host, AudioGeom* a) {
    const int F = 80;
    a->g0 = geom(Tm, F, 1, 5, 5, 1, 1, 2, 2);
    a->g3 = geom(Tm, F, 32, 3, 3, 2, 2, 1, 1);
    a->g6 = geom(a->g3.OH, a->g3.OW, 64, 3, 3, 2, 2, 1, 1);
    a->g9 = geom(a->g6.OH, a->g6.OW, 128, 3, 3, 1, 3, 1, 1);
    a->g12 = geom(a->g9.OH, a->g9.OW, 256, 3, 3, 1, 3, 1, 1);
    a->g15 = geom(a->g12.OH, a->g12.OW, 256, 1, 1, 1, 3, 0, 0);
    if (a->g15.OW != 1) JG_FAIL(h, JG_ERR_ARG, "audio CNN must reduce 80 mel bands to 1");
    a->valid = nullptr;
    if (!valid_host) return JG_OK;
    bool ragged = false;
    for (int b = 0; b < B; ++b) {
        if (valid_host[b] < 4 || valid_host[b] > Tm) JG_FAIL(h, JG_ERR_ARG, "valid_tm[%d] = %d outside 4..Tm = %d", b, valid_host[b], Tm);
        ragged |= valid_host[b] != Tm;
    }
    if (!ragged) return JG_OK;
    RET(wsalloc(h, (size_t)B, &a->valid));
    return upload_i32_async(h, valid_host, (size_t)B, a->valid);
}

static int jegal_audio_impl32(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_host, float* out) {
    const JegalModel& jg = h->jg;
    const int F = 80;
    AudioGeom a;
    RET(audio_setup(h, B, Tm, valid_host, &a));
    float *m0, *c0, *c3, *c6, *c9, *c12, *c15;
    RET(wsalloc(h, (size_t)B * Tm * F, &m0));
    RET(wsalloc(h, (size_t)B * Tm * F * 32, &c0));
    RET(wsalloc(h, (size_t)B * a.g3.OH * a.g3.OW * 64, &c3));
    RET(wsalloc(h, (size_t)B * a.g6.OH * a.g6.OW * 128, &c6));
    RET(wsalloc(h, (size_t)B * a.g9.OH * a.g9.OW * 256, &c9));
    RET(wsalloc(h, (size_t)B * a.g12.OH * a.g12.OW * 256, &c12));
    RET(wsalloc(h, (size_t)B * a.g15.OH * 256, &c15));
    // every layer's rows beyond a clip's own extent are zero: the padding the clip would see alone (jegal_audio_impl)
    auto tail = [&](float* x, int halvings, int H, long row_elems) -> int {
        if (!a.valid) return JG_OK;
        return timed(h, JG_ST_MISC, [&] { return launch_zero_tail32(x, a.valid, halvings, B, H, row_elems, h->stream); });
    };
    const float* mel_in = mel;
    if (a.valid) {
        HIPCHK(h, hipMemcpyAsync(m0, mel, (size_t)B * Tm * F * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        RET(tail(m0, 0, Tm, F));
        mel_in = m0;
    }
    Epi32 e; e.act = 1;
    RET(gemm32(h, JG_ST_CONV, mel_in, 0, B * Tm * F, jg.a0, c0, e, &a.g0));
    RET(tail(c0, 0, Tm, (long)F * 32));
    RET(gemm32(h, JG_ST_CONV, c0, 0, B * a.g3.OH * a.g3.OW, jg.a3, c3, e, &a.g3));
    RET(tail(c3, 1, a.g3.OH, (long)a.g3.OW * 64));
    RET(gemm32(h, JG_ST_CONV, c3, 0, B * a.g6.OH * a.g6.OW, jg.a6, c6, e, &a.g6));
    RET(tail(c6, 2, a.g6.OH, (long)a.g6.OW * 128));
    RET(gemm32(h, JG_ST_CONV, c6, 0, B * a.g9.OH * a.g9.OW, jg.a9, c9, e, &a.g9));
    RET(tail(c9, 2, a.g9.OH, (long)a.g9.OW * 256));
    RET(gemm32(h, JG_ST_CONV, c9, 0, B * a.g12.OH * a.g12.OW, jg.a12, c12, e, &a.g12));
    RET(gemm32(h, JG_ST_CONV, c12, 0, B * a.g15.OH, jg.a15, c15, Epi32(), &a.g15));
    return gemm32(h, JG_ST_GEMM, c15, 256, B * a.g15.OH, jg.op_audio, out);
}

static int jegal_text_impl32(jg_handle* h, const float* states, const float* mask, int B, int L, float* out) {
    const int M = B * L;
    float *x32, *n32;
    RET(wsalloc(h, (size_t)M * 768, &x32));
    RET(wsalloc(h, (size_t)M * 768, &n32));
    HIPCHK(h, hipMemcpyAsync(x32, states, (size_t)M * 768 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    RET(annotated_encoder32(h, h->jg.text_layers, 3, h->jg.text_norm, x32, n32, mask, B, L, 768, 3072));
    return gemm32(h, JG_ST_GEMM, n32, 768, M, h->jg.op_text, out);
}

// the content fusion on fp32 activations: the audit path (x3 = false) and the split-operand ends of the fp16 modes
static int fuse_content_impl32(jg_handle* h, const float* fused, int rows, float* out, bool x3) {
    const JegalModel& jg = h->jg;
    float *a32, *b32;
    RET(wsalloc(h, (size_t)rows * 512, &a32));
    RET(wsalloc(h, (size_t)rows * 512, &b32));
    Epi32 r; r.act = 1;
    RET(gemm_f32(h, x3, fused, 512, rows, jg.fu0, a32, r));
    RET(gemm_f32(h, x3, a32, 512, rows, jg.fu2, b32));
    RET(gemm_f32(h, x3, b32, 512, rows, jg.al_c0, a32, r));
    return gemm_f32(h, x3, a32, 512, rows, jg.al_c2, out);
}

// ------------------------------------------------------------------------------------ fp16 forms
// pre-norm encoder (modules.py:11-59) in place on x32; returns final-norm output in n16
// parts (diagnosis, option audit_jegal_parts): bit 1 = the attention sub-layers, bit 2 = the feed-forward sub-layers run on the fp32 audit
// kernels (encoder_sublayers32, with the audit path above)
static int annotated_encoder(jg_handle* h, const EncLayer* layers, int nl, const LNp& fin, float* x32, f16* n16,
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
    const JegalModel& jg = h->jg;
    if (!jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || T <= 0 || T > 500) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and 0 < T <= 500 (PE table, modules.py:136)");
    if (audit_mask(h) & AUD_JG) return jegal_gestures_impl32(h, feats, mask, B, T, align, out);
    const int M = B * T;
    // the branch's two ends on the fp32 kernel (option jegal_fp32_ends; not in the plain-fp16 / bf16 reported modes, not while calibrating)
    const bool ends32 = split_ends(h, {&jg.ip0, &jg.ip3, &jg.op_rgb, &jg.al_g0, &jg.al_g2});
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
        RET(gemm(h, JG_ST_GEMM, f16in, 1024, M, jg.ip0, e));
        RET(timed(h, JG_ST_NORM, [&] { return LAUNCH(h, launch_layernorm, t32, jg.ip_ln.w, jg.ip_ln.b, M, 512, LN_STD, 1, nullptr, t16, h->stream); }));
        Epi p; p.res = jg.rgb_pe; p.ldr = 512; p.res_mod = T; p.out32 = x32;
        RET(gemm(h, JG_ST_GEMM, t16, 512, M, jg.ip3, p));
    }
    RET(annotated_encoder(h, jg.rgb_layers, 6, jg.rgb_norm, x32, n16, mask, B, T, 512, 2048, parts, n32));
    if (parts & 8) return jegal_tail32(h, n32, M, align, out, ends_x3);
    if (!align) {
        Epi o; o.out32 = out;
        return gemm(h, JG_ST_GEMM, n16, 512, M, jg.op_rgb, o);
    }
    RET(wsalloc(h, (size_t)M * 512, &g16));
    RET(wsalloc(h, (size_t)M * 512, &a16));
    Epi o1; o1.out16 = g16;
    RET(gemm(h, JG_ST_GEMM, n16, 512, M, jg.op_rgb, o1));
    Epi o2; o2.relu = 1; o2.out16 = a16;
    RET(gemm(h, JG_ST_GEMM, g16, 512, M, jg.al_g0, o2));
    Epi o3; o3.out32 = out;
    return gemm(h, JG_ST_GEMM, a16, 512, M, jg.al_g2, o3);
}

// valid_host (optional, host [B]): clip b holds valid_host[b] mel frames, the rest of its Tm rows is batch padding.  Every layer's
// rows beyond the clip's own extent are zeroed (launch_zero_tail), i.e. each clip sees the zero padding it would see alone -- the
// reference's dataset driver runs one clip per step (extract_jegal_embs.py:141), so its result never depends on a longer neighbour.
int jegal_audio_impl(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_host, float* out) {
    const JegalModel& jg = h->jg;
    if (!jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || Tm < 4) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and Tm >= 4");
    if (audit_mask(h) & AUD_CONTENT) return jegal_audio_impl32(h, mel, B, Tm, valid_host, out);
    const int F = 80;
    AudioGeom a;
    RET(audio_setup(h, B, Tm, valid_host, &a));
    f16 *c0, *c3, *c6, *c9, *c12, *c15;
    const long M0 = (long)B * Tm * F;
    RET(wsalloc(h, (size_t)M0 * 32, &c0));
    RET(wsalloc(h, (size_t)B * a.g3.OH * a.g3.OW * 64, &c3));
    RET(wsalloc(h, (size_t)B * a.g6.OH * a.g6.OW * 128, &c6));
    RET(wsalloc(h, (size_t)B * a.g9.OH * a.g9.OW * 256, &c9));
    RET(wsalloc(h, (size_t)B * a.g12.OH * a.g12.OW * 256, &c12));
    RET(wsalloc(h, (size_t)B * a.g15.OH * 256, &c15));
    auto tail = [&](f16* x, int halvings, const ConvGeom& g, int C) -> int {
        if (!a.valid) return JG_OK;
        return timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_zero_tail, x, a.valid, halvings, B, g.OH, (long)g.OW * C, h->stream); });
    };
    // cnn.0 + BN + ReLU straight from the mel frames (round 2: im2col + a K = 32 GEMM on the register-staged kernel)
    RET(timed(h, JG_ST_CONV, [&] { return LAUNCH(h, launch_audio_conv0, mel, B, Tm, F, jg.a0.wh, run_lo(h, jg.a0, false), jg.a0.bias, c0, a.valid, h->stream); }));
    Epi e; e.relu = 1;
    e.out16 = c3; RET(gemm(h, JG_ST_CONV, c0, 0, B * a.g3.OH * a.g3.OW, jg.a3, e, &a.g3));
    RET(tail(c3, 1, a.g3, 64));
    e.out16 = c6; RET(gemm(h, JG_ST_CONV, c3, 0, B * a.g6.OH * a.g6.OW, jg.a6, e, &a.g6));
    RET(tail(c6, 2, a.g6, 128));
    e.out16 = c9; RET(gemm(h, JG_ST_CONV, c6, 0, B * a.g9.OH * a.g9.OW, jg.a9, e, &a.g9));
    RET(tail(c9, 2, a.g9, 256));
    e.out16 = c12; RET(gemm(h, JG_ST_CONV, c9, 0, B * a.g12.OH * a.g12.OW, jg.a12, e, &a.g12));
    e.relu = 0;      // (cnn.15 is 1x1: rows of c12 beyond a clip's extent only reach output rows beyond it, which callers strip)
    e.out16 = c15; RET(gemm(h, JG_ST_CONV, c12, 0, B * a.g15.OH, jg.a15, e, &a.g15));
    Epi o; o.out32 = out;
    return gemm(h, JG_ST_GEMM, c15, 256, B * a.g15.OH, jg.op_audio, o);
}

int jegal_text_impl(jg_handle* h, const float* states, const float* mask, int B, int L, float* out) {
    const JegalModel& jg = h->jg;
    if (!jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || L <= 0) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and L > 0");
    if (audit_mask(h) & AUD_CONTENT) return jegal_text_impl32(h, states, mask, B, L, out);
    const int M = B * L;
    float* x32; f16* n16;
    RET(wsalloc(h, (size_t)M * 768, &x32));
    RET(wsalloc(h, (size_t)M * 768, &n16));
    HIPCHK(h, hipMemcpyAsync(x32, states, (size_t)M * 768 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    const bool x3 = split_ends(h, {&jg.op_text});
    float* n32 = nullptr;
    if (x3) RET(wsalloc(h, (size_t)M * 768, &n32));
    RET(annotated_encoder(h, jg.text_layers, 3, jg.text_norm, x32, n16, mask, B, L, 768, 3072, 0, n32));
    if (x3) return gemm_x3(h, JG_ST_GEMM, n32, 768, M, jg.op_text, out);      // proj_op_text from the final norm's fp32 rows (round 6)
    Epi o; o.out32 = out;
    return gemm(h, JG_ST_GEMM, n16, 768, M, jg.op_text, o);
}

int fuse_content_impl(jg_handle* h, const float* fused, int rows, float* out) {
    const JegalModel& jg = h->jg;
    if (!jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (rows <= 0) JG_FAIL(h, JG_ERR_ARG, "rows must be positive");
    if (audit_mask(h) & AUD_CONTENT) return fuse_content_impl32(h, fused, rows, out, false);
    // round 6: like the gesture branch's ends, the content path's last four GEMMs keep fp32 activations and run on the split-operand
    // kernel (fp32-grade products on the fp16 matrix cores; a few hundred rows: the cost is a launch either way)
    if (split_ends(h, {&jg.fu0, &jg.fu2, &jg.al_c0, &jg.al_c2})) return fuse_content_impl32(h, fused, rows, out, true);
    f16 *x16, *a16, *b16;
    RET(wsalloc(h, (size_t)rows * 512, &x16));
    RET(wsalloc(h, (size_t)rows * 512, &a16));
    RET(wsalloc(h, (size_t)rows * 512, &b16));
    RET(timed(h, JG_ST_MISC, [&] { return LAUNCH(h, launch_cast_f32_f16, fused, x16, (long)rows * 512, h->stream); }));
    Epi r; r.relu = 1; r.out16 = a16;
    RET(gemm(h, JG_ST_GEMM, x16, 512, rows, jg.fu0, r));
    Epi p; p.out16 = b16;
    RET(gemm(h, JG_ST_GEMM, a16, 512, rows, jg.fu2, p));
    RET(gemm(h, JG_ST_GEMM, b16, 512, rows, jg.al_c0, r));
    Epi o; o.out32 = out;
    return gemm(h, JG_ST_GEMM, a16, 512, rows, jg.al_c2, o);
}

}  // namespace engine
