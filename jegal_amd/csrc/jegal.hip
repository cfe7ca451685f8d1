// libjegal_hip: JEGAL -- finalize, and the pre-norm encoder, gesture branch, audio CNN, text branch and content fusion, each written once
// for the 16-bit and the fp32 arithmetics (engine.h, Arith<T>).  Host code only.
#include "engine.h"

#include <algorithm>

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

// ------------------------------------------------------------------------------------ model graphs, once per arithmetic (engine.h, Arith<T>)
// The two sub-layers of a pre-norm encoder layer (modules.py:11-59), in place on the fp32 residual stream:
// x += out(attn(qkv(LN1 x))) and x += w_2(relu(w_1(LN2 x))).  EncBufs: the activations in between, M rows each
template <class T> struct EncBufs { T *n, *qkv, *att, *hid; };
template <class T>
static int enc_bufs(jg_handle* h, int M, int D, int Dff, T* n, EncBufs<T>* s) {
    s->n = n;
    if (!n) RET(wsalloc(h, (size_t)M * D, &s->n));
    RET(wsalloc(h, (size_t)M * 3 * D, &s->qkv));
    RET(wsalloc(h, (size_t)M * D, &s->att));
    return wsalloc(h, (size_t)M * Dff, &s->hid);
}
template <class T>
static int attn_sublayer(jg_handle* h, Arith<T> ar, const EncLayer& L, float* x32, const EncBufs<T>& s, const float* mask, int B, int S, int D) {
    const int M = B * S, H = 8;
    RET(layernorm(h, ar, x32, L.n1, M, D, LN_ANNOTATED, 0, s.n));
    RET(linear(h, ar, s.n, D, M, L.qkv, s.qkv));
    RET(attention(h, ar, s.qkv, mask, B, S, H, D / H, s.att));
    return linear_to32(h, ar, s.att, D, M, L.out, x32, x32, D);
}
template <class T>
static int ff_sublayer(jg_handle* h, Arith<T> ar, const EncLayer& L, float* x32, const EncBufs<T>& s, int M, int D, int Dff) {
    RET(layernorm(h, ar, x32, L.n2, M, D, LN_ANNOTATED, 0, s.n));
    RET(linear(h, ar, s.n, D, M, L.ff1, s.hid, 1));
    return linear_to32(h, ar, s.hid, Dff, M, L.ff2, x32, x32, D);
}

// pre-norm encoder (encoder_rgb, encoder_text) in place on x32; the final norm writes the next GEMM's operand n and, when asked, its fp32
// rows n32 in the same launch.  parts (diagnosis in the 16-bit arithmetic, option audit_jegal_parts): bit 1 = the attention sub-layers,
// bit 2 = the feed-forward sub-layers run on the fp32 audit kernels instead
template <class T>
static int annotated_encoder(jg_handle* h, Arith<T> ar, const EncLayer* layers, int nl, const LNp& fin, float* x32, T* n, const float* mask, int B,
                             int S, int D, int Dff, int parts = 0, float* n32 = nullptr) {
    const int M = B * S;
    EncBufs<T> s;
    EncBufs<float> s32;
    RET(enc_bufs(h, M, D, Dff, n, &s));
    if (parts & 6) RET(enc_bufs(h, M, D, Dff, (float*)nullptr, &s32));
    for (int l = 0; l < nl; ++l) {
        RET(parts & 2 ? attn_sublayer(h, A32(), layers[l], x32, s32, mask, B, S, D) : attn_sublayer(h, ar, layers[l], x32, s, mask, B, S, D));
        RET(parts & 4 ? ff_sublayer(h, A32(), layers[l], x32, s32, M, D, Dff) : ff_sublayer(h, ar, layers[l], x32, s, M, D, Dff));
    }
    return layernorm(h, ar, x32, fin, M, D, LN_ANNOTATED, 0, n, n32);
}

// proj_ip_rgb + positional rows (jegal.py:25-28,84-85): feats (M, 1024) fp32 -> the stream x32 (M, 512); S tokens per clip.
// S == 0: without the positional rows (long tracks: span_gather adds them per window)
template <class T>
static int jegal_input(jg_handle* h, Arith<T> ar, const float* feats, int M, int S, float* x32) {
    const JegalModel& jg = h->jg;
    const T* in;
    float* t32;
    T* t;
    RET(operand(h, ar, feats, (long)M * 1024, &in));
    RET(wsalloc(h, (size_t)M * 512, &t32));
    RET(wsalloc(h, (size_t)M * 512, &t));
    RET(linear_to32(h, ar, in, 1024, M, jg.ip0, t32));
    RET(layernorm(h, ar, t32, jg.ip_ln, M, 512, LN_STD, 1, t));
    return linear_to32(h, ar, t, 512, M, jg.ip3, x32, S ? jg.rgb_pe : nullptr, 512, S);
}

// proj_op_rgb (+ proj_op_align_gesture) from the final norm's rows
template <class T>
static int jegal_tail(jg_handle* h, Arith<T> ar, const T* n, int M, int align, float* out) {
    const JegalModel& jg = h->jg;
    if (!align) return linear_to32(h, ar, n, 512, M, jg.op_rgb, out);
    T *g, *a;
    RET(wsalloc(h, (size_t)M * 512, &g));
    RET(wsalloc(h, (size_t)M * 512, &a));
    RET(linear(h, ar, n, 512, M, jg.op_rgb, g));
    RET(linear(h, ar, g, 512, M, jg.al_g0, a, 1));
    return linear_to32(h, ar, a, 512, M, jg.al_g2, out);
}

// encoder_text + proj_op_text.  end (16-bit arithmetic only): proj_op_text runs in *end from the final norm's fp32 rows (round 6)
template <class T>
static int jegal_text(jg_handle* h, Arith<T> ar, const A32* end, const float* states, const float* mask, int B, int L, float* out) {
    const JegalModel& jg = h->jg;
    const int M = B * L;
    float *x32, *n32 = nullptr;
    T* n;
    RET(wsalloc(h, (size_t)M * 768, &x32));
    RET(wsalloc(h, (size_t)M * 768, &n));
    if (end) RET(wsalloc(h, (size_t)M * 768, &n32));
    HIPCHK(h, hipMemcpyAsync(x32, states, (size_t)M * 768 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    RET(annotated_encoder(h, ar, jg.text_layers, 3, jg.text_norm, x32, n, mask, B, L, 768, 3072, 0, n32));
    return end ? linear_to32(h, *end, n32, 768, M, jg.op_text, out) : linear_to32(h, ar, n, 768, M, jg.op_text, out);
}

// proj_op_fusion_content + proj_op_align_content
template <class T>
static int fuse_content(jg_handle* h, Arith<T> ar, const float* fused, int rows, float* out) {
    const JegalModel& jg = h->jg;
    const T* x;
    T *a, *b;
    RET(operand(h, ar, fused, (long)rows * 512, &x));
    RET(wsalloc(h, (size_t)rows * 512, &a));
    RET(wsalloc(h, (size_t)rows * 512, &b));
    RET(linear(h, ar, x, 512, rows, jg.fu0, a, 1));
    RET(linear(h, ar, a, 512, rows, jg.fu2, b));
    RET(linear(h, ar, b, 512, rows, jg.al_c0, a, 1));
    return linear_to32(h, ar, a, 512, rows, jg.al_c2, out);
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

// cnn.0 .. cnn.15 + proj_op_audio.  Every layer's rows beyond a clip's own extent are zeroed, i.e. each clip sees the zero padding it
// would see alone -- the reference's dataset driver runs one clip per step (extract_jegal_embs.py:141), so its result never depends on
// a longer neighbour.  (cnn.15 is 1x1, without ReLU: rows of c12 beyond a clip's extent only reach output rows beyond it, which callers strip)
template <class T>
static int jegal_audio(jg_handle* h, Arith<T> ar, const float* mel, int B, int Tm, const int32_t* valid_host, float* out) {
    const JegalModel& jg = h->jg;
    const int F = 80;
    AudioGeom a;
    RET(audio_setup(h, B, Tm, valid_host, &a));
    T *c0, *c3, *c6, *c9, *c12, *c15;
    RET(wsalloc(h, (size_t)B * Tm * F * 32, &c0));
    RET(wsalloc(h, (size_t)B * a.g3.OH * a.g3.OW * 64, &c3));
    RET(wsalloc(h, (size_t)B * a.g6.OH * a.g6.OW * 128, &c6));
    RET(wsalloc(h, (size_t)B * a.g9.OH * a.g9.OW * 256, &c9));
    RET(wsalloc(h, (size_t)B * a.g12.OH * a.g12.OW * 256, &c12));
    RET(wsalloc(h, (size_t)B * a.g15.OH * 256, &c15));
    auto conv = [&](const T* x, const Lin& L, const ConvGeom& g, T* y, int relu, int halvings) -> int {
        RET(linear(h, ar, x, 0, B * g.OH * g.OW, L, y, relu, &g));
        return halvings < 0 ? JG_OK : zero_tail(h, ar, y, a.valid, halvings, B, g.OH, (long)g.OW * L.N);
    };
    RET(audio_conv0(h, ar, mel, B, Tm, F, jg.a0, a.g0, a.valid, c0));
    RET(conv(c0, jg.a3, a.g3, c3, 1, 1));
    RET(conv(c3, jg.a6, a.g6, c6, 1, 2));
    RET(conv(c6, jg.a9, a.g9, c9, 1, 2));
    RET(conv(c9, jg.a12, a.g12, c12, 1, -1));
    RET(conv(c12, jg.a15, a.g15, c15, 0, -1));
    return linear_to32(h, ar, c15, 256, B * a.g15.OH, jg.op_audio, out);
}

// ------------------------------------------------------------------------------------ entries: choose the arithmetics and call
// The gesture branch in the 16-bit modes: its two ends keep fp32 activations (option jegal_fp32_ends; not in the plain-fp16 / bf16 reported
// modes, not while calibrating): in production with split operands on the fp16 matrix cores (`ends`), under diagnosis (audit_jegal_parts
// bits 1 / 8) on the fp32 MFMA.  parts: audit_jegal_parts' bits as the graph runs them (1 input projection, 8 final norm + tail in `ends`)
struct GestureEnds { int parts; A32 ends; };
static GestureEnds gesture_ends(const jg_handle* h) {
    const JegalModel& jg = h->jg;
    const bool ends32 = split_ends(h, {&jg.ip0, &jg.ip3, &jg.op_rgb, &jg.al_g0, &jg.al_g2});
    return {h->audit_jegal_parts | (ends32 ? 9 : 0), A32{ends32 && !(h->audit_jegal_parts & 9)}};
}

int jegal_gestures_impl(jg_handle* h, const float* feats, const float* mask, int B, int T, int align, float* out) {
    const JegalModel& jg = h->jg;
    if (!jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || T <= 0 || T > 500) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and 0 < T <= 500 (PE table, modules.py:136)");
    const int M = B * T;
    float *x32, *n32 = nullptr;
    RET(wsalloc(h, (size_t)M * 512, &x32));
    if (audit_mask(h) & AUD_JG) {
        RET(wsalloc(h, (size_t)M * 512, &n32));
        RET(jegal_input(h, A32(), feats, M, T, x32));
        RET(annotated_encoder(h, A32(), jg.rgb_layers, 6, jg.rgb_norm, x32, n32, mask, B, T, 512, 2048));
        return jegal_tail(h, A32(), n32, M, align, out);
    }
    const auto [parts, ends] = gesture_ends(h);
    f16* n16;
    RET(wsalloc(h, (size_t)M * 512, &n16));
    if (parts & 8) RET(wsalloc(h, (size_t)M * 512, &n32));
    RET(parts & 1 ? jegal_input(h, ends, feats, M, T, x32) : jegal_input(h, A16(), feats, M, T, x32));
    RET(annotated_encoder(h, A16(), jg.rgb_layers, 6, jg.rgb_norm, x32, n16, mask, B, T, 512, 2048, parts, n32));
    return parts & 8 ? jegal_tail(h, ends, n32, M, align, out) : jegal_tail(h, A16(), n16, M, align, out);
}

// The window rule of long gesture tracks (include/jegal_hip.h, jg_track_windows), and the only place it is written down: track i =
// rows off[i] .. off[i + 1] - 1 is cut into ceil(T / win) windows; window j emits its core [j win, min((j + 1) win, T)) and is encoded
// over its span [max(0, j win - ctx), min(T, (j + 1) win + ctx)).  table (optional) [cap][4] = (span first row, span length, core
// offset inside the span, core length), rows global.  Pure host arithmetic; nothing is written unless every argument is good.
int plan_track_windows(const int32_t* off, int n_tracks, int win, int ctx, int32_t* table, int cap, int* n_windows, int* span_max) {
    if (n_tracks < 0 || (n_tracks > 0 && !off) || !n_windows || !span_max || win < 1 || ctx < 0 || (long)win + 2L * ctx > TRACK_SPAN_MAX)
        return JG_ERR_ARG;
    long n = 0;
    int smax = 0;
    for (int i = 0; i < n_tracks; ++i) {
        if (off[i] < 0 || off[i + 1] < off[i]) return JG_ERR_ARG;
        const int T = off[i + 1] - off[i];
        n += ((long)T + win - 1) / win;
        // the track's longest span: no span is longer than `bound`, and in a long track the first window clear of both ends reaches it
        const int bound = std::min(T, win + 2 * ctx);
        int st = 0;
        for (long c0 = 0; c0 < T && st < bound; c0 += win)
            st = std::max(st, (int)(std::min((long)T, c0 + win + ctx) - std::max(0L, c0 - ctx)));
        smax = std::max(smax, st);
    }
    if (n > INT32_MAX || (table && (cap < 0 || n > cap))) return JG_ERR_ARG;
    if (table) {
        int32_t* e = table;
        for (int i = 0; i < n_tracks; ++i) {
            const long T = off[i + 1] - off[i];
            for (long c0 = 0; c0 < T; c0 += win, e += 4) {
                const long c1 = std::min(T, c0 + win), s0 = std::max(0L, c0 - ctx), s1 = std::min(T, c0 + win + ctx);
                e[0] = (int32_t)(off[i] + s0); e[1] = (int32_t)(s1 - s0); e[2] = (int32_t)(c0 - s0); e[3] = (int32_t)(c1 - c0);
            }
        }
    }
    *n_windows = (int)n;
    *span_max = smax;
    return JG_OK;
}

// forward_gestures (+ align MLP) over the windows of long tracks.  The row-wise ends run once per TRACK row (a row lies in up to
// (win + 2 ctx) / win spans): proj_ip_rgb on the `rows` track rows, span_gather into the (n_windows, span_max) padded batch with the
// positional rows and the key mask, the encoder as jegal_gestures_impl runs it, core_compact of the final norm's rows -- the operand
// the tail reads, 16-bit or fp32 -- back into track order, proj_op_rgb (+ align) on `rows` rows.  table_host: plan_track_windows
int jegal_gesture_tracks_impl(jg_handle* h, const float* feats, const int32_t* table_host, int n_windows, int span_max, int rows, int align, float* out) {
    const JegalModel& jg = h->jg;
    if (!jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (n_windows <= 0 || rows <= 0 || span_max <= 0 || span_max > TRACK_SPAN_MAX) JG_FAIL(h, JG_ERR_ARG, "empty window table or span_max outside 1..500");
    const int B = n_windows, S = span_max, M = B * S;
    int32_t* table;
    float *p32, *x32, *mask, *n32 = nullptr;
    RET(wsalloc(h, (size_t)B * 4, &table));
    RET(upload_i32_async(h, table_host, (size_t)B * 4, table));
    RET(wsalloc(h, (size_t)rows * 512, &p32));
    RET(wsalloc(h, (size_t)M * 512, &x32));
    RET(wsalloc(h, (size_t)M, &mask));
    auto gather = [&]() { return timed(h, JG_ST_MISC, [&] { return launch_span_gather(p32, jg.rgb_pe, table, B, S, 512, x32, mask, h->stream); }); };
    auto compact = [&](const void* n, int elem_bytes, void* c) {
        return timed(h, JG_ST_MISC, [&] { return launch_core_compact(n, elem_bytes, table, B, S, 512, c, h->stream); });
    };
    if (audit_mask(h) & AUD_JG) {
        float* c32;
        RET(wsalloc(h, (size_t)M * 512, &n32));
        RET(wsalloc(h, (size_t)rows * 512, &c32));
        RET(jegal_input(h, A32(), feats, rows, 0, p32));
        RET(gather());
        RET(annotated_encoder(h, A32(), jg.rgb_layers, 6, jg.rgb_norm, x32, n32, mask, B, S, 512, 2048));
        RET(compact(n32, 4, c32));
        return jegal_tail(h, A32(), c32, rows, align, out);
    }
    const auto [parts, ends] = gesture_ends(h);
    f16 *n16, *c16 = nullptr;
    float* c32 = nullptr;
    RET(wsalloc(h, (size_t)M * 512, &n16));
    if (parts & 8) {
        RET(wsalloc(h, (size_t)M * 512, &n32));
        RET(wsalloc(h, (size_t)rows * 512, &c32));
    } else {
        RET(wsalloc(h, (size_t)rows * 512, &c16));
    }
    RET(parts & 1 ? jegal_input(h, ends, feats, rows, 0, p32) : jegal_input(h, A16(), feats, rows, 0, p32));
    RET(gather());
    RET(annotated_encoder(h, A16(), jg.rgb_layers, 6, jg.rgb_norm, x32, n16, mask, B, S, 512, 2048, parts, n32));
    if (parts & 8) {
        RET(compact(n32, 4, c32));
        return jegal_tail(h, ends, c32, rows, align, out);
    }
    RET(compact(n16, 2, c16));
    return jegal_tail(h, A16(), c16, rows, align, out);
}

// valid_host (optional, host [B]): clip b holds valid_host[b] mel frames, the rest of its Tm rows is batch padding
int jegal_audio_impl(jg_handle* h, const float* mel, int B, int Tm, const int32_t* valid_host, float* out) {
    if (!h->jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || Tm < 4) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and Tm >= 4");
    if (audit_mask(h) & AUD_CONTENT) return jegal_audio(h, A32(), mel, B, Tm, valid_host, out);
    return jegal_audio(h, A16(), mel, B, Tm, valid_host, out);
}

int jegal_text_impl(jg_handle* h, const float* states, const float* mask, int B, int L, float* out) {
    if (!h->jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (B <= 0 || L <= 0) JG_FAIL(h, JG_ERR_ARG, "need B > 0 and L > 0");
    if (audit_mask(h) & AUD_CONTENT) return jegal_text(h, A32(), nullptr, states, mask, B, L, out);
    const A32 x3{true};
    return jegal_text(h, A16(), split_ends(h, {&h->jg.op_text}) ? &x3 : nullptr, states, mask, B, L, out);
}

int fuse_content_impl(jg_handle* h, const float* fused, int rows, float* out) {
    const JegalModel& jg = h->jg;
    if (!jg.m.ready) JG_FAIL(h, JG_ERR_STATE, "JEGAL weights not finalized");
    if (rows <= 0) JG_FAIL(h, JG_ERR_ARG, "rows must be positive");
    if (audit_mask(h) & AUD_CONTENT) return fuse_content(h, A32(), fused, rows, out);
    // round 6: like the gesture branch's ends, the content path's last four GEMMs keep fp32 activations and run on the split-operand
    // kernel (fp32-grade products on the fp16 matrix cores; a few hundred rows: the cost is a launch either way)
    if (split_ends(h, {&jg.fu0, &jg.fu2, &jg.al_c0, &jg.al_c2})) return fuse_content(h, A32{true}, fused, rows, out);
    return fuse_content(h, A16(), fused, rows, out);
}

}  // namespace engine
