// libjegal_hip: GestSync's audio stream (net_aud + ff_aud, gestsync.py:89-146,164-168,346-361) -- finalize and the graph, written once for
// the 16-bit and the fp32 arithmetics (engine.h, Arith<T>).  Host code only; the stream's own kernels: gsa_kernels.hip.
#include "engine.h"

namespace engine {

// `which` bit 3.  Strict: every key of net_aud.conv1..fc6 / bn1..6 and ff_aud.fc7 / bn7 / fc8 must be staged.
// conv1 (C_in = 1, K = 9) stays fp32 for gsa_conv1_pool_kernel.  conv2 .. conv5 are implicit GEMMs over power-of-two channel counts:
// 192 -> 256 and 384 -> 512, the added output channels with zero weights and zero shift (relu(0) = 0, and 0 through the pools), the
// added input slots with zero weights.  fc6 (4 x 2 x 256, NHWC order = the order of the pooled tensor's rows), fc7 and fc8 are plain
// Linears.  Weight forms (weight_form.h), all as model 1: conv2 .. conv5 and fc6 LK_CONV, fc7 and fc8 LK_CONTENT.
int finalize_gestsync_audio(jg_handle* h) {
    drop_model(h, h->gsa);
    GestSyncAudioModel& a = h->gsa;
    Model& m = a.m;
    {
        std::vector<float> wf, shift;         // make_conv's fold and layout with I = 1, slot = 1: [64][9] in natural tap order
        RET(fold_conv(h, "net_aud.conv1", "net_aud.bn1", {64, 1, 1, 3, 3, 1, 0, 0, 1, 1, false}, &wf, &shift));
        RET(upload(h, m, wf, &a.c1w));
        RET(upload(h, m, shift, &a.c1shift));
    }
    RET(make_conv(h, m, "net_aud.conv2", "net_aud.bn2", 192, 64, 1, 3, 3, 64, 0, &a.c2, 1, 2, false, 256));
    RET(make_conv(h, m, "net_aud.conv3", "net_aud.bn3", 384, 192, 1, 3, 3, 256, 0, &a.c3, 1, 1, false, 512));
    RET(make_conv(h, m, "net_aud.conv4", "net_aud.bn4", 256, 384, 1, 3, 3, 512, 0, &a.c4));
    RET(make_conv(h, m, "net_aud.conv5", "net_aud.bn5", 256, 256, 1, 3, 3, 256, 0, &a.c5));
    RET(make_conv(h, m, "net_aud.fc6", "net_aud.bn6", 512, 256, 1, 4, 2, 256, 0, &a.fc6));
    RET(make_conv(h, m, "ff_aud.fc7", "ff_aud.bn7", 512, 512, 1, 1, 1, 512, 0, &a.fc7, 1, 1, false, 0, LK_CONTENT));
    RET(make_conv(h, m, "ff_aud.fc8", "", 1024, 512, 1, 1, 1, 512, 0, &a.fc8, 1, 1, false, 0, LK_CONTENT));
    m.ready = true;
    return JG_OK;
}

// the max-pools of the two arithmetics
static int pool_3x3(jg_handle* h, A16, const f16* in, f16* out, int N, int H, int W, int C) {
    return timed(h, JG_ST_POOL, [&] { return LAUNCH(h, launch_maxpool3x3s2, in, out, N, H, W, C, h->stream, nullptr, 0, nullptr); });
}
static int pool_3x3(jg_handle* h, A32, const float* in, float* out, int N, int H, int W, int C) {
    return timed(h, JG_ST_POOL, [&] { return launch_maxpool3x3s2_32(in, out, N, H, W, C, h->stream); });
}
template <class T>
static int pool_2x3(jg_handle* h, const T* in, T* out, int N, int H, int W, int C) {
    return timed(h, JG_ST_POOL, [&] { return launch_maxpool_2x3_s2(in, out, N, H, W, C, sizeof(T) == 4, h->stream); });
}

// Windows n0 .. n0 + nb - 1 of the source -> out (nb, 1024) fp32.  A window's embedding is a function of its own 8000 values; which GEMM
// instance a layer gets depends on nb alone.
template <class T>
static int gsa_graph(jg_handle* h, Arith<T> ar, const float* src, int clip_form, int n0, int nb, int T_, int Tm, const int* valid, float* out) {
    const GestSyncAudioModel& a = h->gsa;
    const ConvGeom g2 = geom(19, 24, 64, 3, 3, 1, 2, 1, 1);          // -> 19 x 12
    const ConvGeom g3 = geom(9, 5, 256, 3, 3, 1, 1, 1, 1);
    const ConvGeom g4 = geom(9, 5, 512, 3, 3, 1, 1, 1, 1);
    const ConvGeom g5 = geom(9, 5, 256, 3, 3, 1, 1, 1, 1);
    T *p1, *o2, *p2, *o3, *o4, *o5, *p5, *f6, *f7;
    RET(wsalloc(h, (size_t)nb * 19 * 24 * 64, &p1));
    RET(wsalloc(h, (size_t)nb * 19 * 12 * 256, &o2));
    RET(wsalloc(h, (size_t)nb * 9 * 5 * 256, &p2));
    RET(wsalloc(h, (size_t)nb * 9 * 5 * 512, &o3));
    RET(wsalloc(h, (size_t)nb * 9 * 5 * 256, &o4));
    RET(wsalloc(h, (size_t)nb * 9 * 5 * 256, &o5));
    RET(wsalloc(h, (size_t)nb * 4 * 2 * 256, &p5));
    RET(wsalloc(h, (size_t)nb * 512, &f6));
    RET(wsalloc(h, (size_t)nb * 512, &f7));
    RET(timed(h, JG_ST_CONV, [&] {
        return launch_gsa_conv1_pool(src, clip_form, n0, nb, T_, Tm, valid, a.c1w, a.c1shift, p1, sizeof(T) == 4, h->stream);
    }));
    RET(linear(h, ar, p1, 0, nb * 19 * 12, a.c2, o2, 1, &g2));
    RET(pool_3x3(h, ar, o2, p2, nb, 19, 12, 256));
    RET(linear(h, ar, p2, 0, nb * 45, a.c3, o3, 1, &g3));
    RET(linear(h, ar, o3, 0, nb * 45, a.c4, o4, 1, &g4));
    RET(linear(h, ar, o4, 0, nb * 45, a.c5, o5, 1, &g5));
    RET(pool_2x3(h, o5, p5, nb, 9, 5, 256));
    RET(linear(h, ar, p5, 2048, nb, a.fc6, f6, 1));
    RET(linear(h, ar, f6, 512, nb, a.fc7, f7, 1));
    return linear_to32(h, ar, f7, 512, nb, a.fc8, out);
}

// windows per workspace pass: 0.3 MB (16-bit) / 0.6 MB (fp32) of activations per window
constexpr int GSA_PASS_WINDOWS = 4096;

int gestsync_audio_impl(jg_handle* h, const float* src, int clip_form, int B, int Tm, int T, const int32_t* valid_host, float* out) {
    if (B <= 0 || T <= 0 || (clip_form && Tm <= 0)) JG_FAIL(h, JG_ERR_ARG, "need positive sizes");
    if ((long)B * T > (1L << 30)) JG_FAIL(h, JG_ERR_ARG, "too many windows");
    for (int b = 0; valid_host && b < B; ++b)
        if (valid_host[b] < 1 || valid_host[b] > Tm) JG_FAIL(h, JG_ERR_ARG, "valid_tm[%d] = %d outside 1..Tm = %d", b, valid_host[b], Tm);
    if (h->bf16) JG_FAIL(h, JG_ERR_STATE, "GestSync's audio stream has no bf16 build (fp16 and fp32 arithmetics only)");
    if (!h->gsa.m.ready) JG_FAIL(h, JG_ERR_STATE, "GestSync audio weights not finalized (jg_finalize_weights bit 3)");
    const int N = B * T;
    const bool fp32 = audit_mask(h) & AUD_CONV;
    for (int n0 = 0; n0 < N; n0 += GSA_PASS_WINDOWS) {
        const int nb = std::min(GSA_PASS_WINDOWS, N - n0);
        RET(begin_pass(h));
        int* valid = nullptr;
        if (valid_host) {
            RET(wsalloc(h, (size_t)B, &valid));
            RET(upload_i32_async(h, valid_host, (size_t)B, valid));
        }
        float* o = out + (size_t)n0 * 1024;
        if (fp32) RET(gsa_graph(h, A32(), src, clip_form, n0, nb, T, Tm, valid, o));
        else RET(gsa_graph(h, A16(), src, clip_form, n0, nb, T, Tm, valid, o));
    }
    return JG_OK;
}

}  // namespace engine
