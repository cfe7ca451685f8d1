// Recorder of tests/golden/weight_pack_cases.json: what weight finalisation computed BEFORE its arithmetic moved into weight_pack.h.
// The expressions below are copied from that commit's linear.hip (pack_matrix, tap_order, make_conv, the sum of apply_bias_corrections),
// xlmr.hip (the two LayerNorm folds of finalize_xlmr), gestsync.hip (the panel loop of finalize_gestsync) and gestsync_audio.hip (the
// hand-written fold of net_aud.conv1), with the uploads stubbed by host vectors and the tensors of need() passed in.  Nothing here includes
// or calls weight_pack.h, so the table pins the new functions against the old text, not against themselves (weight_form.h, which the old
// text already called, has its own table).  Inputs and outputs are integer bit patterns.
//     /opt/rocm/llvm/bin/clang++ -O3 -std=c++17 -ffp-contract=fast -I include -I jegal_amd/csrc tools/weight_pack_recorder.cpp -o /tmp/wpr
//     /tmp/wpr > tests/golden/weight_pack_cases.json
// (the optimisation flags of jegal_amd/csrc/Makefile's host code, no -march)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "weight_form.h"

using namespace engine;
typedef _Float16 f16;

// ------------------------------------------------------------------------------------ stubs: a handle's policy, a Lin of host vectors
struct jg_handle { int precision = 0; bool bf16 = false, audit_weights = false, conv_round_diffuse = true; };
struct Model { int id = 1; int bc_records = 0; std::vector<float> bc_w32, bc_b32; };
struct Lin {
    std::vector<f16> wh, lo;
    std::vector<float> bias, c1h, c1f, w32d, b32d;
    bool has_lo = false, has_c1 = false, has_32 = false, has_cal = false;
    int N = 0, K = 0;
    WeightForm form = WF_SINGLE;
    bool uncalibrated = false;
};
template <class T> static void upload(const std::vector<T>& v, std::vector<T>* out) { *out = v; }

// ------------------------------------------------------------------------------------ copied: linear.hip
inline uint16_t bf16_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static void pack_matrix(jg_handle* h, Model& m, const std::vector<float>& w, const std::vector<float>& bias, int N, int K, int kind, Lin* L, bool ln_consumer,
                        bool keep32, int diffuse_group) {
    const WeightForm form = weight_form(h->precision, kind, m.id);
    const bool want_lo = lo_kept(form, keep32);
    std::vector<f16> hi((size_t)N * K), lo;
    if (want_lo) lo.resize((size_t)N * K);
    if (h->bf16) {                       // JG_PREC_BF16: single bf16 weights (the 16-bit container is re-typed by the bf16 build)
        for (size_t i = 0; i < hi.size(); ++i) {
            const uint16_t b = bf16_bits(w[i]);
            std::memcpy(&hi[i], &b, 2);
        }
    } else if (diffuse_group > 0 && K % diffuse_group == 0 && form == WF_SINGLE) {
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
    L->has_c1 = false;
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
        upload(c1h, &L->c1h);
        upload(c1f, &L->c1f);
        L->has_c1 = true;
    }
    upload(hi, &L->wh);
    upload(bias, &L->bias);
    L->has_32 = false;
    if (h->audit_weights || h->precision == JG_PREC_FP32 || keep32) {
        upload(w, &L->w32d);
        upload(bias, &L->b32d);
        L->has_32 = true;
    }
    L->has_lo = false;
    if (want_lo) { upload(lo, &L->lo); L->has_lo = true; }
    L->form = form;
    L->uncalibrated = starts_uncalibrated(form, kind);
    L->has_cal = false;
    if (form == WF_BIAS_CORRECTED) {
        m.bc_w32 = w; m.bc_b32 = bias; ++m.bc_records;          // m.bc.push_back({L, mu, 0, w, bias})
        L->has_cal = true;
    }
}

static std::vector<std::pair<int, int>> tap_order(int KH, int KW, int SH, int SW, bool reorder) {
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

struct T { std::vector<float> v; };          // a HostTensor as need() hands it out
// make_conv up to its call of pack_matrix: -> p [N][K], shift [N].  bn: the four BatchNorm tensors or nullptr ("bn.empty()")
static void make_conv(const T* w, const T* b, const T* const* bn, int O, int I, int KT, int KH, int KW, int slot, int kpad, int SH, int SW, bool reorder,
                      int Opad, std::vector<float>* p_out, std::vector<float>* shift_out, int* N_out, int* K_out) {
    std::vector<float> s(O, 1.f), shift(b->v);
    if (bn) {
        const T *g = bn[0], *be = bn[1], *mu = bn[2], *var = bn[3];
        for (int o = 0; o < O; ++o) {
            s[o] = g->v[o] / std::sqrt(var->v[o] + 1e-5f);
            shift[o] = (b->v[o] - mu->v[o]) * s[o] + be->v[o];
        }
    }
    const int K = kpad > 0 ? kpad : KH * KW * slot;
    const int N = Opad > O ? Opad : O;
    shift.resize(N, 0.f);
    std::vector<float> p((size_t)N * K, 0.f);
    const auto order = tap_order(KH, KW, SH, SW, reorder);
    for (int o = 0; o < O; ++o)
        for (int c = 0; c < I; ++c)
            for (int kt = 0; kt < KT; ++kt)
                for (size_t t = 0; t < order.size(); ++t) {
                    const int kh = order[t].first, kw = order[t].second;
                    const float v = w->v[((((size_t)o * I + c) * KT + kt) * KH + kh) * KW + kw] * s[o];
                    p[(size_t)o * K + t * slot + kt * I + c] = v;
                }
    *p_out = p; *shift_out = shift; *N_out = N; *K_out = K;
}

// apply_bias_corrections, between its two copies
static std::vector<float> bias_correction(const std::vector<float>& w32, const std::vector<float>& b32, const std::vector<float>& mu, long mu_rows, int N, int K) {
    std::vector<float> nb(N);
    const double inv = 1.0 / (double)mu_rows;
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        const float* wr = &w32[(size_t)n * K];
        for (int k = 0; k < K; ++k) acc += (double)(wr[k] - (float)(f16)wr[k]) * ((double)mu[k] * inv);
        nb[n] = b32[n] + (float)acc;
    }
    return nb;
}

// ------------------------------------------------------------------------------------ copied: xlmr.hip (finalize_xlmr's two folds)
static void fold_consumer(std::vector<float>& w, std::vector<float>& b, int N, int K, const std::vector<float>& g, const std::vector<float>& be) {
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        float* wr = &w[(size_t)n * K];
        for (int k = 0; k < K; ++k) {
            acc += (double)wr[k] * (double)be[k];
            wr[k] *= g[k];
        }
        b[n] = (float)((double)b[n] + acc);
    }
}
static void make_producer_bias(std::vector<float>& bb, int N, const std::vector<float>& be) {
    for (int n = 0; n < N; ++n) bb[n] += be[n];
}

// ------------------------------------------------------------------------------------ copied: gestsync.hip (finalize_gestsync's panel), shared.h
constexpr int CONV1_BIAS_LANE = 15;
constexpr float CONV1_BIAS_PAIR_SCALE = 9.765625e-04f;        // 2^-10
constexpr long conv1_wd_index(int slot, int ch, int e) { return (long)(slot * 64 + ch) * 16 + e; }
static std::vector<f16> conv1_panel(const std::vector<f16>& hostw, const std::vector<float>& shift) {
    std::vector<f16> wd((size_t)49 * 64 * 16);
    for (int s = 0; s < 49; ++s)
        for (int o = 0; o < 64; ++o)
            for (int e = 0; e < 16; ++e) wd[conv1_wd_index(s, o, e)] = hostw[(size_t)o * 784 + s * 16 + e];
    for (int o = 0; o < 64; ++o) {
        const float v = shift[o] * 255.0f * CONV1_BIAS_PAIR_SCALE;
        const f16 hi = (f16)v;
        wd[conv1_wd_index(0, o, CONV1_BIAS_LANE)] = hi;
        wd[conv1_wd_index(1, o, CONV1_BIAS_LANE)] = (f16)(v - (float)hi);
    }
    return wd;
}

// ------------------------------------------------------------------------------------ copied: gestsync_audio.hip (net_aud.conv1 by hand)
static void audio_conv1(const T* w, const T* b, const T* g, const T* be, const T* mu, const T* var, std::vector<float>* wf_out, std::vector<float>* shift_out) {
    std::vector<float> wf(64 * 9), shift(64);
    for (int o = 0; o < 64; ++o) {
        const float s = g->v[o] / std::sqrt(var->v[o] + 1e-5f);          // as make_conv folds
        for (int k = 0; k < 9; ++k) wf[o * 9 + k] = w->v[o * 9 + k] * s;
        shift[o] = (b->v[o] - mu->v[o]) * s + be->v[o];
    }
    *wf_out = wf; *shift_out = shift;
}

// ------------------------------------------------------------------------------------ inputs and output
static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static float uni(float lo, float hi) { return lo + (hi - lo) * ((float)(rnd() >> 8) * (1.0f / 16777216.0f)); }
static T tensor(size_t n, float lo, float hi) { T t; t.v.resize(n); for (auto& x : t.v) x = uni(lo, hi); return t; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static void put(const char* key, const std::vector<float>& v, bool comma = true) {
    std::printf("\"%s\":[", key);
    for (size_t i = 0; i < v.size(); ++i) { uint32_t u; std::memcpy(&u, &v[i], 4); std::printf("%s%u", i ? "," : "", u); }
    std::printf("]%s", comma ? "," : "");
}
static void put(const char* key, const std::vector<f16>& v, bool comma = true) {
    std::printf("\"%s\":[", key);
    for (size_t i = 0; i < v.size(); ++i) { uint16_t u; std::memcpy(&u, &v[i], 2); std::printf("%s%u", i ? "," : "", (unsigned)u); }
    std::printf("]%s", comma ? "," : "");
}
static void put_lin(const Lin& L) {          // what a packed layer left "on the device"
    put("hi", L.wh);
    if (L.has_lo) put("lo", L.lo); else std::printf("\"lo\":null,");
    if (L.has_c1) { put("c1h", L.c1h); put("c1f", L.c1f); }
    std::printf("\"w32_kept\":%d,\"form\":%d,\"uncalibrated\":%d,\"cal\":%d,", (int)L.has_32, (int)L.form, (int)L.uncalibrated, (int)L.has_cal);
    put("bias", L.bias, false);
}

static jg_handle handle(int precision, bool diffuse = true) {
    jg_handle h;
    h.precision = precision; h.bf16 = precision == JG_PREC_BF16; h.conv_round_diffuse = diffuse;
    return h;
}

int main() {
    // ---- rounding: N = 3, K = 5, every precision mode x layer kind x model x keep32
    const float p2_11 = 4.8828125e-4f, p2_24 = 5.9604644775390625e-8f;
    T w16; w16.v = {1.0f + p2_11, 1.0f + 3 * p2_11,         // exact fp16 ties (to even: down, up)
                    2.0f - p2_11 / 2,                        // rounds up into the next binade
                    1.5f * p2_24, 5.3f * p2_24, p2_24 / 4,   // fp16 subnormals: a tie, an ordinary one, one that rounds to zero
                    1.0f + 2 * p2_11 + 9.5367431640625e-7f,  // hi = 1 + 2^-10, lo = 2^-20: a subnormal lo
                    0.1f, 0.0f, -0.0f, -0.3337f, 30000.7f, -(1.0f + p2_11), 6.1e-5f, -7.123e-3f};
    const float p2_8 = 3.90625e-3f;
    T wbf; wbf.v = {1.0f + p2_8, 1.0f + 3 * p2_8,            // exact bf16 ties
                    2.0f - p2_8 / 4,                         // rounds up into the next binade
                    from_bits(0x7fc00001u), from_bits(0xff800001u),      // a quiet and a signalling NaN
                    1.5f * p2_24, 0.1f, 0.0f, -0.0f, -0.3337f, 30000.7f, -(1.0f + p2_8), 3.0e38f, 1.0e-40f, -7.123e-3f};
    const T b3 = tensor(3, -1.f, 1.f);
    std::printf("{\"round\":{"); put("w16", w16.v); put("wbf", wbf.v); put("bias", b3.v);
    std::printf("\"cases\":[\n");
    int n = 0;
    for (int mode = JG_PREC_FP16; mode <= JG_PREC_FP32; ++mode)
        for (int kind = LK_CONV; kind <= LK_XLMR; ++kind)
            for (int model = 1; model <= 3; ++model)
                for (int keep32 = 0; keep32 <= 1; ++keep32) {
                    jg_handle h = handle(mode);
                    Model m; m.id = model;
                    Lin L;
                    pack_matrix(&h, m, h.bf16 ? wbf.v : w16.v, b3.v, 3, 5, kind, &L, false, keep32 != 0, 0);
                    std::printf("%s{\"precision\":%d,\"kind\":%d,\"model\":%d,\"keep32\":%d,", n++ ? ",\n" : "", mode, kind, model, keep32);
                    put_lin(L);
                    std::printf("}");
                }
    std::printf("\n]},\n");

    // ---- diffusion: N = 2, slot 4, nine taps, two zero padding slots in the middle of a chain; K = 35 with group 4; a form other than single
    std::printf("\"diffuse\":[\n");
    {
        T w = tensor(2 * 36, -0.05f, 0.05f);
        w.v[0 * 36 + 3 * 4 + 1] = 0.f; w.v[0 * 36 + 4 * 4 + 1] = 0.f;       // chain (n 0, slot 1): taps 3 and 4
        w.v[1 * 36 + 5 * 4 + 2] = -0.f;                                      // and a negative zero in another
        const T b = tensor(2, -1.f, 1.f);
        const struct { int mode, K, group; } cs[3] = {{JG_PREC_FP16_RC, 36, 4}, {JG_PREC_FP16_RC, 35, 4}, {JG_PREC_FP16_W2_ALL, 36, 4}};
        for (int i = 0; i < 3; ++i) {
            jg_handle h = handle(cs[i].mode);
            Model m;
            Lin L;
            T wk = w; wk.v.resize((size_t)2 * cs[i].K);
            pack_matrix(&h, m, wk.v, b.v, 2, cs[i].K, LK_CONV, &L, false, false, cs[i].group);
            std::printf("%s{\"precision\":%d,\"kind\":0,\"model\":1,\"N\":2,\"K\":%d,\"group\":%d,", i ? ",\n" : "", cs[i].mode, cs[i].K, cs[i].group);
            put("w", wk.v); put("b", b.v); put_lin(L);
            std::printf("}");
        }
    }
    std::printf("\n],\n");

    // ---- conv matrix: seven shapes
    std::printf("\"conv\":[\n");
    {
        const struct { const char* tag; int O, I, KT, KH, KW, slot, kpad, SH, SW, reorder, Opad, bn; } cs[8] = {
            {"natural", 3, 2, 1, 3, 3, 2, 0, 1, 1, 0, 0, 1},
            {"reorder_2x2", 3, 2, 1, 3, 3, 2, 0, 2, 2, 1, 0, 1},
            {"reorder_1x2", 3, 2, 1, 3, 3, 2, 0, 1, 2, 1, 0, 1},
            {"7x7_reorder_stays_natural", 2, 1, 1, 7, 7, 1, 0, 3, 3, 1, 0, 1},
            {"conv1_form", 2, 3, 5, 2, 2, 16, 0, 1, 1, 0, 0, 1},
            {"kpad", 3, 1, 1, 5, 5, 1, 32, 1, 1, 0, 0, 1},
            {"opad", 3, 2, 1, 3, 3, 2, 0, 1, 1, 0, 4, 1},
            {"no_bn", 3, 2, 1, 3, 3, 2, 0, 1, 1, 0, 0, 0}};
        for (int i = 0; i < 8; ++i) {
            const auto& c = cs[i];
            const T w = tensor((size_t)c.O * c.I * c.KT * c.KH * c.KW, -0.5f, 0.5f), b = tensor(c.O, -1.f, 1.f);
            const T g = tensor(c.O, 0.5f, 1.5f), be = tensor(c.O, -0.5f, 0.5f), mu = tensor(c.O, -0.5f, 0.5f), var = tensor(c.O, 0.1f, 2.f);
            const T* bn[4] = {&g, &be, &mu, &var};
            std::vector<float> p, shift;
            int N, K;
            make_conv(&w, &b, c.bn ? bn : nullptr, c.O, c.I, c.KT, c.KH, c.KW, c.slot, c.kpad, c.SH, c.SW, c.reorder != 0, c.Opad, &p, &shift, &N, &K);
            std::printf("%s{\"tag\":\"%s\",\"O\":%d,\"I\":%d,\"KT\":%d,\"KH\":%d,\"KW\":%d,\"slot\":%d,\"kpad\":%d,\"SH\":%d,\"SW\":%d,\"reorder\":%d,\"Opad\":%d,\"N\":%d,\"K\":%d,",
                        i ? ",\n" : "", c.tag, c.O, c.I, c.KT, c.KH, c.KW, c.slot, c.kpad, c.SH, c.SW, c.reorder, c.Opad, N, K);
            put("w", w.v); put("b", b.v);
            if (c.bn) { put("gamma", g.v); put("beta", be.v); put("mean", mu.v); put("var", var.v); }
            put("matrix", p); put("shift", shift, false);
            std::printf("}");
        }
    }
    std::printf("\n],\n");

    // ---- net_aud.conv1 by hand: O = 64, 3 x 3, I = 1
    {
        const T w = tensor(64 * 9, -0.5f, 0.5f), b = tensor(64, -1.f, 1.f), g = tensor(64, 0.5f, 1.5f), be = tensor(64, -0.5f, 0.5f),
                mu = tensor(64, -0.5f, 0.5f), var = tensor(64, 0.1f, 2.f);
        std::vector<float> wf, shift;
        audio_conv1(&w, &b, &g, &be, &mu, &var, &wf, &shift);
        std::printf("\"audio_conv1\":{");
        put("w", w.v); put("b", b.v); put("gamma", g.v); put("beta", be.v); put("mean", mu.v); put("var", var.v); put("matrix", wf); put("shift", shift, false);
        std::printf("},\n");
    }

    // ---- LayerNorm folds: consumer + column sums at N = 4, K = 6 in single fp16, hi + lo and bf16; the producer's bias
    std::printf("\"ln_consumer\":[\n");
    {
        const T w = tensor(4 * 6, -0.5f, 0.5f), b = tensor(4, -1.f, 1.f), g = tensor(6, 0.5f, 1.5f), be = tensor(6, -0.5f, 0.5f);
        const int modes[3] = {JG_PREC_FP16, JG_PREC_FP16_W2, JG_PREC_BF16};
        for (int i = 0; i < 3; ++i) {
            jg_handle h = handle(modes[i]);
            Model m; m.id = 3;
            Lin L;
            std::vector<float> wf = w.v, bf = b.v;
            fold_consumer(wf, bf, 4, 6, g.v, be.v);
            pack_matrix(&h, m, wf, bf, 4, 6, LK_XLMR, &L, true, false, 0);
            std::printf("%s{\"precision\":%d,\"kind\":3,\"model\":3,\"N\":4,\"K\":6,", i ? ",\n" : "", modes[i]);
            put("w", w.v); put("b", b.v); put("gamma", g.v); put("beta", be.v); put("w_folded", wf); put_lin(L);
            std::printf("}");
        }
    }
    std::printf("\n],\n");
    {
        const T b = tensor(4, -1.f, 1.f), be = tensor(4, -0.5f, 0.5f);
        std::vector<float> bb = b.v;
        make_producer_bias(bb, 4, be.v);
        std::printf("\"ln_producer\":{"); put("b", b.v); put("beta", be.v); put("bias", bb, false);
        std::printf("},\n");
    }

    // ---- conv1 direct panel: hi [64][784] by an integer rule (finite fp16 patterns; lane 15 of every slot zero, as conv1 packs it, but
    // for slots 5 and 40, so that "what the old loop left on the bias lane of slots 2 .. 48" is visible), shift [64] recorded
    {
        std::vector<f16> hostw((size_t)64 * 784);
        for (size_t i = 0; i < hostw.size(); ++i) {
            const unsigned s = (unsigned)(i % 784) / 16, e = (unsigned)i % 16;
            uint16_t u = (uint16_t)(((uint32_t)i * 40503u) >> 4);
            if ((u & 0x7c00u) == 0x7c00u) u &= 0xbfffu;       // no inf / NaN patterns
            if (e == 15 && s != 5 && s != 40) u = 0;
            std::memcpy(&hostw[i], &u, 2);
        }
        T shift = tensor(64, -3.f, 3.f);
        shift.v[7] = 0.f; shift.v[9] = 0.25f;                 // a zero bias and one whose lo half is zero
        const std::vector<f16> wd = conv1_panel(hostw, shift.v);
        uint64_t fnv = 0xcbf29ce484222325ull;                 // FNV-1a 64 over the panel's little-endian bytes
        std::vector<f16> pair0(64), pair1(64);
        for (size_t i = 0; i < wd.size(); ++i) {
            uint16_t u;
            std::memcpy(&u, &wd[i], 2);
            fnv = (fnv ^ (u & 0xffu)) * 0x100000001b3ull;
            fnv = (fnv ^ (u >> 8)) * 0x100000001b3ull;
        }
        for (int o = 0; o < 64; ++o) { pair0[o] = wd[conv1_wd_index(0, o, CONV1_BIAS_LANE)]; pair1[o] = wd[conv1_wd_index(1, o, CONV1_BIAS_LANE)]; }
        std::printf("\"panel\":{\"hi_rule\":\"u16((i * 40503 mod 2^32) >> 4), exponent 31 cleared of bit 14, lane 15 zero but in slots 5 and 40\",");
        put("shift", shift.v); put("bias_hi", pair0); put("bias_lo", pair1);
        std::printf("\"fnv1a64\":\"%016llx\"},\n", (unsigned long long)fnv);
    }

    // ---- bias correction: N = 3, K = 5, rows = 7
    {
        const T w = tensor(15, -0.5f, 0.5f), b = tensor(3, -1.f, 1.f), mu = tensor(5, -20.f, 20.f);
        const std::vector<float> nb = bias_correction(w.v, b.v, mu.v, 7, 3, 5);
        std::printf("\"bias_correction\":{\"rows\":7,"); put("w32", w.v); put("b32", b.v); put("mu", mu.v); put("bias", nb, false);
        std::printf("}}\n");
    }
    return 0;
}
