// libjegal_hip: weight packing, the arithmetic (weight_pack.h).  Host code only, no HIP: any C++17 compiler with _Float16 builds it.
#include "weight_pack.h"

#include <cmath>

namespace engine {

void bn_fold(const float* bias, const float* gamma, const float* beta, const float* mean, const float* var, int O, float* scale, float* shift) {
    for (int o = 0; o < O; ++o) {
        scale[o] = gamma[o] / std::sqrt(var[o] + 1e-5f);
        shift[o] = (bias[o] - mean[o]) * scale[o] + beta[o];
    }
}

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

std::vector<float> conv_matrix(const float* w, const float* scale, const ConvPack& c) {
    const int K = conv_pack_K(c), N = conv_pack_N(c);
    std::vector<float> p((size_t)N * K, 0.f);
    const auto order = tap_order(c.KH, c.KW, c.SH, c.SW, c.reorder);
    for (int o = 0; o < c.O; ++o)
        for (int ch = 0; ch < c.I; ++ch)
            for (int kt = 0; kt < c.KT; ++kt)
                for (size_t t = 0; t < order.size(); ++t) {
                    const int kh = order[t].first, kw = order[t].second;
                    const float v = w[((((size_t)o * c.I + ch) * c.KT + kt) * c.KH + kh) * c.KW + kw] * scale[o];
                    p[(size_t)o * K + t * c.slot + kt * c.I + ch] = v;
                }
    return p;
}

void round_matrix(const float* w, int N, int K, const RoundRule& rule, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo) {
    const size_t n_el = (size_t)N * K;
    hi.assign(n_el, 0);
    lo.assign(rule.keep_lo ? n_el : 0, 0);
    if (rule.bf16) {
        for (size_t i = 0; i < n_el; ++i) hi[i] = bf16_bits(w[i]);
    } else if (rule.diffuse_group > 0 && K % rule.diffuse_group == 0 && rule.form == WF_SINGLE) {
        const int group = rule.diffuse_group, taps = K / group;
        for (int n = 0; n < N; ++n)
            for (int sl = 0; sl < group; ++sl) {
                double carry = 0.0;
                for (int t = 0; t < taps; ++t) {
                    const size_t i = (size_t)n * K + (size_t)t * group + sl;
                    if (w[i] == 0.f) continue;        // padding slots stay exactly zero (and leave the carry alone)
                    const double v = (double)w[i] + carry;
                    const _Float16 a = (_Float16)(float)v;
                    hi[i] = f16_bits(a);
                    carry = v - (double)(float)a;
                }
            }
    } else {
        for (size_t i = 0; i < n_el; ++i) {
            const _Float16 a = (_Float16)w[i];
            hi[i] = f16_bits(a);
            if (rule.keep_lo) lo[i] = f16_bits((_Float16)(w[i] - (float)a));
        }
    }
}

void column_sums(const uint16_t* hi, const uint16_t* lo, int N, int K, bool bf16, float* c1h, float* c1f) {
    for (int n = 0; n < N; ++n) {
        double sh = 0.0, sl = 0.0;
        for (int k = 0; k < K; ++k) {
            const size_t i = (size_t)n * K + k;
            if (bf16) {
                sh += (double)bf16_value(hi[i]);
            } else {
                sh += (double)(float)f16_value(hi[i]);
                if (lo) sl += (double)(float)f16_value(lo[i]);
            }
        }
        c1h[n] = (float)sh;
        c1f[n] = (float)(sh + sl);
    }
}

void fold_ln_consumer(float* w, float* b, int N, int K, const float* gamma, const float* beta) {
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        float* wr = &w[(size_t)n * K];
        for (int k = 0; k < K; ++k) {
            acc += (double)wr[k] * (double)beta[k];
            wr[k] *= gamma[k];
        }
        b[n] = (float)((double)b[n] + acc);
    }
}

void fold_ln_producer(float* b, int N, const float* beta) {
    for (int n = 0; n < N; ++n) b[n] += beta[n];
}

std::vector<uint16_t> conv1_direct_panel(const uint16_t* hi, const float* shift) {
    std::vector<uint16_t> wd((size_t)CONV1_PANEL_SLOTS * CONV1_PANEL_O * 16);
    for (int s = 0; s < CONV1_PANEL_SLOTS; ++s)
        for (int o = 0; o < CONV1_PANEL_O; ++o)
            for (int e = 0; e < 16; ++e) wd[conv1_wd_index(s, o, e)] = hi[(size_t)o * CONV1_PANEL_K + s * 16 + e];
    // bias lane: the kernel sets element CONV1_BIAS_LANE of every pixel slot to "1.0" = CONV1_BIAS_ONE; shift * 255 (times the power
    // of two CONV1_BIAS_PAIR_SCALE that makes the product shift * 255 * 2^-24, conv1_panel.h) as hi + lo fp16 pair
    for (int o = 0; o < CONV1_PANEL_O; ++o) {
        const float v = shift[o] * 255.0f * CONV1_BIAS_PAIR_SCALE;
        const _Float16 h = (_Float16)v;
        wd[conv1_wd_index(0, o, CONV1_BIAS_LANE)] = f16_bits(h);
        wd[conv1_wd_index(1, o, CONV1_BIAS_LANE)] = f16_bits((_Float16)(v - (float)h));
    }
    return wd;
}

void bias_correction(const float* w32, const float* b32, const float* mu, long rows, int N, int K, float* bias) {
    const double inv = 1.0 / (double)rows;
    for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        const float* wr = &w32[(size_t)n * K];
        for (int k = 0; k < K; ++k) acc += (double)(wr[k] - (float)(_Float16)wr[k]) * ((double)mu[k] * inv);
        bias[n] = b32[n] + (float)acc;
    }
}

PackedLayer pack_layer(const float* w, const float* bias, int N, int K, const RoundRule& rule, bool uncalibrated, bool ln_consumer, bool device32) {
    PackedLayer p;
    p.N = N; p.K = K;
    p.form = rule.form;
    p.uncalibrated = uncalibrated;
    round_matrix(w, N, K, rule, p.hi, p.lo);
    if (ln_consumer) {
        p.c1h.resize(N); p.c1f.resize(N);
        column_sums(p.hi.data(), p.lo.empty() ? nullptr : p.lo.data(), N, K, rule.bf16, p.c1h.data(), p.c1f.data());
    }
    p.bias.assign(bias, bias + N);
    p.device32 = device32;
    if (device32 || rule.form == WF_BIAS_CORRECTED) {
        p.w32.assign(w, w + (size_t)N * K);
        p.b32.assign(bias, bias + N);
    }
    return p;
}

}  // namespace engine
