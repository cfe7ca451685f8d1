// Weight packing of libjegal_hip, the arithmetic alone: what a layer's tensors become before anything is uploaded.
//
// Plain functions over host arrays -- no HIP, no handle, no Model, no Lin.  The host units (linear.hip, the finalize_* functions) fetch
// tensors, call these and hand the result to the one upload step (upload_layer, linear.hip); jg_debug_pack_* / jg_debug_conv1_panel /
// jg_debug_bias_correction (checks.hip) run the same functions on caller arrays on a machine without a GPU.  16-bit values are uint16_t
// bit containers; fp16 conversions go through the host's _Float16.  Every float operation keeps the type and order it is written in:
// the device bytes of every layer depend on it (tests/test_weight_pack_cpu.py pins them to the text these functions replaced).
#pragma once
#include "conv1_panel.h"
#include "weight_form.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace engine {

// fp32 -> bf16 bits, round to nearest even; a NaN keeps its sign and top payload bits and is made quiet
inline uint16_t bf16_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_value(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
inline uint16_t f16_bits(_Float16 v) {
    uint16_t b;
    std::memcpy(&b, &v, 2);
    return b;
}
inline _Float16 f16_value(uint16_t b) {
    _Float16 v;
    std::memcpy(&v, &b, 2);
    return v;
}

// Eval BatchNorm behind a conv, folded: scale[o] = gamma / sqrt(var + 1e-5), shift[o] = (bias - mean) scale + beta, in float
void bn_fold(const float* bias, const float* gamma, const float* beta, const float* mean, const float* var, int O, float* scale, float* shift);

// Tap order of a conv layer's K axis: natural (kh, kw) or, for strided layers run with `reorder`, grouped by parity class
// (kh % SH, kw % SW) -- see ConvGeom::taps.  Used by BOTH the weight packing and the geometry (geom(), linear.hip).
std::vector<std::pair<int, int>> tap_order(int KH, int KW, int SH, int SW, bool reorder);

// conv weight [O][I][KT][KH][KW] times scale[o] -> [N][K] fp32 with k = t * slot + (kt * I + c), t the tap's place in tap_order;
// slot = channels per (kh, kw) position after padding (16 for conv1's 5 x 3 temporal stack, I otherwise; needs KT I <= slot),
// K = kpad > 0 ? kpad : KH KW slot (needs KH KW slot <= K), N = max(O, Opad): rows O .. N - 1 and every k no tap reaches are zero
struct ConvPack { int O, I, KT, KH, KW, slot, kpad, Opad, SH, SW; bool reorder; };
inline int conv_pack_K(const ConvPack& c) { return c.kpad > 0 ? c.kpad : c.KH * c.KW * c.slot; }
inline int conv_pack_N(const ConvPack& c) { return c.Opad > c.O ? c.Opad : c.O; }
std::vector<float> conv_matrix(const float* w, const float* scale, const ConvPack& c);

// How a matrix is rounded to 16 bits.  The caller derives it from weight_form() / lo_kept() and its own options.
// diffuse_group > 0 (conv layers, option conv_round_diffuse): fp16 rounding with ERROR DIFFUSION along the taps of one (output channel,
// input slot) pair -- k = tap * diffuse_group + slot -- instead of round-to-nearest per weight: the residuals w - fp16(w) of a
// channel's taps then sum to less than half an ulp, so the part of the weight-rounding error that is the same for every output pixel,
// sum_k (w - fp16(w))[k] E[x_k] = sum_slot E[x_slot] sum_taps (w - fp16(w)), vanishes wherever the input statistics do not depend on the
// tap (everywhere but at the image border); the price is a per-weight residual of up to one ulp instead of half an ulp in the part
// that averages out over pixels.  No calibration, no run-time cost (measured with tools/precision_floor.py).
// It applies to single fp16 weights whose K is a multiple of the group; everything else rounds to nearest.
struct RoundRule {
    bool bf16;              // single bf16 weights (JG_PREC_BF16); a kept lo half is all zero
    WeightForm form;
    bool keep_lo;           // lo_kept(form, keep32)
    int diffuse_group;
};
// [N][K] fp32 -> hi bits and, with rule.keep_lo, lo bits: lo = fp16(w - float(hi)) where the matrix rounds to nearest in fp16, zero elsewhere
void round_matrix(const float* w, int N, int K, const RoundRule& rule, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo);

// Column sums of the weights AS PACKED (Lin::c1h / c1f): of hi alone and of hi + lo (lo may be empty), summed in double
void column_sums(const uint16_t* hi, const uint16_t* lo, int N, int K, bool bf16, float* c1h, float* c1f);

// Implicit LayerNorm(gamma, beta) (xlmr_encode_folded).  Consumer, the Linear BEHIND the LayerNorm: w <- w diag(gamma), b <- b + w beta
// (the old w; summed in double, rounded once).  Producer, the Linear whose output is ADDED to the LayerNorm's output: b <- b + beta.
void fold_ln_consumer(float* w, float* b, int N, int K, const float* gamma, const float* beta);
void fold_ln_producer(float* b, int N, const float* beta);

// Slot-major copy of the packed conv1 matrix for conv1_direct_kernel: Wd[s][o][e] = W[o][s * 16 + e] from hi [64][784], and on the
// bias lane of slots 0 / 1 the hi / lo fp16 pair of shift[o] * 255 * CONV1_BIAS_PAIR_SCALE (conv1_panel.h).  -> [49 * 64 * 16]
constexpr int CONV1_PANEL_O = 64, CONV1_PANEL_SLOTS = 49, CONV1_PANEL_K = CONV1_PANEL_SLOTS * 16;
std::vector<uint16_t> conv1_direct_panel(const uint16_t* hi, const float* shift);

// Bias of a bias-corrected layer after a calibration: b32[n] + sum_k (w32 - fp16(w32))[n][k] * (mu[k] / rows), mu the column sums
// of the layer's input over `rows` rows; the sum in double
void bias_correction(const float* w32, const float* b32, const float* mu, long rows, int N, int K, float* bias);

// One packed layer, everything the upload step needs
struct PackedLayer {
    int N = 0, K = 0;
    WeightForm form = WF_SINGLE;
    bool uncalibrated = false;
    std::vector<uint16_t> hi, lo;       // lo empty: not kept
    std::vector<float> bias;
    std::vector<float> c1h, c1f;        // implicit-LayerNorm consumers only
    // the fp32 matrix and bias as packed, when something keeps them: the device (device32: the fp32 kernels / the audit path) and / or
    // the calibration record of a bias-corrected layer
    std::vector<float> w32, b32;
    bool device32 = false;
};
// w [N][K], bias [N] as the layer runs them (BatchNorm / LayerNorm already folded).  ln_consumer: the column sums are wanted;
// device32: the layer also keeps its fp32 matrix on the device
PackedLayer pack_layer(const float* w, const float* bias, int N, int K, const RoundRule& rule, bool uncalibrated, bool ln_consumer, bool device32);

}  // namespace engine
