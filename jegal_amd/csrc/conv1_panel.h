// conv1's weight panel: the layout and the bias-lane constants that the host packing (weight_pack.hip) and conv1's kernels (conv1.hip,
// through shared.h) share.  No HIP header: a plain C++ compiler reads it as well.
#pragma once

#if defined(__HIPCC__)
#define JG_PANEL_FN __host__ __device__ inline __attribute__((always_inline)) constexpr
#else
#define JG_PANEL_FN inline constexpr
#endif

// conv1's weight panel Wd[slot][ch][16] (49 pixel slots (kh, kw), 64 output channels, 16 halves: 5 frames x 3 colours and the pad
// lane CONV1_BIAS_LANE, which the kernel feeds 1.0): the BN-folded weights, and on the pad lane of slots 0 / 1 the hi / lo halves
// of the channel's bias.
// The pixels reach the MFMA as the fp16 subnormals n 2^-24; the pad lane's "1.0" is 2^-14 (CONV1_BIAS_ONE, the smallest NORMAL fp16)
// and the pair holds 255 shift 2^-10 (CONV1_BIAS_PAIR_SCALE), so the product is 255 shift 2^-24 as it must be.  Not 2^-24 times
// 255 shift: the MFMA aligns the products of a k-step by their operands' exponent FIELDS and keeps 24 bits below the largest; a
// subnormal 2^-24 has the field of 2^-14, the product with a bias of 2^7 sat ten bits above its value and pushed the low bits of
// the step's pixel products out of the window (tests/test_gpu_conv1_fp64.py, tier B: up to 20 % of a channel's outputs one fp16 ulp
// off, none with a zero bias).
constexpr int CONV1_BIAS_LANE = 15;
constexpr unsigned CONV1_BIAS_ONE_BITS = 0x0400u;              // fp16 2^-14
constexpr float CONV1_BIAS_ONE = 6.103515625e-05f;            // 2^-14
constexpr float CONV1_BIAS_PAIR_SCALE = 9.765625e-04f;        // 2^-10 = 2^-24 / CONV1_BIAS_ONE
JG_PANEL_FN long conv1_wd_index(int slot, int ch, int e) { return (long)(slot * 64 + ch) * 16 + e; }
static_assert(conv1_wd_index(0, 0, CONV1_BIAS_LANE) == 15 && conv1_wd_index(1, 2, 3) == 1059 && conv1_wd_index(48, 63, 15) == 49 * 64 * 16 - 1, "conv1 weight panel");
#undef JG_PANEL_FN
