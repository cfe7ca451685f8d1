// The precision contract of libjegal_hip in one place: which weights a packed layer's GEMM runs with.
//
// weight_form() decides once, when a matrix is packed (pack_host, linear.hip), from the handle's precision mode, the layer's kind and
// the model; runs_with_lo() answers at every launch whether the GEMM takes the lo half as a second operand.  The host units ask these
// two (through run_lo, engine.h) instead of reading pointers, and jg_debug_weight_form / jg_debug_gemm_runs_lo (checks.hip) show the
// answers on a machine without a GPU.  Pure: no HIP, no handle, no pointer, no state.
#pragma once
#include "../../include/jegal_hip.h"

namespace engine {

// layer kinds: which precision treatment a matrix gets under the handle's mode
enum { LK_CONV = 0, LK_GESTURE = 1, LK_CONTENT = 2, LK_XLMR = 3 };      // LK_XLMR: bias-corrected like the gesture path (calibrated on token ids)

enum WeightForm {
    WF_SINGLE = 0,              // single 16-bit weights
    WF_SPLIT = 1,               // hi + lo fp16 pair, two MFMAs per fragment
    // single fp16 + the systematic part of the weight-rounding error, (w - fp16(w)) . E[x], folded into the bias by a calibration pass
    // that runs hi+lo and records the mean of the layer's input (linear.hip, "bias-corrected precision")
    WF_BIAS_CORRECTED = 2,
    // single fp16 + a per-clip bias built at every call from the clip's own rows and the lo half (gemm(), linear.hip); hi+lo wherever
    // that epilogue is not available
    WF_RUNTIME_CORRECTED = 3,
};

// model_id: 1 GestSync, 2 JEGAL, 3 XLM-RoBERTa (Model::id)
inline WeightForm weight_form(int precision, int kind, int model_id) {
    const bool conv = kind == LK_CONV;
    switch (precision) {
        case JG_PREC_FP16_W2: return conv ? WF_SINGLE : WF_SPLIT;
        case JG_PREC_FP16_W2_ALL: return WF_SPLIT;
        case JG_PREC_FP16_BC: return conv ? WF_SINGLE : kind == LK_CONTENT ? WF_SPLIT : WF_BIAS_CORRECTED;
        // GestSync's Linears are run-time corrected; the JEGAL gesture branch (M = B*T rows: launch-bound, a 256-row tile meets
        // several clips) and the content path keep hi+lo; XLM-RoBERTa as in JG_PREC_FP16_BC
        case JG_PREC_FP16_RC:
            if (conv) return WF_SINGLE;
            if (kind == LK_XLMR) return WF_BIAS_CORRECTED;
            return kind == LK_GESTURE && model_id == 1 ? WF_RUNTIME_CORRECTED : WF_SPLIT;
        default: return WF_SINGLE;      // JG_PREC_FP16, JG_PREC_BF16, JG_PREC_FP32
    }
}

// Is the lo matrix kept on the device.  keep32: the layer also runs on the split-operand kernel (gemm_x3) whatever its form
inline bool lo_kept(WeightForm f, bool keep32) { return f != WF_SINGLE || keep32; }

// A bias-corrected layer that nothing calibrates implicitly (XLM-RoBERTa: the released checkpoint has strong outlier activation
// dimensions; bias corrections recorded on made-up ids were never validated for it) runs hi+lo until jg_calibrate_xlmr has seen the
// caller's token ids
inline bool starts_uncalibrated(WeightForm f, int kind) { return f == WF_BIAS_CORRECTED && kind == LK_XLMR; }

// Does a GEMM on a layer of form `f` run with the lo operand.  uncalibrated: Lin::uncalibrated; calibrating: a calibration pass is in
// progress (jg_handle::calib); clip_bias: this call takes the per-clip bias.  A site that asks ahead of a launch asks in the form
// that launch will take.
inline bool runs_with_lo(WeightForm f, bool uncalibrated, bool calibrating, bool clip_bias) {
    switch (f) {
        case WF_SPLIT: return true;
        case WF_BIAS_CORRECTED: return uncalibrated || calibrating;
        case WF_RUNTIME_CORRECTED: return !clip_bias;
        default: return false;
    }
}

}  // namespace engine
