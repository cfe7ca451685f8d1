"""Cases, rule and oracle of tests/test_gpu_precision_budget.py (host only; tests/test_precision_budget_cases_cpu.py checks them without
a GPU).

Every 16-bit mode holds the 1e-3 contract because four remedies sit on plain fp16 operands: the run-time correction
(JG_PREC_FP16_RC), the calibrated bias (JG_PREC_FP16_BC), the split-operand ends of the JEGAL branch (option jegal_fp32_ends) and the error
diffusion of the conv weights (option conv_round_diffuse).  A remedy that silently does nothing costs about 2^-12 per product: two to three
times below anything a whole-path bound can see.  So each remedy is measured ALONE -- the stage it acts on is the only one left in 16-bit,
option audit_stages moves the others to the fp32 kernels -- and against the costlier arithmetic it imitates.

Shapes (B, T): 21 B T token rows, 21 T rows per clip.
  (2, 26)   1 092 rows, 546 per clip: below 1 024 per clip, every row of a clip enters its mean (rc_rows_sampled, elementwise_fp16.hip)
  (1, 52)   1 092 rows per clip: from 1 024 on the mean comes from the 16-row runs at every 128th row (9 runs here)
Both have >= 1 024 rows in all (the LayerNorm-fused plan, the only one with the per-clip bias: GEMM_LN_FUSED_MIN_ROWS and gemm(),
linear.hip), >= 256 rows per clip (GEMM_CLIP_MIN_RPC) and B < 8 (one lane); both have the same 1 092 rows, so the two differ in
nothing but where the mean comes from.  (1, 48), 1 008 rows, is the longest single clip the fused plan refuses.  Cost of the oracle per
shape and family on the CPU: 1.2 s for the fp32 conv stack and the fp32 features, 0.5 s for float64 behind the conv stack.
"""
import numpy as np
import torch

import jegal_oracle as O
from jegal_amd import synth

SHAPES = ((2, 26), (1, 52))
ROLE = {(2, 26): "all rows in the mean", (1, 52): "sampled mean"}
TOO_SHORT = (1, 48)                     # 1 008 token rows: the planner refuses the LayerNorm-fused form, the call runs hi+lo
FAMILIES = (("gauss", 0), ("gauss", 1), ("heavy", 0))          # synth._Gen families, as in test_gpu_weight_families.py
FRAMES_SEED = 1234
S = 21                                  # tokens per window (25 frames - 4)
RC_SAMPLE_FROM_RPC = 1024               # rc_rows_sampled: every row below, the 16-row runs at every 128th row from here on
AUD_TOL = 2e-5                          # the fp32 audit kernels against the fp32 oracle (test_gpu_audit_fp32.py)

# option audit_stages: the stages on the fp32 kernels (include/jegal_hip.h).  The stage left in 16-bit is the one under test.
ONLY_CONV, ONLY_GESTSYNC, ONLY_JEGAL, NONE_16BIT, ALL_16BIT = 6, 5, 3, 7, 0
# option audit_jegal_parts under ONLY_JEGAL: attention and feed-forward sub-layers on the fp32 kernels, i.e. only the two ends remain
ONLY_ENDS, ALL_PARTS = 6, 15

# The residual share of removable error energy a remedy may leave (rho_max; None: reported, `on < off` asserted).  From the T = 150
# records, not from this code at these shapes: diffusion with the conv stack isolated leaves 0.06 / 0.19 / 0.45 on gauss+0 / gauss+1 /
# heavy+0 (0.5 = "at least half of the removable energy is gone", which heavy+0 only just meets: reported); the run-time correction has
# on / ideal = 1.04 - 1.07 with off about 4 - 5 x ideal (profiles/r6_rc_ablation.txt), rho about 0.01 - 0.04; the split-operand ends
# are fp32-grade, rho near 0.
RHO_MAX = {"runtime_correction": 0.1, "calibrated_bias": None, "split_ends": 0.1, "conv_diffusion": 0.5}
REPORTED_ONLY = {("conv_diffusion", "heavy+0")}
QUADRATURE_TOL = 0.25                   # the T = 150 records agree to 0.4 - 3.4 %; a mask bit that fails to isolate moves a term by 100 %


def fam_id(f):
    return f"{f[0]}+{f[1]}"


def shape_id(s):
    return f"B{s[0]}xT{s[1]}"


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------------------ the rule
class CaseIsBlind(AssertionError):
    """off^2 < 2 ideal^2: at this shape / isolation the remedy has too little to remove for the case to see it.  Replace the case."""


def rho(ideal, on, off):
    """The residual share of removable error energy, (on^2 - ideal^2) / (off^2 - ideal^2): three errors against the same oracle on the same
    input -- ideal: the costlier arithmetic the remedy imitates, on: the remedy as shipped, off: switched off.  0: the remedy is as good
    as what it imitates; 1: it does nothing.  Precondition (asserted): off^2 >= 2 ideal^2."""
    ideal, on, off = float(ideal), float(on), float(off)
    if not (np.isfinite([ideal, on, off]).all() and ideal >= 0 and on >= 0 and off >= 0):
        raise AssertionError(f"errors must be finite and non-negative: ideal {ideal}, on {on}, off {off}")
    if not off * off >= 2 * ideal * ideal or off == 0:
        raise CaseIsBlind(f"off {off:.3e} is within sqrt(2) of ideal {ideal:.3e}: nothing to remove, the case cannot see the remedy")
    return (on * on - ideal * ideal) / (off * off - ideal * ideal)


def check_remedy(ideal, on, off, rho_max):
    """-> rho; asserts what the table of test_gpu_precision_budget.py asserts of one triple (rho_max None: on < off only)."""
    r = rho(ideal, on, off)
    assert on < off, f"the remedy does not reduce the error: on {on:.3e} >= off {off:.3e} (ideal {ideal:.3e})"
    if rho_max is not None:
        assert r <= rho_max, f"rho {r:.3f} > {rho_max}: ideal {ideal:.3e} on {on:.3e} off {off:.3e}"
    return r


def quadrature(parts):
    return float(np.sqrt(sum(float(p) ** 2 for p in parts)))


def check_quadrature(whole, parts, tol=QUADRATURE_TOL):
    """Independent stages: e(none)^2 ~ sum of the single-stage errors squared.  -> relative deviation of the sum from `whole`."""
    q = quadrature(parts)
    dev = abs(q - whole) / whole
    assert dev <= tol, f"single-stage errors {['%.3e' % p for p in parts]} give {q:.3e} in quadrature, the whole path {whole:.3e}: off by {dev:.1%}"
    return dev


# ------------------------------------------------------------------------------------------------ the graph the launch count is derived from
# GestSync's transformer + ff_vid on the clip path (gs_transformer / gestsync_clip_impl, gestsync.hip), per Linear: (name, N, K, LayerNorm
# fused into the epilogue, ReLU, A is the tiled token plane)
LAYER_LINEARS = (("qkv", 1536, 512, False, 0, True), ("out_proj", 512, 512, True, 0, False), ("linear1", 2048, 512, False, 1, True),
                 ("linear2", 512, 2048, True, 0, False))
FF_VID0 = ("ff_vid.0", 512, 512, False, 1, True)


def corrected_linears(T):
    """The Linear launches of one gestsync_clip pass that take the per-clip bias in the fused plan: four per layer, less layer 0's qkv (by
    linearity it runs over the distinct conv positions and the positional rows: no clip rows, no bias -- from T > 1), plus ff_vid.0;
    ff_vid.2 runs on the window means (B T rows).  24 for T > 1."""
    return [f"layers.{l}.{n[0]}" for l in range(6) for n in LAYER_LINEARS if not (l == 0 and n[0] == "qkv" and T > 1)] + [FF_VID0[0]]


# Engine.profile counts one record per bracketed step, and gemm() (linear.hip) brackets the correction's two kernels (rc_col_mean_kernel,
# rc_gemv_kernel: launch_rc_bias) as ONE step of stage "gemm" in front of the GEMM it corrects
PROFILE_RECORDS_PER_CORRECTION = 1
KERNELS_PER_CORRECTION = 2


def plan_fields(B, T, linear, clip_bias=True):
    """jg_gemm_check fields of `linear` (an entry of LAYER_LINEARS / FF_VID0) at (B, T) as the fused plan asks the planner
    (gs_fused_plan, gestsync.hip), in the per-clip-bias form"""
    _, N, K, ln, relu, tiled = linear
    M = B * T * S
    f = dict(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, bias=True, out16=True, relu=relu, a_tiled=tiled)
    if ln:
        f.update(ln_w=True, ln_b=True, res16=True)
    if clip_bias:
        f.update(bias_clip=True, rpc=T * S, nclips=B)
    return f


# ------------------------------------------------------------------------------------------------ the oracle
def frames_of(B, T):
    return synth.synth_frames(FRAMES_SEED, B, T)


def state_dicts(family):
    name, off = family
    return (synth.gestsync_state_dict(seed=synth.GESTSYNC_SEED + off, include_unused=False, family=name),
            synth.jegal_state_dict(seed=synth.JEGAL_SEED + off, family=name))


def _f64(sd):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}


def oracle_clip(gt, jt, gt64, jt64, frames_u8):
    """One clip (T, 270, 480, 3) uint8 -> dict: feats / emb (the reference of every error: the fp32 conv stack, float64 behind it) and
    feats32 / emb32 (the all-fp32 oracle the model-level tests use)."""
    T = frames_u8.shape[0]
    with torch.no_grad():
        f32, conv = O.gestsync_clip_feats(gt, torch.from_numpy(frames_u8.astype(np.float32) / np.float32(255.0)), return_conv=True)
        e32 = O.l2_normalize(O.jegal_forward_inference(jt, visual_feats=f32[None], visual_mask=torch.ones(1, T))[0])
        f64 = O.gestsync_feats_from_conv(gt64, conv.double())
        e64 = O.l2_normalize(O.jegal_forward_inference(jt64, visual_feats=f64[None], visual_mask=torch.ones(1, T, dtype=torch.float64))[0])
    return dict(feats=f64.numpy(), emb=e64.numpy(), feats32=f32.numpy(), emb32=e32.numpy())


_ORACLE = {}


def oracle(family, shape):
    """-> (frames (B, T, 270, 480, 3) uint8, [oracle_clip per clip]); computed once per (family, shape) and shared: treat as read-only."""
    key = (family, shape)
    if key not in _ORACLE:
        gsd, jsd = state_dicts(family)
        gt, jt = O.tensors(gsd), O.tensors(jsd)
        frames = frames_of(*shape)
        _ORACLE[key] = (frames, [oracle_clip(gt, jt, _f64(gt), _f64(jt), frames[b]) for b in range(shape[0])])
    return _ORACLE[key]


def errors(emb, feats, refs):
    """Worst clip's rel-L2 of the embedding and of the GestSync features against the oracle"""
    B = len(refs)
    return dict(emb=max(rel(emb[b], refs[b]["emb"]) for b in range(B)), feats=max(rel(feats[b], refs[b]["feats"]) for b in range(B)))
