"""Each precision remedy removes the error it was built for (run with -m gpu, through the C ABI; cases, rule and oracle:
tests/precision_budget_cases.py, checked on the CPU by tests/test_precision_budget_cases_cpu.py).

The model-level tests assert 1e-3 on the whole path, and every mode but plain fp16 stays below it even with one of its remedies quietly
switched off (3.5e-4 with all four, 5.7e-4 without split ends and diffusion, 6.6e-4 without any run-time correction).
Here the stage a remedy acts on is the only one left in 16-bit (options audit_weights + audit_stages, audit_jegal_parts), and three
errors against the same oracle (fp32 conv stack, float64 behind it) give the residual share of removable error energy,
rho = (on^2 - ideal^2) / (off^2 - ideal^2): 0 = as good as the costlier arithmetic the remedy imitates, 1 = the remedy does nothing.

  remedy               isolation                          compared on           on                    off                   ideal               rho_max
  run-time correction  audit_stages 5                     features, embedding   JG_PREC_FP16_RC       JG_PREC_FP16          JG_PREC_FP16_W2     0.1
  calibrated bias      audit_stages 5                     features, embedding   JG_PREC_FP16_BC       JG_PREC_FP16          JG_PREC_FP16_W2     reported; on < off
  split-operand ends   audit_stages 3, jegal_parts 6      embedding             jegal_fp32_ends 1     jegal_fp32_ends 0     jegal_parts 15      0.1
  conv error diffusion audit_stages 6                     features              conv_round_diffuse 1  conv_round_diffuse 0  JG_PREC_FP16_W2_ALL 0.5 (heavy+0: reported; on < off)

Per family (gauss+0, gauss+1, heavy+0) and shape ((2, 26): every row of a clip in its mean, (1, 52): the sampled mean), also: the RC
handle issues exactly the correction launches of the graph on top of the W2 handle's GEMM launches (otherwise RC-vs-W2 compares hi+lo
with itself); with every stage on the fp32 kernels (mask 7) the outputs do not depend on mode or option, bit for bit, and are within
2e-5 of the oracle (no remedy touches the fp32 copies); the three single-stage errors add up in quadrature to the whole path's within
25 % (a mask bit that fails to isolate moves a term by 100 %); every output is finite.

Sensitivity, with the library's own switches: the `on` column run with the remedy's off-switch (JG_PREC_FP16 for JG_PREC_FP16_RC,
jegal_fp32_ends = 0, conv_round_diffuse = 0) gives rho = 1 and fails every asserted row; an RC handle with fuse_ln = 0 (hi+lo fall-back)
issues no correction launch and fails the launch-count assertion.

MEASURED on an MI355X (profiles/precision_budget.json, a copy of that run's record, holds every triple, launch count and stage sum; worst case per remedy):
  run-time correction   rho 0.039 on the features (gauss+0 (2, 26): ideal 3.57e-4, on 3.90e-4, off 8.72e-4), 0.013 on the embedding;
                        (2, 26) / (1, 52), i.e. whole / sampled mean: 0.039 / 0.033, 0.020 / 0.019, 0.035 / 0.019 per family
  calibrated bias       rho 0.035 on the features (heavy+0 (2, 26)), 0.014 on the embedding -- reported
  split-operand ends    rho 1.3e-5 (heavy+0 (2, 26): ideal 1.15e-6, on 1.83e-6, off 3.99e-4)
  conv error diffusion  rho 0.21 (gauss+1 (1, 52): ideal 1.09e-4, on 1.43e-4, off 2.29e-4); gauss+0 0.10 / 0.07; heavy+0 0.36 / 0.44 -- reported
  launches              RC 50, W2 26 GEMM-stage steps in every case (24 corrections); RC with fuse_ln = 0: 26
  mask 7                the same bits from all seven handles; at most 1.2e-6 from either oracle
  stages                quadrature sum within -4.1 % .. +1.5 % of the whole path (3.5e-4 .. 4.6e-4)
Wall time of the module: 51 s for the 42 cases (21 handles, 11 s of it the CPU oracle); the slowest case 5.3 s.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import precision_budget_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import precision_engine as PE  # noqa: E402

# a handle per (precision mode, options set before the weights are finalized); every one keeps the fp32 matrices (audit_weights)
CONFIGS = {
    "rc": ("PREC_FP16_RC", {}),                                   # the default: every remedy on
    "fp16": ("PREC_FP16", {}),
    "w2": ("PREC_FP16_W2", {}),
    "bc": ("PREC_FP16_BC", {}),                                   # built-in calibration, when the weights are finalized
    "rc_ends0": ("PREC_FP16_RC", {"jegal_fp32_ends": 0}),
    "rc_diffuse0": ("PREC_FP16_RC", {"conv_round_diffuse": 0}),
    "w2_all": ("PREC_FP16_W2_ALL", {}),
}
M7 = (C.NONE_16BIT, 0)
GS5, CONV6, JG3, ALL0 = (C.ONLY_GESTSYNC, 0), (C.ONLY_CONV, 0), (C.ONLY_JEGAL, 0), (C.ALL_16BIT, 0)
ENDS, ENDS_IDEAL = (C.ONLY_JEGAL, C.ONLY_ENDS), (C.ONLY_JEGAL, C.ALL_PARTS)
# the (audit_stages, audit_jegal_parts) runs of each handle; mask 7 on every one
RUNS = {
    "rc": (GS5, CONV6, JG3, ALL0, ENDS, ENDS_IDEAL, M7),
    "fp16": (GS5, M7),
    "w2": (GS5, M7),
    "bc": (GS5, M7),
    "rc_ends0": (ENDS, M7),
    "rc_diffuse0": (CONV6, M7),
    "w2_all": (CONV6, M7),
}
COUNTED = ("rc", "w2")                  # handles whose GEMM-stage launches of a gestsync_clip pass at audit_stages 5 are counted
LINEAR_LAUNCHES = 6 * 4 + 2             # the Linears of GestSync's transformer + ff_vid, in either plan
CASES = [(f, s) for f in C.FAMILIES for s in C.SHAPES]
TABLE = {}
_MEASURED = {}
_BROKEN = []


def case_id(c):
    return f"{C.fam_id(c[0])}-{C.shape_id(c[1])}"


# where the record goes: JEGAL_RECORD_DIR, e.g. the directory the family table of test_gpu_weight_families.py is collected in; build/
# (git-ignored) otherwise.  profiles/precision_budget.json is a copy of one run's record.
RECORD_DIR = os.environ.get("JEGAL_RECORD_DIR") or os.path.join(ROOT, "build")


def record(key, **kw):
    """Collects every figure in RECORD_DIR/precision_budget.json, as test_gpu_weight_families.record does with its table"""
    TABLE[key] = kw
    try:
        os.makedirs(RECORD_DIR, exist_ok=True)
        with open(os.path.join(RECORD_DIR, "precision_budget.json"), "w") as f:
            json.dump(TABLE, f, indent=1, sort_keys=True)
    except OSError:
        pass


def measure(family, config):
    """Everything the module needs of one handle, at both shapes, then the handle is closed (one alive at a time):
    {(shape, stages, parts): errors vs the oracle}, {(shape, 'mask7'): (emb, feats)}, {(shape, 'gemm_launches'): n}."""
    key = (family, config)
    if key in _MEASURED:
        return _MEASURED[key]
    if _BROKEN:
        raise RuntimeError(f"not run: an earlier handle of this module failed ({_BROKEN[0]!r}); nothing more is started on the GPU")
    try:
        _MEASURED[key] = _measure(family, config)
    except BaseException as exc:
        _BROKEN.append(exc)
        raise
    return _MEASURED[key]


def _measure(family, config):
    import jegal_amd._lib as L
    prec, opts = CONFIGS[config]
    gsd, jsd = C.state_dicts(family)
    out = {}
    e = PE.open_engine(getattr(L, prec), gsd, jsd, audit_weights=True, opts=opts)
    try:
        for shape in C.SHAPES:
            frames, refs = C.oracle(family, shape)
            dev = torch.from_numpy(frames).cuda()
            for stages, parts in RUNS[config]:
                emb, feats = PE.run(e, dev, stages, parts)
                assert np.isfinite(emb).all() and np.isfinite(feats).all(), (family, config, shape, stages, parts)
                out[(shape, stages, parts)] = C.errors(emb, feats, refs)
                if (stages, parts) == M7:
                    out[(shape, "mask7")] = (emb, feats)
            if config in COUNTED:
                # (after the runs above: layer 0's projected positional rows are built once per weight load, by a launch of this stage)
                e.set_option("audit_stages", C.ONLY_GESTSYNC)
                e.set_option("audit_jegal_parts", 0)
                e.profile(True)
                e.profile_reset()
                e.gestsync_clip(dev)
                out[(shape, "gemm_launches")] = e.profile_get()["gemm"][1]
                e.profile(False)
    finally:
        e.close()
    return out


def err(family, config, shape, run, what):
    return measure(family, config)[(shape,) + run][what]


def remedy(name, family, shape, what, ideal, on, off):
    """One row of the table on one output: prints and records the triple and rho, then asserts.  ideal / on / off: (config, run)."""
    i, n, f = (err(family, cfg, shape, run, what) for cfg, run in (ideal, on, off))
    fam = C.fam_id(family)
    rho_max = None if (name, fam) in C.REPORTED_ONLY else C.RHO_MAX[name]
    try:
        r = C.rho(i, n, f)
    except AssertionError:
        r = None
    print(f"\n[{fam} {C.shape_id(shape)}] {name:19s} {what:5s} ideal {i:.3e} on {n:.3e} off {f:.3e} -> rho "
          f"{'n/a' if r is None else format(r, '.4f')} (rho_max {rho_max})", end="")
    record(f"{fam}/{C.shape_id(shape)}/{name}/{what}", ideal=i, on=n, off=f, rho=r, rho_max=rho_max, on_config=on[0], off_config=off[0],
           ideal_config=ideal[0], role=C.ROLE[shape])
    return C.check_remedy(i, n, f, rho_max)


def check_runtime_correction(family, shape, on="rc", off="fp16", ideal="w2"):
    return [remedy("runtime_correction", family, shape, what, (ideal, GS5), (on, GS5), (off, GS5)) for what in ("feats", "emb")]


def check_calibrated_bias(family, shape, on="bc", off="fp16", ideal="w2"):
    return [remedy("calibrated_bias", family, shape, what, (ideal, GS5), (on, GS5), (off, GS5)) for what in ("feats", "emb")]


def check_split_ends(family, shape, on="rc", off="rc_ends0"):
    return [remedy("split_ends", family, shape, "emb", ("rc", ENDS_IDEAL), (on, ENDS), (off, ENDS))]


def check_conv_diffusion(family, shape, on="rc", off="rc_diffuse0", ideal="w2_all"):
    return [remedy("conv_diffusion", family, shape, "feats", (ideal, CONV6), (on, CONV6), (off, CONV6))]


def check_corrected_plan(family, shape, rc="rc", w2="w2"):
    n_rc, n_w2 = (measure(family, c)[(shape, "gemm_launches")] for c in (rc, w2))
    corrected = C.corrected_linears(shape[1])
    print(f"\n[{C.fam_id(family)} {C.shape_id(shape)}] GEMM-stage launches of a gestsync_clip pass at audit_stages 5: {rc} {n_rc}, {w2} {n_w2}; "
          f"{len(corrected)} corrected Linears", end="")
    record(f"{C.fam_id(family)}/{C.shape_id(shape)}/gemm_launches", rc=n_rc, w2=n_w2, corrected_linears=len(corrected),
           kernels_per_correction=C.KERNELS_PER_CORRECTION)
    assert n_w2 == LINEAR_LAUNCHES, (n_w2, LINEAR_LAUNCHES)
    assert n_rc - n_w2 == C.PROFILE_RECORDS_PER_CORRECTION * len(corrected), (n_rc, n_w2, len(corrected))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_runtime_correction_removes_the_weight_rounding_bias(case):
    """Only GestSync's transformer + ff_vid in 16-bit: JG_PREC_FP16_RC (single fp16 weights + lo . E[x] per clip) against plain fp16 and
    against hi+lo, on the features and on the embedding the fp32 JEGAL branch makes of them."""
    check_runtime_correction(*case)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_corrected_plan_was_taken(case):
    """The per-clip bias is two kernels (column means, lo x means) in one bracketed step in front of each corrected Linear.  W2 runs the
    26 Linears; RC runs them and one correction step per corrected Linear of the graph: four per layer, less layer 0's qkv (by
    linearity), plus ff_vid.0 = 24.  This is the check behind "never single fp16 without its correction"
    (test_gpu_runtime_corrected.py): a fall-back to hi+lo shows as a missing step."""
    check_corrected_plan(*case)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_calibrated_bias_reduces_the_error(case):
    """JG_PREC_FP16_BC with the built-in calibration clips (noise, not these clips): rho is printed and recorded, `on < off` asserted."""
    check_calibrated_bias(*case)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_split_operand_ends_are_fp32_grade(case):
    """Exact features into the JEGAL branch, its attention and feed-forward sub-layers on the fp32 kernels: only the input projection and
    the tail are left, on gemm_x3 (fp32 activations, hi+lo weights) or in 16-bit, against all four parts in fp32."""
    check_split_ends(*case)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv_error_diffusion_reaches_the_packed_matrices(case):
    """Only the conv stack in 16-bit: weights rounded with error diffusion across the taps against round-to-nearest and against hi+lo
    conv weights, on GestSync's features."""
    check_conv_diffusion(*case)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_mask_7_is_mode_independent(case):
    """Every stage on the fp32 kernels: the same bits from every handle of the module (five modes, both settings of conv_round_diffuse
    and jegal_fp32_ends) and the fp32 oracle's values -- no remedy touches the fp32 copies of the weights."""
    family, shape = case
    _, refs = C.oracle(family, shape)
    base = measure(family, "rc")[(shape, "mask7")]
    for config in CONFIGS:
        emb, feats = measure(family, config)[(shape, "mask7")]
        assert np.array_equal(emb, base[0]) and np.array_equal(feats, base[1]), (case_id(case), config)
    e32 = max(C.rel(base[0][b], refs[b]["emb32"]) for b in range(shape[0]))
    f32 = max(C.rel(base[1][b], refs[b]["feats32"]) for b in range(shape[0]))
    e = measure(family, "rc")[(shape,) + M7]
    print(f"\n[{case_id(case)}] mask 7 vs the fp32 oracle: emb {e32:.2e} feats {f32:.2e}; vs fp32 conv + float64: emb {e['emb']:.2e} feats {e['feats']:.2e}", end="")
    record(f"{C.fam_id(family)}/{C.shape_id(shape)}/mask7", emb_vs_fp32_oracle=e32, feats_vs_fp32_oracle=f32, emb=e["emb"], feats=e["feats"])
    assert max(e32, f32, e["emb"], e["feats"]) < C.AUD_TOL


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stages_isolate(case):
    """The default mode: conv stack alone, GestSync transformer + ff_vid alone and JEGAL branch alone in 16-bit add up in quadrature to
    the whole path in 16-bit."""
    family, shape = case
    parts = [err(family, "rc", shape, run, "emb") for run in (CONV6, GS5, JG3)]
    whole = err(family, "rc", shape, ALL0, "emb")
    q = C.quadrature(parts)
    print(f"\n[{case_id(case)}] embedding: conv only {parts[0]:.3e} GestSync only {parts[1]:.3e} JEGAL only {parts[2]:.3e} -> {q:.3e} in quadrature; "
          f"all three {whole:.3e} ({(q - whole) / whole:+.1%})", end="")
    record(f"{C.fam_id(family)}/{C.shape_id(shape)}/stages", conv_only=parts[0], gestsync_only=parts[1], jegal_only=parts[2], quadrature=q,
           whole=whole)
    assert whole < 1e-3
    C.check_quadrature(whole, parts)
