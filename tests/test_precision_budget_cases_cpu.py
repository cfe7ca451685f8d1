"""What tests/test_gpu_precision_budget.py rests on, checked without a GPU (tests/precision_budget_cases.py): the rule that turns three
errors into the residual share rho, the two shapes' roles as the planner and the host rules see them (jg_debug_gemm_plan), the weight
forms the table's on / off / ideal columns rely on (jg_debug_weight_form), and the oracle's split into an fp32 conv stack and a float64
rest.  This module fails when either shape stops reaching the corrected plan or when weight_form changes a form the table relies on."""
import os

import numpy as np
import pytest

import precision_budget_cases as C


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jegal_amd._lib as L
    return L


def test_rho_on_hand_made_triples():
    assert C.rho(1.0, 1.0, 2.0) == 0.0                               # on = ideal: nothing is left
    assert C.rho(1.0, 2.0, 2.0) == 1.0                               # on = off: the remedy does nothing
    assert C.rho(0.0, 1.0, 2.0) == 0.25                              # an exact ideal: the share of the energy
    assert C.rho(3.0, 5.0, np.sqrt(73.0)) == pytest.approx(0.25)     # (25 - 9) / (73 - 9)
    assert C.rho(1.0, 0.9, 2.0) < 0 and C.rho(1.0, 3.0, 2.0) > 1     # better than the ideal; worse than nothing
    # the precondition: off^2 >= 2 ideal^2, the boundary included
    assert C.rho(1.0, 1.2, np.sqrt(2.0) + 1e-12) == pytest.approx(0.44, rel=1e-6)
    for blind in ((1.0, 1.0, 1.4), (1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (0.0, 0.0, 0.0)):
        with pytest.raises(C.CaseIsBlind):
            C.rho(*blind)
    for bad in ((np.nan, 1.0, 2.0), (1.0, np.inf, 2.0), (-1.0, 1.0, 2.0), (1.0, 1.0, np.nan)):
        with pytest.raises(AssertionError) as ei:
            C.rho(*bad)
        assert not isinstance(ei.value, C.CaseIsBlind)


def test_check_remedy_and_quadrature():
    assert C.check_remedy(1.0, 1.1, 4.0, 0.1) == pytest.approx(0.21 / 15)
    assert C.check_remedy(1.0, 3.9, 4.0, None) == pytest.approx((3.9 ** 2 - 1) / 15)       # reported rows: on < off only
    with pytest.raises(AssertionError):
        C.check_remedy(1.0, 4.0, 4.0, None)                          # the remedy switched off: rho = 1
    with pytest.raises(AssertionError):
        C.check_remedy(1.0, 4.0, 4.0, 0.1)
    with pytest.raises(AssertionError):
        C.check_remedy(1.0, 2.0, 4.0, 0.1)                           # rho = 0.2
    with pytest.raises(C.CaseIsBlind):
        C.check_remedy(1.0, 0.5, 1.2, 0.5)
    assert C.quadrature((3.0, 4.0, 12.0)) == 13.0
    assert C.check_quadrature(13.0, (3.0, 4.0, 12.0)) == 0.0
    assert C.check_quadrature(10.5, (3.0, 4.0, 12.0)) == pytest.approx(2.5 / 10.5)       # 23.8 %: inside
    with pytest.raises(AssertionError):
        C.check_quadrature(10.0, (3.0, 4.0, 12.0))                   # 13 against 10: 30 %
    with pytest.raises(AssertionError):
        C.check_quadrature(13.0, (3.0, 4.0))                         # a stage that dropped out: 5 against 13
    with pytest.raises(AssertionError):
        C.check_quadrature(5.0, (3.0, 4.0, 4.0))                     # a mask bit that fails to isolate: one term counted twice
    assert set(C.RHO_MAX) == {"runtime_correction", "calibrated_bias", "split_ends", "conv_diffusion"}
    assert C.RHO_MAX == {"runtime_correction": 0.1, "calibrated_bias": None, "split_ends": 0.1, "conv_diffusion": 0.5}
    assert C.QUADRATURE_TOL == 0.25 and C.AUD_TOL == 2e-5
    assert C.FAMILIES == (("gauss", 0), ("gauss", 1), ("heavy", 0)) and C.REPORTED_ONLY == {("conv_diffusion", "heavy+0")}


def rows_sampled(rpc):
    """rc_rows_sampled (elementwise_fp16.hip) in Python"""
    return rpc if rpc < C.RC_SAMPLE_FROM_RPC else sum(min(16, rpc - r0) for r0 in range(0, rpc, 128))


def test_shapes_keep_their_roles(lib):
    csrc = os.path.join(os.path.dirname(lib.LIB_PATH), "csrc")
    text = open(os.path.join(csrc, "gemm_plan.h")).read()
    for name, value in (("GEMM_LN_FUSED_MIN_ROWS", 1024), ("GEMM_CLIP_MIN_RPC", 256), ("GEMM_LN_CLIP_MIN_RPC", 128)):
        assert f"constexpr int {name} = {value};" in text, name
    kernel = open(os.path.join(csrc, "elementwise_fp16.hip")).read()
    assert "if (rpc < 1024) return rpc;" in kernel and "const int step = rpc < 1024 ? 16 : 128;" in kernel
    assert C.SHAPES == ((2, 26), (1, 52))
    (Ba, Ta), (Bs, Ts) = C.SHAPES
    assert Ta * C.S == 546 and rows_sampled(Ta * C.S) == 546          # every row of the clip
    assert Ts * C.S == 1092 and rows_sampled(Ts * C.S) == 9 * 16     # the 16-row runs at rows 0, 128, ..., 1024
    assert C.ROLE[(Ba, Ta)] == "all rows in the mean" and C.ROLE[(Bs, Ts)] == "sampled mean"
    for B, T in C.SHAPES:
        M, rpc = B * T * C.S, T * C.S
        assert M >= 1024 and rpc >= 256 and B < 8 and rpc * B == M
        for lin in C.LAYER_LINEARS + (C.FF_VID0,):
            name, grid = lib.gemm_plan(**C.plan_fields(B, T, lin))[:2]
            assert name.startswith("gemm_glds_kernel<0,") and grid > 0, (B, T, lin, name)        # granted, single fp16 weights
            assert (name == "gemm_glds_kernel<0,0,8,1,8,1,0,0,0>") == lin[3], (lin, name)       # the LayerNorm-fused instance where it belongs
            # the corrected form has no hi+lo instance behind a fused LayerNorm: with a lo operand the planner refuses
            if lin[3]:
                assert lib.gemm_plan(Wl=True, **C.plan_fields(B, T, lin))[0] == "rejected"
    # 21 B T < 1 024: no LayerNorm-fused form, so gs_fused_plan refuses the whole plan and every Linear runs hi+lo
    B, T = C.TOO_SHORT
    assert B * T * C.S == 1008
    for lin in C.LAYER_LINEARS:
        assert (lib.gemm_plan(**C.plan_fields(B, T, lin))[0] == "rejected") == lin[3], lin
    # fewer than 256 rows per clip in a batch of >= 1 024 rows: the per-clip bias of the plain Linears is refused
    for lin in C.LAYER_LINEARS + (C.FF_VID0,):
        if not lin[3]:
            assert lib.gemm_plan(**C.plan_fields(5, 12, lin))[0] == "rejected", lin
            assert lib.gemm_plan(**C.plan_fields(5, 12, lin, clip_bias=False))[0] != "rejected", lin
    # what the launch-count assertion derives from the graph
    assert len(C.corrected_linears(26)) == len(C.corrected_linears(52)) == 24
    assert "layers.0.qkv" not in C.corrected_linears(26) and "layers.1.qkv" in C.corrected_linears(26) and "ff_vid.0" in C.corrected_linears(26)


def test_weight_forms_the_table_relies_on(lib):
    CONV, GESTURE, CONTENT = 0, 1, 2
    GS, JG = 1, 2
    form = lambda prec, kind, model, keep32=False: lib.weight_form(prec, kind, model, keep32)[0]          # noqa: E731
    # JG_PREC_FP16_RC: GestSync's gesture Linears run-time corrected, JEGAL's split (the branch's ends are packed as content Linears or
    # gesture Linears with keep32: split either way, lo on the device for gemm_x3), conv single
    assert form(lib.PREC_FP16_RC, GESTURE, GS) == "runtime_corrected"
    assert lib.weight_form(lib.PREC_FP16_RC, GESTURE, GS)[1]                                    # ... with lo kept for the correction
    for kind in (GESTURE, CONTENT):
        for keep32 in (False, True):
            assert lib.weight_form(lib.PREC_FP16_RC, kind, JG, keep32)[:2] == ("split", True)
    assert form(lib.PREC_FP16_RC, CONV, GS) == "single"
    # `off` of the run-time correction and of nothing else: JG_PREC_FP16 is single everywhere
    for kind, model in ((CONV, GS), (GESTURE, GS), (GESTURE, JG), (CONTENT, JG), (CONV, JG)):
        assert lib.weight_form(lib.PREC_FP16, kind, model)[:2] == ("single", False)
    # `ideal` of the run-time correction and of the calibrated bias: hi+lo Linears on single conv weights
    assert form(lib.PREC_FP16_W2, GESTURE, GS) == "split" and form(lib.PREC_FP16_W2, CONV, GS) == "single"
    # `ideal` of the diffusion: hi+lo conv weights
    assert lib.weight_form(lib.PREC_FP16_W2_ALL, CONV, GS)[:2] == ("split", True)
    # the calibrated bias: GestSync's gesture Linears, calibrated when the weights are finalized
    assert lib.weight_form(lib.PREC_FP16_BC, GESTURE, GS) == ("bias_corrected", True, False)
    assert form(lib.PREC_FP16_BC, CONV, GS) == "single"
    # a run-time corrected GEMM takes lo exactly when it does not take the per-clip bias: never single fp16 without its correction
    assert not lib.gemm_runs_lo("runtime_corrected", clip_bias=True) and lib.gemm_runs_lo("runtime_corrected", clip_bias=False)
    assert not lib.gemm_runs_lo("bias_corrected") and lib.gemm_runs_lo("bias_corrected", calibrating=True)


def test_oracle_split_is_self_consistent():
    """The fp32 conv stack followed by float64 (transformer, ff_vid, JEGAL branch, normalisation) agrees with the all-fp32 oracle to fp32
    rounding: measured 2.7e-7 on the features and 6.5e-7 on the embeddings ((1, 52), gauss+0); 5e-6 is a quarter of AUD_TOL."""
    family, shape = C.FAMILIES[0], C.SHAPES[1]
    frames, refs = C.oracle(family, shape)
    assert frames.shape == (1, 52, 270, 480, 3) and frames.dtype == np.uint8 and len(refs) == 1
    r = refs[0]
    assert r["feats"].dtype == np.float64 and r["emb"].dtype == np.float64 and r["feats32"].dtype == np.float32
    assert r["feats"].shape == (52, 1024) and r["emb"].shape == (52, 512)
    assert np.isfinite(r["feats"]).all() and np.isfinite(r["emb"]).all()
    df, de = C.rel(r["feats32"], r["feats"]), C.rel(r["emb32"], r["emb"])
    print(f"fp32 oracle vs fp32 conv + float64: features {df:.2e}, embeddings {de:.2e}")
    assert 0 < df < 5e-6 and 0 < de < 5e-6
    assert np.allclose(np.linalg.norm(r["emb"], axis=-1), 1.0, rtol=0, atol=1e-12)
    assert C.oracle(family, shape)[1] is refs                        # computed once, shared
    e = C.errors(r["emb32"][None], r["feats32"][None], refs)
    assert e == dict(emb=de, feats=df)
