"""The cases of tests/elementwise_fp64_cases.py checked against themselves, without a GPU.

Bounded families: a plain torch-float32 stand-in of the operation, on the same generators, must lie inside the case's bound, and each
planted defect (the other LayerNorm flavour, the other eps, an ignored `valid`, a missed quarter of K) must lie outside it.  Bit-exact
families: the reference must equal a second, independently written numpy formulation (explicit loops), and each planted defect (an
off-by-one clamp in the gather, position ids counted exclusive of t, a dropped sampled row on the {0, 1} operands) must change bits.
So a GPU failure of tests/test_gpu_elementwise_fp64.py points at the kernel, not at a reference or at a bound that float32 cannot meet.
"""
import numpy as np
import pytest
import torch

import elementwise_fp64_cases as C
from test_gpu_kernels_fp64 import dt16, ulp16

BUILDS = [False, True]


def inside(got, ref, bound, what, limit=1.0):
    r = C.ratio(got, ref, bound)
    print(f"{what}: stand-in observed/bound {r:.3f}")
    assert r <= limit, what
    return r


# ---- bit-exact families: reference == second formulation; defects change bits ---------------------------------------------------------
@pytest.mark.parametrize("bf", BUILDS, ids=["fp16", "bf16"])
def test_stack_frames_reference(bf):
    d16 = dt16(bf)
    for u8 in (True, False):
        for T in C.STACK_T:
            for pad in C.STACK_PAD:
                if T + 2 * pad < 5:
                    continue
                c = C.stack_case(u8, 2, T, 5, 7)
                ref = C.stack_ref(c["frames"], T, pad, d16)
                assert ref.shape == (2, T + 2 * pad - 4, 5, 7, 16) and not ref.isnan().any()
                assert torch.equal(ref, torch.from_numpy(C.stack_ref_loops(c["frames"], T, pad)).to(d16)), (u8, T, pad)
                assert bool((ref[..., 15] == 0).all())
                if u8:
                    assert torch.equal(ref.float()[..., :15].reshape(-1, 5, 3)[:, 2], c["frames"][:, (torch.arange(T + 2 * pad - 4) + 2 - pad).clamp(0, T - 1)]
                                       .float().reshape(-1, 3))
    # the strides address the logical view
    c = C.stack_case(False, 2, 5, 5, 7)
    sb, st, sh, sw, sc = c["strides"]
    flat = c["src"].reshape(-1)
    assert float(flat[1 * sb + 3 * st + 2 * sh + 4 * sw + 2 * sc]) == float(c["frames"][1, 3, 2, 4, 2])


def test_window_gather_reference():
    clamped = 0
    for B, P, Twin, L, D, shift in C.GATHER_ROW_CASES:
        c = C.gather_case(B, P, Twin, L, D, shift)
        ref = C.gather_ref(c, B, P, Twin, L, shift)
        assert np.array_equal(ref.numpy(), C.gather_ref_loops(c, B, P, Twin, L, shift)), (Twin, L, D, shift)
        # an off-by-one clamp at either end changes bits wherever the clamp is reached
        raw = torch.arange(Twin)[:, None] + torch.arange(L)[None, :] - shift
        for lo, hi_off, hit in ((1, 1, bool((raw <= 0).any())), (0, 2, bool((raw >= P - 1).any()))):
            bad = C.gather_ref(c, B, P, Twin, L, shift, lo, hi_off)
            assert torch.equal(bad, ref) != hit, (Twin, L, D, shift, lo, hi_off)
            clamped += hit
    assert clamped >= len(C.GATHER_ROW_CASES)          # both clamps are reached across the cases
    for bf in BUILDS:
        for B, Twin, L in C.GATHER_TILED_CASES:
            M = B * Twin * L
            x16 = torch.randn(M, 512).to(dt16(bf))
            elems = (M + 127) // 128 * 65536 + 4096
            a = C.tiled_plane(x16, elems, 0x7D5A)
            assert np.array_equal(a.numpy(), C.tiled_plane_loops(x16, elems, 0x7D5A)), (bf, M)
            assert int((a != 0x7D5A).sum()) <= M * 512 and bool((a[(M + 127) // 128 * 65536:] == 0x7D5A).all())


@pytest.mark.parametrize("bf", BUILDS, ids=["fp16", "bf16"])
def test_cast_reference(bf):
    for n in (4, 1028):
        x = C.cast_values(n)
        ref = x.to(dt16(bf))
        second = torch.from_numpy(C.cast_ref_numpy(x, bf).copy())
        nan = x.isnan()
        assert bool(ref.isnan()[nan].all()) and not bool(ref.isnan()[~nan].any())
        assert torch.equal(C.bits(ref)[~nan], second[~nan]), (bf, n)
    x = C.cast_values(1028)
    r16 = x.to(torch.float16)
    assert float(r16[13]) == 1.0 and float(r16[14]) == 1 + 2.0 ** -9 and bool(r16[22].isinf()) and float(r16[20]) == 65504.0      # ties to even, overflow
    assert float(r16[4]) == 2.0 ** -23 and float(r16[6]) == 0.0 and float(r16[7]) == 2.0 ** -24 and bool(torch.signbit(r16[1]))     # subnormal ties, -0


def test_zero_tail_and_xlmr_reference():
    assert [C.tail_len(v, 2) for v in (-3, 0, 1, 4, 5, 8, 9, 20)] == [0, 0, 1, 1, 2, 2, 3, 5]
    for halvings in range(4):
        c = C.zero_tail_case(5, 8, halvings, torch.float16)
        nz = [(c["ref"][b] != 0).all(1).sum().item() for b in range(len(c["valid"]))]
        assert nz == [0, 0, 1, 5, 5, 4], (halvings, nz)
    for L in (1, 63, 65, 130):
        ids = C.xlmr_ids(L)
        pid = C.xlmr_pid(ids)
        assert np.array_equal(pid.numpy(), C.xlmr_pid_loops(ids)), L
        assert int(pid.max()) <= C.XL_MAXPOS - 1 and bool((pid[4] == C.XL_PAD).all())
        if L > C.XL_MAXPOS - 2:
            assert int(pid[0, -1]) == C.XL_MAXPOS - 1          # the clamp is reached
        tb = C.xlmr_tables(4)
        ref = C.xlmr_ref(ids, tb)
        loops = np.stack([(tb["word"].numpy()[min(max(int(i), 0), C.XL_VOCAB - 1)] + tb["type"].numpy()) + tb["pos"].numpy()[p]
                          for i, p in zip(ids.reshape(-1), C.xlmr_pid_loops(ids).reshape(-1))])
        assert np.array_equal(ref.numpy(), loops), L
        assert not torch.equal(C.xlmr_ref(ids, tb, inclusive=False), ref), "position ids counted exclusive of t must change bits"
    for bf in BUILDS:
        v = C.xlmr_ref(C.xlmr_ids(65), C.xlmr_tables(256))
        p = C.planes_ref(v, dt16(bf))
        assert float((p["hi"].double() + p["lo"].double() - v.double()).abs().max()) <= 2.0 ** (-16 if bf else -22) * float(v.abs().max())
        s1 = v.reshape(v.shape[0], -1, 64).sum(-1)
        s2 = (v * v).reshape(v.shape[0], -1, 64).sum(-1)
        inside(s1, p["s1"], p["b1"], "planes sum")
        inside(s2, p["s2"], p["b2"], "planes sum of squares")


def test_rc_mean_reference():
    for rpc in (1, 15, 17, 259, 1023, 1024, 1030, 1100, 1157, 3150):
        rows = [r for r in range(rpc) if rpc < 1024 or (r >> 4) % 8 == 0]
        assert C.rc_sample(rpc).tolist() == rows and C.rc_rows_sampled(rpc) == len(rows), rpc
    for rpc_all, nclips, valid in C.RC_MEAN_CASES:
        c = C.rc_mean_case(rpc_all, nclips, valid, 512, 520)
        for cl in range(nclips):
            rows = C.rc_clip_rows(rpc_all, valid, cl)
            blk = c["A"][cl * rpc_all:(cl + 1) * rpc_all, :512]
            assert int((~blk.isnan().any(1)).sum()) == len(rows) and not bool(c["A"][rows, :512].isnan().any())
            assert bool(c["A"][:, 512:].isnan().all())
            # a dropped or an extra row changes the bits of a good part of the columns (fp16 spacing near 1/2 is 2^-11 < 1 / R)
            s = c["a01"][rows].float().sum(0)
            R = torch.tensor(float(len(rows)))
            drop = ((s - c["a01"][rows[-1]].float()) / R).to(torch.float16)
            extra_row = min(int(rows[-1]) + 1, nclips * rpc_all - 1)
            extra = ((s + c["a01"][extra_row].float()) / R).to(torch.float16)
            assert float((drop != c["mean16"][cl]).float().mean()) >= 0.25, (rpc_all, cl)
            if extra_row != int(rows[-1]):
                assert float((extra != c["mean16"][cl]).float().mean()) >= 0.25, (rpc_all, cl)


# ---- bounded families: float32 stand-ins inside, defects outside ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [512, 768])
def test_layernorm_bounds(D):
    for family in C.LN_FAMILIES:
        for rows in C.LN_ROWS:
            c = C.ln_input(family, rows, D)
            for flavour in (C.LN_STD, C.LN_ANNOTATED):
                for relu in (0, 1):
                    k = C.ln_case(c, flavour, relu)
                    got = C.ln_standin(c, flavour, relu)
                    inside(got, k["ref"], k["bound"], f"layernorm {family} rows {rows} D {D} flavour {flavour} relu {relu}")
                    assert C.ln_nrm(got, k) <= k["nbound"]
                    check_ln_defects(c, k, family, relu)
                    for bf in BUILDS:
                        inside(got.to(dt16(bf)), k["ref"], k["bound"] + ulp16(k["ref"], bf), "  16-bit")


def check_ln_defects(c, k, family, relu):
    """The bounds must see the other flavour in every case, and the other eps where eps matters (the 1e-3 family)."""
    defects = ["other_flavour"] + (["other_eps"] if family == "small" else [])
    for d in defects:
        assert C.ratio(k[d], k["ref"], k["bound"]) >= 5, (d, family)
        assert C.ln_nrm(k[d], k) >= 10 * k["nbound"], (d, family)


def test_layernorm_planes_bounds():
    for bf in BUILDS:
        for family in C.LN_FAMILIES:
            c = C.planes_input(family, 5, dt16(bf))
            k = C.ln_case(c, C.LN_STD, 0, x64=c["x64"])
            got = C.ln_standin(c, C.LN_STD, 0, x32=c["hi"].float() + c["lo"].float())
            inside(got, k["ref"], k["bound"], f"layernorm_planes {family} bf {bf}")
            assert C.ln_nrm(got, k) <= k["nbound"]
            check_ln_defects(c, k, family, 0)


def test_reduction_bounds():
    for rows, P, nconst in ((1, 4, 0), (1, 12, 1), (255, 4, 8), (257, 12, 8)):
        c = C.ln_stats_case(rows, P, nconst)
        m, r = C.ln_stats_standin(c)
        inside(m, c["mean"], c["bmean"], f"ln_stats mean rows {rows} P {P}")
        inside(r, c["rstd"], c["brstd"], f"ln_stats rstd rows {rows} P {P}")
        if nconst == 8:
            raw = c["raw_var"][:8]
            assert bool((raw < 0).any()) and bool((raw > 0).any()), "the constant rows must reach the clamp from both sides"
            assert float(raw.abs().max()) < 1e-6
    for bf in BUILDS:
        for L in (1, 21, 50):
            c = C.group_mean_case(33, L, 8, dt16(bf))
            got = (c["x"].float().reshape(33, L, 8).sum(1) * (1.0 / L)).to(dt16(bf))
            if L == 1:
                assert torch.equal(got.double(), c["ref"])
            inside(got, c["ref"], c["bound"] + ulp16(c["ref"], bf), f"group_mean L {L} bf {bf}")
            wrong = c["x"].float().reshape(33, L, 8).sum(1) / (L + 1)          # a wrong divisor
            assert C.ratio(wrong, c["ref"], c["bound"] + ulp16(c["ref"], bf)) > 1
    for M in (1, 63, 64, 65, 200):
        for st in (False, True):
            c = C.col_sum_case(M, 520, st)
            a = c["A"].float()
            if st:
                a = (a - c["stats"][:, :1]) * c["stats"][:, 1:]
            got = (c["out0"] + a.sum(0)) + a.sum(0)
            inside(got, c["ref"], c["bound"], f"col_sum M {M} stats {st}")
            if M > 1:
                assert C.ratio((c["out0"] + a[1:].sum(0)) + a.sum(0), c["ref"], c["bound"]) > 1, "a dropped row"
    for S, N, K in ((3, 1, 1), (3, 5, 70), (3, 5, 512)):
        for with_lo in (False, True):
            for with_bias in (False, True):
                c = C.pe_project_case(S, N, K, with_lo, with_bias)
                got = C.pe_project_standin(c)
                # (K = 1 without bias: two roundings of one product sit exactly on 2 K u; the 16-bit store's ulp covers the second-order term)
                inside(got.to(torch.float16), c["ref"], c["bound"] + ulp16(c["ref"]), f"pe_project K {K} lo {with_lo} bias {with_bias}")
    for rows in (1, 5):
        for D in (4, 260, 512):
            c = C.l2norm_case(rows, D)
            x = c["x"]
            inside(x / x.norm(dim=1, keepdim=True).clamp_min(1e-12), c["ref"], c["bound"], f"l2norm rows {rows} D {D}")
    for n in (1, 5):
        for D in (1, 100, 768):
            c = C.pool_case(n, D)
            got = C.pool_standin(c)
            inside(got, c["ref"], c["bound"], f"pool n {n} D {D}")
            assert torch.equal(got[0].double(), c["ref"][0])          # length 1: an exact copy


def test_rc_out_bounds():
    for rpc_all, nclips, valid, K, N, tiled, bias in C.RC_OUT_CASES:
        c = C.rc_out_case(rpc_all, nclips, valid, K, N, bias)
        got = C.rc_out_standin(c, rpc_all, nclips, valid)
        inside(got, c["ref"], c["bound"], f"rc_bias rpc {rpc_all} clips {nclips} K {K} N {N}")
        # the correction itself is far above the bound, so a missed quarter of K or a missing bias shows; an ignored `valid` too
        # (zero-mean lo: |corr| ~ sqrt(K) 2^-12 / 2 against a bound of ~ K 2^-12 2^-11 / 2 -- a factor 2^11 / sqrt(K) >= 45)
        assert float(c["corr"].norm() / c["bound"].norm()) >= 10
        assert C.ratio(C.rc_out_standin(c, rpc_all, nclips, valid, drop_quarter=True), c["ref"], c["bound"]) > 5
        if bias:
            assert C.ratio(got - c["bias"], c["ref"], c["bound"]) > 5
        if valid is not None and any(v < rpc_all for v in valid):
            assert C.ratio(C.rc_out_standin(c, rpc_all, nclips, valid, ignore_valid=True), c["ref"], c["bound"]) > 1


@pytest.mark.parametrize("bf", BUILDS, ids=["fp16", "bf16"])
def test_audio_conv0_bounds(bf):
    d16 = dt16(bf)
    for Tm in C.AUDIO_TM:
        for F_ in C.AUDIO_F:
            for vi, valid in enumerate(C.audio_valids(Tm)):
                c = C.audio_conv0_case(Tm, F_, valid, with_lo=bool((Tm + vi) & 1), d16=d16)
                got = C.audio_conv0_standin(c, d16)
                bound = c["bound"] + ulp16(c["ref"], bf)
                inside(got.to(d16), c["ref"], bound, f"audio_conv0 Tm {Tm} F {F_} valid {valid}")
                for b in range(3):
                    assert bool((c["ref"][b, c["Tv"][b]:] == 0).all()) and bool(c["mel_dev"][b, c["Tv"][b]:].isnan().all())
                if valid is not None and Tm >= 3 and any(0 < t < Tm for t in c["Tv"]):
                    assert C.ratio(C.audio_conv0_standin(c, d16, ignore_valid=True), c["ref"], bound) > 1, "an ignored valid must show"
