"""The cases of tests/audit32_fp64_cases.py checked against themselves, without a GPU.

Conv: a plain float32 F.conv2d over the weights un-packed from the test's own packing must lie inside every case's bounds; the float64
product of the explicitly gathered patch matrix with the packed weights must reproduce the float64 F.conv2d reference (two formulations
of the same sum); and each planted defect must lie outside the bounds of every case it applies to:
  * two taps of the k order swapped;
  * a padding tap that reads the neighbouring pixel instead of zero;
  * rows taken from the next image;
  * the last k-quad dropped (the K % 16 tail);
  * the n tail dropped;
and, for the exact families,
  * a pool window shifted by one column;
  * the temporal clamp of stack_frames off by one frame, at either end.
The planner's threshold arithmetic of the cases is asserted as numbers.  So a GPU failure of tests/test_gpu_audit32_fp64.py points at
the kernel, not at a reference, a packing or a bound that float32 cannot meet.
"""
import numpy as np
import torch
import torch.nn.functional as F

import audit32_fp64_cases as C


def run_conv_cases(cases, with_defects):
    seen = set()
    for name, g, o in cases:
        d = C.conv32_data(g)
        k = C.case_opts(g, o)
        seen.add(k["kname"])
        act, scale, bias = k["act"], k["scale"], k["bias"]
        v, eb, nb = C.conv32_expect(d, act, scale, bias)
        M, K, N = d["M"], d["K"], g["N"]
        assert v.shape == (M, N) and bool((eb > 0).all()) and not v.isnan().any()
        r = C.conv32_ratio(C.conv32_standin(g, d, act, scale, bias), v, eb, nb)
        print(f"{name:32s} {k['kname']:24s} M={M} N={N} K={K} stand-in observed/bound {r:.3f}")
        assert r <= 1, name
        # the framed operands hold exactly the case's values and NaN everywhere else
        wb = C.w_buffer(d, k["ldw"], k["w_off"])
        rows = wb[k["w_off"]:].view(N + 16, k["ldw"])
        assert torch.equal(rows[:N, :K], d["wp"]) and bool(rows[N:].isnan().all()) and bool(rows[:, K:].isnan().all()) and bool(wb[:k["w_off"]].isnan().all())
        assert bool(d["inbuf"][0].isnan().all()) and bool(d["inbuf"][-1].isnan().all()) and torch.equal(d["inbuf"][1:-1], d["x"])
        if not with_defects:
            continue
        X = C.patches(d["x"], g)
        assert X.shape == (M, K)
        second = X.double() @ d["wp"].double().T
        assert float((second - d["acc"]).abs().max()) <= 1e-12 * float(d["mag"].max()), name          # the same sum, formulated twice

        def outside(Y, what):
            rr = C.conv32_ratio(C.epilogue32(Y, d, act, scale, bias), v, eb, nb)
            print(f"    {what}: observed/bound {rr:.1f}")
            assert rr > 1, (name, what)
        order = C.tap_order(g["KH"], g["KW"], g["SH"], g["SW"], g["reorder"])
        if len(order) > 1:
            swapped = list(order)
            swapped[0], swapped[-1] = swapped[-1], swapped[0]
            outside(C.patches(d["x"], g, order=swapped) @ d["wp"].T, "two taps swapped")
        if g["PH"] or g["PW"]:
            outside(C.patches(d["x"], g, clamp_pad=True) @ d["wp"].T, "a padding tap reads the neighbouring pixel")
        X2 = X.clone()
        idx = torch.arange(64, 128)
        X2[idx] = X[(idx + d["OH"] * d["OW"]) % M]
        outside(X2 @ d["wp"].T, "rows 64 .. 127 taken from the next image")
        X3 = X.clone()
        X3[:, (K - 1) // 4 * 4:] = 0
        outside(X3 @ d["wp"].T, "the last k-quad dropped")
        Y = X @ d["wp"].T
        Y[:, (N - 1) // 4 * 4:] = 0
        outside(Y, "the n tail dropped")
    return seen


def test_conv32_small_cases_standins_and_defects():
    seen = run_conv_cases(C.SMALL_CASES, True)
    assert seen == {"gemm32_kernel<1,1,64>", "gemm32_kernel<1,0,64>"}, seen
    C._DATA.clear()


def test_conv32_planner_cases_standins():
    seen = run_conv_cases(C.PLANNER_CASES, False)
    assert seen == {"gemm32_kernel<1,1,128>", "gemm32_kernel<1,1,64>", "gemm32_kernel<1,0,128>"}, seen
    C._DATA.clear()


def test_planner_threshold_arithmetic():
    """launch_gemm32's rule, restated in the case module: the 128 tile from ceil(M / 128) ceil(N / 128) >= 384 on."""
    assert C.conv_M(C.THR_ABOVE) == 12427 and C.tiles128(12427, 512) == 98 * 4 == 392
    assert C.conv_M(C.THR_BELOW) == 12138 and C.tiles128(12138, 512) == 95 * 4 == 380
    assert C.conv_M(C.THR_C1) == 12427
    assert C.conv_M(C.CONV1_FORM) == 779 * 63 == 49077 and C.tiles128(49077, 64) == 384
    assert C.tiles128(C.conv_M(dict(C.CONV1_FORM, nimg=778)), 64) == 383          # one image fewer: the 64 tile
    opts = lambda g, o: C.case_opts(g, o)["kname"]
    assert opts(C.THR_ABOVE, {}) == "gemm32_kernel<1,1,128>" and opts(C.THR_BELOW, {}) == "gemm32_kernel<1,1,64>"
    assert opts(C.THR_C1, {}) == "gemm32_kernel<1,0,128>" and opts(C.CONV1_FORM, {}) == "gemm32_kernel<1,1,128>"
    assert opts(C.C1_55, {}) == opts(C.C2_33, {}) == "gemm32_kernel<1,0,64>"
    assert opts(C.CONV5, dict(w_off=1, ldw_extra=1)) == "gemm32_kernel<1,0,64>" and opts(C.CONV5, {}) == "gemm32_kernel<1,1,64>"
    every = {C.case_opts(g, o)["kname"] for cases in C.CONV_FAMILIES.values() for _, g, o in cases}
    assert every == C.CONV32_INSTANCES
    # the shapes the issue fixes
    assert (C.conv_M(C.C1_55), 25) == (273, C.C1_55["KH"] * C.C1_55["KW"] * C.C1_55["C"])
    assert C.conv_M(C.AUDIO_DEEP) == 270 and 9 * 512 == 4608
    assert all(C.conv_M(g) > 256 and C.conv_M(g) % 64 for _, g, _ in C.SMALL_CASES)
    assert C.plan32(6400, 1024, 0, 0, conv=0).endswith(",128>") and C.tiles128(6400, 1024) == 400


def test_stack_frames32_reference():
    for u8 in (True, False):
        for T in C.STACK_T:
            c = C.stack32_case(u8, 2, T, 5, 7)
            sb, st, sh, sw, sc = c["strides"]
            flat = c["buf"].reshape(-1)[c["offset"]:]
            b, t, h, w, ch = 1, T - 1, 2, 4, 2
            got, want = flat[b * sb + t * st + h * sh + w * sw + ch * sc], c["framed"][b, t + 1, h, w, ch]          # the strides address the logical view
            assert float(got) == float(want)
            assert (2 - 1) * sb + (T - 1) * st + 4 * sh + 6 * sw + 2 * sc < flat.numel()
            for pad in C.STACK_PAD:
                if T + 2 * pad < 5:
                    continue
                ref = C.stack32_ref(c, u8, T, pad)
                assert ref.shape == (2, T + 2 * pad - 4, 5, 7, 16) and not ref.isnan().any() and bool((ref[..., 15] == 0).all())
                assert np.array_equal(ref.numpy(), C.stack32_ref_loops(c, u8, T, pad)), (u8, T, pad)          # torch's division == numpy's / np.float32(255)
                if u8:
                    assert float(ref.max()) <= 1.0
                # a clamp that is off by one frame reads a guard frame wherever the clamp is reached
                raw = torch.arange(T + 2 * pad - 4)[:, None] + torch.arange(5)[None, :] - pad
                for lo, hi, hit in ((-1, T - 1, bool((raw < 0).any())), (0, T, bool((raw > T - 1).any()))):
                    assert C.same_bits(C.stack32_ref(c, u8, T, pad, lo, hi), ref) != hit, (u8, T, pad, lo, hi)
    x = torch.arange(256, dtype=torch.float32)
    assert np.array_equal(torch.div(x, torch.tensor(255.0)).numpy(), x.numpy() / np.float32(255))
    assert not np.array_equal((x * torch.tensor(1 / 255.0)).numpy(), x.numpy() / np.float32(255))          # a reciprocal multiply would show


def test_maxpool32_reference():
    for shape in C.POOL_SHAPES:
        c = C.pool_case(*shape)
        nimg, H, W, Cc = shape
        assert c["ref"].shape == (nimg, c["OH"], c["OW"], Cc) and not c["ref"].isnan().any()
        assert np.array_equal(c["ref"].numpy(), C.pool_ref_loops(c["x"])), shape
        assert np.array_equal(c["ref"].numpy(), C.pool_ref_loops(c["xdev"])), shape          # the NaN row / column is outside every window
        assert c["unread"] == (1 - H % 2, 1 - W % 2) and bool(c["xdev"].isnan().any()) == (H % 2 == 0 or W % 2 == 0)
        assert not np.array_equal(c["ref"].numpy(), C.pool_ref_loops(c["xdev"], shift=1)), shape          # a window shifted by one column
        assert bool(c["buf"][0].isnan().all()) and bool(c["buf"][-1].isnan().all())
    assert torch.equal(F.max_pool2d(torch.tensor([[[[1.0, 2, 3], [4, 9, 6], [7, 8, 5]]]]), 3, 2).reshape(-1), torch.tensor([9.0]))


def test_zero_tail32_reference():
    for H in C.ZT_H:
        for row_elems in C.ZT_ROW_ELEMS:
            for halvings in C.ZT_HALVINGS:
                c = C.zero_tail32_case(H, row_elems, halvings)
                assert not bool((c["x"] == 0).any())
                for b, v in enumerate(c["valid"]):
                    n = max(v, 0)
                    for _ in range(halvings):
                        n = (n + 1) // 2
                    n = min(n, H)
                    assert bool((c["ref"][b, :n] == c["x"][b, :n]).all()) and bool((c["ref"][b, n:] == 0).all()), (H, row_elems, halvings, b)
                kept = [int((c["ref"][b] != 0).any(1).sum()) for b in range(len(c["valid"]))]
                assert kept[:3] == [0, 0, 1] and kept[3] == kept[4] == H and (H == 1 or kept[5] == H - 1), kept
    assert [r // 4 for r in C.ZT_ROW_ELEMS] == [2, 256, 257]


def test_group_mean32_standin():
    for L in C.GM_L:
        for D in C.GM_D:
            for groups in C.GM_GROUPS:
                c = C.group_mean32_case(groups, L, D)
                x = c["x"].reshape(groups, L, D)
                acc = torch.zeros(groups, D)
                for j in range(L):          # the kernel's order: one fp32 addition per row, one division
                    acc = acc + x[:, j]
                r = C.ratio(acc / float(L), c["ref"], c["bound"])
                print(f"group_mean32 L {L} D {D} groups {groups}: stand-in observed/bound {r:.3f}")
                assert r <= 1
                if L == 1:
                    assert torch.equal(acc / 1.0, c["x"])
                else:          # a group that starts one row late, a sum divided by L + 1
                    late = c["buf"][L + 1:L + 1 + groups * L].reshape(groups, L, D).mean(1)
                    assert C.ratio(late, c["ref"], c["bound"]) > 1
                    assert C.ratio(acc / float(L + 1), c["ref"], c["bound"]) > 1
                assert bool(c["buf"][:L].isnan().all()) and bool(c["buf"][-L:].isnan().all())
