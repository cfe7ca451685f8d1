"""tests/conv1_fp64_cases.py checked without a GPU: the operands survive the library's fold and roundings unchanged, every sum is exact,
the per-frame decomposition equals conv3d, a plain fp32 evaluation stays inside the tier-A bound and reproduces the tier-B bits, and
every shape and zero-band family has the property it was chosen for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv1_fp64_cases as C


def clip_of(frames, b, p, T, pad):
    """(1, 3, 5, 270, 480) float64: the five frames position (b, p) reads"""
    return torch.stack([frames[b, C.frame_of(p, dt, T, pad)] for dt in range(5)], 0).permute(3, 0, 1, 2)[None].double()


def test_shape_properties():
    C.check_shape_properties()
    assert len(C.CASES) == 6 + 2 * len(C.ZERO_FAMILIES)


def test_operands_survive_fold_and_rounding():
    ops = C.operands()
    sd, w, shift, k = ops["sd"], ops["w"], ops["shift"], ops["k"]
    s, sh32 = C.folded_fp32(sd)
    assert np.array_equal(s, (2.0 ** k).astype(np.float32)), "BN scale is not 2^k exactly in float32"
    assert np.array_equal(sh32.astype(np.float64), shift.numpy()) and float(shift.abs().max()) <= 2
    # each step of (b - mu) s + be on its own, as a compiler that does not contract evaluates it
    b, mu, be = sd["net_vid.conv1.bias"], sd["net_vid.bn1.running_mean"], sd["net_vid.bn1.bias"]
    d = (b - mu).astype(np.float32)
    assert np.array_equal(d.astype(np.float64), b.astype(np.float64) - mu.astype(np.float64))
    assert np.array_equal((d * s).astype(np.float64), d.astype(np.float64) * s.astype(np.float64))
    wf = torch.from_numpy(sd["net_vid.conv1.weight"] * s[:, None, None, None, None])              # make_conv: w * s in fp32
    assert wf.dtype == torch.float32 and torch.equal(wf.double(), w)
    assert torch.equal(wf.half().double(), w) and torch.equal(wf.bfloat16().double(), w)          # round-to-nearest, error diffusion (carry 0), bf16
    assert set(np.unique(k)) == {-2, -1, 0, 1, 2}
    v, hi, lo = C.bias_pair(shift)
    assert torch.equal(v, 255.0 * shift * 2.0 ** -10) and torch.equal(hi + lo, v)
    assert int((lo != 0).sum()) >= 48, "the lo half of the bias pair must matter in almost every channel"
    assert not torch.equal(hi, v)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_sums_are_exact(case):
    d = C.case_data(case)
    print(f"{C.case_id(case)}: max |partial sum| bound {d['units']:.0f} units = {d['units'] / 2 ** 24:.3f} x 2^24")
    assert d["units"] < 2 ** 24 and d["fp32_exact"]
    assert torch.isfinite(d["ref"]).all() and (d["core"] > 0).all()


def test_decomposition_equals_conv3d():
    """per-frame conv2d terms summed per position == conv3d on the replicate-padded clip, float64, exactly"""
    B, T, pad = C.SHAPES["b1t3p4"]
    d = C.case_data(("b1t3p4", "dense"))
    ops = C.operands()
    x = d["frames"][0].permute(3, 0, 1, 2)[None].double()                                        # (1, 3, T, H, W)
    xp = F.pad(x, (0, 0, 0, 0, pad, pad), mode="replicate")
    y = F.conv3d(xp, ops["w"], stride=(1, 3, 3))[0] / 255.0 + ops["shift"][:, None, None, None]   # (64, P, 88, 158)
    ref = F.max_pool2d(y.clamp_min(0).permute(1, 0, 2, 3), 3, 2).permute(0, 2, 3, 1)
    diff = float((ref - d["ref"]).abs().max())
    print("decomposition vs conv3d: max difference", diff)
    assert diff == 0.0


@pytest.mark.parametrize("shape", ["b1t3p4", "b2t2p2"])
def test_fp32_emulation(shape):
    """conv3d in float32 (another summation order), times float32(1/255), .half(), pooled: inside the tier-A bound; its bits are the
    expected bits; the bias added after the scaling (the implicit-GEMM epilogue) stays inside the bound too."""
    B, T, pad = C.SHAPES[shape]
    P = C.positions(T, pad)
    d = C.case_data((shape, "dense"))
    ops = C.operands()
    w32, sh32, c = ops["w"].float(), ops["shift"].float(), torch.tensor(C.C255)
    bnd = C.bound(d)
    worst, worst_imp, rounded = 0.0, 0.0, []
    for b in range(B):
        for p in range(P):
            acc = F.conv3d(clip_of(d["frames"], b, p, T, pad).float(), w32, stride=(1, 3, 3))[0, :, 0]
            A32 = acc + (255.0 * sh32)[:, None, None]
            got = F.max_pool2d((A32 * c).clamp_min(0).half().float()[None], 3, 2)[0].half().permute(1, 2, 0)
            imp = F.max_pool2d((acc * c + sh32[:, None, None]).clamp_min(0).half().float()[None], 3, 2)[0].half().permute(1, 2, 0)
            i = b * P + p
            assert torch.equal(got.view(torch.int16), d["bits"][i]), (shape, b, p)
            worst = max(worst, float(((got.double() - d["ref"][i]).abs() / bnd[i]).max()))
            worst_imp = max(worst_imp, float(((imp.double() - d["ref"][i]).abs() / bnd[i]).max()))
            rounded.append(C.correctly_rounded_share(got, d["ref"][i]))
    print(f"{shape}: fp32 emulation observed / bound {worst:.3f} (bias after scaling: {worst_imp:.3f}), correctly rounded {min(rounded):.4%}")
    assert worst <= 1 and worst_imp <= 1


def test_dropped_lo_half_changes_bits():
    """the defect tier B exists for: the lo half of the bias pair dropped moves single ulps that tier A cannot see"""
    d = C.case_data(("b1t5p0", "dense"))
    ops = C.operands()
    _, hi, lo = C.bias_pair(ops["shift"])
    clip = clip_of(d["frames"], 0, 0, 5, 0)
    A = F.conv3d(clip, ops["w"], stride=(1, 3, 3))[0, :, 0] + (hi * 2.0 ** 10)[:, None, None]
    got = F.max_pool2d((A.float() * torch.tensor(C.C255)).clamp_min(0).half().float()[None], 3, 2)[0].half().permute(1, 2, 0)
    share = float((got.view(torch.int16) != d["bits"][0]).double().mean())
    ratio = float(((got.double() - d["ref"][0]).abs() / C.bound(d)[0]).max())
    print(f"lo half dropped: {share:.2%} of the bits differ, observed / bound {ratio:.3f}")
    assert share > 0.02


def test_zero_families():
    ops = C.operands()
    zb = C.zero_patch_bits(ops)
    full = (1 << C.ROW_TILES) - 1

    def bands(*rts):
        return sum(1 << r for r in rts)
    for shape in C.ZERO_SHAPES:
        B, T, pad = C.SHAPES[shape]
        P = C.positions(T, pad)
        z = {f: C.zero_bands(C.make_frames(shape, f)) for f in C.ZERO_FAMILIES}
        assert all(m == bands(*range(8)) for row in z["mask"] for m in row)                       # tiles 0..7 skipped, band 8 partial
        assert {m for row in z["mask_jitter"] for m in row} == {bands(*range(7)), bands(*range(8)), bands(*range(10))}
        assert all(m == bands(10, 11, 12) for row in z["middle"] for m in row)
        assert all(m == bands(*range(17, 22)) for row in z["bottom"] for m in row)
        assert z["unread_rows"] == z["bottom"]
        assert z["black"][min(1, B - 1)] == [full] * T and all(m == 0 for b, row in enumerate(z["black"]) if b != min(1, B - 1) for m in row)
        for f, (r, c) in C.LONE.items():
            fr = C.LONE_FRAME % T
            hit = {rt for rt in range(C.ROW_TILES) if 12 * rt <= r < 12 * rt + 16}
            assert z[f][0][fr] == bands(*(set(range(8)) - hit)) and hit, (f, hit)                    # the band(s) with the byte must run
            assert all(z[f][b][t] == bands(*range(8)) for b in range(B) for t in range(T) if (b, t) != (0, fr))
    # references: every output over an all-zero patch is the constant; a lone byte a window reads changes the reference
    d = C.case_data(("b1t3p4", "mask"))
    assert (d["bits"][:, :15] == zb).all()                       # pooled rows <= 14 read conv rows <= 30: input rows <= 96 < 110
    assert not (d["bits"][:, 18] == zb).all()
    for f in ("lone_byte_first", "lone_byte_1424", "lone_byte_bandend"):
        dl = C.case_data(("b1t3p4", f))
        n = int((dl["bits"] != d["bits"]).sum())
        big = int(((dl["ref"] - d["ref"]).abs() > C.bound(d)).sum())
        print(f"{f}: {n} expected bit patterns differ from mask's, {big} references differ by more than the tier-A bound")
        assert n >= 8 and big >= 1
    # byte 1439 belongs to pixel 479: conv column 157 ends at pixel 477 and the pool reads conv columns <= 156, so nothing changes -- the
    # case is about the scan's last lane finding the byte and the band running all the same
    dl = C.case_data(("b1t3p4", "lone_byte_last"))
    assert torch.equal(dl["bits"], d["bits"])
    du, db = C.case_data(("b1t3p4", "unread_rows")), C.case_data(("b1t3p4", "bottom"))
    assert torch.equal(du["bits"], db["bits"]) and torch.equal(du["ref"], db["ref"])
    dk = C.case_data(("b1t3p4", "black"))
    assert (dk["bits"] == zb).all()
