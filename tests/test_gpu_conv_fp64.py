"""Kernel-level checks of the conv instances of launch_gemm, the compaction row maps and the max-pool against float64 (run with -m gpu).

Every conv case runs ONE launch through jg_debug_conv_check (include/jegal_hip.h): the geometry comes from the function production uses
(engine::geom), the handle's options pick the instance, and -- for the cases with per-image row-skip counts s2 -- the production
launch_conv_rowmaps builds the compacted row map in front of the GEMM, as gs_conv_stack does.  The reference is float64
torch.nn.functional.conv2d on the CPU over exactly the operands the kernel received (16-bit values are exact in float64, hi+lo weights
are summed in float64), with scale, bias and ReLU applied in float64.  The test packs the weights ITSELF, from the description of the k
order in jegal_amd/csrc/common.h (ConvGeom::taps: parity-class order for `reorder` layers of <= 32 taps, natural order otherwise), never
by calling the library: a disagreement between geom()'s tap table and the packing is one of the defects to catch.  The weights are
drawn independently per tap, so a swapped tap, a padding tap that reads a neighbouring pixel or a row taken from the wrong image moves
the result by O(|ref|).

Row skip (ConvGeom::rowmap / in_op / const_in), restated here from shared.h (conv_skip_decode): image img computes output rows
oh >= s = decode(s2[img], op) and nothing else -- rows oh < s must still hold the sentinel bit pattern afterwards -- and its input rows
ih < rin = decode(s2[img], op - 1) come from the const image instead of the input, where they hold NaN on the device.

Guards, all inside allocations: the input is [one NaN image | nimg images | one NaN image], Wh / Wl carry NaN in columns K .. ldw-1 and
in 16 extra rows, the const image is followed by a NaN image, outputs carry 128 guard rows and ldc > N guard columns of sentinel bits.
Every output element is compared.

Bounds, derived as in test_gpu_kernels_fp64.py (u = 2^-24, K = KH KW C):
  * element-wise  |got - ref| <= 2 K u (conv2d(|in|, |w|) |scale| + |bias|)  [+ 1 ulp of ref for 16-bit outputs]
  * norm-wise for fp32 outputs  ||got - ref|| / ||ref|| <= 2 sqrt(K) u; every hi+lo case asserts that dropping the lo half would exceed
    10x that bound on its own operands.
The max-pool and the row maps are exact: torch.equal / numpy.array_equal.  Each case prints observed / bound.

Seeded defects these tests were seen to fail on (each built into a scratch copy of the library, never committed): two entries of geom()'s
tap table swapped (family "tiles": observed / bound 234 .. 932), the `ih < rin` select of the ROWCONST loader dropped ("rowconst": 842 ..
1311), a padding tap reading the pixel address instead of the zero page ("tiles": 1509 .. 1e5), `first` of conv_rowmap_fill_kernel off by
one (test_conv_rowmaps_exact: every map entry).  ReLU turns a NaN that was read into 0, so each row-skip family also has cases without it.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_kernels_fp64 as K64
from test_gpu_kernels_fp64 import (DEV, SENT16, SENT32, U, dt16, engine, guarded, guards_intact, nrm_ratio, operand, planned, rejects, ulp16,
                                   urnd)

pytestmark = pytest.mark.gpu

# every conv instance of the table in jegal_amd/csrc/gemm_plan.h: gemm_glds_kernel<W2,CONV,MI,WM,WN,LNF,SPR,XE,C32>, gemm_kernel<WM,WN,CONV,W2>
CONV_INSTANCES = {
    "gemm_glds_kernel<0,1,2,4,2,0,0,0,0>", "gemm_glds_kernel<1,1,2,4,2,0,0,0,0>",          # 128x128
    "gemm_glds_kernel<0,1,4,4,2,0,0,0,0>", "gemm_glds_kernel<1,1,4,4,2,0,0,0,0>",          # 256x128
    "gemm_glds_kernel<0,1,8,2,4,0,0,0,0>",                                                 # 256x256
    "gemm_glds_kernel<0,1,8,4,2,0,0,0,0>",                                                 # 512x128 (the tall tile)
    "gemm_glds_kernel<0,1,2,8,1,0,0,0,1>",                                                 # C = 32, 256x64
    # behind a row-skipping producer (SPR: the loader reads ConvGeom::const_in)
    "gemm_glds_kernel<0,1,2,4,2,0,1,0,0>", "gemm_glds_kernel<1,1,2,4,2,0,1,0,0>",
    "gemm_glds_kernel<0,1,4,4,2,0,1,0,0>", "gemm_glds_kernel<1,1,4,4,2,0,1,0,0>",
    "gemm_glds_kernel<0,1,8,2,4,0,1,0,0>",
    # register-staged conv forms
    "gemm_kernel<4,1,1,0>", "gemm_kernel<4,1,1,1>", "gemm_kernel<2,2,1,0>", "gemm_kernel<2,2,1,1>",
}
SEEN = set()
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in K64._ENGINES.values():
        e.close()
    K64._ENGINES.clear()
    _DATA.clear()


# ---- what the test restates from the library's headers ---------------------------------------------------------------------------
def skip_decode(w, op):
    """conv_skip_decode (shared.h): op 0 the count itself, op 1 / 2 / 3: w // 2 - (op - 1); never negative."""
    return max(w if op == 0 else w // 2 - (op - 1), 0)


def tap_order(KH, KW, SH, SW, reorder):
    """ConvGeom::taps (common.h): the k order of the taps, by parity class (kh % SH, kw % SW) for `reorder` layers of <= 32 taps."""
    if reorder and KH * KW <= 32:
        return [(kh, kw) for ph in range(SH) for pw in range(SW) for kh in range(ph, KH, SH) for kw in range(pw, KW, SW)]
    return [(kh, kw) for kh in range(KH) for kw in range(KW)]


def geo(nimg, H, W, C, N, KH, KW, SH, SW, PH, PW, reorder):
    return dict(nimg=nimg, H=H, W=W, C=C, N=N, KH=KH, KW=KW, SH=SH, SW=SW, PH=PH, PW=PW, reorder=int(reorder))


# the shapes: about 30 output pixels per image, so a tile spans many images; M a little over 256 and no multiple of 128
CONV2 = geo(9, 13, 15, 64, 128, 5, 5, 2, 2, 0, 0, True)          # 5 x 6 per image, M 270, K 1600: all four tap words (25 taps)
CONV3 = geo(9, 9, 12, 128, 256, 3, 3, 2, 2, 1, 1, True)          # 5 x 6, M 270: the bottom tap row falls outside
CONV3_ODD = geo(9, 9, 11, 128, 256, 3, 3, 2, 2, 1, 1, True)      # ... and with odd W the right tap column too (conv3 itself: W = 37)
CONV4 = geo(9, 6, 9, 256, 256, 3, 3, 1, 2, 1, 1, True)           # 6 x 5, M 270, K 2304
CONV5 = geo(3, 9, 11, 64, 128, 3, 3, 1, 1, 1, 1, True)           # 9 x 11, M 297: padding on all four sides
AUDIO33 = geo(9, 15, 5, 64, 128, 3, 3, 1, 3, 1, 1, False)        # 15 x 2, M 270: natural tap order (tap_table = 0)
AUDIO11 = geo(9, 30, 3, 64, 128, 1, 1, 1, 3, 0, 0, False)        # 30 x 1, M 270: a single tap, a single k-tile
TALL = geo(32, 64, 64, 64, 128, 1, 1, 1, 1, 0, 0, False)         # M = 131072: the planner's threshold of the 512x128 tile
TALL_BELOW = geo(1, 2047, 64, 64, 128, 1, 1, 1, 1, 0, 0, False)  # M = 131008, one image row below it (and ih up to the packed-coordinate limit)
C32_33 = geo(11, 10, 10, 32, 64, 3, 3, 2, 2, 1, 1, False)        # 5 x 5, M 275, K 288: the last k-tile holds one tap
C32_22 = geo(8, 10, 10, 32, 64, 2, 2, 2, 2, 1, 1, False)         # 6 x 6, M 288, K 128: an even number of taps
CONV1 = geo(5, 25, 31, 16, 64, 7, 7, 3, 3, 0, 0, False)          # 7 x 9, M 315, K 784 (K % 64 = 16): conv1's implicit form
CONV5_M255 = geo(3, 5, 17, 64, 128, 3, 3, 1, 1, 1, 1, True)      # M 255 < 256
CONV5_N192 = dict(CONV5, N=192)
CONV5_C32 = dict(CONV5, C=32)


# ---- operands and the float64 reference, computed once per (shape, weights, skip) and shared between the store forms ------------------
_DATA = {}


def conv_data(g, w2, bf, s2, op, use_const, ldw, seed):
    key = (tuple(sorted(g.items())), w2, bf, None if s2 is None else tuple(s2), op, use_const, ldw, seed)
    if key in _DATA:
        return _DATA[key]
    gen = torch.Generator().manual_seed(seed)
    d16 = dt16(bf)
    nimg, H, W, C, N, KH, KW, SH, SW, PH, PW = (g[k] for k in ("nimg", "H", "W", "C", "N", "KH", "KW", "SH", "SW", "PH", "PW"))
    K = KH * KW * C
    OH, OW = (H + 2 * PH - KH) // SH + 1, (W + 2 * PW - KW) // SW + 1
    M = nimg * OH * OW
    x = urnd(gen, (nimg, H, W, C)).to(d16).double()
    w = urnd(gen, (N, C, KH, KW)) / math.sqrt(K) * 2                    # independent per tap
    wh = w.to(d16).double()
    wl = (w - wh).to(d16).double() if w2 else None
    weff = wh + wl if w2 else wh
    cimg = urnd(gen, (H, W, C)).to(d16).double()
    sc, bi = urnd(gen, (N,), 0.5, 1.5).float(), urnd(gen, (N,)).float()
    xref, xdev = x, x
    s = [0] * nimg
    if s2 is not None:
        s = [skip_decode(v, op) for v in s2]
        if use_const:
            xref, xdev = x.clone(), x.clone()
            for i, v in enumerate(s2):
                rin = min(skip_decode(v, op - 1), H)
                xref[i, :rin] = cimg[:rin]                               # the reference input: where(ih < rin, const_in, in[img])
                xdev[i, :rin] = float("nan")                             # the device input: nobody may read these rows
    assert all(v < OH for v in s)

    def conv(a, b):
        return F.conv2d(a.permute(0, 3, 1, 2), b, stride=(SH, SW), padding=(PH, PW)).permute(0, 2, 3, 1).reshape(M, N)
    order = tap_order(KH, KW, SH, SW, g["reorder"])

    def pack(t4):                                                        # Wpacked[o][t C + c] = w[o][c][kh_t][kw_t]
        return torch.cat([t4[:, :, kh, kw] for kh, kw in order], 1)
    inbuf = torch.full((nimg + 2, H, W, C), float("nan"), dtype=d16)
    inbuf[1:nimg + 1] = xdev.to(d16)
    cbuf = torch.full((2, H, W, C), float("nan"), dtype=d16)
    cbuf[0] = cimg.to(d16)
    d = dict(M=M, K=K, OH=OH, OW=OW, acc=conv(xref, weff), mag=conv(xref.abs(), weff.abs()), lo=conv(xref, wl) if w2 else None, sc=sc, bi=bi,
             computed=torch.tensor([oh >= s[i] for i in range(nimg) for oh in range(OH) for _ in range(OW)]),
             inbuf=inbuf.to(DEV), Wh=operand(pack(wh), ldw, d16), Wl=operand(pack(wl), ldw, d16) if w2 else None, cbuf=cbuf.to(DEV),
             sc_dev=sc.to(DEV), bi_dev=bi.to(DEV))
    _DATA[key] = d
    return d


OUT_FORMS = ("rows16", "frag16", "both")      # out16 alone with ldc % 8 == 0: the row-transposing epilogue; ldc = N + 4: the fragment store; + fp32


def conv_args(g, d, *, w2, out, scale, bias, relu, ldw, bf, s2, op, use_const):
    """(arguments of debug_conv_check, the same question for the planner, the output buffers)"""
    N, M = g["N"], d["M"]
    ldc = N + 4 if out in ("frag16", "f32") else N + 8
    d16 = dt16(bf)
    o32 = guarded(M, ldc, torch.float32) if out in ("f32", "both") else None
    o16 = guarded(M, ldc, d16) if out != "f32" else None
    kw = dict({k: g[k] for k in ("nimg", "H", "W", "C", "KH", "KW", "SH", "SW", "PH", "PW", "reorder", "N")}, Wh=d["Wh"], ldw=ldw, K=d["K"], relu=relu,
              ldc=ldc, op=op, s2_host=s2)
    kw["in"] = d["inbuf"][1:]                     # image 0: a NaN image in front of it and one behind the last
    pk = dict(M=M, N=N, K=d["K"], ldw=ldw, ldc=ldc, relu=relu, Wh=True,
              conv=dict({k: g[k] for k in ("H", "W", "C", "KH", "KW", "PH", "PW")}, tap_table=int(bool(g["reorder"]) and g["KH"] * g["KW"] <= 32),
                        rowmap=s2 is not None, const_in=bool(use_const)))
    for name, val in (("Wl", d["Wl"] if w2 else None), ("scale", d["sc_dev"] if scale else None), ("bias", d["bi_dev"] if bias else None),
                      ("out32", o32), ("out16", o16), ("const_in", d["cbuf"] if use_const else None)):
        if val is not None:
            kw[name] = val
            if name != "const_in":
                pk[name] = True
    return kw, pk, o32, o16


def conv_case(name, g, *, w2=False, out="rows16", scale=False, bias=True, relu=1, bf=False, opts=None, s2=None, op=0, use_const=False, ldw=None,
              seed=11, family="conv"):
    """One conv launch vs float64 -> list of failures."""
    ldw = ldw or g["KH"] * g["KW"] * g["C"] + 8            # NaN columns behind K in every weight row
    d = conv_data(g, w2, bf, s2, op, use_const, ldw, seed)
    M, N, K = d["M"], g["N"], d["K"]
    e = engine(prec=4 if bf else None, **(opts or {}))
    kw, pk, o32, o16 = conv_args(g, d, w2=w2, out=out, scale=scale, bias=bias, relu=relu, ldw=ldw, bf=bf, s2=s2, op=op, use_const=use_const)
    e.debug_conv_check(**kw)
    torch.cuda.synchronize()
    kname = e.debug_last_kernel()
    want = planned(pk, opts)
    assert kname == want, f"{name}: launched {kname}, the planner says {want}"
    SEEN.add(kname)

    scd = d["sc"].double() if scale else torch.ones(N, dtype=torch.float64)
    bid = d["bi"].double() if bias else torch.zeros(N, dtype=torch.float64)
    act = (lambda t: t.clamp_min(0)) if relu else (lambda t: t)
    pre = d["acc"] * scd + bid
    v = act(pre)
    eb = 2 * K * U * (d["mag"] * scd.abs() + bid.abs())
    comp = d["computed"]
    nb = 2 * math.sqrt(K) * U
    fails = []
    if w2:          # the defect the norm-wise bound exists for: the lo half dropped
        drop = nrm_ratio(act(pre - d["lo"] * scd)[comp], v[comp])
        assert drop >= 10 * nb, f"{name}: bound {nb:.2e} too loose to see a dropped lo half ({drop:.2e})"
    worst = 0.0
    for buf, is16 in ((o32, False), (o16, True)):
        if buf is None:
            continue
        what = "16" if is16 else "32"
        if not guards_intact(buf, M, N):
            fails.append(f"{name}: guard of out{what} overwritten")
        raw = buf[:M, :N].view(torch.int16 if is16 else torch.int32).cpu()
        if not bool((raw[~comp] == (SENT16 if is16 else SENT32)).all()):
            fails.append(f"{name}: out{what} rows of the skipped part were written")
        got = buf[:M, :N].double().cpu()[comp]
        vv = v[comp]
        bound = eb[comp] + (ulp16(vv, bf) if is16 else 0)
        r = float(((got - vv).abs() / bound).max()) if got.isfinite().all() else float("inf")
        worst = max(worst, r)
        if not is16:
            worst = max(worst, nrm_ratio(got, vv) / nb)
    RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    print(f"{name:34s} {kname:38s} M={M} N={N} K={K} out={out} rows {int(comp.sum())} observed/bound {worst:.3f}")
    if not worst <= 1:
        fails.append(f"{name}: observed/bound {worst:.3f} ({kname})")
    return fails


# ---- the cases, in families of a few seconds each ---------------------------------------------------------------------------------------
BIG = dict(gemm_small_tile=0)
S2_OH5 = [0, 1, 4, 2, 3, 0, 4, 1, 2]          # op 0 on 5 output rows: none, one, the maximum that leaves one row, values between
S2_TALL = [0, 1, 63, 17, 40, 2, 62, 5] * 4    # op 0 on 64 output rows
S2_CONV3 = [0, 1, 9, 2, 3, 4, 5, 8, 7]        # op 1 on 9 x 12: s = s2 // 2 <= 4, rin = s2 (9: the whole input is the const image)
S2_CONV4 = [0, 1, 13, 2, 3, 6, 7, 12, 5]      # op 2 on 6 x 9: s = s2 // 2 - 1 <= 5, rin = s2 // 2
S2_CONV5 = [5, 21, 10]                        # op 3 on 9 x 11: s = s2 // 2 - 2 <= 8, rin = s2 // 2 - 1


def family_tiles():
    """every LDS-DMA tile without a row map: the three store forms each, hi+lo weights, tap tables, padding, the C = 32 instance"""
    f = []
    for out in OUT_FORMS:
        f += conv_case(f"conv2_small_{out}", CONV2, out=out)
        f += conv_case(f"conv2_small_w2_{out}", CONV2, w2=True, out=out)
        f += conv_case(f"conv2_256x128_{out}", CONV2, out=out, opts=BIG)
        f += conv_case(f"conv2_256x128_w2_{out}", CONV2, w2=True, out=out, opts=BIG)
        f += conv_case(f"conv3_256x256_{out}", CONV3, out=out, opts=BIG)
    f += conv_case("conv3_oddw_256x256", CONV3_ODD, opts=BIG)
    f += conv_case("conv3_oddw_small_f32", CONV3_ODD, out="f32", scale=True)
    f += conv_case("conv4_small", CONV4, out="both")
    f += conv_case("conv4_256x256", CONV4, out="f32", opts=BIG)
    f += conv_case("conv5_small", CONV5, out="both", scale=True)
    f += conv_case("conv5_small_norelu_nobias", CONV5, out="f32", relu=0, bias=False)
    f += conv_case("audio_3x3_natural", AUDIO33, out="both")
    f += conv_case("audio_1x1", AUDIO11, out="both")
    f += conv_case("c32_3x3_ldw320", C32_33, ldw=320)
    f += conv_case("c32_2x2", C32_22, scale=True)
    return f


def family_tall():
    """the 512x128 tile at the planner's threshold, its three store forms, and the 256x128 tile one image row below it"""
    f = []
    for out in OUT_FORMS:
        f += conv_case(f"tall_{out}", TALL, out=out)
    f += conv_case("tall_below_threshold", TALL_BELOW, out="both")
    _DATA.clear()
    return f


def family_tall_rowmap():
    f = []
    for out in OUT_FORMS:
        f += conv_case(f"tall_rowmap_{out}", TALL, out=out, s2=S2_TALL)
    _DATA.clear()
    return f


def family_rowmap():
    """row map only (conv2's form, op 0, no const image): the non-SPR tiles, the three store forms each"""
    f = []
    for out in OUT_FORMS:
        f += conv_case(f"rowmap_small_{out}", CONV2, out=out, s2=S2_OH5)
        f += conv_case(f"rowmap_small_w2_{out}", CONV2, w2=True, out=out, s2=S2_OH5)
        f += conv_case(f"rowmap_256x128_{out}", CONV2, out=out, s2=S2_OH5, opts=BIG)
        f += conv_case(f"rowmap_256x128_w2_{out}", CONV2, w2=True, out=out, s2=S2_OH5, opts=BIG)
        f += conv_case(f"rowmap_256x256_{out}", CONV3, out=out, s2=S2_OH5, opts=BIG)
    f += conv_case("rowmap_conv5_small", CONV5, out="both", s2=[0, 8, 3])
    f += conv_case("rowmap_conv5_small_norelu", CONV5, out="f32", relu=0, scale=True, s2=[0, 8, 3])
    return f


def family_rowconst():
    """row map + const image (conv3 / conv4 / conv5's form, op 1 / 2 / 3): the five SPR instances, the three store forms each"""
    f = []
    for out in OUT_FORMS:
        f += conv_case(f"const_conv5_small_{out}", CONV5, out=out, s2=S2_CONV5, op=3, use_const=True)
        f += conv_case(f"const_conv5_small_w2_{out}", CONV5, w2=True, out=out, s2=S2_CONV5, op=3, use_const=True)
        f += conv_case(f"const_conv5_256x128_{out}", CONV5, out=out, s2=S2_CONV5, op=3, use_const=True, opts=BIG)
        f += conv_case(f"const_conv5_256x128_w2_{out}", CONV5, w2=True, out=out, s2=S2_CONV5, op=3, use_const=True, opts=BIG)
        f += conv_case(f"const_conv3_256x256_{out}", CONV3, out=out, s2=S2_CONV3, op=1, use_const=True, opts=BIG)
    f += conv_case("const_conv3_oddw_small", CONV3_ODD, out="both", s2=S2_CONV3, op=1, use_const=True)
    f += conv_case("const_conv4_small", CONV4, out="both", s2=S2_CONV4, op=2, use_const=True)
    f += conv_case("const_conv4_256x256", CONV4, s2=S2_CONV4, op=2, use_const=True, opts=BIG)
    # without ReLU a NaN that was read reaches the output as NaN (ReLU turns it into 0)
    f += conv_case("const_conv4_small_norelu", CONV4, out="f32", relu=0, s2=S2_CONV4, op=2, use_const=True)
    f += conv_case("const_conv3_256x256_norelu", CONV3_ODD, out="both", relu=0, scale=True, s2=S2_CONV3, op=1, use_const=True, opts=BIG)
    # every image keeps a single output row: 54 compacted rows, less than one tile, while the grid was planned from the full M
    f += conv_case("const_conv3_one_row_each", CONV3, out="both", s2=[9] * 9, op=1, use_const=True, opts=BIG)
    f += conv_case("const_conv3_one_row_each_small", CONV3, s2=[9] * 9, op=1, use_const=True)
    # s2 = 0 everywhere: the map is the identity and rin = 0
    f += conv_case("const_conv3_identity", CONV3, out="both", s2=[0] * 9, op=1, use_const=True, opts=BIG)
    f += conv_case("const_conv5_identity", CONV5, s2=[0] * 3, op=3, use_const=True)
    return f


def family_staged():
    """the conv forms of the register-staged kernel"""
    f = []
    f += conv_case("staged_conv1", CONV1, out="both", scale=True)
    f += conv_case("staged_conv1_w2", CONV1, w2=True, out="f32", scale=True)
    f += conv_case("staged_m255", CONV5_M255, out="both")
    f += conv_case("staged_glds_off_w2", CONV5, w2=True, out="f32", opts=dict(gemm_glds=0))
    f += conv_case("staged_n192", CONV5_N192, out="both")
    f += conv_case("staged_c32_n128", CONV5_C32, out="f32", relu=0)
    return f


def family_persistence():
    """several rounds per workgroup (6 tiles on 1 and 2 workgroups), and one workgroup per tile"""
    f = []
    for label, opts in (("numcu1", dict(num_cu=1)), ("numcu2", dict(num_cu=2)), ("persistent_off", dict(gemm_persistent=0)),
                        ("numcu1_counted_off", dict(num_cu=1, gemm_counted=0))):
        f += conv_case(f"const_conv3_{label}", CONV3, s2=S2_CONV3, op=1, use_const=True, opts=opts)
        f += conv_case(f"const_conv3_{label}_both", CONV3, out="both", s2=S2_CONV3, op=1, use_const=True, opts=opts)
    f += conv_case("rowmap_conv2_numcu1", CONV2, w2=True, s2=S2_OH5, opts=dict(num_cu=1))
    f += conv_case("conv3_numcu2", CONV3, out="frag16", opts=dict(num_cu=2))
    return f


def family_bf16():
    """the second build of the kernels (precision mode 4)"""
    f = []
    f += conv_case("bf_staged_conv1", CONV1, out="both", scale=True, bf=True)
    f += conv_case("bf_conv2_small", CONV2, bf=True)
    f += conv_case("bf_conv2_small_rowmap_both", CONV2, out="both", s2=S2_OH5, bf=True)
    f += conv_case("bf_conv4_256x256", CONV4, out="frag16", bf=True, opts=BIG)
    f += conv_case("bf_const_conv4_256x256", CONV4, out="both", s2=S2_CONV4, op=2, use_const=True, bf=True, opts=BIG)
    return f


FAMILIES = dict(tiles=family_tiles, tall=family_tall, tall_rowmap=family_tall_rowmap, rowmap=family_rowmap, rowconst=family_rowconst,
                staged=family_staged, persistence=family_persistence, bf16=family_bf16)
_RAN = {}


def run_family(name):
    """Each family runs once per session; the coverage test at the end runs whatever has not run yet."""
    if name not in _RAN:
        _RAN[name] = FAMILIES[name]()
        print("worst observed/bound so far:", {k: round(v, 3) for k, v in RATIOS.items()})
    return _RAN[name]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_conv_gemm_vs_fp64(family):
    fails = run_family(family)
    assert not fails, "\n".join(fails)


def test_conv_instance_coverage():
    """Every conv instance of the table was launched on its own by a case above, and nothing outside the list."""
    for name in FAMILIES:
        run_family(name)
    missing, extra = CONV_INSTANCES - SEEN, SEEN - CONV_INSTANCES
    assert not missing and not extra, f"instances never run: {sorted(missing)}; not in the list: {sorted(extra)}"


def test_conv_launcher_rejections():
    """What the conv check point and the planner refuse comes back as JG_ERR_ARG, launches nothing and leaves the outputs untouched."""
    def refused(g, pin_plan, opts=None, s2=None, op=0, use_const=False, ldw=None, out="rows16", **change):
        ldw = ldw or g["KH"] * g["KW"] * g["C"] + 8
        d = conv_data(g, False, False, None, 0, False, ldw, 11)
        kw, pk, o32, o16 = conv_args(g, d, w2=False, out=out, scale=False, bias=True, relu=1, ldw=ldw, bf=False, s2=s2, op=op, use_const=use_const)
        kw.update(change)
        pk.update({k: v for k, v in change.items() if k in ("relu", "K", "ldc", "ldw")})
        e = engine(**(opts or {}))
        assert rejects(e.debug_conv_check, **kw), (g, change)
        assert e.debug_last_kernel() == ""
        torch.cuda.synchronize()
        for buf in (o32, o16):
            assert buf is None or guards_intact(buf, 0, 0), "a refused launch wrote to its output"
        if pin_plan:
            assert planned(pk, opts) == "rejected", (g, change)

    refused(CONV5_M255, True, s2=[0, 1, 2])                                   # row map with M < 256: only the LDS-DMA kernel knows the compaction
    refused(CONV5, True, s2=[0, 8, 3], opts=dict(gemm_glds=0))                # row map with the LDS-DMA kernels off
    refused(CONV5, True, s2=S2_CONV5, op=3, use_const=True, opts=dict(gemm_glds=0))
    refused(C32_33, True, s2=[0] * 11)                                        # row map on N = 64: neither the C = 32 instance nor the staged kernel
    refused(CONV5, False, relu=2)                                             # the conv epilogues know ReLU only
    refused(CONV5, False, K=CONV5["C"] * 9 - 64)                              # K != KH KW C
    refused(CONV5, False, K=CONV5["C"] * 9 + 64, ldw=CONV5["C"] * 9 + 64)
    refused(CONV5, False, s2=[0, 9, 3])                                       # op 0: s = 9 = OH leaves image 1 no row
    refused(CONV5, False, s2=[0, 22, 3], op=3, use_const=True)                # op 3: s = 22 // 2 - 2 = 9
    refused(CONV5, False, s2=[0, 256, 3])                                     # outside the map entry's top byte
    refused(CONV5, False, s2=[0, -1, 3])
    refused(CONV5, True, out="both", ldc=CONV5["N"] + 2)                      # ldc % 4 != 0: every store writes 4 columns
    refused(CONV5, True, ldw=CONV5["C"] * 9 + 4)                              # ldw % 8 != 0: the loaders take 16-byte pieces of a weight row
    refused(CONV5_M255, True, ldw=CONV5["C"] * 9 + 4)


# ---- max-pool (launch_maxpool3x3s2): exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [False, True], ids=["fp16", "bf16"])
def test_maxpool_exact(bf):
    e = engine(prec=4 if bf else None)
    d16 = dt16(bf)
    gen = torch.Generator().manual_seed(21)
    for H, W, C in ((10, 10, 256), (11, 10, 8), (7, 9, 64)):
        OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        for nimg in (1, 5):
            x = urnd(gen, (nimg, H, W, C), -4, 4).to(d16)
            cimg = urnd(gen, (H, W, C), -4, 4).to(d16)
            # in_op 3: rin = s2 // 2 - 2 -- none (two ways), one row, in between, the whole image
            skips = [None, [0] * nimg, ([2 * (H + 2), 5, 6, 2 * (H // 2 + 2), 2 * (H + 1)] * 2)[:nimg] if nimg > 1 else [2 * (H + 2)], [7] * nimg]
            for s2 in skips:
                xref, xdev = x.clone(), x.clone()
                if s2 is not None:
                    for i, v in enumerate(s2):
                        rin = skip_decode(v, 3)
                        assert rin <= H
                        xref[i, :rin] = cimg[:rin]
                        xdev[i, :rin] = float("nan")                     # the left-out input rows: nobody may read them
                inbuf = torch.full((nimg + 2, H, W, C), float("nan"), dtype=d16)
                inbuf[1:nimg + 1] = xdev
                inbuf = inbuf.to(DEV)
                cbuf = torch.full((2, H, W, C), float("nan"), dtype=d16)
                cbuf[0] = cimg
                out = guarded(nimg * OH * OW, C, d16)
                e.debug_maxpool(inbuf[1:nimg + 1], out, s2_host=s2, in_op=3, const_in=cbuf.to(DEV) if s2 is not None else None)
                torch.cuda.synchronize()
                assert e.debug_last_kernel() == "maxpool_kernel"
                ref = F.max_pool2d(xref.double().permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).reshape(nimg * OH * OW, C).to(d16)
                got = out[:nimg * OH * OW].cpu()
                assert guards_intact(out, nimg * OH * OW, C), (H, W, C, nimg, s2)
                assert torch.equal(got, ref), (H, W, C, nimg, s2, int((got != ref).sum()))
    z = torch.zeros(5 * 10 * 10 * 64, dtype=d16, device=DEV)
    xs = z.view(5, 10, 10, 64)
    assert rejects(e.debug_maxpool, xs, z, s2_host=[0, 0, 0, 0, 26], in_op=3, const_in=z)         # rin = 11 > H
    assert rejects(e.debug_maxpool, xs, z, s2_host=[0] * 5, in_op=3)                              # s2 without the const image
    assert rejects(e.debug_maxpool, z.view(5, 10, 160, 4), z)                                     # C % 8 != 0
    assert rejects(e.debug_maxpool, z.view(50, 2, 10, 32), z)                                     # H < 3
    assert e.debug_last_kernel() == ""


# ---- compaction row maps (launch_conv_rowmaps): exact -----------------------------------------------------------------------------------
GS_LAYERS = [(20, 37), (10, 19), (10, 10), (10, 10)]      # conv2 .. conv5 of GestSync, ops 0 .. 3
FILL = 0x5A5A5A5A


def rowmap_ref(s2, OH, OW, op):
    s = np.array([skip_decode(int(v), op) for v in s2], np.int64)
    cnt = (OH - s) * OW
    base = np.concatenate([[0], np.cumsum(cnt)])
    per = OH * OW
    m = np.concatenate([np.arange(i * per + s[i] * OW, (i + 1) * per, dtype=np.int64) | (int(s2[i]) << 24) for i in range(len(s2))])
    return m.astype(np.int32), base.astype(np.int32), int(base[-1])


@pytest.mark.parametrize("NF", [1, 5, 1023, 1024, 1025, 2500])         # 1, 2 and 3 images per thread of the scan
def test_conv_rowmaps_exact(NF):
    e = engine()
    rng = np.random.default_rng(NF)
    for label, s2 in (("random", rng.integers(0, 20, NF)), ("zero", np.zeros(NF, np.int64)), ("max", np.full(NF, 19))):
        res = e.debug_conv_rowmaps(s2, GS_LAYERS, fill=FILL)
        assert len(res) == 4
        for op, ((OH, OW), (m, base, total)) in enumerate(zip(GS_LAYERS, res)):
            mref, bref, tref = rowmap_ref(s2, OH, OW, op)
            assert total == tref, (label, op, total, tref)
            assert np.array_equal(base, bref), (label, op)
            assert np.array_equal(m[:total], mref), (label, op, int((m[:total] != mref).sum()))
            assert (m[total:] == FILL).all(), (label, op, "the tail of the map buffer was written")
            assert ((m[:total] & 0xffffff) < NF * OH * OW).all() and np.array_equal((m[:total].view(np.uint32) >> 24), np.repeat(s2, np.diff(bref)))
    if NF == 5:
        res = e.debug_conv_rowmaps([3, 0, 19, 7, 12], GS_LAYERS[:2], fill=FILL)      # fewer layers than four
        for op, ((OH, OW), (m, base, total)) in enumerate(zip(GS_LAYERS, res)):
            mref, bref, tref = rowmap_ref([3, 0, 19, 7, 12], OH, OW, op)
            assert total == tref and np.array_equal(base, bref) and np.array_equal(m[:total], mref) and (m[total:] == FILL).all()


def test_conv_rowmaps_rejections():
    e = engine()
    assert rejects(e.debug_conv_rowmaps, np.zeros(22672, np.int32), GS_LAYERS[:1])            # NF * 740 >= 2^24: the 24-bit row index
    assert e.debug_last_kernel() == ""
    assert rejects(e.debug_conv_rowmaps, [0, 1], GS_LAYERS + [(10, 10)])                      # five layers
    assert rejects(e.debug_conv_rowmaps, [0, 1], [])
    assert rejects(e.debug_conv_rowmaps, [0, 21], GS_LAYERS[:1])                              # s = 21 > OH
    assert rejects(e.debug_conv_rowmaps, [0, 256], GS_LAYERS[:1])
