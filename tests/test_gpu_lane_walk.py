"""Walk factors (options lane_walk_gemm / _conv / _lnf / _conv1, jegal_amd/csrc/shared.h): inside a two-lane batch a persistent kernel launches
factor x num_cu workgroups instead of num_cu.  Which workgroup computes a tile must not change a bit of it (run with -m gpu).

Every kernel case runs ONE launch per factor 1 .. 4 through the check points of the sibling files (option debug_lanes = 1 marks the launch
as part of a two-lane batch), on a shape whose grid exceeds the device's CUs from factor 2 on, and asserts
  * the float64 agreement of the sibling test, at its tolerance (test_gpu_kernels_fp64.gemm_case, the LayerNorm-fused bound of
    ln_fused_case, tiers A and B of test_gpu_conv1_fp64), and
  * torch.equal on the whole output buffers, guards included, between factor 1 and every other factor.
The end-to-end case runs extract_gesture on 8 clips x 90 frames under ws_poison: factor 1, the default factors, every factor at 4 and
one stream give the same bits.

conv1, one clip of T = 100 frames with pad 4 (104 positions, 520 strips): the frames alternate between two images, so the positions read
only a handful of distinct frame 5-tuples and the float64 reference (conv1_fp64_cases.epilogue on the per-frame sums) is computed once per
tuple.  Rows 0 .. 109 of both images are zero: with conv1_zero_skip = 1 the skip table and the constant fill run, with 0 they do not.

The conv case is a 1 x 1 convolution (K = 64, the shortest k loop of the 256 x 256 conv instance) of 5 400 images of 6 x 5 pixels with a
row map that skips 0 .. 2 leading rows per image: 135 000 computed rows, 528 tiles.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv1_fp64_cases as C
import test_gpu_conv1_fp64 as C1
import test_gpu_conv_fp64 as CV
import test_gpu_kernels_fp64 as K64
from test_gpu_kernels_fp64 import DEV, SENT16, U, engine, operand, ulp16, urnd

pytestmark = pytest.mark.gpu

FACTORS = (1, 2, 3, 4)


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in K64._ENGINES.values():
        e.close()
    K64._ENGINES.clear()
    C1._LOADED.clear()


class captured:
    """Records the keyword arguments of every call of a check point (debug_gemm_check or debug_conv_check) (the output tensors among them) while a sibling's case function runs."""

    def __init__(self, entry="debug_gemm_check"):
        self.entry = entry

    def __enter__(self):
        from jegal_amd._lib import Engine
        self.cls, self.orig, self.calls = Engine, getattr(Engine, self.entry), []

        def spy(eng, **kw):
            self.calls.append(dict(kw))
            return self.orig(eng, **kw)
        setattr(Engine, self.entry, spy)
        return self.calls

    def __exit__(self, *exc):
        setattr(self.cls, self.entry, self.orig)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("w2", [False, True], ids=["single", "hi+lo"])
def test_plain_gemm_128x128(w2):
    """M = 4096, N = 2304, K = 128 on the 128 x 128 tile: 576 tiles."""
    from jegal_amd._lib import gemm_plan
    M, N, K = 4096, 2304, 128
    assert 576 > num_cu()
    first = None
    for f in FACTORS:
        opts = dict(gemm_tile=1, debug_lanes=1, lane_walk_gemm=f)
        with captured() as calls:
            fails = K64.gemm_case(f"walk{f}{'_w2' if w2 else ''}", M, N, K, w2=w2, out="both", opts=opts)
        assert not fails, "\n".join(fails)
        kw = calls[-1]
        grid = gemm_plan(num_cu=num_cu(), opts=opts, **kw)[1]
        assert grid == min(576, f * num_cu()) and (f == 1 or grid > num_cu())
        out = (kw["out32"], kw["out16"])
        if first is None:
            first = out
        else:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, out)), f"factor {f} differs from factor 1"


LNF_SHAPE = (66560, 512, 64, 3328, 20)          # M, N, K, rows per clip, clips: 520 tiles of 128 x 512
LNF_FACTOR1 = {}                                # "bits": the plane the factor-1 out-of-place launch of these operands left (CPU int16)


@functools.lru_cache(maxsize=1)
def ln_fused_clip_bias_operands():
    """The operands of test_ln_fused_clip_bias on the host, built once (tests/test_gpu_token_plane_fp64.py launches them in place)."""
    M, N, K, rpc, ncl = LNF_SHAPE
    g = torch.Generator().manual_seed(7)
    a = urnd(g, (M, K)).half().double()
    wh = (urnd(g, (N, K)) / math.sqrt(K) * 2).half().double()
    bias = urnd(g, (N,)).float()
    gam, bet = urnd(g, (N,), 0.5, 1.5).float(), urnd(g, (N,)).float()
    bc = urnd(g, (ncl, N), -2, 2).float()
    R = M // 128
    r16 = urnd(g, (M, N), -2, 2).half()
    plane16 = torch.full((R * 65536 + 65536,), float("nan"), dtype=torch.float16)
    plane16[ln_fused_plane_index()] = r16.ravel()
    return dict(a=a, wh=wh, bias=bias, gam=gam, bet=bet, bc=bc, r16=r16, plane16=plane16)


def ln_fused_plane_index():
    """Where element (m, n) of the LNF_SHAPE token rows lies in the tiled plane, row-major over (m, n)."""
    M, N = LNF_SHAPE[:2]
    m = np.arange(M, dtype=np.int64)[:, None]
    n = np.arange(N, dtype=np.int64)[None, :]
    return torch.from_numpy(((m >> 7) * 65536 + (n >> 6) * 8192 + ((m & 127) >> 4) * 1024 + ((n & 63) >> 4) * 256 + (m & 15) * 16 + (n & 15)).ravel())


def ln_fused_clip_bias_kw(ops):
    """... on the device, as the keyword arguments of debug_gemm_check (out16 is the caller's)."""
    M, N, K, rpc, ncl = LNF_SHAPE
    return dict(A=operand(ops["a"], K, torch.float16), lda=K, Wh=operand(ops["wh"], K, torch.float16), ldw=K, M=M, N=N, K=K, bias=ops["bias"].to(DEV),
                ln_w=ops["gam"].to(DEV), ln_b=ops["bet"].to(DEV), res16=ops["plane16"].to(DEV), bias_clip=ops["bc"].to(DEV), rpc=rpc, nclips=ncl)


def ln_fused_clip_bias_launch(kw, f, out16):
    """One launch at walk factor f inside a two-lane batch; the instance and the grid are asserted."""
    from jegal_amd._lib import gemm_plan
    opts = dict(debug_lanes=1, lane_walk_lnf=f)
    e = engine(**opts)
    e.debug_gemm_check(out16=out16, **kw)
    torch.cuda.synchronize()
    name, grid = gemm_plan(num_cu=num_cu(), opts=opts, out16=out16, **kw)[:2]
    assert e.debug_last_kernel() == name == "gemm_glds_kernel<0,0,8,1,8,1,0,0,0>"
    assert grid == min(520, f * num_cu()) and (f == 1 or grid > num_cu())
    return out16


def ln_fused_sentinel_plane():
    return torch.full((LNF_SHAPE[0] // 128 * 65536 + 65536,), SENT16, dtype=torch.int16, device=DEV).view(torch.float16)


def ln_fused_clip_bias_factor1_bits(kw):
    """The plane the factor-1 out-of-place launch leaves, as CPU int16: launched once per session, by whichever test asks first."""
    if "bits" not in LNF_FACTOR1:
        LNF_FACTOR1["bits"] = bits(ln_fused_clip_bias_launch(kw, 1, ln_fused_sentinel_plane())).cpu()
    return LNF_FACTOR1["bits"]


def test_ln_fused_clip_bias():
    """Residual + LayerNorm fused, M = 66 560, N = 512, K = 64, per-clip bias with 3328 rows per clip: 520 tiles.  Reference and bound as in
    test_gpu_kernels_fp64.ln_fused_case."""
    M, N, K, rpc, ncl = LNF_SHAPE
    ops = ln_fused_clip_bias_operands()
    a, wh, gam, bet, bc, r16 = (ops[k] for k in ("a", "wh", "gam", "bet", "bc", "r16"))
    R = M // 128
    off16 = ln_fused_plane_index()
    kw = ln_fused_clip_bias_kw(ops)
    first = ln_fused_clip_bias_factor1_bits(kw)
    for f in FACTORS[1:]:
        o = ln_fused_clip_bias_launch(kw, f, ln_fused_sentinel_plane())
        assert torch.equal(bits(o).cpu(), first), f"factor {f} differs from factor 1"
    res = r16.double()
    badd = bc.double()[torch.clamp(torch.arange(M) // rpc, max=ncl - 1)]
    x = a @ wh.T + badd + res
    ex = 2 * K * U * ((a.abs() @ wh.abs().T) + badd.abs() + res.abs())
    del badd, res
    mu = x.mean(1, keepdim=True)
    sig = ((x - mu) ** 2).mean(1, keepdim=True).add(1e-5).sqrt()
    xh = (x - mu) / sig
    del x
    y = xh * gam.double() + bet.double()
    ey = gam.double().abs() * (ex + ex.max(1, keepdim=True).values * (1 + xh.abs())) / sig + 2.0 ** -20 * (gam.double() * xh).abs() + 2 * U * y.abs()
    del ex, xh
    o16 = first.view(torch.float16)
    assert bool((first[R * 65536:] == SENT16).all()), "guard tile of out16 overwritten"
    got = o16[off16].view(M, N).double()
    ratio = float(((got - y).abs() / (ey + ulp16(y))).max()) if got.isfinite().all() else float("inf")
    print(f"ln_fused M={M} K={K} clip=({rpc}, {ncl}) observed/bound {ratio:.3f}")
    assert ratio <= 1


def test_conv_256x256_row_map():
    """The 256 x 256 conv instance with a row map, 528 tiles of computed rows (the kernel counts its tiles from the map's total)."""
    from jegal_amd._lib import gemm_plan
    nimg = 5400
    g = CV.geo(nimg, 6, 5, 64, 256, 1, 1, 1, 1, 0, 0, False)
    s2 = [i % 3 for i in range(nimg)]
    rows = sum((6 - v) * 5 for v in s2)
    assert (rows + 255) // 256 == 528 and 528 > 2 * num_cu()
    first = None
    for f in FACTORS:
        opts = dict(debug_lanes=1, lane_walk_conv=f)
        with captured("debug_conv_check") as calls:
            fails = CV.conv_case(f"walk{f}_rowmap", g, out="rows16", s2=s2, opts=opts)
        assert not fails, "\n".join(fails)
        assert engine(**opts).debug_last_kernel() == "gemm_glds_kernel<0,1,8,2,4,0,0,0,0>"
        pk = dict(M=nimg * 30, N=256, K=64, ldw=calls[-1]["ldw"], ldc=calls[-1]["ldc"], relu=1, Wh=True, bias=True, out16=True,
                  conv=dict(H=6, W=5, C=64, KH=1, KW=1, PH=0, PW=0, tap_table=0, rowmap=True, const_in=False))
        grid = gemm_plan(num_cu=num_cu(), opts=opts, **pk)[1]
        assert grid == min((nimg * 30 + 255) // 256, f * num_cu())
        out = calls[-1]["out16"]
        if first is None:
            first = out
        else:
            assert torch.equal(bits(out), bits(first)), f"factor {f} differs from factor 1"


def test_conv1_one_clip_520_strips():
    """One clip, T = 100, pad 4: 520 strips.  Factors 1 .. 4 x conv1_zero_skip on / off: the same bits, and they are the expected ones."""
    B, T, pad = 1, 100, 4
    P = C.positions(T, pad)
    assert C.strips(B, T, pad) == 520 > num_cu()
    rng = np.random.default_rng(11)
    two = rng.integers(0, 256, (2, C.IH, C.IW, 3), dtype=np.uint8)
    two[:, :110] = 0                                                    # bands 0 .. 7 zero: tiles skipped outright, tile 8 partial
    two = torch.from_numpy(two)
    frames = two[torch.arange(T) % 2][None].contiguous()
    ops = C.operands()
    w = ops["w"]
    wk = torch.cat([w, w.abs()], 0).permute(2, 0, 1, 3, 4).reshape(5 * 2 * C.OC, 3, 7, 7)
    per = [F.conv2d(two[i].permute(2, 0, 1)[None].double(), wk, stride=3)[0].view(5, 2 * C.OC, C.CH, C.CW) for i in range(2)]
    groups = {}
    for p in range(P):
        groups.setdefault(tuple(C.frame_of(p, dt, T, pad) % 2 for dt in range(5)), []).append(p)
    expect = {}
    for ids in groups:
        s = sum(per[ids[dt]][dt] for dt in range(5))
        ref, core, bts, _, exact = C.epilogue(s[:C.OC], s[C.OC:], ops)
        assert exact
        expect[ids] = (ref, core + ulp16(ref), bts)
    e = C1.handle()
    src, ptr = C1.guarded_input(frames)
    n = P * C.PH * C.PW * C.OC
    first = None
    try:
        e.set_option("debug_lanes", 1)
        for f in FACTORS:
            e.set_option("lane_walk_conv1", f)
            for z in (1, 0):
                got = C1.launch(e, dict(conv1_zero_skip=z), ptr, B, T, pad, n).cpu()
                if first is None:
                    first = got
                    g4 = got.view(P, C.PH, C.PW, C.OC)
                    for ids, ps in groups.items():
                        ref, bnd, bts = expect[ids]
                        sub = g4[ps]
                        assert torch.equal(sub, bts[None].expand_as(sub)), f"tier B: positions {ps[:4]}.. (frames {ids})"
                        val = sub.view(torch.float16).double()
                        assert bool(((val - ref[None]).abs() <= bnd[None]).all()), f"tier A: positions {ps[:4]}.. (frames {ids})"
                else:
                    assert torch.equal(got, first), f"factor {f}, conv1_zero_skip={z} differs from factor 1"
    finally:
        e.set_option("debug_lanes", 0)
        e.set_option("lane_walk_conv1", 1)
    del src


def test_extract_gesture_two_lanes_bit_equal():
    """8 clips x 90 frames under ws_poison: factor 1, the default factors, every factor at 4, one stream."""
    from jegal_amd import synth
    from jegal_amd._lib import Engine
    from jegal_amd.gestsync import GestSync
    from jegal_amd.jegal import JEGAL
    frames = torch.from_numpy(synth.synth_frames(5, 8, 90)).to(DEV)
    e = Engine(0)
    try:
        gs = GestSync(engine=e).load_state_dict(synth.gestsync_state_dict(include_unused=False))
        jg = JEGAL(engine=e).load_state_dict(synth.jegal_state_dict())
        e.set_option("ws_poison", 1)
        outs = {}
        for name, opts in (("default", {}), ("factor 1", dict(lane_walk=1)), ("factor 4", dict(lane_walk=4)), ("one stream", dict(dual_stream=0))):
            for k, v in opts.items():          # (the default factors run first, on the untouched handle)
                e.set_option(k, v)
            outs[name] = e.extract_gesture(frames).cpu()
            torch.cuda.synchronize()
        del gs, jg
    finally:
        e.close()
    assert bool(torch.isfinite(outs["factor 1"]).all())
    for name, o in outs.items():
        assert torch.equal(o, outs["factor 1"]), f"{name} differs from factor 1"
