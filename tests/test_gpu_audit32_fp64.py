"""Kernel-level checks of the fp32 audit kernels (jegal_amd/csrc/audit32.hip) against float64 at tile and image edges (run with -m gpu).

Every case runs ONE production launch through a check point of include/jegal_hip.h: jg_debug_conv32 (launch_gemm32 with conv = 1, the
geometry from engine::geom), jg_debug_stack_frames32, jg_debug_maxpool32, jg_debug_group_mean32 and jg_debug_zero_tail32.  Cases,
references and bounds come from tests/audit32_fp64_cases.py, where tests/test_audit32_cases_cpu.py checks them without a GPU.

Guards, all inside allocations: conv inputs are [one NaN image | nimg images | one NaN image], W holds NaN in the columns K .. ldw-1, in 16
extra rows and in front of an offset pointer; outputs carry 128 guard rows and ldc - N guard columns of SENT32; the sources of the exact
families carry NaN (u8: complemented) frames, images, rows and groups around what the kernel may read.  Every output element is compared
and the guards are checked intact.  Every argument set that could leave a buffer is refused by the check point before anything is
enqueued: each family asserts its rejections, after which the output still holds its sentinel.

Conv cases print observed / bound (element-wise 2 K u (conv2d(|in|, |w|) |scale| + |bias|), norm-wise 2 sqrt(K) u; u = 2^-24) and must
stay <= 1; stack_frames32, maxpool32 and zero_tail32 must be equal bit for bit; group_mean32 is held to (L + 1) u sum|x| / L.  The names of
the launched instances must cover gemm32_kernel<1,1,64>, <1,0,64>, <1,1,128> and <1,0,128>.

Seeded defects these tests were seen to fail on, on the MI355X (each built into a scratch copy of the library, never committed; each by
construction reads and writes inside the framed buffers):
  * two entries of geom()'s tap table swapped: every tap-table case, vector and scalar loader (observed / bound 62 071 .. 1 034 140); the
    natural-order cases are untouched, as they must be;
  * the padding test of both conv loaders dropped: every padded case of all four instances (NaN from the guard images without ReLU;
    47 819 .. 928 459 with it);
  * the `k < K` guards of the weight loader's last quad dropped: the C = 1 and C = 2 cases and the K = 36 threshold cases on both tiles
    (NaN without ReLU; 1.4e6 .. 1.7e6 with it);
  * stack_frames32: the upper, and the lower, frame clamp off by one (bits differ from the first clamped case on);
  * maxpool32: the window one column to the right (45 elements of the first shape);
  * zero_tail32: the first zeroed row kept;  group_mean32: the sum divided by L + 1 (the L = 1 bit comparison).
"""
import pytest
import torch

import audit32_fp64_cases as C
import test_gpu_kernels_fp64 as K64
from test_gpu_kernels_fp64 import DEV, engine, guarded, guards_intact, note, rejects

pytestmark = pytest.mark.gpu

SEEN = set()
_RAN = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in K64._ENGINES.values():
        e.close()
    K64._ENGINES.clear()
    C._DATA.clear()


def launched(e, name):
    torch.cuda.synchronize()
    assert e.debug_last_kernel() == name, (e.debug_last_kernel(), name)


def geometry(g):
    return [g[k] for k in ("nimg", "H", "W", "C", "KH", "KW", "SH", "SW", "PH", "PW", "reorder")]


# ================================================================================================================================ conv
def conv32_case(name, g, o, family):
    """One conv launch vs float64 -> list of failures."""
    d = C.conv32_data(g)
    k = C.case_opts(g, o)
    M, N, K = d["M"], g["N"], d["K"]
    e = engine()
    inbuf = d["inbuf"].to(DEV)
    wbuf = C.w_buffer(d, k["ldw"], k["w_off"]).to(DEV)
    out = guarded(M, k["ldc"], torch.float32)
    e.debug_conv32(inbuf[1:], *geometry(g), wbuf[k["w_off"]:], k["ldw"], N, out, k["ldc"], scale=d["sc"].to(DEV) if k["scale"] else None,
                   bias=d["bi"].to(DEV) if k["bias"] else None, act=k["act"])
    torch.cuda.synchronize()
    kname = e.debug_last_kernel()
    assert kname == k["kname"], f"{name}: launched {kname}, launch_gemm32's rule says {k['kname']}"
    SEEN.add(kname)
    v, eb, nb = C.conv32_expect(d, k["act"], k["scale"], k["bias"])
    fails = []
    if not guards_intact(out, M, N):
        fails.append(f"{name}: guard of out overwritten")
    r = C.conv32_ratio(out[:M, :N].cpu(), v, eb, nb)
    note("conv32_" + family, r)
    print(f"{name:32s} {kname:24s} M={M} N={N} K={K} act={k['act']} observed/bound {r:.3f}")
    if not r <= 1:
        fails.append(f"{name}: observed/bound {r:.3f} ({kname})")
    return fails


def run_family(family):
    """Each family runs once per session; the coverage test runs whatever has not run yet.  The operands of a family are freed behind it."""
    if family not in _RAN:
        fails = []
        for name, g, o in C.CONV_FAMILIES[family]:
            fails += conv32_case(name, g, o, family)
        C._DATA.clear()
        torch.cuda.empty_cache()
        print(f"worst observed/bound, conv32_{family}: {K64.RATIOS.get('conv32_' + family, 0.0):.3f}")
        _RAN[family] = fails
    return _RAN[family]


@pytest.mark.parametrize("family", list(C.CONV_FAMILIES))
def test_conv32_vs_fp64(family):
    fails = run_family(family)
    assert not fails, "\n".join(fails)


def test_conv32_instance_coverage():
    """All four conv instances of gemm32_kernel were launched on their own by a case above, and nothing else."""
    for family in C.CONV_FAMILIES:
        run_family(family)
    assert SEEN == C.CONV32_INSTANCES, SEEN ^ C.CONV32_INSTANCES


def test_conv32_rejections():
    """What jg_debug_conv32 and launch_gemm32 refuse comes back as JG_ERR_ARG, launches nothing and leaves the output untouched."""
    e = engine()
    g = C.CONV5
    d = C.conv32_data(g)
    k = C.case_opts(g, {})
    inbuf, wbuf = d["inbuf"].to(DEV), C.w_buffer(d, k["ldw"], 0).to(DEV)
    out = guarded(d["M"], k["ldc"], torch.float32)
    base = dict(x=inbuf[1:], Wt=wbuf, ldw=k["ldw"], N=g["N"], out=out, ldc=k["ldc"], act=1,
                **{key: g[key] for key in ("nimg", "H", "W", "C", "KH", "KW", "SH", "SW", "PH", "PW", "reorder")})
    bad = [dict(x=None), dict(Wt=None), dict(out=None),                                             # null pointers
           dict(nimg=0), dict(H=0), dict(W=-1), dict(C=0), dict(KH=0), dict(KW=0), dict(SH=0), dict(SW=0), dict(N=0), dict(PH=-1), dict(PW=-1),
           dict(ldw=d["K"] - 1), dict(ldc=g["N"] - 1),
           dict(H=1, PH=0), dict(W=2, PW=0),                                                        # the kernel larger than the padded image
           dict(KH=16, PH=8),                                                                       # a tap code has four bits per coordinate
           dict(nimg=2 ** 31 // 99 + 1),                                                            # M = nimg 99 >= 2^31
           dict(act=3), dict(act=-1),
           dict(C=48, ldw=9 * 48), dict(C=3, ldw=27)]                                               # C no power of two: the launcher's own rule
    for change in bad:
        assert rejects(e.debug_conv32, **dict(base, **change)), change
        assert e.debug_last_kernel() == "", change
    torch.cuda.synchronize()
    assert guards_intact(out, 0, 0), "a refused launch wrote to its output"
    C._DATA.clear()


# ====================================================================================================================== exact families
def test_stack_frames32_exact():
    e = engine()
    B, H, W = 2, 5, 7
    for u8 in (True, False):
        for T in C.STACK_T:
            c = C.stack32_case(u8, B, T, H, W)
            src = c["buf"].to(DEV).view(-1)[c["offset"]:]          # frame 0 of clip 0: a guard frame in front of it and behind every clip
            for pad in C.STACK_PAD:
                n = B * max(T + 2 * pad - 4, 1) * H * W
                out = guarded(n, 16, torch.float32)
                if T + 2 * pad < 5:
                    assert rejects(e.debug_stack_frames32, src, c["strides"], B, T, pad, H, W, out)
                    continue
                e.debug_stack_frames32(src, c["strides"], B, T, pad, H, W, out)
                launched(e, f"stack_frames32_kernel<{'uint8_t' if u8 else 'float'}>")
                assert guards_intact(out, n, 16), (u8, T, pad)
                ref = C.stack32_ref(c, u8, T, pad).reshape(n, 16)
                got = out[:n].cpu()
                assert C.same_bits(got, ref), (u8, T, pad, int((C.bits(got) != C.bits(ref)).sum()))
    sb, st, sh, sw, sc = c["strides"]
    out = guarded(n, 16, torch.float32)
    assert rejects(e.debug_stack_frames32, src, (2 * sb, st, sh, sw, sc), B, T, 2, H, W, out)          # the second clip would lie outside src
    assert rejects(e.debug_stack_frames32, src, (sb, st, sh, -1, sc), B, T, 2, H, W, out)
    assert rejects(e.debug_stack_frames32, src, c["strides"], B, T, 2, H, W, out.view(-1)[1:])          # dst not 16-byte aligned
    assert rejects(e.debug_stack_frames32, src, c["strides"], 0, T, 2, H, W, out)
    assert rejects(e.debug_stack_frames32, src, c["strides"], B, T, 2, 0, W, out)
    assert rejects(e.debug_stack_frames32, None, c["strides"], B, T, 2, H, W, out)
    assert rejects(e.debug_stack_frames32, src, c["strides"], B, T, 2, H, W, None)
    assert e.debug_last_kernel() == ""
    torch.cuda.synchronize()
    assert guards_intact(out, 0, 0)


def test_maxpool32_exact():
    e = engine()
    for shape in C.POOL_SHAPES:
        nimg, H, W, Cc = shape
        c = C.pool_case(*shape)
        rows = nimg * c["OH"] * c["OW"]
        buf = c["buf"].to(DEV)
        out = guarded(rows, Cc, torch.float32)
        e.debug_maxpool32(buf[1:nimg + 1], out)
        launched(e, "maxpool32_kernel")
        assert guards_intact(out, rows, Cc), shape
        got = out[:rows].cpu()
        ref = c["ref"].reshape(rows, Cc)
        assert torch.equal(got, ref), (shape, int((got != ref).sum()))
    out = guarded(rows, Cc, torch.float32)
    z = torch.zeros(2 * 10 * 10 * 256 + 4, dtype=torch.float32, device=DEV)
    zi = z[:-4]
    assert rejects(e.debug_maxpool32, zi[:50400].view(2, 10, 420, 6), out)            # C % 4 != 0
    assert rejects(e.debug_maxpool32, zi.view(100, 2, 4, 64), out)                    # H < 3
    assert rejects(e.debug_maxpool32, zi.view(100, 4, 2, 64), out)                    # W < 3
    assert rejects(e.debug_maxpool32, z[1:-3].view(2, 10, 10, 256), out)              # 16-byte loads
    assert rejects(e.debug_maxpool32, zi.view(2, 10, 10, 256), out.view(-1)[1:])      # 16-byte stores
    assert rejects(e.debug_maxpool32, zi[:0].view(0, 10, 10, 256), out)
    assert rejects(e.debug_maxpool32, zi.view(2, 10, 10, 256), None)
    assert e.debug_last_kernel() == ""
    torch.cuda.synchronize()
    assert guards_intact(out, 0, 0)


def test_zero_tail32_exact():
    e = engine()
    for H in C.ZT_H:
        for row_elems in C.ZT_ROW_ELEMS:
            for halvings in C.ZT_HALVINGS:
                c = C.zero_tail32_case(H, row_elems, halvings)
                B = len(c["valid"])
                buf = guarded(B * H, row_elems, torch.float32)
                buf.view(torch.int32)[:B * H] = c["x"].reshape(B * H, row_elems).to(DEV)
                e.debug_zero_tail32(buf, c["valid"], halvings, B, H, row_elems)
                launched(e, "zero_tail32_kernel")
                assert guards_intact(buf, B * H, row_elems), (H, row_elems, halvings)
                got = buf.view(torch.int32)[:B * H].cpu()
                assert torch.equal(got, c["ref"].reshape(B * H, row_elems)), (H, row_elems, halvings)
    buf = guarded(B * H, 8, torch.float32)
    assert rejects(e.debug_zero_tail32, buf, c["valid"], 1, B, H, 6)                    # row_elems % 4: 16-byte stores
    assert rejects(e.debug_zero_tail32, buf, c["valid"][:-1], 1, B, H, 8)               # one entry per clip
    assert rejects(e.debug_zero_tail32, buf, c["valid"] + [1], 1, B, H, 8)
    assert rejects(e.debug_zero_tail32, buf, None, 1, B, H, 8)
    assert rejects(e.debug_zero_tail32, buf, c["valid"], -1, B, H, 8)
    assert rejects(e.debug_zero_tail32, buf, c["valid"], 31, B, H, 8)
    assert rejects(e.debug_zero_tail32, buf.view(-1)[1:], c["valid"], 1, B, H, 8)
    assert rejects(e.debug_zero_tail32, buf, [], 1, 0, H, 8)
    assert rejects(e.debug_zero_tail32, buf, c["valid"], 1, B, 0, 8)
    assert rejects(e.debug_zero_tail32, None, c["valid"], 1, B, H, 8)
    assert e.debug_last_kernel() == ""
    torch.cuda.synchronize()
    assert guards_intact(buf, 0, 0)


# ============================================================================================================================ bounded
def test_group_mean32():
    e = engine()
    fails = []
    for L in C.GM_L:
        for D in C.GM_D:
            for groups in C.GM_GROUPS:
                c = C.group_mean32_case(groups, L, D)
                buf = c["buf"].to(DEV)
                out = guarded(groups, D, torch.float32)
                e.debug_group_mean32(buf[L:], groups, L, D, out)
                launched(e, "group_mean32_kernel")
                assert guards_intact(out, groups, D), (L, D, groups)
                got = out[:groups].cpu()
                if L == 1:
                    assert C.same_bits(got, c["x"]), (D, groups)
                r = C.ratio(got, c["ref"], c["bound"])
                note("group_mean32", r)
                print(f"group_mean32 L {L} D {D} groups {groups} observed/bound {r:.3f}")
                if not r <= 1:
                    fails.append(f"group_mean32 L {L} D {D} groups {groups}: observed/bound {r:.3f}")
    x = buf[L:]
    out = guarded(groups, D, torch.float32)
    assert rejects(e.debug_group_mean32, x, groups, L, 6, out)          # D % 4: 16-byte accesses
    assert rejects(e.debug_group_mean32, x, groups, 0, D, out)
    assert rejects(e.debug_group_mean32, x, 0, L, D, out)
    assert rejects(e.debug_group_mean32, x, groups, L, 0, out)
    assert rejects(e.debug_group_mean32, x.view(-1)[1:], 1, L, D, out)
    assert rejects(e.debug_group_mean32, x, groups, L, D, out.view(-1)[1:])
    assert rejects(e.debug_group_mean32, None, groups, L, D, out)
    assert e.debug_last_kernel() == ""
    torch.cuda.synchronize()
    assert guards_intact(out, 0, 0)
    print(f"worst observed/bound, group_mean32: {K64.RATIOS.get('group_mean32', 0.0):.3f}")
    assert not fails, "\n".join(fails)
