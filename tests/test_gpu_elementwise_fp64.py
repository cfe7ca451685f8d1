"""Kernel-level checks of the element-wise and reduction launchers against float64 (run with -m gpu).

Every case runs ONE production launch through a jg_debug_* check point (include/jegal_hip.h) -- launch_segment_mean, launch_ragged_mean and
launch_l2norm through the public jg_word_pool, jg_pool_mean and jg_l2norm -- on an fp16 and, where the launcher exists in both builds, a bf16
handle.  Cases, references and bounds come from tests/elementwise_fp64_cases.py, where tests/test_elementwise_cases_cpu.py checks them
without a GPU.  Outputs are pre-filled with a sentinel bit pattern and carry guard rows (and guard columns where there is a leading
dimension); inputs carry NaN in every element the kernel must not read.  Everything lies inside an allocation, and every argument set
that could leave one is refused by the check point before anything is enqueued: each test asserts such rejections too.

Bit-exact families compare bits (NaN inputs as NaN-ness); bounded families print and assert observed / bound, the bound derived in the
case module.  A family whose output is 16-bit also prints how many ulps its result lies from the correctly rounded reference
("ulps off"), and layernorm notes its fp32 output under a key of its own: with a 16-bit store the bound is dominated by the store's ulp.
"""
import pytest
import torch

import elementwise_fp64_cases as C
import test_gpu_kernels_fp64 as K64
from test_gpu_kernels_fp64 import DEV, SENT16, dt16, engine, guarded, guards_intact, note, operand, rejects, ulp16

pytestmark = pytest.mark.gpu

BUILDS = pytest.mark.parametrize("bf", [False, True], ids=["fp16", "bf16"])
NAN = float("nan")
NAN16 = 0x7E00


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in K64._ENGINES.values():
        e.close()
    K64._ENGINES.clear()


def eng(bf=False):
    return engine(prec=4 if bf else None)


def framed(x):
    """x on the device inside a buffer with 64 NaN elements in front and behind (floating point only)."""
    flat = torch.full((x.numel() + 128,), NAN, dtype=x.dtype)
    flat[64:64 + x.numel()] = x.reshape(-1)
    return flat.to(DEV)[64:64 + x.numel()].view(x.shape)


def launched(e, name):
    torch.cuda.synchronize()
    assert e.debug_last_kernel() == name, (e.debug_last_kernel(), name)


def state_error(fn, *a, **kw):
    from jegal_amd._lib import JegalError
    with pytest.raises(JegalError) as ei:
        fn(*a, **kw)
    return ei.value.code == -3          # JG_ERR_STATE


def bounded(family, what, got, ref, bound):
    r = C.ratio(got, ref, bound)
    note(family, r)
    print(f"{family:18s} {what:60s} observed/bound {r:.3f}")
    return [] if r <= 1 else [f"{family} {what}: observed/bound {r:.3f}"]


def bounded16(family, what, got, ref, bound, bf):
    """A 16-bit output: the bound + one ulp of the reference; prints the distance from the correctly rounded reference as well."""
    u16 = ulp16(ref, bf)
    off = C.ratio(got, ref.to(dt16(bf)).double(), u16)
    note(family + "_ulps_off", off)
    print(f"{family:18s} {what:60s} ulps off the rounded reference {off:.3f}")
    return bounded(family, what, got, ref, bound + u16)


def report(family, fails):
    print(f"worst observed/bound, {family}: {K64.RATIOS.get(family, 0.0):.3f}")
    assert not fails, "\n".join(fails)


# ======================================================================================================================= bit-exact
@BUILDS
def test_stack_frames_exact(bf):
    e, d16 = eng(bf), dt16(bf)
    B, H, W = 2, 5, 7
    for u8 in (True, False):
        for T in C.STACK_T:
            c = C.stack_case(u8, B, T, H, W)
            src = c["src"].to(DEV) if u8 else framed(c["src"])
            for pad in C.STACK_PAD:
                n = B * max(T + 2 * pad - 4, 1) * H * W
                out = guarded(n, 16, d16)
                if T + 2 * pad < 5:
                    assert rejects(e.debug_stack_frames, src, c["strides"], B, T, pad, H, W, out)
                    continue
                e.debug_stack_frames(src, c["strides"], B, T, pad, H, W, out)
                launched(e, f"stack_frames_kernel<{'uint8_t' if u8 else 'float'}>")
                assert guards_intact(out, n, 16), (u8, T, pad)
                ref = C.stack_ref(c["frames"], T, pad, d16).reshape(n, 16)
                assert C.same_bits(out[:n].cpu(), ref), (u8, T, pad)
    sb, st, sh, sw, sc = c["strides"]
    assert rejects(e.debug_stack_frames, src, (sb + 4, st, sh, sw, sc), B, T, 2, H, W, out)          # the last frame would end outside src
    assert rejects(e.debug_stack_frames, src, (sb, st, sh, -1, sc), B, T, 2, H, W, out)
    assert rejects(e.debug_stack_frames, src, c["strides"], B, T, 2, H, W, out.view(-1)[4:])          # dst not 16-byte aligned
    assert rejects(e.debug_stack_frames, src, c["strides"], 0, T, 2, H, W, out)
    assert e.debug_last_kernel() == ""


@BUILDS
def test_window_gather_rows_exact(bf):
    e, d16 = eng(bf), dt16(bf)
    for B, P, Twin, L, D, shift in C.GATHER_ROW_CASES:
        c = C.gather_case(B, P, Twin, L, D, shift)
        conv, pe = framed(c["conv"]), framed(c["pe"])
        ref = C.gather_ref(c, B, P, Twin, L, shift)
        M = B * Twin * L
        for with16 in (True, False):
            x32 = guarded(M, D, torch.float32)
            x16 = guarded(M, D, d16)
            e.debug_window_gather(conv, pe, B, P, Twin, L, D, shift, False, x32, x16 if with16 else None)
            launched(e, "window_gather_kernel")
            key = (Twin, L, D, shift, with16)
            assert guards_intact(x32, M, D) and guards_intact(x16, M if with16 else 0, D), key
            assert C.same_bits(x32[:M].cpu(), ref), key
            if with16:
                assert C.same_bits(x16[:M].cpu(), ref.to(d16)), key
    for bad in (dict(D=6), dict(P=0), dict(L=0), dict(Twin=0), dict(B=0), dict(x32=None), dict(conv=conv.view(-1)[1:]), dict(shift=-1)):
        kw = dict(conv=conv, pe=pe, B=B, P=P, Twin=Twin, L=L, D=D, shift=shift, tiled=False, x32=x32, x16=x16)
        kw.update(bad)
        assert rejects(e.debug_window_gather, **kw), bad
    assert e.debug_last_kernel() == ""


@BUILDS
def test_window_gather_tiled_exact(bf):
    e, d16 = eng(bf), dt16(bf)
    for B, Twin, L in C.GATHER_TILED_CASES:
        M = B * Twin * L
        P, shift = max(2, (Twin + L) // 2), 2
        c = C.gather_case(B, P, Twin, L, 512, shift)
        elems = (M + 127) // 128 * 65536 + 128 * 512          # whole 128-row tiles + a guard
        plane = torch.full((elems,), SENT16, dtype=torch.int16, device=DEV)
        e.debug_window_gather(framed(c["conv"]), framed(c["pe"]), B, P, Twin, L, 512, shift, True, None, plane.view(d16))
        launched(e, "window_gather_tiled_kernel")
        ref = C.tiled_plane(C.gather_ref(c, B, P, Twin, L, shift).to(d16), elems, SENT16)          # rows >= M keep the sentinel
        diff = int((plane.cpu() != ref).sum())
        assert diff == 0, (M, diff)
    conv, pe = framed(c["conv"]), framed(c["pe"])
    assert rejects(e.debug_window_gather, conv, pe, B, P, Twin, L, 256, shift, True, None, plane.view(d16))          # D != 512
    assert rejects(e.debug_window_gather, conv, pe, B, P, Twin, L, 512, shift, True, None, None)
    assert rejects(e.debug_window_gather, conv, pe, B, P, Twin, 0, 512, shift, True, None, plane.view(d16))
    assert e.debug_last_kernel() == ""


@BUILDS
def test_cast_exact(bf):
    e, d16 = eng(bf), dt16(bf)
    for n in (4, 1028):
        x = C.cast_values(n)
        out = guarded(1, n + 8, d16)
        e.debug_cast(framed(x), out, n)
        launched(e, "cast_kernel")
        assert guards_intact(out, 1, n)
        got, ref = out[0, :n].cpu(), x.to(d16)
        bad = [(float(x[i]), float(got[i]), float(ref[i])) for i in range(n) if not C.same_bits(got[i:i + 1], ref[i:i + 1])]
        assert not bad, bad[:8]
    assert rejects(e.debug_cast, framed(x), out, 6)            # n % 4: the launcher's rule
    assert rejects(e.debug_cast, framed(x), out, 0)
    assert rejects(e.debug_cast, framed(x)[1:], out, 4)        # 16-byte loads
    assert e.debug_last_kernel() == ""


@BUILDS
def test_zero_tail_exact(bf):
    e, d16 = eng(bf), dt16(bf)
    for H in (1, 5):
        for row_elems in (8, 264):
            for halvings in range(4):
                c = C.zero_tail_case(H, row_elems, halvings, d16)
                B = len(c["valid"])
                buf = guarded(B * H, row_elems, d16)
                buf[:B * H] = c["x"].reshape(B * H, row_elems).to(DEV)
                e.debug_zero_tail(buf, c["valid"], halvings, B, H, row_elems)
                launched(e, "zero_tail_kernel")
                assert guards_intact(buf, B * H, row_elems), (H, row_elems, halvings)
                assert C.same_bits(buf[:B * H].cpu(), c["ref"].reshape(B * H, row_elems)), (H, row_elems, halvings)
    assert rejects(e.debug_zero_tail, buf, c["valid"], 1, B, H, 12)               # row_elems % 8: the launcher's rule
    assert rejects(e.debug_zero_tail, buf, c["valid"][:-1], 1, B, H, 8)           # one entry per clip
    assert rejects(e.debug_zero_tail, buf, None, 1, B, H, 8)
    assert rejects(e.debug_zero_tail, buf, c["valid"], -1, B, H, 8)
    assert e.debug_last_kernel() == ""


def test_mask_transpose_broadcast_exact():
    e = eng()
    for n in (1, 257):
        x = torch.tensor(([0, 1, -1, 2, -2 ** 31] * 52)[:n], dtype=torch.int32)
        out = guarded(1, n + 8, torch.float32)
        e.debug_mask_i32_f32(x.to(DEV), out, n)
        launched(e, "mask_i32_f32_kernel")
        assert guards_intact(out, 1, n) and torch.equal(out[0, :n].cpu(), (x != 0).float())
    assert rejects(e.debug_mask_i32_f32, x.to(DEV), out, 0) and rejects(e.debug_mask_i32_f32, None, out, 4)
    for L in (1, 21, 33):
        for D in (1, 32, 40):
            x = torch.randn(2, L, D)
            out = guarded(2 * D, L, torch.float32)
            e.debug_transpose_tokens(framed(x), 2, L, D, out)
            launched(e, "transpose_tokens_kernel")
            assert guards_intact(out, 2 * D, L) and torch.equal(out[:2 * D].cpu().view(2, D, L), x.transpose(1, 2)), (L, D)
    assert rejects(e.debug_transpose_tokens, framed(x), 65536, L, D, out) and rejects(e.debug_transpose_tokens, framed(x), 2, 0, D, out)
    v = torch.randn(64).half()
    for pixels in (3, 4096 * 256 // 64 + 1):          # one pass; a little above grid x block (the grid-stride branch)
        out = guarded(pixels, 64, torch.float16)
        e.debug_broadcast_channels(framed(v), 64, out, pixels)
        launched(e, "broadcast_channels_kernel")
        assert guards_intact(out, pixels, 64) and C.same_bits(out[:pixels].cpu(), v.expand(pixels, 64))
    assert rejects(e.debug_broadcast_channels, framed(v), 0, out, 3) and rejects(e.debug_broadcast_channels, framed(v), 64, out, 0)
    assert e.debug_last_kernel() == ""
    assert state_error(eng(True).debug_broadcast_channels, framed(v), 64, out, 3)


def test_xlmr_embed_exact():
    e = eng()
    for L in (1, 63, 65, 130):
        ids = C.xlmr_ids(L)
        B = ids.shape[0]
        for D in (4, 768):
            tb = C.xlmr_tables(D)
            out = guarded(B * L, D, torch.float32)
            e.debug_xlmr_embed(ids.to(DEV), B, L, D, C.XL_PAD, C.XL_VOCAB, C.XL_MAXPOS, framed(tb["word"]), framed(tb["pos"]), framed(tb["type"]), out)
            launched(e, "xlmr_embed_kernel")
            assert guards_intact(out, B * L, D), (L, D)
            assert C.same_bits(out[:B * L].cpu(), C.xlmr_ref(ids, tb)), (L, D)
    a = (ids.to(DEV), B, L)
    t = (framed(tb["word"]), framed(tb["pos"]), framed(tb["type"]), out)
    assert rejects(e.debug_xlmr_embed, *a, 6, C.XL_PAD, C.XL_VOCAB, C.XL_MAXPOS, *t)           # D % 4: the launcher's rule
    assert rejects(e.debug_xlmr_embed, *a, 4, C.XL_MAXPOS, C.XL_VOCAB, C.XL_MAXPOS, *t)       # pad_id outside the position table
    assert rejects(e.debug_xlmr_embed, *a, 4, C.XL_PAD, 0, C.XL_MAXPOS, *t)
    assert rejects(e.debug_xlmr_embed, None, B, L, 4, C.XL_PAD, C.XL_VOCAB, C.XL_MAXPOS, *t)
    assert e.debug_last_kernel() == ""


@BUILDS
def test_xlmr_embed_planes(bf):
    e, d16 = eng(bf), dt16(bf)
    fails = []
    for L in (1, 63, 65, 130):
        ids = C.xlmr_ids(L)
        B = ids.shape[0]
        M = B * L
        for D in (256, 768):
            tb = C.xlmr_tables(D)
            hi, lo, part = guarded(M, D, d16), guarded(M, D, d16), guarded(M, D // 64 * 2, torch.float32)
            e.debug_xlmr_embed_planes(ids.to(DEV), B, L, D, C.XL_PAD, C.XL_VOCAB, C.XL_MAXPOS, framed(tb["word"]), framed(tb["pos"]), framed(tb["type"]),
                                      hi, lo, part)
            launched(e, "xlmr_embed_planes_kernel")
            p = C.planes_ref(C.xlmr_ref(ids, tb), d16)
            assert guards_intact(hi, M, D) and guards_intact(lo, M, D) and guards_intact(part, M, D // 64 * 2), (L, D)
            assert C.same_bits(hi[:M].cpu(), p["hi"]) and C.same_bits(lo[:M].cpu(), p["lo"]), (L, D)
            got = part[:M].cpu().view(M, D // 64, 2)
            fails += bounded("xlmr_planes_part", f"L {L} D {D} sum", got[..., 0], p["s1"], p["b1"])
            fails += bounded("xlmr_planes_part", f"L {L} D {D} sum of squares", got[..., 1], p["s2"], p["b2"])
    a = (ids.to(DEV), B, L)
    assert rejects(e.debug_xlmr_embed_planes, *a, 128, C.XL_PAD, C.XL_VOCAB, C.XL_MAXPOS, framed(tb["word"]), framed(tb["pos"]), framed(tb["type"]), hi, lo, part)
    assert rejects(e.debug_xlmr_embed_planes, *a, 256, C.XL_PAD, C.XL_VOCAB, C.XL_MAXPOS, framed(tb["word"]), framed(tb["pos"]), framed(tb["type"]), hi, None, part)
    assert e.debug_last_kernel() == ""
    report("xlmr_planes_part", fails)


RC_SHAPES = [(512, 520, 0), (2048, 2056, 0), (512, 512, 1)]          # (K, lda, tiled)


@pytest.mark.parametrize("K,lda,tiled", RC_SHAPES, ids=["k512", "k2048", "tiled"])
def test_rc_bias_mean_plane_exact(K, lda, tiled):
    e = eng()
    N = 32
    lo = torch.zeros((N, K), dtype=torch.float16, device=DEV)
    for rpc_all, nclips, valid in C.RC_MEAN_CASES:
        c = C.rc_mean_case(rpc_all, nclips, valid, K, lda)
        M = nclips * rpc_all
        if tiled:
            A = C.tiled_plane(c["A"], (M + 127) // 128 * 65536, NAN16).view(torch.float16).to(DEV)          # rows >= M: NaN
        else:
            A = operand(c["A"], lda, torch.float16, extra_rows=0)
        scratch = guarded(nclips, K, torch.float32)
        out = guarded(nclips, N, torch.float32)
        e.debug_rc_bias(A, lda, tiled, nclips, rpc_all, lo, None, N, K, scratch, out, valid=valid)
        launched(e, "rc_col_mean_kernel+rc_gemv_kernel")
        got = scratch.view(-1).view(torch.float16)[:nclips * K].view(nclips, K).cpu()
        wrong = (got.view(torch.int16) != c["mean16"].view(torch.int16)).sum(1).tolist()
        assert not any(wrong), (rpc_all, nclips, valid, wrong)
        assert guards_intact(scratch, nclips, K) and guards_intact(out, nclips, N), (rpc_all, nclips)
        assert bool((scratch.view(torch.int32)[:nclips].view(-1)[nclips * K // 2:] == K64.SENT32).all()), "only the fp16 mean plane is written"
        assert bool((out[:nclips] == 0).all())
    a = dict(A=A, lda=lda, tiled=tiled, nclips=nclips, rpc=rpc_all, lo=lo, bias=None, N=N, K=K, scratch=scratch, out=out, valid=valid)
    for bad in (dict(valid=[1] * (nclips + 1)), dict(N=48), dict(rpc=0), dict(scratch=scratch.view(-1)[:nclips * K - 4]), dict(lo=None)) + (
            () if tiled else (dict(lda=K - 8), dict(lda=lda + 4), dict(nclips=nclips + 1, valid=None))):
        kw = dict(a)
        kw.update(bad)
        assert rejects(e.debug_rc_bias, **kw), bad
    assert e.debug_last_kernel() == ""


# ========================================================================================================================= bounded
@BUILDS
@pytest.mark.parametrize("D", [512, 768])
def test_layernorm(bf, D):
    e, d16 = eng(bf), dt16(bf)
    fails = []
    w = b = None
    for family in C.LN_FAMILIES:
        for rows in C.LN_ROWS:
            c = C.ln_input(family, rows, D)
            w, b = framed(c["w"]), framed(c["b"])
            for flavour in (C.LN_STD, C.LN_ANNOTATED):
                for relu in (0, 1):
                    k = C.ln_case(c, flavour, relu)
                    for d in ["other_flavour"] + (["other_eps"] if family == "small" else []):          # the bounds see the defects
                        assert C.ratio(k[d], k["ref"], k["bound"]) >= 5 and C.ln_nrm(k[d], k) >= 10 * k["nbound"], (d, family, rows)
                    for form in ("out32", "out16", "both", "inplace", "inplace16"):          # in place: out32 == in, alone or with out16
                        x = framed(c["x"])
                        inplace = form.startswith("inplace")
                        o32 = guarded(rows, D, torch.float32) if form in ("out32", "both") else None
                        o16 = guarded(rows, D, d16) if form in ("out16", "both", "inplace16") else None
                        e.debug_layernorm(x, w, b, rows, D, flavour, relu, out32=x if inplace else o32, out16=o16)
                        launched(e, f"layernorm_kernel<{D // 256}>")
                        what = f"{family} rows {rows} D {D} flavour {flavour} relu {relu} {form}"
                        got32 = x.cpu() if inplace else (o32[:rows].cpu() if o32 is not None else None)
                        for buf in (o32, o16):
                            assert buf is None or guards_intact(buf, rows, D), what
                        if got32 is not None:
                            fails += bounded("layernorm_fp32", what, got32, k["ref"], k["bound"])
                            nr = C.ln_nrm(got32, k) / k["nbound"] if bool(got32.isfinite().all()) else float("inf")
                            note("layernorm_norm", nr)
                            if nr > 1:
                                fails.append(f"layernorm {what}: norm-wise observed/bound {nr:.3f}")
                        if o16 is not None:
                            fails += bounded16("layernorm_16bit", what, o16[:rows].cpu(), k["ref"], k["bound"], bf)
    x = framed(c["x"])
    o32 = guarded(rows, D, torch.float32)
    assert rejects(e.debug_layernorm, x, w, b, rows, 256, 0, 0, out32=o32)          # another D: the launcher's rule
    assert rejects(e.debug_layernorm, x, w, b, rows, D, 2, 0, out32=o32)
    assert rejects(e.debug_layernorm, x, w, b, rows, D, 0, 0)
    assert rejects(e.debug_layernorm, x.view(-1)[1:], w, b, 1, D, 0, 0, out32=o32)
    assert rejects(e.debug_layernorm, x, w, b, 0, D, 0, 0, out32=o32)
    assert e.debug_last_kernel() == ""
    for key in ("layernorm_norm", "layernorm_16bit", "layernorm_16bit_ulps_off"):
        print(f"worst observed/bound, {key}: {K64.RATIOS.get(key, 0.0):.3f}")
    report("layernorm_fp32", fails)


def test_a_refused_check_point_does_not_keep_the_previous_name():
    """The name belongs to one call: after a launch that recorded its instance, a call of ANOTHER check point that the check point itself
    refuses (max-pool with C = 4: no launcher is reached) reads "", not the earlier call's name."""
    e = eng()
    c = C.ln_input(C.LN_FAMILIES[0], 4, 512)
    o32 = guarded(4, 512, torch.float32)
    e.debug_layernorm(framed(c["x"]), framed(c["w"]), framed(c["b"]), 4, 512, C.LN_STD, 0, out32=o32)
    launched(e, "layernorm_kernel<2>")
    img = torch.zeros(1, 5, 5, 4, dtype=torch.float16, device=DEV)
    out = guarded(4, 4, torch.float16)
    assert rejects(e.debug_maxpool, img, out)
    assert e.debug_last_kernel() == ""
    torch.cuda.synchronize()
    assert guards_intact(out, 0, 0), "a refused launch wrote to its output"


@BUILDS
def test_layernorm_planes(bf):
    e, d16 = eng(bf), dt16(bf)
    fails = []
    for family in C.LN_FAMILIES:
        for rows in C.LN_ROWS:
            c = C.planes_input(family, rows, d16)
            k = C.ln_case(c, C.LN_STD, 0, x64=c["x64"])
            for d in ["other_flavour"] + (["other_eps"] if family == "small" else []):
                assert C.ratio(k[d], k["ref"], k["bound"]) >= 5 and C.ln_nrm(k[d], k) >= 10 * k["nbound"], (d, family, rows)
            out = guarded(rows, 768, torch.float32)
            e.debug_layernorm_planes(framed(c["hi"]), framed(c["lo"]), framed(c["w"]), framed(c["b"]), rows, 768, out)
            launched(e, "layernorm_planes_kernel<3>")
            assert guards_intact(out, rows, 768)
            got = out[:rows].cpu()
            fails += bounded("layernorm_planes", f"{family} rows {rows}", got, k["ref"], k["bound"])
            nr = C.ln_nrm(got, k) / k["nbound"] if bool(got.isfinite().all()) else float("inf")
            note("layernorm_planes_norm", nr)
            if nr > 1:
                fails.append(f"layernorm_planes {family} rows {rows}: norm-wise observed/bound {nr:.3f}")
    assert rejects(e.debug_layernorm_planes, framed(c["hi"]), framed(c["lo"]), framed(c["w"]), framed(c["b"]), rows, 512, out)
    assert rejects(e.debug_layernorm_planes, framed(c["hi"]), None, framed(c["w"]), framed(c["b"]), rows, 768, out)
    assert e.debug_last_kernel() == ""
    print(f"worst norm-wise observed/bound: {K64.RATIOS.get('layernorm_planes_norm', 0.0):.3f}")
    report("layernorm_planes", fails)


def test_ln_stats():
    e = eng()
    fails = []
    for rows, P, nconst in ((1, 4, 0), (1, 12, 1), (255, 4, 8), (257, 12, 8), (257, 4, 8), (255, 12, 8)):
        c = C.ln_stats_case(rows, P, nconst)
        out = guarded(rows, 2, torch.float32)
        e.debug_ln_stats(framed(c["part"]), rows, P, out)
        launched(e, "ln_stats_kernel")
        assert guards_intact(out, rows, 2)
        got = out[:rows].cpu()
        fails += bounded("ln_stats", f"rows {rows} P {P} mean", got[:, 0], c["mean"], c["bmean"])
        fails += bounded("ln_stats", f"rows {rows} P {P} rstd", got[:, 1], c["rstd"], c["brstd"])
    assert rejects(e.debug_ln_stats, framed(c["part"]), rows, 0, out) and rejects(e.debug_ln_stats, framed(c["part"]), 0, P, out)
    assert e.debug_last_kernel() == ""
    report("ln_stats", fails)


@BUILDS
def test_group_mean(bf):
    e, d16 = eng(bf), dt16(bf)
    fails = []
    for L in (1, 21, 50):
        for D in (8, 512):
            for groups in (1, 33):
                c = C.group_mean_case(groups, L, D, d16)
                out = guarded(groups, D, d16)
                e.debug_group_mean(framed(c["x"]), groups, L, D, out)
                launched(e, "group_mean_kernel")
                assert guards_intact(out, groups, D)
                got = out[:groups].cpu()
                if L == 1:
                    assert C.same_bits(got, c["x"]), (D, groups)
                fails += bounded16("group_mean", f"L {L} D {D} groups {groups}", got, c["ref"], c["bound"], bf)
    x = framed(c["x"])
    assert rejects(e.debug_group_mean, x, groups, L, 12, out)          # D % 8 and L <= 0: the launcher's rules
    assert rejects(e.debug_group_mean, x, groups, 0, D, out)
    assert rejects(e.debug_group_mean, x, 0, L, D, out) and rejects(e.debug_group_mean, x.view(-1)[4:], 1, L, D, out)
    assert e.debug_last_kernel() == ""
    print(f"worst ulps off the rounded reference, group_mean: {K64.RATIOS.get('group_mean_ulps_off', 0.0):.3f}")
    report("group_mean", fails)


def test_col_sum():
    e = eng()
    fails = []
    for K in (8, 520):
        lda = K + 8
        for M in (1, 63, 64, 65, 200):
            for with_stats in (False, True):
                c = C.col_sum_case(M, K, with_stats)
                A = operand(c["A"], lda, torch.float16)
                scratch = guarded(64, K, torch.float32)
                out = guarded(1, K + 8, torch.float32)
                out[0, :K] = c["out0"].to(DEV)
                st = framed(c["stats"]) if with_stats else None
                for _ in range(2):          # out accumulates across calls
                    e.debug_col_sum(A, lda, M, K, scratch, out, stats=st)
                launched(e, "col_sum_kernel+col_sum_finish_kernel")
                assert guards_intact(scratch, 64, K) and guards_intact(out, 1, K), (M, K, with_stats)
                fails += bounded("col_sum", f"M {M} K {K} stats {with_stats}", out[0, :K].cpu(), c["ref"], c["bound"])
    for bad in (dict(K=12, lda=24), dict(lda=K - 8), dict(lda=K + 4), dict(A=A.view(-1)[4:]), dict(scratch=scratch.view(-1)[:64 * K - 1]), dict(M=0)):
        kw = dict(A=A, lda=lda, M=M, K=K, scratch=scratch, out=out)
        kw.update(bad)
        assert rejects(e.debug_col_sum, **kw), bad
    assert e.debug_last_kernel() == ""
    assert state_error(eng(True).debug_col_sum, A, lda, M, K, scratch, out)
    report("col_sum", fails)


def test_rc_bias_out():
    e = eng()
    fails = []
    for rpc_all, nclips, valid, K, N, tiled, bias in C.RC_OUT_CASES:
        c = C.rc_out_case(rpc_all, nclips, valid, K, N, bias)
        M = nclips * rpc_all
        lda = K if tiled else K + 8
        if tiled:
            A = C.tiled_plane(c["A"], (M + 127) // 128 * 65536, NAN16).view(torch.float16).to(DEV)
        else:
            A = operand(c["A"], lda, torch.float16, extra_rows=0)
        scratch = guarded(nclips, K, torch.float32)
        out = guarded(nclips, N, torch.float32)
        e.debug_rc_bias(A, lda, tiled, nclips, rpc_all, operand(c["lo"], K, torch.float16), framed(c["bias"]) if bias else None, N, K, scratch, out,
                        valid=valid)
        launched(e, "rc_col_mean_kernel+rc_gemv_kernel")
        assert guards_intact(scratch, nclips, K) and guards_intact(out, nclips, N)
        fails += bounded("rc_bias_out", f"rpc {rpc_all} clips {nclips} K {K} N {N} tiled {tiled} bias {bias}", out[:nclips].cpu(), c["ref"], c["bound"])
    lo = operand(c["lo"], K, torch.float16)
    assert rejects(e.debug_rc_bias, A, 1024, 0, nclips, 1, lo, None, N, 1024, scratch, out)          # rc_bias_ok: K = 1024
    big = torch.zeros(128 * 2048, dtype=torch.float16, device=DEV)
    assert rejects(e.debug_rc_bias, big, 2048, 1, 1, 16, lo, None, 32, 2048, scratch, out)           # tiled with K = 2048
    assert rejects(e.debug_rc_bias, A, lda, 0, nclips, rpc_all, lo, None, 48, K, scratch, out)       # N = 48
    assert rejects(e.debug_rc_bias, A, lda, 0, nclips, rpc_all + 1, lo, None, N, K, scratch, out)    # more rows than A holds
    assert e.debug_last_kernel() == ""
    assert state_error(eng(True).debug_rc_bias, A, lda, 0, nclips, rpc_all, lo, None, N, K, scratch, out)
    report("rc_bias_out", fails)


def test_pe_project():
    e = eng()
    fails = []
    S = 3
    for N in (1, 5):
        for K in (1, 70, 512):
            for with_lo in (False, True):
                for with_bias in (False, True):
                    c = C.pe_project_case(S, N, K, with_lo, with_bias)
                    out = guarded(1, S * N + 8, torch.float16)
                    e.debug_pe_project(framed(c["pe"]), S, framed(c["wh"]), framed(c["wl"]) if with_lo else None, framed(c["bias"]) if with_bias else None,
                                       N, K, out)
                    launched(e, "pe_project_kernel")
                    assert guards_intact(out, 1, S * N)
                    fails += bounded16("pe_project", f"N {N} K {K} lo {with_lo} bias {with_bias}", out[0, :S * N].cpu().view(S, N), c["ref"], c["bound"],
                                       False)
    assert rejects(e.debug_pe_project, framed(c["pe"]), S, None, None, None, N, K, out) and rejects(e.debug_pe_project, framed(c["pe"]), S, framed(c["wh"]),
                                                                                                  None, None, N, 0, out)
    assert e.debug_last_kernel() == ""
    assert state_error(eng(True).debug_pe_project, framed(c["pe"]), S, framed(c["wh"]), None, None, N, K, out)
    print(f"worst ulps off the rounded reference, pe_project: {K64.RATIOS.get('pe_project_ulps_off', 0.0):.3f}")
    report("pe_project", fails)


@BUILDS
def test_audio_conv0(bf):
    e, d16 = eng(bf), dt16(bf)
    fails = []
    for Tm in C.AUDIO_TM:
        for F_ in C.AUDIO_F:
            for vi, valid in enumerate(C.audio_valids(Tm)):
                c = C.audio_conv0_case(Tm, F_, valid, with_lo=bool((Tm + vi) & 1), d16=d16)
                n = 3 * Tm * F_
                out = guarded(n, 32, d16)
                e.debug_audio_conv0(framed(c["mel_dev"]), 3, Tm, F_, framed(c["wh"]), framed(c["wl"]) if c["wl"] is not None else None, framed(c["bias"]), out,
                                    valid=valid)
                launched(e, "audio_conv0_kernel")
                assert guards_intact(out, n, 32), (Tm, F_, valid)
                got = out[:n].cpu().view(3, Tm, F_, 32)
                for b in range(3):
                    assert bool((got[b, c["Tv"][b]:] == 0).all()), (Tm, F_, valid, "rows beyond valid must be exactly zero")
                fails += bounded16("audio_conv0", f"Tm {Tm} F {F_} valid {valid}", got, c["ref"], c["bound"], bf)
    a = (framed(c["wh"]), None, framed(c["bias"]), out)
    assert rejects(e.debug_audio_conv0, framed(torch.zeros(3, 1, 81)), 3, 1, 81, *a)                  # F = 81: the launcher's rule
    assert rejects(e.debug_audio_conv0, framed(c["mel"]), 3, Tm, F_, *a, valid=[1, 2])                # one entry per clip
    assert rejects(e.debug_audio_conv0, framed(c["mel"]), 3, Tm, F_, framed(c["wh"]), None, None, out)
    assert e.debug_last_kernel() == ""
    print(f"worst ulps off the rounded reference, audio_conv0: {K64.RATIOS.get('audio_conv0_ulps_off', 0.0):.3f}")
    report("audio_conv0", fails)


def test_l2norm():
    e = eng()
    fails = []
    for rows in (1, 5):
        for D in (4, 260, 512):
            c = C.l2norm_case(rows, D)
            for inplace in (False, True):
                buf = guarded(rows, D, torch.float32)
                x = framed(c["x"])
                if inplace:
                    buf[:rows] = x
                e._bind_stream()
                e._ck(e.lib.jg_l2norm(e.h, buf.data_ptr() if inplace else x.data_ptr(), buf.data_ptr(), rows, D))
                torch.cuda.synchronize()
                assert guards_intact(buf, rows, D)
                got = buf[:rows].cpu()
                if rows > 1:
                    assert bool((got[rows // 2] == 0).all()), "the zero row"
                fails += bounded("l2norm", f"rows {rows} D {D} inplace {inplace}", got, c["ref"], c["bound"])
    with pytest.raises(Exception) as ei:
        e._ck(e.lib.jg_l2norm(e.h, x.data_ptr(), buf.data_ptr(), 1, 6))          # D % 4
    assert ei.value.code == -1
    report("l2norm", fails)


@BUILDS
def test_word_pool(bf):
    """launch_segment_mean exists in both builds (jg_word_pool dispatches it); its fp32 destination makes the values the same in both."""
    e = eng(bf)
    fails = []
    for n in (1, 5):
        for D in (1, 100, 768):
            c = C.pool_case(n, D)
            x = framed(c["x"])
            ld, col = D + 24, 8
            dst = guarded(n, ld, torch.float32)
            e.word_pool(x, c["seg"], dst, col)          # dst_ld > D, dst_col > 0
            torch.cuda.synchronize()
            flat = dst.view(torch.int32).cpu()
            assert bool((flat[n:] == K64.SENT32).all()) and bool((flat[:n, :col] == K64.SENT32).all()) and bool((flat[:n, col + D:] == K64.SENT32).all()), (n, D)
            got = dst[:n, col:col + D].cpu().flip(0)          # segment i went to row n - 1 - i
            assert torch.equal(got[0], c["x"][0]), "a segment of length 1 is an exact copy"
            fails += bounded("word_pool", f"n {n} D {D}", got, c["ref"], c["bound"])
    report("word_pool", fails)


def test_pool_mean():
    e = eng()
    fails = []
    for n in (1, 5):
        for D in (1, 100, 768):
            c = C.pool_case(n, D)
            x = framed(c["x"])
            off = torch.tensor(c["off"], dtype=torch.int32, device=DEV)
            out = guarded(n, D, torch.float32)
            e._bind_stream()
            e._ck(e.lib.jg_pool_mean(e.h, x.data_ptr(), off.data_ptr(), n, D, out.data_ptr()))
            torch.cuda.synchronize()
            assert guards_intact(out, n, D)
            got = out[:n].cpu()
            assert torch.equal(got[0], c["x"][0]), "a block of one row is an exact copy"
            fails += bounded("pool_mean", f"n {n} D {D}", got, c["ref"], c["bound"])
    report("pool_mean", fails)
