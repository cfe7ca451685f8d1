"""Kernel-level checks of the GEMM forms the fused transformer launches, against float64 and bit for bit (run with -m gpu).

The GestSync transformer under gs_fused_plan (gestsync.hip) launches gemm_glds_kernel in three forms that no other file launches:
  * the tiled fp16 token plane as A operand (GemmArgs::a_tiled; shared.h, x16t_index): qkv (N = 1536) and linear1 (N = 2048, ReLU), with
    the per-clip bias of the run-time corrected weights or without it;
  * residual + LayerNorm fused with out16 = res16, i.e. in place on the token plane;
  * the implicit-LayerNorm producer (ln_mode 2) with out16 / out_lo = xres_hi / xres_lo (engine::gemm in linear.hip, XLM-R).
Every case is ONE launch through jg_debug_gemm_check (include/jegal_hip.h; its a_tiled member hands A over as the plane), built by the
helpers of tests/test_gpu_kernels_fp64.py: gemm_case(tiled=True), ln_fused_case(inplace=True), implicit_ln_case(inplace=True).  Reference,
bounds and guards are those helpers' (derived, not measured; its docstring has the derivations).  What this file adds to them:
  * the plane A holds whole 128-row tiles plus one guard tile; the rows >= M of the last tile and the guard tile hold NaN bits, so a read
    of a row >= M or behind the plane puts NaN into an output and fails the finite check, inside the allocation;
  * tiled = row-major, bit for bit: the loader puts the same 16-byte chunks at the same LDS addresses whichever way A is laid out, and the
    k order is the instance's own, so where the planner names one instance for both forms the results are equal by construction.  The
    tolerance is zero and derived; any wrong chunk of any k-tile of any row block shows, however small its effect on the norm;
  * in place = out of place, bit for bit, on the same operands: every output element depends on the residual element of its own position
    alone (and LayerNorm on its own row), so equality holds exactly when each workgroup reads what it needs before anything overwrites it.

The defects these cases exist for, and which cases see them:
  1. `(c & 1) * 8` dropped from the loader's chunk offset (every odd 8-column chunk reads its even neighbour).  Stays inside the plane.
  2. a k step of `sk0` instead of `sk0 * (X16T_COLBLK / 64)` (k-tile kt reads 64 kt elements on, inside the first column block, instead of
     column block kt).  Stays inside the plane.
     Both were built into a scratch copy of the library (never committed) and this file was run on each once: SEEDED DEFECTS below.
  3. the row clamp (`m < Mrows ? m : Mrows - 1`) applied after x16t_row_off instead of before.  Not run: it reads rows the caller never
     filled, in production behind the plane.  Argued from the code: x16t_row_off is increasing in m, so a clamp of the offset to
     x16t_row_off(M - 1) is the same address; the variants that differ clamp to a row-major quantity ((M - 1) * lda, which lies in another
     row's quads: rows < M of the last GEMM tile then stay right and only rows >= M move) or do not clamp at all.  A row of A feeds its own
     output row alone and rows >= M are not stored, so neither variant changes a stored value: no check of outputs can see them, here or
     end to end.  What the cases do pin is a clamp that moves a row < M (a clamp to M - 2, or to the last row of the previous 16-row block):
     M = 129, 257, 383, 1029 put the last valid row at positions 0, 0, 14 and 4 of a 16-row block, and both the float64 bound and the bit
     comparison fail on that row.  With M = 383 under the 256-row tiles, rows 384 .. 511 of the last GEMM tile belong to a fourth plane
     tile that a caller does not own; the guard tile is there so that even an unclamped read stays inside the allocation.
  4. `lda` addressing taken on a tiled launch (`a.A + m * lda + c * 8`): not run as a mutant (same reason for M near the plane's end).
     Argued: row m would read plane elements 512 m .., which are 16-row x 16-column quads of other rows; every output is off by O(|ref|),
     and every (a), (b) and (d) case fails the bound and the bit comparison.
  5. in place: a residual (or xres) read that happens after another wave's store of the same rows.  The LayerNorm-fused tile is 128 x 512,
     whole rows, and the ln_mode 2 tiles are 128 .. 256 columns of rows that the other column tiles' workgroups also read -- but only
     their own columns.  A change that moves a store in front of another workgroup's read of the same elements (tile tickets, split K, a
     deeper DMA ring that prefetches the next tile's residual) fails the bit comparison with the out-of-place run on M = 1029 / 1153 / 66 560
     (520 tiles over 4 x num_cu workgroups) and on the (w2, tile) grid of ln_mode 2.

SEEDED DEFECTS (scratch builds, this file alone, one run each on the MI355X).  Under either defect the same three tests fail and the other
nine pass (the in-place and refusal tests do not take the tiled loader):
  test_tiled_a_instances_and_m_tails_vs_fp64_and_row_major, test_production_forms_vs_fp64_and_row_major: every one of the 32 + 4 cases fails
  both checks -- the float64 bound and the bit comparison with the row-major launch (99.9 % of the elements differ; 62 - 66 % under ReLU) --
  and test_tiled_a_inside_a_two_lane_batch fails its bound.  No row-major launch fails.
  defect 1: observed / bound 3.0e3 .. 2.8e5, every value finite (the wrong chunk is a valid row's).
  defect 2: observed / bound 3.9e3 at M = 128 and inf wherever M is no multiple of 128 (k-tiles 1 .. 7 reach the NaN rows >= M of the last
  plane tile through the rows of its first column block); 3.7e5 at M = 4096.

Measured on the MI355X, worst observed / bound per family: tiled_a 0.373, production 0.415, two_lanes 0.375, ln_fused_in_place 0.328,
ln_mode2_in_place 0.402; every bit comparison holds.  The file takes 5 s in all (12 tests, under 4 s of it start-up), no test more than 0.7 s.
"""
import pytest
import torch

import test_gpu_kernels_fp64 as K64
import test_gpu_lane_walk as LW
from elementwise_fp64_cases import tiled_index
from test_gpu_kernels_fp64 import DEV, NAN16, SENT16, SENT32, engine, guarded, planned

pytestmark = pytest.mark.gpu

JG_ERR_ARG, JG_ERR_STATE = -1, -3
WORST = {}                 # family -> worst observed / bound of this file's launches (printed by every test)

# the instances the planner can give a tiled launch (plan_glds in jegal_amd/csrc/gemm_plan.hip: plain, K = 512 <= 1024) -> gemm_tile
TILED_INSTANCES = {
    "gemm_glds_kernel<0,0,2,4,2,0,0,0,0>": 1, "gemm_glds_kernel<1,0,2,4,2,0,0,0,0>": 1,
    "gemm_glds_kernel<0,0,4,4,2,0,0,0,0>": 2, "gemm_glds_kernel<1,0,4,4,2,0,0,0,0>": 2,
    "gemm_glds_kernel<0,0,8,2,4,0,1,0,0>": 3,
}
# 128: the planner's minimum; 129: one row in a second plane tile; 255 / 257: around a 256-row GEMM tile; 383: three plane tiles under a
# 256-row GEMM tile, whose last tile clamps rows that would lie in a plane tile that does not exist; 1029: several tiles and a tail
M_TAILS = (128, 129, 255, 257, 383, 1029)
TILED_CASES = [(f"tiled_t{t}{'_w2' if w2 else ''}_m{M}", M, 256, dict(w2=w2, out="f16", opts=dict(gemm_tile=t)))
               for t in (1, 2, 3) for w2 in ((False, True) if t < 3 else (False,)) for M in M_TAILS]
TILED_CASES += [
    ("tiled_t1_n384", 257, 384, dict(w2=True, out="f16", opts=dict(gemm_tile=1))),                       # N % 256 != 0
    ("tiled_t2_both_resmod", 383, 256, dict(out="both", res=True, res_mod=21, opts=dict(gemm_tile=2))),  # fp32 + fp16 outputs, residual
]
# 1092 = 4 clips x 13 frames x 21 tokens; 273 rows per clip >= GEMM_CLIP_MIN_RPC: clip boundaries inside 16-row blocks and inside tiles
PRODUCTION_CASES = [
    ("qkv", 1092, 1536, dict(out="f16")),
    ("linear1", 1092, 2048, dict(out="f16", relu=1)),
    ("qkv_clip_bias", 1092, 1536, dict(out="f16", bias_clip=(273, 4))),
    ("qkv_clip_bias_clamped", 1092, 1536, dict(out="f16", bias_clip=(273, 3))),          # the last clip's index clamps
]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in K64._ENGINES.values():
        e.close()
    K64._ENGINES.clear()


class family:
    """The helpers' observed / bound notes (K64.RATIOS) of the launches inside the block, kept under this file's own family name."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.saved = dict(K64.RATIOS)
        K64.RATIOS.clear()

    def __exit__(self, *exc):
        if K64.RATIOS:
            WORST[self.name] = max(WORST.get(self.name, 0.0), *K64.RATIOS.values())
        K64.RATIOS.clear()
        K64.RATIOS.update(self.saved)


def report():
    print("worst observed/bound:", {k: round(v, 3) for k, v in WORST.items()})


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def tiled_and_row_major(name, M, N, **kw):
    """One tiled launch and one row-major launch (lda = 512) of the same operands, each against float64; where the planner names the same
    instance for both, their result regions are compared bit for bit.  -> (failures, the tiled launch's instance)"""
    opts = kw.get("opts")
    fails, run = [], {}
    for tiled in (True, False):
        with LW.captured() as calls:
            fails += K64.gemm_case(name if tiled else name + "_row_major", M, N, 512, tiled=tiled, lda=512, **kw)
        run[tiled] = calls[-1]
    assert run[True]["a_tiled"] == 1 and "a_tiled" not in run[False] and run[True]["A"].numel() == (M + 127) // 128 * 65536 + 65536
    inst = {t: planned(c, opts) for t, c in run.items()}
    if inst[True] != inst[False]:          # nothing here is expected to take this branch: the planner does not read a_tiled once it has admitted the launch
        print(f"{name}: the planner names {inst[True]} (tiled) and {inst[False]} (row-major): no bit comparison")
        return fails, inst[True]
    for k in ("out32", "out16"):
        if k in run[True] and not torch.equal(bits(run[True][k][:M, :N]), bits(run[False][k][:M, :N])):
            diff = int((bits(run[True][k][:M, :N]) != bits(run[False][k][:M, :N])).sum())
            fails.append(f"{name}: {k} of the tiled launch differs from the row-major launch in {diff} of {M * N} elements ({inst[True]})")
    return fails, inst[True]


def test_tiled_a_instances_and_m_tails_vs_fp64_and_row_major():
    """(a) + (c): the five instances x the M tails, N = 256 (and one N = 384, one fp32 + fp16 output with a residual)."""
    fails, seen = [], {}
    with family("tiled_a"):
        for name, M, N, kw in TILED_CASES:
            f, inst = tiled_and_row_major(name, M, N, **kw)
            fails += f
            seen.setdefault(inst, set()).add(kw["opts"]["gemm_tile"])
    report()
    assert not fails, "\n".join(fails)
    assert {k: {v} for k, v in TILED_INSTANCES.items()} == seen, seen


def test_production_forms_vs_fp64_and_row_major():
    """(b) + (c): qkv, linear1 and the run-time corrected qkv at M = 1092 under the planner's own choice of tile."""
    fails = []
    with family("production"):
        for name, M, N, kw in PRODUCTION_CASES:
            f, inst = tiled_and_row_major(name, M, N, **kw)
            fails += f
            assert inst in TILED_INSTANCES, inst
    report()
    assert not fails, "\n".join(fails)


def test_tiled_a_inside_a_two_lane_batch():
    """(d): M = 4096, N = 2304, K = 512 on the 128 x 128 tile: 32 x 18 = 576 tiles, more than the CUs.  Walk factors 1 and 4 give the same
    bits, guards included."""
    from jegal_amd._lib import gemm_plan
    M, N, K, tiles = 4096, 2304, 512, (4096 // 128) * (2304 // 128)
    ncu = LW.num_cu()
    assert tiles > ncu
    opts = {f: dict(gemm_tile=1, debug_lanes=1, lane_walk_gemm=f) for f in (1, 4)}
    with family("two_lanes"), LW.captured() as calls:
        fails = K64.gemm_case("tiled_walk1", M, N, K, tiled=True, lda=512, out="both", opts=opts[1])
    report()
    assert not fails, "\n".join(fails)
    kw1 = calls[-1]
    kw4 = dict(kw1, out32=guarded(M, kw1["ldc"], torch.float32), out16=guarded(M, kw1["ldc"], torch.float16))
    e = engine(**opts[4])
    e.debug_gemm_check(**kw4)
    torch.cuda.synchronize()
    assert e.debug_last_kernel() == planned(kw4, opts[4]) == "gemm_glds_kernel<0,0,2,4,2,0,0,0,0>"
    grid = {f: gemm_plan(num_cu=ncu, opts=opts[f], **kw)[1] for f, kw in ((1, kw1), (4, kw4))}
    assert grid[1] == min(tiles, ncu) and grid[4] == min(tiles, 4 * ncu) and grid[4] > ncu, grid
    for k in ("out32", "out16"):
        assert torch.equal(bits(kw1[k]), bits(kw4[k])), f"{k}: factor 4 differs from factor 1"


@pytest.mark.parametrize("M, clip", [(1029, None), (1153, (300, 3))])
def test_ln_fused_in_place(M, clip):
    """(e): out16 = res16.  The float64 bound holds and rows < M equal the out-of-place launch of the same operands bit for bit."""
    with family("ln_fused_in_place"):
        with LW.captured() as sep:
            fails = K64.ln_fused_case(M, clip)
        with LW.captured() as inp:
            fails += K64.ln_fused_case(M, clip, inplace=True)
    report()
    sep, inp = sep[-1], inp[-1]
    assert inp["out16"].data_ptr() == inp["res16"].data_ptr() and sep["out16"].data_ptr() != sep["res16"].data_ptr()
    idx = tiled_index(torch.arange(M)[:, None], torch.arange(512)[None, :]).reshape(-1)
    a, b = bits(inp["out16"]).cpu()[idx], bits(sep["out16"]).cpu()[idx]
    if not torch.equal(a, b):
        fails.append(f"ln_fused M={M} clip={clip}: in place differs from out of place in {int((a != b).sum())} of {M * 512} elements")
    assert not fails, "\n".join(fails)


def test_ln_fused_in_place_four_workgroups_per_cu():
    """(e): the operands of test_gpu_lane_walk.test_ln_fused_clip_bias (M = 66 560: 520 whole tiles), lane_walk_lnf = 4, out16 = res16,
    against that test's factor-1 out-of-place plane (which it checked against float64)."""
    ops = LW.ln_fused_clip_bias_operands()
    kw = LW.ln_fused_clip_bias_kw(ops)
    try:
        first = LW.ln_fused_clip_bias_factor1_bits(kw)
        given = ops["plane16"].view(torch.int16)
        R = LW.LNF_SHAPE[0] // 128
        got = bits(LW.ln_fused_clip_bias_launch(kw, 4, kw["res16"])).cpu()
    finally:          # ~0.5 GB of host operands: not kept for the files that follow
        LW.ln_fused_clip_bias_operands.cache_clear()
        LW.LNF_FACTOR1.clear()
    assert torch.equal(got[R * 65536:], given[R * 65536:]), "the guard tile behind the plane changed"
    assert bool((got[R * 65536:] == NAN16).all())
    diff = int((got[:R * 65536] != first[:R * 65536]).sum())
    assert diff == 0, f"in place at factor 4 differs from out of place at factor 1 in {diff} elements"


@pytest.mark.parametrize("M, N, K, w2, tile", [(257, 512, 512, True, 1), (257, 512, 512, True, 2), (257, 512, 512, False, 1), (257, 512, 512, False, 3),
                                               (1029, 768, 1024, False, 3)])
def test_implicit_ln_producer_in_place(M, N, K, w2, tile):
    """(e): out16 / out_lo = xres_hi / xres_lo.  The float64 bounds on hi, hi + lo and stat_out hold, and all three equal the out-of-place
    launch of the same operands bit for bit."""
    with family("ln_mode2_in_place"):
        with LW.captured() as sep:
            fails = K64.implicit_ln_case(2, M, N, K, w2, tile)
        with LW.captured() as inp:
            fails += K64.implicit_ln_case(2, M, N, K, w2, tile, inplace=True)
    report()
    sep, inp = sep[-1], inp[-1]
    assert inp["out16"].data_ptr() == inp["xres_hi"].data_ptr() and inp["out_lo"].data_ptr() == inp["xres_lo"].data_ptr()
    assert sep["out16"].data_ptr() != sep["xres_hi"].data_ptr() and sep["out_lo"].data_ptr() != sep["xres_lo"].data_ptr()
    for k, cols in (("out16", N), ("out_lo", N), ("stat_out", N // 64 * 2)):
        a, b = bits(inp[k][:M, :cols]), bits(sep[k][:M, :cols])
        if not torch.equal(a, b):
            fails.append(f"ln_mode 2 M={M} N={N} w2={w2} tile={tile}: {k} in place differs from out of place in {int((a != b).sum())} elements")
    assert not fails, "\n".join(fails)


def test_tiled_a_refusals():
    """(f): what the planner does not admit with a_tiled comes back as JG_ERR_ARG, writes nothing and names no kernel; each argument set is
    admitted once a_tiled is taken away, so the refusal is the tiled rule's.  On a bf16 handle the check point itself says JG_ERR_STATE."""
    from jegal_amd._lib import JegalError
    z16 = torch.zeros(2048 * 1024, dtype=torch.float16, device=DEV)          # 32 plane tiles
    z32 = torch.zeros(2048 * 1024, dtype=torch.float32, device=DEV)
    out = torch.full((2048 * 1024,), SENT16, dtype=torch.int16, device=DEV)
    out_b = out.clone()
    stat = torch.full((2048 * 64,), SENT32, dtype=torch.int32, device=DEV)
    good = dict(A=z16, lda=512, Wh=z16, ldw=512, M=256, N=256, K=512, ldc=256, bias=z32, a_tiled=1)
    base = dict(good, out16=out.view(torch.float16))
    named = dict(good, out16=torch.empty(256 * 256, dtype=torch.float16, device=DEV))
    ln2 = dict(ln_mode=2, ln_stats=z32, scale=z32, xres_hi=z16, xres_lo=z16, out_lo=out_b.view(torch.float16), stat_out=stat.view(torch.float32))
    bad = [
        ("K = 448", dict(base, K=448), None),
        ("K = 1024", dict(base, K=1024, lda=1024, ldw=1024), None),
        ("N = 64", dict(base, N=64, ldc=64), None),
        ("N = 200", dict(base, N=200, ldc=200), None),
        ("M = 127", dict(base, M=127), None),
        ("gemm_glds = 0", dict(base), dict(gemm_glds=0)),
        ("ln_mode 1", dict(base, ln_mode=1, ln_stats=z32, scale=z32), None),
        ("ln_mode 2", dict(base, **ln2), None),
        ("ln_w", dict(base, M=1024, N=512, ldc=512, ln_w=z32, ln_b=z32, res16=z16), None),
    ]
    for what, kw, opts in bad:
        e = engine(**(opts or {}))
        e.debug_gemm_check(**(dict(named, a_tiled=0) if opts else named))      # a named launch first (gemm_glds = 0 admits the row-major form only)
        assert e.debug_last_kernel() != "", what
        with pytest.raises(JegalError) as ei:
            e.debug_gemm_check(**kw)
        assert ei.value.code == JG_ERR_ARG, what
        assert e.debug_last_kernel() == "", what
        assert planned(kw, opts) == "rejected", what
        assert planned(dict(kw, a_tiled=0), opts) != "rejected", what
    torch.cuda.synchronize()
    assert bool((out == SENT16).all()) and bool((out_b == SENT16).all()) and bool((stat == SENT32).all())
    eb = engine(prec=4)
    with pytest.raises(JegalError) as ei:
        eb.debug_gemm_check(**base)
    assert ei.value.code == JG_ERR_STATE
    assert eb.debug_last_kernel() == ""
    torch.cuda.synchronize()
    assert bool((out == SENT16).all())
