"""jg_sim_search through the C ABI (run with -m gpu): jg_sim_topk / jg_sim_topk_grouped over a gallery of fp32 or fp16 rows that is cut
into slices, one workgroup per query block and slice, and reduced by a second kernel.  The contract is bit equality: whatever `slices` is,
with and without merge, idx / score hold what the plain entry leaves for the gallery widened to fp32.

Every call goes through `scall`: idx / score are pre-filled with a -7 / NaN pattern (or with the list to merge into) and followed by a
guard of 64 elements that must come back untouched, as tests/test_gpu_sim_topk.py::call does.  The references are the plain entries on
the same device operands (`topk_call`, `gcall`) and, on small-integer operands, whose scores are exact in any order, numpy (`expected`).
The float64 rule is check_fp64_grouped of tests/test_gpu_sim_topk_grouped.py, unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_sim_topk import GUARD, INT32_MAX, JG_ERR_ARG, NAN_BITS, P, bits, call as topk_call, dev
from test_gpu_sim_topk_grouped import check_fp64_grouped, dev_i32, exact_scores, expected, gcall, ints, offsets

pytestmark = pytest.mark.gpu
JG_F32, JG_F16 = 0, 1


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def scall(eng, q, g, off, k, slices=0, gallery_offset=0, merge=0, init=None, n_queries=None, n_gallery=None, n_groups=None, D=None, dtype=None,
          expect=0, qp=None, gp=None, null_off=False, null_idx=False, null_score=False):
    """One jg_sim_search call; q: device fp32 (rows, D), g: device fp32 or fp16 (rows, D), off: host group offsets or None (ungrouped).
    -> (idx (n,k) int32, score (n,k) float32) host arrays; asserts the return code and the guards; on an error or an empty call asserts
    that nothing at all was written."""
    nq = q.shape[0] if n_queries is None else n_queries
    ng = g.shape[0] if n_gallery is None else n_gallery
    ngr = (0 if off is None else len(off) - 1) if n_groups is None else n_groups
    offd = None if off is None else dev_i32(off)
    rows, kraw, k = q.shape[0], k, max(k, 1)
    idx = torch.full((rows * k + GUARD,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((rows * k + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    if init is not None:
        idx[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[0], np.int32).reshape(-1)).cuda()
        sc[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[1], np.float32).reshape(-1).view(np.int32)).cuda()
    before_i, before_s = idx.cpu().numpy(), sc.cpu().numpy()
    eng._bind_stream()
    rc = eng.lib.jg_sim_search(eng.h, P(q) if qp is None else qp, nq, P(g) if gp is None else gp,
                               (JG_F16 if g.dtype == torch.float16 else JG_F32) if dtype is None else dtype, ng, q.shape[1] if D is None else D, kraw,
                               None if null_off or offd is None else P(offd), ngr, gallery_offset, merge, slices,
                               None if null_idx else P(idx), None if null_score else P(sc))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    ri, rs = idx.cpu().numpy(), sc.cpu().numpy()
    assert np.all(ri[rows * k:] == -7) and np.all(rs[rows * k:] == NAN_BITS), "guard overwritten"
    if expect != 0 or nq <= 0:
        assert np.array_equal(ri, before_i) and np.array_equal(rs, before_s), "an output was written"
    if 0 < nq < rows:                                                   # rows the call was not asked for
        assert np.array_equal(ri[nq * k:], before_i[nq * k:]) and np.array_equal(rs[nq * k:], before_s[nq * k:])
    return ri[:rows * k].reshape(rows, k), rs[:rows * k].view(np.float32).reshape(rows, k)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def plain(eng, qd, gd, off, k, **kw):
    """the entry jg_sim_search must reproduce, on the same device operands"""
    return topk_call(eng, qd, gd, k, **kw) if off is None else gcall(eng, qd, gd, off, k, **kw)


def one_row_groups(n):
    return np.arange(n + 1, dtype=np.int64)


SLICES = (0, 1, 2, 3, 7)
SIZES = sorted({1, 63, 64, 65, 1037} | {64 * s + d for s in (2, 3, 7) for d in (-1, 0, 1)})


# ------------------------------------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("nq,D", [(1, 64), (64, 64), (65, 64), (1, 128), (64, 128), (65, 128)])
def test_every_cut_gives_the_bits_of_the_plain_entries(eng, nq, D):
    """entries in -2..2: every score is an integer, exact in any order, and most pairs tie.  Gallery sizes around the tile and around
    64 S rows for the forced S; slices 0 (chosen), 1, 2, 3, 7, one per tile and more than tiles; grouped (random groups of 0..5 rows
    with a few rows in no group at either end) and ungrouped"""
    rng = np.random.default_rng(8100 + nq + D)
    q, g = ints(rng, (nq, D)), ints(rng, (max(SIZES), D))
    qd = dev(q)
    for ng in SIZES:
        gd = dev(g[:ng])
        tiles = -(-ng // 64)
        sizes = rng.integers(0, 6, ng)
        off = offsets(sizes, first=min(2, ng - 1))
        off = off[off <= max(ng - 3, off[0])]
        s = exact_scores(q, g[:ng])
        for k in (1, 10, 64, 65, 128):
            for o, want in ((None, expected(s, one_row_groups(ng), k)), (off, expected(s, off, k))):
                ref = plain(eng, qd, gd, o, k, n_gallery=ng)
                assert same(ref, want), (ng, k, o is None)
                for slices in SLICES + (tiles, tiles + 5):
                    got = scall(eng, qd, gd, o, k, slices=slices, n_gallery=ng)
                    assert same(got, ref), (ng, k, o is None, slices)


# ------------------------------------------------------------------------------------------------ 2. groups against slices
def axis_scores(values, D=64, nq=3):
    """a gallery whose row j scores values[j] for query 0, -values[j] for query 1 and 0 for query 2: small integers on one axis"""
    g = np.zeros((len(values), D), np.float32)
    g[:, 0] = values
    q = np.zeros((nq, D), np.float32)
    q[0, 0], q[1, 0] = 1, -1
    return q, g


def check_groups(eng, q, g, off, ks, slices_list, tag):
    qd, gd = dev(q), dev(g)
    s = exact_scores(q, g)
    out = {}
    for k in ks:
        want = expected(s, off, k)
        assert same(gcall(eng, qd, gd, off, k, n_gallery=g.shape[0]), want), (tag, k)
        for slices in slices_list:
            got = scall(eng, qd, gd, off, k, slices=slices, n_gallery=g.shape[0])
            assert same(got, want), (tag, k, slices)
            out[(k, slices)] = got
    return out


def test_group_shapes_against_slice_boundaries(eng):
    rng = np.random.default_rng(8200)
    n = 448                                                              # 7 tiles: slices = 7 cuts at every multiple of 64
    every = (0, 1, 2, 3, 7)
    q, g = ints(rng, (65, 64)), ints(rng, (n, 64))
    check_groups(eng, q, g, np.asarray([0, n]), (1, 5), every, "one group across all slices")
    check_groups(eng, q, g, offsets(rng.integers(0, 2, 2 * n))[:n + 1].clip(0, n), (1, 10, 128), every, "one-row and empty groups")
    on_cuts = np.asarray([0, 64, 64, 100, 128, 192, 192, 192, 300, 320, 384, 448])
    check_groups(eng, q, g, on_cuts, (1, 4, 64), every, "group boundaries on slice boundaries, empty groups there too")
    check_groups(eng, q, g, np.asarray([70, 120, 130, 200, 380]), (1, 3, 10), every, "whole slices outside every group at both ends")
    check_groups(eng, q, g, np.asarray([5, 60, 64, 128, 440]), (2, 10), every, "rows outside every group at both ends")


def test_a_champion_tie_across_slices_goes_to_the_first_row(eng):
    """group [40, 300) holds its best score twice, at rows 50 (slice 0) and 200 (slice 3 of 7, slice 1 of 2): row 50 is the champion;
    query 1 sees the scores negated, so for it the tie is among the other rows"""
    values = np.full(448, 1.0)
    values[[50, 200]] = 9
    values[[10, 400]] = 7                                               # the neighbours' champions
    q, g = axis_scores(values)
    off = np.asarray([0, 40, 300, 448])
    out = check_groups(eng, q, g, off, (1, 2, 3), (0, 1, 2, 3, 7), "tie")
    for key, (idx, score) in out.items():
        assert idx[0, 0] == 50 and score[0, 0] == 9, key
        assert 200 not in idx[0], key


def test_a_champion_beaten_out_of_its_slice_while_a_weaker_part_survives(eng):
    """Two slices of 64 rows, k = 2.  Groups B = [0, 20), C = [20, 40), A = [40, 90) across the cut, E = [90, 128).  In slice 0 the
    champions are C (30), B (20) and A's row 50 (10): row 50 misses the slice's list of two.  In slice 1 A's weaker part survives with row
    70 (5) next to E (1).  The reduction must return C and B -- and never row 70, which is not its group's champion; with k = 3, row 50
    is in slice 0's list and replaces row 70 wherever the two meet."""
    values = np.zeros(128)
    values[5], values[25], values[50], values[70], values[100] = 20, 30, 10, 5, 1
    values[values == 0] = -3
    q, g = axis_scores(values)
    off = np.asarray([0, 20, 40, 90, 128])
    out = check_groups(eng, q, g, off, (1, 2, 3, 4), (1, 2), "beaten champion")
    assert out[(2, 2)][0][0].tolist() == [25, 5] and out[(3, 2)][0][0].tolist() == [25, 5, 50] and out[(4, 2)][0][0].tolist() == [25, 5, 50, 100]
    assert all(70 not in idx[0] for idx, _ in out.values())
    assert eng.debug_last_kernel() == "sim_topk_kernel<float,64,1>+sim_topk_reduce_kernel<64,1>"


def test_duplicate_rows_nan_rows_and_a_gallery_smaller_than_k(eng):
    rng = np.random.default_rng(8300)
    g = rng.standard_normal((300, 128)).astype(np.float32)
    g[250], g[130] = g[3], g[70]                                         # equal rows in different slices (of 2, 3 and 5)
    q = np.stack([g[3], g[70], rng.standard_normal(128).astype(np.float32)]) * 2.0
    qd, gd = dev(q), dev(g)
    ref = topk_call(eng, qd, gd, 10)
    for slices in (0, 2, 3, 5):
        idx, score = scall(eng, qd, gd, None, 10, slices=slices)
        assert same((idx, score), ref), slices
        assert idx[0, :2].tolist() == [3, 250] and bits(score[0, 0]) == bits(score[0, 1]), slices      # one score, the smaller row first
        assert idx[1, :2].tolist() == [70, 130] and bits(score[1, 0]) == bits(score[1, 1]), slices
    # NaN rows are never candidates; fewer candidates than k leave -1 / -inf; small integers, so numpy knows the answer
    gi = ints(rng, (150, 64))
    gi[[0, 5, 63, 64, 100, 149]] = np.nan
    gi[128:140] = np.nan                                                 # a run that holds all of one group
    qi = ints(rng, (65, 64))
    s = exact_scores(qi, gi)
    off = np.asarray([0, 7, 64, 128, 140, 150])
    for o in (None, off):
        for k in (10, 128):                                              # (5 groups, 4 with a champion; 132 rows that are numbers)
            want = expected(s, one_row_groups(150) if o is None else o, k)
            for slices in (0, 1, 2, 3):
                got = scall(eng, dev(qi), dev(gi), o, k, slices=slices)
                assert same(got, want), (o is None, k, slices)
            assert np.all(np.sum(want[0] >= 0, axis=1) == min(k, 132 if o is None else 4))      # fewer candidates than k leave empty slots


# ------------------------------------------------------------------------------------------------ 3. a 16-bit gallery
def test_fp16_gallery_gives_the_bits_of_the_widened_gallery(eng):
    """fp16 rows with subnormals, +-0, the largest finite value and NaN rows, widened exactly on the way in: JG_F16 on the stored rows and
    JG_F32 on gallery.float() give one result, grouped and not, for every cut; and that result is the plain entry's"""
    rng = np.random.default_rng(8400)
    n, D = 333, 128
    h = rng.standard_normal((n, D)).astype(np.float16)
    h[rng.random((n, D)) < 0.05] = np.float16(6e-8)                      # the smallest subnormal
    h[rng.random((n, D)) < 0.05] = np.float16(-3.1e-5)                   # a subnormal near the normal range
    h[rng.random((n, D)) < 0.05] = np.float16(0.0)
    h[rng.random((n, D)) < 0.05] = np.float16(-0.0)
    h[rng.random((n, D)) < 0.01] = np.float16(65504.0)
    h[rng.random((n, D)) < 0.01] = np.float16(-65504.0)
    h[[4, 64, 200]] = np.float16(np.nan)
    h[10], h[11] = np.float16(0.0), np.float16(-0.0)                     # rows of zeros: every score is +0.0
    q = rng.standard_normal((65, D)).astype(np.float32)
    q[3] = 0.0
    g16 = torch.from_numpy(h).cuda()
    g32 = g16.float()
    assert np.array_equal(g32.cpu().numpy().view(np.uint32), h.astype(np.float32).view(np.uint32))
    qd = dev(q)
    off = offsets(rng.integers(0, 12, 60))
    off = off[off <= n]
    for o in (None, off):
        for k in (10, 128):
            ref = plain(eng, qd, g32, o, k)
            assert not np.isnan(ref[1]).any() and not np.any(np.isin(ref[0], [4, 64, 200]))
            for slices in (0, 1, 2, 6):
                assert same(scall(eng, qd, g32, o, k, slices=slices), ref), (o is None, k, slices, "fp32")
                assert same(scall(eng, qd, g16, o, k, slices=slices), ref), (o is None, k, slices, "fp16")
    assert eng.debug_last_kernel() == "sim_topk_kernel<_Float16,128,1>+sim_topk_reduce_kernel<128,1>"
    scall(eng, qd, g16, None, 10, slices=1)
    assert eng.debug_last_kernel() == "sim_topk_kernel<_Float16,64,0>"


# ------------------------------------------------------------------------------------------------ 4. merge, poison, determinism
@pytest.fixture(scope="module")
def grouped_rows():
    rng = np.random.default_rng(8500)
    sizes = rng.integers(0, 9, 300)
    off = offsets(sizes)
    n = int(off[-1])
    return ints(rng, (70, 64), -3, 4), ints(rng, (n, 64), -3, 4), off


@pytest.mark.parametrize("k", [10, 128])
def test_merged_pieces_with_their_own_cuts_equal_the_single_call(eng, grouped_rows, k):
    """the gallery in four pieces cut at group boundaries, in shuffled orders, each piece with another `slices`; fp16 and fp32 pieces mixed
    (small integers are exact in both); grouped and not"""
    q, g, off = grouped_rows
    n = g.shape[0]
    qd = dev(q)
    rng = np.random.default_rng(8501)
    cuts = [0, 40, 41, 170, 300]                                         # groups per piece: 40, 1, 129, 130
    for grouped in (True, False):
        want = expected(exact_scores(q, g), off if grouped else one_row_groups(n), k)
        for trial in range(3):
            order = rng.permutation(4)
            cur = None
            for step, pc in enumerate(order):
                ga, gb = cuts[pc], cuts[pc + 1]
                r0, r1 = int(off[ga]), int(off[gb])
                piece = dev(g[r0:r1])
                if (trial + pc) % 2:
                    piece = piece.half()
                cur = scall(eng, qd, piece, off[ga:gb + 1] - r0 if grouped else None, k, slices=(0, 1, 2, 5)[(trial + step) % 4], gallery_offset=r0,
                            merge=int(step > 0), init=cur, n_gallery=r1 - r0)
            assert same(cur, want), (grouped, order.tolist())
    # merge = 0 never reads idx / score: a list that would win every comparison changes nothing
    hostile = (np.tile(np.arange(k, dtype=np.int32), (q.shape[0], 1)), np.full((q.shape[0], k), np.inf, np.float32))
    for slices in (1, 4):
        assert same(scall(eng, qd, dev(g), off, k, slices=slices, merge=0, init=hostile), expected(exact_scores(q, g), off, k))
    # no row or no group: the list is kept with merge, -1 / -inf without
    kept = expected(exact_scores(q, g), off, k)
    for kw in (dict(off=off, n_gallery=0), dict(off=off[:1]), dict(off=None, n_gallery=0)):
        o = kw.pop("off")
        for slices in (0, 3):
            assert same(scall(eng, qd, dev(g), o, k, slices=slices, merge=1, init=kept, **kw), kept)
            idx, score = scall(eng, qd, dev(g), o, k, slices=slices, **kw)
            assert np.all(idx == -1) and np.all(np.isneginf(score))


def test_poisoned_workspace_and_a_second_run_give_the_same_bits(eng, grouped_rows):
    q, g, off = grouped_rows
    qd, gd, g16 = dev(q), dev(g), dev(g).half()
    first = {(o is None, k, s): scall(eng, qd, gal, o, k, slices=s) for o in (None, off) for k in (10, 128) for s in (0, 7) for gal in (gd,)}
    eng.set_option("ws_poison", 1)
    try:
        for (ungrouped, k, s), want in first.items():
            assert same(scall(eng, qd, gd, None if ungrouped else off, k, slices=s), want), (ungrouped, k, s, "poisoned")
            assert same(scall(eng, qd, g16, None if ungrouped else off, k, slices=s), want), (ungrouped, k, s, "poisoned fp16")
    finally:
        eng.set_option("ws_poison", 0)
    for (ungrouped, k, s), want in first.items():
        assert same(scall(eng, qd, gd, None if ungrouped else off, k, slices=s), want), (ungrouped, k, s, "second run")


# ------------------------------------------------------------------------------------------------ 5. hostile offsets and arguments
@pytest.mark.parametrize("k", [10, 128])
def test_hostile_offsets_stay_inside_the_buffers(eng, k):
    """offsets that are no partition.  The result is unspecified; the call returns JG_OK, the guards are intact (scall) and every idx is -1 or
    one of the call's rows"""
    rng = np.random.default_rng(8600)
    q, g = dev(rng.standard_normal((65, 64))), dev(rng.standard_normal((300, 64)))
    big, small = 2 ** 31 - 1, -2 ** 31
    for off in ([300, 200, 100, 0], [0, 100, 50, 300], [0, 1000, 2000, 100000], [-50, 10, 5, 400], [0, big, small, big], [small, big],
                [big, small], [5, 5, 5, 5], rng.integers(-400, 700, 200).tolist(), rng.integers(small, big, 64).tolist()):
        for slices in (0, 2, 5):
            for base in (0, INT32_MAX - 300):
                idx, _ = scall(eng, q, g, off, k, slices=slices, gallery_offset=base)
                assert np.all((idx == -1) | ((idx >= base) & (idx - base < 300))), (off[:4], slices, base)


def test_bad_arguments_launch_nothing(eng):
    rng = np.random.default_rng(8700)
    q, g = dev(rng.standard_normal((70, 128))), dev(rng.standard_normal((90, 128)))
    off = [0, 30, 90]
    bad = [dict(qp=ctypes.c_void_p(None)), dict(gp=ctypes.c_void_p(None)), dict(null_idx=True), dict(null_score=True), dict(null_off=True),
           dict(dtype=2), dict(dtype=3), dict(dtype=-1), dict(slices=-1), dict(slices=1025),
           dict(k=0), dict(k=129), dict(k=-1), dict(D=0), dict(D=-64), dict(D=96), dict(n_queries=-1), dict(n_gallery=-1), dict(n_groups=-1),
           dict(gallery_offset=-1), dict(gallery_offset=INT32_MAX - 89), dict(gallery_offset=INT32_MAX),
           dict(qp=ctypes.c_void_p(q.data_ptr() + 4)), dict(gp=ctypes.c_void_p(g.data_ptr() + 8))]
    for kw in bad:
        kw = dict(kw)
        scall(eng, q, g, off, kw.pop("k", 5), expect=JG_ERR_ARG, **kw)
        assert eng.debug_last_kernel() == ""
    scall(eng, q, g, None, 5, n_groups=3, expect=JG_ERR_ARG)                # NULL offsets mean ungrouped: no group count goes with them
    scall(eng, q, g.half(), off, 5, gp=ctypes.c_void_p(g.data_ptr() + 8), expect=JG_ERR_ARG)
    many = torch.zeros((70000, 64), dtype=torch.float32, device="cuda")     # 2 x 70000 x 128 keys are more than the lists may take
    scall(eng, many, g[:, :64].contiguous(), None, 128, slices=2, expect=JG_ERR_ARG)
    scall(eng, q, g, off, 5, gallery_offset=INT32_MAX - 90, slices=2)       # the last offset that fits
    scall(eng, q, g, off, 5, n_queries=0)                                   # JG_OK, nothing launched, nothing written
    scall(eng, q, g, off, 5, slices=1024)                                   # the most slices that may be asked for: one per tile is what runs
    idx, _ = scall(eng, q, g, off, 5, n_queries=3, slices=2)                # fewer queries than rows: the others untouched (scall)
    assert np.all(idx[:3, :2] >= 0) and np.all(idx[:3, 2:] == -1)


def test_last_kernel_names_what_was_launched(eng):
    rng = np.random.default_rng(8800)
    q, g = dev(rng.standard_normal((5, 64))), dev(rng.standard_normal((200, 64)))
    for gal, gt in ((g, "float"), (g.half(), "_Float16")):
        for off, grouped in ((None, 0), ([0, 100, 200], 1)):
            for k, L in ((64, 64), (65, 128)):
                scall(eng, q, gal, off, k, slices=1)
                assert eng.debug_last_kernel() == f"sim_topk_kernel<{gt},{L},{grouped}>"
                scall(eng, q, gal, off, k, slices=3)
                assert eng.debug_last_kernel() == f"sim_topk_kernel<{gt},{L},{grouped}>+sim_topk_reduce_kernel<{L},{grouped}>"
    scall(eng, q, g, None, 5, slices=0)                                     # 4 tiles: too few for two slices of the smallest size
    assert eng.debug_last_kernel() == "sim_topk_kernel<float,64,0>"


# ------------------------------------------------------------------------------------------------ 6. float64
@pytest.mark.parametrize("slices", [0, 5])
def test_against_float64_unit_rows(eng, slices):
    rng = np.random.default_rng(8900)
    D, n = 512, 3000
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = unit(rng.standard_normal((65, D)))
    walk = np.cumsum(rng.standard_normal((n, D)) * 0.05, axis=0) + rng.standard_normal((1, D))     # neighbouring frames nearly equal
    sizes = [150] * 19 + [37, 1, 62, 50]
    off = offsets(sizes)
    assert off[-1] == n
    for name, gal in (("random", unit(rng.standard_normal((n, D)))), ("smooth", unit(walk))):
        gd = dev(gal)
        for k in (10, 128):
            idx, score = scall(eng, dev(q), gd, off, k, slices=slices)
            check_fp64_grouped(f"{name} slices={slices} k={k}", q, gal, off, idx, score, k)
            assert same((idx, score), gcall(eng, dev(q), gd, off, k))
        h = gd.half()                                                       # the 16-bit corpus, judged as stored
        idx, score = scall(eng, dev(q), h, off, 10, slices=slices)
        check_fp64_grouped(f"{name} fp16 slices={slices}", q, h.float().cpu().numpy(), off, idx, score, 10)


# ------------------------------------------------------------------------------------------------ 7. the Python front ends
def test_engine_and_corpus_front_ends(eng):
    from jegal_amd import metrics as M
    rng = np.random.default_rng(9000)
    lens = [150, 150, 37, 1, 150, 62, 90]
    clips = [rng.standard_normal((t, 512)).astype(np.float32) * 3.0 for t in lens]
    q = np.stack([clips[4][100], clips[2][0], rng.standard_normal(512).astype(np.float32)])
    rows = eng.l2norm(torch.from_numpy(np.concatenate(clips, 0)))
    off = offsets(lens)
    qn = eng.l2norm(torch.from_numpy(q))
    want = eng.sim_topk_grouped(qn, rows, off, 5)
    for slices in (0, 1, 4):
        got = eng.sim_search(qn, rows, 5, g_offsets=off, slices=slices)
        assert got[0].dtype == torch.int32 and torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    plain_want = eng.sim_topk(qn, rows, 7)
    got = eng.sim_search(qn, rows.cpu().numpy(), 7, slices=3)                # an array, ungrouped
    assert torch.equal(got[0], plain_want[0]) and torch.equal(got[1].view(torch.int32), plain_want[1].view(torch.int32))
    half = rows.half()
    want16 = eng.sim_topk_grouped(qn, half.float(), off, 5)
    part = eng.sim_search(qn, half[off[3]:], 5, g_offsets=off[3:] - off[3], gallery_offset=int(off[3]))
    both = eng.sim_search(qn, half[:off[3]], 5, g_offsets=off[:4], merge_into=part, slices=2)
    assert both[0] is part[0] and torch.equal(both[0], want16[0]) and torch.equal(both[1].view(torch.int32), want16[1].view(torch.int32))
    none = eng.sim_search(qn, torch.zeros(0, 512, dtype=torch.float16), 4)
    assert bool((none[0] == -1).all()) and bool(torch.isneginf(none[1]).all())
    # Corpus: float32 rows give search()'s triple; float16 rows search()'s on the stored rows; the rows stay on the device
    for segment, max_rows in ((0, None), (40, 300)):
        ref = M.search(q, clips, k=4, segment=segment, engine=eng, max_rows=max_rows)
        c32 = M.Corpus.build(clips, dtype="float32", engine=eng)
        assert all(np.array_equal(a, b) for a, b in zip(c32.search(q, k=4, segment=segment, engine=eng, max_rows=max_rows), ref))
        c16 = M.Corpus.build(clips, engine=eng)
        stored = np.split(c16.rows.astype(np.float32), np.cumsum(lens)[:-1])
        ref16 = M.search(qn.cpu().numpy(), stored, k=4, segment=segment, normalize=False, engine=eng, max_rows=max_rows)
        got16 = c16.search(q, k=4, segment=segment, engine=eng, max_rows=max_rows)
        assert all(np.array_equal(a, b) for a, b in zip(got16, ref16))
        assert (got16[0][0, 0], got16[1][0, 0]) == (4, 100) and (got16[0][1, 0], got16[1][1, 0]) == (2, 0)
    c16.search(q, k=4, engine=eng)
    held = c16._dev[1]
    assert held.dtype == torch.float16 and held.is_cuda
    c16.search(q, k=4, engine=eng)
    assert c16._dev[1] is held
