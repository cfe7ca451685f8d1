"""jg_sim_coupling through the C ABI (run with -m gpu): late interaction between queries of several word rows and groups of gallery rows.
The contract is that a score depends on the rows of its query and its group alone, bit for bit: sim_coupling_cases.coupling_expected
restates it from a dense fp32 s, and every cut into slices, every k, every way of merging pieces and either gallery type must give its bits.

Every call goes through `ccall`: idx / score are pre-filled with a -7 / NaN pattern (or with the list to merge into) and followed by a guard
of 64 elements, `pair` has pair_ld = n_queries + 3 with the same pattern in the pad columns and behind its end; guards and pads must come
back untouched, and on an error or an empty call nothing at all may be written.

Float operands: jg_sim_topk with k = n_gallery returns every s(w, t), bit-identical by its contract, so the dense s comes from the device
and no CPU dot product has to match an MFMA chain.  Against float64, for unit rows, |score - score64| <= (D + W) 2^-24: an element's chain
is within D 2^-24 (sum |w_d g_d| <= 1), a max does not amplify an element's error, the W - 1 adds of partial sums of at most W each err by
at most W 2^-24, which the division by W brings to (W - 1) 2^-24, and the division itself rounds once.  Derived, not measured."""
import ctypes

import numpy as np
import pytest
import torch

import sim_coupling_cases as C
from test_gpu_sim_topk import GUARD, INT32_MAX, JG_ERR_ARG, NAN_BITS, P, bits, call as topk_call, dev
from test_gpu_sim_topk_grouped import dev_i32, exact_scores, ints

pytestmark = pytest.mark.gpu
JG_F32, JG_F16 = 0, 1
PAD = 3


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def ccall(eng, w, w_off, g, g_off, k, slices=0, group_offset=0, merge=0, init=None, want_pair=True, n_queries=None, n_gallery=None, n_groups=None,
          D=None, dtype=None, expect=0, wp=None, gp=None, null_woff=False, null_goff=False, null_idx=False, null_score=False, pair_ld=None):
    """One jg_sim_coupling call; w: device fp32 (rows, D), w_off: host word offsets, g: device fp32 or fp16 (rows, D), g_off: host group
    offsets.  -> (idx (nq, k) int32, score (nq, k) float32, pair (groups, nq) float32 or None) host arrays."""
    woff = np.ascontiguousarray(w_off, np.int32)
    rows = len(woff) - 1
    nq = rows if n_queries is None else n_queries
    ng = g.shape[0] if n_gallery is None else n_gallery
    groups = len(g_off) - 1
    ngr = groups if n_groups is None else n_groups
    goffd = dev_i32(g_off)
    kraw, k = k, max(k, 1)
    ld = rows + PAD
    idx = torch.full((rows * k + GUARD,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((rows * k + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    pair = torch.full((groups * ld + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda") if want_pair else None
    if init is not None:
        idx[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[0], np.int32).reshape(-1)).cuda()
        sc[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[1], np.float32).reshape(-1).view(np.int32)).cuda()
    before_i, before_s = idx.cpu().numpy(), sc.cpu().numpy()
    eng._bind_stream()
    rc = eng.lib.jg_sim_coupling(eng.h, P(w) if wp is None else wp, None if null_woff else woff.ctypes.data_as(ctypes.c_void_p), nq,
                                 P(g) if gp is None else gp, (JG_F16 if g.dtype == torch.float16 else JG_F32) if dtype is None else dtype, ng,
                                 w.shape[1] if D is None else D, kraw, None if null_goff else P(goffd), ngr, group_offset, merge, slices,
                                 None if null_idx else P(idx), None if null_score else P(sc), P(pair), ld if pair_ld is None else pair_ld)
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    ri, rs = idx.cpu().numpy(), sc.cpu().numpy()
    assert np.all(ri[rows * k:] == -7) and np.all(rs[rows * k:] == NAN_BITS), "guard overwritten"
    rp = None
    if want_pair:
        rp = pair.cpu().numpy()
        assert np.all(rp[groups * ld:] == NAN_BITS), "pair guard overwritten"
        rp = rp[:groups * ld].reshape(groups, ld)
        assert np.all(rp[:, rows:] == NAN_BITS), "pair pad columns overwritten"
        if expect != 0 or nq <= 0:
            assert np.all(rp == NAN_BITS), "pair was written"
        assert np.all(rp[max(ngr, 0):] == NAN_BITS) and np.all(rp[:, max(nq, 0):] == NAN_BITS), "pair written outside the call's groups and queries"
        rp = np.ascontiguousarray(rp[:, :rows]).view(np.float32)
    if expect != 0 or nq <= 0:
        assert np.array_equal(ri, before_i) and np.array_equal(rs, before_s), "an output was written"
    if 0 < nq < rows:                                                   # queries the call was not asked for
        assert np.array_equal(ri[nq * k:], before_i[nq * k:]) and np.array_equal(rs[nq * k:], before_s[nq * k:])
    return ri[:rows * k].reshape(rows, k), rs[:rows * k].view(np.float32).reshape(rows, k), rp


def same_pair(a, b):
    """NaN in the same places, the bits of every score equal"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def same(a, b):
    """idx and the bits of score equal, and pair where both have one"""
    if not (np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))):
        return False
    return a[2] is None or b[2] is None or same_pair(a[2], b[2])


def f32(s):
    with np.errstate(invalid="ignore"):
        return np.asarray(s).astype(np.float32)


# W from {1, 2, 7, 17, 63, 64}: 63 + 1 fills the first tile exactly, 64 is a tile of its own, 17 + 7 + 2 + 1 + 17 + 17 = 61 leaves no room
# for the next 7 (it moves), and the last 2 does not fit behind 63
W_COUNTS = [63, 1, 64, 17, 7, 2, 1, 17, 17, 7, 2, 1, 64, 63, 2]
SIZES = sorted({1, 63, 64, 65, 129, 1037} | {64 * s + d for s in (2, 3, 7) for d in (-1, 1)})


def random_groups(rng, ng):
    """groups of 0..5 rows with a few rows in no group at both ends, empty groups also at the end"""
    sizes = rng.integers(0, 6, ng)
    off = C.offsets_of_counts(sizes, first=min(2, ng - 1))
    off = off[off <= max(ng - 3, off[0])]
    return np.concatenate([off, [off[-1]] * 2])


# ------------------------------------------------------------------------------------------------ 1. every cut, exact operands
@pytest.mark.parametrize("D", [64, 128])
def test_every_cut_gives_the_bits_of_the_restatement(eng, D):
    """entries in -2..2: every product, max and sum is an integer, exact in any order, so only the one division rounds"""
    rng = np.random.default_rng(9600 + D)
    w_off = C.offsets_of_counts(W_COUNTS)
    assert C.plan_expected(w_off) == [0, 2, 3, 9, 12, 13, 14, 15]
    w, g = ints(rng, (int(w_off[-1]), D)), ints(rng, (max(SIZES), D))
    wd = dev(w)
    for ng in SIZES:
        gd = dev(g[:ng])
        tiles = -(-ng // 64)
        g_off = random_groups(rng, ng)
        s = f32(exact_scores(w, g[:ng]))
        for k in (1, 10, 64, 65, 128):
            want = C.coupling_expected(s, w_off, g_off, k)
            if k == 10 and ng > 1:
                scorable = ~np.isnan(want[2])
                assert scorable.any() and (np.diff(g_off) > 0)[scorable.any(axis=1)].all() and np.isnan(want[2][np.diff(g_off) == 0]).all()
            for slices in (0, 1, 2, 3, 7, tiles, tiles + 5):
                got = ccall(eng, wd, w_off, gd, g_off, k, slices=slices, n_gallery=ng)
                assert same(got, want), (ng, k, slices)


# ------------------------------------------------------------------------------------------------ 2. a group across tiles and slices
def test_a_group_across_tiles_and_slices(eng):
    """groups of 1, 200 and 70 rows, one slice per tile: the group of 200 begins in slice 0, whose workgroup walks on through tiles 1 .. 3;
    the three words of query 0 have their best frames in rows 31 (tile 0), 100 (tile 1) and 199 (tile 3) of that group, word 2's second
    best in tile 2"""
    D = 64
    g = np.zeros((271, D), np.float32)
    g[:, 0] = g[:, 1] = g[:, 2] = -1
    g[31, 0], g[100, 1], g[199, 2], g[150, 2] = 9, 7, 5, 4
    g[0, :3] = 3                                                             # the group of one row
    g[205, 0], g[260, 1], g[270, 2] = 8, 8, 1                                # the group of 70
    w = np.zeros((5, D), np.float32)
    w[0, 0] = w[1, 1] = w[2, 2] = 1                                          # query 0: three axis words
    w[3, 2] = 1                                                              # query 1: the third word alone
    w[4, 0] = -1                                                             # query 2: prefers every other frame
    w_off, g_off = [0, 3, 4, 5], [0, 1, 201, 271]
    s = f32(exact_scores(w, g))
    for k in (1, 3):
        want = C.coupling_expected(s, w_off, g_off, k)
        assert want[0][0, 0] == 1 and want[1][0, 0] == np.float32(21) / np.float32(3) and want[1][1, 0] == 5 and want[0][1, 0] == 1
        for slices in (1, 2, 5, 0):
            got = ccall(eng, dev(w), w_off, dev(g), g_off, k, slices=slices)
            assert same(got, want), (k, slices)
    ccall(eng, dev(w), w_off, dev(g), g_off, 3, slices=5)
    assert eng.debug_last_kernel() == "sim_coupling_kernel<float,64>+sim_topk_reduce_kernel<64,0>"
    # the same rows shifted so that the long group begins on a tile boundary, and behind one
    for shift in (63, 64):
        g2 = np.concatenate([np.full((shift, D), -2, np.float32), g])
        off2 = [0, shift] + [o + shift for o in g_off[1:]]
        want = C.coupling_expected(f32(exact_scores(w, g2)), w_off, off2, 3)
        for slices in (1, 3, 6):
            assert same(ccall(eng, dev(w), w_off, dev(g2), off2, 3, slices=slices), want), (shift, slices)


# ------------------------------------------------------------------------------------------------ 3. float operands
def dense_from_topk(eng, wd, gd, n_gallery):
    """every s(w, t) with the device's bits: jg_sim_topk with k = n_gallery returns all of them"""
    idx, sc = topk_call(eng, wd, gd, n_gallery, n_gallery=n_gallery)
    s = np.full((wd.shape[0], n_gallery), np.nan, np.float32)
    np.put_along_axis(s, idx.astype(np.int64), sc, axis=1)
    assert not np.isnan(s).any()
    return s


@pytest.mark.parametrize("D,ng", [(64, 128), (512, 128), (512, 97)])
def test_float_operands_bit_for_bit_and_against_float64(eng, D, ng):
    rng = np.random.default_rng(9700 + D + ng)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    counts = [1, 2, 7, 17, 9, 3, 17, 8, 64, 5]
    w_off = C.offsets_of_counts(counts)
    w, g = unit(rng.standard_normal((int(w_off[-1]), D))), unit(rng.standard_normal((ng, D)))
    g[1::7] = g[0]                                                           # equal frames: exact ties between one-row groups
    g_off = C.offsets_of_counts([1, 1, 5, 0, 30, 1, 1, 1, 20, 17, 1, 13][:12])
    g_off = g_off[g_off <= ng]
    wd, gd = dev(w), dev(g)
    s = dense_from_topk(eng, wd, gd, ng)
    s64 = C.brute_force_scores(w, g, w_off, g_off)
    scorable = int(np.sum(np.diff(g_off) > 0))
    worst = worst_c = 0.0
    for k in (3, 10):
        want = C.coupling_expected(s, w_off, g_off, k)
        for slices in (0, 1, 2):
            got = ccall(eng, wd, w_off, gd, g_off, k, slices=slices)
            assert same(got, want), (k, slices)
        idx, score, pair = got
        for q, W in enumerate(counts):
            b = (D + W) * 2.0 ** -24
            n = min(k, scorable)
            assert np.all(idx[q, :n] >= 0) and np.all(idx[q, n:] == -1)
            kept = idx[q, :n]
            worst = max(worst, float(np.abs(score[q, :n].astype(np.float64) - s64[q, kept]).max() / b))
            worst = max(worst, float(np.nanmax(np.abs(pair[:, q].astype(np.float64) - s64[q])) / b))
            left = np.ones(len(g_off) - 1, bool)
            left[kept] = False
            left &= ~np.isnan(s64[q])
            if left.any():                                                   # a group left out beats no kept one by more than both bounds
                worst_c = max(worst_c, float((s64[q, left].max() - s64[q, kept].min()) / (2 * b)))
    print(f"D={D} ng={ng}: worst |score - score64| / ((D + W) 2^-24) = {worst:.4f}; worst (left out - weakest kept) / (2 bound) = {worst_c:.4f}")
    assert worst <= 1.0 and worst_c <= 1.0


# ------------------------------------------------------------------------------------------------ 4. a 16-bit gallery
@pytest.mark.parametrize("ng", [129, 1037])
def test_fp16_gallery_gives_the_bits_of_the_widened_gallery(eng, ng):
    rng = np.random.default_rng(9800 + ng)
    w_off = C.offsets_of_counts(W_COUNTS)
    w = ints(rng, (int(w_off[-1]), 128))
    h = rng.standard_normal((ng, 128)).astype(np.float16)
    h[rng.random((ng, 128)) < 0.05] = np.float16(6e-8)                       # the smallest subnormal
    h[rng.random((ng, 128)) < 0.05] = np.float16(-0.0)
    h[rng.random((ng, 128)) < 0.01] = np.float16(65504.0)
    g16 = torch.from_numpy(h).cuda()
    g32 = g16.float()
    g_off = random_groups(rng, ng)
    wd = dev(w)
    for k in (10, 128):
        ref = ccall(eng, wd, w_off, g32, g_off, k, slices=1)
        assert not np.isnan(ref[1]).any() and np.all(ref[0][:, 0] >= 0)
        for slices in (0, 1, 3):
            assert same(ccall(eng, wd, w_off, g16, g_off, k, slices=slices), ref), (k, slices)
            assert same(ccall(eng, wd, w_off, g32, g_off, k, slices=slices), ref), (k, slices, "fp32")
    assert eng.debug_last_kernel() == "sim_coupling_kernel<float,128>+sim_topk_reduce_kernel<128,0>"


# ------------------------------------------------------------------------------------------------ 5. merge
@pytest.mark.parametrize("k", [10, 128])
def test_merged_pieces_equal_the_single_call(eng, k):
    rng = np.random.default_rng(9900)
    w_off = C.offsets_of_counts(W_COUNTS)
    sizes = rng.integers(0, 9, 150)
    g_off = C.offsets_of_counts(sizes)
    n = int(g_off[-1])
    w, g = ints(rng, (int(w_off[-1]), 64)), ints(rng, (n, 64))
    wd = dev(w)
    s = f32(exact_scores(w, g))
    want = C.coupling_expected(s, w_off, g_off, k)
    assert same(ccall(eng, wd, w_off, dev(g), g_off, k), want)
    cuts = [0, 40, 41, 150]                                                  # groups per piece: 40, 1, 109
    for order in ((0, 1, 2), (2, 0, 1)):
        cur = None
        for step, pc in enumerate(order):
            ga, gb = cuts[pc], cuts[pc + 1]
            r0, r1 = int(g_off[ga]), int(g_off[gb])
            piece = dev(g[r0:r1])
            if pc == 1:
                piece = piece.half()                                         # (small integers are exact in both types)
            got = ccall(eng, wd, w_off, piece, g_off[ga:gb + 1] - r0, k, slices=(0, 2, 5)[step], group_offset=ga, merge=int(step > 0),
                        init=cur, n_gallery=r1 - r0)
            assert same_pair(got[2], want[2][ga:gb]), (order, pc)          # pair: this call's local groups
            cur = got[:2]
        assert same(cur + (None,), want), order
    # a seeded list with empty slots: one scorable group first, the rest merged in; and merge = 0 never reads idx / score
    g1 = int(np.argmax(np.diff(g_off) > 0)) + 1                             # the groups up to the first one with a row
    few = ccall(eng, wd, w_off, dev(g[:int(g_off[g1])]), g_off[:g1 + 1], k)
    assert np.all(few[0][:, 0] == g1 - 1) and np.all(few[0][:, 1:] == -1)
    rest = ccall(eng, wd, w_off, dev(g[int(g_off[g1]):]), g_off[g1:] - g_off[g1], k, slices=3, group_offset=g1, merge=1, init=few[:2])
    assert same(rest[:2] + (None,), want)
    hostile = (np.tile(np.arange(k, dtype=np.int32), (len(W_COUNTS), 1)), np.full((len(W_COUNTS), k), np.inf, np.float32))
    for slices in (1, 4):
        assert same(ccall(eng, wd, w_off, dev(g), g_off, k, slices=slices, merge=0, init=hostile), want)
    base = INT32_MAX - 150                                                   # the last group_offset that fits
    got = ccall(eng, wd, w_off, dev(g), g_off, k, slices=2, group_offset=base)
    assert same(got, C.coupling_expected(s, w_off, g_off, k, group_offset=base))


# ------------------------------------------------------------------------------------------------ 6. special values
def test_nan_negative_zero_ties_and_too_few_groups(eng):
    rng = np.random.default_rng(10000)
    D = 64
    w_off = [0, 2, 5, 6, 8]
    w = ints(rng, (8, D))
    w[5] = np.nan                                                            # query 2 is one NaN word: it has no score anywhere
    g = ints(rng, (150, D))
    g[[0, 5, 63, 64, 100, 149]] = np.nan                                     # NaN frames are skipped
    g[128:140] = np.nan                                                      # ... and a group of nothing else has no score
    g[20:30] = 0
    g[20:30:2] = -0.0                                                        # a group whose every product is +-0.0
    g[40:47] = g[70:77]                                                      # two groups of equal rows: equal scores
    g_off = np.asarray([0, 7, 20, 30, 40, 47, 64, 70, 77, 128, 140, 150])
    s = f32(exact_scores(w, g))
    for k in (4, 20):
        want = C.coupling_expected(s, w_off, g_off, k)
        for slices in (0, 1, 3):
            got = ccall(eng, dev(w), w_off, dev(g), g_off, k, slices=slices)
            assert same(got, want), (k, slices)
        idx, score, pair = got
        assert np.all(idx[2] == -1) and np.all(np.isneginf(score[2])) and np.isnan(pair[:, 2]).all()
        assert np.isnan(pair[9]).all() and not np.any(idx == 9)              # the group of NaN rows
        assert not np.isnan(pair[[0, 5, 8, 10]][:, [0, 1, 3]]).any() and not np.isnan(score).any()
        assert np.all(pair[2][[0, 1, 3]] == 0) and not np.signbit(pair[2][[0, 1, 3]]).any()       # -0.0 counts as +0.0
        for q in (0, 1, 3):
            assert bits(pair[4, q]) == bits(pair[7, q])
            at = idx[q].tolist()
            if 4 in at and 7 in at:
                assert at.index(4) < at.index(7)                             # equal scores: the smaller group first
        if k == 20:                                                          # 10 scorable groups: the rest of the list is empty
            assert np.all(np.sum(idx >= 0, axis=1) == [10, 10, 0, 10]) and np.all(np.isneginf(score[idx < 0]))
    # 0.0 against -0.0 as the only difference between two groups: a tie, the smaller group first, and +0.0 comes back
    z = np.zeros((4, D), np.float32)
    z[1, 0], z[2, 0], z[3, 0] = -0.0, 0.0, -1.0
    one = np.zeros((1, D), np.float32)
    one[0, 0] = 1
    idx, score, pair = ccall(eng, dev(one), [0, 1], dev(z), [0, 1, 2, 3, 4], 4)
    assert idx.tolist() == [[0, 1, 2, 3]] and bits(score)[0].tolist() == [0, 0, 0, bits(np.float32(-1.0))] and bits(pair)[:3, 0].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ 7. refusals and empty calls
def test_bad_arguments_launch_nothing(eng):
    rng = np.random.default_rng(10100)
    w, g = dev(rng.standard_normal((70, 128))), dev(rng.standard_normal((90, 128)))
    w_off, g_off = [0, 3, 20, 70], [0, 30, 90]
    bad = [dict(wp=ctypes.c_void_p(None)), dict(gp=ctypes.c_void_p(None)), dict(null_idx=True), dict(null_score=True), dict(null_goff=True),
           dict(null_woff=True), dict(dtype=2), dict(dtype=-1), dict(slices=-1), dict(slices=1025), dict(k=0), dict(k=129), dict(k=-1),
           dict(D=0), dict(D=-64), dict(D=96), dict(n_queries=-1), dict(n_gallery=-1), dict(n_groups=-1), dict(group_offset=-1),
           dict(group_offset=INT32_MAX - 1), dict(group_offset=INT32_MAX), dict(pair_ld=2), dict(pair_ld=-1),
           dict(wp=ctypes.c_void_p(w.data_ptr() + 4)), dict(gp=ctypes.c_void_p(g.data_ptr() + 8)),
           dict(w_off=[0, 3, 3, 70]), dict(w_off=[0, 3, 68, 70]), dict(w_off=[0, 20, 10, 70]), dict(w_off=[1, 3, 20, 70])]
    for kw in bad:
        kw = dict(kw)
        ccall(eng, w, kw.pop("w_off", w_off), g, g_off, kw.pop("k", 5), expect=JG_ERR_ARG, **kw)
        assert eng.debug_last_kernel() == ""
    ccall(eng, w, w_off, g.half(), g_off, 5, gp=ctypes.c_void_p(g.data_ptr() + 8), expect=JG_ERR_ARG)
    many = torch.zeros((70000, 64), dtype=torch.float32, device="cuda")      # 2 x 70000 x 128 keys are more than the lists may take
    ccall(eng, many, np.arange(70001), g[:, :64].contiguous(), g_off, 128, slices=2, want_pair=False, expect=JG_ERR_ARG)
    ccall(eng, w, w_off, g, g_off, 5, n_queries=0)                           # JG_OK, nothing launched, nothing written
    ccall(eng, w, w_off, g, g_off, 5, group_offset=INT32_MAX - 2, slices=2)  # the last offset that fits
    ccall(eng, w, w_off, g, g_off, 5, slices=1024)                           # the most slices that may be asked for: one per tile is what runs
    idx, _, pair = ccall(eng, w, w_off, g, g_off, 5, n_queries=2, slices=2)  # fewer queries than offsets: the others untouched (ccall)
    assert np.all(idx[:2, :2] >= 0) and np.all(idx[:2, 2:] == -1) and not np.isnan(pair[:, :2]).any()
    # no group or no gallery row: the lists are filled, or with merge kept; pair holds no score
    kept = ccall(eng, w, w_off, g, g_off, 5)[:2]
    for kw in (dict(n_gallery=0), dict(n_groups=0)):
        for slices in (0, 3):
            got = ccall(eng, w, w_off, g, g_off, 5, slices=slices, merge=1, init=kept, **kw)
            assert same(got[:2] + (None,), kept + (None,)) and np.isnan(got[2]).all()
            idx, score, pair = ccall(eng, w, w_off, g, g_off, 5, slices=slices, **kw)
            assert np.all(idx == -1) and np.all(np.isneginf(score)) and np.isnan(pair).all()


# ------------------------------------------------------------------------------------------------ 8. what was launched
def test_last_kernel_names_what_was_launched(eng):
    rng = np.random.default_rng(10200)
    w, g = dev(rng.standard_normal((5, 64))), dev(rng.standard_normal((200, 64)))
    for gal, gt in ((g, "float"), (g.half(), "_Float16")):
        for k, L in ((64, 64), (65, 128)):
            for want_pair in (False, True):                                  # (the NaN fill of pair is a launch of the entry's, not named)
                ccall(eng, w, [0, 2, 5], gal, [0, 100, 200], k, slices=1, want_pair=want_pair)
                assert eng.debug_last_kernel() == f"sim_coupling_kernel<{gt},{L}>"
                ccall(eng, w, [0, 2, 5], gal, [0, 100, 200], k, slices=3, want_pair=want_pair)
                assert eng.debug_last_kernel() == f"sim_coupling_kernel<{gt},{L}>+sim_topk_reduce_kernel<{L},0>"
    ccall(eng, w, [0, 2, 5], g, [0, 100, 200], 5, slices=0)                  # 4 tiles: too few for two slices of the smallest size
    assert eng.debug_last_kernel() == "sim_coupling_kernel<float,64>"


def test_poisoned_workspace_and_a_second_run_give_the_same_bits(eng):
    rng = np.random.default_rng(10300)
    w_off = C.offsets_of_counts(W_COUNTS)
    g_off = C.offsets_of_counts(rng.integers(0, 9, 120))
    w, g = dev(ints(rng, (int(w_off[-1]), 64))), dev(ints(rng, (int(g_off[-1]), 64)))
    first = {(k, s): ccall(eng, w, w_off, g, g_off, k, slices=s) for k in (10, 128) for s in (0, 7)}
    eng.set_option("ws_poison", 1)
    try:
        for (k, s), want in first.items():
            assert same(ccall(eng, w, w_off, g, g_off, k, slices=s), want), (k, s, "poisoned")
    finally:
        eng.set_option("ws_poison", 0)
    for (k, s), want in first.items():
        assert same(ccall(eng, w, w_off, g.half(), g_off, k, slices=s), want), (k, s, "second run, fp16")


# ------------------------------------------------------------------------------------------------ 9. the Python front ends
def test_python_front_ends_on_the_device(eng):
    from jegal_amd import metrics as M
    rng = np.random.default_rng(10400)
    lens, words = [5, 40, 17, 9, 33, 21], [1, 9, 4, 4, 2, 7]
    clips = [ints(rng, (t, 64)) for t in lens]
    contents = [ints(rng, (n, 64)) for n in words]
    contents[3] = contents[2].copy()                                         # a planted tie: two utterances with the same words
    w_off, g_off = M.offsets_of(contents), M.offsets_of(clips)
    want = C.coupling_scores(f32(exact_scores(np.concatenate(contents), np.concatenate(clips))), w_off, g_off)
    m = M.coupling_matrix(contents, clips, normalize=False, engine=eng)
    assert m.is_cuda and tuple(m.shape) == (6, 6) and np.array_equal(bits(m.cpu().numpy()), bits(want)) and np.array_equal(want[2], want[3])
    # (integer rows are not unit rows: the metrics are checked on the normalised ones the function works with)
    res = M.coupling_retrieval_metrics(contents, clips, engine=eng)
    mn = M.coupling_matrix(contents, clips, engine=eng).cpu().numpy()
    assert np.array_equal(bits(mn[2]), bits(mn[3]))
    d = np.diag(mn)
    for key, s in (("c2g", mn), ("g2c", mn.T)):
        assert res[key] == M.metrics_from_ranks((s > d[:, None]).sum(1), (s == d[:, None]).sum(1)), key
    assert (mn[:, 2] == mn[2, 2]).sum() >= 2                                 # the tie is there to be counted in g2c
    # Engine.sim_coupling: the list next to the matrix, and merge_into in place
    idx, score, mat = eng.sim_coupling(torch.from_numpy(np.concatenate(contents)), w_off, torch.from_numpy(np.concatenate(clips)), g_off, 4,
                                       want_matrix=True)
    e_idx, e_score, _ = C.coupling_expected(f32(exact_scores(np.concatenate(contents), np.concatenate(clips))), w_off, g_off, 4)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), e_idx) and np.array_equal(bits(score.cpu().numpy()), bits(e_score))
    assert tuple(mat.shape) == (6, 6) and not mat.is_contiguous() and np.array_equal(bits(mat.cpu().numpy()), bits(want))
    # search_phrases: pieces under max_rows equal one piece, segments decode to (clip, start)
    one = M.search_phrases(contents, clips, k=5, segment=8, normalize=False, engine=eng)
    cut = M.search_phrases(contents, clips, k=5, segment=8, normalize=False, engine=eng, max_rows=48)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(one, cut))
    goff8, gclip, gstart = M.search_groups(lens, 8)
    e8 = C.coupling_expected(f32(exact_scores(np.concatenate(contents), np.concatenate(clips))), w_off, goff8, 5)
    assert np.array_equal(one[0], gclip[e8[0]]) and np.array_equal(one[1], gstart[e8[0]]) and np.array_equal(bits(one[2]), bits(e8[1]))
    # Corpus.search_phrases over float16 rows: search_phrases on the widened stored rows
    fl = [rng.standard_normal((t, 64)).astype(np.float32) for t in lens]
    ph = [rng.standard_normal((n, 64)).astype(np.float32) for n in words]
    c16 = M.Corpus.build(fl, engine=eng)
    stored = np.split(c16.rows.astype(np.float32), np.cumsum(lens)[:-1])
    pn = [eng.l2norm(torch.from_numpy(p)).cpu().numpy() for p in ph]
    for segment, max_rows in ((0, None), (8, 48)):
        got = c16.search_phrases(ph, k=4, segment=segment, engine=eng, max_rows=max_rows)
        ref = M.search_phrases(pn, stored, k=4, segment=segment, normalize=False, engine=eng, max_rows=max_rows)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)) and np.all(got[0] >= 0)
    assert c16._dev[1].dtype == torch.float16 and c16._dev[1].is_cuda
