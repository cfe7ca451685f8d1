"""jg_sim_ordered and jg_sim_align through the C ABI (run with -m gpu): phrases matched in word order.  The contract is that a score depends
on the rows of its query and its group alone, bit for bit: sim_ordered_cases.ordered_expected restates it from a dense fp32 s, and every cut
into slices, every k, every way of merging pieces and either gallery type must give its bits; sim_ordered_cases.align_expected restates the
frames.

Every jg_sim_ordered call goes through `ocall`, test_gpu_sim_coupling.ccall with the other entry: idx / score pre-filled with -7 / NaN (or
the list to merge into) and followed by a guard, `pair` with pad columns and a guard; all must come back untouched, and on an error or an
empty call nothing at all may be written.  `acall` does the same for jg_sim_align with frames_ld = Wmax + 2.

Float operands: jg_sim_topk with k = n_gallery returns every s(w, t), bit-identical by its contract, so the dense s comes from the device.
Against float64, for unit rows, |score - score64| <= (D + W) 2^-24: test_gpu_sim_coupling.py derives it for the mean of W elements each
within D 2^-24 and a chain of W - 1 adds; it holds for every monotone assignment p, and |max_p x_p - max_p y_p| <= max_p |x_p - y_p|."""
import ctypes

import numpy as np
import pytest
import torch

import sim_coupling_cases as C
import sim_ordered_cases as O
import test_gpu_sim_coupling as TC
from test_gpu_sim_coupling import ccall, f32, same, same_pair
from test_gpu_sim_topk import GUARD, INT32_MAX, JG_ERR_ARG, NAN_BITS, P, bits, call as topk_call, dev
from test_gpu_sim_topk_grouped import dev_i32, exact_scores, gcall, ints

pytestmark = pytest.mark.gpu
JG_F32, JG_F16 = 0, 1
FPAD = 2


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


class _Renamed:
    """eng.lib with jg_sim_coupling answering as jg_sim_ordered: the two entries share one parameter list, so ccall serves both"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, "jg_sim_ordered" if name == "jg_sim_coupling" else name)


class _EngView:
    def __init__(self, eng):
        self._eng, self.lib = eng, _Renamed(eng.lib)

    def __getattr__(self, name):
        return getattr(self._eng, name)


def ocall(eng, *a, **kw):
    """One jg_sim_ordered call with ccall's pre-filled outputs, guards and return values"""
    return ccall(_EngView(eng), *a, **kw)


def acall(eng, w, w_off, g, g_off, idx, ordered, group_offset=0, init=None, expect=0, n_queries=None, n_gallery=None, n_groups=None, D=None,
          k=None, dtype=None, frames_ld=None, wp=None, gp=None, null=()):
    """One jg_sim_align call; idx: host (nq, k) int32.  frames / score start from init = (frames (nq, k, Wmax), score) or a -9 / 0x7fc12345
    sentinel.  -> (frames (nq, k, Wmax) int32, score bits (nq, k) int32) host arrays, the pad columns and guards checked."""
    woff = np.ascontiguousarray(w_off, np.int32)
    rows, kk = idx.shape
    wmax = int(np.diff(woff).max())
    ld = wmax + FPAD if frames_ld is None or expect != 0 else frames_ld
    SENT = 0x7fc12345
    fr = torch.full((rows * kk * ld + GUARD,), -9, dtype=torch.int32, device="cuda")
    sc = torch.full((rows * kk + GUARD,), SENT, dtype=torch.int32, device="cuda")
    if init is not None:
        full = np.full((rows, kk, ld), -9, np.int32)
        full[:, :, :wmax] = init[0]
        fr[:rows * kk * ld] = torch.from_numpy(full.reshape(-1)).cuda()
        sc[:rows * kk] = torch.from_numpy(np.ascontiguousarray(init[1]).view(np.int32).reshape(-1)).cuda()
    before_f, before_s = fr.cpu().numpy(), sc.cpu().numpy()
    idxd, goffd = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda(), dev_i32(g_off)
    eng._bind_stream()
    rc = eng.lib.jg_sim_align(eng.h, P(w) if wp is None else wp, None if "woff" in null else woff.ctypes.data_as(ctypes.c_void_p),
                              rows if n_queries is None else n_queries, P(g) if gp is None else gp,
                              (JG_F16 if g.dtype == torch.float16 else JG_F32) if dtype is None else dtype,
                              g.shape[0] if n_gallery is None else n_gallery, w.shape[1] if D is None else D,
                              None if "goff" in null else P(goffd), len(g_off) - 1 if n_groups is None else n_groups, group_offset,
                              None if "idx" in null else P(idxd), kk if k is None else k, ordered, None if "frames" in null else P(fr),
                              ld if frames_ld is None else frames_ld, None if "score" in null else P(sc))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    rf, rs = fr.cpu().numpy(), sc.cpu().numpy()
    assert np.all(rf[rows * kk * ld:] == -9) and np.all(rs[rows * kk:] == SENT), "guard overwritten"
    if expect != 0 or (n_queries is not None and n_queries <= 0):
        assert np.array_equal(rf, before_f) and np.array_equal(rs, before_s), "an output was written"
    rf = rf[:rows * kk * ld].reshape(rows, kk, ld)
    handled = (idx >= group_offset) & (idx < group_offset + (len(g_off) - 1 if n_groups is None else n_groups))
    if expect == 0 and n_queries is None:
        assert np.all(rf[handled][:, wmax:] == -1), "a handled slot is -1 up to frames_ld"
        assert np.array_equal(rf[~handled], before_f[:rows * kk * ld].reshape(rows, kk, ld)[~handled]), "a slot of another piece was written"
        assert np.array_equal(rs[:rows * kk].reshape(rows, kk)[~handled], before_s[:rows * kk].reshape(rows, kk)[~handled])
    return rf[:, :, :wmax].copy(), rs[:rows * kk].reshape(rows, kk).copy()


def same_align(got, want):
    """frames equal; scores NaN in the same places and bit-equal elsewhere (slots that were not written hold acall's -9 / NaN sentinel
    and compare as the -1 / NaN of the restatement's default; acall itself checks that they were not written)"""
    gs, ws = got[1].view(np.float32), np.asarray(want[1], np.float32)
    return np.array_equal(np.where(got[0] == -9, -1, got[0]), want[0]) and np.array_equal(np.isnan(gs), np.isnan(ws)) and np.array_equal(bits(gs)[~np.isnan(gs)], bits(ws)[~np.isnan(ws)])


def check_align(eng, wd, w_off, gd, g_off, s, res_o, res_c, tag):
    """7.: jg_sim_align for the lists of both entries: frames and scores of the restatement, the scores of the entry that made the list, frames
    in order, and s re-added at the frames"""
    w_off = np.asarray(w_off, np.int64)
    for ordered, res in ((1, res_o), (0, res_c)):
        got = acall(eng, wd, w_off, gd, g_off, res[0], ordered)
        want = O.align_expected(s, w_off, g_off, res[0], bool(ordered))
        assert same_align(got, want), (tag, ordered)
        live = res[0] >= 0
        sc = got[1].view(np.float32)
        assert np.array_equal(bits(sc[live]), bits(res[1][live])), (tag, ordered, "the score of the entry that made idx")
        assert np.all(np.isnan(sc[~live]))
        for q in range(len(w_off) - 1):
            W = int(w_off[q + 1] - w_off[q])
            for r in np.nonzero(live[q])[0]:
                t = got[0][q, r, :W]
                assert np.all(t >= 0) and np.all(got[0][q, r, W:] == -1)
                if ordered:
                    assert np.all(np.diff(t) >= 0), (tag, q, r)
                acc = np.float32(0)
                for i in range(W):
                    acc = np.float32(acc + (s[w_off[q] + i, t[i]] + np.float32(0)))
                assert bits(np.float32(acc / np.float32(W))) == bits(sc[q, r]), (tag, ordered, q, r)


# ------------------------------------------------------------------------------------------------ 1. every cut, exact operands
W_COUNTS = [1, 3, 64, 7, 2, 60, 1]                                            # four query tiles: 1 + 3, 64, 7 + 2 (60 moves), 60 + 1


def groups_200(rng):
    """200 rows (four tiles): groups of 0..5 rows up to row 40, one of 150 rows from row 40 (it runs through tiles 0 .. 2 and, with two
    slices of two tiles, on into the second slice), small ones behind it"""
    head = C.offsets_of_counts(rng.integers(0, 6, 40))
    head = head[head < 40]
    return np.concatenate([head, [40, 190], 190 + np.cumsum(rng.integers(0, 6, 4))]).clip(max=200)


@pytest.mark.parametrize("D", [64, 128])
def test_every_cut_gives_the_bits_of_the_restatement(eng, D):
    """entries in -2..2: every product, sum and max is an integer, exact in any order, so only the one division rounds"""
    rng = np.random.default_rng(12000 + D)
    w_off = C.offsets_of_counts(W_COUNTS)
    assert C.plan_expected(w_off) == [0, 2, 3, 5, 7]
    ng = 200
    w, g = ints(rng, (int(w_off[-1]), D)), ints(rng, (ng, D))
    wd, gd = dev(w), dev(g)
    s = f32(exact_scores(w, g))
    small = C.offsets_of_counts(rng.integers(0, 6, 80), first=2)
    layouts = {"long": groups_200(rng),
               "at 64": np.concatenate([small[small < 64], [64], 64 + np.cumsum(rng.integers(0, 6, 60))]).clip(max=198)}
    assert 64 in layouts["at 64"] and 150 in np.diff(layouts["long"])
    for name, g_off in layouts.items():
        for k in (1, 10, 128):
            want = O.ordered_expected(s, w_off, g_off, k)
            for slices in (0, 1, 2, 3):
                got = ocall(eng, wd, w_off, gd, g_off, k, slices=slices)
                assert same(got, want), (name, k, slices)
            if k == 10:
                assert np.sum(~np.isnan(want[2])) > 20 and np.all(want[0][:, 0] >= 0)
                check_align(eng, wd, w_off, gd, g_off, s, got, ccall(eng, wd, w_off, gd, g_off, k), name)


# ------------------------------------------------------------------------------------------------ 2. float operands
def dense_from_topk(eng, wd, gd, n_gallery):
    """every s(w, t) with the device's bits: jg_sim_topk with k = the rows of the gallery returns all of them"""
    s = np.full((wd.shape[0], n_gallery), np.nan, np.float32)
    for a in range(0, n_gallery, 128):                                       # (k <= 128: a piece at a time; the bits do not depend on the cut)
        b = min(a + 128, n_gallery)
        idx, sc = topk_call(eng, wd, gd[a:b].contiguous(), b - a, n_gallery=b - a)
        np.put_along_axis(s[:, a:b], idx.astype(np.int64), sc, axis=1)
    assert not np.isnan(s).any()
    return s


def monotone_best64(s64, a, b):
    """the assignment problem in float64 -> the best mean"""
    M = np.zeros(b - a)
    for i in range(s64.shape[0]):
        M = np.maximum.accumulate(M + s64[i, a:b])
    return M[-1] / s64.shape[0]


@pytest.mark.parametrize("D,ng", [(64, 128), (512, 128), (512, 97)])
def test_float_operands_bit_for_bit_and_against_float64(eng, D, ng):
    rng = np.random.default_rng(12100 + D + ng)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    counts = [1, 2, 7, 17, 9, 3, 17, 8, 64, 5]
    w_off = C.offsets_of_counts(counts)
    w, g = unit(rng.standard_normal((int(w_off[-1]), D))), unit(rng.standard_normal((ng, D)))
    g[1::7] = g[0]                                                           # equal frames: exact ties inside and between groups
    g_off = C.offsets_of_counts([1, 1, 5, 0, 30, 1, 1, 1, 20, 17, 1, 13])
    g_off = g_off[g_off <= ng]
    wd, gd = dev(w), dev(g)
    s = dense_from_topk(eng, wd, gd, ng)
    s64 = w.astype(np.float64) @ g.astype(np.float64).T
    worst = 0.0
    for k in (3, 10):
        want = O.ordered_expected(s, w_off, g_off, k)
        for slices in (0, 1, 2):
            got = ocall(eng, wd, w_off, gd, g_off, k, slices=slices)
            assert same(got, want), (k, slices)
    pair = got[2]
    for q, W in enumerate(counts):
        for gi in range(len(g_off) - 1):
            if g_off[gi + 1] > g_off[gi]:
                ref = monotone_best64(s64[w_off[q]:w_off[q + 1]], int(g_off[gi]), int(g_off[gi + 1]))
                worst = max(worst, abs(float(pair[gi, q]) - ref) / ((D + W) * 2.0 ** -24))
            else:
                assert np.isnan(pair[gi, q])
    print(f"D={D} ng={ng}: worst |score - score64| / ((D + W) 2^-24) = {worst:.4f}")
    assert worst <= 1.0
    check_align(eng, wd, w_off, gd, g_off, s, got, ccall(eng, wd, w_off, gd, g_off, 10), (D, ng))


# ------------------------------------------------------------------------------------------------ 3. the three consequences
def test_the_three_consequences_on_the_device(eng):
    rng = np.random.default_rng(12200)
    D = 64
    # W = 1: jg_sim_topk_grouped's score, and the row it returns is the frame jg_sim_align gives
    w, g = dev(rng.standard_normal((70, D))), dev(rng.standard_normal((150, D)))
    g_off = C.offsets_of_counts([10, 0, 54, 1, 70, 15])
    one = ocall(eng, w, np.arange(71), g, g_off, 4, slices=2)
    rows, sc = gcall(eng, w, g, g_off, 4)
    assert np.array_equal(bits(one[1]), bits(sc)) and np.array_equal(one[0], np.searchsorted(g_off, rows, side="right") - 1)
    fr, fs = acall(eng, w, np.arange(71), g, g_off, one[0], 1)
    assert np.array_equal(fr[:, :, 0], rows) and np.array_equal(fs, bits(sc))
    # ordered <= coupling everywhere, bit-equal where the first arg-max frames are in order
    w_off = C.offsets_of_counts([2, 3, 1, 5, 9, 2, 4, 30])
    wd = dev(rng.standard_normal((int(w_off[-1]), D)))
    s = dense_from_topk(eng, wd, g, 150)
    po, pc = ocall(eng, wd, w_off, g, g_off, 1)[2], ccall(eng, wd, w_off, g, g_off, 1)[2]
    has = ~np.isnan(pc)
    assert np.array_equal(has, ~np.isnan(po)) and np.all(po[has] <= pc[has])
    in_order = O.first_argmax_in_order(s, w_off, g_off).T
    assert in_order.sum() >= 8 and (has & ~in_order).sum() >= 8 and np.array_equal(bits(po[in_order]), bits(pc[in_order]))
    assert np.any(po[has & ~in_order] < pc[has & ~in_order])
    # planted: two clips hold the same frames in opposite order
    a, b_, c = (np.eye(D, dtype=np.float32)[i] for i in range(3))
    clip = np.stack([a, c * 0.1, b_, c * 0.2])
    gal = np.concatenate([clip[::-1], clip])                                 # clip 0 reversed, clip 1 in word order
    words = np.stack([a, b_])
    tie = ccall(eng, dev(words), [0, 2], dev(gal), [0, 4, 8], 2)
    assert tie[0].tolist() == [[0, 1]] and bits(tie[1][0, 0]) == bits(tie[1][0, 1]) and tie[1][0, 0] == 1.0
    got = ocall(eng, dev(words), [0, 2], dev(gal), [0, 4, 8], 2)
    assert got[0].tolist() == [[1, 0]] and got[1].tolist() == [[1.0, 0.5]]
    fr, _ = acall(eng, dev(words), [0, 2], dev(gal), [0, 4, 8], got[0], 1)
    assert fr[0].tolist() == [[4, 6], [0, 1]]                                # the reversed clip: word 1 on its frame, word 0 on the first frame before it
    fr, _ = acall(eng, dev(words), [0, 2], dev(gal), [0, 4, 8], tie[0], 0)
    assert fr[0].tolist() == [[3, 1], [4, 6]]
    # more words than frames: 7 words against groups of 1, 2 and 3 frames
    w7, g6 = ints(rng, (7, D)), ints(rng, (6, D))
    s7 = f32(exact_scores(w7, g6))
    got = ocall(eng, dev(w7), [0, 7], dev(g6), [0, 1, 3, 6], 3)
    assert same(got, O.ordered_expected(s7, [0, 7], [0, 1, 3, 6], 3)) and np.all(got[0] >= 0)
    assert same_align(acall(eng, dev(w7), [0, 7], dev(g6), [0, 1, 3, 6], got[0], 1), O.align_expected(s7, [0, 7], [0, 1, 3, 6], got[0], True))


# ------------------------------------------------------------------------------------------------ 4. a 16-bit gallery
@pytest.mark.parametrize("ng", [129, 1037])
def test_fp16_gallery_gives_the_bits_of_the_widened_gallery(eng, ng):
    rng = np.random.default_rng(12300 + ng)
    w_off = C.offsets_of_counts(TC.W_COUNTS)
    w = ints(rng, (int(w_off[-1]), 128))
    h = rng.standard_normal((ng, 128)).astype(np.float16)
    h[rng.random((ng, 128)) < 0.05] = np.float16(6e-8)
    h[rng.random((ng, 128)) < 0.05] = np.float16(-0.0)
    h[rng.random((ng, 128)) < 0.01] = np.float16(65504.0)
    g16 = torch.from_numpy(h).cuda()
    g32 = g16.float()
    g_off = TC.random_groups(rng, ng)
    wd = dev(w)
    for k in (10, 128):
        ref = ocall(eng, wd, w_off, g32, g_off, k, slices=1)
        assert not np.isnan(ref[1]).any() and np.all(ref[0][:, 0] >= 0)
        for slices in (0, 3):
            assert same(ocall(eng, wd, w_off, g16, g_off, k, slices=slices), ref), (k, slices)
    assert eng.debug_last_kernel() == "sim_ordered_kernel<_Float16,128>+sim_topk_reduce_kernel<128,0>"
    for ordered in (0, 1):
        a16, a32 = acall(eng, wd, w_off, g16, g_off, ref[0][:, :8].copy(), ordered), acall(eng, wd, w_off, g32, g_off, ref[0][:, :8].copy(), ordered)
        assert np.array_equal(a16[0], a32[0]) and np.array_equal(a16[1], a32[1]) and np.all(a16[0][:, :, 0] >= 0)
    assert eng.debug_last_kernel() == "sim_align_kernel<float>"


# ------------------------------------------------------------------------------------------------ 5. merge
@pytest.mark.parametrize("k", [10, 128])
def test_merged_pieces_equal_the_single_call(eng, k):
    rng = np.random.default_rng(12400)
    w_off = C.offsets_of_counts(W_COUNTS)
    g_off = C.offsets_of_counts(rng.integers(0, 9, 150))
    n = int(g_off[-1])
    w, g = ints(rng, (int(w_off[-1]), 64)), ints(rng, (n, 64))
    wd = dev(w)
    s = f32(exact_scores(w, g))
    want = O.ordered_expected(s, w_off, g_off, k)
    assert same(ocall(eng, wd, w_off, dev(g), g_off, k), want)
    cuts = [0, 40, 41, 150]
    for order in ((0, 1, 2), (2, 0, 1)):
        cur = None
        for step, pc in enumerate(order):
            ga, gb = cuts[pc], cuts[pc + 1]
            r0, r1 = int(g_off[ga]), int(g_off[gb])
            piece = dev(g[r0:r1])
            if pc == 1:
                piece = piece.half()
            got = ocall(eng, wd, w_off, piece, g_off[ga:gb + 1] - r0, k, slices=(0, 2, 5)[step], group_offset=ga, merge=int(step > 0), init=cur,
                        n_gallery=r1 - r0)
            assert same_pair(got[2], want[2][ga:gb]), (order, pc)
            cur = got[:2]
        assert same(cur + (None,), want), order
        # the frames, piece by piece with the final idx: a piece fills the slots of its own groups and leaves the others
        fill = None
        for pc in order:
            ga, gb = cuts[pc], cuts[pc + 1]
            r0, r1 = int(g_off[ga]), int(g_off[gb])
            fill = acall(eng, wd, w_off, dev(g[r0:r1]), g_off[ga:gb + 1] - r0, cur[0], 1, group_offset=ga,
                         init=None if fill is None else (fill[0], fill[1].view(np.float32)))
            fill[0][(cur[0] >= ga) & (cur[0] < gb)] += np.where(fill[0][(cur[0] >= ga) & (cur[0] < gb)] >= 0, r0, 0).astype(np.int32)
        whole = O.align_expected(s, w_off, g_off, cur[0], True)
        live = cur[0] >= 0
        assert np.array_equal(fill[0][live], whole[0][live]) and np.array_equal(bits(fill[1].view(np.float32)[live]), bits(whole[1][live]))
        assert np.all(fill[0][~live] == -9)                                  # a slot holding -1 keeps the sentinel


# ------------------------------------------------------------------------------------------------ 6. special values
def test_nan_negative_zero_ties_and_too_few_groups(eng):
    rng = np.random.default_rng(12500)
    D = 64
    w_off = [0, 2, 5, 6, 8]
    w = ints(rng, (8, D))
    w[5] = np.nan                                                            # query 2 is one NaN word: it has no score anywhere
    g = ints(rng, (150, D))
    g[[0, 5, 63, 64, 100, 149]] = np.nan                                     # NaN frames are skipped
    g[128:140] = np.nan                                                      # ... and a group of nothing else has no score
    g[20:30] = 0
    g[20:30:2] = -0.0
    g[40:47] = g[70:77]                                                      # two groups of equal rows: equal scores
    g_off = np.asarray([0, 7, 20, 30, 40, 47, 64, 70, 77, 128, 140, 150])
    s = f32(exact_scores(w, g))
    for k in (4, 20):
        want = O.ordered_expected(s, w_off, g_off, k)
        for slices in (0, 1, 3):
            got = ocall(eng, dev(w), w_off, dev(g), g_off, k, slices=slices)
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
        if k == 20:
            assert np.all(np.sum(idx >= 0, axis=1) == [10, 10, 0, 10]) and np.all(np.isneginf(score[idx < 0]))
    for ordered, res in ((1, got), (0, ccall(eng, dev(w), w_off, dev(g), g_off, 20))):
        al = acall(eng, dev(w), w_off, dev(g), g_off, res[0], ordered)
        assert same_align(al, O.align_expected(s, w_off, g_off, res[0], bool(ordered)))
        assert not np.isin(al[0], [0, 5, 63, 64, 100, 149]).any()            # a NaN frame is nobody's
    # idx naming pairs without a score: the NaN query, the NaN group, an empty group -> -1 / NaN, written
    probe = np.asarray([[9, 0], [3, 9], [0, 1], [9, 9]], np.int32)
    goff2 = np.concatenate([g_off[:3], g_off[2:]])                           # group 2 is now empty, the NaN group is 10
    probe2 = np.where(probe == 9, 10, probe).astype(np.int32)
    probe2[0, 1] = 2
    for ordered in (0, 1):
        fr, sc = acall(eng, dev(w), w_off, dev(g), goff2, probe2, ordered)
        assert same_align((fr, sc), O.align_expected(s, w_off, goff2, probe2, bool(ordered)))
        assert np.all(fr[0, 1] == -1) and np.all(fr[2] == -1) and np.all(fr[probe2 == 10] == -1) and np.isnan(sc.view(np.float32)[0, 1])


# ------------------------------------------------------------------------------------------------ 7. the longest group that is aligned
def test_align_takes_groups_of_up_to_8192_rows(eng):
    rng = np.random.default_rng(12600)
    D = 64
    n = 5 + 8192 + 8193 + 3
    g = ints(rng, (n, D))
    g[5 + 8000] = 2                                                          # the best frame of every +2 word, deep in the 126th tile
    w = ints(rng, (3, D))
    w[1] = 2
    g_off = [5, 5 + 8192, 5 + 8192 + 8193, n]                                # 8192 rows from an unaligned row: 129 tiles; 8193 rows; 3 rows
    s = f32(exact_scores(w, g))
    idx = np.asarray([[0, 1, 2], [1, 0, -1]], np.int32)
    wd, gd = dev(w), dev(g)
    for ordered in (0, 1):
        got = acall(eng, wd, [0, 1, 3], gd, g_off, idx, ordered)
        want = O.align_expected(s, [0, 1, 3], g_off, idx, bool(ordered))
        assert same_align(got, want), ordered
        assert np.all(got[0][idx == 1] == -1) and np.all(got[0][0, 0, :1] >= 5) and got[0][1, 1, 0] == 5 + 8000
        assert np.all(got[0][1, 2] == -9)                                    # the slot holding -1 is not written
    # the two scoring entries have no such limit, and agree with the frames where there are some
    so, sc = ocall(eng, wd, [0, 1, 3], gd, g_off, 3, want_pair=False), ccall(eng, wd, [0, 1, 3], gd, g_off, 3, want_pair=False)
    assert same(so, O.ordered_expected(s, [0, 1, 3], g_off, 3)) and same(sc, C.coupling_expected(s, [0, 1, 3], g_off, 3))
    al = acall(eng, wd, [0, 1, 3], gd, g_off, so[0], 1)
    ok = so[0] != 1
    assert np.array_equal(al[1][ok], bits(so[1])[ok]) and np.all(np.isnan(al[1].view(np.float32)[~ok]))


# ------------------------------------------------------------------------------------------------ 8. refusals and empty calls
def test_bad_arguments_launch_nothing(eng):
    rng = np.random.default_rng(12700)
    w, g = dev(rng.standard_normal((70, 128))), dev(rng.standard_normal((90, 128)))
    w_off, g_off = [0, 3, 20, 70], [0, 30, 90]
    bad = [dict(wp=ctypes.c_void_p(None)), dict(gp=ctypes.c_void_p(None)), dict(null_idx=True), dict(null_score=True), dict(null_goff=True),
           dict(null_woff=True), dict(dtype=2), dict(slices=-1), dict(slices=1025), dict(k=0), dict(k=129), dict(D=0), dict(D=96),
           dict(n_queries=-1), dict(n_gallery=-1), dict(n_groups=-1), dict(group_offset=-1), dict(group_offset=INT32_MAX - 1), dict(pair_ld=2),
           dict(wp=ctypes.c_void_p(w.data_ptr() + 4)), dict(gp=ctypes.c_void_p(g.data_ptr() + 8)),
           dict(w_off=[0, 3, 3, 70]), dict(w_off=[0, 3, 68, 70]), dict(w_off=[0, 20, 10, 70]), dict(w_off=[1, 3, 20, 70])]
    for kw in bad:
        kw = dict(kw)
        ocall(eng, w, kw.pop("w_off", w_off), g, g_off, kw.pop("k", 5), expect=JG_ERR_ARG, **kw)
        assert eng.debug_last_kernel() == ""
    ocall(eng, w, w_off, g, g_off, 5, n_queries=0)                           # JG_OK, nothing launched, nothing written
    assert eng.debug_last_kernel() == ""
    kept = ocall(eng, w, w_off, g, g_off, 5)[:2]
    for kw in (dict(n_gallery=0), dict(n_groups=0)):
        got = ocall(eng, w, w_off, g, g_off, 5, slices=3, merge=1, init=kept, **kw)
        assert same(got[:2] + (None,), kept + (None,)) and np.isnan(got[2]).all()
        idx, score, pair = ocall(eng, w, w_off, g, g_off, 5, **kw)
        assert np.all(idx == -1) and np.all(np.isneginf(score)) and np.isnan(pair).all()
    # jg_sim_align
    idx = kept[0]
    bad = [dict(wp=ctypes.c_void_p(None)), dict(gp=ctypes.c_void_p(None)), dict(null=("idx",)), dict(null=("frames",)), dict(null=("score",)),
           dict(null=("goff",)), dict(null=("woff",)), dict(dtype=2), dict(dtype=-1), dict(k=0), dict(k=129), dict(k=-1), dict(D=0), dict(D=96),
           dict(n_queries=-1), dict(n_gallery=-1), dict(n_groups=-1), dict(group_offset=-1), dict(group_offset=INT32_MAX - 1),
           dict(frames_ld=49), dict(frames_ld=0), dict(frames_ld=-1), dict(wp=ctypes.c_void_p(w.data_ptr() + 4)),
           dict(gp=ctypes.c_void_p(g.data_ptr() + 8)), dict(w_off=[0, 3, 3, 70]), dict(w_off=[0, 3, 68, 70]), dict(w_off=[1, 3, 20, 70])]
    for kw in bad:
        kw = dict(kw)
        acall(eng, w, kw.pop("w_off", w_off), g, g_off, idx, 1, expect=JG_ERR_ARG, **kw)
        assert eng.debug_last_kernel() == ""
    acall(eng, w, w_off, g, g_off, idx, 1, n_queries=0)                      # JG_OK, nothing launched, nothing written
    assert eng.debug_last_kernel() == ""
    fr, _ = acall(eng, w, w_off, g, g_off, idx, 1, frames_ld=50)             # the longest query exactly
    assert np.all(fr[:, :2, 0] >= 0)
    assert eng.debug_last_kernel() == "sim_align_kernel<float>"
    # offsets that are no partition: some result, nothing outside the outputs (the guards of ocall / acall) -- only that
    for hostile in ([90, 30, 0], [-5, 200, 1000], [0, 2 ** 31 - 1, -2 ** 31]):
        res = ocall(eng, w, w_off, g, hostile, 5, slices=2)
        acall(eng, w, w_off, g, hostile, np.where(res[0] >= 0, res[0], 0).astype(np.int32), 1)
        acall(eng, w, w_off, g, hostile, np.tile(np.asarray([[0, 1, 0, 1, 0]], np.int32), (3, 1)), 0)


# ------------------------------------------------------------------------------------------------ 9. what was launched, and the workspace
def test_poisoned_workspace_and_the_names_of_the_launches(eng):
    rng = np.random.default_rng(12800)
    w_off = C.offsets_of_counts(W_COUNTS)
    g_off = C.offsets_of_counts(rng.integers(0, 9, 120))
    w, g = dev(ints(rng, (int(w_off[-1]), 64))), dev(ints(rng, (int(g_off[-1]), 64)))
    first = {(k, s): ocall(eng, w, w_off, g, g_off, k, slices=s) for k in (10, 128) for s in (1, 7)}
    al = acall(eng, w, w_off, g, g_off, first[(10, 1)][0], 1)
    eng.set_option("ws_poison", 1)
    try:
        for (k, s), want in first.items():
            assert same(ocall(eng, w, w_off, g, g_off, k, slices=s), want), (k, s, "poisoned")
            L = 64 if k <= 64 else 128
            assert eng.debug_last_kernel() == f"sim_ordered_kernel<float,{L}>" + (f"+sim_topk_reduce_kernel<{L},0>" if s > 1 else "")
        again = acall(eng, w, w_off, g, g_off, first[(10, 1)][0], 1)
        assert np.array_equal(again[0], al[0]) and np.array_equal(again[1], al[1])
    finally:
        eng.set_option("ws_poison", 0)
    for (k, s), want in first.items():
        assert same(ocall(eng, w, w_off, g.half(), g_off, k, slices=s), want), (k, s, "second run, fp16")
    assert eng.debug_last_kernel() == "sim_ordered_kernel<_Float16,128>+sim_topk_reduce_kernel<128,0>"


# ------------------------------------------------------------------------------------------------ 10. the Python front ends
def test_python_front_ends_on_the_device(eng):
    from jegal_amd import metrics as M
    rng = np.random.default_rng(12900)
    lens = [5, 40, 17, 70, 33, 21]
    clips = [rng.standard_normal((t, 64)).astype(np.float32) for t in lens]
    # the phrase: frames 60, 31 and 8 of clip 3 in THAT order, and the same three planted in word order at 4, 11 and 29 of clip 4
    words = [clips[3][60].copy(), clips[3][31].copy(), clips[3][8].copy()]
    for t, wd in zip((4, 11, 29), words):
        clips[4][t] = wd + 0.05 * rng.standard_normal(64).astype(np.float32)
    phrases = [np.stack(words), clips[1][7:8].copy(), rng.standard_normal((9, 64)).astype(np.float32)]
    un = M.search_phrases(phrases, clips, k=4, engine=eng, align=True)
    got = M.search_phrases(phrases, clips, k=4, engine=eng, order=True, align=True)
    assert un[0][0, 0] == 3 and un[3][0, 0, :3].tolist() == [60, 31, 8]
    assert got[0][0, 0] == 4 and got[3][0, 0, :3].tolist() == [4, 11, 29] and np.all(got[3][0, :, 3:] == -1)
    assert got[0][1, 0] == 1 and got[3][1, 0, 0] == 7 and got[3].shape == (3, 4, 9) and got[3].dtype == np.int32
    assert np.all(np.diff(np.where(got[3] >= 0, got[3], 10 ** 6), axis=2) >= 0) and np.all(got[2] <= un[2])
    # pieces under max_rows and segments: the result of one piece; the frames lie in the returned segment
    one = M.search_phrases(phrases, clips, k=5, segment=16, engine=eng, order=True, align=True)
    cut = M.search_phrases(phrases, clips, k=5, segment=16, engine=eng, order=True, align=True, max_rows=48)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(one, cut))
    live = one[3] >= 0
    assert np.all((one[3] >= one[1][:, :, None])[live]) and np.all((one[3] < one[1][:, :, None] + 16)[live]) and one[0][1, 0] == 1 and one[3][1, 0, 0] == 7
    # against the restatement, from the device's own s
    pn = [eng.l2norm(torch.from_numpy(p)) for p in phrases]
    gn = eng.l2norm(torch.from_numpy(np.concatenate(clips)))
    s = dense_from_topk(eng, torch.cat(pn), gn, sum(lens))
    w_off, g_off = M.offsets_of(phrases), M.offsets_of(clips)
    e = O.ordered_expected(s, w_off, g_off, 4)
    assert np.array_equal(got[0], e[0]) and np.array_equal(bits(got[2]), bits(e[1]))
    fr = O.align_expected(s, w_off, g_off, e[0], True)[0]
    assert np.array_equal(got[3], np.where(fr >= 0, fr - g_off[np.maximum(e[0], 0)][:, :, None], -1))
    # Corpus.search_phrases over float16 rows: search_phrases on the widened stored rows
    c16 = M.Corpus.build(clips, engine=eng)
    stored = np.split(c16.rows.astype(np.float32), np.cumsum(lens)[:-1])
    for segment, max_rows in ((0, None), (16, 48)):
        a = c16.search_phrases(phrases, k=4, segment=segment, engine=eng, max_rows=max_rows, order=True, align=True)
        b = M.search_phrases([p.cpu().numpy() for p in pn], stored, k=4, segment=segment, normalize=False, engine=eng, max_rows=max_rows,
                             order=True, align=True)
        assert len(a) == 4 and all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0][0, 0] == 4
    # coupling_retrieval_metrics(ordered): utterances are frames of their own clip in order -> every partner first; the matrix is the entry's
    contents = [np.stack([c[i] for i in np.sort(rng.choice(len(c), min(len(c), 4), replace=False))]) for c in clips]
    res = M.coupling_retrieval_metrics(contents, clips, engine=eng, ordered=True)
    assert res["c2g"]["R1"] == 1.0 and res["c2g"]["MR"] == 1.0
    mo, mc = M.coupling_matrix(contents, clips, engine=eng, ordered=True).cpu().numpy(), M.coupling_matrix(contents, clips, engine=eng).cpu().numpy()
    assert mo.shape == (6, 6) and np.all(mo <= mc) and np.any(mo < mc) and np.array_equal(bits(np.diag(mo)), bits(np.diag(mc)))
    # Engine.sim_align with into: only this call's slots change
    idx, _ = eng.sim_ordered(torch.cat(pn), w_off, gn, g_off, 4)
    frames, score = eng.sim_align(torch.cat(pn), w_off, gn, g_off, idx, True)
    assert tuple(frames.shape) == (3, 4, 9) and frames.dtype == torch.int32 and np.array_equal(frames.cpu().numpy(), fr)
    half = eng.sim_align(torch.cat(pn), w_off, gn[:int(g_off[3])], g_off[:4], idx, True)
    assert np.array_equal(half[0].cpu().numpy()[e[0] < 3], fr[e[0] < 3]) and np.all(half[0].cpu().numpy()[e[0] >= 3] == -1)
    assert np.all(np.isnan(half[1].cpu().numpy()[e[0] >= 3]))
    full = eng.sim_align(torch.cat(pn), w_off, gn[int(g_off[3]):], g_off[3:] - g_off[3], idx, True, group_offset=3, into=half)
    assert full[0] is half[0] and np.array_equal(np.isnan(full[1].cpu().numpy()), e[0] < 0)
