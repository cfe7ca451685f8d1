"""jg_sim_topk_grouped and jg_group_of_rows through the C ABI (run with -m gpu): the gallery rows are cut into contiguous groups, a group
scores as its best row (first arg-max), and per query row the k best groups come back, each as the row that earned the score -- never two
rows of one group; scores bit-identical to jg_sim_topk's; pieces of a gallery, cut at group boundaries, merged into the result of the whole.

Every call goes through `gcall`: idx / score are pre-filled with a -7 / NaN pattern (or with the list to merge into) and followed by a
guard of 64 elements that must come back untouched, as tests/test_gpu_sim_topk.py::call does.

Exact cases use small-integer operands: every score is exact in fp32 in any order, and the expected list comes from numpy (`expected`)
with no tolerance.

Float64 rule (check_fp64_grouped), the bound of tests/test_gpu_sim_topk.py: b_ij = D * 2^-24 * sum_k |q_ik g_jk| bounds the error of a
length-D fp32 fma chain.  (a) a returned score is within b of the float64 dot product of its pair; (b) the list is sorted by (score
descending, row ascending) in its own fp32 values, its rows lie in range and in distinct groups, and it holds min(k, groups with a row)
entries; (c) no row of a group left out beats the weakest returned row (in float64) by more than the two bounds together; and, by the same
argument inside a group, (d) no row of a returned group beats the returned row by more than the two bounds together.  No case is left
out of any of them."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

from test_gpu_sim_topk import GUARD, INT32_MAX, JG_ERR_ARG, NAN_BITS, P, bits, call as topk_call, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def dev_i32(a):
    """host ints -> device int32; an empty array still gets a (non-null) buffer"""
    a = np.asarray(a, np.int64).reshape(-1)
    t = torch.zeros(max(a.size, 1), dtype=torch.int32, device="cuda")
    t[:a.size] = torch.from_numpy(a.astype(np.int32))
    return t


def gcall(eng, q, g, off, k, gallery_offset=0, merge=0, init=None, n_queries=None, n_gallery=None, n_groups=None, D=None, expect=0,
          qp=None, gp=None, null_off=False, null_idx=False, null_score=False):
    """One jg_sim_topk_grouped call; q / g: device tensors (rows, D), off: host group offsets (n_groups + 1 entries, local rows).
    init = (idx, score) host arrays to start from (merge, or a hostile pattern).  -> (idx (n,k) int32, score (n,k) float32) host arrays;
    asserts the return code and the guards; on an error or an empty call asserts that nothing at all was written."""
    nq = q.shape[0] if n_queries is None else n_queries
    ng = g.shape[0] if n_gallery is None else n_gallery
    ngr = len(off) - 1 if n_groups is None else n_groups
    offd = dev_i32(off)
    rows, kraw, k = q.shape[0], k, max(k, 1)
    idx = torch.full((rows * k + GUARD,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((rows * k + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    if init is not None:
        idx[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[0], np.int32).reshape(-1)).cuda()
        sc[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[1], np.float32).reshape(-1).view(np.int32)).cuda()
    before_i, before_s = idx.cpu().numpy(), sc.cpu().numpy()
    eng._bind_stream()
    rc = eng.lib.jg_sim_topk_grouped(eng.h, P(q) if qp is None else qp, P(g) if gp is None else gp, nq, ng, q.shape[1] if D is None else D,
                                     kraw, None if null_off else P(offd), ngr, gallery_offset, merge, None if null_idx else P(idx),
                                     None if null_score else P(sc))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    ri, rs = idx.cpu().numpy(), sc.cpu().numpy()
    assert np.all(ri[rows * k:] == -7) and np.all(rs[rows * k:] == NAN_BITS), "guard overwritten"
    if expect != 0 or nq <= 0:
        assert np.array_equal(ri, before_i) and np.array_equal(rs, before_s), "an output was written"
    if 0 < nq < rows:                                                   # rows the call was not asked for
        assert np.array_equal(ri[nq * k:], before_i[nq * k:]) and np.array_equal(rs[nq * k:], before_s[nq * k:])
    return ri[:rows * k].reshape(rows, k), rs[:rows * k].view(np.float32).reshape(rows, k)


def offsets(sizes, first=0):
    return np.concatenate([[first], first + np.cumsum(sizes)]).astype(np.int64)


def exact_scores(q, g):
    """float64 scores of small-integer (or NaN) operands: exact, and NaN where a gallery row is NaN"""
    with np.errstate(invalid="ignore"):
        return q.astype(np.float64) @ g.astype(np.float64).T if g.shape[0] else np.zeros((q.shape[0], 0))


def expected(s, off, k, offset=0, init=None):
    """s: (nq, ng) scores that fp32 holds exactly (NaN: no candidate), off: group offsets -> the list jg_sim_topk_grouped must return:
    per group its first arg-max row, of those (and of init = an earlier list for other rows) the k best by (score desc, row asc)"""
    nq = s.shape[0]
    nan = np.isnan(s)
    sc = np.where(nan, -np.inf, s) + 0.0                                 # (-0.0 counts and comes back as +0.0)
    rows, vals, ok = [], [], []
    for a, b in zip(off[:-1], off[1:]):
        a, b = int(max(a, 0)), int(min(b, s.shape[1]))
        if b > a:
            j = np.argmax(sc[:, a:b], axis=1)                            # the first arg-max
            rows.append(offset + a + j)
            vals.append(sc[np.arange(nq), a + j])
            ok.append(~np.all(nan[:, a:b], axis=1))
    if init is not None:
        for r in range(init[0].shape[1]):
            rows.append(init[0][:, r].astype(np.int64))
            vals.append(init[1][:, r].astype(np.float64))
            ok.append(init[0][:, r] >= 0)
    idx = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), -np.inf, np.float32)
    if not rows:
        return idx, out
    rows, vals, ok = np.stack(rows, 1), np.stack(vals, 1), np.stack(ok, 1)
    for i in range(nq):
        r, v = rows[i][ok[i]], vals[i][ok[i]]
        order = np.lexsort((r, -v))[:k]
        idx[i, :len(order)] = r[order]
        out[i, :len(order)] = v[order]
    return idx, out


def check_exact(eng, q, g, off, k, offset=0, tag=""):
    idx, sc = gcall(eng, dev(q), dev(g), off, k, gallery_offset=offset, n_queries=q.shape[0], n_gallery=g.shape[0])
    want_i, want_s = expected(exact_scores(q, g), off, k, offset)
    assert np.array_equal(idx, want_i), (tag, q.shape, g.shape, k)
    assert np.array_equal(bits(sc), bits(want_s)), (tag, q.shape, g.shape, k)
    return idx, sc


def ints(rng, shape, lo=-2, hi=3):
    return rng.integers(lo, hi, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. groups of one row = jg_sim_topk
@pytest.mark.parametrize("k", [1, 10, 64, 65, 128])
def test_groups_of_one_row_give_the_bits_of_sim_topk(eng, k):
    rng = np.random.default_rng(5100)
    for D in (64, 512):
        q, g = ints(rng, (130, D)), ints(rng, (333, D))
        gd = dev(g)
        for nq in (1, 64, 65, 130):
            qd = dev(q[:nq])
            want_i, want_s = topk_call(eng, qd, gd, k)
            idx, sc = gcall(eng, qd, gd, np.arange(334), k)
            assert np.array_equal(idx, want_i) and np.array_equal(bits(sc), bits(want_s)), (D, nq)
    # float rows: the scores are jg_sim_topk's bit for bit whatever they are
    qf, gf = rng.standard_normal((65, 512)).astype(np.float32), rng.standard_normal((200, 512)).astype(np.float32)
    want_i, want_s = topk_call(eng, dev(qf), dev(gf), k, gallery_offset=1000)
    idx, sc = gcall(eng, dev(qf), dev(gf), np.arange(201), k, gallery_offset=1000)
    assert np.array_equal(idx, want_i) and np.array_equal(bits(sc), bits(want_s))


# ------------------------------------------------------------------------------------------------ 2. group and tile boundaries
@pytest.mark.parametrize("nq,D", [(1, 64), (64, 64), (65, 512), (130, 64)])
def test_group_boundaries_against_tile_boundaries(eng, nq, D):
    """groups that end at row 63 / begin at row 64, that span several 64-row tiles, and empty groups at the start, in the middle and at the
    end; then the same gallery behind 1, 63 and 64 leading rows (a group without a champion, or rows that belong to no group)"""
    rng = np.random.default_rng(5200 + nq + D)
    sizes = [0, 1, 62, 3, 0, 70, 200, 0, 5, 0]
    q, g = ints(rng, (nq, D)), ints(rng, (sum(sizes), D))
    off = offsets(sizes)
    base = {k: check_exact(eng, q, g, off, k, tag="plain") for k in (1, 3, 10)}
    assert np.all(np.sum(base[10][0] >= 0, axis=1) == 6)                   # six groups have a row
    check_exact(eng, q, g, offsets([64, 64, 64, 64, 85]), 10, tag="groups = tiles")
    check_exact(eng, q, g, offsets([63, 1, 128, 149]), 3, tag="63 / 64")
    check_exact(eng, q, g, offsets(sizes[:6]), 10, tag="rows behind the last group belong to none")
    for lead in (1, 63, 64):
        nan_rows = np.full((lead, D), np.nan, np.float32)                  # a dummy group in front: every score NaN, never a champion
        junk = ints(rng, (lead, D), 50, 60)                                # or rows in front of the first group: they would win, and belong to none
        for k in (1, 3, 10):
            for tag, front, o in (("dummy group", nan_rows, np.concatenate([[0], off + lead])), ("no group", junk, off + lead)):
                idx, sc = gcall(eng, dev(q), dev(np.concatenate([front, g])), o, k)
                assert np.array_equal(idx, np.where(base[k][0] >= 0, base[k][0] + lead, -1)), (tag, lead, k)
                assert np.array_equal(bits(sc), bits(base[k][1])), (tag, lead, k)


# ------------------------------------------------------------------------------------------------ 3. champion dynamics
@pytest.mark.parametrize("shape", ["ascending", "descending", "peak"])
def test_a_long_group_keeps_one_entry(eng, shape):
    """three groups of 50, 200 and 45 rows; the scores of the 200-row group (rows 50 .. 249: four tiles) rise from row to row, fall, or peak
    in its middle: its champion improves from tile to tile, or never.  The result holds min(k, 3) entries -- a kernel that keeps several
    rows of a group fills the k = 10 list with rows of the long group"""
    rng = np.random.default_rng(5300)
    t = np.arange(200)
    v = {"ascending": 10 * t, "descending": 10 * (199 - t), "peak": 10 * (100 - np.abs(t - 100))}[shape]
    g = np.zeros((295, 64), np.float32)
    g[:, 0] = np.concatenate([rng.integers(0, 1500, 50), v, rng.integers(0, 1500, 45)])
    g[:, 1] = rng.integers(-3, 4, 295)
    q = np.zeros((65, 64), np.float32)
    q[:, 0], q[:, 1] = rng.integers(1, 4, 65), rng.integers(-1, 2, 65)     # score = a v + b w, a >= 1, |b w| <= 3 < 10: the shape decides
    off = offsets([50, 200, 45])
    peak = {"ascending": 249, "descending": 50, "peak": 150}[shape]
    for k in (1, 3, 10):
        idx, sc = check_exact(eng, q, g, off, k, tag=shape)
        n = min(k, 3)
        assert np.all(idx[:, :n] >= 0) and np.all(idx[:, n:] == -1) and np.all(np.isneginf(sc[:, n:]))
        if k >= 3:
            assert np.all(np.sum(idx == peak, axis=1) == 1)                # the long group, as its best row
            assert np.all(np.sum((idx >= 50) & (idx < 250), axis=1) == 1)


# ------------------------------------------------------------------------------------------------ 4. eviction
@pytest.fixture(scope="module")
def small_groups():
    """~300 groups of 1..3 rows (and a few empty ones), D = 64, 65 queries: random integer rows, and a copy whose scores carry a trend that
    rises with the row, so that every tile evicts entries and a group's later row beats its earlier one"""
    rng = np.random.default_rng(5400)
    sizes = rng.integers(1, 4, 300)
    sizes[rng.integers(0, 300, 10)] = 0
    n = int(sizes.sum())
    q, g = ints(rng, (65, 64)), ints(rng, (n, 64))
    q[:, 0] = 1
    trend = g.copy()
    trend[:, 0] = np.arange(n) // 2
    return {"q": q, "random": g, "trend": trend, "off": offsets(sizes)}


@pytest.mark.parametrize("k", [64, 128])
def test_eviction_with_many_small_groups(eng, small_groups, k):
    sg = small_groups
    for name in ("random", "trend", "trend reversed"):
        g = sg["trend"][::-1].copy() if name == "trend reversed" else sg[name]
        off = sg["off"] if name != "trend reversed" else (sg["off"][-1] - sg["off"][::-1])
        idx, sc = check_exact(eng, sg["q"], g, off, k, tag=name)
        grp = np.searchsorted(off, idx, side="right")
        assert all(len(set(grp[i].tolist())) == k for i in range(idx.shape[0])), name


# ------------------------------------------------------------------------------------------------ 5. ties and special values
def test_ties_go_to_the_smaller_row(eng):
    rng = np.random.default_rng(5500)
    q = ints(rng, (65, 64))
    row = ints(rng, (1, 64))
    sizes = [3, 1, 4, 60, 2, 70, 1]
    same = np.repeat(row, sum(sizes), axis=0)                              # every row equal: a group's champion is its first row, groups in order
    off = offsets(sizes)
    for k in (1, 5, 10):
        idx, sc = check_exact(eng, q, same, off, k, tag="all equal")
        assert np.array_equal(idx[0, :min(k, 7)], off[:-1][:min(k, 7)])
    g = ints(rng, (141, 64))
    g[100:141] = g[20:61]                                                  # duplicates in other groups, and (rows 20 / 21) inside one
    g[21] = g[20]
    g[101] = g[100]
    for k in (1, 10, 64):
        check_exact(eng, q, g, off, k, tag="duplicates")


def test_nan_and_negative_zero(eng):
    rng = np.random.default_rng(5600)
    q, g = ints(rng, (65, 64)), ints(rng, (200, 64))
    sizes = [10, 5, 60, 0, 25, 100]
    off = offsets(sizes)
    g[10:15] = np.nan                                                      # group 1: every row NaN -> never returned
    g[[0, 20, 74, 75, 199]] = np.nan                                       # rows inside groups: ignored, the first and the last row of a group among them
    for k in (1, 4, 10):
        idx, sc = check_exact(eng, q, g, off, k, tag="nan")
        assert not np.isin(idx, [0, 10, 11, 12, 13, 14, 20, 74, 75, 199]).any()
        assert np.all(np.sum(idx >= 0, axis=1) == min(k, 4))               # four groups have a champion; k larger: the rest is empty
        assert not np.isnan(sc).any()
    z = np.zeros((65, 64), np.float32)
    z[1::2] = -0.0
    neg = -np.abs(ints(rng, (200, 64))) - 0.0                              # -0.0 entries and negative ones: products of both signs of zero
    for qq, gg in ((z, neg), (q, np.concatenate([z[:40], neg[:160]])), (z, g)):
        idx, sc = check_exact(eng, qq, gg, off, 10, tag="zeros")
        assert not np.any(bits(sc) == np.int32(-2 ** 31))                  # -0.0 comes back as +0.0


def test_no_group_no_gallery(eng):
    rng = np.random.default_rng(5700)
    q, g = ints(rng, (65, 64)), ints(rng, (90, 64))
    qd, gd = dev(q), dev(g)
    held = expected(exact_scores(q, g), offsets([40, 50]), 7, offset=500)
    for kw in (dict(off=[0], n_groups=0), dict(off=[0, 0], n_gallery=0), dict(off=[0, 0, 0]), dict(off=[90, 90]), dict(off=[5], n_groups=0, null_off=True)):
        off = kw.pop("off")
        idx, sc = gcall(eng, qd, gd, off, 7, **kw)
        assert np.all(idx == -1) and np.all(np.isneginf(sc)), off
        idx, sc = gcall(eng, qd, gd, off, 7, merge=1, init=held, **kw)       # with merge the list stays
        assert np.array_equal(idx, held[0]) and np.array_equal(bits(sc), bits(held[1])), off
    idx, sc = check_exact(eng, q, g, offsets([40, 50]), 7)                     # k larger than the number of groups
    assert np.all(idx[:, 2:] == -1)


# ------------------------------------------------------------------------------------------------ 6. merge
@pytest.mark.parametrize("k", [10, 128])
def test_merged_pieces_equal_the_single_call(eng, small_groups, k):
    """a gallery cut at group boundaries into 2 and 5 pieces, merged forward, in reverse and shuffled; clip-sized groups that span tiles too"""
    rng = np.random.default_rng(5800)
    sg = small_groups
    long_sizes = [150, 1, 149, 0, 70, 64, 130]
    cases = [("small", sg["q"], sg["trend"], sg["off"]), ("small random", sg["q"], sg["random"], sg["off"]),
             ("clips", ints(rng, (130, 512)), ints(rng, (sum(long_sizes), 512)), offsets(long_sizes))]
    for name, q, g, off in cases:
        want_i, want_s = check_exact(eng, q, g, off, k, tag=name)
        qd, G = dev(q), len(off) - 1
        for pieces in (2, 5):
            cuts = np.unique(np.concatenate([[0, G], rng.integers(1, G, pieces - 1)])) if name != "clips" else np.asarray([0, 2, 3, 5, 6, 7][:pieces] + [G])
            cuts = np.unique(cuts)
            parts = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
            orders = [list(range(len(parts))), list(range(len(parts)))[::-1], list(rng.permutation(len(parts)))]
            for order in orders:
                cur = None
                for n, p in enumerate(order):
                    ga, gb = parts[p]
                    r0, r1 = int(off[ga]), int(off[gb])
                    cur = gcall(eng, qd, dev(g[r0:r1]), off[ga:gb + 1] - r0, k, gallery_offset=r0, merge=int(n > 0), init=cur, n_gallery=r1 - r0)
                assert np.array_equal(cur[0], want_i), (name, pieces, order)
                assert np.array_equal(bits(cur[1]), bits(want_s)), (name, pieces, order)
    # merge = 0 never reads idx / score: a list that would win every comparison changes nothing
    hostile = (np.tile(np.arange(k, dtype=np.int32), (q.shape[0], 1)), np.full((q.shape[0], k), np.inf, np.float32))
    got = gcall(eng, qd, dev(g), off, k, merge=0, init=hostile)
    assert np.array_equal(got[0], want_i) and np.array_equal(bits(got[1]), bits(want_s))


# ------------------------------------------------------------------------------------------------ 7. float64
def check_fp64_grouped(name, q, g, off, idx, score, k):
    """(a) .. (d) of the module docstring for the list (idx, score) of queries q (n, D) against gallery g (m, D) in groups off, host float32"""
    D = q.shape[1]
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    s64 = q64 @ g64.T
    b = D * 2.0 ** -24 * (np.abs(q64) @ np.abs(g64).T)
    in_group = np.zeros(g.shape[0], bool)
    in_group[off[0]:off[-1]] = True
    n_nonempty = int(np.sum(np.diff(off) > 0))
    worst_a = worst_c = worst_d = 0.0
    for i in range(q.shape[0]):
        n = int(np.sum(idx[i] >= 0))
        assert n == min(k, n_nonempty), (name, i, n)
        assert np.all(idx[i, n:] == -1) and np.all(np.isneginf(score[i, n:])), (name, i)
        ii, ss = idx[i, :n], score[i, :n]
        assert not np.isnan(ss).any() and np.all((ii >= off[0]) & (ii < off[-1])), (name, i)
        assert np.all((ss[:-1] > ss[1:]) | ((ss[:-1] == ss[1:]) & (ii[:-1] < ii[1:]))), (name, i)
        grp = np.searchsorted(off, ii, side="right") - 1
        assert len(set(grp.tolist())) == n, (name, i)                      # distinct groups
        worst_a = max(worst_a, float((np.abs(ss.astype(np.float64) - s64[i, ii]) / b[i, ii]).max()))
        jk = ii[np.argmin(s64[i, ii])]
        left = in_group.copy()
        for gi in grp:
            left[off[gi]:off[gi + 1]] = False
        if left.any():
            worst_c = max(worst_c, float(((s64[i, left] - s64[i, jk]) / (b[i, left] + b[i, jk])).max()))
        for gi, j in zip(grp, ii):
            rows = np.arange(off[gi], off[gi + 1])
            worst_d = max(worst_d, float(((s64[i, rows] - s64[i, j]) / (b[i, rows] + b[i, j])).max()))
    print(f"{name}: (a) worst |score - s64| / b = {worst_a:.4f}; (c) worst (s64[row of a group left out] - s64[weakest kept]) / (b + b) = "
          f"{worst_c:.4f}; (d) worst (s64[row of a returned group] - s64[returned row]) / (b + b) = {worst_d:.4f}")
    assert worst_a <= 1.0, name
    assert worst_c <= 1.0, name
    assert worst_d <= 1.0, name


@pytest.mark.parametrize("nq,D", [(130, 512), (65, 64)])
def test_against_float64_random_rows(eng, nq, D):
    rng = np.random.default_rng(5900 + D)
    q = (rng.standard_normal((nq, D)) * rng.uniform(0.1, 30, (nq, 1))).astype(np.float32)
    layouts = {"clips": [150, 150, 37, 150, 1, 150, 62], "small": rng.integers(0, 6, 260).tolist()}
    for lname, sizes in layouts.items():
        n = int(np.sum(sizes))
        g = (rng.standard_normal((n, D)) * rng.uniform(0.1, 30, (n, 1))).astype(np.float32)
        walk = np.cumsum(rng.standard_normal((n, D)).astype(np.float32) * 0.05, axis=0) + g[:1]          # neighbouring frames nearly equal
        for gname, gal in (("random", g), ("smooth", walk.astype(np.float32))):
            off = offsets(sizes)
            for k in (10, 128):
                idx, score = gcall(eng, dev(q), dev(gal), off, k)
                check_fp64_grouped(f"{lname} {gname} nq={nq} D={D} k={k}", q, gal, off, idx, score, k)
            pad = offsets(sizes, first=3)
            pad = pad[pad <= n - 2]                                        # rows in front of the first and behind the last group
            idx, score = gcall(eng, dev(q), dev(gal), pad, 10)
            check_fp64_grouped(f"{lname} {gname} nq={nq} D={D} inner groups", q, gal, pad, idx, score, 10)


# ------------------------------------------------------------------------------------------------ 8. arguments
def test_bad_arguments_launch_nothing(eng):
    rng = np.random.default_rng(6000)
    q, g = dev(rng.standard_normal((70, 128))), dev(rng.standard_normal((90, 128)))
    off = [0, 30, 90]
    bad = [dict(qp=ctypes.c_void_p(None)), dict(gp=ctypes.c_void_p(None)), dict(null_idx=True), dict(null_score=True), dict(null_off=True),
           dict(k=0), dict(k=129), dict(k=-1), dict(D=0), dict(D=-64), dict(D=96), dict(n_queries=-1), dict(n_gallery=-1), dict(n_groups=-1),
           dict(gallery_offset=-1), dict(gallery_offset=INT32_MAX - 89), dict(gallery_offset=INT32_MAX),
           dict(qp=ctypes.c_void_p(q.data_ptr() + 4)), dict(gp=ctypes.c_void_p(g.data_ptr() + 8))]
    for kw in bad:
        kw = dict(kw)
        gcall(eng, q, g, off, kw.pop("k", 5), expect=JG_ERR_ARG, **kw)
    gcall(eng, q, g, off, 5, gallery_offset=INT32_MAX - 90)                  # the last offset that fits
    gcall(eng, q, g, off, 5, n_queries=0)                                    # JG_OK, nothing launched, nothing written
    idx, _ = gcall(eng, q, g, off, 5, n_queries=3)                           # fewer queries than rows: the others untouched (gcall)
    assert np.all(idx[:3, :2] >= 0) and np.all(idx[:3, 2:] == -1)


@pytest.mark.parametrize("k", [10, 128])
def test_hostile_offsets_stay_inside_the_buffers(eng, k):
    """offsets that are no partition: descending, beyond the gallery, negative, the int32 extremes.  The result is unspecified; the call
    returns JG_OK and the guards behind idx and score are intact (gcall asserts them) -- only that"""
    rng = np.random.default_rng(6100)
    q, g = dev(rng.standard_normal((65, 64))), dev(rng.standard_normal((300, 64)))
    big, small = 2 ** 31 - 1, -2 ** 31
    for off in ([300, 200, 100, 0], [0, 100, 50, 300], [0, 1000, 2000, 100000], [-50, 10, 5, 400], [0, big, small, big], [small, big],
                [big, small], [5, 5, 5, 5], rng.integers(-400, 700, 200).tolist(), rng.integers(small, big, 64).tolist()):
        gcall(eng, q, g, off, k)
        gcall(eng, q, g, off, k, gallery_offset=INT32_MAX - 300)


# ------------------------------------------------------------------------------------------------ 9. jg_group_of_rows
def test_group_of_rows_against_searchsorted(eng):
    rng = np.random.default_rng(6200)
    sizes = [0, 3, 1, 0, 0, 64, 7, 0, 150, 2, 0]
    for first, shift in ((0, 0), (5, 0), (5, 1000)):
        off = offsets(sizes, first)
        rows = np.concatenate([rng.integers(-3, off[-1] + 10, 500), off, off - 1, [-1, -1, -7]]).astype(np.int64)
        idx = np.where(rows < 0, rows, rows + shift).astype(np.int32)       # negative entries stay what they are: empty slots
        n = idx.size
        grp = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
        pos = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
        eng._bind_stream()
        assert eng.lib.jg_group_of_rows(eng.h, P(dev_i32(idx)), n, P(dev_i32(off)), len(off) - 1, shift, P(grp), P(pos)) == 0
        torch.cuda.synchronize()
        gh, ph = grp.cpu().numpy(), pos.cpu().numpy()
        assert np.all(gh[n:] == -7) and np.all(ph[n:] == -7), "guard overwritten"
        ok = (rows >= off[0]) & (rows < off[-1])
        want_g = np.where(ok, np.searchsorted(off, rows, side="right") - 1, -1)
        want_p = np.where(ok, rows - off[np.maximum(want_g, 0)], -1)
        assert np.array_equal(gh[:n], want_g) and np.array_equal(ph[:n], want_p), (first, shift)
        assert np.all(np.diff(off)[want_g[ok]] > 0)                          # never an empty group
        fg, fp = eng.group_of_rows(torch.from_numpy(idx[:300].reshape(100, 3)), off, shift)       # the Engine's form keeps the shape
        assert tuple(fg.shape) == (100, 3) and np.array_equal(fg.cpu().numpy().reshape(-1), want_g[:300]) and np.array_equal(fp.cpu().numpy().reshape(-1), want_p[:300])
    # arguments: nothing written
    idx, off = dev_i32([1, 2, 3]), dev_i32([0, 2, 4])
    grp = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    pos = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    for args in ((None, 3, P(off), 2, 0, P(grp), P(pos)), (P(idx), 3, None, 2, 0, P(grp), P(pos)), (P(idx), 3, P(off), 2, 0, None, P(pos)),
                 (P(idx), 3, P(off), 2, 0, P(grp), None), (P(idx), -1, P(off), 2, 0, P(grp), P(pos)), (P(idx), 3, P(off), -1, 0, P(grp), P(pos)),
                 (P(idx), 3, P(off), 2, -1, P(grp), P(pos))):
        assert eng.lib.jg_group_of_rows(eng.h, *args) == JG_ERR_ARG, args
    assert eng.lib.jg_group_of_rows(eng.h, P(idx), 0, P(off), 2, 0, P(grp), P(pos)) == 0
    torch.cuda.synchronize()
    assert bool((grp == -7).all()) and bool((pos == -7).all())
    assert eng.lib.jg_group_of_rows(eng.h, P(idx), 3, None, 0, 0, P(grp), P(pos)) == 0          # no group: every row is in none
    torch.cuda.synchronize()
    assert bool((grp == -1).all()) and bool((pos == -1).all())
    for hostile in ([4, 2, 0], [0, 2 ** 31 - 1, -2 ** 31]):                  # some group and position, nothing else
        assert eng.lib.jg_group_of_rows(eng.h, P(idx), 3, P(dev_i32(hostile)), 2, 0, P(grp), P(pos)) == 0
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 10. the front ends
@pytest.fixture(scope="module")
def corpus():
    """12 clips of 1..200 frames, D = 512, neighbouring frames nearly equal; three query rows: frame 131 of clip 7, frame 0 of clip 3, random"""
    rng = np.random.default_rng(6300)
    lens = [40, 150, 1, 64, 200, 13, 150, 170, 65, 128, 90, 7]
    clips = []
    for t in lens:
        c = np.cumsum(rng.standard_normal((t, 512)) * 0.3, axis=0) + rng.standard_normal(512)
        clips.append((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))
    q = np.stack([clips[7][131], clips[3][0], rng.standard_normal(512).astype(np.float32)])
    return q, clips


def test_engine_front_end(eng, corpus):
    q, clips = corpus
    g = np.concatenate(clips)
    off = offsets([len(c) for c in clips])
    want = gcall(eng, dev(q), dev(g), off, 5)
    idx, score = eng.sim_topk_grouped(torch.from_numpy(q), torch.from_numpy(g), off, 5)
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and tuple(idx.shape) == (3, 5)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(bits(score.cpu().numpy()), bits(want[1]))
    cut = int(off[5])
    part = eng.sim_topk_grouped(torch.from_numpy(q), torch.from_numpy(g[cut:]), torch.from_numpy(off[5:] - cut).cuda(), 5, gallery_offset=cut)
    both = eng.sim_topk_grouped(torch.from_numpy(q), torch.from_numpy(g[:cut]), off[:6], 5, merge_into=part)
    assert both[0] is part[0] and np.array_equal(both[0].cpu().numpy(), want[0]) and np.array_equal(bits(both[1].cpu().numpy()), bits(want[1]))
    none = eng.sim_topk_grouped(torch.from_numpy(q), torch.zeros(0, 512), [0], 4)
    assert bool((none[0] == -1).all()) and bool(torch.isneginf(none[1]).all())


def test_search_and_its_driver(eng, corpus, tmp_path, capsys):
    from jegal_amd import drivers, metrics as M
    q, clips = corpus
    clip, frame, score = M.search(q * 2.0, [c * 3.0 for c in clips], k=5, engine=eng)
    assert clip.dtype == np.int32 and frame.dtype == np.int32 and score.dtype == np.float32 and clip.shape == (3, 5)
    assert (clip[0, 0], frame[0, 0]) == (7, 131) and (clip[1, 0], frame[1, 0]) == (3, 0)      # the planted rows come back first
    assert np.allclose(score[:2, 0], 1.0, atol=1e-5)
    assert all(len(set(clip[i].tolist())) == 5 for i in range(3))
    # by its definition, in float64: every clip's best frame (ties aside: the corpus has none within 1e-5)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    best = np.stack([(qn.astype(np.float64) @ c.astype(np.float64).T).max(axis=1) for c in clips], 1)
    order = np.argsort(-best, axis=1)[:, :5]
    assert np.array_equal(clip, order) and np.allclose(score, np.take_along_axis(best, order, 1), atol=1e-5)
    for max_rows in (200, 400):                                                               # in pieces: the same bits
        got = M.search(q * 2.0, [c * 3.0 for c in clips], k=5, engine=eng, max_rows=max_rows)
        assert np.array_equal(got[0], clip) and np.array_equal(got[1], frame) and np.array_equal(bits(got[2]), bits(score))
    sclip, sframe, sscore = M.search(q * 2.0, [c * 3.0 for c in clips], k=20, segment=50, engine=eng)
    assert np.array_equal(sclip[:, 0], clip[:, 0]) and np.array_equal(sframe[:, 0], frame[:, 0]) and np.array_equal(bits(sscore[:, 0]), bits(score[:, 0]))
    runs = [set(zip(sclip[i].tolist(), (sframe[i] // 50).tolist())) for i in range(3)]
    assert all(len(r) == 20 for r in runs)                                                    # one entry per run of 50 frames
    assert any(np.sum(sclip[i] == sclip[i, 0]) > 1 for i in range(3))                         # a long clip with several moments
    pieces = M.search(q * 2.0, [c * 3.0 for c in clips], k=20, segment=50, engine=eng, max_rows=120)
    assert np.array_equal(pieces[0], sclip) and np.array_equal(pieces[1], sframe) and np.array_equal(bits(pieces[2]), bits(sscore))
    few = M.search(q, clips[:3], k=5, engine=eng)
    assert np.all(few[0][:, 3:] == -1) and np.all(few[1][:, 3:] == -1) and np.all(np.isneginf(few[2][:, 3:])) and np.all(few[0][:, :3] >= 0)
    # the driver
    src, res = tmp_path / "pkl", tmp_path / "res"
    src.mkdir()
    names = []
    for i, c in enumerate(clips):
        names.append(f"vid{i:03d}__t")
        with open(src / (names[-1] + ".pkl"), "wb") as f:
            pickle.dump({"gesture_emb": c, "content_emb": None, "info": {"fname": names[-1]}}, f)
    query = tmp_path / "query.pkl"
    with open(query, "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": q, "info": {"fname": "query", "word_boundaries": [["so", 0, 3], ["big", 4, 9], ["um", 10, 11]]}}, f)
    assert drivers.cmd_search(["--path", str(src), "--query", str(query), "--topk", "5", "--res_dir", str(res)], engine=eng) == 0
    z = np.load(res / "search_query.npz")
    assert list(z["names"]) == names and list(z["words"]) == ["so", "big", "um"]
    assert np.array_equal(z["clip"], clip) and np.array_equal(z["frame"], frame) and np.allclose(z["score"], score, atol=1e-6)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("search: \"")]
    assert len(lines) == 3 and "vid007__t@131" in lines[0] and "vid003__t@0" in lines[1]
    assert drivers.cmd_search(["--path", str(src), "--query", str(query), "--level", "phrase", "--topk", "3", "--segment", "50", "--res_dir", str(res)],
                              engine=eng) == 0
    z = np.load(res / "search_query.npz")
    want = M.search(q.mean(axis=0, keepdims=True), clips, k=3, segment=50, engine=eng)
    assert list(z["words"]) == ["so big um"] and np.array_equal(z["clip"], want[0]) and np.array_equal(z["frame"], want[1])
