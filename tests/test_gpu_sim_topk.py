"""jg_sim_topk through the C ABI (run with -m gpu): per query row the k gallery rows with the largest dot product, best first, ties to the
smaller gallery row; scores bit-identical to what jg_sim_rank compares; pieces of a gallery merged into the result of the whole.

Every call goes through `call`: idx / score are pre-filled with a -7 / NaN pattern (or with the list to merge into) and followed by a
guard of 64 elements that must come back untouched.

Float64 rule (check_fp64): b_ij = D * 2^-24 * sum_k |q_ik g_jk| bounds the error of a length-D fp32 fma chain (D roundings of at most
2^-24 relative each, of partial sums that are at most sum |q g| in magnitude: the standard bound, derived, not measured).  (a) a returned
score is within b of the float64 dot product of its pair; (b) the list is sorted by (score descending, index ascending) in its own fp32
values, its indices distinct and in range; (c) no row left out beats the weakest returned row (in float64) by more than the two bounds
together.  No case is left out of any of the three."""
import ctypes

import numpy as np
import pytest
import torch

from jegal_amd import synth

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC0BEEF      # a quiet NaN with a payload, as int32
GUARD = 64
JG_ERR_ARG = -1
INT32_MAX = 2 ** 31 - 1
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def dev(a):
    """host float32 rows -> device; an empty set still gets a (non-null) buffer"""
    a = np.ascontiguousarray(a, np.float32)
    t = torch.zeros((max(a.shape[0], 1), a.shape[1]), dtype=torch.float32, device="cuda")
    t[:a.shape[0]] = torch.from_numpy(a)
    return t


def call(eng, q, g, k, gallery_offset=0, merge=0, init=None, n_queries=None, n_gallery=None, D=None, expect=0, qp=None, gp=None,
         null_idx=False, null_score=False):
    """One jg_sim_topk call; q / g: device tensors (rows, D).  init = (idx, score) host arrays to start from (merge, or a hostile pattern).
    -> (idx (n,k) int32, score (n,k) float32) host arrays; asserts the return code and the guards; on an error or an empty call asserts that
    nothing at all was written."""
    nq = q.shape[0] if n_queries is None else n_queries
    ng = g.shape[0] if n_gallery is None else n_gallery
    rows, kraw, k = q.shape[0], k, max(k, 1)                            # (a bad k cannot size the outputs: one slot per row stands in)
    idx = torch.full((rows * k + GUARD,), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((rows * k + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    if init is not None:
        idx[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[0], np.int32).reshape(-1)).cuda()
        sc[:rows * k] = torch.from_numpy(np.ascontiguousarray(init[1], np.float32).reshape(-1).view(np.int32)).cuda()
    before_i, before_s = idx.cpu().numpy(), sc.cpu().numpy()
    eng._bind_stream()
    rc = eng.lib.jg_sim_topk(eng.h, P(q) if qp is None else qp, P(g) if gp is None else gp, nq, ng, q.shape[1] if D is None else D, kraw,
                             gallery_offset, merge, None if null_idx else P(idx), None if null_score else P(sc))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    ri, rs = idx.cpu().numpy(), sc.cpu().numpy()
    assert np.all(ri[rows * k:] == -7) and np.all(rs[rows * k:] == NAN_BITS), "guard overwritten"
    if expect != 0 or nq <= 0:
        assert np.array_equal(ri, before_i) and np.array_equal(rs, before_s), "an output was written"
    if 0 < nq < rows:                                                   # rows the call was not asked for
        assert np.array_equal(ri[nq * k:], before_i[nq * k:]) and np.array_equal(rs[nq * k:], before_s[nq * k:])
    return ri[:rows * k].reshape(rows, k), rs[:rows * k].view(np.float32).reshape(rows, k)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def expected_exact(s, k, offset=0):
    """s: (nq, ng) scores that fp32 holds exactly -> the list jg_sim_topk must return"""
    nq, ng = s.shape
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    idx = np.full((nq, k), -1, np.int32)
    sc = np.full((nq, k), -np.inf, np.float32)
    idx[:, :order.shape[1]] = order + offset
    sc[:, :order.shape[1]] = np.take_along_axis(s, order, axis=1)
    return idx, sc


def check_exact(eng, q, g, k, offset=0):
    s = (q.astype(np.int64) @ g.astype(np.int64).T).astype(np.float64) if g.shape[0] else np.zeros((q.shape[0], 0))
    idx, sc = call(eng, dev(q), dev(g), k, gallery_offset=offset, n_queries=q.shape[0], n_gallery=g.shape[0])
    want_i, want_s = expected_exact(s, k, offset)
    assert np.array_equal(idx, want_i), (q.shape, g.shape, k)
    assert np.array_equal(bits(sc), bits(want_s)), (q.shape, g.shape, k)


def check_sorted(idx, score, lo, hi):
    """(b): sorted by (score desc, idx asc) in the list's own values; indices distinct, inside lo .. hi - 1; empty slots (-1 / -inf) last"""
    for i in range(idx.shape[0]):
        n = int(np.sum(idx[i] >= 0))
        assert np.all(idx[i, n:] == -1) and np.all(np.isneginf(score[i, n:])), i
        ii, ss = idx[i, :n], score[i, :n]
        assert not np.isnan(ss).any() and np.all((ii >= lo) & (ii < hi)) and len(set(ii.tolist())) == n, i
        assert np.all((ss[:-1] > ss[1:]) | ((ss[:-1] == ss[1:]) & (ii[:-1] < ii[1:]))), i


def check_fp64(name, q, g, idx, score, k):
    """(a), (b), (c) of the module docstring for the list (idx, score) of queries q (n, D) against gallery g (m, D), host float32"""
    D = q.shape[1]
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    s64 = q64 @ g64.T
    b = D * 2.0 ** -24 * (np.abs(q64) @ np.abs(g64).T)
    check_sorted(idx, score, 0, g.shape[0])
    assert np.all(np.sum(idx >= 0, axis=1) == min(k, g.shape[0])), name
    worst_a = worst_c = 0.0
    for i in range(q.shape[0]):
        ii = idx[i][idx[i] >= 0]
        da = np.abs(score[i, :len(ii)].astype(np.float64) - s64[i, ii]) / b[i, ii]
        worst_a = max(worst_a, float(da.max()))
        jk = ii[np.argmin(s64[i, ii])]
        out = np.ones(g.shape[0], bool)
        out[ii] = False
        if out.any():
            worst_c = max(worst_c, float(((s64[i, out] - s64[i, jk]) / (b[i, out] + b[i, jk])).max()))
    print(f"{name}: (a) worst |score - s64| / b = {worst_a:.4f}; (c) worst (s64[left out] - s64[weakest kept]) / (b + b) = {worst_c:.4f}")
    assert worst_a <= 1.0, name
    assert worst_c <= 1.0, name


# ------------------------------------------------------------------------------------------------ shared inputs
@pytest.fixture(scope="module")
def planted(eng):
    """synth.planted_retrieval(1237, 1000), rows normalised on the engine as retrieval_metrics does, and a gallery copy with 40 duplicated
    rows: row 500 + 3 i repeats row 7 i, so query 7 i has two best rows with one score.  Host arrays."""
    ge, ce = synth.planted_retrieval(1237, 1000)
    g = eng.l2norm(torch.from_numpy(ge)).cpu().numpy()
    c = eng.l2norm(torch.from_numpy(ce)).cpu().numpy()
    gd = g.copy()
    dups = [(7 * i, 500 + 3 * i) for i in range(40)]
    for a, b in dups:
        gd[b] = gd[a]
    return {"g": g, "c": c, "gd": gd, "dups": dups}


def planted_inputs(p):
    return [("c2g", p["c"], p["g"]), ("g2c", p["g"], p["c"]), ("c2g_dup", p["c"], p["gd"])]


@pytest.fixture(scope="module")
def planted_single(eng, planted):
    """the single-call result for every planted input and k: what the sharded and the merged forms must reproduce"""
    return {(name, k): call(eng, dev(q), dev(g), k) for name, q, g in planted_inputs(planted) for k in (1, 10, 50, 128)}


# ------------------------------------------------------------------------------------------------ 1. exact selection
@pytest.mark.parametrize("k", [1, 2, 50, 64, 65, 128])
def test_exact_selection_on_integer_scores(eng, k):
    """entries in -2..2, D = 64: every dot product is an integer, exact in any order, and most pairs tie"""
    rng = np.random.default_rng(4100)
    q = rng.integers(-2, 3, (130, 64)).astype(np.float32)
    g = rng.integers(-2, 3, (1000, 64)).astype(np.float32)
    for nq in (1, 63, 64, 65, 130):
        for ng in (1, 63, 64, 65, 129, 1000):
            check_exact(eng, q[:nq], g[:ng], k)
    check_exact(eng, q[:65], g[:0], k)                                      # no gallery row: -1 / -inf
    check_exact(eng, q[:65], g[:129], k, offset=INT32_MAX - 129)            # the largest indices an int32 holds
    check_exact(eng, q[:65], np.repeat(g[:1], 200, axis=0), k)              # all gallery rows identical: idx 0 .. k-1
    check_exact(eng, np.abs(q[:65]) + 1, -np.abs(g[:129]) - 1, k)           # all scores negative
    z = np.zeros((65, 64), np.float32)
    z[1::2] = -0.0
    check_exact(eng, z, g[:129], k)                                         # rows of +-0 against mixed signs: every score ties at +0
    check_exact(eng, q[:65], np.concatenate([z[:40], g[:89]]), k)


# ------------------------------------------------------------------------------------------------ 2. adversarial order
@pytest.mark.parametrize("k", [10, 100])
def test_every_tile_flushes(eng, k):
    """a gallery whose similarity to the queries rises with the index: every entry of every tile beats the threshold; and its reverse"""
    rng = np.random.default_rng(4200)
    u = rng.standard_normal(128)
    u /= np.linalg.norm(u)
    q = (u + 0.05 * rng.standard_normal((3, 128))).astype(np.float32)
    g = (np.arange(1, 2001)[:, None] / 2000.0 * u).astype(np.float32)
    fi, fs = call(eng, dev(q), dev(g), k)
    ri, rs = call(eng, dev(q), dev(g[::-1]), k)
    check_fp64("ascending", q, g, fi, fs, k)
    check_fp64("descending", q, g[::-1], ri, rs, k)
    assert np.all(fi[:, 0] >= 2000 - 2 * k)                                 # (the best rows are the last ones)
    for i in range(3):                                                      # a row's score does not depend on where the row stands
        fwd = sorted(zip(fi[i].tolist(), bits(fs[i]).tolist()))
        rev = sorted(zip((1999 - ri[i]).tolist(), bits(rs[i]).tolist()))
        assert fwd == rev, i


# ------------------------------------------------------------------------------------------------ 3. consistency with jg_sim_rank
@pytest.mark.parametrize("k", [1, 10, 50])
def test_consistent_with_sim_rank(eng, planted, planted_single, k):
    for name, q, g in planted_inputs(planted):
        idx, score = planted_single[(name, k)]
        rank, ties = (t.cpu().numpy() for t in eng.sim_rank(torch.from_numpy(q), torch.from_numpy(g)))
        check_sorted(idx, score, 0, g.shape[0])
        for i in range(q.shape[0]):
            r, t = int(rank[i]), int(ties[i])
            pos = np.flatnonzero(idx[i] == i)
            if r + t <= k:
                assert len(pos) == 1, (name, i, r, t)
            if r >= k:
                assert len(pos) == 0, (name, i, r, t)
            if len(pos):
                p = int(pos[0])
                assert r <= p < r + t, (name, i, p, r, t)
                assert int(np.sum(score[i] > score[i, p])) == r, (name, i, p, r)
                assert int(np.sum(score[i] == score[i, p])) <= t
        if name == "c2g_dup" and k >= 2:
            seen = 0
            for a, b in planted["dups"]:                                    # equal rows: one score, the smaller row first
                for i in range(q.shape[0]):
                    pa, pb = np.flatnonzero(idx[i] == a), np.flatnonzero(idx[i] == b)
                    if len(pa) and len(pb):
                        seen += 1
                        assert bits(score[i, pa[0]]) == bits(score[i, pb[0]]) and pb[0] == pa[0] + 1, (i, a, b)
            assert seen >= 30          # (a planted partner sits 4.8 +- 1 sigma above the other rows: a handful of the 40 may miss a top 10)
        # query-sharded form: eight contiguous blocks against the full gallery
        per = -(-q.shape[0] // 8)
        gd = dev(g)
        parts = [call(eng, dev(q[r * per:(r + 1) * per]), gd, k) for r in range(8)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), idx)
        assert np.array_equal(bits(np.concatenate([p[1] for p in parts])), bits(score))


@pytest.mark.parametrize("D", [64, 192])
def test_rank_and_ties_follow_from_the_topk_bits(eng, D):
    """One tile loop serves both kernels: k = 128 returns every one of 100 scores per query, and jg_sim_rank's rank / ties are the counts
    of those very bits above / equal to the query's own (row_offset + i).  Two gallery tiles (the second partial), two query blocks (the
    second of one row), one (D = 64) and three (D = 192) k chunks; gallery rows 3 and 70 are equal, and each is some query's own row."""
    rng = np.random.default_rng(4350 + D)
    g = rng.standard_normal((100, D)).astype(np.float32)
    q = rng.standard_normal((65, D)).astype(np.float32)
    g[70] = g[3]
    qd, gd = dev(q), dev(g)
    idx, score = call(eng, qd, gd, 128)
    assert np.all(idx[:, 100:] == -1) and np.all(np.isneginf(score[:, 100:]))
    assert np.array_equal(np.sort(idx[:, :100], axis=1), np.tile(np.arange(100, dtype=np.int32), (65, 1)))
    s = np.empty((65, 100), np.float32)
    np.put_along_axis(s, idx[:, :100].astype(np.int64), score[:, :100], axis=1)
    assert np.array_equal(bits(s[:, 3]), bits(s[:, 70]))
    for row_offset in (0, 35):
        rank, ties = (t.cpu().numpy() for t in eng.sim_rank(qd, gd, row_offset=row_offset))
        own = s[np.arange(65), row_offset + np.arange(65)][:, None]
        want_rank, want_ties = np.sum(s > own, axis=1), np.sum(s == own, axis=1)
        assert want_ties[(3, 70)[row_offset > 0] - row_offset] >= 2           # (query 3 owns row 3, query 35 row 70: the equal pair)
        assert np.array_equal(rank, want_rank), (D, row_offset)
        assert np.array_equal(ties, want_ties), (D, row_offset)


# ------------------------------------------------------------------------------------------------ 4. float64
@pytest.mark.parametrize("k", [10, 128])
def test_against_float64_planted(planted, planted_single, k):
    for name, q, g in planted_inputs(planted):
        idx, score = planted_single[(name, k)]
        check_fp64(f"{name} k={k}", q, g, idx, score, k)


@pytest.mark.parametrize("D", [512, 576])
def test_against_float64_scaled_rows(eng, D):
    rng = np.random.default_rng(4400 + D)
    q = (rng.standard_normal((65, D)) * rng.uniform(0.1, 30, (65, 1))).astype(np.float32)
    g = (rng.standard_normal((129, D)) * rng.uniform(0.1, 30, (129, 1))).astype(np.float32)
    for k in (10, 128):
        idx, score = call(eng, dev(q), dev(g), k)
        check_fp64(f"scaled D={D} k={k}", q, g, idx, score, k)


# ------------------------------------------------------------------------------------------------ 5. merge
@pytest.mark.parametrize("k", [10, 128])
def test_merged_pieces_equal_the_single_call(eng, planted, planted_single, k):
    """the gallery in three unequal pieces (333, 70 and 597 rows: no multiple of the tile; the middle one holds fewer than 128 rows, so at
    k = 128 a list with empty slots is merged into), each with its gallery_offset, in two orders"""
    cuts = [(0, 333), (333, 403), (403, 1000)]
    for name, q, g in planted_inputs(planted):
        want_i, want_s = planted_single[(name, k)]
        qd = dev(q)
        pieces = [dev(g[a:b]) for a, b in cuts]
        for order, first_merge in (((0, 1, 2), 0), ((1, 2, 0), 0), ((2, 0, 1), 1)):
            # first_merge: the first piece merges into an explicitly empty list instead of writing over the pre-filled pattern
            cur = (np.full((q.shape[0], k), -1, np.int32), np.full((q.shape[0], k), -np.inf, np.float32)) if first_merge else None
            for n, pc in enumerate(order):
                cur = call(eng, qd, pieces[pc], k, gallery_offset=cuts[pc][0], merge=int(n > 0 or first_merge), init=cur)
            assert np.array_equal(cur[0], want_i), (name, order)
            assert np.array_equal(bits(cur[1]), bits(want_s)), (name, order)
    # merge = 0 never reads idx / score: a list that would win every comparison changes nothing
    name, q, g = planted_inputs(planted)[0]
    hostile = (np.tile(np.arange(k, dtype=np.int32), (q.shape[0], 1)), np.full((q.shape[0], k), np.inf, np.float32))
    got = call(eng, dev(q), dev(g), k, merge=0, init=hostile)
    assert np.array_equal(got[0], planted_single[(name, k)][0]) and np.array_equal(bits(got[1]), bits(planted_single[(name, k)][1]))


# ------------------------------------------------------------------------------------------------ 6. determinism and arguments
def test_two_runs_give_the_same_bits(eng, planted, planted_single):
    for name, q, g in planted_inputs(planted):
        for k in (10, 128):
            idx, score = call(eng, dev(q), dev(g), k)
            assert np.array_equal(idx, planted_single[(name, k)][0]) and np.array_equal(bits(score), bits(planted_single[(name, k)][1]))


def test_bad_arguments_launch_nothing(eng):
    rng = np.random.default_rng(4600)
    q, g = dev(rng.standard_normal((70, 128))), dev(rng.standard_normal((90, 128)))
    bad = [dict(qp=ctypes.c_void_p(None)), dict(gp=ctypes.c_void_p(None)), dict(null_idx=True), dict(null_score=True),
           dict(k=0), dict(k=129), dict(k=-1), dict(D=0), dict(D=-64), dict(D=96), dict(n_queries=-1), dict(n_gallery=-1),
           dict(gallery_offset=-1), dict(gallery_offset=INT32_MAX - 89), dict(gallery_offset=INT32_MAX),
           dict(qp=ctypes.c_void_p(q.data_ptr() + 4)), dict(gp=ctypes.c_void_p(g.data_ptr() + 8))]
    for kw in bad:
        kw = dict(kw)
        call(eng, q, g, kw.pop("k", 5), expect=JG_ERR_ARG, **kw)
    call(eng, q, g, 5, gallery_offset=INT32_MAX - 90)                       # the last offset that fits
    call(eng, q, g, 5, n_queries=0)                                         # JG_OK, nothing launched, nothing written
    idx, score = call(eng, q, g, 5, n_gallery=0)
    assert np.all(idx == -1) and np.all(np.isneginf(score))


def test_engine_and_metrics_front_ends(eng, planted, planted_single):
    """Engine.sim_topk (with merge_into) and metrics.retrieve give the C entry's result"""
    from jegal_amd import metrics as M
    q, g = planted["c"], planted["g"]
    want_i, want_s = planted_single[("c2g", 10)]
    idx, score = eng.sim_topk(torch.from_numpy(q), torch.from_numpy(g), 10)
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and tuple(idx.shape) == (1000, 10)
    assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(bits(score.cpu().numpy()), bits(want_s))
    part = eng.sim_topk(torch.from_numpy(q), torch.from_numpy(g[600:]), 10, gallery_offset=600)
    both = eng.sim_topk(torch.from_numpy(q), torch.from_numpy(g[:600]), 10, merge_into=part)
    assert both[0] is part[0] and np.array_equal(both[0].cpu().numpy(), want_i) and np.array_equal(bits(both[1].cpu().numpy()), bits(want_s))
    none = eng.sim_topk(torch.from_numpy(q[:3]), torch.zeros(0, 512), 4)
    assert bool((none[0] == -1).all()) and bool(torch.isneginf(none[1]).all())
    ri, rs = M.retrieve(q * 3.0, g * 0.5, k=10, engine=eng)                  # un-normalised means in, the same neighbours out
    assert ri.dtype == np.int32 and rs.dtype == np.float32 and ri.shape == (1000, 10)
    assert np.mean(ri == want_i) > 0.99 and np.allclose(rs, want_s, atol=1e-6)
