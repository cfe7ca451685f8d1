"""The contract of jg_sim_coupling restated with numpy, shared by tests/test_sim_coupling_cpu.py and tests/test_gpu_sim_coupling.py.

From a dense float32 s (n_words, n_gallery) of word-frame products: -0.0 counts as +0.0, a NaN is skipped, m(w, g) = the max over the rows
of group g (none: NaN), score(q, g) = the m(w, g) of q's words added in float32 in ascending word order, one chain, divided by float32(W_q)
in float32; no score (NaN) if any word has no m.  Per query the k best groups by (score descending, group ascending)."""
import numpy as np


def coupling_scores(s, w_off, g_off):
    """-> (n_queries, n_groups) float32, NaN where the pair has no score"""
    s = np.asarray(s, np.float32) + np.float32(0.0)                     # -0.0 + 0.0 = +0.0
    w_off, g_off = np.asarray(w_off, np.int64), np.asarray(g_off, np.int64)
    n_words, n_gallery = s.shape
    m = np.full((n_words, len(g_off) - 1), np.nan, np.float32)
    for g, (a, b) in enumerate(zip(g_off[:-1], g_off[1:])):
        a, b = int(max(a, 0)), int(min(b, n_gallery))
        if b > a:
            m[:, g] = np.fmax.reduce(s[:, a:b], axis=1)                 # fmax skips a NaN; all NaN: NaN
    out = np.full((len(w_off) - 1, m.shape[1]), np.nan, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q, (w0, w1) in enumerate(zip(w_off[:-1], w_off[1:])):
            acc = np.zeros(m.shape[1], np.float32)
            for w in range(int(w0), int(w1)):                           # one float32 chain per group, in word order (a NaN stays)
                acc = acc + m[w]
            out[q] = acc / np.float32(w1 - w0)
    assert out.dtype == np.float32
    return out


def coupling_expected(s, w_off, g_off, k, group_offset=0, init=None):
    """-> (idx (nq, k) int32 = group_offset + g, score (nq, k) float32, pair (n_groups, nq) float32: NaN where there is no score).
    init = (idx, score) of an earlier call on other groups, merged in."""
    sc = coupling_scores(s, w_off, g_off)
    nq, ng = sc.shape
    idx = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        ok = ~np.isnan(sc[q])
        grp = (group_offset + np.nonzero(ok)[0]).astype(np.int64)
        val = sc[q][ok] + np.float32(0.0)
        if init is not None:
            keep = init[0][q] >= 0
            grp = np.concatenate([grp, init[0][q][keep].astype(np.int64)])
            val = np.concatenate([val, init[1][q][keep].astype(np.float32)])
        order = np.lexsort((grp, -val.astype(np.float64)))[:k]          # stable: the larger score, then the smaller group
        idx[q, :len(order)] = grp[order]
        out[q, :len(order)] = val[order]
    return idx, out, np.ascontiguousarray(sc.T)


def brute_force_scores(words, gallery, w_off, g_off):
    """the definition in float64, straight from the operands: exact wherever every product and sum is -> (n_queries, n_groups)"""
    s = np.asarray(words, np.float64) @ np.asarray(gallery, np.float64).T
    out = np.full((len(w_off) - 1, len(g_off) - 1), np.nan)
    for q in range(len(w_off) - 1):
        for g in range(len(g_off) - 1):
            a, b = int(g_off[g]), int(g_off[g + 1])
            best = []
            for w in range(int(w_off[q]), int(w_off[q + 1])):
                row = s[w, a:b]
                row = row[~np.isnan(row)]
                best.append(row.max() if row.size else np.nan)
            out[q, g] = np.mean(best) if not np.isnan(best).any() else np.nan
    return out


def plan_expected(w_off):
    """The packing rule: queries in order into tiles of at most 64 word rows, never split -> tile_first_query (n_tiles + 1 entries)"""
    first, used = [], 64
    for q in range(len(w_off) - 1):
        W = int(w_off[q + 1]) - int(w_off[q])
        assert 1 <= W <= 64
        if used + W > 64:
            first.append(q)
            used = 0
        used += W
    return first + [len(w_off) - 1]


def offsets_of_counts(counts, first=0):
    return np.concatenate([[first], first + np.cumsum(counts)]).astype(np.int64)
