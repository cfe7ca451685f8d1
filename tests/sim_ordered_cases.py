"""The contracts of jg_sim_ordered and jg_sim_align restated with numpy, shared by tests/test_sim_ordered_cpu.py and
tests/test_gpu_sim_ordered.py.

From a dense float32 s (n_words, n_gallery) of word-frame products, -0.0 as +0.0, NaN = no value; a query owns the word rows w_1 .. w_W,
a group the gallery rows [a, b) clamped to 0 .. n_gallery, t counts from a, T = b - a:
    M_0(t) = +0.0;  E_i(t) = M_(i-1)(t) + s(w_i, t) (one float32 add);  M_i(t) = fmax over t' <= t of E_i(t') (NaN: none)
    score(q, g) = M_W(T - 1) / float32(W); none (NaN) when M_W(T - 1) is NaN or T == 0.
Alignment, ordered: t_W = the first arg-max of E_W over [0, T), t_i = the first arg-max of E_i over [0, t_(i+1)].  Unordered: E_i = s(w_i, .),
every word searches [0, T), and the score is the M_i(T - 1) added in word order / W: jg_sim_coupling's."""
import itertools

import numpy as np

from sim_coupling_cases import coupling_expected, coupling_scores


def _clean(s):
    return np.asarray(s, np.float32) + np.float32(0.0)                   # -0.0 + 0.0 = +0.0


def _range(g_off, g, n_gallery):
    return int(max(g_off[g], 0)), int(min(g_off[g + 1], n_gallery))


def ordered_tables(s, a, b, ordered=True):
    """the E_i of one (query rows of s, group [a, b)) pair -> (W, T) float32"""
    E = np.empty((s.shape[0], b - a), np.float32)
    M = np.zeros(b - a, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(s.shape[0]):
            E[i] = (M if ordered else np.float32(0.0)) + s[i, a:b]
            M = np.fmax.accumulate(E[i])                                # skips a NaN; none so far: NaN
    return E


def ordered_scores(s, w_off, g_off):
    """-> (n_queries, n_groups) float32, NaN where the pair has no score"""
    s = _clean(s)
    w_off, g_off = np.asarray(w_off, np.int64), np.asarray(g_off, np.int64)
    out = np.full((len(w_off) - 1, len(g_off) - 1), np.nan, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(len(g_off) - 1):
            a, b = _range(g_off, g, s.shape[1])
            if b <= a:
                continue
            for q, (w0, w1) in enumerate(zip(w_off[:-1], w_off[1:])):
                M = np.zeros(b - a, np.float32)
                for w in range(int(w0), int(w1)):
                    E = M + s[w, a:b]
                    M = np.fmax.accumulate(E)
                out[q, g] = M[-1] / np.float32(w1 - w0)
    assert out.dtype == np.float32
    return out


def ordered_expected(s, w_off, g_off, k, group_offset=0, init=None):
    """-> (idx (nq, k) int32 = group_offset + g, score (nq, k) float32, pair (n_groups, nq) float32) by coupling_expected's selection rule:
    that function is handed the ordered scores as a matrix of one-word queries against one-row groups, whose coupling score is the entry
    itself (0 + x and x / 1 are exact, a NaN stays "no score")"""
    sc = ordered_scores(s, w_off, g_off)
    return coupling_expected(sc, np.arange(sc.shape[0] + 1), np.arange(sc.shape[1] + 1), k, group_offset, init)


def align_expected(s, w_off, g_off, idx, ordered, group_offset=0, frames=None, score=None, max_rows=8192):
    """-> (frames (nq, k, Wmax) int32, score (nq, k) float32): local gallery rows a + t_i, -1 behind W; slots whose idx is not one of
    group_offset .. group_offset + n_groups - 1 keep what frames / score held (default: -1 / NaN)"""
    s = _clean(s)
    w_off, g_off = np.asarray(w_off, np.int64), np.asarray(g_off, np.int64)
    nq, k = idx.shape
    wmax = int(np.diff(w_off).max()) if nq else 1
    frames = np.full((nq, k, wmax), -1, np.int32) if frames is None else frames.copy()
    score = np.full((nq, k), np.nan, np.float32) if score is None else score.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(nq):
            w0, w1 = int(w_off[q]), int(w_off[q + 1])
            for r in range(k):
                g = int(idx[q, r]) - group_offset
                if idx[q, r] < 0 or not 0 <= g < len(g_off) - 1:
                    continue
                frames[q, r], score[q, r] = -1, np.nan
                a, b = _range(g_off, g, s.shape[1])
                if b <= a or b - a > max_rows:
                    continue
                E = ordered_tables(s[w0:w1], a, b, ordered)
                if np.isnan(E).all(axis=1).any() or (ordered and np.isnan(E[-1]).all()):
                    continue
                limit, ts = b - a - 1, []
                for i in range(w1 - w0 - 1, -1, -1):
                    t = int(np.nanargmax(E[i, :limit + 1]))             # the first arg-max, NaN skipped
                    ts.append(t)
                    if ordered:
                        limit = t
                ts = ts[::-1]
                frames[q, r, :w1 - w0] = a + np.asarray(ts)
                if ordered:
                    score[q, r] = E[-1, ts[-1]] / np.float32(w1 - w0)
                else:
                    acc = np.float32(0.0)
                    for i, t in enumerate(ts):
                        acc = np.float32(acc + E[i, t])
                    score[q, r] = acc / np.float32(w1 - w0)
    return frames, score


def brute_force_ordered(s, a, b):
    """float64 over every non-decreasing assignment of the rows of s to the columns [a, b): (best mean or NaN, the first best assignment in
    the backtrack's order -- the last word as early as possible, then the word before it, ...).  Tiny sizes only."""
    s = np.asarray(s, np.float64)
    W, T = s.shape[0], b - a
    best, best_ts = np.nan, None
    for ts in itertools.combinations_with_replacement(range(T), W):
        v = sum(s[i, a + t] for i, t in enumerate(ts))
        if np.isnan(v):
            continue
        key = tuple(reversed(ts))
        if best_ts is None or v > best or (v == best and key < tuple(reversed(best_ts))):
            best, best_ts = v, ts
    return (best / W if best_ts is not None else np.nan), best_ts


def first_argmax_in_order(s, w_off, g_off):
    """(n_queries, n_groups) bool: every word has a value and the words' first arg-max frames are non-decreasing"""
    s = _clean(s)
    out = np.zeros((len(w_off) - 1, len(g_off) - 1), bool)
    for g in range(len(g_off) - 1):
        a, b = _range(g_off, g, s.shape[1])
        if b <= a:
            continue
        for q in range(len(w_off) - 1):
            rows = s[int(w_off[q]):int(w_off[q + 1]), a:b]
            if np.isnan(rows).all(axis=1).any():
                continue
            out[q, g] = bool(np.all(np.diff(np.nanargmax(rows, axis=1)) >= 0))
    return out


__all__ = ["ordered_scores", "ordered_expected", "align_expected", "brute_force_ordered", "first_argmax_in_order", "coupling_scores", "coupling_expected"]
