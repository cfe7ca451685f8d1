"""Inputs and references of the talk heat map (jg_attn_talk), shared by tests/test_attn_talk_cases_cpu.py, tests/test_attn_talk_cpu.py and
tests/test_gpu_attn_talk.py: the planted track, a float64 evaluation of the definition (include/jegal_hip.h, jg_attn_talk), its fp32 twin
(the same formula in torch fp32: the yardstick of the error rule), and the derived outputs (band, per-word and per-frame arg-max).

Definition: word w is IN REACH of frame f iff start_w - reach <= f <= end_w + reach;
P[w][f] = exp(x_wf - m_f) / sum over the words in reach of f of exp(x_w'f - m_f), x = <c_w, g_f> / temp, m_f the maximum over those words.
Matrices here are dense (W, T) with NaN where the word is not in reach of the frame."""
import numpy as np
import torch

TEMP = 0.07
FRAME_BLOCK = 128        # TALK_FB of jegal_amd/csrc/spotting.hip
MAX_BLOCK_W = 128        # TALK_MAX_BLOCK_W of jegal_amd/csrc/shared.h

# The inputs of the GPU accuracy tests: (seed, T, W, span, gap, reach, D).  Both normalize modes run on each; test_attn_talk_cases_cpu.py
# asserts that each has at least 90 % decidable words and frames (the seeds of the small case were taken for that: its words' best
# frames sit near probability 1, where two frames of a word can come within 1e-3 of each other).
ACCURACY_INPUTS = [(20, 700, 140, 4, 1, 40, 512), (21, 1000, 400, 2, 1, 25, 512), (30, 135, 20, 5, 2, 12, 64), (37, 135, 20, 5, 2, 12, 192)]


def planted_talk(seed, T, W, span, gap, d=512):
    """Unit content rows and N(0, 1/d) frame rows; word j sits on frames j (span + gap) .. + span - 1 (cut at T; a word that starts
    beyond T has no frame), and each of its frames gets a_f c_j added, a_f ~ U(0.15, 0.55): the softmax stays unsaturated and the
    frames of a word differ.  -> (g (T, d) float32, c (W, d) float32, start (W,), end (W,) int64)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((W, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    g = rng.standard_normal((T, d)) / np.sqrt(d)
    start = np.arange(W, dtype=np.int64) * (span + gap)
    end = start + span - 1
    for j in range(W):
        lo, hi = int(start[j]), int(min(end[j], T - 1))
        if lo <= hi:
            g[lo:hi + 1] += rng.uniform(0.15, 0.55, (hi - lo + 1, 1)) * c[j][None]
    return g.astype(np.float32), c.astype(np.float32), start, end


def reach_mask(T, start, end, reach):
    """(W, T) bool: word w in reach of frame f"""
    f = np.arange(T, dtype=np.int64)[None]
    return (np.asarray(start, np.int64)[:, None] - reach <= f) & (f <= np.asarray(end, np.int64)[:, None] + reach)


def talk64(g, c, start, end, reach, normalize, temp=TEMP):
    """the definition in float64 -> (W, T), NaN outside the reach"""
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    if normalize:
        g = g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
        c = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)
    m = reach_mask(g.shape[0], start, end, reach).T                  # (T, W): the softmax runs along the words, as in the clip form
    x = np.where(m, g @ c.T / temp, -np.inf)
    with np.errstate(invalid="ignore"):
        e = np.where(m, np.exp(x - x.max(axis=1, keepdims=True)), 0.0)
        p = e / e.sum(axis=1, keepdims=True)
    return np.where(m, p, np.nan).T


def talk32(g, c, start, end, reach, normalize, temp=TEMP):
    """the fp32 twin: the same formula as torch evaluates it in float32 (F.normalize, mm, masked softmax over the words)"""
    gt, ct = torch.from_numpy(np.asarray(g, np.float32)), torch.from_numpy(np.asarray(c, np.float32))
    if normalize:
        gt, ct = torch.nn.functional.normalize(gt, dim=1), torch.nn.functional.normalize(ct, dim=1)
    m = torch.from_numpy(reach_mask(gt.shape[0], start, end, reach).T.copy())        # (T, W)
    x = (torch.mm(gt, ct.t()) / temp).masked_fill(~m, float("-inf"))
    p = torch.softmax(x, dim=1)                                                      # a frame without a word: NaN row
    return np.where(m.numpy(), p.numpy(), np.float32(np.nan)).T


def band_of(P, start, reach, pitch):
    """(W, T) -> the band layout (W, pitch): band[w][j] = P[w][start_w - reach + j], NaN outside 0..T-1"""
    W, T = P.shape
    out = np.full((W, pitch), np.nan, P.dtype)
    for w in range(W):
        f0 = int(start[w]) - reach
        lo, hi = max(f0, 0), min(f0 + pitch, T)
        if lo < hi:
            out[w, lo - f0:hi - f0] = P[w, lo:hi]
    return out


def band_pitch(start, end, reach):
    return 2 * reach + int((np.asarray(end) - np.asarray(start)).max()) + 1


def word_best(P):
    """per word: (first arg-max frame over its non-NaN frames, that value); -1 / NaN when it has none"""
    has = ~np.isnan(P).all(axis=1)
    q = np.where(np.isnan(P), -np.inf, P)
    f = np.where(has, q.argmax(axis=1), -1).astype(np.int32)
    return f, np.where(has, q.max(axis=1), np.nan)


def frame_best(P):
    """per frame: (arg-max word, the smaller index on ties, that value); -1 / NaN when no word is in reach"""
    f, s = word_best(P.T)
    return f, s


def decidable(P, axis):
    """bool per word (axis=1) or per frame (axis=0) that has an entry: the float64 best beats the runner-up by more than 1e-3 relative
    (an only entry is decidable); and the mask of those that have an entry"""
    q = np.where(np.isnan(P), -np.inf, P)
    q = q if axis == 1 else q.T
    has = np.isfinite(q).any(axis=1)
    srt = np.sort(q, axis=1)
    best, second = srt[:, -1], (srt[:, -2] if q.shape[1] > 1 else np.full(q.shape[0], -np.inf))
    with np.errstate(invalid="ignore"):
        return has & (best - second > 1e-3 * best), has


def err(X, P64):
    """distance of X from the float64 matrix over the entries in reach: (max-abs, max relative error over entries >= 1e-3)"""
    m = ~np.isnan(P64)
    d = np.abs(np.asarray(X, np.float64)[m] - P64[m])
    big = P64[m] >= 1e-3
    return float(d.max()) if d.size else 0.0, float((d[big] / P64[m][big]).max()) if big.any() else 0.0


def block_candidates(T, start, end, reach):
    """words in reach of any frame of each block of FRAME_BLOCK frames, counted from the definition (not from a search)"""
    m = reach_mask(T, start, end, reach)
    return np.array([int(m[:, f0:f0 + FRAME_BLOCK].any(axis=1).sum()) for f0 in range(0, T, FRAME_BLOCK)], np.int64)
