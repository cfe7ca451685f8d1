"""Cases, float64 references and derived bounds for the first-generation metric entries jg_sim_rank, jg_spot and jg_asd (jegal_amd/csrc/retrieval.hip, spotting.hip, asd.hip).

Imports without a GPU: tests/test_gpu_metrics_fp64.py feeds the cases to the public C ABI, tests/test_metrics_cases_cpu.py feeds them to plain
float32 numpy statements of the kernels' arithmetic and to planted defects, so that references, bounds and margin conditions are checked
where no GPU is.  Every generator is seeded by its parameters and returns float32 arrays holding exactly the values the kernel receives.

u = 2^-24.  The bounds are derived from the arithmetic the kernels are documented to do, never from what a kernel returned:

sim_rank, exact.  Entries are integers in [-3, 3]: a dot product over D <= 1024 is an integer of magnitude <= 9 * 1024 < 2^24, so every partial
    sum in whatever order is exact in fp32 and rank / ties must EQUAL the int64 counts.

sim_rank, float.  An fp32 dot product of D terms, in any order and with or without fused multiply-adds, errs by at most
    b_ij = (D + 2) u sum_d |q_d g_d|   (D products, D - 1 additions, first order; + 2 covers the second-order terms for D <= 1024).
    s_ij > d_i as the kernel sees it is certain when s64_ij > d64_i + b_ij + b_ii and impossible when s64_ij < d64_i - b_ij - b_ii, so
        #{s64_ij > d64_i + b_ij + b_ii} <= rank_i <= rank_i + ties_i <= #{s64_ij >= d64_i - b_ij - b_ii}
    with nothing left out.  A score depends on its two rows alone, so bit-identical copies of the partner row tie exactly: ties_i >= 1 + copies.

spot.  p = softmax_w(<g^_t, c^_w> / temp)[target], g^ = g / max(|g|, 1e-12).  Logit error, in units of u / temp and relative to sum_d |g^_d c^_d| <= 1
    (Cauchy-Schwarz on unit rows):
        the D-term dot product in any order                                                          D - 1
        three roundings per product (g_d gn, c_d cn, their product)                                  3
        the two reciprocal norms: a sum of squares is formed per lane (<= 16 terms for D <= 1024) and by a 6-step butterfly, so it is
        off by <= (16 + 6 + 1) u relatively, its square root by half of that + 1, the reciprocal by 1 more: (11.5 + 2) u each           27
        the division by temp and the subtraction of the row maximum (|L - max| <= 2 / temp)                                              3
    => |dL| <= (D + 32) u / temp: c1 = 32.  A logit error d moves exp(L_w - max) by a factor e^d in the numerator and, at most, in every term
    of the denominator: 2 (D + c1) u / temp relative to p.  The softmax itself: expf to 2 ulp in the numerator and in each of the W terms, their
    sum (W - 1 additions, any order) and the division: (W + 4) u, c2 = 4.  So
        |score - p64| <= SPOT_BOUND(D, W) p64 = (2 (D + 32) u / temp + (W + 4) u) p64.
    pred is exact because the generator ASSERTS, for every clip, that the float64 winner beats every frame that is not a bit-identical copy of it
    by more than twice that bound (relative to the winner's probability); bit-identical frames give bit-equal probabilities (a frame's
    probability depends on its row and the clip's words alone), and among them the first wins.  With W = 1 the softmax is exp(0) / exp(0): every
    probability is 1.0 exactly whatever the logit, all frames tie, pred = 0 and score = 1.0 -- exact by construction, no margin is involved.

asd.  cos = <q, c> / max(|q| |c|, 1e-8).  With the same accounting (dot D - 1, product rounding 1, two norms at (11.5 + 1) u each, their product,
    the division, the division by temp, and 4 u for the softmax's exp / sum / division keeping strictly ordered values apart) a cosine is off by
    at most (D + 32) u.  The generator asserts for EVERY query and each of the three candidate counts that the float64 winner's cosine exceeds that of
    every candidate that is not a bit-identical copy of it by more than ASD_MARGIN(D) = 2 (D + 32) u; then the arg-max is determined, copies
    tie bit for bit and the first wins.
"""
import numpy as np

from test_gpu_kernels_fp64 import U

TEMP = float(np.float32(0.07))          # what the C ABI's float receives


def rng(*seed):
    """A generator seeded by the case's parameters, mixed arithmetically (the same cases under every interpreter)."""
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v) + 12345) % 2147483647
    return np.random.default_rng(s)


def offsets(lengths):
    off = np.zeros(len(lengths) + 1, np.int32)
    off[1:] = np.cumsum(lengths)
    return off


# ============================================================================================================================== sim_rank
RANK_EXACT_SHAPES = [(1, 1, 0, 64), (1, 65, 64, 64), (63, 64, 1, 128), (64, 64, 0, 64), (65, 130, 65, 512), (5, 200, 195, 1024), (130, 130, 0, 64)]
RANK_FLOAT_SHAPE = (70, 150, 40, 512)          # (n_local, n_total, row_offset, D)


def rank_exact_case(n_local, n_total, row_offset, D):
    """Integer rows in [-3, 3]; from 5 queries on, query 2 is all zeros (zero_query); from 5 gallery rows on, one gallery row is zero and up to
    three partner rows are copied over other gallery rows (the last row among them: the last tile's last valid column)."""
    r = rng(11, n_local, n_total, row_offset, D)
    e1 = r.integers(-3, 4, (n_local, D)).astype(np.float32)
    e2 = r.integers(-3, 4, (n_total, D)).astype(np.float32)
    zero_query = None
    if n_local >= 5:
        zero_query = 2
        e1[2] = 0
    if n_total >= 5:
        partners = set(range(row_offset, row_offset + n_local))
        free = [j for j in range(n_total) if j not in partners] or [j for j in range(n_total) if j != row_offset]
        e2[free[len(free) // 2]] = 0
        for k, i in enumerate(sorted({0, n_local // 2, n_local - 1})):
            dst = n_total - 1 if k == 0 else free[(7 * k + 1) % len(free)]
            if dst != row_offset + i:          # (a row that is another query's partner may be overwritten: the counts are taken afterwards)
                e2[dst] = e2[row_offset + i]
    s = e1.astype(np.int64) @ e2.astype(np.int64).T
    assert int(np.abs(s).max(initial=0)) < 2 ** 24
    rank, ties = rank_counts(s, row_offset)
    if zero_query is not None:
        assert rank[zero_query] == 0 and ties[zero_query] == n_total
    return dict(e1=e1, e2=e2, rank=rank, ties=ties, zero_query=zero_query, s=s)


def rank_counts(s, row_offset, gt=np.greater, diag_at_i=False, count_self=True, pad_to=None):
    """rank / ties from a score matrix (n_local, n_total).  The keyword arguments are the planted defects of the CPU test: another comparison,
    the diagonal taken at column i, ties without the partner itself, and the gallery padded with zero-score columns up to a multiple of pad_to
    (a last tile whose column guard is missing)."""
    n = s.shape[0]
    cols = np.arange(n) + (0 if diag_at_i else row_offset)
    d = s[np.arange(n), np.minimum(cols, s.shape[1] - 1)][:, None]
    if pad_to:
        s = np.concatenate([s, np.zeros((n, -s.shape[1] % pad_to), s.dtype)], axis=1)
    rank = gt(s, d).sum(1).astype(np.int64)
    ties = (s == d).sum(1).astype(np.int64) - (0 if count_self else 1)
    return rank, ties


def rank_float_case():
    n_local, n_total, row_offset, D = RANK_FLOAT_SHAPE
    r = rng(12, n_local, n_total, row_offset, D)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    e1, e2 = unit(r.standard_normal((n_local, D))), unit(r.standard_normal((n_total, D)))
    copies = np.zeros(n_local, np.int64)
    for i, dst in ((3, 0), (3, 149), (31, 127), (69, 128)):          # query 3's partner twice, in the first and in the last tile
        e2[dst] = e2[row_offset + i]
        copies[i] += 1
    q, g = e1.astype(np.float64), e2.astype(np.float64)
    s = q @ g.T
    b = (D + 2) * U * (np.abs(q) @ np.abs(g).T)
    idx = np.arange(n_local)
    d, bd = s[idx, row_offset + idx][:, None], b[idx, row_offset + idx][:, None]
    lo = (s > d + b + bd).sum(1)
    hi = (s >= d - b - bd).sum(1)
    assert bool((hi >= lo + 1 + copies).all())
    return dict(e1=e1, e2=e2, lo=lo, hi=hi, copies=copies)


def rank_interval_fails(c, rank, ties):
    """The float case's assertions on a (rank, ties) pair -> list of failures; observed / bound is not a ratio here but a containment."""
    rank, ties = np.asarray(rank, np.int64), np.asarray(ties, np.int64)
    bad = []
    for i in range(len(rank)):
        if not c["lo"][i] <= rank[i] <= c["hi"][i]:
            bad.append(f"query {i}: rank {rank[i]} outside [{c['lo'][i]}, {c['hi'][i]}]")
        if rank[i] + ties[i] > c["hi"][i]:
            bad.append(f"query {i}: rank + ties {rank[i] + ties[i]} > {c['hi'][i]}")
        if ties[i] < 1 + c["copies"][i]:
            bad.append(f"query {i}: ties {ties[i]} < 1 + {c['copies'][i]} copies")
    return bad


# ================================================================================================================================== spot
SPOT_C1, SPOT_C2 = 32, 4
SPOT_SHAPES = [(1, 1, 64), (5, 3, 1), (67, 65, 100), (130, 5, 1024), (9, 1024, 128), (8192, 1, 64), (8192, 2, 64)]          # (T, W, D)
TIE_STEPS = (1, 3, 64, 65)          # copies of the winner at t + 1, t + 3 (another wave), t + 64, t + 65 (another pass of the lane scan), and last


def spot_bound(D, W, temp=TEMP):
    return 2 * (D + SPOT_C1) * U / temp + (W + SPOT_C2) * U


def spot_ref(g, c, target, temp=TEMP):
    """float64 probabilities of column `target` for every frame."""
    g, c = g.astype(np.float64), c.astype(np.float64)
    gn = g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
    cn = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)
    L = np.stack([(gn * cn[w][None]).sum(1) for w in range(len(cn))], axis=1) / temp          # row-wise: equal rows give equal bits
    L -= L.max(1, keepdims=True)
    P = np.exp(L)
    return P[:, target] / P.sum(1)


def spot_clip(T, W, D, target, winner=None, seed=0, zero_rows=False, copies=()):
    """One clip.  Frames lean away from the target word (so that no ordinary frame's probability saturates near the winner's, whatever T), the
    frame `winner` leans towards it.  D = 1: unit rows are +-1, so the signs are set instead: the winner alone agrees with the target word, which
    alone has its sign.  zero_rows: a zero gesture row and a zero (non-target) content row.  copies: frames overwritten by the winner's row."""
    r = rng(21, T, W, D, target, seed)
    winner = (2 * T) // 3 if winner is None else winner
    g = r.standard_normal((T, D))
    c = r.standard_normal((W, D))
    src = max([winner, *copies])          # the winner's row is drawn where its last copy lies: the same row wherever the first one is
    if D == 1:
        g, c = -np.abs(g) - 0.1, -np.abs(c) - 0.1
        g[src] *= -1
        c[target] *= -1
    else:
        ct = c[target] / np.linalg.norm(c[target])
        g -= 2.0 * np.sqrt(D) * ct
        g[src] += 2.5 * np.sqrt(D) * ct
    g[winner] = g[src]
    if zero_rows:
        g[(winner + 5) % T] = 0
        c[(target + 1) % W] = 0
    g, c = g.astype(np.float32), c.astype(np.float32)
    for t in copies:
        g[t] = g[winner]
    p = spot_ref(g, c, target)
    pred = int(np.argmax(p))
    if W > 1:          # (W = 1: exact by construction, see the module docstring)
        same = (g == g[pred]).all(1)
        assert pred == min(np.flatnonzero(same)) == min([winner, *copies]), (T, W, D, pred, winner)
        gap = (p[pred] - p[~same]) / p[pred]
        assert gap.size == 0 or float(gap.min()) > 2 * spot_bound(D, W), (T, W, D, float(gap.min()), spot_bound(D, W))
    else:
        assert pred == 0 and bool((p == 1.0).all())
    return dict(g=g, c=c, T=T, W=W, D=D, target=target, pred=pred, p=float(p[pred]), bound=spot_bound(D, W) * float(p[pred]), winner=winner)


def spot_targets(W):
    return sorted({0, W // 2, W - 1})


def spot_cases():
    """Every shape with each of its targets (0, a middle word, W - 1); the zero rows go into the (130, 5, 1024) clips."""
    return [spot_clip(T, W, D, tg, zero_rows=(T, W) == (130, 5)) for T, W, D in SPOT_SHAPES for tg in spot_targets(W)]


def spot_tie_cases(T=130, W=5, D=64, t=20):
    """Two targets x six clips: clip k holds the winner's row at the positions tie_positions[k:] only, so pred = tie_positions[k] and all six
    scores of a target are bit-equal: every position (its wave, its lane, its pass of the lane scan) computes the same probability."""
    pos = [t] + [t + s for s in TIE_STEPS] + [T - 1]
    out = []
    for tg in (0, W - 1):
        for k in range(len(pos)):
            out.append(spot_clip(T, W, D, tg, winner=pos[k], seed=77, copies=pos[k + 1:]))
            assert out[-1]["pred"] == pos[k]
    return pos, out


def spot_batch(clips):
    """Concatenated rows, offsets and targets of clips of one D."""
    return dict(g=np.concatenate([c["g"] for c in clips]), c=np.concatenate([c["c"] for c in clips]),
                goff=offsets([c["T"] for c in clips]), coff=offsets([c["W"] for c in clips]),
                target=np.asarray([c["target"] for c in clips], np.int32), D=clips[0]["D"])


def spot_mixed_batch(D=64):
    """[valid, T = 0, valid, W = 0, target = W, valid, T = 8193] -> (batch, flags): flagged clips must read -1 / NaN, the others what they read alone."""
    ok = [spot_clip(9, 4, D, 1, seed=1), spot_clip(70, 3, D, 2, seed=2), spot_clip(5, 7, D, 0, seed=3)]
    r = rng(22, D)
    rows = lambda n: r.standard_normal((n, D)).astype(np.float32)
    empty_t = dict(g=rows(0), c=rows(3), T=0, W=3, D=D, target=0)
    empty_w = dict(g=rows(4), c=rows(0), T=4, W=0, D=D, target=0)
    bad_tg = dict(g=rows(6), c=rows(5), T=6, W=5, D=D, target=5)
    long_t = dict(g=rows(8193), c=rows(2), T=8193, W=2, D=D, target=1)
    clips = [ok[0], empty_t, ok[1], empty_w, bad_tg, ok[2], long_t]
    return clips, [False, True, False, True, True, False, True]


def spot32(g, c, target, temp=np.float32(TEMP), last=False, drop_word=False, normalise=True, lane_last=False):
    """A plain float32 numpy statement of spot_kernel -> (pred, score).  A frame's probability is a function of its row and the words alone (a
    row-wise sum, not a blocked matmul), as in the kernel.  Keyword arguments = the planted defects: last arg-max, softmax over W - 1 words,
    rows not normalised, the first index of a lane's strided scan lost (a lane keeps the LAST of equal values among t = lane, lane + 64, ..)."""
    f = np.float32
    one = f(1)
    gn = one / np.maximum(np.sqrt((g * g).sum(1, dtype=f)), f(1e-12)) if normalise else np.ones(len(g), f)
    cn = one / np.maximum(np.sqrt((c * c).sum(1, dtype=f)), f(1e-12)) if normalise else np.ones(len(c), f)
    gs, cs = g * gn[:, None], c * cn[:, None]
    L = np.stack([(gs * cs[w][None]).sum(1, dtype=f) for w in range(len(c))], axis=1) / temp
    Ls = L[:, :-1] if drop_word and L.shape[1] > 1 else L
    E = np.exp(Ls - Ls.max(1, keepdims=True))
    a = (np.exp(L[:, target] - Ls.max(1)) / E.sum(1, dtype=f)).astype(f)
    if last:
        pred = len(a) - 1 - int(np.argmax(a[::-1]))
    elif lane_last:
        best, bi = f(-np.inf), 2 ** 31 - 1
        for lane in range(min(64, len(a))):
            sub = a[lane::64]
            k = len(sub) - 1 - int(np.argmax(sub[::-1]))
            if sub[k] > best or (sub[k] == best and lane + 64 * k < bi):
                best, bi = sub[k], lane + 64 * k
        pred = bi
    else:
        pred = int(np.argmax(a))
    return pred, float(a[pred])


# =================================================================================================================================== asd
ASD_C = 32
# (n, D, candidates per query): every count of 0, 1, .. 7 and 9, n in {1, 4, 5, 9}, D in {1, 64, 100, 512, 1024}
ASD_BATCHES = [(1, 1, [3]), (4, 64, [0, 1, 2, 7]), (5, 100, [3, 4, 5, 6, 9]), (9, 512, [6, 0, 7, 2, 9, 6, 5, 4, 6]), (4, 1024, [6, 6, 9, 3])]
# what a query of the (9, 512) batch plants on top (index -> kind)
ASD_SPECIAL = {0: "dup13", 3: "zero_query", 5: "dup35", 6: "zero_cand_wins", 7: "zero_cand", 8: "tiny"}


def asd_margin(D):
    return 2 * (D + ASD_C) * U


def asd_cos64(q, cand):
    q, cand = q.astype(np.float64), cand.astype(np.float64)
    return (cand * q[None]).sum(1) / np.maximum(np.linalg.norm(q) * np.linalg.norm(cand, axis=1), 1e-8)


def asd_ref(q, cand, limit=6):
    """float64 -> [first arg-max over the first min(2 | 4 | 6, P, limit) candidates] (-1 without candidates); asserts the margin condition."""
    P = min(len(cand), limit)
    if P == 0:
        return [-1, -1, -1]
    if not q.any():          # every product is 0 * c = 0 in any arithmetic: all cosines are exactly 0 / 1e-8 = 0, the first wins -- no margin involved
        return [0, 0, 0]
    cos = asd_cos64(q, cand[:P])
    out = []
    for k in (2, 4, 6):
        k = min(k, P)
        w = int(np.argmax(cos[:k]))
        others = ~(cand[:k] == cand[w]).all(1)
        assert w == min(np.flatnonzero(~others)), "the first of the copies"
        gap = cos[w] - cos[:k][others]
        assert gap.size == 0 or float(gap.min()) > asd_margin(len(q)), (len(q), k, float(gap.min()))
        out.append(w)
    return out


def asd_batch(n, D, counts):
    """Queries, candidates, offsets, the float64 predictions and, per query, whether the oracle's fp32 statement is expected to agree
    (`plain`: at least one candidate, nothing zero or tiny).  Candidates lean towards the query by a strength that grows with the odd indices
    (1 < 3 < 5), so the three columns differ; index 6, which no column may consider, leans most."""
    assert len(counts) == n
    r = rng(31, n, D, *counts)
    q = r.standard_normal((n, D))
    cands, plain, kinds = [], [], []
    lean = {1: 0.3, 3: 0.6, 5: 0.9, 6: 1.5}
    for i, P in enumerate(counts):
        kind = ASD_SPECIAL.get(i) if (n, D) == (9, 512) else None
        qi = q[i] / np.linalg.norm(q[i])
        c = r.standard_normal((P, D))
        if D == 1:          # cosines are +-1: one candidate alone has the query's sign
            c = -np.sign(q[i]) * (np.abs(c) + 0.1)
            if P > 1:
                c[1] *= -1
        else:
            for p in range(P):
                c[p] += lean.get(p, 0.0) * np.sqrt(D) * qi
        if kind == "dup13":
            c[3] = c[1]
            c[5] -= 0.9 * np.sqrt(D) * qi          # the copies are the best of all six: columns 1, 1, 1
        elif kind == "dup35":
            c[5] = c[3]                             # columns 1, 3, 3
        elif kind == "zero_query":
            q[i] = 0
        elif kind == "zero_cand_wins":             # every non-zero candidate leans away: the zero candidate's cosine 0 is the largest
            c = r.standard_normal((P, D)) - 0.5 * np.sqrt(D) * qi
            c[2] = 0
        elif kind == "zero_cand":
            c[0] = 0
        elif kind == "tiny":                       # |q| |c| < 1e-8 for the tiny candidate 1 only: eps applies to the PRODUCT of the norms
            q[i] *= 1e-5 / np.linalg.norm(q[i])
            c[1] = 1e-5 * qi + 1e-7 * r.standard_normal(D) / np.sqrt(D)
        cands.append(c.astype(np.float32))
        plain.append(P > 0 and kind in (None, "dup13", "dup35"))
        kinds.append(kind)
    q = q.astype(np.float32)
    pred = np.asarray([asd_ref(q[i], cands[i]) for i in range(n)], np.int32)
    for i, P in enumerate(counts):
        if P >= 7 and kinds[i] is None and D > 1:
            assert int(np.argmax(asd_cos64(q[i], cands[i]))) == 6 and 6 not in pred[i], "the best of all candidates sits where no column looks"
        if P >= 6 and kinds[i] is None and D > 1:
            assert pred[i].tolist() == [1, 3, 5]
    return dict(q=q, cand=np.concatenate(cands) if cands else np.zeros((0, D), np.float32), cands=cands, coff=offsets(counts), pred=pred,
                plain=plain, kinds=kinds, n=n, D=D)


def asd32(q, cand, temp=np.float32(TEMP), limit=6, last=False, eps_each=False):
    """A plain float32 numpy statement of asd_kernel for one query -> three indices.  Keyword arguments = the planted defects: `limit`
    candidates considered instead of six, last arg-max, eps applied to each norm instead of to their product."""
    f = np.float32
    P = min(len(cand), limit)
    if P == 0:
        return [-1, -1, -1]
    qn = np.sqrt((q * q).sum(dtype=f))
    cn = np.sqrt((cand[:P] * cand[:P]).sum(1, dtype=f))
    den = np.maximum(qn, f(1e-8)) * np.maximum(cn, f(1e-8)) if eps_each else np.maximum(qn * cn, f(1e-8))
    sim = ((cand[:P] * q[None]).sum(1, dtype=f) / den / temp).astype(f)
    out = []
    for k in (2, 4, 6):
        k = min(max(k, limit if limit > 6 and k == 6 else k), P)
        e = np.exp(sim[:k] - sim[:k].max())
        sc = (e / e.sum(dtype=f)).astype(f)
        out.append(k - 1 - int(np.argmax(sc[::-1])) if last else int(np.argmax(sc)))
    return out
