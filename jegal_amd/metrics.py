"""Task metrics on the GPU (evaluation/evaluate_{retrieval,spotting,asd}.py of the reference).

The N x N similarity matrix is never materialised: ``jg_sim_rank`` counts, per query row, the
gallery rows that beat / tie the diagonal (exact-fp32 MFMA), which is all ``compute_metrics``
(evaluate_retrieval.py:51-65) uses.  With ``torch.distributed`` initialised, queries are sharded
across ranks (contiguous blocks, the --rank/--nshard rule of extract_gestsync_feats.py:366-370) and
the gallery is assembled with one all-gather (RCCL over xGMI on MI355X).
"""
import ast

import numpy as np
import torch

from ._lib import Engine
from . import dist as jdist


def cat_rows(x):
    """One float32 (rows, D) tensor from a ragged batch -- a list of per-item (n_i, D) arrays or tensors -- or from one (n, D) array or
    tensor.  Host arrays: one np.concatenate to float32 and one CPU tensor (the engine entry that takes it uploads it, once); tensors: the
    torch.cat of the float32 parts where they lie (the extractors' outputs stay on the device).  One matrix is not copied."""
    if isinstance(x, torch.Tensor):
        return x.to(torch.float32)
    if not isinstance(x, (list, tuple)) or (len(x) and np.ndim(x[0]) < 2):          # (a list of plain rows is one matrix)
        return torch.as_tensor(np.asarray(x, np.float32))
    if len(x) and isinstance(x[0], torch.Tensor):
        return torch.cat([torch.as_tensor(m).to(torch.float32) for m in x], 0)
    return torch.as_tensor(np.concatenate([np.asarray(m, np.float32) for m in x], 0))


def offsets_of(mats):
    """the (n + 1,) int32 row offsets of a ragged batch in cat_rows' order"""
    off = np.zeros(len(mats) + 1, np.int32)
    off[1:] = np.cumsum([m.shape[0] for m in mats])
    return off


def to_host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


_offsets, _host = offsets_of, to_host          # (the names these two had before they were public)


def span(off, i):
    """the rows of item i in a flat result laid out by the offsets `off`"""
    return slice(int(off[i]), int(off[i + 1]))


def window_starts(n, win, hop):
    """the first frame of each of n windows, `hop` apart (win == 0: the one window over everything starts at 0) -> (n,) int32"""
    return (np.arange(n) * (hop if win else 0)).astype(np.int32)


def boundary_list(wb):
    """the word boundaries of one clip as a list: the list itself, or its repr as the csv rows hold it"""
    return ast.literal_eval(wb) if isinstance(wb, str) else wb


def word_bounds(wb):
    """word boundaries of one clip -> (words [str], start (W,) int64, end (W,) int64): [word, start, end] triplets, (start, end) pairs (no
    word: the first entry stands in) or the repr of either"""
    wb = boundary_list(wb)
    return [str(b[0]) for b in wb], np.asarray([b[-2] for b in wb], np.int64), np.asarray([b[-1] for b in wb], np.int64)


def check_word_count(n_bounds, n_rows, name=None):
    """every content row needs its boundary; name: what the message is about (a file, "utterance 3")"""
    if n_bounds != n_rows:
        raise ValueError("{}{} word boundaries for {} content rows".format("" if name is None else "{}: ".format(name), n_bounds, n_rows))


def video_level(engine, mats):
    """Temporal mean per clip (evaluate_retrieval.py:30-31): list of (T_i,512) -> (N,512) device."""
    return engine.pool_mean(cat_rows(mats), offsets_of(mats))


def metrics_from_ranks(rank, ties):
    """Rebuild the reference's `ind` vector (one entry per tied position) and its statistics."""
    rank = np.asarray(rank, np.int64)
    ties = np.asarray(ties, np.int64)
    ind = np.concatenate([np.arange(r, r + t) for r, t in zip(rank, ties)]) if len(rank) else np.zeros(0, np.int64)
    n = len(ind)
    out = {f"R{k}": float(np.sum(ind < k)) / n for k in (1, 5, 10, 25, 50)}
    out["MR"] = float(np.median(ind) + 1)
    return out


def _normalised_and_gathered(eng, queries, gallery):
    """What retrieval_metrics, retrieve and partner_ranks start from: both sets L2-normalised, the gallery all-gathered over the ranks (a
    single process: the rows themselves) -> (queries, gallery, the row of the gallery at which this rank's block begins)"""
    q = eng.l2norm(cat_rows(queries))
    g, row_offset = jdist.all_gather_rows(eng.l2norm(cat_rows(gallery)))
    return q, g, row_offset


def retrieval_metrics(emb1, emb2, engine=None):
    """get_similarity_matrix + compute_metrics (evaluate_retrieval.py:38-65) for query set emb1
    against gallery emb2 (both (N,512), un-normalised video-level means).  Sharded over ranks when
    torch.distributed is initialised: every rank passes ITS contiguous block of rows."""
    eng = engine or Engine.get()
    e1, gallery, row_offset = _normalised_and_gathered(eng, emb1, emb2)
    rank, ties = eng.sim_rank(e1, gallery, row_offset)
    if jdist.world_size() > 1:
        rank, _ = jdist.all_gather_rows(rank.to(torch.int32).reshape(-1, 1))
        ties, _ = jdist.all_gather_rows(ties.to(torch.int32).reshape(-1, 1))
    return metrics_from_ranks(rank.flatten().cpu().numpy(), ties.flatten().cpu().numpy())


def retrieve(emb_q, emb_g, k=10, engine=None):
    """The retrieval itself: for each row of the query set emb_q the k rows of the gallery emb_g with the largest cosine similarity, best
    first, ties to the smaller gallery row (both (N,512), un-normalised video-level means, as for retrieval_metrics).  The scores are the
    ones retrieval_metrics ranks by, bit for bit (jg_sim_topk next to jg_sim_rank); the N x N matrix is never written.  Sharded like
    retrieval_metrics when torch.distributed is initialised: every rank passes ITS contiguous block of both sets, the gallery is
    all-gathered, each rank runs its queries and the results are gathered in rank order.
    Returns host arrays (idx (N,k) int32: global gallery rows, -1 where the gallery has fewer than k; score (N,k) float32)."""
    eng = engine or Engine.get()
    q, g, _ = _normalised_and_gathered(eng, emb_q, emb_g)
    idx, score = eng.sim_topk(q, g, k)
    idx, _ = jdist.all_gather_rows(idx)
    score, _ = jdist.all_gather_rows(score)
    return to_host(idx), to_host(score)


def search_groups(lengths, segment=0):
    """The groups search() cuts a list of clips into: (g_offsets (G + 1,) int64 over the concatenated frame rows, clip (G,) int32, start (G,)
    int32 = the group's first frame inside its clip).  segment == 0: one group per clip; segment > 0: runs of `segment` frames, the last run
    of a clip shorter, every clip ending a group."""
    sizes, clip, start = [], [], []
    for i, t in enumerate(int(t) for t in lengths):
        step = segment if segment > 0 else max(t, 1)
        for s in range(0, max(t, 1), step):            # (an empty clip is one empty group)
            sizes.append(min(step, t - s))
            clip.append(i)
            start.append(s)
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return off, np.asarray(clip, np.int32), np.asarray(start, np.int32)


def _search_walk(queries, dim, corpus, k, segment, normalize, engine, max_rows, phrases=False):
    """The walk of search() and Corpus.search(), and (phrases) of their search_phrases: check the arguments, cut the clips into groups (search_groups) and the groups into pieces
    of at most max_rows rows, score piece after piece into one merged top-k list, and decode its gallery rows into (clip, frame, score).
    corpus(q) checks the (Q, D) query tensor against the gallery and returns (the frames of every clip, score_piece); score_piece(eng, q,
    r0, r1, c0, c1, g_offsets, res) brings the gallery rows r0 .. r1 - 1 (of the clips c0 .. c1 - 1) to the device and scores them with the
    caller's entry, merging into res.  dim: what a message calls the queries' D.
    phrases: `queries` is a list of (W_i, D) word matrices, each ONE query (q: their rows, Q: their number); score_piece gets the piece's
    first group as a ninth argument and returns GROUPS (Engine.sim_coupling), and `frame` is the first frame of the returned group.
    align_piece (phrases only; corpus(q) may return it as a third value): align_piece(eng, q, r0, r1, c0, c1, g_offsets, g0, idx, into)
    passes the piece once more with the FINAL idx (Engine.sim_align, which writes the slots of the piece's groups only) -> into =
    (frames, score); a fourth array comes back, word_frame
    (Q, k, Wmax) int32: the frame inside the returned clip of every word, -1 behind a query's words and where there is no result."""
    k, segment = int(k), int(segment)
    if not 1 <= k <= 128:
        raise ValueError("k must be 1..128")
    if segment < 0:
        raise ValueError("segment must be >= 0 (0: one group per clip)")
    q = cat_rows(queries)
    if q.ndim != 2:
        raise ValueError("queries must be (Q, {})".format(dim))
    Q = len(queries) if phrases else int(q.shape[0])
    lengths, score_piece, align_piece = (tuple(corpus(q)) + (None,))[:3]
    goff, gclip, gstart = search_groups(lengths, segment)
    n_groups = len(gclip)
    if goff[-1] > 2 ** 31 - 1:
        raise ValueError("more than INT32_MAX gallery rows")
    sizes = np.diff(goff)
    if max_rows is not None and (int(max_rows) < 1 or (n_groups and sizes.max() > int(max_rows))):
        raise ValueError("max_rows must hold the largest group ({} rows): groups are never split; use segment".format(int(sizes.max()) if n_groups else 0))
    empty = (np.full((Q, k), -1, np.int32), np.full((Q, k), -1, np.int32), np.full((Q, k), -np.inf, np.float32))
    if align_piece:
        empty += (np.full((Q, k, max([int(m.shape[0]) for m in queries] or [0])), -1, np.int32),)
    if Q == 0 or goff[-1] == 0:
        return empty
    eng = engine or Engine.get()
    if normalize:
        q = eng.l2norm(q)
    res, g0, pieces = None, 0, []
    while g0 < n_groups:                             # pieces = runs of whole groups of at most max_rows rows
        g1 = n_groups
        if max_rows is not None:
            g1 = g0 + 1
            while g1 < n_groups and goff[g1 + 1] - goff[g0] <= int(max_rows):
                g1 += 1
        r0, r1 = int(goff[g0]), int(goff[g1])
        if r1 > r0:
            res = score_piece(eng, q, r0, r1, int(gclip[g0]), int(gclip[g1 - 1]) + 1, goff[g0:g1 + 1] - r0, res, *([g0] if phrases else []))
            pieces.append((g0, g1, r0, r1))
        g0 = g1
    if res is None:
        return empty
    word_frame = None
    if align_piece:
        # every piece once more, now that the lists are final: a piece fills the slots of its own groups with rows counted from its first
        into, piece_row0 = None, np.zeros(n_groups, np.int64)
        for g0, g1, r0, r1 in pieces:
            into = align_piece(eng, q, r0, r1, int(gclip[g0]), int(gclip[g1 - 1]) + 1, goff[g0:g1 + 1] - r0, g0, res[0], into)
            piece_row0[g0:g1] = r0
        rows, grp = to_host(into[0]).astype(np.int64), np.maximum(to_host(res[0]).astype(np.int64), 0)
        clip_row0 = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])[gclip[grp]]
        word_frame = np.where(rows >= 0, rows + (piece_row0[grp] - clip_row0)[:, :, None], -1).astype(np.int32)
    grp, pos = (res[0], torch.zeros_like(res[0])) if phrases else eng.group_of_rows(res[0], goff, 0)
    grp, pos, score = to_host(grp).astype(np.int64), to_host(pos).astype(np.int32), to_host(res[1]).astype(np.float32)
    found = grp >= 0
    clip = np.where(found, gclip[np.maximum(grp, 0)], -1).astype(np.int32)
    frame = np.where(found, gstart[np.maximum(grp, 0)] + pos, -1).astype(np.int32)
    return (clip, frame, score) if word_frame is None else (clip, frame, score, word_frame)


def search(queries, clips, k=10, segment=0, normalize=True, engine=None, max_rows=None):
    """For each query row (a word, a phrase: (Q, D), the space of the content embeddings), the k clips of a corpus that gesture it and the
    frame at which they do: clips is a list of (T_i, D) frame-level gesture arrays; a clip scores as its best frame (jg_sim_topk_grouped:
    no pooling, no Q x sum T matrix, scores as jg_sim_topk computes them).  segment > 0: the groups are runs of `segment` frames of a clip
    instead of whole clips, so a long track can come back with several moments.  normalize: rows are L2-normalised first (cosine
    similarity); False: the rows as stored.  max_rows: the gallery goes to the device in pieces of at most that many rows, cut at group
    boundaries and merged -- the same result, for corpora larger than device memory.
    Returns host arrays (clip (Q, k) int32, frame (Q, k) int32: the frame inside the clip, score (Q, k) float32), best first, ties to the
    earlier clip and frame; -1 / -1 / -inf where fewer than k groups exist."""
    def corpus(q):
        D = int(q.shape[1])
        mats = [c if isinstance(c, torch.Tensor) else np.asarray(c, np.float32) for c in clips]
        if any(c.ndim != 2 or c.shape[1] != D for c in mats):
            raise ValueError("every clip must be (T_i, {}) like the queries".format(D))
        first_row = np.concatenate([[0], np.cumsum([c.shape[0] for c in mats])])

        def score_piece(eng, q, r0, r1, c0, c1, g_offsets, res):        # the rows of the piece come from the clips c0 .. c1 - 1
            rows = cat_rows(mats[c0:c1])[r0 - int(first_row[c0]):r1 - int(first_row[c0])]
            if normalize:
                rows = eng.l2norm(rows)
            return eng.sim_topk_grouped(q, rows, g_offsets, int(k), gallery_offset=r0, merge_into=res)
        return [c.shape[0] for c in mats], score_piece
    return _search_walk(queries, "D", corpus, k, segment, normalize, engine, max_rows)


def _phrase_list(queries):
    """search_phrases' queries: a list of (W_i, D) word matrices of 1..64 rows each -> (the list as float32 arrays or tensors, w_offsets)"""
    mats = [m.to(torch.float32) if isinstance(m, torch.Tensor) else np.asarray(m, np.float32) for m in queries]
    if any(m.ndim != 2 for m in mats) or len({int(m.shape[1]) for m in mats}) > 1:
        raise ValueError("queries must be a list of (W_i, D) word matrices with one D")
    if any(not 1 <= m.shape[0] <= 64 for m in mats):
        raise ValueError("a query must have 1..64 word rows")
    return mats, offsets_of(mats)


def _no_phrases(k, align=False):
    if not 1 <= int(k) <= 128:
        raise ValueError("k must be 1..128")
    out = np.zeros((0, int(k)), np.int32), np.zeros((0, int(k)), np.int32), np.zeros((0, int(k)), np.float32)
    return out + (np.zeros((0, int(k), 0), np.int32),) if align else out


def _phrase_pieces(rows_of, w_off, k, order, align):
    """score_piece and align_piece of the two search_phrases (_search_walk): rows_of(eng, r0, r1, c0, c1) brings a piece's rows to the
    device; order: jg_sim_ordered instead of jg_sim_coupling (called only then)."""
    def score_piece(eng, q, r0, r1, c0, c1, g_offsets, res, g0):
        entry = eng.sim_ordered if order else eng.sim_coupling
        return entry(q, w_off, rows_of(eng, r0, r1, c0, c1), g_offsets, int(k), group_offset=g0, merge_into=res)

    def align_piece(eng, q, r0, r1, c0, c1, g_offsets, g0, idx, into):
        return eng.sim_align(q, w_off, rows_of(eng, r0, r1, c0, c1), g_offsets, idx, bool(order), group_offset=g0, into=into)
    return score_piece, align_piece if align else None


def search_phrases(queries, clips, k=10, segment=0, normalize=True, engine=None, max_rows=None, order=False, align=False):
    """search() for queries of several words that keeps the word-to-frame structure (late interaction, jg_sim_coupling): queries is a list
    of (W_i, D) word matrices (1..64 rows each), each ONE query; a group of frames (a clip, or a run of `segment` frames of it) scores as
    the mean over the query's words of each word's best frame in the group -- no pooling of the words or the frames, no (words) x (frames)
    matrix.  clips, segment, normalize and max_rows as for search(); pieces are cut at group boundaries and merged, the same result.
    Returns host arrays (clip (Q, k) int32, start (Q, k) int32: the first frame of the returned group inside its clip (search_groups),
    score (Q, k) float32), best first, ties to the earlier group; -1 / -1 / -inf where fewer than k groups have a score.
    order: the words are assigned to frames in word order (jg_sim_ordered): the score is the best mean over frames t_1 <= .. <= t_W, one
    frame may serve consecutive words; it never exceeds the unordered score.
    align: a fourth array, word_frame (Q, k, Wmax) int32: the frame inside the returned clip (counted from the clip's first frame, also
    with segment > 0) that every word of the query took in the returned group (jg_sim_align); -1 behind a query's words and in empty
    slots.  Under max_rows the pieces are passed a second time, after the lists are final."""
    mats_q, w_off = _phrase_list(queries)
    if not mats_q:
        return _no_phrases(k, align)

    def corpus(q):
        D = int(q.shape[1])
        mats = [c if isinstance(c, torch.Tensor) else np.asarray(c, np.float32) for c in clips]
        if any(c.ndim != 2 or c.shape[1] != D for c in mats):
            raise ValueError("every clip must be (T_i, {}) like the queries".format(D))
        first_row = np.concatenate([[0], np.cumsum([c.shape[0] for c in mats])])

        def rows_of(eng, r0, r1, c0, c1):
            rows = cat_rows(mats[c0:c1])[r0 - int(first_row[c0]):r1 - int(first_row[c0])]
            return eng.l2norm(rows) if normalize else rows
        return ([c.shape[0] for c in mats],) + _phrase_pieces(rows_of, w_off, k, order, align)
    return _search_walk(mats_q, "D", corpus, k, segment, normalize, engine, max_rows, phrases=True)


def coupling_matrix(contents, gestures, normalize=True, engine=None, ordered=False):
    """The late-interaction score of every utterance against every clip: contents is a list of (W_i, D) word matrices (1..64 rows each),
    gestures a list of (T_j, D) frame matrices; entry (i, j) is the mean over utterance i's words of each word's largest product with a
    frame of clip j (normalize: rows L2-normalised first, so cosines).  One jg_sim_coupling call; the (words) x (frames) matrix is never
    written.  Returns the (N_c, N_g) float32 matrix on the engine's device; NaN where a pair has no score (an empty clip).
    ordered: the words take frames in word order (one jg_sim_ordered call instead), never more than the unordered entry."""
    eng = engine or Engine.get()
    mats_c, w_off = _phrase_list(contents)
    if not mats_c or not len(gestures):
        return torch.full((len(mats_c), len(gestures)), float("nan"), dtype=torch.float32, device=eng.device)
    w, g = cat_rows(mats_c), cat_rows(gestures)
    if normalize:
        w, g = eng.l2norm(w), eng.l2norm(g)
    return (eng.sim_ordered if ordered else eng.sim_coupling)(w, w_off, g, offsets_of(gestures), 1, want_matrix=True)[2]


def coupling_retrieval_metrics(contents, gestures, engine=None, ordered=False):
    """R@K and the median rank of evaluate_retrieval with the late-interaction score in place of the cosine of the pooled vectors:
    {"c2g": .., "g2c": ..}, each in metrics_from_ranks' form, both from the one coupling_matrix (utterance i belongs to clip i).  The rank
    of a partner is the number of strictly larger entries in its row (c2g) or its column (g2c), ties counted as jg_sim_rank counts them.
    g2c here ranks the UTTERANCES for a clip by the same word -> frame score (every word of the utterance looks for its best frame in the
    clip); it is not a second, frame -> word score.  Counted with torch on the device matrix.  Single process only.
    ordered: from coupling_matrix(ordered=True), the score with the words in order."""
    if jdist.world_size() > 1:
        raise RuntimeError("coupling_retrieval_metrics runs in one process: it is not sharded over ranks")
    if len(contents) != len(gestures):
        raise ValueError("one clip per utterance")
    M = coupling_matrix(contents, gestures, engine=engine, ordered=ordered)
    d = M.diagonal()
    out = {}
    for name, part, own in (("c2g", M, d[:, None]), ("g2c", M.t(), d[:, None])):
        rank, ties = (part > own).sum(1), (part == own).sum(1)
        out[name] = metrics_from_ranks(to_host(rank), to_host(ties))
    return out


class Corpus:
    """The frame rows of many clips, prepared once and searched many times: what search() does with a list of clips on every call --
    concatenate, normalise, upload -- happens in build(), and the rows may be kept in 16 bits, as the reference's CUDA path writes them
    (half the bytes on disk, in the upload and on the device; jg_sim_search reads them as they are).
    rows (sum T, D) float16 or float32, lengths (N,) int64 frames per clip, names (N,) str, normalized: whether build() L2-normalised the
    rows.  A 16-bit corpus is searched AS STORED: a score is the exact fp32 chain over the stored rows, the one search() computes for
    rows.astype(float32).  Against the float32 corpus of the same clips a score differs by at most sum_d |q_d| (2^-11 |g_d| + 2^-25) --
    fp16 rounds to nearest even with a relative error of 2^-11 on normal values and an absolute one of 2^-25 below 2^-14 -- plus the two
    fp32 chain bounds D 2^-24 sum_d |q_d g_d| (derived from the formats, not measured)."""
    VERSION = 1
    CHUNK = 1 << 18              # rows that build() normalises at a time

    def __init__(self, rows, lengths, names, normalized):
        self.rows = np.ascontiguousarray(rows)
        self.lengths = np.asarray(lengths, np.int64).reshape(-1)
        self.names = np.asarray(names, dtype=str).reshape(-1)
        self.normalized = bool(normalized)
        if self.rows.dtype not in (np.float16, np.float32) or self.rows.ndim != 2:
            raise ValueError("rows must be a (sum T, D) float16 or float32 array")
        if (self.lengths < 0).any() or int(self.lengths.sum()) != self.rows.shape[0] or len(self.names) != len(self.lengths):
            raise ValueError("lengths must be >= 0 and add up to the rows, with one name per clip")
        if self.rows.shape[0] > 2 ** 31 - 1:
            raise ValueError("more than INT32_MAX gallery rows")
        self._dev = None         # (engine, the rows on its device): kept between searches

    @classmethod
    def build(cls, clips, names=None, dtype="float16", normalize=True, engine=None):
        """clips: a list of (T_i, D) frame-level arrays; names: one per clip (default: "0", "1", ..).  normalize: the rows are L2-normalised in
        fp32 (engine.l2norm, as search() does); then they are rounded to dtype ("float16" or "float32") to nearest even, the bits of
        numpy.astype."""
        dtype = np.dtype(dtype)
        if dtype not in (np.float16, np.float32):
            raise ValueError("dtype must be float16 or float32")
        clips = [to_host(c).astype(np.float32, copy=False) if isinstance(c, torch.Tensor) else np.asarray(c, np.float32) for c in clips]
        D = clips[0].shape[1] if clips and clips[0].ndim == 2 else 0
        if any(c.ndim != 2 or c.shape[1] != D for c in clips):
            raise ValueError("every clip must be (T_i, D) with one D")
        names = [str(i) for i in range(len(clips))] if names is None else list(names)
        if len(names) != len(clips):
            raise ValueError("names needs one entry per clip")
        rows = np.concatenate(clips, 0) if clips else np.zeros((0, 0), np.float32)
        if normalize and rows.shape[0]:
            eng = engine or Engine.get()
            rows = np.concatenate([to_host(eng.l2norm(torch.from_numpy(rows[a:a + cls.CHUNK]))).astype(np.float32, copy=False)
                                   for a in range(0, rows.shape[0], cls.CHUNK)], 0)
        return cls(rows.astype(dtype), [c.shape[0] for c in clips], names, normalize)

    def save(self, path):
        """one uncompressed .npz: rows, lengths, names, normalized, version"""
        np.savez(path, rows=self.rows, lengths=self.lengths, names=self.names, normalized=np.asarray(self.normalized), version=np.asarray(self.VERSION))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if int(z["version"]) != cls.VERSION:
                raise ValueError("{}: corpus version {}, this package reads {}".format(path, int(z["version"]), cls.VERSION))
            return cls(z["rows"], z["lengths"], z["names"], bool(z["normalized"]))

    def _device_rows(self, eng, r0, r1, keep):
        """rows r0 .. r1 - 1 on the engine's device, in their stored type; keep: the whole corpus, uploaded once per engine"""
        if not keep:
            return torch.from_numpy(self.rows[r0:r1]).to(eng.device)
        if self._dev is None or self._dev[0] is not eng:
            self._dev = (eng, torch.from_numpy(self.rows).to(eng.device))
        return self._dev[1]

    def search(self, queries, k=10, segment=0, normalize=True, engine=None, max_rows=None):
        """search() over the prepared rows: the same (clip, frame, score) triple, the same groups (segment) and the same piece-wise merging at
        group boundaries under max_rows, through jg_sim_search, which spreads the rows over every CU.  normalize: the QUERY rows are
        L2-normalised first (the corpus rows are what build() made them).  Without max_rows the rows stay on the engine's device between
        calls: repeated searches upload the queries only."""
        def corpus(q):
            if self.rows.shape[0] and q.shape[1] != self.rows.shape[1]:
                raise ValueError("queries must be (Q, {})".format(self.rows.shape[1]))

            def score_piece(eng, q, r0, r1, c0, c1, g_offsets, res):
                return eng.sim_search(q, self._device_rows(eng, r0, r1, max_rows is None), int(k), g_offsets=g_offsets, gallery_offset=r0,
                                      merge_into=res)
            return self.lengths, score_piece
        return _search_walk(queries, self.rows.shape[1], corpus, k, segment, normalize, engine, max_rows)

    def search_phrases(self, queries, k=10, segment=0, normalize=True, engine=None, max_rows=None, order=False, align=False):
        """search_phrases() over the prepared rows, 16- or 32-bit as stored: the same (clip, start, score) triple through jg_sim_coupling,
        or jg_sim_ordered with order, and word_frame with align; the rest as for search()."""
        mats_q, w_off = _phrase_list(queries)
        if not mats_q:
            return _no_phrases(k, align)

        def corpus(q):
            if self.rows.shape[0] and q.shape[1] != self.rows.shape[1]:
                raise ValueError("queries must be (W_i, {})".format(self.rows.shape[1]))

            def rows_of(eng, r0, r1, c0, c1):
                return self._device_rows(eng, r0, r1, max_rows is None)
            return (self.lengths,) + _phrase_pieces(rows_of, w_off, k, order, align)
        return _search_walk(mats_q, self.rows.shape[1], corpus, k, segment, normalize, engine, max_rows, phrases=True)


def partner_ranks(emb1, emb2, engine=None):
    """jg_sim_rank's rank of every query's own partner (row i of emb1 belongs to row i of emb2), the number retrieval_metrics turns into
    R@K: host int32 (N,), over all ranks' rows in rank order when sharded."""
    eng = engine or Engine.get()
    e1, gallery, row_offset = _normalised_and_gathered(eng, emb1, emb2)
    rank, _ = eng.sim_rank(e1, gallery, row_offset)
    rank, _ = jdist.all_gather_rows(rank.to(torch.int32).reshape(-1, 1))
    return to_host(rank).reshape(-1).astype(np.int32)


def reduce_counts(counts, device=None):
    """Sum a short list of integer counters over the ranks (spotting / ASD need only this): every rank evaluates ITS
    contiguous block of clips (jdist.shard_range) and the totals are all-reduced -- RCCL on device tensors under nccl, host
    tensors under gloo.  Single process: the counts themselves."""
    counts = [int(c) for c in counts]
    if jdist.world_size() == 1:
        return counts
    t = torch.tensor(counts, dtype=torch.int64, device=device if jdist.backend() == "nccl" else "cpu")
    return [int(v) for v in jdist.all_reduce_sum(t).cpu()]


def spotting_counts(pred, score, word_boundaries, target_idx, thresh=0.5, frame_thresh=9):
    """(correct, total) of get_spotting_acc (evaluate_spotting.py:59-90) from the per-clip argmax frame and its probability:
    correct iff start - frame_thresh <= pred <= end + frame_thresh and score >= thresh (:77-84)."""
    correct = 0
    for i, (wb, t) in enumerate(zip(word_boundaries, target_idx)):
        s = max(0, wb[t][1] - frame_thresh)
        e = wb[t][2] + frame_thresh
        if s <= int(pred[i]) <= e and float(score[i]) >= thresh:
            correct += 1
    return correct, len(word_boundaries)


def spotting_accuracy(gestures, contents, word_boundaries, targets, thresh=0.5, frame_thresh=9, engine=None, offsets=None):
    """get_spotting_acc (evaluate_spotting.py:59-90).  ``targets`` are word indices (the reference
    looks the target boundary up in the clip's list, :70) or [word,start,end] boundaries.
    Sharded when torch.distributed is initialised: every rank passes ITS block of clips, the two counters are all-reduced.
    gestures / contents: lists of per-clip (T_i,512) / (W_i,512) arrays as the evaluators load them from the .pkl files, or -- with
    ``offsets=(g_offsets, c_offsets)`` -- the already concatenated (sum T,512) / (sum W,512) tensors (device-resident galleries)."""
    eng = engine or Engine.get()
    wbs = [boundary_list(w) for w in word_boundaries]
    tidx = []
    for wb, t in zip(wbs, targets):
        if isinstance(t, str):
            t = ast.literal_eval(t)
        tidx.append(wb.index(t) if isinstance(t, (list, tuple)) else int(t))
    correct = 0
    if len(wbs):                                  # (a rank may hold no clip when there are fewer clips than ranks)
        if offsets is not None:
            g, c, (goff, coff) = gestures, contents, offsets
        else:
            g, c, goff, coff = cat_rows(gestures), cat_rows(contents), offsets_of(gestures), offsets_of(contents)
        pred, score = eng.spot(g, c, goff, coff, tidx)
        correct, _ = spotting_counts(pred.cpu().numpy(), score.cpu().numpy(), wbs, tidx, thresh, frame_thresh)
    correct, total = reduce_counts([correct, len(wbs)], eng.device)
    return 100.0 * correct / max(1, total)


def _ragged_inputs(gestures, contents, offsets):
    """lists of per-clip arrays, or concatenated tensors with offsets=(g_offsets, c_offsets) -> (g, c, host g_offsets, host c_offsets)"""
    if offsets is not None:
        goff, coff = (o.cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o) for o in offsets)
        return gestures, contents, goff.astype(np.int64), coff.astype(np.int64)
    if not len(gestures):
        return None, None, np.zeros(1, np.int64), np.zeros(1, np.int64)
    return cat_rows(gestures), cat_rows(contents), offsets_of(gestures).astype(np.int64), offsets_of(contents).astype(np.int64)


def attn_call(gestures, contents, temp, normalize, engine, offsets, want_matrix):
    """One Engine.attn_matrix call for the batch -> (matrices | None, [(frames, scores)]) per clip, on the host"""
    g, c, goff, coff = _ragged_inputs(gestures, contents, offsets)
    n = len(goff) - 1
    if n == 0:
        return [], []
    eng = engine or Engine.get()
    A, aoff, bf, bs = eng.attn_matrix(g, c, goff, coff, temp=temp, normalize=normalize, want_matrix=want_matrix)
    T, W = np.diff(goff), np.diff(coff)
    mats = None
    if want_matrix:
        A = to_host(A)
        mats = [A[span(aoff, i)].reshape(W[i], T[i]) for i in range(n)]
    bf, bs = to_host(bf), to_host(bs)
    return mats, [(bf[span(coff, i)], bs[span(coff, i)]) for i in range(n)]


def attention_matrices(gestures, contents, temp=0.07, normalize=True, engine=None, offsets=None):
    """The gesture-word heat maps of a batch of clips: per clip softmax((G C^T) / temp, dim=1)^T, float32 (W_i, T_i) -- get_attn_matrix of
    evaluate_spotting.py:39-57 (normalize=True: rows L2-normalised first) or of utils/plot_heatmap.py:34-59 (normalize=False: rows as stored).
    Inputs as for spotting_accuracy: lists of per-clip (T_i,512) / (W_i,512) arrays, or the concatenated tensors with
    ``offsets=(g_offsets, c_offsets)``.  One jg_attn_matrix call for the whole batch."""
    return attn_call(gestures, contents, temp, normalize, engine, offsets, True)[0]


def spot_words(gestures, contents, temp=0.07, normalize=True, engine=None, offsets=None):
    """Every word of every clip localised (evaluate_spotting.py:72-73 applied to each row of the attention matrix): per clip
    (frames int32 (W_i,), scores float32 (W_i,)) = first arg-max frame of the word's row and its probability.  The matrix itself is
    not written (jg_attn_matrix with A = NULL)."""
    return attn_call(gestures, contents, temp, normalize, engine, offsets, False)[1]


def sync_offset(vid_feats, aud_feats, max_shift=15, min_overlap=1, engine=None):
    """Audio-visual offset of every clip of a ragged batch from its GestSync window embeddings: vid_feats / aud_feats are lists of per-clip
    (Tv_i, D) / (Ta_i, D) arrays (GestSync.extract_clip_feats / extract_clip_audio_feats rows; Ta_i may differ from Tv_i).  For each shift
    d in -max_shift .. max_shift the curve holds the mean cosine of the pairs (video row t, audio row t + d); a shift with fewer than
    min_overlap pairs is NaN and cannot win.  One jg_sync_offset call.
    Returns host arrays (offsets (n,) int32: d > 0 means the audio row matching video row t is row t + d, i.e. the audio track lags by d
    frames; conf (n,) float32: the curve's maximum minus its median; curves (n, 2 max_shift + 1) float32).  A clip without rows, with more
    than 8192, or without a shift of min_overlap pairs: offset 0, conf NaN."""
    if len(vid_feats) != len(aud_feats):
        raise ValueError("one audio array per video array")
    n, W = len(vid_feats), 2 * int(max_shift) + 1
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros((0, W), np.float32)
    eng = engine or Engine.get()
    off, conf, curve = eng.sync_offset(cat_rows(vid_feats), cat_rows(aud_feats), offsets_of(vid_feats), offsets_of(aud_feats), max_shift, min_overlap)
    return to_host(off), to_host(conf), to_host(curve)


def sync_timeline(vid_feats, aud_feats, win=125, hop=25, max_shift=15, min_overlap=1, audio_of=None, engine=None):
    """The audio-visual offset as a function of time: vid_feats / aud_feats are lists of per-track (Tv, D) / (Ta, D) arrays (host arrays or
    device tensors, as for sync_offset; tracks of any length up to 2^20 rows).  Clip i is video track i against audio track audio_of[i]
    (default: i; several clips may name one audio track).  Window j of a clip covers its frames j hop .. j hop + win - 1 (cut at the
    track's end), Tv <= win ? 1 : ceil((Tv - win) / hop) + 1 windows per clip; win = 0: one window over the whole track.  One
    jg_sync_offset_windows call.
    Returns per clip a dict(start (n_win,) int32: the first frame of each window; offset (n_win,) int32; conf (n_win,) float32; curve
    (n_win, 2 max_shift + 1) float32), each as in sync_offset but over the window's frames.  A window without a shift of min_overlap
    pairs: offset 0, conf NaN."""
    n = len(vid_feats)
    if (len(aud_feats) != n) if audio_of is None else (len(audio_of) != n):
        raise ValueError("one audio array per video array, or one audio_of entry per video array")
    if n == 0:
        return []
    if not len(aud_feats):
        raise ValueError("no audio track")
    eng = engine or Engine.get()
    off, conf, curve, w_off, _ = eng.sync_offset_windows(cat_rows(vid_feats), cat_rows(aud_feats), offsets_of(vid_feats), offsets_of(aud_feats),
                                                        a_of=audio_of, max_shift=max_shift, min_overlap=min_overlap, win=win, hop=hop)
    off, conf, curve = to_host(off), to_host(conf), to_host(curve)
    out = []
    for i in range(n):
        w = span(w_off, i)
        out.append(dict(start=window_starts(w.stop - w.start, win, hop), offset=off[w], conf=conf[w], curve=curve[w]))
    return out


def sync_speaker(tracks, audio, win=125, hop=25, max_shift=15, min_overlap=1, engine=None):
    """Which face is in sync with this audio, and when: every video track of `tracks` (a list of (Tv_p, D) arrays, co-temporal: frame t of
    each is the same instant) against the ONE audio track `audio` (Ta, D), per window of `win` frames, `hop` apart (win = 0: one window
    over everything).  One jg_sync_offset_windows call; the audio is not copied per track.
    Returns (speaker (n_win,) int32: per window the track with the largest confidence, the first on ties, -1 where every confidence is
    NaN; conf (n_win, n_tracks) float32).  n_win covers the longest track; a track that has ended reads NaN."""
    P = len(tracks)
    if P == 0:
        return np.zeros(0, np.int32), np.zeros((0, 0), np.float32)
    eng = engine or Engine.get()
    n_win = int(eng.sync_window_counts([max(int(t.shape[0]) for t in tracks)], int(win), int(hop))[0])
    _, conf, _, _, _ = eng.sync_offset_windows(cat_rows(tracks), cat_rows([audio]), offsets_of(tracks), offsets_of([audio]), a_of=np.zeros(P, np.int64),
                                                 max_shift=max_shift, min_overlap=min_overlap, win=win, hop=hop, n_windows=[n_win] * P,
                                                 want_curve=False)
    conf = to_host(conf).reshape(P, n_win).T.copy()
    none = np.isnan(conf).all(axis=1)
    speaker = np.where(none, -1, np.argmax(np.where(np.isnan(conf), -np.inf, conf), axis=1)).astype(np.int32)
    return speaker, conf


def asd_counts(pred):
    """[correct for 2, 4, 6 speakers, queries] from jg_asd's (n,3) argmax indices: the positive is candidate 0 (evaluate_asd.py:101-113)."""
    pred = np.asarray(pred).reshape(-1, 3)
    return [int(np.sum(pred[:, k] == 0)) for k in range(3)] + [int(pred.shape[0])]


def asd_accuracy(query_content, candidate_gestures, engine=None):
    """evaluate_asd.py:94-113: query_content (N,512) video-level; candidate_gestures = list of (P_i,512)
    with the positive at index 0.  Returns accuracies for 2/4/6 speakers.
    Sharded when torch.distributed is initialised: every rank passes ITS block of queries, the four counters are all-reduced."""
    eng = engine or Engine.get()
    counts = [0, 0, 0, 0]
    if len(candidate_gestures):
        counts = asd_counts(eng.asd(cat_rows(query_content), cat_rows(candidate_gestures), offsets_of(candidate_gestures)).cpu().numpy())
    c2, c4, c6, n = reduce_counts(counts, eng.device)
    n = max(1, n)
    return c2 / n, c4 / n, c6 / n


def asd_scores(contents, candidates, temp=0.07, engine=None):
    """Active-speaker detection itself (evaluate_asd.py:26-51 without the grading): per query the word-level content (W_i, D) and a list
    of 1..64 frame-level candidate arrays (T, D) -> per query (prob (P_i,) float32 = softmax(cosine(mean content, mean gesture) / temp)
    over its candidates, pred = the first arg-max).  One jg_asd_windows call (clip-level mode) for the batch."""
    if not len(contents):
        return []
    if len(candidates) != len(contents):
        raise ValueError("one candidate list per query")
    eng = engine or Engine.get()
    tracks = [t for cands in candidates for t in cands]
    s_off = np.zeros(len(candidates) + 1, np.int64)
    s_off[1:] = np.cumsum([len(cands) for cands in candidates])
    prob, p_off, pred, _, _ = eng.asd_windows(cat_rows(tracks), offsets_of(tracks), cat_rows(contents), offsets_of(contents), np.arange(len(tracks)),
                                              s_off, win=0, temp=temp)
    prob, pred = to_host(prob), to_host(pred)
    return [(prob[span(p_off, i)], int(pred[i])) for i in range(len(contents))]


def batch_bounds(word_boundaries, contents, names=None):
    """the word boundaries of every item of a batch, each checked against its content rows (names: what to call the items in the message)
    -> the concatenated (start, end)"""
    se = [word_bounds(wb)[1:] for wb in word_boundaries]
    for i, ((s, _), c) in enumerate(zip(se, contents)):
        check_word_count(len(s), len(c), None if names is None else names[i])
    return np.concatenate([s for s, _ in se]), np.concatenate([e for _, e in se])


def asd_timeline(contents, word_boundaries, tracks, win=25, hop=5, temp=0.07, engine=None):
    """Who gestures to the speech, and when: for a scene with the word-level content (W, D) of one utterance, its word boundaries (frames
    of the scene, inclusive) and a list of 1..64 co-temporal frame-level tracks (T_p, D), the speaker probabilities of every window of
    `win` frames, `hop` frames apart -> dict(start (n_win,) int32: first frame of each window, prob (n_win, P) float32, pred (n_win,)
    int32), n_win = ceil(longest track / hop).  A window without a word or beyond every track is undecided (pred -1, prob NaN); a track
    that has ended gets prob 0.  One scene (contents a (W, D) array) or a list of scenes (-> a list of dicts); one jg_asd_windows call."""
    single = not isinstance(contents, (list, tuple))
    if single:
        contents, word_boundaries, tracks = [contents], [word_boundaries], [tracks]
    if not len(contents):
        return []
    if win < 1 or hop < 1:
        raise ValueError("win and hop must be >= 1")
    eng = engine or Engine.get()
    flat = [t for scene in tracks for t in scene]
    s_off = np.zeros(len(tracks) + 1, np.int64)
    s_off[1:] = np.cumsum([len(scene) for scene in tracks])
    start, end = batch_bounds(word_boundaries, contents)
    prob, p_off, pred, w_off, _ = eng.asd_windows(cat_rows(flat), offsets_of(flat), cat_rows(contents), offsets_of(contents), np.arange(len(flat)), s_off,
                                                  win=win, hop=hop, word_start=start, word_end=end, temp=temp)
    prob, pred = to_host(prob), to_host(pred)
    out = []
    for i, scene in enumerate(tracks):
        w = span(w_off, i)
        n_win = w.stop - w.start
        out.append(dict(start=window_starts(n_win, win, hop), prob=prob[span(p_off, i)].reshape(n_win, len(scene)), pred=pred[w]))
    return out[0] if single else out


def _talk_call(gesture, content, word_boundaries, reach, temp, normalize, engine, want_band):
    """One Engine.attn_talk call for a track or a list of tracks -> per track a dict of host arrays"""
    single = not isinstance(gesture, (list, tuple))
    if single:
        gesture, content, word_boundaries = [gesture], [content], [word_boundaries]
    if not (len(gesture) == len(content) == len(word_boundaries)):
        raise ValueError("one content array and one list of word boundaries per track")
    if not len(gesture):
        return []
    start, end = batch_bounds(word_boundaries, content)
    eng = engine or Engine.get()
    goff, coff = offsets_of(gesture).astype(np.int64), offsets_of(content).astype(np.int64)
    band, bf, bs, fw, fp = eng.attn_talk(cat_rows(gesture), cat_rows(content), goff, coff, start, end, reach=reach, temp=temp, normalize=normalize,
                                         want_band=want_band)
    bf, bs, fw, fp = to_host(bf), to_host(bs), to_host(fw), to_host(fp)
    band = to_host(band) if want_band else None
    out = []
    for i in range(len(gesture)):
        w, f = span(coff, i), span(goff, i)
        d = dict(best_frame=bf[w], best_score=bs[w], frame_word=fw[f], frame_prob=fp[f])
        if want_band:
            d.update(first_frame=(start[w] - int(reach)).astype(np.int32), band=band[w])
        out.append(d)
    return out[0] if single else out


def talk_heatmap(gesture, content, word_boundaries, reach=110, temp=0.07, normalize=True, engine=None):
    """The gesture-word heat map along a whole talk: a track's frame rows (T, D) -- embed_tracks' gesture_emb, of any length up to 2^20 --
    against the W word rows of its transcript, word_boundaries = [word, start, end] triplets (or (start, end) pairs) with inclusive
    frames on the track's axis, in transcript order.  Word w is in reach of frame f iff start_w - reach <= f <= end_w + reach, and the
    softmax of a frame runs over the words in reach of it: every frame sees the words a clip of 2 reach + 1 frames centred on it would
    contain (the clip form, attention_matrices, runs its softmax over all words of a clip of at most 220 frames, which is what the
    model was trained on; reach = 110 is half of that, a choice and not a measured optimum).  One track, or lists of tracks (-> a
    list); one jg_attn_talk call for the batch.
    Returns per track a dict of host arrays: band (W, 2 reach + longest word) float32 with band[w][j] = the probability of word w at
    frame first_frame[w] + j (NaN outside the track, beyond end_w + reach, or undecided); first_frame (W,) int32 = start_w - reach;
    best_frame (W,) int32 / best_score (W,) float32: the word's first arg-max frame and that probability (-1 / NaN without a frame);
    frame_word (T,) int32 / frame_prob (T,) float32: the frame's most probable word and its probability (-1 / NaN when no word is in
    reach).  More than 128 words in reach of a block of 128 frames is refused (ValueError): lower reach."""
    return _talk_call(gesture, content, word_boundaries, reach, temp, normalize, engine, True)


def spot_talk(gesture, content, word_boundaries, reach=110, temp=0.07, normalize=True, engine=None):
    """talk_heatmap without the band: every word of a talk localised (best_frame, best_score) and every frame labelled (frame_word,
    frame_prob); the band is not written (jg_attn_talk with band = NULL)."""
    return _talk_call(gesture, content, word_boundaries, reach, temp, normalize, engine, False)


def talk_words(utterances, starts):
    """The word rows of a talk from its utterances: `utterances` are feature dicts {"content_emb" (W_i, 512), "info": {word_boundaries}} as
    extract_jegal_embs / inference_embs --modalities ta write them from wav and text alone (the utterance is the unit the content encoders
    were trained on), `starts` the first frame of each utterance on the talk's frame axis.  Returns (content (sum W, 512) float32, bounds =
    [[word, start, end]] on the talk's axis), utterances in the order of their starts.  Raises ValueError when the shifted boundaries are
    not in order (utterances that overlap out of order), or when an utterance's boundaries do not match its content rows."""
    starts = np.asarray(starts, np.int64).reshape(-1)
    if len(utterances) != starts.size:
        raise ValueError("one start frame per utterance")
    rows, bounds = [], []
    for i in np.argsort(starts, kind="stable"):
        u = utterances[int(i)]
        if u.get("content_emb") is None:
            raise ValueError("utterance {} holds no content_emb".format(int(i)))
        c = np.asarray(u["content_emb"], np.float32)
        words, s, e = word_bounds(u["info"]["word_boundaries"])
        check_word_count(len(words), len(c), "utterance {}".format(int(i)))
        rows.append(c)
        bounds += [[w, int(a) + int(starts[i]), int(b) + int(starts[i])] for w, a, b in zip(words, s, e)]
    s, e = np.asarray([b[1] for b in bounds], np.int64), np.asarray([b[2] for b in bounds], np.int64)
    if (np.diff(s) < 0).any() or (np.diff(e) < 0).any() or (s > e).any():
        raise ValueError("the utterances overlap out of order: the shifted word boundaries are not non-decreasing")
    content = np.concatenate(rows, 0) if rows else np.zeros((0, 512), np.float32)
    return content, bounds
