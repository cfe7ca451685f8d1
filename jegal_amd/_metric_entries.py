"""The metric entries of the engine (jg_pool_mean .. jg_asd_windows) as a class that Engine (_lib.py) inherits from, with the one set of
argument rules they share.  Every check comes before the wrapper touches its handle or the device."""
import ctypes

import numpy as np
import torch

# The limits the C entries refuse on, named as in csrc/shared.h (tests/test_metric_entries_cpu.py keeps the two equal).
SIM_TOPK_MAX_K = 128
SIM_SEARCH_MAX_SLICES, SIM_SEARCH_MAX_WS = 1024, 64 << 20
COUPLING_MAX_W = 64
SPOT_MAX_W, SPOT_MAX_T = 1024, 8192
SYNC_MAX_R, SYNC_MAX_T, SYNC_MAX_D = 64, 8192, 1024
SYNCW_MAX_T, SYNCW_MAX_WINDOWS, SYNCW_MAX_BAND_LOG2 = 1 << 20, 1 << 20, 40
ASDW_MAX_D, ASDW_MAX_P, ASDW_MAX_WIN = 1024, 64, 8192
TALK_MAX_T, TALK_MAX_REACH, TALK_MAX_BLOCK_W = 1 << 20, 1024, 128
LIMITS = {k: v for k, v in globals().items() if k.isupper()}
INT32_MAX = 2 ** 31 - 1
TALK_FB = 128        # frames per block of jg_attn_talk (csrc/spotting.hip), aligned to the track's first frame


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _shape(x):
    """The shape of a tensor, an array or nested lists, without moving anything."""
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _row_pair(a, b, names, multiple=64, max_D=None):
    """Two (rows, D) operands with the same D >= 1, a multiple of `multiple` and at most max_D -> their shapes."""
    sa, sb = _shape(a), _shape(b)
    if len(sa) != 2 or len(sb) != 2 or sa[1] != sb[1] or sa[1] < 1 or sa[1] % multiple or (max_D and sa[1] > max_D):
        raise ValueError(f"{names} must be (rows, D) with the same D" + (f", a positive multiple of {multiple}" if multiple > 1 else "")
                         + (f", at most {max_D}" if max_D else ""))
    return sa, sb


def _offsets(offsets, rows, name, n=None, host=True):
    """Row offsets of `name` -> int64 host array: 1-d integers, n + 1 entries when the caller knows n, a non-decreasing partition inside
    0 .. rows (rows None: any end), int32 range.  host=False: the entry also takes a tensor, whose values are not read (no sync): only its
    shape and type are looked at, as the C entry takes it, and it comes back as it is.  Blocks = len(result) - 1."""
    dev = not host and isinstance(offsets, torch.Tensor)
    off = offsets if dev else np.asarray(offsets)
    if off.ndim != 1 or len(off) < 1 or not (off.dtype in (torch.int32, torch.int64) if dev else np.issubdtype(off.dtype, np.integer)):
        raise ValueError(f"{name} must be 1-d integers, blocks + 1 entries")
    if n is not None and len(off) != n + 1:
        raise ValueError(f"{name} needs {n + 1} entries (blocks + 1), not {len(off)}")
    if dev:
        return off
    off = off.astype(np.int64)
    if off[0] < 0 or off[-1] > (INT32_MAX if rows is None else min(rows, INT32_MAX)) or np.any(np.diff(off) < 0):
        raise ValueError(f"{name} must be non-decreasing and lie inside 0 .. rows (int32)")
    return off


def _within(lens, lo, hi, what):
    """Block lengths (or counts), each within lo .. hi -> the same."""
    if lens.size and (lens.min() < lo or lens.max() > hi):
        raise ValueError(f"{what}: {lo}..{hi} each")
    return lens


def _ragged(counts, what=None):
    """Counts -> the int64 offsets of their ragged blocks (one entry more); with `what` (the device takes them as int32): int32 range."""
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    if what and off[-1] > INT32_MAX:
        raise ValueError(f"more than 2^31 {what} in one call")
    return off


def _ints(a):
    return np.asarray(a, np.int64).reshape(-1)


class MetricEntries:
    """Engine's metric methods.  Uses Engine's handle (lib, h, device) and helpers (_ck, _bind_stream, _f32, _i32)."""

    def pool_mean(self, x, offsets):
        xs = _shape(x)
        if len(xs) != 2 or xs[1] < 1:
            raise ValueError("x must be (rows, D)")
        n = len(_offsets(offsets, xs[0], "offsets", host=False)) - 1
        self._bind_stream()
        x, off = self._f32(x), self._i32(offsets)
        out = torch.empty((n, x.shape[-1]), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_pool_mean(self.h, _ptr(x), _ptr(off), n, x.shape[-1], _ptr(out)))
        return out

    def sim_rank(self, e1, e2, row_offset=0):
        s1, s2 = _row_pair(e1, e2, "e1 / e2")
        row_offset = int(row_offset)
        if row_offset < 0 or row_offset + s1[0] > s2[0]:
            raise ValueError("row_offset must be >= 0 and row_offset + rows of e1 <= rows of e2")
        self._bind_stream()
        e1, e2 = self._f32(e1), self._f32(e2)
        n_local, D = e1.shape
        rank, ties = (torch.empty(n_local, dtype=torch.int32, device=self.device) for _ in range(2))
        self._ck(self.lib.jg_sim_rank(self.h, _ptr(e1), _ptr(e2), n_local, e2.shape[0], row_offset, D, _ptr(rank), _ptr(ties)))
        return rank, ties

    def _sim_topk_args(self, entry, queries, gallery, k, gallery_offset, merge_into, g_offsets=None):
        """What sim_topk and sim_topk_grouped (`entry`; the latter passes g_offsets) share: the checks of the shapes, k, gallery_offset,
        the group offsets and merge_into, then the stream, and the result to fill: merge_into's pair, or an empty one (-1 / -inf).
        Returns (rows of queries, rows of gallery, D, k, gallery_offset, groups or None, idx, score)."""
        qs, gs = _row_pair(queries, gallery, "queries / gallery")
        k, gallery_offset = int(k), int(gallery_offset)
        if not 1 <= k <= SIM_TOPK_MAX_K:
            raise ValueError(f"jg_{entry} limit: 1 <= k <= {SIM_TOPK_MAX_K}")
        if gallery_offset < 0 or gallery_offset + gs[0] > INT32_MAX:
            raise ValueError("gallery_offset must be >= 0 and gallery_offset + gallery rows <= INT32_MAX")
        n_groups = None if g_offsets is None else len(_offsets(g_offsets, gs[0], "g_offsets", host=False)) - 1
        if merge_into is not None:
            if not isinstance(merge_into, (tuple, list)) or len(merge_into) != 2 or not all(isinstance(t, torch.Tensor) for t in merge_into):
                raise ValueError(f"merge_into must be the (idx, score) pair of an earlier {entry} call")
            idx, score = merge_into
            if (tuple(idx.shape) != (qs[0], k) or tuple(score.shape) != (qs[0], k) or idx.dtype != torch.int32 or score.dtype != torch.float32
                    or not idx.is_contiguous() or not score.is_contiguous()):
                raise ValueError(f"merge_into must be contiguous (idx int32, score float32) tensors of shape ({qs[0]}, {k})")
            if idx.device != self.device or score.device != self.device:
                raise ValueError(f"merge_into must be on {self.device}")
        self._bind_stream()
        if merge_into is None:
            idx = torch.full((qs[0], k), -1, dtype=torch.int32, device=self.device)
            score = torch.full((qs[0], k), float("-inf"), dtype=torch.float32, device=self.device)
        return qs[0], gs[0], qs[1], k, gallery_offset, n_groups, idx, score

    def sim_topk(self, queries, gallery, k, gallery_offset=0, merge_into=None):
        """jg_sim_topk: per query row the k gallery rows with the largest <q_i, g_j> (rows as stored: normalise first, as for sim_rank), best
        first; on equal scores the smaller gallery row first.  queries (n, D) / gallery (m, D), D % 64 == 0, 1 <= k <= 128.
        Returns (idx (n, k) int32 = gallery_offset + j, score (n, k) float32) as device tensors; slots beyond the candidates are -1 / -inf.
        merge_into = (idx, score) of an earlier call with the same queries and k on OTHER gallery rows: the two are updated in place to the
        best k of the union and returned (a gallery too large for the device goes through in pieces, each with its gallery_offset)."""
        n, m, D, k, gallery_offset, _, idx, score = self._sim_topk_args("sim_topk", queries, gallery, k, gallery_offset, merge_into)
        q, g = self._f32(queries), self._f32(gallery)
        if n and m:                                    # (no gallery row: nothing to merge, or the empty result)
            self._ck(self.lib.jg_sim_topk(self.h, _ptr(q), _ptr(g), n, m, D, k, gallery_offset, int(merge_into is not None), _ptr(idx), _ptr(score)))
        return idx, score

    def sim_topk_grouped(self, queries, gallery, g_offsets, k, gallery_offset=0, merge_into=None):
        """jg_sim_topk_grouped: the gallery rows are cut into contiguous groups (group i = rows g_offsets[i] .. g_offsets[i + 1] - 1 of
        `gallery`; a host array or a tensor of groups + 1 entries), a group scores as its best row, and per query row the k best groups come
        back, each as the row that earned the score: (idx (n, k) int32 = gallery_offset + row, score (n, k) float32), device tensors, best
        first, on equal scores the smaller row; never two rows of one group; -1 / -inf where fewer than k groups have a row.  Scores are
        those of sim_topk / sim_rank bit for bit.  merge_into = (idx, score) of an earlier call with the same queries and k on OTHER
        gallery rows, cut at group boundaries: updated in place to the best k of the union and returned."""
        n, m, D, k, gallery_offset, n_groups, idx, score = self._sim_topk_args("sim_topk_grouped", queries, gallery, k, gallery_offset,
                                                                               merge_into, g_offsets)
        q, g, off = self._f32(queries), self._f32(gallery), self._i32(g_offsets)
        if n and m and n_groups:                       # (no gallery row, no group: nothing to merge, or the empty result)
            self._ck(self.lib.jg_sim_topk_grouped(self.h, _ptr(q), _ptr(g), n, m, D, k, _ptr(off), n_groups, gallery_offset,
                                                  int(merge_into is not None), _ptr(idx), _ptr(score)))
        return idx, score

    def sim_search(self, queries, gallery, k, g_offsets=None, gallery_offset=0, merge_into=None, slices=0):
        """jg_sim_search: sim_topk (g_offsets None) or sim_topk_grouped over a gallery of float32 or float16 rows (a tensor or an array; a
        float16 gallery is searched as stored and gives the bits of the call on gallery.float()) that the device walks in `slices` slices at
        once, one workgroup per 64 query rows and slice (0: the library chooses, search_plan in _lib.py); the bits do not depend on the
        slices.  The other arguments and the (idx, score) result are those of the two entries; a gallery that is a contiguous tensor on
        the engine's device is used where it lies."""
        dtype = getattr(gallery, "dtype", None)
        if dtype not in (torch.float32, torch.float16, np.dtype(np.float32), np.dtype(np.float16)):
            raise ValueError("gallery must be a float32 or float16 tensor or array")
        slices = int(slices)
        if not 0 <= slices <= SIM_SEARCH_MAX_SLICES:
            raise ValueError(f"jg_sim_search limit: 0 <= slices <= {SIM_SEARCH_MAX_SLICES} (0: the library chooses)")
        qs, gs = _shape(queries), _shape(gallery)
        if slices and len(qs) == 2 and len(gs) == 2 and 1 <= int(k) <= SIM_TOPK_MAX_K and gs[0] <= INT32_MAX:
            from ._lib import JegalError, search_plan      # (the planner is a host function of the library: no handle, no device)
            try:
                search_plan(qs[0], gs[0], int(k), slices=slices)
            except JegalError:
                raise ValueError(f"jg_sim_search limit: {slices} slices of {qs[0]} x {int(k)} keys exceed {SIM_SEARCH_MAX_WS} bytes") from None
        n, m, D, k, gallery_offset, n_groups, idx, score = self._sim_topk_args("sim_search", queries, gallery, k, gallery_offset, merge_into,
                                                                               g_offsets)
        q, g = self._f32(queries), torch.as_tensor(gallery, device=self.device).contiguous()
        off = None if g_offsets is None else self._i32(g_offsets)
        if n and m and n_groups != 0:                  # (no gallery row, no group: nothing to merge, or the empty result)
            self._ck(self.lib.jg_sim_search(self.h, _ptr(q), n, _ptr(g), 1 if g.dtype == torch.float16 else 0, m, D, k, _ptr(off), n_groups or 0,
                                            gallery_offset, int(merge_into is not None), slices, _ptr(idx), _ptr(score)))
        return idx, score

    def sim_coupling(self, words, w_offsets, gallery, g_offsets, k, group_offset=0, merge_into=None, slices=0, want_matrix=False):
        """jg_sim_coupling (late interaction): query q = the word rows w_offsets[q] .. w_offsets[q + 1] - 1 of `words` (a HOST array of
        queries + 1 entries, 1..64 rows each), group g = the rows g_offsets[g] .. g_offsets[g + 1] - 1 of `gallery` (float32 or float16 rows;
        a host array or a tensor of groups + 1 entries).  A group scores as the mean over the query's words of each word's best row in it
        (rows as stored: normalise first); per query the k best groups come back: (idx (n, k) int32 = group_offset + g, score (n, k)
        float32), device tensors, best first, on equal scores the smaller group, -1 / -inf where fewer groups have a score.  A score's bits
        depend on its query's and its group's rows only.  merge_into = (idx, score) of an earlier call with the same queries and k on OTHER
        groups (group_offset): updated in place to the best k of the union.  slices as for sim_search.  want_matrix: also the
        (n, groups) matrix of all scores of this call (NaN where a pair has none), a transposed view of the group-major buffer."""
        return self._sim_coupling("sim_coupling", words, w_offsets, gallery, g_offsets, k, group_offset, merge_into, slices, want_matrix)

    def sim_ordered(self, words, w_offsets, gallery, g_offsets, k, group_offset=0, merge_into=None, slices=0, want_matrix=False):
        """jg_sim_ordered: sim_coupling with the words of a query assigned to rows of the group in word order -- the score is the best mean
        of <word i, row t_i> over t_1 <= t_2 <= .. <= t_W (one row may serve consecutive words), the sum one float32 chain in word order.
        Arguments, checks and returns are sim_coupling's; a score never exceeds sim_coupling's and equals it where the words' best rows
        are in order already."""
        return self._sim_coupling("sim_ordered", words, w_offsets, gallery, g_offsets, k, group_offset, merge_into, slices, want_matrix)

    def _phrase_operands(self, entry, words, w_offsets, gallery, g_offsets, group_offset):
        """What sim_coupling, sim_ordered and sim_align check of their shared operands before anything else
        -> (shape of words, shape of gallery, host w_offsets, queries, groups, group_offset)"""
        dtype = getattr(gallery, "dtype", None)
        if dtype not in (torch.float32, torch.float16, np.dtype(np.float32), np.dtype(np.float16)):
            raise ValueError("gallery must be a float32 or float16 tensor or array")
        group_offset = int(group_offset)
        ws, gs = _row_pair(words, gallery, "words / gallery")
        woh = _offsets(w_offsets, ws[0], "w_offsets")
        if woh[0] != 0:
            raise ValueError("w_offsets must start at 0")
        _within(np.diff(woh), 1, COUPLING_MAX_W, f"jg_{entry} limits: word rows per query")
        n_groups = len(_offsets(g_offsets, gs[0], "g_offsets", host=False)) - 1
        if group_offset < 0 or group_offset + n_groups > INT32_MAX:
            raise ValueError("group_offset must be >= 0 and group_offset + groups <= INT32_MAX")
        return ws, gs, woh, woh.size - 1, n_groups, group_offset

    def _sim_coupling(self, entry, words, w_offsets, gallery, g_offsets, k, group_offset, merge_into, slices, want_matrix):
        """The body of sim_coupling and sim_ordered (`entry`): the two differ in the C entry they call and in nothing else."""
        if getattr(gallery, "dtype", None) is None:        # (first, as ever: _phrase_operands names the types)
            raise ValueError("gallery must be a float32 or float16 tensor or array")
        slices = int(slices)
        if not 0 <= slices <= SIM_SEARCH_MAX_SLICES:
            raise ValueError(f"jg_{entry} limit: 0 <= slices <= {SIM_SEARCH_MAX_SLICES} (0: the library chooses)")
        ws, gs, woh, n, n_groups, group_offset = self._phrase_operands(entry, words, w_offsets, gallery, g_offsets, group_offset)
        if slices and 1 <= int(k) <= SIM_TOPK_MAX_K and gs[0] <= INT32_MAX:
            from ._lib import JegalError, coupling_plan    # (the planner is a host function of the library: no handle, no device)
            try:
                coupling_plan(woh, gs[0], int(k), slices=slices)
            except JegalError:
                raise ValueError(f"jg_{entry} limit: {slices} slices of {n} x {int(k)} keys exceed {SIM_SEARCH_MAX_WS} bytes") from None
        # k and merge_into as the top-k entries check them, with one row of the result per QUERY: (n, D) stands for the queries
        _, m, D, k, _, _, idx, score = self._sim_topk_args(entry, np.broadcast_to(np.float32(0), (n, ws[1])), gallery, k, 0, merge_into)
        w, g, off = self._f32(words), torch.as_tensor(gallery, device=self.device).contiguous(), self._i32(g_offsets)
        pair = torch.full((n_groups, n), float("nan"), dtype=torch.float32, device=self.device) if want_matrix else None
        if n and m and n_groups:                       # (no gallery row, no group: nothing to merge, or the empty result)
            wo = np.ascontiguousarray(woh, np.int32)
            self._ck(getattr(self.lib, "jg_" + entry)(self.h, _ptr(w), wo.ctypes.data_as(ctypes.c_void_p), n, _ptr(g),
                                                      1 if g.dtype == torch.float16 else 0, m, D, k, _ptr(off), n_groups, group_offset,
                                                      int(merge_into is not None), slices, _ptr(idx), _ptr(score), _ptr(pair), n))
        return (idx, score, pair.t()) if want_matrix else (idx, score)

    def sim_align(self, words, w_offsets, gallery, g_offsets, idx, ordered, group_offset=0, into=None):
        """jg_sim_align: the rows behind a result of sim_coupling (ordered False) or sim_ordered (True).  words .. g_offsets and group_offset:
        the operands of that call; idx (n, k) int32 on the device: its result.  Returns device tensors (frames (n, k, Wmax) int32, score
        (n, k) float32), Wmax = the longest query: frames[q, r, i] = the row of `gallery` that word i of query q took in the group idx[q, r]
        (-1 behind the query's words, or where the pair has no score or the group more than 8192 rows), score the pair's score with the bits
        of the call that made idx.  Only slots whose idx lies in group_offset .. group_offset + groups - 1 are written; the others keep -1
        / NaN, or what `into` = (frames, score) of an earlier call held: merged pieces are aligned piece by piece with the final idx."""
        ws, gs, woh, n, n_groups, group_offset = self._phrase_operands("sim_align", words, w_offsets, gallery, g_offsets, group_offset)
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.ndim != 2 or idx.shape[0] != n or not idx.is_contiguous():
            raise ValueError(f"idx must be the contiguous int32 ({n}, k) tensor of sim_coupling or sim_ordered")
        k = int(idx.shape[1])
        if not 1 <= k <= SIM_TOPK_MAX_K:
            raise ValueError(f"jg_sim_align limit: 1 <= k <= {SIM_TOPK_MAX_K}")
        wmax = int(np.diff(woh).max()) if n else 1
        if into is not None:
            if not isinstance(into, (tuple, list)) or len(into) != 2 or not all(isinstance(t, torch.Tensor) for t in into):
                raise ValueError("into must be the (frames, score) pair of an earlier sim_align call")
            frames, score = into
            if (tuple(frames.shape) != (n, k, wmax) or tuple(score.shape) != (n, k) or frames.dtype != torch.int32 or score.dtype != torch.float32
                    or not frames.is_contiguous() or not score.is_contiguous()):
                raise ValueError(f"into must be contiguous (frames int32 ({n}, {k}, {wmax}), score float32 ({n}, {k})) tensors")
        if idx.device != self.device or (into is not None and (frames.device != self.device or score.device != self.device)):
            raise ValueError(f"idx and into must be on {self.device}")
        self._bind_stream()
        if into is None:
            frames = torch.full((n, k, wmax), -1, dtype=torch.int32, device=self.device)
            score = torch.full((n, k), float("nan"), dtype=torch.float32, device=self.device)
        w, g, off = self._f32(words), torch.as_tensor(gallery, device=self.device).contiguous(), self._i32(g_offsets)
        if n and gs[0] and n_groups:
            wo = np.ascontiguousarray(woh, np.int32)
            self._ck(self.lib.jg_sim_align(self.h, _ptr(w), wo.ctypes.data_as(ctypes.c_void_p), n, _ptr(g), 1 if g.dtype == torch.float16 else 0,
                                           gs[0], ws[1], _ptr(off), n_groups, group_offset, _ptr(idx), k, int(bool(ordered)), _ptr(frames), wmax,
                                           _ptr(score)))
        return frames, score

    def group_of_rows(self, idx, g_offsets, gallery_offset=0):
        """jg_group_of_rows: the rows sim_topk_grouped returned (an int32 tensor of any shape) -> (grp, pos) int32 device tensors of that
        shape: the group whose range holds idx - gallery_offset and the row's place inside it; -1 / -1 for idx < 0 or a row in no group.
        After merged calls: the offsets of the whole gallery with gallery_offset = 0."""
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32:
            raise ValueError("idx must be an int32 tensor (the idx of sim_topk_grouped)")
        gallery_offset = int(gallery_offset)
        if not 0 <= gallery_offset <= INT32_MAX:
            raise ValueError("gallery_offset must be 0 .. INT32_MAX")
        n_groups = len(_offsets(g_offsets, None, "g_offsets", host=False)) - 1
        self._bind_stream()
        rows, off = self._i32(idx), self._i32(g_offsets)
        grp, pos = torch.full_like(rows, -1), torch.full_like(rows, -1)
        if rows.numel():
            self._ck(self.lib.jg_group_of_rows(self.h, _ptr(rows), rows.numel(), _ptr(off), n_groups, gallery_offset, _ptr(grp), _ptr(pos)))
        return grp, pos

    def spot(self, gesture, content, g_offsets, c_offsets, targets, temp=0.07):
        gs, cs = _row_pair(gesture, content, "gesture / content", multiple=1)
        tgh = _ints(targets)
        n = tgh.size
        goh, coh = _offsets(g_offsets, gs[0], "g_offsets", n), _offsets(c_offsets, cs[0], "c_offsets", n)
        _within(np.diff(goh), 1, SPOT_MAX_T, "jg_spot limits: frames per clip")
        W = _within(np.diff(coh), 1, SPOT_MAX_W, "jg_spot limits: words per clip")
        if (tgh < 0).any() or (tgh >= W).any():
            raise ValueError("jg_spot limits: 0 <= target < words")
        self._bind_stream()
        g, c = self._f32(gesture), self._f32(content)
        go, co, tg = self._i32(goh), self._i32(coh), self._i32(tgh)
        pred = torch.empty(n, dtype=torch.int32, device=self.device)
        score = torch.empty(n, dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_spot(self.h, _ptr(g), _ptr(c), _ptr(go), _ptr(co), _ptr(tg), n, gs[1], temp, _ptr(pred), _ptr(score)))
        return pred, score

    def attn_matrix(self, gesture, content, g_offsets, c_offsets, temp=0.07, normalize=True, want_matrix=True):
        """jg_attn_matrix: per clip A_i = softmax((G_i C_i^T) / temp, dim=1)^T (W_i, T_i) and, for every word, its first arg-max frame and
        that probability.  gesture (sum T, D) / content (sum W, D); g_offsets / c_offsets: HOST arrays of n + 1 entries.
        Returns (A_flat | None, a_offsets, best_frame, best_score): clip i's matrix is A_flat[a_offsets[i] : a_offsets[i + 1]].reshape(W_i, T_i)
        (a_offsets: host int64, n + 1 entries), best_* are device tensors indexed like content's rows (c_offsets[-1] entries: clip i's words
        are best_*[c_offsets[i] : c_offsets[i + 1]]; entries no clip covers are -1 / NaN).  want_matrix=False: no matrix is written."""
        gs, cs = _row_pair(gesture, content, "gesture / content")
        goh = _offsets(g_offsets, gs[0], "g_offsets")
        n = goh.size - 1
        coh = _offsets(c_offsets, cs[0], "c_offsets", n)
        T = _within(np.diff(goh), 1, SPOT_MAX_T, "jg_attn_matrix limits: frames per clip")
        W = _within(np.diff(coh), 1, SPOT_MAX_W, "jg_attn_matrix limits: words per clip")
        if not temp > 0:
            raise ValueError("temp must be positive")
        a_off = _ragged(T * W)
        self._bind_stream()
        g, c = self._f32(gesture), self._f32(content)
        A = torch.empty(int(a_off[-1]), dtype=torch.float32, device=self.device) if want_matrix else None
        best_frame = torch.full((int(coh[-1]),), -1, dtype=torch.int32, device=self.device)
        best_score = torch.full((int(coh[-1]),), float("nan"), dtype=torch.float32, device=self.device)
        if n == 0:
            return A, a_off, best_frame, best_score
        go, co = self._i32(goh), self._i32(coh)
        ao = torch.as_tensor(a_off[:-1].copy(), device=self.device) if want_matrix else None
        self._ck(self.lib.jg_attn_matrix(self.h, _ptr(g), _ptr(c), _ptr(go), _ptr(co), n, gs[1], int(T.max()), float(temp),
                                         int(bool(normalize)), _ptr(A), _ptr(ao), _ptr(best_frame), _ptr(best_score)))
        return A, a_off, best_frame, best_score

    @staticmethod
    def talk_block_candidates(T, start, end, reach):
        """jg_attn_talk's candidates per block of 128 frames of ONE track of T frames whose words have the inclusive bounds start / end
        (non-decreasing): the number of words in reach of any frame of the block, as the kernel's two searches count them."""
        start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
        f0 = np.arange(0, max(int(T), 0), TALK_FB, dtype=np.int64)
        last = np.minimum(f0 + TALK_FB, T) - 1
        lo = np.searchsorted(end + reach, f0, side="left")
        hi = np.searchsorted(start - reach, last, side="right")
        return np.maximum(hi - lo, 0)

    def attn_talk(self, gesture, content, g_offsets, c_offsets, word_start, word_end, reach=110, temp=0.07, normalize=True, want_band=True,
                  want_best=True, want_frames=True):
        """jg_attn_talk: the gesture-word heat map along whole tracks.  gesture (sum T, D) / content (sum W, D); g_offsets / c_offsets: HOST
        arrays of n + 1 entries; word_start / word_end: one inclusive frame bound per content row, on the frame axis of the word's track,
        non-decreasing along a track.  Word w is in reach of frame f iff start_w - reach <= f <= end_w + reach, and every frame's softmax
        runs over the words in reach of it.
        Returns device tensors (band (sum W, 2 reach + longest word) | None, best_frame, best_score (sum W,) | None, frame_word, frame_prob
        (sum T,) | None): band[w][j] is the word's probability at frame start_w - reach + j (NaN outside the track or beyond end_w + reach),
        best_* its first arg-max frame and that probability (-1 / NaN without a frame), frame_* the frame's arg-max word counted from
        the track's first word and its probability (-1 / NaN when no word is in reach).  Content rows no track covers read NaN / -1."""
        reach = int(reach)
        if not 0 <= reach <= TALK_MAX_REACH:
            raise ValueError(f"jg_attn_talk limits: reach 0..{TALK_MAX_REACH}")
        if not temp > 0:
            raise ValueError("temp must be positive")
        if not (want_band or want_best or want_frames):
            raise ValueError("no output asked for")
        gs, cs = _row_pair(gesture, content, "gesture / content")
        goh = _offsets(g_offsets, gs[0], "g_offsets")
        n = goh.size - 1
        coh = _offsets(c_offsets, cs[0], "c_offsets", n)
        T = _within(np.diff(goh), 0, TALK_MAX_T, "jg_attn_talk limits: frames per track")
        wsh, weh = _ints(word_start), _ints(word_end)
        if wsh.size != cs[0] or weh.size != cs[0] or (cs[0] and max(np.abs(wsh).max(), np.abs(weh).max()) > INT32_MAX):
            raise ValueError("word_start / word_end need one int32 entry per content row")
        if (wsh > weh).any():
            raise ValueError("word_start must be <= word_end")
        for i in range(n):
            s, e = wsh[coh[i]:coh[i + 1]], weh[coh[i]:coh[i + 1]]
            if (np.diff(s) < 0).any() or (np.diff(e) < 0).any():
                raise ValueError(f"track {i}: word_start / word_end must be non-decreasing (transcript order)")
            cand = self.talk_block_candidates(T[i], s, e, reach)
            if cand.size and cand.max() > TALK_MAX_BLOCK_W:
                raise ValueError(f"track {i}: {int(cand.max())} words in reach of the {TALK_FB} frames from {int(cand.argmax()) * TALK_FB}; "
                                 f"jg_attn_talk decides at most {TALK_MAX_BLOCK_W} per block: lower reach")
        pitch = 2 * reach + (int((weh - wsh).max()) + 1 if cs[0] else 1)
        if want_band and cs[0] * pitch > INT32_MAX:
            raise ValueError("jg_attn_talk limits: content rows x (2 reach + longest word) < 2^31")
        self._bind_stream()
        nan = float("nan")
        band = torch.full((cs[0], pitch), nan, dtype=torch.float32, device=self.device) if want_band else None
        best_frame = torch.full((cs[0],), -1, dtype=torch.int32, device=self.device) if want_best else None
        best_score = torch.full((cs[0],), nan, dtype=torch.float32, device=self.device) if want_best else None
        frame_word = torch.full((gs[0],), -1, dtype=torch.int32, device=self.device) if want_frames else None
        frame_prob = torch.full((gs[0],), nan, dtype=torch.float32, device=self.device) if want_frames else None
        if n and gs[0] and cs[0]:                      # (no frame or no word at all: every output is the undecided value already)
            g, c = self._f32(gesture), self._f32(content)
            go, co, ws, we = (self._i32(a) for a in (goh, coh, wsh, weh))
            self._ck(self.lib.jg_attn_talk(self.h, _ptr(g), _ptr(go), n, gs[0], max(int(T.max()), 1), _ptr(c), _ptr(co), cs[0], _ptr(ws), _ptr(we),
                                           gs[1], reach, float(temp), int(bool(normalize)), _ptr(band), pitch, _ptr(best_frame),
                                           _ptr(best_score), _ptr(frame_word), _ptr(frame_prob)))
        return band, best_frame, best_score, frame_word, frame_prob

    def sync_offset(self, vid, aud, v_offsets, a_offsets, max_shift=15, min_overlap=1, want_curve=True):
        """jg_sync_offset: per clip the audio-visual offset (frames; d > 0: audio row t + d matches video row t), its confidence
        (max - median of the curve) and the curve of mean cosines over the shifts -max_shift .. max_shift.  vid (sum Tv, D) / aud (sum Ta, D)
        rows as stored; v_offsets / a_offsets: n + 1 row offsets each (host arrays or device int32 tensors).
        Returns device tensors (offset (n,) int32, conf (n,) fp32, curve (n, 2 max_shift + 1) fp32 or None).  A clip with no rows, more than
        8192 rows, or no shift with min_overlap pairs: offset 0, conf NaN, NaN curve."""
        R, mo = int(max_shift), int(min_overlap)
        if not 0 <= R <= SYNC_MAX_R or mo < 1:
            raise ValueError(f"jg_sync_offset limits: max_shift 0..{SYNC_MAX_R}, min_overlap >= 1")
        vs, as_ = _row_pair(vid, aud, "vid / aud", max_D=SYNC_MAX_D)
        n = len(_offsets(v_offsets, vs[0], "v_offsets", host=False)) - 1
        _offsets(a_offsets, as_[0], "a_offsets", n, host=False)
        self._bind_stream()
        v, a = self._f32(vid), self._f32(aud)
        vo, ao = self._i32(v_offsets), self._i32(a_offsets)
        offset = torch.zeros((n,), dtype=torch.int32, device=self.device)
        conf = torch.full((n,), float("nan"), dtype=torch.float32, device=self.device)
        curve = torch.full((n, 2 * R + 1), float("nan"), dtype=torch.float32, device=self.device) if want_curve else None
        if n == 0 or vs[0] == 0 or as_[0] == 0:          # (no rows at all: every clip is outside the limits)
            return offset, conf, curve
        self._ck(self.lib.jg_sync_offset(self.h, _ptr(v), _ptr(vo), _ptr(a), _ptr(ao), n, vs[1], R, mo, _ptr(curve), _ptr(offset), _ptr(conf)))
        return offset, conf, curve

    @staticmethod
    def sync_window_counts(Tv, win, hop):
        """windows that cover tracks of Tv rows: Tv <= win ? 1 : ceil((Tv - win) / hop) + 1 (win == 0: one)"""
        Tv = np.asarray(Tv, np.int64)
        if not win:
            return np.ones_like(Tv)
        return np.where(Tv <= win, 1, -(-(Tv - win) // hop) + 1)

    def sync_offset_windows(self, vid, aud, v_offsets, a_offsets, a_of=None, max_shift=15, min_overlap=1, win=0, hop=1, n_windows=None,
                            want_curve=True, want_band=False):
        """jg_sync_offset_windows: the audio-visual offset over time.  Clip i is video track i (rows v_offsets[i] : v_offsets[i + 1] of vid)
        against audio track a_of[i] (default: i; rows a_offsets[j] : a_offsets[j + 1] of aud; several clips may name one track); all offsets
        are HOST arrays.  Window j of a clip covers its video rows j hop .. min(j hop + win, Tv) - 1; win == 0: one window over all rows
        (jg_sync_offset's bits).  Clip i gets n_windows[i] windows (default: the count that covers it, sync_window_counts).
        Returns (offset, conf, curve | None, w_offsets, band | None): clip i's windows are the rows w_offsets[i] : w_offsets[i + 1] of
        offset (int32), conf (fp32) and curve (·, 2 max_shift + 1); band (rows of vid, 2 max_shift + 1) holds every cosine (NaN where the
        audio row does not exist), with want_band; device tensors, w_offsets host int64.  A window that begins behind its track or has no
        shift with min_overlap pairs: offset 0, conf NaN.  Tracks may have up to 2^20 rows."""
        R, mo, win, hop = int(max_shift), int(min_overlap), int(win), int(hop)
        if not 0 <= R <= SYNC_MAX_R or mo < 1:
            raise ValueError(f"jg_sync_offset_windows limits: max_shift 0..{SYNC_MAX_R}, min_overlap >= 1")
        if not 0 <= win <= INT32_MAX or (win and not 1 <= hop <= INT32_MAX):
            raise ValueError("jg_sync_offset_windows limits: win >= 0 (0: one window over all rows), hop >= 1")
        vs, as_ = _row_pair(vid, aud, "vid / aud", max_D=SYNC_MAX_D)
        voh, aoh = _offsets(v_offsets, vs[0], "v_offsets"), _offsets(a_offsets, as_[0], "a_offsets")
        n, n_aud = voh.size - 1, aoh.size - 1
        if a_of is None:
            if n_aud != n:
                raise ValueError("without a_of clip i takes audio track i: as many audio tracks as clips")
            aof = np.arange(n, dtype=np.int64)
        else:
            aof = _ints(a_of)
            if aof.size != n or (n and (aof.min() < 0 or aof.max() >= n_aud)):
                raise ValueError("a_of needs one entry per clip, inside 0 .. audio tracks - 1")
        Tv = _within(np.diff(voh), 1, SYNCW_MAX_T, "jg_sync_offset_windows limits: rows per video track")
        Ta = _within(np.diff(aoh)[aof], 1, SYNCW_MAX_T, "jg_sync_offset_windows limits: rows per audio track of a clip")
        if vs[0] * (2 * R + 1) >= 2 ** SYNCW_MAX_BAND_LOG2:
            raise ValueError(f"jg_sync_offset_windows limits: rows of vid x (2 max_shift + 1) < 2^{SYNCW_MAX_BAND_LOG2}")
        nw = self.sync_window_counts(Tv, win, hop) if n_windows is None else _ints(n_windows)
        if nw.size != n or (n and (nw.min() < 1 or nw.max() > SYNCW_MAX_WINDOWS)):
            raise ValueError(f"jg_sync_offset_windows limits: 1..{SYNCW_MAX_WINDOWS} windows per clip, one count per clip")
        w_off = _ragged(nw, "windows")
        self._bind_stream()
        nwin, W = int(w_off[-1]), 2 * R + 1
        offset = torch.zeros((nwin,), dtype=torch.int32, device=self.device)
        conf = torch.full((nwin,), float("nan"), dtype=torch.float32, device=self.device)
        curve = torch.full((nwin, W), float("nan"), dtype=torch.float32, device=self.device) if want_curve else None
        band = torch.full((vs[0], W), float("nan"), dtype=torch.float32, device=self.device) if want_band else None
        if n == 0:
            return offset, conf, curve, w_off, band
        v, a = self._f32(vid), self._f32(aud)
        vo, ao, wo = (self._i32(x) for x in (voh, aoh, w_off))
        af = None if a_of is None else self._i32(aof)
        self._ck(self.lib.jg_sync_offset_windows(self.h, _ptr(v), _ptr(vo), n, vs[0], int(max(Tv.max(), Ta.max())), _ptr(a), _ptr(ao),
                                                 n_aud, _ptr(af), vs[1], R, mo, win, hop, _ptr(wo), int(nw.max()), _ptr(band), _ptr(curve),
                                                 _ptr(offset), _ptr(conf)))
        return offset, conf, curve, w_off, band

    def asd(self, query, cand, c_offsets, temp=0.07):
        qs, cs = _row_pair(query, cand, "query / cand", multiple=1)
        _offsets(c_offsets, cs[0], "c_offsets", qs[0], host=False)
        self._bind_stream()
        q, c, co = self._f32(query), self._f32(cand), self._i32(c_offsets)
        n = q.shape[0]
        pred = torch.empty((n, 3), dtype=torch.int32, device=self.device)
        self._ck(self.lib.jg_asd(self.h, _ptr(q), _ptr(c), _ptr(co), n, q.shape[-1], temp, _ptr(pred)))
        return pred

    def asd_windows(self, gesture, g_offsets, content, c_offsets, trk, s_offsets, win=0, hop=1, n_windows=None, word_start=None,
                    word_end=None, temp=0.07, want_cos=False):
        """jg_asd_windows: per scene and time window the probability that each candidate track gestures to the utterance, and the winner.
        gesture (sum T, D): frame rows of the tracks, g_offsets their n_tracks + 1 row offsets; content (sum W, D): word rows of the scenes'
        utterances, c_offsets (n + 1); trk / s_offsets (n + 1): scene i's candidates are the tracks trk[s_offsets[i] : s_offsets[i + 1]]; all
        offsets are HOST arrays.  win == 0: one window per scene over every frame and word (clip-level ASD).  win > 0: window j covers frames
        j hop .. j hop + win - 1, word_start / word_end (sum W) are the words' inclusive frame bounds, and scene i gets n_windows[i]
        windows (default: ceil(its longest candidate track / hop)).
        Returns (prob, p_offsets, pred, w_offsets, cosv | None): scene i's probabilities are prob[p_offsets[i] : p_offsets[i + 1]].reshape(
        n_win_i, P_i) (cosv likewise, with want_cos), its winners pred[w_offsets[i] : w_offsets[i + 1]]; prob / cosv / pred are device tensors,
        the offsets host int64.  A window without a word or without a frame of any candidate reads pred -1 and NaN; a candidate without
        a frame in a decided window prob 0 and cosv NaN."""
        win, hop = int(win), int(hop)
        if not 0 <= win <= ASDW_MAX_WIN or (win and hop < 1):
            raise ValueError(f"jg_asd_windows limits: win 0 (clip level) or 1..{ASDW_MAX_WIN} frames, hop >= 1")
        if not temp > 0:
            raise ValueError("temp must be positive")
        gs, cs = _row_pair(gesture, content, "gesture / content", max_D=ASDW_MAX_D)
        tk = _ints(trk)
        goh, soh = _offsets(g_offsets, gs[0], "g_offsets"), _offsets(s_offsets, tk.size, "s_offsets")
        n, n_tracks = soh.size - 1, goh.size - 1
        coh = _offsets(c_offsets, cs[0], "c_offsets", n)
        T = np.diff(goh)
        P = _within(np.diff(soh), 1, ASDW_MAX_P, "jg_asd_windows limits: candidates per scene")
        _within(np.diff(coh), 1, SPOT_MAX_W, "jg_asd_windows limits: words per scene")
        used = tk[soh[0]:soh[-1]]
        if used.size and (used.min() < 0 or used.max() >= n_tracks or T[used].min() < 1 or T[used].max() > SPOT_MAX_T):
            raise ValueError(f"jg_asd_windows limits: candidates must be existing tracks of 1..{SPOT_MAX_T} frames")
        if win:
            if word_start is None or word_end is None:
                raise ValueError("windows need word_start / word_end")
            wsh, weh = _ints(word_start), _ints(word_end)
            if wsh.size < coh[-1] or weh.size != wsh.size or (n and max(np.abs(wsh).max(), np.abs(weh).max()) > INT32_MAX):
                raise ValueError("word_start / word_end need one int32 entry per content row")
            if n_windows is None:
                n_windows = [-(-int(T[tk[soh[i]:soh[i + 1]]].max()) // hop) for i in range(n)]
        elif n_windows is None:
            n_windows = np.ones(n, np.int64)
        nw = _ints(n_windows)
        if nw.size != n or (n and (nw.min() < 1 or nw.max() > ASDW_MAX_WIN)):
            raise ValueError(f"jg_asd_windows limits: 1..{ASDW_MAX_WIN} windows per scene, one count per scene")
        w_off, p_off = _ragged(nw, "windows"), _ragged(nw * P)
        self._bind_stream()
        prob = torch.full((int(p_off[-1]),), float("nan"), dtype=torch.float32, device=self.device)
        cosv = torch.full((int(p_off[-1]),), float("nan"), dtype=torch.float32, device=self.device) if want_cos else None
        pred = torch.full((int(w_off[-1]),), -1, dtype=torch.int32, device=self.device)
        if n == 0:
            return prob, p_off, pred, w_off, cosv
        g, c = self._f32(gesture), self._f32(content)
        go, co, so, tr, wo = (self._i32(a) for a in (goh, coh, soh, tk, w_off))
        ws, we = (self._i32(wsh), self._i32(weh)) if win else (None, None)
        po = torch.as_tensor(p_off[:-1].copy(), device=self.device)
        self._ck(self.lib.jg_asd_windows(self.h, _ptr(g), _ptr(go), n_tracks, _ptr(c), _ptr(co), _ptr(ws), _ptr(we), _ptr(tr), _ptr(so), n,
                                         gs[1], win, hop, _ptr(wo), _ptr(po), int(nw.max()), float(temp), _ptr(prob), _ptr(cosv), _ptr(pred)))
        return prob, p_off, pred, w_off, cosv
