"""The host side of jg_sim_ordered and jg_sim_align without a GPU: the restatement in sim_ordered_cases.py against a float64 search over
every monotone assignment, the three consequences of the definition, the argument checks Engine.sim_ordered / Engine.sim_align make before
they need a device, the library's exports and the new kernels' resources, and metrics.search_phrases(order, align) /
Corpus.search_phrases / coupling_matrix(ordered) / coupling_retrieval_metrics(ordered) with their drivers on a stand-in engine that
computes the two entries with the restatement."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import sim_coupling_cases as C
import sim_ordered_cases as O
from jegal_amd import drivers, metrics as M
from jegal_amd._lib import _SIGS, EXPORTS, Engine
from test_sim_coupling_cpu import CouplingEngine
from test_sim_topk_grouped_cpu import grouped_reference, scores, write_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OrderedEngine(CouplingEngine):
    """... and sim_ordered / sim_align with the contracts of Engine's, from the restatement in sim_ordered_cases.py"""

    def sim_ordered(self, words, w_offsets, gallery, g_offsets, k, group_offset=0, merge_into=None, slices=0, want_matrix=False):
        assert isinstance(gallery, torch.Tensor) and gallery.dtype in (torch.float16, torch.float32)
        off, woff = np.asarray(g_offsets, np.int64), np.asarray(w_offsets, np.int64)
        assert off[0] == 0 and off[-1] == gallery.shape[0] and np.all(np.diff(off) >= 0)
        self.names.append("sim_ordered")
        self.calls.append(dict(n=len(woff) - 1, m=gallery.shape[0], groups=len(off) - 1, k=k, offset=group_offset, merge=merge_into is not None,
                               dtype=gallery.dtype))
        self.galleries.append(gallery)
        init = None if merge_into is None else (merge_into[0].numpy(), merge_into[1].numpy())
        idx, sc, pair = O.ordered_expected(scores(words.numpy(), gallery.float().numpy()), woff, off, k, group_offset, init)
        res = (torch.from_numpy(idx), torch.from_numpy(sc))
        return res + (torch.from_numpy(pair).t(),) if want_matrix else res

    def sim_align(self, words, w_offsets, gallery, g_offsets, idx, ordered, group_offset=0, into=None):
        off, woff = np.asarray(g_offsets, np.int64), np.asarray(w_offsets, np.int64)
        assert off[0] == 0 and off[-1] == gallery.shape[0] and isinstance(ordered, bool)
        self.names.append("sim_align")
        self.aligns.append(dict(m=gallery.shape[0], offset=group_offset, ordered=ordered, into=into is not None))
        held = (None, None) if into is None else (into[0].numpy(), into[1].numpy())
        fr, sc = O.align_expected(scores(words.numpy(), gallery.float().numpy()), woff, off, idx.numpy(), ordered, group_offset, *held)
        return torch.from_numpy(fr), torch.from_numpy(sc)

    def __init__(self):
        super().__init__()
        self.aligns = []


# ------------------------------------------------------------------------------------------------ the restatement
def tiny_case(rng):
    W, T = int(rng.integers(1, 5)), int(rng.integers(1, 7))
    s = rng.integers(-3, 4, (W, T + 2)).astype(np.float32)
    s[rng.random(s.shape) < 0.15] = np.nan
    s[rng.random(s.shape) < 0.1] = -0.0
    return s, W, T


def test_restatement_equals_the_search_over_monotone_assignments():
    """integer entries: every sum is exact, so the float64 search and the float32 chain agree to the last bit, arg-max ties included"""
    rng = np.random.default_rng(11000)
    seen_nan = seen_tie = 0
    for trial in range(300):
        s, W, T = tiny_case(rng)
        a, b = 1, 1 + T                                                       # a group inside the row, columns on both sides
        want, want_ts = O.brute_force_ordered(s, a, b)
        got = O.ordered_scores(s, [0, W], [a, b])
        idx = np.zeros((1, 1), np.int32)
        fr, sc = O.align_expected(s, [0, W], [a, b], idx, True)
        if want_ts is None:
            seen_nan += 1
            assert np.isnan(got[0, 0]) and np.isnan(sc[0, 0]) and np.all(fr == -1)
            continue
        assert got[0, 0] == np.float32(np.float32(want * W) / np.float32(W)) and not (got[0, 0] == 0 and np.signbit(got[0, 0]))
        assert fr[0, 0].tolist() == [a + t for t in want_ts] and sc[0, 0].view(np.int32) == got[0, 0].view(np.int32)
        assert np.all(np.diff(fr[0, 0]) >= 0)
        # re-adding s at the frames, in word order, gives the score
        acc = np.float32(0)
        for i, t in enumerate(fr[0, 0]):
            acc = np.float32(acc + (s[i, t] + np.float32(0)))
        assert (acc / np.float32(W)).view(np.int32) == sc[0, 0].view(np.int32)
        seen_tie += int(len(set(want_ts)) < W)                              # consecutive words on one frame
        # unordered: every word's first arg-max, and jg_sim_coupling's score
        fu, su = O.align_expected(s, [0, W], [a, b], idx, False)
        cs = C.coupling_scores(s, [0, W], [a, b])[0, 0]
        assert np.isnan(cs) == np.isnan(su[0, 0]) and (np.isnan(cs) or cs.view(np.int32) == su[0, 0].view(np.int32))
        if not np.isnan(cs):
            assert fu[0, 0].tolist() == [a + int(np.nanargmax(s[i, a:b])) for i in range(W)]
    assert seen_nan > 5 and seen_tie > 20


def test_the_three_consequences():
    rng = np.random.default_rng(11100)
    in_order = out_of_order = 0
    for trial in range(60):
        nw, ng = int(rng.integers(3, 20)), int(rng.integers(4, 40))
        s = (rng.standard_normal((nw, ng)) * 3).astype(np.float32) if trial % 2 else rng.integers(-3, 4, (nw, ng)).astype(np.float32)
        s[rng.random(s.shape) < 0.05] = np.nan
        w_off = C.offsets_of_counts(np.diff(np.unique(np.concatenate([[0, nw], rng.integers(0, nw, 3)]))))
        g_off = np.unique(np.concatenate([[0, ng], rng.integers(0, ng, 5)]))
        o, c = O.ordered_scores(s, w_off, g_off), C.coupling_scores(s, w_off, g_off)
        both = ~np.isnan(o)
        # a pair with an ordered score has a coupling score (the converse fails where NaNs block every monotone path)
        assert not np.any(both & np.isnan(c))
        assert np.all(o[both] <= c[both])                                     # 2. never more than the bag of words
        same = O.first_argmax_in_order(s, w_off, g_off)
        assert np.array_equal(o[same].view(np.int32), c[same].view(np.int32))  # 3. equal where the best frames are in order already
        in_order += int(same.sum())
        out_of_order += int((both & ~same & (o < c)).sum())
        # 1. W = 1: the grouped top-k score
        one = O.ordered_expected(s, np.arange(nw + 1), g_off, 3)
        ok_rows = ~np.isnan(s).all(axis=1)
        ref = grouped_reference(np.where(np.isnan(s), -np.inf, s + np.float32(0)), g_off, 3)
        grp_of = np.searchsorted(g_off, np.maximum(ref[0], 0), side="right") - 1
        full = ~np.isnan(s).any(axis=1)                                       # (the reference knows no NaN: rows without one)
        assert np.array_equal(one[0][full], np.where(ref[0] >= 0, grp_of, -1)[full])
        assert np.array_equal(one[1][full].view(np.int32), ref[1][full].view(np.int32)) and ok_rows.any()
    assert in_order > 50 and out_of_order > 50
    # two clips with the same frames in opposite order tie as bags of words; the clip in word order wins under ordered
    s = np.asarray([[5, 1, 1, 5], [1, 4, 4, 1]], np.float32)                   # word 0 likes frames 0 and 3, word 1 frames 1 and 2
    assert C.coupling_expected(s, [0, 2], [0, 2, 4], 2)[0].tolist() == [[0, 1]] and np.all(C.coupling_scores(s, [0, 2], [0, 2, 4]) == 4.5)
    idx, sc, _ = O.ordered_expected(s, [0, 2], [0, 2, 4], 2)
    assert idx.tolist() == [[0, 1]] and sc.tolist() == [[4.5, 3.0]]
    idx, sc, _ = O.ordered_expected(s[:, [2, 3, 0, 1]], [0, 2], [0, 2, 4], 2)          # the two clips swapped
    assert idx.tolist() == [[1, 0]] and sc.tolist() == [[4.5, 3.0]]
    # more words than frames: consecutive words share a frame
    s = np.asarray([[1, 0], [0, 2], [3, 0], [0, 1]], np.float32)
    fr, sc = O.align_expected(s, [0, 4], [0, 2], np.zeros((1, 1), np.int32), True)
    assert fr[0, 0].tolist() == [0, 0, 0, 1] and sc[0, 0] == np.float32(5) / np.float32(4)
    # merging two halves gives the whole, with the selection rule of the coupling entry
    s = rng.integers(-2, 3, (6, 30)).astype(np.float32)
    g_off = np.arange(0, 31, 3)
    whole = O.ordered_expected(s, [0, 2, 6], g_off, 4)
    part = O.ordered_expected(s[:, 15:], [0, 2, 6], g_off[5:] - 15, 4, group_offset=5)
    both = O.ordered_expected(s[:, :15], [0, 2, 6], g_off[:6], 4, init=part[:2])
    assert np.array_equal(both[0], whole[0]) and np.array_equal(both[1], whole[1])


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_entries_and_the_kernels_do_not_spill():
    import __graft_entry__ as G
    G.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jegal_amd", "libjegal_hip.so"))
    assert hasattr(lib, "jg_sim_ordered") and hasattr(lib, "jg_sim_align")
    header = open(os.path.join(ROOT, "include", "jegal_hip.h")).read()
    assert "jg_sim_ordered(" in header and "jg_sim_align(" in header
    assert len(_SIGS["jg_sim_ordered"]) == 18 and _SIGS["jg_sim_ordered"] == _SIGS["jg_sim_coupling"] and "jg_sim_ordered" in EXPORTS
    assert len(_SIGS["jg_sim_align"]) == 17 and "jg_sim_align" in EXPORTS
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    ordered = {k: v for k, v in res.items() if "sim_ordered_kernel" in k}
    align = {k: v for k, v in res.items() if "sim_align_kernel" in k}
    assert len(ordered) == 4 and len(align) == 2                             # fp32 / fp16 gallery (x lists of 64 / 128)
    for name, r in {**ordered, **align}.items():
        assert r["spill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 128, (name, r)
    coupling = {k: v for k, v in res.items() if "sim_coupling_kernel" in k}
    topk = sorted(v["lds"] for k, v in res.items() if "sim_topk_kernel" in k)
    assert len(coupling) == 4 and len(topk) == 8                             # what test_sim_coupling_cpu.py pins is what it was
    assert sorted({v["lds"] for v in coupling.values()}) == [topk[0] + 1040, topk[-1] + 1040]
    # the score tile's own 16 KB in place of the two partial maxima: + 16384 - 512 on the coupling kernel
    assert sorted({v["lds"] for v in ordered.values()}) == [topk[0] + 1040 + 15872, topk[-1] + 1040 + 15872]
    assert {v["lds"] for v in align.values()} == {3 * 16384 + 64 * 129 * 8 + 256}
    src = open(os.path.join(ROOT, "jegal_amd", "csrc", "retrieval.hip")).read()
    assert 'record_kernel("sim_ordered_kernel<' in src and 'record_kernel("sim_align_kernel<' in src


def test_engine_refuses_bad_arguments_before_it_needs_a_device():
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    w, g = torch.zeros(20, 128), torch.zeros(30, 128)
    woff, goff = [0, 3, 20], [0, 10, 10, 30]
    ok_i, ok_s = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5)
    good = dict(words=w, w_offsets=woff, gallery=g, g_offsets=goff, k=5)
    bad = [dict(words=torch.zeros(128)), dict(gallery=torch.zeros(30, 64)), dict(gallery=g.double()), dict(gallery=[[0.0] * 128] * 30),
           dict(k=0), dict(k=129), dict(slices=-1), dict(slices=1025), dict(group_offset=-1), dict(group_offset=2 ** 31 - 3),
           dict(w_offsets=[0, 3, 3, 20]), dict(w_offsets=[0, 65], words=torch.zeros(65, 128)), dict(w_offsets=[1, 20]), dict(w_offsets=[0, 21]),
           dict(g_offsets=[0, 20, 10, 30]), dict(g_offsets=[0, 31]), dict(merge_into=ok_i), dict(merge_into=(ok_i, ok_s[:, :4])),
           dict(words=torch.zeros(70000, 64), w_offsets=np.arange(70001), gallery=torch.zeros(128, 64), g_offsets=[0, 128], k=128, slices=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.sim_ordered(**{**good, **kw})
    for kw in (dict(), dict(gallery=g.half(), k=128, slices=1024), dict(w_offsets=[0, 3, 19], want_matrix=True)):
        with pytest.raises(AttributeError):           # past every check, it fails at the first use of the handle
            eng.sim_ordered(**{**good, **kw})
    eng.device = torch.device("cpu")                  # (sim_align compares devices before it binds the stream)
    good = dict(words=w, w_offsets=woff, gallery=g, g_offsets=goff, idx=ok_i, ordered=True)
    fr, sc = torch.zeros(2, 5, 17, dtype=torch.int32), torch.zeros(2, 5)
    bad = [dict(words=torch.zeros(128)), dict(gallery=torch.zeros(30, 64)), dict(gallery=g.double()), dict(group_offset=-1),
           dict(group_offset=2 ** 31 - 3), dict(w_offsets=[0, 3, 3, 20]), dict(w_offsets=[1, 20]), dict(g_offsets=[0, 31]),
           dict(idx=ok_i.long()), dict(idx=ok_s), dict(idx=torch.zeros(3, 5, dtype=torch.int32)), dict(idx=torch.zeros(2, 129, dtype=torch.int32)),
           dict(idx=torch.zeros(2, 0, dtype=torch.int32)), dict(idx=torch.zeros(5, 2, dtype=torch.int32).t()), dict(idx=ok_i.numpy()),
           dict(into=fr), dict(into=(fr[:, :, :16].contiguous(), sc)), dict(into=(fr, sc[:, :4])), dict(into=(fr.float(), sc)), dict(into=(sc, fr))]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.sim_align(**{**good, **kw})
    for kw in (dict(), dict(ordered=False, gallery=g.half(), into=(fr, sc)), dict(group_offset=2 ** 31 - 4)):
        with pytest.raises(AttributeError):
            eng.sim_align(**{**good, **kw})


# ------------------------------------------------------------------------------------------------ metrics on the stand-in engine
@pytest.fixture(scope="module")
def corpus():
    """9 clips of 1..40 frames, D = 64.  Phrase 0 = frames 22, 17 and 3 of clip 5 IN THAT ORDER: as a bag of words clip 5 is perfect, in
    word order it is not; clip 7 holds the same three frames in word order at 2, 9 and 15 with some noise.  Phrase 1 = frame 0 of clip 2;
    phrase 2 = 9 random words."""
    rng = np.random.default_rng(11200)
    lens = [12, 1, 30, 7, 40, 25, 3, 18, 9]
    clips = [(rng.standard_normal((t, 64)) * rng.uniform(0.5, 3.0, (t, 1))).astype(np.float32) for t in lens]
    words = [clips[5][22], clips[5][17], clips[5][3]]
    for t, wd in zip((2, 9, 15), words):
        clips[7][t] = wd + 0.2 * rng.standard_normal(64).astype(np.float32)
    phrases = [np.stack(words), clips[2][:1] * 0.5, rng.standard_normal((9, 64)).astype(np.float32)]
    return phrases, clips


def brute_ordered(phrases, clips, k, segment=0):
    """search_phrases(order=True, align=True) by its definition, group by group, through the restatement"""
    n = lambda x: OrderedEngine().l2norm(np.asarray(x, np.float32)).numpy()
    out = []
    wmax = max(len(p) for p in phrases)
    for p in phrases:
        cand = []
        for c, rows in enumerate(clips):
            s = scores(n(p), n(rows))
            step = segment if segment > 0 else max(s.shape[1], 1)
            for a in range(0, s.shape[1], step):
                b = min(a + step, s.shape[1])
                sc = O.ordered_scores(s, [0, len(p)], [a, b])[0, 0]
                fr = O.align_expected(s, [0, len(p)], [a, b], np.zeros((1, 1), np.int32), True)[0][0, 0]
                cand.append((-float(sc), c, a, fr.tolist() + [-1] * (wmax - len(p))))
        cand.sort(key=lambda x: x[:3])
        out.append(cand[:k] + [(np.inf, -1, -1, [-1] * wmax)] * (k - len(cand[:k])))
    col = lambda i, t: np.asarray([[x[i] for x in row] for row in out], t)
    return col(1, np.int32), col(2, np.int32), -col(0, np.float32), col(3, np.int32)


@pytest.mark.parametrize("segment,max_rows", [(0, None), (8, None), (0, 40), (8, 8), (8, 20)])
def test_search_phrases_in_order_with_frames(corpus, segment, max_rows):
    phrases, clips = corpus
    eng = OrderedEngine()
    got = M.search_phrases(phrases, clips, k=6, segment=segment, engine=eng, max_rows=max_rows, order=True, align=True)
    want = brute_ordered(phrases, clips, 6, segment)
    assert [a.dtype for a in got] == [np.int32, np.int32, np.float32, np.int32] and got[3].shape == (3, 6, 9)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    scored = [n for n in eng.names if n != "sim_align"]
    assert scored == ["sim_ordered"] * len(eng.calls) and eng.names[len(scored):] == ["sim_align"] * len(eng.aligns)     # every piece, then every piece again
    assert len(eng.aligns) == len(eng.calls) and [a["into"] for a in eng.aligns] == [False] + [True] * (len(eng.aligns) - 1)
    assert all(a["ordered"] is True for a in eng.aligns) and [a["offset"] for a in eng.aligns] == [c["offset"] for c in eng.calls]
    assert (len(eng.calls) == 1) == (max_rows is None)
    if segment == 0:
        assert got[0][0, 0] == 7 and got[3][0, 0, :3].tolist() == [2, 9, 15] and np.all(got[3][0, :, 3:] == -1)     # the clip in word order, and where
        assert got[0][1, 0] == 2 and got[3][1, 0].tolist() == [0] + [-1] * 8
    # the frames count from the clip's first frame, also inside a segment: they lie in the returned group
    size = segment if segment else 10 ** 9
    live = got[3] >= 0
    lo, hi = got[1][:, :, None], got[1][:, :, None] + size
    assert np.all((got[3] >= lo)[live]) and np.all((got[3] < hi)[live]) and np.all(np.diff(np.where(live, got[3], 10 ** 6), axis=2) >= 0)
    # the unordered call: clip 5 wins as a bag of words, its frames come back out of order, and sim_ordered is never called
    eng2 = OrderedEngine()
    un = M.search_phrases(phrases, clips, k=6, segment=segment, engine=eng2, max_rows=max_rows, align=True)
    plain = M.search_phrases(phrases, clips, k=6, segment=segment, engine=CouplingEngine(), max_rows=max_rows)
    assert all(np.array_equal(a, b) for a, b in zip(un[:3], plain)) and "sim_ordered" not in eng2.names
    assert all(a["ordered"] is False for a in eng2.aligns)
    if segment == 0:
        assert un[0][0, 0] == 5 and un[3][0, 0, :3].tolist() == [22, 17, 3]
    assert np.all(got[2] <= un[2][:, :1] + 0) and np.all(got[2][:, 0] <= un[2][:, 0])
    # order without align: three arrays, no second pass
    eng3 = OrderedEngine()
    three = M.search_phrases(phrases, clips, k=6, segment=segment, engine=eng3, max_rows=max_rows, order=True)
    assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, got[:3])) and "sim_align" not in eng3.names


def test_search_phrases_edge_cases(corpus):
    phrases, clips = corpus
    eng = OrderedEngine()
    for kw in (dict(k=0), dict(max_rows=39)):
        with pytest.raises(ValueError):
            M.search_phrases(phrases, clips, engine=eng, order=True, align=True, **kw)
    assert not eng.calls and not eng.aligns
    none = M.search_phrases([], clips, k=3, engine=eng, order=True, align=True)
    assert len(none) == 4 and none[3].shape == (0, 3, 0) and len(M.search_phrases([], clips, k=3, engine=eng, order=True)) == 3
    for nothing in (M.search_phrases(phrases, [], k=3, engine=eng, align=True),
                    M.search_phrases(phrases, [np.zeros((0, 64), np.float32)], k=3, engine=eng, order=True, align=True)):
        assert len(nothing) == 4 and nothing[3].shape == (3, 3, 9) and np.all(nothing[3] == -1) and np.all(nothing[0] == -1)
    clip, start, score, wf = M.search_phrases(phrases, [clips[0], np.zeros((0, 64), np.float32), clips[2]], k=3, engine=eng, order=True, align=True)
    assert np.all(clip[:, 2] == -1) and np.all(wf[:, 2] == -1) and np.all(wf[:, :2, 0] >= 0)       # an empty clip has no score and no frames
    assert np.all(wf[2, :2] >= 0) and np.all(wf[0, :2, 3:] == -1)


def test_corpus_search_phrases_over_the_stored_rows(corpus):
    phrases, clips = corpus
    eng = OrderedEngine()
    c32 = M.Corpus.build(clips, dtype="float32", engine=eng)
    c16 = M.Corpus.build(clips, engine=eng)
    pn = [eng.l2norm(p).numpy() for p in phrases]
    widened = np.split(c16.rows.astype(np.float32), np.cumsum(c16.lengths)[:-1])
    for segment, max_rows in ((0, None), (8, 20)):
        for order in (True, False):
            want = M.search_phrases(phrases, clips, k=5, segment=segment, engine=OrderedEngine(), max_rows=max_rows, order=order, align=True)
            eng.calls.clear(), eng.names.clear()
            got = c32.search_phrases(phrases, k=5, segment=segment, engine=eng, max_rows=max_rows, order=order, align=True)
            assert len(got) == 4 and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
            assert ("sim_ordered" in eng.names) == order and ("sim_coupling" in eng.names) != order and "sim_align" in eng.names
            got16 = c16.search_phrases(phrases, k=5, segment=segment, engine=eng, max_rows=max_rows, order=order, align=True)
            want16 = M.search_phrases(pn, widened, k=5, segment=segment, normalize=False, engine=OrderedEngine(), max_rows=max_rows, order=order,
                                      align=True)
            assert all(np.array_equal(a, b) for a, b in zip(got16, want16)) and got16[0][0, 0] == (7 if order else 5)
    assert c16.search_phrases([], k=4, engine=eng, align=True)[3].shape == (0, 4, 0)
    assert len(c16.search_phrases(phrases, k=4, engine=eng)) == 3            # the call of before is what it was


def test_coupling_matrix_and_retrieval_metrics_in_order(corpus):
    phrases, clips = corpus
    rng = np.random.default_rng(11300)
    contents = [np.stack([c[i] for i in rng.integers(0, len(c), int(rng.integers(1, 10)))]) + 0.3 * rng.standard_normal((1, 64)).astype(np.float32)
                for c in clips]
    eng = OrderedEngine()
    m = M.coupling_matrix(contents, clips, engine=eng, ordered=True)
    assert eng.names == ["sim_ordered"] and tuple(m.shape) == (9, 9) and m.dtype == torch.float32
    n = lambda x: eng.l2norm(x).numpy()
    s = scores(np.concatenate([n(c) for c in contents]), np.concatenate([n(c) for c in clips]))
    want = O.ordered_scores(s, M.offsets_of(contents), M.offsets_of(clips))
    assert np.array_equal(m.numpy(), want)
    un = M.coupling_matrix(contents, clips, engine=eng).numpy()
    assert eng.names == ["sim_ordered", "sim_coupling"] and np.all(want <= un) and np.any(want < un)
    res = M.coupling_retrieval_metrics(contents, clips, engine=eng, ordered=True)
    assert eng.names[-1] == "sim_ordered"
    d = np.diag(want)
    for key, part in (("c2g", want), ("g2c", want.T)):
        assert res[key] == M.metrics_from_ranks((part > d[:, None]).sum(1), (part == d[:, None]).sum(1)), key
    assert tuple(M.coupling_matrix([], clips, engine=eng, ordered=True).shape) == (0, 9)


# ------------------------------------------------------------------------------------------------ the drivers
def test_search_level_ordered_with_align(corpus, tmp_path, capsys):
    phrases, clips = corpus
    src = tmp_path / "pkl"
    src.mkdir()
    names = write_corpus(src, clips)
    query = tmp_path / "hello_there.pkl"
    with open(query, "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": phrases[0],
                     "info": {"fname": "hello_there", "word_boundaries": [["hello", 0, 4], ["there", 5, 9], ["now", 10, 12]]}}, f)
    eng = OrderedEngine()
    assert drivers.cmd_index(["--path", str(src), "--out", str(tmp_path / "c32.npz"), "--dtype", "float32"], engine=eng) == 0
    capsys.readouterr()
    for extra, segment, max_rows in (([], 0, None), (["--segment", "8", "--max_rows", "24"], 8, 24)):
        want = brute_ordered(phrases[:1], clips, 4, segment)
        outs = []
        for n, corpus_args in enumerate((["--path", str(src)], ["--index", str(tmp_path / "c32.npz")])):
            res = tmp_path / f"res{len(extra)}_{n}"
            eng.calls.clear(), eng.names.clear()
            assert drivers.cmd_search(corpus_args + ["--query", str(query), "--level", "ordered", "--align", "--topk", "4", "--res_dir", str(res)]
                                      + extra, engine=eng) == 0
            assert set(eng.names) == {"sim_ordered", "sim_align"} and all(c["n"] == 1 for c in eng.calls)
            lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("search: \"")]
            assert len(lines) == 1
            if not segment:
                assert lines[0].startswith("search: \"hello there now\" -> 4 of 9 clips: vid007__t@0 (") and "[hello@2 there@9 now@15]" in lines[0]
            z = np.load(res / "search_hello_there.npz")
            assert sorted(z.files) == ["clip", "frame", "names", "score", "start", "word_frame", "words"]
            assert list(z["names"]) == names and z["word_frame"].dtype == np.int32 and z["word_frame"].shape == (1, 4, 3)
            for key, w in zip(("clip", "start", "score", "word_frame"), want):
                assert np.array_equal(z[key], w), key
            outs.append(z)
        assert all(np.array_equal(outs[0][key], outs[1][key]) for key in outs[0].files)
    # --level coupling --align: the bag of words with every word's own best frame; without --align the file of before
    res = tmp_path / "un"
    eng.names.clear()
    assert drivers.cmd_search(["--path", str(src), "--query", str(query), "--level", "coupling", "--align", "--topk", "4", "--res_dir", str(res)],
                              engine=eng) == 0
    z = np.load(res / "search_hello_there.npz")
    assert set(eng.names) == {"sim_coupling", "sim_align"} and z["clip"][0, 0] == 5 and z["word_frame"][0, 0].tolist() == [22, 17, 3]
    assert "[hello@22 there@17 now@3]" in capsys.readouterr().out
    assert drivers.cmd_search(["--path", str(src), "--query", str(query), "--level", "ordered", "--topk", "4", "--res_dir", str(res)], engine=eng) == 0
    assert sorted(np.load(res / "search_hello_there.npz").files) == ["clip", "frame", "names", "score", "start", "words"]
    eng.names.clear()
    with pytest.raises(SystemExit, match="--align"):
        drivers.cmd_search(["--path", str(src), "--query", str(query), "--level", "word", "--align"], engine=eng)
    long_query = tmp_path / "long.pkl"
    with open(long_query, "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": np.ones((65, 64), np.float32), "info": {"fname": "long"}}, f)
    with pytest.raises(SystemExit, match="64"):
        drivers.cmd_search(["--path", str(src), "--query", str(long_query), "--level", "ordered"], engine=eng)
    assert not eng.names


def test_evaluate_retrieval_score_ordered(corpus, tmp_path, capsys):
    phrases, clips = corpus
    rng = np.random.default_rng(11400)
    contents = [np.stack([c[i] for i in np.sort(rng.integers(0, len(c), int(rng.integers(1, 10))))]) for c in clips]
    src = tmp_path / "pkl"
    src.mkdir()
    for i, (g, c) in enumerate(zip(clips, contents)):
        with open(src / f"vid{i:03d}__t.pkl", "wb") as f:
            pickle.dump({"gesture_emb": g, "content_emb": c, "info": {"fname": f"vid{i:03d}__t"}}, f)
    line = "R@1: {:.2f} - R@5: {:.2f} - R@10: {:.2f} - R@25: {:.2f} - R@50: {:.2f} | Median R: {:.1f}"
    fmt = lambda m: line.format(m["R1"] * 100, m["R5"] * 100, m["R10"] * 100, m["R25"] * 100, m["R50"] * 100, m["MR"])
    eng = OrderedEngine()
    res = drivers.cmd_evaluate_retrieval(["--path", str(src), "--score", "ordered"], engine=eng)
    assert eng.names == ["sim_ordered"]
    want = M.coupling_retrieval_metrics(contents, clips, engine=eng, ordered=True)
    assert res == {"Content to Gesture": want["c2g"], "Gesture to Content": want["g2c"]}
    assert capsys.readouterr().out.splitlines() == ["No of files =  9", "Content to Gesture Retrieval scores:", fmt(want["c2g"]),
                                                    "Gesture to Content Retrieval scores:", fmt(want["g2c"])]
    assert res["Content to Gesture"]["R1"] == 1.0                            # the words are frames of their own clip, in order
    eng.names.clear()
    drivers.cmd_evaluate_retrieval(["--path", str(src), "--score", "coupling"], engine=eng)
    assert eng.names == ["sim_coupling"]
