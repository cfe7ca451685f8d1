"""The host side of jg_sim_coupling without a GPU: the plan (jg_debug_coupling_plan: a pure host function of the library) against the
packing rule restated in sim_coupling_cases.py, that restatement against a float64 brute force, the argument checks Engine.sim_coupling
makes before it needs a device, the library's exports and the new kernels' resources, and metrics.search_phrases / Corpus.search_phrases /
coupling_matrix / coupling_retrieval_metrics with their drivers on a stand-in engine that computes sim_coupling with numpy."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import sim_coupling_cases as C
from jegal_amd import drivers, metrics as M
from jegal_amd._lib import _SIGS, EXPORTS, Engine, JegalError, coupling_plan, search_plan
from jegal_amd._metric_entries import COUPLING_MAX_W, SIM_SEARCH_MAX_SLICES, SIM_SEARCH_MAX_WS
from test_sim_search_cpu import SearchEngine
from test_sim_topk_grouped_cpu import scores, write_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class CouplingEngine(SearchEngine):
    """... and sim_coupling with Engine.sim_coupling's contract, from the restatement in sim_coupling_cases.py; pool_mean and sim_rank
    for the pooled evaluation, each call recorded by name"""

    def __init__(self):
        super().__init__()
        self.names = []

    def sim_coupling(self, words, w_offsets, gallery, g_offsets, k, group_offset=0, merge_into=None, slices=0, want_matrix=False):
        assert isinstance(gallery, torch.Tensor) and gallery.dtype in (torch.float16, torch.float32)
        off, woff = np.asarray(g_offsets, np.int64), np.asarray(w_offsets, np.int64)
        assert off[0] == 0 and off[-1] == gallery.shape[0] and np.all(np.diff(off) >= 0)          # a piece is cut at group boundaries
        assert woff[0] == 0 and woff[-1] == words.shape[0] and np.all(np.diff(woff) >= 1) and np.all(np.diff(woff) <= 64)
        self.names.append("sim_coupling")
        self.calls.append(dict(n=len(woff) - 1, m=gallery.shape[0], groups=len(off) - 1, k=k, offset=group_offset, merge=merge_into is not None,
                               dtype=gallery.dtype))
        self.galleries.append(gallery)
        init = None if merge_into is None else (merge_into[0].numpy(), merge_into[1].numpy())
        idx, sc, pair = C.coupling_expected(scores(words.numpy(), gallery.float().numpy()), woff, off, k, group_offset, init)
        res = (torch.from_numpy(idx), torch.from_numpy(sc))
        return res + (torch.from_numpy(pair).t(),) if want_matrix else res

    def pool_mean(self, x, offsets):
        self.names.append("pool_mean")
        x = torch.as_tensor(x, dtype=torch.float32)
        return torch.stack([x[a:b].mean(0) for a, b in zip(offsets[:-1], offsets[1:])])

    def sim_rank(self, e1, e2, row_offset=0):
        self.names.append("sim_rank")
        s = e1 @ e2.t()
        d = s.diagonal()[:, None]
        return (s > d).sum(1).to(torch.int32), (s == d).sum(1).to(torch.int32)


# ------------------------------------------------------------------------------------------------ the plan
def check_plan(w_counts, n_gallery=1000, k=10, num_cu=256, slices=0):
    w_off = C.offsets_of_counts(w_counts)
    tfq, S, R, ws = coupling_plan(w_off, n_gallery, k, num_cu, slices)
    want = C.plan_expected(w_off)
    assert tfq.tolist() == want, w_counts
    n_tiles, nq = len(want) - 1, len(w_counts)
    for a, b in zip(want[:-1], want[1:]):                                   # whole queries, at most 64 word rows, and no room wasted
        assert a < b and w_off[b] - w_off[a] <= 64
        assert b == nq or w_off[b + 1] - w_off[a] > 64
    # the cut is jg_debug_search_plan's with the query tiles in place of the query blocks: n_tiles * 64 query rows have as many blocks
    S2, R2, _ = search_plan(n_tiles * 64, n_gallery, 1, num_cu, slices)
    assert (S, R) == (S2, R2) and ws == (S * nq * k * 8 if S > 1 else 0)
    return tfq, S, R, ws


def test_plan_packs_whole_queries_in_order():
    assert len(_SIGS["jg_debug_coupling_plan"]) == 11 and "jg_debug_coupling_plan" in EXPORTS
    assert check_plan([1] * 130)[0].tolist() == [0, 64, 128, 130]
    assert check_plan([64] * 5)[0].tolist() == [0, 1, 2, 3, 4, 5]
    assert check_plan([60, 4, 1])[0].tolist() == [0, 2, 3]                   # fills a tile exactly, then starts a new one
    assert check_plan([60, 5])[0].tolist() == [0, 1, 2]                      # does not fit: it moves
    assert check_plan([])[0].tolist() == [0]
    rng = np.random.default_rng(9100)
    for trial in range(20):
        counts = rng.integers(1, 18, int(rng.integers(1, 400))).tolist()
        for n_gallery, slices in ((0, 0), (63, 0), (1500000, 0), (1500000, 7), (4096, 1024)):
            check_plan(counts, n_gallery, int(rng.integers(1, 129)), 256, slices)
    tfq, S, R, ws = check_plan([8] * 500, 75000, 10, 256)                    # the real lists: 63 tiles of 8 queries, every CU gets work
    assert len(tfq) == 64 and S > 1 and ws == S * 500 * 10 * 8


def test_plan_refuses_what_the_entry_refuses():
    good = dict(w_offsets=[0, 3, 10], n_gallery=1000, k=10, num_cu=256, slices=0)
    coupling_plan(**good)
    bad = [dict(w_offsets=[0, 3, 3]), dict(w_offsets=[0, 65]), dict(w_offsets=[0, 5, 4]), dict(w_offsets=[1, 5]), dict(k=0), dict(k=129),
           dict(slices=SIM_SEARCH_MAX_SLICES + 1), dict(slices=-1), dict(n_gallery=-1), dict(num_cu=0),
           dict(w_offsets=np.arange(70001), n_gallery=128, k=128, slices=2)]       # 2 x 70000 x 128 keys: beyond the 64 MiB of lists
    for kw in bad:
        with pytest.raises(JegalError):
            coupling_plan(**{**good, **kw})
    assert COUPLING_MAX_W == 64 and 2 * 70000 * 128 * 8 > SIM_SEARCH_MAX_WS
    coupling_plan(**{**good, "w_offsets": [0, 64, 128]})
    coupling_plan(np.arange(70001), 128, 128, slices=1)                      # one slice writes no lists


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_equals_the_float64_definition_on_exact_operands():
    rng = np.random.default_rng(9200)
    for D in (8, 64):
        words = rng.integers(-2, 3, (40, D)).astype(np.float32)
        gallery = rng.integers(-2, 3, (90, D)).astype(np.float32)
        gallery[[7, 30, 31, 32]] = np.nan                                    # rows 30 .. 32 are all of one group
        w_off = C.offsets_of_counts([1, 2, 7, 17, 3, 10])
        g_off = np.asarray([2, 2, 10, 30, 33, 33, 60, 61, 88])
        with np.errstate(invalid="ignore"):
            s = (words.astype(np.float64) @ gallery.astype(np.float64).T).astype(np.float32)
        want = C.brute_force_scores(words, gallery, w_off, g_off)
        got = C.coupling_scores(s, w_off, g_off)
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(got[:, [0, 3, 4]]).all() and not np.isnan(got[:, [1, 2, 5, 6, 7]]).any()      # empty and all-NaN groups have no score
        assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)].astype(np.float32))
        for k in (1, 3, 8):
            idx, sc, pair = C.coupling_expected(s, w_off, g_off, k, group_offset=100)
            assert np.array_equal(pair.T[~np.isnan(got)], got[~np.isnan(got)])
            for q in range(len(w_off) - 1):
                cand = sorted((-float(v), 100 + g) for g, v in enumerate(want[q]) if not np.isnan(v))[:k]
                assert idx[q, :len(cand)].tolist() == [g for _, g in cand] and sc[q, :len(cand)].tolist() == [np.float32(-v) for v, _ in cand]
                assert np.all(idx[q, len(cand):] == -1) and np.all(np.isneginf(sc[q, len(cand):]))
    # -0.0 counts as +0.0 and a tie goes to the smaller group; merging two halves gives the whole
    s = np.asarray([[-0.0, 0.0, -1.0], [0.0, -0.0, -1.0]], np.float32)
    idx, sc, _ = C.coupling_expected(s, [0, 2], [0, 1, 2, 3], 3)
    assert idx.tolist() == [[0, 1, 2]] and not np.signbit(sc[0, :2]).any()
    part = C.coupling_expected(s[:, 2:], [0, 2], [0, 1], 3, group_offset=2)
    both = C.coupling_expected(s[:, :2], [0, 2], [0, 1, 2], 3, init=part[:2])
    assert np.array_equal(both[0], idx) and np.array_equal(both[1], sc)


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_entries_and_the_kernels_do_not_spill():
    import __graft_entry__ as G
    G.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jegal_amd", "libjegal_hip.so"))
    assert hasattr(lib, "jg_sim_coupling") and hasattr(lib, "jg_debug_coupling_plan")
    header = open(os.path.join(ROOT, "include", "jegal_hip.h")).read()
    assert "jg_sim_coupling(" in header and "jg_debug_coupling_plan(" in header
    assert len(_SIGS["jg_sim_coupling"]) == 18 and "jg_sim_coupling" in EXPORTS
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    mine = {k: v for k, v in res.items() if "sim_coupling_kernel" in k}
    assert len(mine) == 4                                                    # fp32 / fp16 gallery x lists of 64 / 128
    topk = sorted(v["lds"] for k, v in res.items() if "sim_topk_kernel" in k)
    for name, r in mine.items():
        assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)                                   # two workgroups of 256 threads per CU, as LDS allows at k <= 64
    # sim_topk_kernel's LDS plus the two partial maxima, the running maxima and the tile's word offsets: about 1 KB
    assert sorted({v["lds"] for v in mine.values()}) == [topk[0] + 1040, topk[-1] + 1040]
    fill = [v for k, v in res.items() if "coupling_fill_kernel" in k]
    assert len(fill) == 1 and fill[0]["spill"] == 0 and fill[0]["scratch"] == 0
    src = open(os.path.join(ROOT, "jegal_amd", "csrc", "retrieval.hip")).read()
    assert 'record_kernel("sim_coupling_kernel<' in src


def test_engine_refuses_bad_arguments_before_it_needs_a_device():
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    w, g = torch.zeros(20, 128), torch.zeros(30, 128)
    woff, goff = [0, 3, 20], [0, 10, 10, 30]
    ok_i, ok_s = torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5)
    good = dict(words=w, w_offsets=woff, gallery=g, g_offsets=goff, k=5)
    bad = [dict(words=torch.zeros(128)), dict(gallery=torch.zeros(30, 64)), dict(words=torch.zeros(20, 96), gallery=torch.zeros(30, 96)),
           dict(gallery=g.double()), dict(gallery=[[0.0] * 128] * 30), dict(k=0), dict(k=129), dict(slices=-1),
           dict(slices=SIM_SEARCH_MAX_SLICES + 1), dict(group_offset=-1), dict(group_offset=2 ** 31 - 3),
           dict(w_offsets=[0, 3, 3, 20]), dict(w_offsets=[0, 65], words=torch.zeros(65, 128)), dict(w_offsets=[0, 5, 4, 20]),
           dict(w_offsets=[1, 20]), dict(w_offsets=[0, 21]), dict(w_offsets=[[0, 20]]), dict(w_offsets=[0.0, 20.0]),
           dict(g_offsets=[0, 20, 10, 30]), dict(g_offsets=[0, 31]), dict(g_offsets=[]),
           dict(merge_into=ok_i), dict(merge_into=(ok_i, ok_s[:, :4])), dict(merge_into=(ok_s, ok_i)),
           dict(merge_into=(torch.zeros(20, 5, dtype=torch.int32), torch.zeros(20, 5))),      # one row per QUERY, not per word
           dict(words=torch.zeros(70000, 64), w_offsets=np.arange(70001), gallery=torch.zeros(128, 64), g_offsets=[0, 128], k=128, slices=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.sim_coupling(**{**good, **kw})
    for kw in (dict(), dict(gallery=g.half(), k=128, slices=SIM_SEARCH_MAX_SLICES), dict(gallery=np.zeros((30, 128), np.float16), group_offset=2 ** 31 - 4),
               dict(w_offsets=[0, 3, 19], want_matrix=True),
               dict(words=torch.zeros(70000, 64), w_offsets=np.arange(70001), gallery=torch.zeros(128, 64), g_offsets=[0, 128], k=128, slices=1)):
        with pytest.raises(AttributeError):           # in order: past every check, it fails at the first use of the handle
            eng.sim_coupling(**{**good, **kw})


# ------------------------------------------------------------------------------------------------ metrics on the stand-in engine
@pytest.fixture(scope="module")
def corpus():
    """9 clips of 1..40 frames, D = 64; phrase 0 = frames 3, 17 and 22 of clip 5, phrase 1 = frame 0 of clip 2, phrase 2 = 9 random words"""
    rng = np.random.default_rng(9300)
    lens = [12, 1, 30, 7, 40, 25, 3, 18, 9]
    clips = [(rng.standard_normal((t, 64)) * rng.uniform(0.5, 3.0, (t, 1))).astype(np.float32) for t in lens]
    phrases = [np.stack([clips[5][3], clips[5][17] * 2.0, clips[5][22]]), clips[2][:1] * 0.5, rng.standard_normal((9, 64)).astype(np.float32)]
    return phrases, clips


def brute_phrases(phrases, clips, k, segment=0, normalize=True):
    """search_phrases by its definition: every group's mean of the words' best frames, the k best groups"""
    n = lambda x: CouplingEngine().l2norm(np.asarray(x, np.float32)).numpy() if normalize else np.asarray(x, np.float32)      # (the stand-in's bits)
    out = []
    for p in phrases:
        cand = []
        for c, rows in enumerate(clips):
            s = scores(n(p), n(rows))
            step = segment if segment > 0 else max(s.shape[1], 1)
            for a in range(0, s.shape[1], step):
                m = s[:, a:a + step].max(axis=1)
                acc = np.float32(0)
                for v in m:
                    acc = np.float32(acc + v)
                cand.append((-float(acc / np.float32(len(m))), c, a))
        cand.sort()
        out.append(cand[:k] + [(np.inf, -1, -1)] * (k - len(cand[:k])))
    return (np.asarray([[c for _, c, _ in row] for row in out], np.int32), np.asarray([[a for _, _, a in row] for row in out], np.int32),
            np.asarray([[-v for v, _, _ in row] for row in out], np.float32))


@pytest.mark.parametrize("segment,max_rows", [(0, None), (8, None), (0, 40), (0, 60), (8, 8), (8, 20)])
def test_search_phrases_decodes_groups_and_merges_pieces(corpus, segment, max_rows):
    phrases, clips = corpus
    eng = CouplingEngine()
    got = M.search_phrases(phrases, clips, k=6, segment=segment, engine=eng, max_rows=max_rows)
    want = brute_phrases(phrases, clips, 6, segment)
    assert [a.dtype for a in got] == [np.int32, np.int32, np.float32] and got[0].shape == (3, 6)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[0][0, 0] == 5 and got[0][1, 0] == 2 and got[1][1, 0] == 0
    if segment:
        assert got[1][0, 0] in (0, 16) and np.all(got[1][got[0] >= 0] % 8 == 0)       # `start` is the first frame of the returned group
    else:
        assert np.all(got[1][got[0] >= 0] == 0)
    assert eng.names == ["sim_coupling"] * len(eng.calls) and all(c["n"] == 3 and c["k"] == 6 for c in eng.calls)
    assert [c["merge"] for c in eng.calls] == [False] + [True] * (len(eng.calls) - 1)
    assert sum(c["m"] for c in eng.calls) == 145
    assert [c["offset"] for c in eng.calls] == np.cumsum([0] + [c["groups"] for c in eng.calls[:-1]]).tolist()      # group_offset: the piece's first group
    if max_rows is None:
        assert len(eng.calls) == 1
    else:
        assert len(eng.calls) > 1 and all(c["m"] <= max_rows for c in eng.calls)
        one = M.search_phrases(phrases, clips, k=6, segment=segment, engine=CouplingEngine())
        assert all(np.array_equal(a, b) for a, b in zip(got, one))
    # search() and its walk are what they were: the same stand-in still answers it
    plain = M.search(np.concatenate(phrases), clips, k=4, segment=segment, engine=CouplingEngine(), max_rows=max_rows)
    assert plain[0].shape == (13, 4) and plain[0][1, 0] == 5 and plain[1][1, 0] == 17


def test_search_phrases_edge_cases(corpus):
    phrases, clips = corpus
    eng = CouplingEngine()
    with pytest.raises(ValueError, match="64"):
        M.search_phrases([np.zeros((65, 64), np.float32)], clips, engine=eng)
    for bad in ([np.zeros((0, 64), np.float32)], [np.zeros(64, np.float32)], [phrases[0], np.zeros((2, 128), np.float32)]):
        with pytest.raises(ValueError):
            M.search_phrases(bad, clips, engine=eng)
    for kw in (dict(k=0), dict(k=129), dict(segment=-1), dict(max_rows=0), dict(max_rows=39)):
        with pytest.raises(ValueError):
            M.search_phrases(phrases, clips, engine=eng, **kw)
    with pytest.raises(ValueError):
        M.search_phrases([p[:, :32] for p in phrases], clips, engine=eng)
    assert not eng.calls
    for nothing in (M.search_phrases([], clips, k=3, engine=eng), M.search_phrases(phrases, [], k=3, engine=eng),
                    M.search_phrases(phrases, [np.zeros((0, 64), np.float32)], k=3, engine=eng)):
        assert nothing[0].shape == nothing[1].shape == nothing[2].shape and nothing[0].shape[1] == 3
        assert np.all(nothing[0] == -1) and np.all(nothing[1] == -1) and np.all(np.isneginf(nothing[2]))
    clip, start, _ = M.search_phrases(phrases, [clips[0], np.zeros((0, 64), np.float32), clips[2]], k=3, engine=eng)
    assert np.all(np.sort(clip[:, :2], axis=1) == [0, 2]) and np.all(clip[:, 2] == -1) and np.all(start[:, 2] == -1)     # an empty clip has no score


def test_corpus_search_phrases_over_the_stored_rows(corpus):
    phrases, clips = corpus
    eng = CouplingEngine()
    c32 = M.Corpus.build(clips, dtype="float32", engine=eng)
    c16 = M.Corpus.build(clips, engine=eng)
    pn = [eng.l2norm(p).numpy() for p in phrases]
    widened = np.split(c16.rows.astype(np.float32), np.cumsum(c16.lengths)[:-1])
    for segment, max_rows in ((0, None), (8, 20)):
        want = M.search_phrases(phrases, clips, k=5, segment=segment, engine=CouplingEngine(), max_rows=max_rows)
        eng.calls.clear()
        got = c32.search_phrases(phrases, k=5, segment=segment, engine=eng, max_rows=max_rows)
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
        assert all(c["dtype"] == torch.float32 for c in eng.calls) and (len(eng.calls) == 1) == (max_rows is None)
        eng.calls.clear()
        got16 = c16.search_phrases(phrases, k=5, segment=segment, engine=eng, max_rows=max_rows)
        want16 = M.search_phrases(pn, widened, k=5, segment=segment, normalize=False, engine=CouplingEngine(), max_rows=max_rows)
        assert all(np.array_equal(a, b) for a, b in zip(got16, want16))
        assert all(c["dtype"] == torch.float16 for c in eng.calls) and got16[0][0, 0] == 5
    c16.search_phrases(phrases, k=3, engine=eng)                             # the device copy is kept between searches, as for search()
    assert eng.galleries[-1] is c16._dev[1]
    with pytest.raises(ValueError):
        c16.search_phrases([p[:, :32] for p in phrases], engine=eng)
    assert c16.search_phrases([], k=4, engine=eng)[0].shape == (0, 4)


def test_coupling_matrix_and_retrieval_metrics(corpus):
    phrases, clips = corpus
    rng = np.random.default_rng(9400)
    contents = [np.stack([c[i] for i in rng.integers(0, len(c), int(rng.integers(1, 10)))]) + 0.3 * rng.standard_normal((1, 64)).astype(np.float32)
                for c in clips]
    contents[4] = contents[6]                                                # two utterances with the same words: their rows tie
    eng = CouplingEngine()
    m = M.coupling_matrix(contents, clips, engine=eng)
    assert isinstance(m, torch.Tensor) and tuple(m.shape) == (9, 9) and m.dtype == torch.float32
    n = lambda x: eng.l2norm(x).numpy()
    want = C.coupling_scores(scores(np.concatenate([n(c) for c in contents]), np.concatenate([n(c) for c in clips])),
                             M.offsets_of(contents), M.offsets_of(clips))
    assert np.array_equal(m.numpy(), want) and np.array_equal(m.numpy()[4], m.numpy()[6])
    raw = M.coupling_matrix(contents, clips, normalize=False, engine=eng).numpy()
    assert np.array_equal(raw, C.coupling_scores(scores(np.concatenate(contents), np.concatenate(clips)), M.offsets_of(contents), M.offsets_of(clips)))
    res = M.coupling_retrieval_metrics(contents, clips, engine=eng)
    d = np.diag(want)
    for key, s in (("c2g", want), ("g2c", want.T)):
        rank, ties = (s > d[:, None]).sum(1), (s == d[:, None]).sum(1)
        assert res[key] == M.metrics_from_ranks(rank, ties), key
    assert (want[:, 4] == want[4, 4]).sum() == 2 and sorted(res["c2g"]) == ["MR", "R1", "R10", "R25", "R5", "R50"]
    with pytest.raises(ValueError):
        M.coupling_retrieval_metrics(contents[:3], clips, engine=eng)
    assert tuple(M.coupling_matrix([], clips, engine=eng).shape) == (0, 9)


# ------------------------------------------------------------------------------------------------ the drivers
def test_search_level_coupling_with_path_and_with_index(corpus, tmp_path, capsys):
    phrases, clips = corpus
    src = tmp_path / "pkl"
    src.mkdir()
    names = write_corpus(src, clips)
    query = tmp_path / "hello_there.pkl"
    with open(query, "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": phrases[0],
                     "info": {"fname": "hello_there", "word_boundaries": [["hello", 0, 4], ["there", 5, 9], ["now", 10, 12]]}}, f)
    eng = CouplingEngine()
    assert drivers.cmd_index(["--path", str(src), "--out", str(tmp_path / "c32.npz"), "--dtype", "float32"], engine=eng) == 0
    capsys.readouterr()
    for extra, segment, max_rows in (([], 0, None), (["--segment", "8", "--max_rows", "24"], 8, 24)):
        want = brute_phrases(phrases[:1], clips, 4, segment)
        outs = []
        for n, corpus_args in enumerate((["--path", str(src)], ["--index", str(tmp_path / "c32.npz")])):
            res = tmp_path / f"res{len(extra)}_{n}"
            eng.calls.clear()
            assert drivers.cmd_search(corpus_args + ["--query", str(query), "--level", "coupling", "--topk", "4", "--res_dir", str(res)] + extra,
                                      engine=eng) == 0
            assert eng.calls and all(c["n"] == 1 for c in eng.calls)         # the three words are ONE query
            lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("search: \"")]
            assert len(lines) == 1 and lines[0].startswith("search: \"hello there now\" -> 4 of 9 clips: vid005__t@")
            z = np.load(res / "search_hello_there.npz")
            assert sorted(z.files) == ["clip", "frame", "names", "score", "start", "words"]
            assert list(z["names"]) == names and list(z["words"]) == ["hello there now"]
            assert np.array_equal(z["clip"], want[0]) and np.array_equal(z["start"], want[1]) and np.array_equal(z["score"], want[2])
            assert np.array_equal(z["frame"], z["start"]) and z["start"].dtype == np.int32      # readers of `frame` keep working
            outs.append(z)
        assert all(np.array_equal(outs[0][key], outs[1][key]) for key in outs[0].files)
    # more than 64 words: refused with the limit named, before any engine call
    long_query = tmp_path / "long.pkl"
    with open(long_query, "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": np.ones((65, 64), np.float32), "info": {"fname": "long"}}, f)
    eng.calls.clear()
    for corpus_args in (["--path", str(src)], ["--index", str(tmp_path / "c32.npz")]):
        with pytest.raises(SystemExit, match="64"):
            drivers.cmd_search(corpus_args + ["--query", str(long_query), "--level", "coupling"], engine=eng)
    assert not eng.calls
    assert drivers.cmd_search(["--path", str(src), "--query", str(long_query), "--level", "phrase", "--topk", "2", "--res_dir", str(tmp_path / "p")],
                              engine=eng) == 0                               # (the other levels have no such limit)
    assert sorted(np.load(tmp_path / "p" / "search_long.npz").files) == ["clip", "frame", "names", "score", "words"]


def test_evaluate_retrieval_score_switch(corpus, tmp_path, capsys):
    phrases, clips = corpus
    rng = np.random.default_rng(9500)
    contents = [np.stack([c[i] for i in rng.integers(0, len(c), int(rng.integers(1, 10)))]) for c in clips]
    src = tmp_path / "pkl"
    src.mkdir()
    for i, (g, c) in enumerate(zip(clips, contents)):
        with open(src / f"vid{i:03d}__t.pkl", "wb") as f:
            pickle.dump({"gesture_emb": g, "content_emb": c, "info": {"fname": f"vid{i:03d}__t"}}, f)
    line = "R@1: {:.2f} - R@5: {:.2f} - R@10: {:.2f} - R@25: {:.2f} - R@50: {:.2f} | Median R: {:.1f}"
    fmt = lambda m: line.format(m["R1"] * 100, m["R5"] * 100, m["R10"] * 100, m["R25"] * 100, m["R50"] * 100, m["MR"])
    # pooled, the default: exactly the calls and the lines of the command as it was
    outs = []
    for argv in (["--path", str(src)], ["--path", str(src), "--score", "pooled"]):
        eng = CouplingEngine()
        res = drivers.cmd_evaluate_retrieval(argv, engine=eng)
        assert eng.names == ["pool_mean", "pool_mean", "sim_rank", "sim_rank"]
        gv, cv = M.video_level(eng, clips), M.video_level(eng, contents)
        assert res == {"Content to Gesture": M.retrieval_metrics(cv, gv, engine=eng), "Gesture to Content": M.retrieval_metrics(gv, cv, engine=eng)}
        outs.append(capsys.readouterr().out)
        assert outs[-1].splitlines() == ["No of files =  9", "Content to Gesture Retrieval scores:", fmt(res["Content to Gesture"]),
                                         "Gesture to Content Retrieval scores:", fmt(res["Gesture to Content"])]
    assert outs[0] == outs[1]
    eng = CouplingEngine()
    res = drivers.cmd_evaluate_retrieval(["--path", str(src), "--score", "coupling"], engine=eng)
    assert eng.names == ["sim_coupling"]
    want = M.coupling_retrieval_metrics(contents, clips, engine=eng)
    assert res == {"Content to Gesture": want["c2g"], "Gesture to Content": want["g2c"]}
    assert capsys.readouterr().out.splitlines() == ["No of files =  9", "Content to Gesture Retrieval scores:", fmt(want["c2g"]),
                                                    "Gesture to Content Retrieval scores:", fmt(want["g2c"])]
    assert res["Content to Gesture"]["R1"] == 1.0                            # every word of an utterance is a frame of its own clip
    with pytest.raises(SystemExit):
        drivers.cmd_evaluate_retrieval(["--path", str(src), "--score", "other"], engine=eng)
