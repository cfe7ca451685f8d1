"""The host side of jg_sim_search without a GPU: the planner that cuts a gallery into slices (jg_debug_search_plan: a pure host function of
the library), the argument checks Engine.sim_search makes before it needs a device, and metrics.Corpus with the index / search --index
drivers on a stand-in engine that computes sim_search with numpy (the stand-in of tests/test_sim_topk_grouped_cpu.py, one method more)."""
import itertools
import pickle

import numpy as np
import pytest
import torch

from jegal_amd import drivers, metrics as M
from jegal_amd._lib import _SIGS, EXPORTS, Engine, JegalError, search_plan
from jegal_amd._metric_entries import SIM_SEARCH_MAX_SLICES, SIM_SEARCH_MAX_WS
from test_sim_topk_grouped_cpu import NumpyEngine, grouped_reference, scores, write_corpus


class SearchEngine(NumpyEngine):
    """... and sim_search with Engine.sim_search's contract: the gallery is widened, then scored as sim_topk_grouped scores it"""

    def __init__(self):
        super().__init__()
        self.galleries = []

    def sim_search(self, queries, gallery, k, g_offsets=None, gallery_offset=0, merge_into=None, slices=0):
        assert isinstance(gallery, torch.Tensor) and gallery.dtype in (torch.float16, torch.float32)
        off = np.asarray(g_offsets, np.int64)
        assert off[0] == 0 and off[-1] == gallery.shape[0] and np.all(np.diff(off) >= 0)          # a piece is cut at group boundaries
        self.calls.append(dict(n=queries.shape[0], m=gallery.shape[0], groups=len(off) - 1, k=k, offset=gallery_offset, merge=merge_into is not None,
                               dtype=gallery.dtype))
        self.galleries.append(gallery)
        init = None if merge_into is None else (merge_into[0].numpy(), merge_into[1].numpy())
        idx, sc = grouped_reference(scores(queries.numpy(), gallery.float().numpy()), off, k, gallery_offset, init)
        return torch.from_numpy(idx), torch.from_numpy(sc)


# ------------------------------------------------------------------------------------------------ the planner
def check_plan(nq, ng, k, num_cu, slices_in=0):
    S, R, ws = search_plan(nq, ng, k, num_cu, slices_in)
    tiles = -(-ng // 64)
    assert R > 0 and R % 64 == 0, (nq, ng, k, num_cu, slices_in)
    assert 1 <= S <= max(tiles, 1) and S <= SIM_SEARCH_MAX_SLICES
    assert (S - 1) * R < max(ng, 1) and S * R >= ng                     # every slice holds a row, and together they hold all rows
    assert ws == (S * nq * k * 8 if S > 1 else 0) and ws <= SIM_SEARCH_MAX_WS
    return S, R, ws


def test_plan_cuts_whole_tiles_and_covers_the_gallery():
    assert len(_SIGS["jg_debug_search_plan"]) == 8 and "jg_debug_search_plan" in EXPORTS
    queries = [1, 2, 63, 64, 65, 500, 511, 512, 513, 1024, 16320, 16321, 20000]
    galleries = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4096, 600000, 2 ** 21 - 1, 2 ** 21]
    for nq, ng, k, num_cu in itertools.product(queries, galleries, (1, 128), (8, 256)):
        S, R, ws = check_plan(nq, ng, k, num_cu)
        if -(-nq // 64) >= num_cu:
            assert S == 1, (nq, ng, k, num_cu)                          # the query blocks alone fill the device
        for forced in (1, 2, 3, 7, max(-(-ng // 64), 1), -(-ng // 64) + 5, SIM_SEARCH_MAX_SLICES):
            tiles = max(-(-ng // 64), 1)
            want = min(forced, tiles)
            per = -(-tiles // want)
            want = -(-tiles // per)                                     # the tiles dealt out evenly: never more slices than asked for
            if forced > SIM_SEARCH_MAX_SLICES or (want > 1 and want * nq * k * 8 > SIM_SEARCH_MAX_WS):
                with pytest.raises(JegalError):
                    search_plan(nq, ng, k, num_cu, forced)
            else:
                assert check_plan(nq, ng, k, num_cu, forced)[:2] == (want, per * 64), (nq, ng, k, num_cu, forced)
    # one query row against the README's corpus: every CU gets work
    S, R, _ = search_plan(1, 600000, 10, 256)
    assert 256 <= S <= SIM_SEARCH_MAX_SLICES
    assert search_plan(1, 600000, 10, 8)[0] < S                         # ... and a small device fewer slices
    assert search_plan(0, 1000, 10, 256) == (1, 1024, 0)                # no query: nothing to cut
    for bad in (dict(n_queries=-1), dict(n_gallery=-1), dict(k=0), dict(k=129), dict(num_cu=0), dict(slices=-1), dict(slices=SIM_SEARCH_MAX_SLICES + 1)):
        with pytest.raises(JegalError):
            search_plan(**{**dict(n_queries=5, n_gallery=1000, k=10, num_cu=256, slices=0), **bad})


# ------------------------------------------------------------------------------------------------ Engine.sim_search
def test_engine_refuses_bad_arguments_before_it_needs_a_device():
    assert len(_SIGS["jg_sim_search"]) == 15 and "jg_sim_search" in EXPORTS
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    q, g = torch.zeros(20, 512), torch.zeros(30, 512)
    off = [0, 10, 10, 30]
    ok_i, ok_s = torch.zeros(20, 5, dtype=torch.int32), torch.zeros(20, 5)
    bad = [dict(queries=torch.zeros(512), gallery=g, k=5),                                         # not (rows, D)
           dict(queries=q, gallery=torch.zeros(30, 256), k=5),                                     # different D
           dict(queries=torch.zeros(20, 96), gallery=torch.zeros(30, 96), k=5),                    # D % 64
           dict(queries=torch.zeros(20, 0), gallery=torch.zeros(30, 0), k=5),                      # D = 0
           dict(queries=q, gallery=g.double(), k=5), dict(queries=q, gallery=g.to(torch.bfloat16), k=5),       # gallery types
           dict(queries=q, gallery=g.to(torch.int32), k=5), dict(queries=q, gallery=np.zeros((30, 512), np.float64), k=5),
           dict(queries=q, gallery=[[0.0] * 512] * 30, k=5),
           dict(queries=q, gallery=g, k=0), dict(queries=q, gallery=g, k=129),
           dict(queries=q, gallery=g, k=5, gallery_offset=-1),
           dict(queries=q, gallery=g, k=5, gallery_offset=2 ** 31 - 30),                           # gallery_offset + rows > INT32_MAX
           dict(queries=q, gallery=g, k=5, slices=-1), dict(queries=q, gallery=g, k=5, slices=SIM_SEARCH_MAX_SLICES + 1),
           dict(queries=torch.zeros(70000, 64), gallery=torch.zeros(128, 64), k=128, slices=2),    # 2 x 70000 x 128 keys: beyond the lists' cap
           dict(queries=q, gallery=g, k=5, g_offsets=[]),                                          # no entry at all
           dict(queries=q, gallery=g, k=5, g_offsets=[[0, 30]]),                                   # not 1-d
           dict(queries=q, gallery=g, k=5, g_offsets=[0.0, 30.0]),                                 # not integers
           dict(queries=q, gallery=g, k=5, g_offsets=[0, 20, 10, 30]),                             # decreasing
           dict(queries=q, gallery=g, k=5, g_offsets=[-1, 30]),
           dict(queries=q, gallery=g, k=5, g_offsets=[0, 31]),                                     # beyond the gallery
           dict(queries=q, gallery=g, k=5, g_offsets=torch.zeros(4)),                              # a float tensor
           dict(queries=q, gallery=g, k=5, g_offsets=off, merge_into=ok_i),                        # not a pair
           dict(queries=q, gallery=g, k=5, merge_into=(ok_i, ok_s[:, :4])),                        # shapes
           dict(queries=q, gallery=g, k=5, merge_into=(ok_i.to(torch.int64), ok_s)),               # dtypes
           dict(queries=q, gallery=g, k=5, g_offsets=off, merge_into=(ok_s, ok_i))]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.sim_search(**kw)
    # what is in order gets past every check and fails at the first use of the handle
    for kw in (dict(queries=q, gallery=g, k=5), dict(queries=q, gallery=g.half(), k=128, g_offsets=off, slices=SIM_SEARCH_MAX_SLICES),
               dict(queries=q, gallery=np.zeros((30, 512), np.float16), k=1, gallery_offset=2 ** 31 - 31, slices=1),
               dict(queries=torch.zeros(70000, 64), gallery=torch.zeros(128, 64), k=128, slices=1)):
        with pytest.raises(AttributeError):
            eng.sim_search(**kw)


# ------------------------------------------------------------------------------------------------ metrics.Corpus
@pytest.fixture(scope="module")
def clips():
    """9 clips of 1..40 frames, D = 64, rows of any length; query 0 points along frame 17 of clip 5, query 1 along frame 0 of clip 2"""
    rng = np.random.default_rng(7411)
    lens = [12, 1, 30, 7, 40, 25, 3, 18, 9]
    c = [(rng.standard_normal((t, 64)) * rng.uniform(0.5, 3.0, (t, 1))).astype(np.float32) for t in lens]
    q = np.stack([c[5][17] * 2.0, c[2][0] * 0.5, rng.standard_normal(64).astype(np.float32)])
    return q, c


@pytest.mark.parametrize("segment,max_rows", [(0, None), (7, None), (0, 40), (0, 60), (7, 7), (7, 20)])
def test_float32_corpus_returns_the_triple_of_search(clips, segment, max_rows):
    q, c = clips
    want = M.search(q, c, k=6, segment=segment, engine=NumpyEngine(), max_rows=max_rows)
    eng = SearchEngine()
    corpus = M.Corpus.build(c, dtype="float32", engine=eng)
    assert corpus.rows.dtype == np.float32 and corpus.normalized and corpus.lengths.tolist() == [len(x) for x in c]
    got = corpus.search(q, k=6, segment=segment, engine=eng, max_rows=max_rows)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    assert (got[0][0, 0], got[1][0, 0]) == (5, 17) and (got[0][1, 0], got[1][1, 0]) == (2, 0)
    assert all(cl["dtype"] == torch.float32 for cl in eng.calls)
    assert [cl["merge"] for cl in eng.calls] == [False] + [True] * (len(eng.calls) - 1)
    assert sum(cl["m"] for cl in eng.calls) == 145 and [cl["offset"] for cl in eng.calls] == np.cumsum([0] + [cl["m"] for cl in eng.calls[:-1]]).tolist()
    if max_rows is None:
        assert len(eng.calls) == 1
        corpus.search(q[:1], k=3, engine=eng)                               # the device copy is kept: the same tensor goes in again
        assert eng.galleries[-1] is eng.galleries[0]
        other = SearchEngine()
        corpus.search(q[:1], k=3, engine=other)                             # ... per engine
        assert other.galleries[0] is not eng.galleries[0]
    else:
        assert len(eng.calls) > 1 and all(cl["m"] <= max_rows for cl in eng.calls)


def test_corpus_edge_cases(clips):
    q, c = clips
    eng = SearchEngine()
    corpus = M.Corpus.build(c, dtype="float32", engine=eng)
    with pytest.raises(ValueError):
        corpus.search(q, k=6, engine=eng, max_rows=39)                      # the 40-frame clip is one group
    for bad in (dict(k=0), dict(k=129), dict(segment=-1), dict(max_rows=0)):
        with pytest.raises(ValueError):
            corpus.search(q, engine=eng, **{"k": 5, **bad})
    with pytest.raises(ValueError):
        corpus.search(q[:, :32], engine=eng)
    with pytest.raises(ValueError):
        corpus.search(q[0], engine=eng)
    assert not eng.calls
    with pytest.raises(ValueError):
        M.Corpus.build(c, dtype="float64", engine=eng)
    with pytest.raises(ValueError):
        M.Corpus.build(c, names=["a"], engine=eng)
    for nothing in (M.Corpus.build([], engine=eng).search(q, k=3, engine=eng),
                    M.Corpus.build([np.zeros((0, 64), np.float32)], engine=eng).search(q, k=3, engine=eng),
                    corpus.search(np.zeros((0, 64), np.float32), k=3, engine=eng)):
        assert nothing[0].shape == nothing[1].shape == nothing[2].shape and nothing[0].shape[1] == 3
        assert np.all(nothing[0] == -1) and np.all(nothing[1] == -1) and np.all(np.isneginf(nothing[2]))
    with_empty = M.Corpus.build([c[0], np.zeros((0, 64), np.float32), c[2]], engine=eng)
    clip, frame, _ = with_empty.search(q, k=3, engine=eng)                  # an empty clip is an empty group: never returned
    assert np.all(np.sort(clip[:, :2], axis=1) == [0, 2]) and np.all(clip[:, 2] == -1) and (clip[1, 0], frame[1, 0]) == (2, 0)
    raw = M.Corpus.build(c, dtype="float32", normalize=False)               # the rows as they are: no engine is asked for anything
    assert not raw.normalized and np.array_equal(raw.rows, np.concatenate(c, 0))


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_save_and_load_are_bit_equal(clips, tmp_path, dtype):
    q, c = clips
    eng = SearchEngine()
    corpus = M.Corpus.build(c, names=[f"clip{i}" for i in range(len(c))], dtype=dtype, engine=eng)
    corpus.save(tmp_path / "corpus.npz")
    with np.load(tmp_path / "corpus.npz") as z:
        assert sorted(z.files) == ["lengths", "names", "normalized", "rows", "version"]
    back = M.Corpus.load(tmp_path / "corpus.npz")
    assert back.rows.dtype == np.dtype(dtype) and np.array_equal(back.rows.view(np.uint8), corpus.rows.view(np.uint8))
    assert np.array_equal(back.lengths, corpus.lengths) and back.names.tolist() == corpus.names.tolist() and back.normalized is True
    a, b = corpus.search(q, k=5, segment=7, engine=eng), back.search(q, k=5, segment=7, engine=eng)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_float16_corpus_is_searched_as_stored(clips):
    """The rows are float32-normalised, then rounded as numpy rounds; the search is search() on the widened stored rows; and a score is
    within sum_d |q_d| (2^-11 |g_d| + 2^-25) + 2 D 2^-24 sum_d |q_d g_d| of the float32 corpus's for the same row (fp16 rounding to
    nearest: 2^-11 relative, 2^-25 absolute below the normal range; the two fp32 chain bounds of tests/test_gpu_sim_topk.py)."""
    q, c = clips
    eng = SearchEngine()
    c32 = M.Corpus.build(c, dtype="float32", engine=eng)
    c16 = M.Corpus.build(c, engine=eng)                                     # (float16 is the default)
    assert c16.rows.dtype == np.float16 and np.array_equal(c16.rows.view(np.uint16), c32.rows.astype(np.float16).view(np.uint16))
    qn = eng.l2norm(q).numpy()
    widened = np.split(c16.rows.astype(np.float32), np.cumsum(c16.lengths)[:-1])
    for segment, max_rows in ((0, None), (7, 20)):
        got = c16.search(q, k=8, segment=segment, engine=eng, max_rows=max_rows)
        want = M.search(qn, widened, k=8, segment=segment, normalize=False, engine=NumpyEngine(), max_rows=max_rows)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert (got[0][0, 0], got[1][0, 0]) == (5, 17) and (got[0][1, 0], got[1][1, 0]) == (2, 0)
        ref = c32.search(q, k=8, segment=segment, engine=eng, max_rows=max_rows)
        first = np.concatenate([[0], np.cumsum(c32.lengths)])
        g32 = c32.rows.astype(np.float64)
        bound = np.abs(qn.astype(np.float64)) @ (2.0 ** -11 * np.abs(g32) + 2.0 ** -25).T + 2 * 64 * 2.0 ** -24 * (np.abs(qn.astype(np.float64)) @ np.abs(g32).T)
        for i in range(len(q)):
            found = got[0][i] >= 0
            rows = first[got[0][i][found]] + got[1][i][found]
            s32 = scores(qn[i:i + 1], c32.rows[rows])[0]
            assert np.all(np.abs(got[2][i][found].astype(np.float64) - s32) <= bound[i, rows]), (segment, i)
            # every score moved by at most the largest bound, so the r-th best champion did too
            assert np.all(np.abs(got[2][i][found].astype(np.float64) - ref[2][i][found]) <= bound[i].max()), (segment, i)
    assert {cl["dtype"] for cl in eng.calls} == {torch.float16, torch.float32}


def test_index_then_search_index_writes_what_search_path_writes(clips, tmp_path, capsys):
    q, c = clips
    src = tmp_path / "pkl"
    src.mkdir()
    names = write_corpus(src, c)
    with open(src / "text_only.pkl", "wb") as f:                            # a .pkl without gesture_emb is no clip, for either command
        pickle.dump({"gesture_emb": None, "content_emb": q, "info": {"fname": "text_only"}}, f)
    query = tmp_path / "hello_there.pkl"
    with open(query, "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": q,
                     "info": {"fname": "hello_there", "word_boundaries": [["hello", 0, 4], ["there", 5, 9], ["now", 10, 12]]}}, f)
    assert "index" in drivers.COMMANDS
    eng = SearchEngine()
    assert drivers.cmd_index(["--path", str(src), "--out", str(tmp_path / "c32.npz"), "--dtype", "float32"], engine=eng) == 0
    assert drivers.cmd_index(["--path", str(src), "--out", str(tmp_path / "c16")], engine=eng) == 0          # (.npz is added)
    assert "index: 9 clips, 145 rows x 64 float16" in capsys.readouterr().out
    c16 = M.Corpus.load(tmp_path / "c16.npz")
    assert c16.rows.dtype == np.float16 and c16.names.tolist() == names and c16.lengths.tolist() == [len(x) for x in c]
    for extra in ([], ["--segment", "16", "--max_rows", "48", "--level", "phrase", "--topk", "12"]):
        outs = []
        for n, corpus_args in enumerate((["--path", str(src)], ["--index", str(tmp_path / "c32.npz")])):
            res = tmp_path / f"res{len(extra)}_{n}"
            assert drivers.cmd_search(corpus_args + ["--query", str(query), "--topk", "4", "--res_dir", str(res)] + extra, engine=eng) == 0
            outs.append(([l for l in capsys.readouterr().out.splitlines() if l.startswith("search: ")], np.load(res / "search_hello_there.npz")))
        (lines_p, zp), (lines_i, zi) = outs
        assert sorted(zi.files) == sorted(zp.files) == ["clip", "frame", "names", "score", "words"]
        for key in zp.files:
            assert zi[key].dtype == zp[key].dtype and np.array_equal(zi[key], zp[key]), key
        assert [l.replace(str(tmp_path / f"res{len(extra)}_1"), "") for l in lines_i] == [l.replace(str(tmp_path / f"res{len(extra)}_0"), "") for l in lines_p]
        assert lines_i[0].startswith("search: \"hello") and "vid005__t@17" in lines_i[0]
    res = tmp_path / "res16"
    assert drivers.cmd_search(["--index", str(tmp_path / "c16.npz"), "--query", str(query), "--topk", "4", "--res_dir", str(res)], engine=eng) == 0
    z16 = np.load(res / "search_hello_there.npz")
    assert np.array_equal(z16["clip"][:2, 0], [5, 2]) and np.array_equal(z16["frame"][:2, 0], [17, 0]) and np.allclose(z16["score"][:2, 0], 1.0, atol=1e-3)
    for wrong in ([], ["--path", str(src), "--index", str(tmp_path / "c32.npz")]):                 # exactly one of the two
        with pytest.raises(SystemExit):
            drivers.cmd_search(wrong + ["--query", str(query)], engine=eng)
    with pytest.raises(SystemExit):
        drivers.cmd_index(["--path", str(tmp_path / "res16"), "--out", str(tmp_path / "none.npz")], engine=eng)      # no .pkl there
