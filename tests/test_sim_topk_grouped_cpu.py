"""The host side of the grouped top-k feature without a GPU: metrics.search and the search driver reach the device only through
engine.l2norm / sim_topk_grouped / group_of_rows, so a stand-in engine that computes them with numpy drives them here; plus the argument
checks Engine.sim_topk_grouped and Engine.group_of_rows make before they need a device, and the two names in the ctypes table."""
import pickle

import numpy as np
import pytest
import torch

from jegal_amd import drivers, metrics as M
from jegal_amd._lib import _SIGS, EXPORTS, Engine


def scores(q, g):
    """float64 dot products rounded to fp32: what any exact-enough fp32 kernel returns, whatever its blocking"""
    return (np.asarray(q, np.float64) @ np.asarray(g, np.float64).T).astype(np.float32)


def grouped_reference(s, off, k, offset=0, init=None):
    """s (nq, ng) scores, off: group offsets (local rows) -> (idx, score) of jg_sim_topk_grouped: per group its first arg-max row, the k best
    of those by (score descending, row ascending), merged with init = (idx, score) of other rows"""
    nq = s.shape[0]
    idx = np.full((nq, k), -1, np.int32)
    sc = np.full((nq, k), -np.inf, np.float32)
    for i in range(nq):
        cand = []
        if init is not None:
            cand = [(-float(v), int(j)) for j, v in zip(init[0][i], init[1][i]) if j >= 0]
        for a, b in zip(off[:-1], off[1:]):
            row = np.where(np.isnan(s[i, a:b]), -np.inf, s[i, a:b] + 0.0)
            if b > a and not np.all(np.isnan(s[i, a:b])):
                j = int(np.argmax(row))
                cand.append((-float(row[j]), offset + int(a) + j))
        cand.sort()
        for r, (v, j) in enumerate(cand[:k]):
            idx[i, r], sc[i, r] = j, -v
    return idx, sc


class NumpyEngine:
    """l2norm / sim_topk_grouped / group_of_rows with the Engine's contracts, computed on the host"""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def l2norm(self, x):
        x = torch.as_tensor(x, dtype=torch.float32)
        return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)

    def sim_topk_grouped(self, queries, gallery, g_offsets, k, gallery_offset=0, merge_into=None):
        off = np.asarray(g_offsets, np.int64)
        assert off[0] == 0 and off[-1] == gallery.shape[0] and np.all(np.diff(off) >= 0)      # a piece is cut at group boundaries
        self.calls.append(dict(n=queries.shape[0], m=gallery.shape[0], groups=len(off) - 1, k=k, offset=gallery_offset, merge=merge_into is not None))
        init = None if merge_into is None else (merge_into[0].numpy(), merge_into[1].numpy())
        idx, sc = grouped_reference(scores(queries.numpy(), gallery.numpy()), off, k, gallery_offset, init)
        return torch.from_numpy(idx), torch.from_numpy(sc)

    def group_of_rows(self, idx, g_offsets, gallery_offset=0):
        off = np.asarray(g_offsets, np.int64)
        j = idx.numpy().astype(np.int64) - gallery_offset
        ok = (idx.numpy() >= 0) & (j >= off[0]) & (j < off[-1])
        grp = np.where(ok, np.searchsorted(off, j, side="right") - 1, -1)
        pos = np.where(ok, j - off[np.maximum(grp, 0)], -1)
        return torch.from_numpy(grp.astype(np.int32)), torch.from_numpy(pos.astype(np.int32))


@pytest.fixture(scope="module")
def corpus():
    """9 clips of 1..40 frames, D = 64, unit rows; query 0 equals frame 17 of clip 5, query 1 frame 0 of clip 2, query 2 is random"""
    rng = np.random.default_rng(7301)
    lens = [12, 1, 30, 7, 40, 25, 3, 18, 9]
    clips = [rng.standard_normal((t, 64)).astype(np.float32) for t in lens]
    clips = [c / np.linalg.norm(c, axis=1, keepdims=True) for c in clips]
    q = np.stack([clips[5][17], clips[2][0], rng.standard_normal(64).astype(np.float32)])
    return q, clips


def brute(q, clips, k, segment=0, normalize=True):
    """metrics.search by its definition: every group's best frame, the k best groups"""
    n = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12) if normalize else x
    qn = n(np.asarray(q, np.float32)).astype(np.float32)
    out = []
    for i in range(len(qn)):
        cand = []
        for c, rows in enumerate(clips):
            s = scores(qn[i:i + 1], n(rows).astype(np.float32))[0]
            step = segment if segment > 0 else len(s)
            for a in range(0, len(s), step):
                j = a + int(np.argmax(s[a:a + step]))
                cand.append((-float(s[j]), c, j))
        cand.sort()
        out.append(cand[:k] + [(np.inf, -1, -1)] * (k - len(cand[:k])))
    clip = np.asarray([[c for _, c, _ in row] for row in out], np.int32)
    frame = np.asarray([[f for _, _, f in row] for row in out], np.int32)
    score = np.asarray([[-v for v, _, _ in row] for row in out], np.float32)
    return clip, frame, score


def test_search_groups_cut_clips_into_segments():
    off, clip, start = M.search_groups([5, 0, 7], 0)
    assert off.tolist() == [0, 5, 5, 12] and clip.tolist() == [0, 1, 2] and start.tolist() == [0, 0, 0]
    off, clip, start = M.search_groups([5, 0, 7], 3)             # the last run of a clip is shorter; every clip ends a group
    assert off.tolist() == [0, 3, 5, 5, 8, 11, 12] and clip.tolist() == [0, 0, 1, 2, 2, 2] and start.tolist() == [0, 3, 0, 0, 3, 6]


def test_search_finds_the_clip_and_the_frame(corpus):
    q, clips = corpus
    eng = NumpyEngine()
    clip, frame, score = M.search(q * 3.0, [c * 0.5 for c in clips], k=4, engine=eng)         # un-normalised rows in
    assert eng.calls == [dict(n=3, m=145, groups=9, k=4, offset=0, merge=False)]
    assert clip.dtype == np.int32 and frame.dtype == np.int32 and score.dtype == np.float32 and clip.shape == frame.shape == score.shape == (3, 4)
    assert (clip[0, 0], frame[0, 0]) == (5, 17) and (clip[1, 0], frame[1, 0]) == (2, 0)
    assert np.allclose(score[:2, 0], 1.0, atol=1e-6)
    want = brute(q, clips, 4)
    assert np.array_equal(clip, want[0]) and np.array_equal(frame, want[1]) and np.allclose(score, want[2], atol=1e-6)
    for i in range(3):
        assert len(set(clip[i].tolist())) == 4                   # never two frames of one clip
    raw = M.search(q * 3.0, clips, k=4, normalize=False, engine=eng)                          # the rows as stored: the scores scale
    want_raw = brute(q * 3.0, clips, 4, normalize=False)
    assert np.array_equal(raw[0], want_raw[0]) and np.array_equal(raw[1], want_raw[1]) and np.allclose(raw[2], want_raw[2], atol=1e-5)
    assert np.allclose(raw[2][:2, 0], 3.0, atol=1e-5)
    as_lists = M.search([row for row in q], [torch.from_numpy(c) for c in clips], k=4, engine=eng)
    assert np.array_equal(as_lists[0], clip) and np.array_equal(as_lists[1], frame) and np.allclose(as_lists[2], score, atol=1e-6)


def test_search_segments_return_several_moments_of_a_clip(corpus):
    q, clips = corpus
    eng = NumpyEngine()
    clip, frame, score = M.search(q, clips, k=30, segment=8, engine=eng)
    n_groups = sum(-(-len(c) // 8) for c in clips)               # 23 groups: 7 empty slots behind them
    assert eng.calls[-1]["groups"] == n_groups == 23
    want = brute(q, clips, 30, segment=8)
    assert np.array_equal(clip, want[0]) and np.array_equal(frame, want[1]) and np.allclose(score, want[2], atol=1e-6)
    assert np.all(clip[:, 23:] == -1) and np.all(frame[:, 23:] == -1) and np.all(np.isneginf(score[:, 23:]))
    assert (clip[0, 0], frame[0, 0]) == (5, 17)
    for i in range(3):                                           # one entry per (clip, run of 8 frames), and clip 4 (40 frames) with all 5 of its runs
        runs = list(zip(clip[i, :23].tolist(), (frame[i, :23] // 8).tolist()))
        assert len(set(runs)) == 23 and sum(1 for c, _ in runs if c == 4) == 5
    plain = M.search(q, clips, k=1, engine=eng)                  # the best moment of all is the same with and without segments
    assert np.array_equal(plain[0][:, 0], clip[:, 0]) and np.array_equal(plain[1][:, 0], frame[:, 0]) and np.array_equal(plain[2][:, 0], score[:, 0])


@pytest.mark.parametrize("segment,max_rows", [(0, 40), (0, 60), (8, 8), (8, 20), (0, 1000)])
def test_search_in_pieces_equals_the_single_call(corpus, segment, max_rows):
    q, clips = corpus
    one = M.search(q, clips, k=6, segment=segment, engine=NumpyEngine())
    eng = NumpyEngine()
    got = M.search(q, clips, k=6, segment=segment, engine=eng, max_rows=max_rows)
    assert all(np.array_equal(a, b) for a, b in zip(got, one))
    assert all(c["m"] <= max_rows for c in eng.calls)
    assert [c["merge"] for c in eng.calls] == [False] + [True] * (len(eng.calls) - 1)
    assert sum(c["m"] for c in eng.calls) == 145 and [c["offset"] for c in eng.calls] == np.cumsum([0] + [c["m"] for c in eng.calls[:-1]]).tolist()
    if max_rows < 145:
        assert len(eng.calls) > 1


def test_search_edge_cases(corpus):
    q, clips = corpus
    eng = NumpyEngine()
    with pytest.raises(ValueError):
        M.search(q, clips, k=6, engine=eng, max_rows=39)         # the 40-frame clip is one group: groups are never split
    for bad in (dict(k=0), dict(k=129), dict(segment=-1), dict(max_rows=0)):
        with pytest.raises(ValueError):
            M.search(q, clips, engine=eng, **{"k": 5, **bad})
    with pytest.raises(ValueError):
        M.search(q[:, :32], clips, engine=eng)
    with pytest.raises(ValueError):
        M.search(q[0], clips, engine=eng)
    assert not eng.calls                                         # every refusal came before the engine was asked for anything
    for nothing in (M.search(q, [], k=3, engine=eng), M.search(q, [np.zeros((0, 64), np.float32)], k=3, engine=eng),
                    M.search(np.zeros((0, 64), np.float32), clips, k=3, engine=eng)):
        assert nothing[0].shape == nothing[1].shape == nothing[2].shape and nothing[0].shape[1] == 3
        assert np.all(nothing[0] == -1) and np.all(nothing[1] == -1) and np.all(np.isneginf(nothing[2]))
    with_empty = [clips[0], np.zeros((0, 64), np.float32), clips[2]]
    clip, frame, score = M.search(q, with_empty, k=3, engine=eng)            # an empty clip is an empty group: never returned
    assert np.all(np.sort(clip[:, :2], axis=1) == [0, 2]) and np.all(clip[:, 2] == -1) and (clip[1, 0], frame[1, 0]) == (2, 0)


def write_corpus(path, clips):
    names = []
    for i, g in enumerate(clips):
        names.append(f"vid{i:03d}__t")
        with open(path / (names[-1] + ".pkl"), "wb") as f:
            pickle.dump({"gesture_emb": g, "content_emb": None, "info": {"fname": names[-1]}}, f)
    return names


def test_search_driver_writes_npz(corpus, tmp_path, capsys):
    q, clips = corpus
    src, res = tmp_path / "pkl", tmp_path / "res"
    src.mkdir()
    names = write_corpus(src, clips)
    query = tmp_path / "hello_there.pkl"
    with open(query, "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": q * 2.0,
                     "info": {"fname": "hello_there", "word_boundaries": [["hello", 0, 4], ["there", 5, 9], ["now", 10, 12]]}}, f)
    assert "search" in drivers.COMMANDS
    eng = NumpyEngine()
    assert drivers.cmd_search(["--path", str(src), "--query", str(query), "--topk", "4", "--res_dir", str(res)], engine=eng) == 0
    assert [p.name for p in res.iterdir()] == ["search_hello_there.npz"]
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("search: \"")]
    assert len(lines) == 3 and lines[0].startswith("search: \"hello\" -> 4 of 9 clips: vid005__t@17")       # one line per query row
    z = np.load(res / "search_hello_there.npz")
    assert sorted(z.files) == ["clip", "frame", "names", "score", "words"]
    assert list(z["names"]) == names and list(z["words"]) == ["hello", "there", "now"]
    want = brute(q, clips, 4)
    assert z["clip"].dtype == np.int32 and z["frame"].dtype == np.int32 and z["score"].dtype == np.float32
    assert np.array_equal(z["clip"], want[0]) and np.array_equal(z["frame"], want[1]) and np.allclose(z["score"], want[2], atol=1e-6)
    # --level phrase: one query row, the mean of the words' rows; --segment and --max_rows go through to metrics.search
    res2 = tmp_path / "phrase"
    assert drivers.cmd_search(["--path", str(src), "--query", str(query), "--level", "phrase", "--topk", "12", "--segment", "16", "--max_rows", "48",
                               "--res_dir", str(res2)], engine=eng) == 0
    z = np.load(res2 / "search_hello_there.npz")
    assert list(z["words"]) == ["hello there now"] and z["clip"].shape == (1, 12)
    want = brute((q * 2.0).mean(axis=0, keepdims=True), clips, 12, segment=16)
    assert np.array_equal(z["clip"], want[0]) and np.array_equal(z["frame"], want[1]) and np.allclose(z["score"], want[2], atol=1e-6)
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith("search: \"")]) == 1
    # --normalize 0: the rows as stored
    res3 = tmp_path / "raw"
    assert drivers.cmd_search(["--path", str(src), "--query", str(query), "--topk", "4", "--normalize", "0", "--res_dir", str(res3)], engine=eng) == 0
    want = brute(q * 2.0, clips, 4, normalize=False)
    z = np.load(res3 / "search_hello_there.npz")
    assert np.array_equal(z["clip"], want[0]) and np.allclose(z["score"], want[2], atol=1e-5)
    with pytest.raises(SystemExit):
        drivers.cmd_search(["--path", str(src), "--query", str(query), "--topk", "129"], engine=eng)
    with pytest.raises(SystemExit):
        drivers.cmd_search(["--path", str(res), "--query", str(query)], engine=eng)              # no .pkl there
    with pytest.raises(SystemExit):
        drivers.cmd_search(["--path", str(src), "--query", str(src / (names[0] + ".pkl"))], engine=eng)      # a query file without content_emb


def test_engine_refuses_bad_arguments_before_it_needs_a_device():
    assert len(_SIGS["jg_sim_topk_grouped"]) == 13 and "jg_sim_topk_grouped" in EXPORTS
    assert len(_SIGS["jg_group_of_rows"]) == 8 and "jg_group_of_rows" in EXPORTS
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    q, g = torch.zeros(20, 512), torch.zeros(30, 512)
    off = [0, 10, 10, 30]
    ok_i, ok_s = torch.zeros(20, 5, dtype=torch.int32), torch.zeros(20, 5)
    bad = [dict(queries=torch.zeros(512), gallery=g, g_offsets=off, k=5),                          # not (rows, D)
           dict(queries=q, gallery=torch.zeros(30, 256), g_offsets=off, k=5),                      # different D
           dict(queries=torch.zeros(20, 96), gallery=torch.zeros(30, 96), g_offsets=off, k=5),     # D % 64
           dict(queries=torch.zeros(20, 0), gallery=torch.zeros(30, 0), g_offsets=off, k=5),       # D = 0
           dict(queries=q, gallery=g, g_offsets=off, k=0), dict(queries=q, gallery=g, g_offsets=off, k=129),
           dict(queries=q, gallery=g, g_offsets=off, k=5, gallery_offset=-1),
           dict(queries=q, gallery=g, g_offsets=off, k=5, gallery_offset=2 ** 31 - 30),            # gallery_offset + rows > INT32_MAX
           dict(queries=q, gallery=g, g_offsets=[], k=5),                                          # no entry at all
           dict(queries=q, gallery=g, g_offsets=[[0, 30]], k=5),                                   # not 1-d
           dict(queries=q, gallery=g, g_offsets=[0.0, 30.0], k=5),                                 # not integers
           dict(queries=q, gallery=g, g_offsets=[0, 20, 10, 30], k=5),                             # decreasing
           dict(queries=q, gallery=g, g_offsets=[-1, 30], k=5),
           dict(queries=q, gallery=g, g_offsets=[0, 31], k=5),                                     # beyond the gallery
           dict(queries=q, gallery=g, g_offsets=torch.zeros(4), k=5),                              # a float tensor
           dict(queries=q, gallery=g, g_offsets=off, k=5, merge_into=ok_i),                        # not a pair
           dict(queries=q, gallery=g, g_offsets=off, k=5, merge_into=(ok_i, ok_s[:, :4])),         # shapes
           dict(queries=q, gallery=g, g_offsets=off, k=5, merge_into=(ok_i.to(torch.int64), ok_s)),        # dtypes
           dict(queries=q, gallery=g, g_offsets=off, k=5, merge_into=(ok_s, ok_i))]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.sim_topk_grouped(**kw)
    for kw in (dict(idx=ok_s, g_offsets=off), dict(idx=ok_i.numpy(), g_offsets=off), dict(idx=ok_i, g_offsets=[0, 20, 10]),
               dict(idx=ok_i, g_offsets=[]), dict(idx=ok_i, g_offsets=off, gallery_offset=-1)):
        with pytest.raises(ValueError):
            eng.group_of_rows(**kw)
