"""The host side of the talk heat map without a GPU: what Engine.attn_talk refuses before it needs a device (the 128-candidate rule
restated on the host among it), metrics.talk_words, and metrics.talk_heatmap / spot_talk and the spot_talk driver, which reach the device
only through engine.attn_talk, driven by a stand-in engine that evaluates the definition on the host (tests/attn_talk_cases.py)."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import attn_talk_cases as C
from jegal_amd import drivers, metrics as M
from jegal_amd._lib import _SIGS, Engine
from jegal_amd._metric_entries import LIMITS, MetricEntries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostEngine:
    """attn_talk with Engine.attn_talk's contract, computed by the fp32 twin on the host"""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def attn_talk(self, gesture, content, g_offsets, c_offsets, word_start, word_end, reach=110, temp=0.07, normalize=True, want_band=True,
                  want_best=True, want_frames=True):
        self.calls.append(dict(n=len(g_offsets) - 1, reach=reach, normalize=normalize, want_band=want_band))
        g, c = np.asarray(gesture, np.float32), np.asarray(content, np.float32)
        s, e = np.asarray(word_start, np.int64), np.asarray(word_end, np.int64)
        pitch = 2 * reach + int((e - s).max()) + 1
        band = np.full((len(c), pitch), np.nan, np.float32)
        bf, bs = np.full(len(c), -1, np.int32), np.full(len(c), np.nan, np.float32)
        fw, fp = np.full(len(g), -1, np.int32), np.full(len(g), np.nan, np.float32)
        for i in range(len(g_offsets) - 1):
            f, w = slice(g_offsets[i], g_offsets[i + 1]), slice(c_offsets[i], c_offsets[i + 1])
            Pm = C.talk32(g[f], c[w], s[w], e[w], reach, normalize, temp)
            band[w] = C.band_of(Pm, s[w], reach, pitch)
            bf[w], bs[w] = C.word_best(Pm)
            fw[f], fp[f] = C.frame_best(Pm)
        t = torch.from_numpy
        return (t(band) if want_band else None), t(bf), t(bs), t(fw), t(fp)


GOOD = dict(gesture=torch.zeros(300, 64), content=torch.zeros(6, 64), g_offsets=[0, 100, 300], c_offsets=[0, 2, 6],
            word_start=[0, 5, 0, 5, 10, 15], word_end=[3, 8, 3, 8, 13, 18])


def outcome(kw):
    eng = Engine.__new__(Engine)                     # no handle, no device: every check comes before either is touched
    try:
        eng.attn_talk(**kw)
    except ValueError as e:
        return "refused: " + str(e)
    except AttributeError:
        return "passed"
    return "returned"


def test_wrapper_refuses_before_it_needs_a_device():
    assert len(_SIGS["jg_attn_talk"]) == 21
    assert (LIMITS["TALK_MAX_T"], LIMITS["TALK_MAX_REACH"], LIMITS["TALK_MAX_BLOCK_W"]) == (2 ** 20, 1024, 128)
    assert outcome(GOOD) == "passed"
    bad = [dict(reach=-1), dict(reach=1025), dict(temp=0.0), dict(want_band=False, want_best=False, want_frames=False),
           dict(gesture=torch.zeros(300, 96), content=torch.zeros(6, 96)), dict(content=torch.zeros(6, 128)), dict(gesture=torch.zeros(300)),
           dict(g_offsets=[0, 300]), dict(g_offsets=[0, 100, 301]), dict(g_offsets=[-1, 100, 300]), dict(g_offsets=[0, 200, 100]),
           dict(c_offsets=[0, 6]), dict(c_offsets=[0, 2, 7]), dict(c_offsets=[0, 4, 2]),
           dict(word_start=[0, 5, 0, 5, 10]), dict(word_end=[3, 8, 3, 8, 13, 18, 20]), dict(word_end=[3, 8, 3, 8, 13, 2 ** 31]),
           dict(word_start=[0, 9, 0, 5, 10, 15]),                                   # start > end
           dict(word_start=[0, 5, 0, 5, 4, 15]), dict(word_end=[3, 8, 3, 14, 13, 18]),      # not in transcript order inside track 1
           dict(gesture=torch.zeros(2 ** 20 + 1, 64), g_offsets=[0, 2 ** 20 + 1], c_offsets=[0, 6], word_start=[0, 5, 6, 7, 10, 15],
                word_end=[3, 8, 9, 10, 13, 18])]
    wrong = [(kw, got) for kw in bad if not (got := outcome(dict(GOOD, **kw))).startswith("refused")]
    assert not wrong, wrong
    one = dict(word_start=[0, 5, 6, 7, 10, 15], word_end=[3, 8, 9, 10, 13, 18])      # in order as the words of ONE track
    ok = [dict(reach=0), dict(reach=1024), dict(g_offsets=[0, 0, 300]), dict(c_offsets=[0, 0, 6], **one), dict(word_start=[0, 5, -9, 5, 10, 15]),
          dict(word_start=[0, 5, 0, 5, 10, 500], word_end=[3, 8, 3, 8, 13, 600]),   # a word outside its track
          dict(word_start=[5, 5, 0, 0, 0, 0], word_end=[8, 8, 3, 3, 3, 3]),         # equal bounds; track 1 starts again below track 0's
          dict(gesture=torch.zeros(2 ** 20, 64), g_offsets=[0, 2 ** 20], c_offsets=[0, 6], **one), dict(want_band=False)]
    wrong = [(kw, got) for kw in ok if (got := outcome(dict(GOOD, **kw))) != "passed"]
    assert not wrong, wrong


def test_the_candidate_rule_on_the_host():
    # 129 one-frame words on 129 frames: at reach 200 the first block has 129 candidates, at reach 0 it has 128
    s = np.arange(129)
    kw = dict(gesture=torch.zeros(129, 64), content=torch.zeros(129, 64), g_offsets=[0, 129], c_offsets=[0, 129], word_start=s, word_end=s)
    got = outcome(dict(kw, reach=200))
    assert got.startswith("refused") and "lower reach" in got and "129 words" in got
    assert outcome(dict(kw, reach=0)) == "passed"
    assert outcome(dict(kw, reach=200, content=torch.zeros(128, 64), c_offsets=[0, 128], word_start=s[:128], word_end=s[:128])) == "passed"
    # the searches count what the definition gives, block by block
    for seed, T, W, span, gap, reach, _ in C.ACCURACY_INPUTS:
        _, _, st, en = C.planted_talk(seed, T, W, span, gap, 64)
        assert np.array_equal(MetricEntries.talk_block_candidates(T, st, en, reach), C.block_candidates(T, st, en, reach))
    rng = np.random.default_rng(0)
    for T in (1, 127, 128, 129, 400):
        st = np.sort(rng.integers(-50, T + 50, 60))
        en = np.maximum.accumulate(st + rng.integers(0, 40, 60))
        for reach in (0, 7, 300):
            assert np.array_equal(MetricEntries.talk_block_candidates(T, st, en, reach), C.block_candidates(T, st, en, reach)), (T, reach)
    assert MetricEntries.talk_block_candidates(0, [0], [3], 5).size == 0


def utterance(rng, words, schema):
    c = rng.standard_normal((len(words), 512)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    if schema == "series":
        import pandas as pd
        info = pd.Series({"filename": "v/0", "word_boundaries": str([list(w) for w in words])})
    else:
        info = {"fname": "u", "word_boundaries": [list(w) for w in words], "text": "t"}
    return {"gesture_emb": None, "content_emb": c, "info": info}


def test_talk_words():
    rng = np.random.default_rng(1)
    u0 = utterance(rng, [("a", 0, 3), ("b", 4, 9)], "dict")
    u1 = utterance(rng, [("c", 2, 5), ("d", 6, 6), ("e", 7, 12)], "series")
    content, bounds = M.talk_words([u1, u0], [100, 10])                      # in the order of the starts, whatever the order given
    assert bounds == [["a", 10, 13], ["b", 14, 19], ["c", 102, 105], ["d", 106, 106], ["e", 107, 112]]
    assert content.dtype == np.float32 and np.array_equal(content, np.concatenate([u0["content_emb"], u1["content_emb"]]))
    assert M.talk_words([], [])[1] == [] and M.talk_words([], [])[0].shape == (0, 512)
    M.talk_words([u0, u1], [10, 18])                                         # overlapping in order: u1's first word starts at 20 > 14
    with pytest.raises(ValueError, match="overlap out of order"):
        M.talk_words([u0, u1], [10, 11])                                     # u1's first word would start at 13, before "b" at 14
    with pytest.raises(ValueError):
        M.talk_words([u0], [0, 5])
    with pytest.raises(ValueError, match="word boundaries"):
        M.talk_words([dict(u0, content_emb=u0["content_emb"][:1])], [0])
    with pytest.raises(ValueError, match="content_emb"):
        M.talk_words([dict(u0, content_emb=None)], [0])


def test_talk_heatmap_and_spot_talk_make_one_call():
    g0, c0, s0, e0 = C.planted_talk(2, 90, 12, 5, 2, 64)
    g1, c1, s1, e1 = C.planted_talk(3, 40, 3, 4, 1, 64)
    wb0, wb1 = [[f"w{j}", int(a), int(b)] for j, (a, b) in enumerate(zip(s0, e0))], str([(int(a), int(b)) for a, b in zip(s1, e1)])
    eng = HostEngine()
    res = M.talk_heatmap([g0, g1], [c0, c1], [wb0, wb1], reach=6, engine=eng)
    assert eng.calls == [dict(n=2, reach=6, normalize=True, want_band=True)]
    for r, (g, c, s, e) in zip(res, ((g0, c0, s0, e0), (g1, c1, s1, e1))):
        Pm = C.talk32(g, c, s, e, 6, True)
        assert sorted(r) == ["band", "best_frame", "best_score", "first_frame", "frame_prob", "frame_word"]
        assert r["band"].shape == (len(c), 17) and np.array_equal(r["first_frame"], s - 6) and r["first_frame"].dtype == np.int32
        assert np.array_equal(r["band"], C.band_of(Pm, s, 6, 17), equal_nan=True)
        assert np.array_equal(r["best_frame"], C.word_best(Pm)[0]) and np.array_equal(r["frame_word"], C.frame_best(Pm)[0])
        assert r["frame_word"].shape == (len(g),) and r["best_score"].shape == (len(c),)
    one = M.spot_talk(g1, c1, wb1, reach=6, normalize=False, engine=eng)     # one track in, one dict out
    assert eng.calls[-1] == dict(n=1, reach=6, normalize=False, want_band=False)
    assert sorted(one) == ["best_frame", "best_score", "frame_prob", "frame_word"]
    assert M.talk_heatmap([], [], [], engine=HostEngine()) == []
    with pytest.raises(ValueError, match="word boundaries"):
        M.talk_heatmap(g1, c1, wb0, engine=eng)


def test_driver_on_both_info_schemas(tmp_path):
    import pandas as pd
    g, c, s, e = C.planted_talk(6, 260, 30, 6, 2)
    words = [(f"w{j}", int(a), int(b)) for j, (a, b) in enumerate(zip(s, e))]
    src, res = tmp_path / "pkl", tmp_path / "res"
    src.mkdir()
    with open(src / "vid__trk.pkl", "wb") as f:                              # what embed_tracks writes
        pickle.dump({"gesture_emb": g, "content_emb": None, "info": {"fname": "vid/trk", "win": 120, "ctx": 50}}, f)
    # --content: one feature .pkl on the track's axis, in either info schema
    for schema in ("dict", "series"):
        info = {"fname": "x", "word_boundaries": [list(w) for w in words], "text": "t"} if schema == "dict" else \
            pd.Series({"filename": "v/0", "word_boundaries": str([list(w) for w in words])})
        with open(src / f"content_{schema}.pkl", "wb") as f:
            pickle.dump({"gesture_emb": None, "content_emb": c, "info": info}, f)
        eng = HostEngine()
        assert drivers.cmd_spot_talk(["--gesture", str(src / "vid__trk.pkl"), "--content", str(src / f"content_{schema}.pkl"),
                                      "--res_dir", str(res / schema)], engine=eng) == 0
        assert eng.calls == [dict(n=1, reach=110, normalize=False, want_band=True)]          # the defaults: one call
        z = np.load(res / schema / "vid__trk.talk.npz")
        assert sorted(z.files) == sorted(["words", "word_start", "word_end", "first_frame", "band", "best_frame", "best_score", "frame_word",
                                          "frame_prob"])
        Pm = C.talk32(g, c, s, e, 110, False)
        assert list(z["words"]) == [w[0] for w in words] and np.array_equal(z["word_start"], s) and np.array_equal(z["word_end"], e)
        assert z["band"].dtype == np.float32 and z["band"].shape == (30, 226) and np.array_equal(z["first_frame"], s - 110)
        assert np.array_equal(z["band"], C.band_of(Pm, s, 110, 226), equal_nan=True)
        assert z["best_frame"].dtype == np.int32 and np.array_equal(z["best_frame"], C.word_best(Pm)[0])
        assert z["frame_word"].shape == (260,) and np.array_equal(z["frame_word"], C.frame_best(Pm)[0])
    # --utterances: utterance-level files with their first frames; the same talk cut in three, listed out of order
    cuts = [(0, 10, 0), (10, 22, int(s[10])), (22, 30, int(s[22]) - 3)]
    rows = []
    for k, (a, b, first) in enumerate(cuts):
        wb = [[w[0], w[1] - first, w[2] - first] for w in words[a:b]]
        info = {"fname": f"u{k}", "word_boundaries": wb, "text": "t"} if k != 1 else pd.Series({"filename": f"talk/u{k}", "word_boundaries": str(wb)})
        with open(src / f"talk__u{k}.pkl", "wb") as f:
            pickle.dump({"gesture_emb": None, "content_emb": c[a:b], "info": info}, f)
        rows.append({"filename": f"talk/u{k}", "start_frame": first})
    pd.DataFrame([rows[2], rows[0], rows[1]]).to_csv(tmp_path / "list.csv", index=False)
    eng = HostEngine()
    assert drivers.cmd_spot_talk(["--gesture", str(src / "vid__trk.pkl"), "--utterances", str(tmp_path / "list.csv"), "--path", str(src),
                                  "--reach", "20", "--normalize", "1", "--band", "0", "--res_dir", str(res)], engine=eng) == 0
    assert eng.calls == [dict(n=1, reach=20, normalize=True, want_band=False)]
    z = np.load(res / "vid__trk.talk.npz")
    assert "band" not in z.files and "first_frame" not in z.files
    Pm = C.talk32(g, c, s, e, 20, True)
    assert list(z["words"]) == [w[0] for w in words] and np.array_equal(z["word_start"], s)
    assert np.array_equal(z["best_frame"], C.word_best(Pm)[0]) and np.array_equal(z["best_score"], C.word_best(Pm)[1].astype(np.float32), equal_nan=True)
    assert "spot_talk" in drivers.COMMANDS
    for argv in (["--gesture", str(src / "vid__trk.pkl")],                                                   # no words at all
                 ["--gesture", str(src / "vid__trk.pkl"), "--utterances", str(tmp_path / "list.csv")],        # a list without --path
                 ["--gesture", str(src / "vid__trk.pkl"), "--content", str(src / "vid__trk.pkl")]):           # a .pkl without content_emb
        with pytest.raises(SystemExit):
            drivers.cmd_spot_talk(argv + ["--res_dir", str(res)], engine=eng)
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        drivers.cmd_spot_talk(["--help"])
    assert "not a measured optimum" in " ".join(buf.getvalue().split())                                      # the help says what reach = 110 is


def test_library_exports_the_entry_and_its_kernels_do_not_spill():
    import __graft_entry__ as G
    G.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jegal_amd", "libjegal_hip.so"))
    assert hasattr(lib, "jg_attn_talk")
    assert "jg_attn_talk(" in open(os.path.join(ROOT, "include", "jegal_hip.h")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    mine = {k: v for k, v in res.items() if "attn_talk" in k}
    assert len(mine) == 3 and sum("attn_talk_kernel" in k for k in mine) == 1
    clips = {k: v for k, v in res.items() if "attn_matrix_kernel<" in k}        # the clip form shares the talk kernel's parts
    assert len(clips) == 2
    for name, r in {**mine, **clips}.items():
        assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
    talk = next(v for k, v in mine.items() if "attn_talk_kernel" in k)
    clip = next(v for k, v in res.items() if "attn_matrix_kernel<false>" in k)
    assert talk["vgpr"] <= 256 and talk["lds"] <= clip["lds"]               # the parts of the in-register form, with 128 candidates for 1024 words
    src = open(os.path.join(ROOT, "jegal_amd", "csrc", "spotting.hip")).read()
    assert 'record_kernel("attn_talk_' in src
