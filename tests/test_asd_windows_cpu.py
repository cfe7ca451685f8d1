"""The host side of the ASD-over-time feature without a GPU: metrics.asd_scores, metrics.asd_timeline and the asd driver reach the device
only through engine.asd_windows, so a stand-in engine that evaluates the entry's formula in numpy (windows_ref of the GPU test) drives them
here; plus the fixture synth.planted_scene, the argument checks Engine.asd_windows makes before it needs a device, and the built library's
export and kernel resources."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from jegal_amd import drivers, metrics as M, synth
from jegal_amd._lib import _SIGS, EXPORTS, Engine
from test_gpu_asd_windows import SHAPES, make_scene, windows_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class NumpyEngine:
    """asd_windows with Engine.asd_windows's contract, computed on the host in float32"""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def asd_windows(self, gesture, g_offsets, content, c_offsets, trk, s_offsets, win=0, hop=1, n_windows=None, word_start=None,
                    word_end=None, temp=0.07, want_cos=False):
        g, c = np.asarray(gesture, np.float32), np.asarray(content, np.float32)
        n = len(s_offsets) - 1
        tracks = [g[g_offsets[t]:g_offsets[t + 1]] for t in range(len(g_offsets) - 1)]
        self.calls.append(dict(n=n, tracks=len(tracks), win=win, hop=hop))
        probs, preds, coss = [], [], []
        for i in range(n):
            cand = [int(t) for t in trk[s_offsets[i]:s_offsets[i + 1]]]
            rows = slice(c_offsets[i], c_offsets[i + 1])
            nw = 1 if not win else int(n_windows[i]) if n_windows is not None else -(-max(len(tracks[t]) for t in cand) // hop)
            sc = dict(content=c[rows], ws=word_start[rows] if win else None, we=word_end[rows] if win else None, trk=cand, n_win=nw)
            p, cs, d = windows_ref(tracks, sc, win, hop, np.float32, temp)
            probs.append(p)
            coss.append(cs)
            preds.append(d)
        w_off, p_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        w_off[1:], p_off[1:] = np.cumsum([len(d) for d in preds]), np.cumsum([p.size for p in probs])
        flat = lambda xs: torch.from_numpy(np.concatenate([x.reshape(-1) for x in xs]).astype(np.float32))
        return flat(probs), p_off, torch.from_numpy(np.concatenate(preds)), w_off, flat(coss) if want_cos else None


# ------------------------------------------------------------------------------------------------ the fixture
def test_planted_scene_is_deterministic_and_has_the_promised_shape():
    c, b, tr, sp = synth.planted_scene(4, 5, 40, 7)
    c2, b2, tr2, sp2 = synth.planted_scene(4, 5, 40, 7)
    assert np.array_equal(c, c2) and b == b2 and sp == sp2 and all(np.array_equal(x, y) for x, y in zip(tr, tr2))
    assert not np.array_equal(c, synth.planted_scene(5, 5, 40, 7)[0])
    assert c.shape == (7, 512) and c.dtype == np.float32 and np.allclose(np.linalg.norm(c, axis=1), 1, atol=1e-6)
    assert [t.shape for t in tr] == [(33, 512)] + [(40, 512)] * 4 and all(t.dtype == np.float32 for t in tr)
    assert b == [[f"w{j}", 5 * j, 5 * j + 3] for j in range(7)]            # a silent gap frame behind every word
    assert sp == [0, 0, 0, 1, 1, 1, 2]
    for j, (_, s, e) in enumerate(b):                                        # the speaker's frames carry the word, the gap frame does not
        assert all(float(tr[sp[j]][t] @ c[j]) > 0.8 for t in range(s, e + 1))
        assert abs(float(tr[sp[j]][e + 1] @ c[j])) < 0.3
    c, b, tr, _ = synth.planted_scene(4, 2, 30, 3, d=64, span=8, turns=1)
    assert c.shape == (3, 64) and [t.shape for t in tr] == [(23, 64), (30, 64)] and b[2] == ["w2", 16, 22]


@pytest.mark.parametrize("P,T,W,win,hop", SHAPES)
def test_planted_scene_windows_are_decidable(P, T, W, win, hop):
    """what the GPU test relies on: on these shapes every decided window is decidable (best prob more than 1e-3 relative above the
    runner-up, in float64), the fp32 evaluation's prob error lies between 1e-10 and 6e-7, and 2..17 windows per scene are undecided"""
    for seed in (1, 2, 3):
        c, b, tr, _ = synth.planted_scene(seed, P, T, W)
        sc = make_scene(c, b, range(P), -(-T // hop) + 1)
        p64, _, d64 = windows_ref(tr, sc, win, hop)
        p32, _, d32 = windows_ref(tr, sc, win, hop, np.float32)
        ok = d64 >= 0
        assert 2 <= int((~ok).sum()) <= 17 and d64[-1] == -1
        top = np.sort(p64[ok], axis=1)
        if P > 1:
            assert np.all(top[:, -1] - top[:, -2] > 1e-3 * top[:, -1])
        assert np.array_equal(d32, d64)
        assert 1e-10 <= np.abs(p32[ok] - p64[ok]).max() <= 6e-7


# ------------------------------------------------------------------------------------------------ metrics
def test_asd_scores_lays_out_one_clip_level_call():
    contents, positives, negatives = synth.planted_asd(9007, 12)
    cands = [[p] + list(ns) for p, ns in zip(positives, negatives)]
    eng = NumpyEngine()
    scores = M.asd_scores(contents, cands, engine=eng)
    assert eng.calls == [dict(n=12, tracks=sum(len(cs) for cs in cands), win=0, hop=1)]
    assert [len(p) for p, _ in scores] == [len(cs) for cs in cands] and sorted({len(cs) for cs in cands}) == [1, 3, 5, 6]
    for ct, cs, (prob, pred) in zip(contents, cands, scores):
        want, _, d = windows_ref(cs, dict(content=ct, ws=None, we=None, trk=range(len(cs)), n_win=1), 0, 1, np.float32)
        assert prob.dtype == np.float32 and np.array_equal(prob, want[0]) and pred == d[0] and isinstance(pred, int)
    assert any(pred != 0 for _, pred in scores)                              # (the fixture's hard negatives win somewhere)
    assert M.asd_scores([], [], engine=eng) == []
    with pytest.raises(ValueError):
        M.asd_scores(contents, cands[:3], engine=eng)


def test_asd_timeline_windows_offsets_and_a_single_scene():
    eng = NumpyEngine()
    made = [synth.planted_scene(s, P, T, W) for s, P, T, W in ((1, 4, 60, 10), (2, 2, 43, 6), (3, 3, 31, 4))]
    lines = M.asd_timeline([m[0] for m in made], [m[1] for m in made], [m[2] for m in made], win=9, hop=4, engine=eng)
    assert eng.calls == [dict(n=3, tracks=9, win=9, hop=4)]
    for (c, b, tr, _), t in zip(made, lines):
        n_win = -(-max(len(x) for x in tr) // 4)
        assert sorted(t) == ["pred", "prob", "start"]
        assert np.array_equal(t["start"], 4 * np.arange(n_win)) and t["start"].dtype == np.int32
        want, _, d = windows_ref(tr, make_scene(c, b, range(len(tr)), n_win), 9, 4, np.float32)
        assert t["prob"].shape == (n_win, len(tr)) and np.array_equal(t["prob"], want, equal_nan=True) and np.array_equal(t["pred"], d)
    c, b, tr, _ = made[1]
    one = M.asd_timeline(c, str(b), tr, win=9, hop=4, engine=eng)          # one scene; boundaries as the csv rows hold them
    assert np.array_equal(one["prob"], lines[1]["prob"], equal_nan=True) and np.array_equal(one["pred"], lines[1]["pred"])
    pairs = M.asd_timeline(c, [(s, e) for _, s, e in b], tr, win=9, hop=4, engine=eng)          # (start, end) pairs
    assert np.array_equal(pairs["prob"], one["prob"], equal_nan=True)
    default = M.asd_timeline(c, b, tr, engine=eng)
    assert eng.calls[-1] == dict(n=1, tracks=2, win=25, hop=5) and default["prob"].shape == (9, 2)
    assert M.asd_timeline([], [], [], engine=eng) == []
    with pytest.raises(ValueError):
        M.asd_timeline(c, b[:-1], tr, engine=eng)                            # fewer boundaries than content rows
    with pytest.raises(ValueError):
        M.asd_timeline(c, b, tr, win=0, engine=eng)


# ------------------------------------------------------------------------------------------------ driver
def write_dataset(tmp_path, n_neg_extra=0):
    """feature .pkl files and a csv in the form evaluate_asd reads: every query's candidates are its own clip and its neg_files that exist"""
    import pandas as pd
    src = tmp_path / "pkl"
    src.mkdir(exist_ok=True)
    made = [synth.planted_scene(40 + i, 3, 30 + 4 * i, 4 + i) for i in range(4)]
    clips = {}
    for i, (c, b, tr, _) in enumerate(made):
        for p, t in enumerate(tr):
            clips[f"vid{i}/{p:05d}"] = dict(gesture_emb=t, content_emb=c if p == 0 else c[:2],
                                             info=pd.Series({"filename": f"vid{i}/{p:05d}", "word_boundaries": str(b if p == 0 else b[:2])}))
    for k in range(n_neg_extra):
        clips[f"more/{k:05d}"] = dict(gesture_emb=made[0][2][1][:9], content_emb=made[0][0][:1], info={"fname": "x", "word_boundaries": made[0][1][:1]})
    for name, ft in clips.items():
        with open(src / (name.replace("/", "__") + ".pkl"), "wb") as f:
            pickle.dump(ft, f)
    rows = [dict(filename=f"vid{i}/00000", neg_files=str([f"vid{i}/00001", "gone/00000", f"vid{i}/00002", f"vid{(i + 1) % 4}/00000"]))
            for i in range(4)]
    rows.insert(2, dict(filename="gone/00001", neg_files=str(["vid0/00001"])))              # a query without a .pkl is skipped
    if n_neg_extra:
        rows.append(dict(filename="vid0/00000", neg_files=str([f"more/{k:05d}" for k in range(n_neg_extra)])))
    pd.DataFrame(rows).to_csv(tmp_path / "avs_asd.csv", index=False)
    return src, made


def test_driver_writes_both_npz_schemas(tmp_path, capsys):
    src, made = write_dataset(tmp_path)
    res, eng = tmp_path / "res", NumpyEngine()
    assert "asd" in drivers.COMMANDS
    assert drivers.cmd_asd(["--path", str(src), "--file", str(tmp_path / "avs_asd.csv"), "--res_dir", str(res)], engine=eng) == 0
    assert eng.calls == [dict(n=4, tracks=12, win=0, hop=1)]                  # every clip on the device once, one call
    assert [p.name for p in res.iterdir()] == ["asd.npz"]
    z = np.load(res / "asd.npz")
    assert sorted(z.files) == ["cand_names", "cand_offsets", "names", "pred", "prob"]
    assert list(z["names"]) == [f"vid{i}__00000" for i in range(4)]
    assert list(z["cand_offsets"]) == [0, 4, 8, 12, 16] and z["prob"].dtype == np.float32 and z["pred"].dtype == np.int32
    assert list(z["cand_names"][4:8]) == ["vid1__00000", "vid1__00001", "vid1__00002", "vid2__00000"]       # the query first, missing files dropped
    for i, (c, _, tr, _) in enumerate(made):
        cands = tr + [made[(i + 1) % 4][2][0]]
        want, _, d = windows_ref(cands, dict(content=c, ws=None, we=None, trk=range(4), n_win=1), 0, 1, np.float32)
        assert np.array_equal(z["prob"][4 * i:4 * i + 4], want[0]) and z["pred"][i] == d[0]
    assert "ASD: 4 queries" in capsys.readouterr().out
    # --win: the clip-level file and every query's timeline
    res2 = tmp_path / "res2"
    assert drivers.cmd_asd(["--path", str(src), "--file", str(tmp_path / "avs_asd.csv"), "--res_dir", str(res2), "--win", "6", "--hop", "2"],
                           engine=eng) == 0
    assert eng.calls[-2:] == [dict(n=4, tracks=12, win=0, hop=1), dict(n=4, tracks=12, win=6, hop=2)]
    assert sorted(p.name for p in res2.iterdir()) == ["asd.npz"] + [f"vid{i}__00000.asd.npz" for i in range(4)]
    assert np.array_equal(np.load(res2 / "asd.npz")["prob"], z["prob"])
    for i, (c, b, tr, _) in enumerate(made):
        t = np.load(res2 / f"vid{i}__00000.asd.npz")
        cands = tr + [made[(i + 1) % 4][2][0]]
        n_win = -(-max(len(x) for x in cands) // 2)
        assert sorted(t.files) == ["candidates", "pred", "prob", "start"]
        assert list(t["candidates"]) == list(z["cand_names"][4 * i:4 * i + 4])
        assert np.array_equal(t["start"], 2 * np.arange(n_win)) and t["start"].dtype == np.int32 and t["pred"].dtype == np.int32
        want, _, d = windows_ref(cands, make_scene(c, b, range(4), n_win), 6, 2, np.float32)
        assert t["prob"].dtype == np.float32 and np.array_equal(t["prob"], want, equal_nan=True) and np.array_equal(t["pred"], d)
    with pytest.raises(SystemExit):
        drivers.cmd_asd(["--path", str(src), "--file", str(tmp_path / "avs_asd.csv"), "--win", "0"], engine=eng)
    with pytest.raises(SystemExit) as help_exit:
        drivers.cmd_asd(["--help"])
    assert help_exit.value.code == 0 and "sharding over ranks is not built" in capsys.readouterr().out


def test_driver_refuses_a_query_with_more_than_64_candidates(tmp_path):
    src, _ = write_dataset(tmp_path, n_neg_extra=64)
    eng = NumpyEngine()
    with pytest.raises(SystemExit) as refusal:
        drivers.cmd_asd(["--path", str(src), "--file", str(tmp_path / "avs_asd.csv"), "--res_dir", str(tmp_path / "res")], engine=eng)
    assert "65 candidates" in str(refusal.value) and "vid0/00000" in str(refusal.value) and eng.calls == []
    src, _ = write_dataset(tmp_path, n_neg_extra=63)                          # 64 candidates are taken
    assert drivers.cmd_asd(["--path", str(src), "--file", str(tmp_path / "avs_asd.csv"), "--res_dir", str(tmp_path / "res")], engine=eng) == 0
    assert list(np.load(tmp_path / "res" / "asd.npz")["cand_offsets"]) == [0, 4, 8, 12, 16, 80]


# ------------------------------------------------------------------------------------------------ the engine's own checks, the library
def test_engine_asd_windows_refuses_bad_arguments_before_it_needs_a_device():
    assert len(_SIGS["jg_asd_windows"]) == 21 and "jg_asd_windows" in EXPORTS
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    g, c = torch.zeros(30, 512), torch.zeros(6, 512)
    good = dict(gesture=g, g_offsets=[0, 10, 30], content=c, c_offsets=[0, 2, 6], trk=[0, 1, 1], s_offsets=[0, 2, 3], win=5, hop=2,
                word_start=[0, 5, 0, 5, 10, 15], word_end=[3, 8, 3, 8, 13, 18])
    bad = [dict(c_offsets=[0, 6]),                                           # different scene counts
           dict(s_offsets=[0, 0, 3]), dict(trk=list(range(2)) * 40, s_offsets=[0, 65, 80], g_offsets=[0, 10, 30]),      # 0 and 65 candidates
           dict(c_offsets=[0, 0, 6]),                                        # a scene without words
           dict(trk=[0, 2, 1]), dict(trk=[0, -1, 1]),                        # a candidate that is no track
           dict(g_offsets=[0, 0, 30]),                                       # a candidate without frames
           dict(g_offsets=[0, 10, 40]), dict(c_offsets=[0, 2, 7]), dict(s_offsets=[0, 2, 4]),       # offsets beyond the rows
           dict(win=-1), dict(win=8193), dict(hop=0), dict(temp=0.0),
           dict(word_start=None), dict(word_end=[3, 8, 3]),                  # windows need one bound per word
           dict(n_windows=[3]), dict(n_windows=[0, 3]), dict(n_windows=[3, 8193]),
           dict(gesture=torch.zeros(30, 96), content=torch.zeros(6, 96)), dict(content=torch.zeros(6, 256)),
           dict(gesture=torch.zeros(30, 1088), content=torch.zeros(6, 1088))]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.asd_windows(**dict(good, **kw))
    with pytest.raises(ValueError):
        eng.asd_windows(torch.zeros(9000, 512), [0, 9000], c, [0, 6], [0], [0, 1])           # a track of more than 8192 frames
    with pytest.raises(ValueError):
        eng.asd_windows(g, [0, 30], torch.zeros(1025, 512), [0, 1025], [0], [0, 1])          # more than 1024 words


def test_library_exports_the_entry_and_the_kernel_needs_no_scratch():
    import __graft_entry__ as G
    G.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jegal_amd", "libjegal_hip.so"))
    assert hasattr(lib, "jg_asd_windows")
    assert "jg_asd_windows(" in open(os.path.join(ROOT, "include", "jegal_hip.h")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    mine = {k: v for k, v in kernel_resources().items() if "asd_windows_kernel" in k}
    assert len(mine) == 3                                                    # D <= 256, <= 512, <= 1024
    for name, r in mine.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds"] <= 16 * 1024, (name, r)
