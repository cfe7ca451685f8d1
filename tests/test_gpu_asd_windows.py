"""jg_asd_windows through the C ABI (run with -m gpu): per scene and time window the probability that each candidate track gestures to the
utterance, against a float64 evaluation of the entry's formula (windows_ref below: own code, numpy) and the same evaluation in float32.

Error rule, for prob and for cosv separately: err(kernel) <= max(4 x err(fp32 evaluation), 8 x 2^-23) in max-abs, both errors against
float64 over the decided windows of one input.  The factor 4 is the rule of tests/test_gpu_attn_matrix.py (another summation order plus the
device expf); the floor is 8 ulp at 1.0: a saturated softmax leaves the fp32 evaluation's own error near 1e-10.
Arg-max rule: a window is decidable if, in float64, its best prob beats the runner-up by more than 1e-3 relative; a decidable window must
match the float64 arg-max exactly, any other must pick a candidate within 1e-3 relative of the best; at least 95 % of the decided windows
of every input are decidable (asserted)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from jegal_amd import synth

pytestmark = pytest.mark.gpu
TEMP = 0.07
WB = 16                    # ASDW_WB of jegal_amd/csrc/asd.hip: windows per workgroup
NAN_BITS = 0x7FC0BEEF      # a quiet NaN with a payload, as int32
FLOOR = 8 * 2.0 ** -23
PTR = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
#: P, T, W, win, hop of synth.planted_scene: the shapes on which tests/test_asd_windows_cpu.py shows every decided window to be decidable
SHAPES = [(4, 60, 10, 25, 5), (4, 60, 10, 9, 1), (6, 150, 30, 25, 1), (2, 40, 6, 1, 1), (64, 33, 5, 12, 7), (3, 70, 10, 25, 25)]


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ the reference
def windows_ref(tracks, scene, win, hop, dt=np.float64, temp=TEMP):
    """The entry's formula for one scene = dict(content (W,D), ws, we (W,), trk [P] indices into tracks, n_win) -> (prob (n_win,P), cosv
    (n_win,P), pred (n_win,)), every step in `dt`.  Undecided windows: NaN rows and pred -1; absent candidates: prob 0, cosv NaN."""
    trk, n_win = list(scene["trk"]), int(scene["n_win"])
    P = len(trk)
    prob, cosv, pred = np.full((n_win, P), np.nan, dt), np.full((n_win, P), np.nan, dt), np.full(n_win, -1, np.int32)
    c, ws, we = np.asarray(scene["content"], dt), np.asarray(scene["ws"]), np.asarray(scene["we"])
    for j in range(n_win):
        lo, hi = (j * hop, j * hop + win - 1) if win else (0, 1 << 30)
        sel = (we >= lo) & (ws <= hi) if win else np.ones(c.shape[0], bool)
        if not sel.any():
            continue
        q = c[sel].mean(axis=0, dtype=dt)
        qn = np.sqrt((q * q).sum(dtype=dt))
        cs = np.full(P, np.nan, dt)
        for p, t in enumerate(trk):
            rows = np.asarray(tracks[t][lo:hi + 1], dt)
            if rows.shape[0]:
                g = rows.mean(axis=0, dtype=dt)
                cs[p] = (q * g).sum(dtype=dt) / max(qn * np.sqrt((g * g).sum(dtype=dt)), dt(1e-8))
        present = ~np.isnan(cs)
        if not present.any():
            continue
        x = cs[present] / dt(temp)
        e = np.exp(x - x.max())
        prob[j] = 0
        prob[j, present] = e / e.sum(dtype=dt)
        cosv[j] = cs
        pred[j] = int(np.argmax(np.where(present, prob[j], -1)))
    return prob, cosv, pred


def undecided_ref(scene):
    n, P = int(scene["n_win"]), len(scene["trk"])
    return np.full((n, P), np.nan), np.full((n, P), np.nan), np.full(n, -1, np.int32)


def make_scene(content, bounds, trk, n_win):
    return dict(content=np.asarray(content, np.float32), ws=np.asarray([b[-2] for b in bounds], np.int32).reshape(-1),
                we=np.asarray([b[-1] for b in bounds], np.int32).reshape(-1), trk=list(trk), n_win=int(n_win))


def planted(seeds, P, T, W, hop, extra=1, tracks=None, **kw):
    """planted_scene per seed as scenes of one batch, ceil(T / hop) + extra windows each -> (tracks, scenes, speakers)"""
    tracks = [] if tracks is None else tracks
    scenes, speakers = [], []
    for seed in seeds:
        c, b, tr, sp = synth.planted_scene(seed, P, T, W, **kw)
        scenes.append(make_scene(c, b, range(len(tracks), len(tracks) + P), -(-T // hop) + extra))
        tracks += tr
        speakers.append(sp)
    return tracks, scenes, speakers


# ------------------------------------------------------------------------------------------------ the C entry
def call(eng, tracks, scenes, win, hop, gap=0, max_windows=None, want_cos=True, null_bounds=False, expect=0):
    """One jg_asd_windows call.  prob / cosv are pre-filled with a NaN pattern and laid out with `gap` unused elements behind every scene's
    block and a guard of 64 at the end; pred is pre-filled with -7 and has a guard of 8; null_bounds: word_start = word_end = NULL.  -> dict(prob, cosv, pred: per scene; raw buffers)"""
    D = tracks[0].shape[1]
    g = torch.from_numpy(np.ascontiguousarray(np.concatenate(tracks), np.float32)).cuda()
    goff = np.concatenate([[0], np.cumsum([t.shape[0] for t in tracks])])
    rows = [s["content"].reshape(-1, D) for s in scenes]
    c = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows + [np.zeros((1, D), np.float32)]), np.float32)).cuda()
    coff = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])])
    ws = torch.from_numpy(np.concatenate([s["ws"] for s in scenes] + [np.zeros(1, np.int32)]).astype(np.int32)).cuda()
    we = torch.from_numpy(np.concatenate([s["we"] for s in scenes] + [np.zeros(1, np.int32)]).astype(np.int32)).cuda()
    trk = torch.from_numpy(np.asarray([t for s in scenes for t in s["trk"]] + [0], np.int32)).cuda()
    P = np.array([len(s["trk"]) for s in scenes], np.int64)
    NW = np.array([s["n_win"] for s in scenes], np.int64)
    soff, woff = np.concatenate([[0], np.cumsum(P)]), np.concatenate([[0], np.cumsum(NW)])
    poff = np.concatenate([[0], np.cumsum(NW * P + gap)])
    prob = torch.full((int(poff[-1]) + 64,), NAN_BITS, dtype=torch.int32, device="cuda")
    cosv = torch.full((int(poff[-1]) + 64,), NAN_BITS, dtype=torch.int32, device="cuda") if want_cos else None
    pred = torch.full((int(woff[-1]) + 8,), -7, dtype=torch.int32, device="cuda")
    i32 = lambda v: torch.as_tensor(np.asarray(v, np.int32), device="cuda")
    go, co, so, wo = i32(goff), i32(coff), i32(soff), i32(woff)
    po = torch.as_tensor(poff[:-1].astype(np.int64), device="cuda")
    if null_bounds:
        ws = we = None
    eng._bind_stream()
    rc = eng.lib.jg_asd_windows(eng.h, PTR(g), PTR(go), len(tracks), PTR(c), PTR(co), PTR(ws), PTR(we), PTR(trk), PTR(so), len(scenes), D,
                                win, hop, PTR(wo), PTR(po), int(max_windows or NW.max()), TEMP, PTR(prob), PTR(cosv), PTR(pred))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    spans = [(int(poff[i]), int(poff[i] + NW[i] * P[i])) for i in range(len(scenes))]
    out = {"spans": spans, "raw_prob": prob.cpu().numpy(), "raw_pred": pred.cpu().numpy(), "n_pred": int(woff[-1])}
    cut = lambda raw: [raw[s:e].view(np.float32).reshape(NW[i], P[i]) for i, (s, e) in enumerate(spans)]
    out["prob"] = cut(out["raw_prob"])
    if want_cos:
        out["raw_cosv"] = cosv.cpu().numpy()
        out["cosv"] = cut(out["raw_cosv"])
    out["pred"] = [out["raw_pred"][woff[i]:woff[i + 1]] for i in range(len(scenes))]
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check(name, out, refs64, refs32, min_share=0.95):
    """structure (undecided windows, absent candidates) exactly, then the error rule and the arg-max rule over the decided windows"""
    err = {"prob": [0.0, 0.0], "cosv": [0.0, 0.0]}
    n = dec = 0
    for i, ((p64, c64, d64), (p32, c32, _)) in enumerate(zip(refs64, refs32)):
        kp, kc, kd = out["prob"][i], out["cosv"][i], out["pred"][i]
        und = d64 < 0
        assert np.array_equal(kd < 0, und), (name, i, "undecided windows")
        assert np.all(kd[und] == -1) and np.isnan(kp[und]).all() and np.isnan(kc[und]).all(), (name, i)
        ok = ~und
        if not ok.any():
            continue
        absent = np.isnan(c64[ok])
        assert np.array_equal(np.isnan(kc[ok]), absent) and np.all(kp[ok][absent] == 0) and not np.isnan(kp[ok]).any(), (name, i, "absent")
        assert np.allclose(kp[ok].sum(axis=1, dtype=np.float64), 1.0, atol=1e-5), (name, i)
        for key, k, r64, r32 in (("prob", kp, p64, p32), ("cosv", kc, c64, c32)):
            err[key][0] = max(err[key][0], float(np.nanmax(np.abs(k[ok].astype(np.float64) - r64[ok]))))
            err[key][1] = max(err[key][1], float(np.nanmax(np.abs(r32[ok].astype(np.float64) - r64[ok]))))
        for j in np.flatnonzero(ok):
            row = np.where(np.isnan(c64[j]), -1.0, p64[j])
            best = int(np.argmax(row))
            second = np.partition(row, -2)[-2] if row.size > 1 else -1.0
            decidable = row[best] - second > 1e-3 * row[best]
            n += 1
            dec += bool(decidable)
            assert 0 <= kd[j] < row.size, (name, i, j, kd[j])
            if decidable:
                assert kd[j] == best, (name, i, j, int(kd[j]), best)
            else:
                assert row[kd[j]] >= row[best] * (1 - 1e-3), (name, i, j, int(kd[j]), best)
    print(f"{name}: prob max-abs kernel {err['prob'][0]:.3e} fp32 evaluation {err['prob'][1]:.3e} | cosv kernel {err['cosv'][0]:.3e} "
          f"fp32 evaluation {err['cosv'][1]:.3e} | {dec}/{n} decidable windows")
    for key, (k, r) in err.items():
        assert k <= max(4 * r, FLOOR), (name, key, k, r)
    assert n > 0 and dec >= min_share * n, (name, dec, n)


def run_and_check(eng, name, tracks, scenes, win, hop, **kw):
    out = call(eng, tracks, scenes, win, hop, **kw)
    check(name, out, [windows_ref(tracks, s, win, hop) for s in scenes], [windows_ref(tracks, s, win, hop, np.float32) for s in scenes])
    return out


# ------------------------------------------------------------------------------------------------ 1. the planted shapes
@pytest.mark.parametrize("P,T,W,win,hop", SHAPES)
def test_planted_shapes_with_a_window_past_the_end(eng, P, T, W, win, hop):
    tracks, scenes, _ = planted((1, 2, 3), P, T, W, hop)
    out = run_and_check(eng, f"P{P} T{T} W{W} win{win} hop{hop}", tracks, scenes, win, hop)
    for pred, prob in zip(out["pred"], out["prob"]):
        assert pred[-1] == -1 and np.isnan(prob[-1]).all()             # the window past the end
        assert 2 <= int((pred < 0).sum()) <= 17                         # gap frames and the tail


# ------------------------------------------------------------------------------------------------ 2. every path boundary
@pytest.mark.parametrize("n_win", [WB - 1, WB, WB + 1])
def test_window_block_edges(eng, n_win):
    tracks, scenes, _ = planted((5, 6), 3, 60, 10, 3)
    for s in scenes:
        s["n_win"] = n_win
    scenes[1]["n_win"] = n_win + 2 * WB                                # a longer neighbour: the grid is sized by it
    run_and_check(eng, f"n_win {n_win}", tracks, scenes, 9, 3)


@pytest.mark.parametrize("D", [64, 320, 1024])
def test_feature_widths(eng, D):
    tracks, scenes, _ = planted((7, 8), 4, 45, 8, 4, d=D)
    run_and_check(eng, f"D {D}", tracks, scenes, 10, 4)


def test_one_candidate_has_probability_one(eng):
    tracks, scenes, _ = planted((9,), 1, 40, 6, 3, extra=0)
    out = run_and_check(eng, "P 1", tracks, scenes, 6, 3)
    decided = out["pred"][0] >= 0
    assert decided.any() and np.all(out["prob"][0][decided] == np.float32(1.0)) and np.all(out["pred"][0][decided] == 0)


def test_window_that_only_the_longer_tracks_reach(eng):
    tracks, scenes, _ = planted((10,), 3, 60, 12, 5, extra=0)          # track 0 has 53 frames, word 11 lies on frames 55..58
    out = run_and_check(eng, "short track", tracks, scenes, 5, 5)
    prob, cosv = out["prob"][0][11], out["cosv"][0][11]
    assert out["pred"][0][11] in (1, 2) and prob[0] == 0 and np.isnan(cosv[0]) and not np.isnan(cosv[1:]).any()
    assert abs(float(prob[1:].sum(dtype=np.float64)) - 1) < 1e-6
    assert not np.isnan(out["cosv"][0][10]).any()                      # frames 50..54: track 0 still has 50..52


def test_hop_larger_than_the_window(eng):
    tracks, scenes, _ = planted((11, 12), 4, 80, 16, 9)
    run_and_check(eng, "win 4 hop 9", tracks, scenes, 4, 9)


# ------------------------------------------------------------------------------------------------ 3. golden: the reference's evaluate_asd
def test_clip_level_equals_the_reference_evaluation(eng, golden_dir):
    from jegal_amd import metrics as M
    gold = np.load(os.path.join(golden_dir, "asd.npz"))
    n = int(gold["n"])
    contents, positives, negatives = synth.planted_asd(int(gold["seed"]), n)
    tracks, scenes = [], []
    for i in range(n):                                                 # three scene lists over the same frames: the first 2, 4, 6 candidates
        first = len(tracks)
        tracks += [positives[i]] + list(negatives[i])
        for k in (2, 4, 6):
            scenes.append(dict(content=contents[i], ws=np.zeros(len(contents[i]), np.int32), we=np.zeros(len(contents[i]), np.int32),
                               trk=list(range(first, first + min(k, 1 + len(negatives[i])))), n_win=1))
    out = run_and_check(eng, "planted_asd(9007, 48) x {2, 4, 6}", tracks, scenes, 0, 1)
    pred = np.array([int(p[0]) for p in out["pred"]]).reshape(n, 3)
    assert np.array_equal(pred, gold["preds"])
    q = M.video_level(eng, contents)
    cands = [M.video_level(eng, [positives[i]] + list(negatives[i])) for i in range(n)]
    old = eng.asd(q, torch.cat(cands), M._offsets(cands)).cpu().numpy()
    assert np.array_equal(pred, old)


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_same_frames_through_another_hop(eng):
    tracks, scenes, _ = planted((13,), 4, 60, 10, 5, extra=0)
    a = call(eng, tracks, scenes, 25, 5)
    scenes[0]["n_win"] = 6
    b = call(eng, tracks, scenes, 25, 10)
    assert a["pred"][0][2] >= 0
    for key in ("prob", "cosv"):                                       # frames 10..34 as (hop 5, j = 2) and as (hop 10, j = 1)
        assert np.array_equal(bits(a[key][0][2]), bits(b[key][0][1])), key
    assert a["pred"][0][2] == b["pred"][0][1]


def test_a_scene_alone_and_as_the_last_of_five(eng):
    tracks, scenes, _ = planted((14, 15, 16, 17, 18), 5, 70, 12, 2)
    five = call(eng, tracks, scenes, 25, 2)
    alone = call(eng, tracks, scenes[4:], 25, 2)
    again = call(eng, tracks, scenes[4:], 25, 2)
    for key in ("prob", "cosv", "pred"):
        assert np.array_equal(bits(five[key][4]), bits(alone[key][0])), key
        assert np.array_equal(bits(alone[key][0]), bits(again[key][0])), key         # two runs of one call
    assert (alone["pred"][0] >= 0).sum() > WB                          # (more than one workgroup per scene)


def test_clip_level_is_one_window_over_everything(eng):
    tracks, scenes, _ = planted((19, 20), 6, 150, 30, 150, extra=0)
    a = call(eng, tracks, scenes, 0, 1)
    b = call(eng, tracks, scenes, 8192, 8192)
    for i in range(2):
        assert a["pred"][i][0] >= 0 and a["pred"][i][0] == b["pred"][i][0]
        for key in ("prob", "cosv"):
            assert np.array_equal(bits(a[key][i]), bits(b[key][i])), key
    null = call(eng, tracks, scenes, 0, 1, null_bounds=True)
    assert np.array_equal(bits(null["prob"][1]), bits(a["prob"][1]))


def test_a_track_listed_twice_ties_to_the_first(eng):
    tracks, scenes, _ = planted((21,), 3, 60, 10, 5, extra=0)
    scenes[0]["trk"] = [1, 0, 2, 0]
    out = call(eng, tracks, scenes, 10, 5)
    prob, cosv, pred = out["prob"][0], out["cosv"][0], out["pred"][0]
    assert np.array_equal(bits(prob[:, 1]), bits(prob[:, 3])) and np.array_equal(bits(cosv[:, 1]), bits(cosv[:, 3]))
    won = [j for j in range(len(pred)) if pred[j] >= 0 and prob[j, 1] == np.nanmax(prob[j])]
    assert won and all(pred[j] == 1 for j in won)                      # track 0 speaks the first three words
    assert not (pred == 3).any()


# ------------------------------------------------------------------------------------------------ 5. nothing else is written
def test_nothing_outside_the_described_elements_is_written(eng):
    tracks, scenes, _ = planted((22, 23, 24), 5, 33, 5, 3)
    out = call(eng, tracks, scenes, 7, 3, gap=3)
    inside = np.zeros(out["raw_prob"].size, bool)
    for s, e in out["spans"]:
        inside[s:e] = True
    assert (~inside).sum() == 3 * 3 + 64
    for raw in (out["raw_prob"], out["raw_cosv"]):
        assert np.all(raw[~inside] == NAN_BITS) and not np.any(raw[inside] == NAN_BITS)
    assert np.all(out["raw_pred"][out["n_pred"]:] == -7) and not np.any(out["raw_pred"][:out["n_pred"]] == -7)
    check("gapped layout", out, [windows_ref(tracks, s, 7, 3) for s in scenes], [windows_ref(tracks, s, 7, 3, np.float32) for s in scenes])
    no_cos = call(eng, tracks, scenes, 7, 3, gap=3, want_cos=False)    # cosv == NULL
    assert np.array_equal(no_cos["raw_prob"], out["raw_prob"]) and np.array_equal(no_cos["raw_pred"], out["raw_pred"])


# ------------------------------------------------------------------------------------------------ 6. scenes outside the limits
@pytest.mark.parametrize("what", ["P=0", "P=65", "W=0", "trk=-1", "trk=n_tracks", "windows>max_windows"])
def test_an_invalid_scene_is_undecided_and_its_neighbours_are_untouched(eng, what):
    tracks, scenes, _ = planted((25, 26, 27), 4, 40, 7, 4)
    bad, max_windows = dict(scenes[1]), None
    if what == "P=0":
        bad["trk"] = []
    elif what == "P=65":
        bad["trk"] = [i % len(tracks) for i in range(65)]
    elif what == "W=0":
        bad.update(content=np.zeros((0, 512), np.float32), ws=np.zeros(0, np.int32), we=np.zeros(0, np.int32))
    elif what == "trk=-1":
        bad["trk"] = [4, -1, 6]
    elif what == "trk=n_tracks":
        bad["trk"] = [4, 5, len(tracks)]
    else:
        bad["n_win"], max_windows = 3 * WB + 5, scenes[0]["n_win"]
    out = call(eng, tracks, [scenes[0], bad, scenes[2]], 10, 4, gap=2, max_windows=max_windows)
    assert np.all(out["pred"][1] == -1) and out["pred"][1].size == bad["n_win"]
    assert np.isnan(out["prob"][1]).all() and np.isnan(out["cosv"][1]).all() and out["prob"][1].shape == (bad["n_win"], len(bad["trk"]))
    ok = call(eng, tracks, [scenes[0], scenes[2]], 10, 4)
    for i, j in ((0, 0), (2, 1)):
        for key in ("prob", "cosv", "pred"):
            assert np.array_equal(bits(out[key][i]), bits(ok[key][j])), (what, key, i)
    inside = np.zeros(out["raw_prob"].size, bool)
    for s, e in out["spans"]:
        inside[s:e] = True
    assert np.all(out["raw_prob"][~inside] == NAN_BITS) and np.all(out["raw_cosv"][~inside] == NAN_BITS)
    assert np.all(out["raw_pred"][out["n_pred"]:] == -7)
    refs = lambda dt: [windows_ref(tracks, scenes[0], 10, 4, dt), undecided_ref(bad), windows_ref(tracks, scenes[2], 10, 4, dt)]
    check(what, out, refs(np.float64), refs(np.float32))


# ------------------------------------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments_return_an_error_and_launch_nothing(eng):
    dev = lambda v, dt=torch.int32: torch.tensor(v, dtype=dt, device="cuda")
    g, c = torch.zeros(8, 512, device="cuda"), torch.zeros(2, 512, device="cuda")
    prob = torch.full((16,), NAN_BITS, dtype=torch.int32, device="cuda")
    cosv = torch.full((16,), NAN_BITS, dtype=torch.int32, device="cuda")
    pred = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    good = dict(g=g, go=dev([0, 8]), nt=1, c=c, co=dev([0, 2]), ws=dev([0, 3]), we=dev([2, 5]), trk=dev([0]), so=dev([0, 1]), n=1, D=512,
                win=4, hop=2, wo=dev([0, 4]), po=dev([0], torch.int64), mw=4, temp=TEMP, prob=prob, cosv=cosv, pred=pred)
    odd = torch.zeros(8 * 512 + 1, device="cuda")[1:]                   # 4 bytes off a 16-byte boundary
    bad = [dict(g=None), dict(go=None), dict(c=None), dict(co=None), dict(trk=None), dict(so=None), dict(wo=None), dict(po=None),
           dict(prob=None), dict(pred=None), dict(D=0), dict(D=-64), dict(D=96), dict(D=1088), dict(win=-1), dict(hop=0), dict(hop=-3),
           dict(win=8193), dict(temp=0.0), dict(temp=-1.0), dict(mw=0), dict(mw=8193), dict(ws=None), dict(we=None), dict(g=odd), dict(c=odd)]

    def run(a):
        return eng.lib.jg_asd_windows(eng.h, PTR(a["g"]), PTR(a["go"]), a["nt"], PTR(a["c"]), PTR(a["co"]), PTR(a["ws"]), PTR(a["we"]),
                                      PTR(a["trk"]), PTR(a["so"]), a["n"], a["D"], a["win"], a["hop"], PTR(a["wo"]), PTR(a["po"]), a["mw"],
                                      a["temp"], PTR(a["prob"]), PTR(a["cosv"]), PTR(a["pred"]))

    eng._bind_stream()
    eng.profile(True)
    eng.profile_reset()
    try:
        for b in bad:
            rc = run(dict(good, **b))
            assert rc == -1, (b, rc)
        assert run(dict(good, n=0)) == 0                                # no scene: JG_OK, nothing launched
        assert all(n == 0 for _, n in eng.profile_get().values())
    finally:
        eng.profile(False)
    torch.cuda.synchronize()
    assert np.all(prob.cpu().numpy() == NAN_BITS) and np.all(cosv.cpu().numpy() == NAN_BITS) and np.all(pred.cpu().numpy() == -7)
    assert run(dict(good, win=0, hop=0, ws=None, we=None, cosv=None)) == 0              # clip level: no bounds, no hop, no cosv
    torch.cuda.synchronize()
    assert np.all(pred.cpu().numpy()[:4] == 0) and np.all(cosv.cpu().numpy() == NAN_BITS)        # (all-zero rows: cos 0, one candidate)
    assert np.all(prob.cpu().numpy()[:4].view(np.float32) == 1.0) and np.all(prob.cpu().numpy()[4:] == NAN_BITS)


# ------------------------------------------------------------------------------------------------ 8. the Python layers
def test_asd_scores_and_asd_timeline(eng):
    from jegal_amd import metrics as M
    tracks, scenes, speakers = planted((28, 29), 4, 60, 10, 1, extra=0)
    per_scene = [[tracks[t] for t in s["trk"]] for s in scenes]
    bounds = [[[f"w{j}", int(a), int(b)] for j, (a, b) in enumerate(zip(s["ws"], s["we"]))] for s in scenes]
    lines = M.asd_timeline([s["content"] for s in scenes], bounds, per_scene, win=9, hop=1, engine=eng)
    assert [sorted(t) for t in lines] == [["pred", "prob", "start"]] * 2
    out = {"prob": [t["prob"] for t in lines], "pred": [t["pred"] for t in lines]}
    refs64 = [windows_ref(tracks, s, 9, 1) for s in scenes]
    out["cosv"] = [np.where(np.isnan(r[1]), np.nan, 0).astype(np.float32) for r in refs64]        # (the timeline returns no cosines)
    refs0 = lambda refs: [(p, np.where(np.isnan(c), np.nan, 0), d) for p, c, d in refs]
    check("asd_timeline", out, refs0(refs64), refs0([windows_ref(tracks, s, 9, 1, np.float32) for s in scenes]))
    for t, s, sp in zip(lines, scenes, speakers):
        assert t["prob"].shape == (60, 4) and t["pred"].shape == (60,) and np.array_equal(t["start"], np.arange(60))
        n = 0
        for j in range(60):                                             # a turn = 3 words = 15 frames: windows wholly inside one, the speaker wins
            turn = j // 15
            if t["pred"][j] >= 0 and j + 8 <= 15 * turn + 14:
                assert t["pred"][j] == sp[3 * turn] == turn % 4, (j, turn)
                n += 1
        assert n == 25                                                  # 7 windows per turn; frames 49.. of the last one have no word
    one = M.asd_timeline(scenes[0]["content"], bounds[0], per_scene[0], win=9, hop=1, engine=eng)          # one scene
    assert np.array_equal(bits(one["prob"]), bits(lines[0]["prob"])) and np.array_equal(one["pred"], lines[0]["pred"])
    # clip level
    contents, positives, negatives = synth.planted_asd(31, 9)
    cands = [[p] + list(ns) for p, ns in zip(positives, negatives)]
    scores = M.asd_scores(contents, cands, engine=eng)
    flat = [t for cs in cands for t in cs]
    sc, first = [], 0
    for ct, cs in zip(contents, cands):
        sc.append(dict(content=ct, ws=np.zeros(len(ct), np.int32), we=np.zeros(len(ct), np.int32), trk=list(range(first, first + len(cs))), n_win=1))
        first += len(cs)
    out = {"prob": [p.reshape(1, -1) for p, _ in scores], "pred": [np.array([d], np.int32) for _, d in scores],
           "cosv": [np.zeros((1, len(cs)), np.float32) for cs in cands]}
    check("asd_scores", out, refs0([windows_ref(flat, s, 0, 1) for s in sc]), refs0([windows_ref(flat, s, 0, 1, np.float32) for s in sc]))
