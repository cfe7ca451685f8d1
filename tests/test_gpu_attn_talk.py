"""jg_attn_talk through the C ABI (run with -m gpu): the gesture-word heat map along whole tracks against the float64 evaluation of its
definition (tests/attn_talk_cases.py; the inputs are qualified in tests/test_attn_talk_cases_cpu.py).

Error rule, the one of tests/test_gpu_attn_matrix.py (the kernel is built from the same parts): err(X) = distance of X from the float64
band as (max-abs, max relative error over entries whose true value is >= 1e-3); the kernel is held to err(kernel) <= 4 x err(fp32 twin)
in both parts, the twin being the same formula in torch fp32.  Arg-max rule: a word (a frame) is decidable if, in float64, its best frame
(word) beats the runner-up by more than 1e-3 relative; decidable ones must match the float64 arg-max exactly, the others must come within
1e-3 relative of the best.  Every output is pre-filled with sentinel bits and followed by a guard of 64 elements.

Ratios err(kernel) / err(twin) measured on MI355X as (max-abs, relative), normalize 1 | 0 (each test prints its own):
  (700, 140, 4, 1, reach 40)  D = 512: (1.00, 0.81) | (0.66, 1.00)
  (1000, 400, 2, 1, reach 25) D = 512: (0.92, 0.94) | (0.92, 0.79)
  (135, 20, 5, 2, reach 12)   D = 64:  (0.88, 0.91) | (1.00, 1.00)
  (135, 20, 5, 2, reach 12)   D = 192: (0.93, 0.61) | (0.63, 0.55)
"""
import ctypes

import numpy as np
import pytest
import torch

import attn_talk_cases as C
from test_gpu_attn_matrix import call as clip_call

pytestmark = pytest.mark.gpu
TEMP = C.TEMP
NAN_BITS = 0x7FC0BEEF      # a quiet NaN with a payload, as int32: never what the kernel writes
GUARD = 64
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def call(eng, tracks, reach, normalize=1, pitch=None, max_frames=None, want=("band", "best", "frames"), expect=0):
    """One jg_attn_talk call on tracks = [(g (T, D), c (W, D), start, end)].  -> dict(pitch, raw: the five outputs with their guards as
    int32, and per track band (W, pitch) / best_frame / best_score / frame_word / frame_prob)"""
    D = tracks[0][0].shape[1]
    T, W = np.array([t[0].shape[0] for t in tracks]), np.array([t[1].shape[0] for t in tracks])
    goff, coff = np.concatenate([[0], np.cumsum(T)]), np.concatenate([[0], np.cumsum(W)])
    n_rows, n_words = int(goff[-1]), int(coff[-1])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(x).reshape(-1) for x in a] + [np.zeros(4)]), dt)).cuda()
    g, c = dev([t[0] for t in tracks], np.float32), dev([t[1] for t in tracks], np.float32)
    ws, we = dev([t[2] for t in tracks], np.int32), dev([t[3] for t in tracks], np.int32)
    go, co = (torch.as_tensor(v.astype(np.int32), device="cuda") for v in (goff, coff))
    if pitch is None:
        pitch = max([C.band_pitch(t[2], t[3], reach) for t in tracks if len(t[2])] + [1])
    fill = lambda n: torch.full((n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    band = fill(n_words * pitch) if "band" in want else None
    bf, bs = (fill(n_words), fill(n_words)) if "best" in want else (None, None)
    fw, fp = (fill(n_rows), fill(n_rows)) if "frames" in want else (None, None)
    eng._bind_stream()
    rc = eng.lib.jg_attn_talk(eng.h, P(g), P(go), len(tracks), n_rows, int(max_frames or max(T.max(), 1)), P(c), P(co), n_words, P(ws), P(we),
                              D, reach, TEMP, normalize, P(band), pitch, P(bf), P(bs), P(fw), P(fp))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    raw = {k: (None if v is None else v.cpu().numpy()) for k, v in dict(band=band, best_frame=bf, best_score=bs, frame_word=fw, frame_prob=fp).items()}
    sizes = dict(band=n_words * pitch, best_frame=n_words, best_score=n_words, frame_word=n_rows, frame_prob=n_rows)
    out = {"pitch": pitch, "raw": raw, "tracks": []}
    for k, v in raw.items():
        if v is not None:
            assert np.all(v[sizes[k]:] == NAN_BITS), f"{k}: the guard was written"
            if rc == 0:
                assert not np.any(v[:sizes[k]] == NAN_BITS), f"{k}: an element was not written"
    for i in range(len(tracks)):
        w, f = slice(int(coff[i]), int(coff[i + 1])), slice(int(goff[i]), int(goff[i + 1]))
        d = {}
        if band is not None:
            d["band"] = raw["band"][:n_words * pitch].view(np.float32).reshape(n_words, pitch)[w]
        if bf is not None:
            d["best_frame"], d["best_score"] = raw["best_frame"][w], raw["best_score"][w].view(np.float32)
        if fw is not None:
            d["frame_word"], d["frame_prob"] = raw["frame_word"][f], raw["frame_prob"][f].view(np.float32)
        out["tracks"].append(d)
    return out


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in a) and a.keys() == b.keys()


def check_argmax(name, what, P64, idx, min_share=0.9):
    """rows of P64 = the words (frames), idx = the kernel's arg-max per row (-1: none)"""
    dec, has = C.decidable(P64, 1)
    want, _ = C.word_best(P64)
    assert np.array_equal(idx >= 0, has), (name, what)
    for r in np.nonzero(has)[0]:
        assert not np.isnan(P64[r, idx[r]]), (name, what, r)
        if dec[r]:
            assert idx[r] == want[r], (name, what, r, int(idx[r]), int(want[r]))
        else:
            assert P64[r, idx[r]] >= P64[r, want[r]] * (1 - 1e-3), (name, what, r, int(idx[r]), int(want[r]))
    print(f"{name}: {dec.sum()}/{has.sum()} decidable {what}")
    assert dec.sum() >= min_share * has.sum(), (name, what)


def check_track(name, r, pitch, g, c, s, e, reach, normalize, min_share=0.9):
    T = g.shape[0]
    P64 = C.talk64(g, c, s, e, reach, normalize)
    B64, B32 = C.band_of(P64, s, reach, pitch), C.band_of(C.talk32(g, c, s, e, reach, normalize), s, reach, pitch)
    assert np.array_equal(np.isnan(r["band"]), np.isnan(B64)), name
    k, t = C.err(r["band"], B64), C.err(B32, B64)
    print(f"{name}: kernel max-abs {k[0]:.3e} rel {k[1]:.3e} | fp32 twin max-abs {t[0]:.3e} rel {t[1]:.3e} | "
          f"ratios {k[0] / max(t[0], 1e-30):.2f} {k[1] / max(t[1], 1e-30):.2f}")
    assert k[0] <= 4 * t[0] and k[1] <= 4 * t[1], (name, k, t)
    check_argmax(name, "words", P64, r["best_frame"], min_share)
    check_argmax(name, "frames", P64.T, r["frame_word"], min_share)
    # best_score is the band entry bit for bit, and so is frame_prob
    for w in np.nonzero(r["best_frame"] >= 0)[0]:
        j = int(r["best_frame"][w] - (s[w] - reach))
        if j < pitch:
            assert bits(r["band"][w, j:j + 1])[0] == bits(r["best_score"][w:w + 1])[0], (name, w)
    assert np.isnan(r["best_score"][r["best_frame"] < 0]).all()
    for f in range(T):
        w = int(r["frame_word"][f])
        if w >= 0 and f - (s[w] - reach) < pitch:
            assert bits(r["band"][w, f - (s[w] - reach):][:1])[0] == bits(r["frame_prob"][f:f + 1])[0], (name, f)
    assert np.isnan(r["frame_prob"][r["frame_word"] < 0]).all()


# ------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("case", C.ACCURACY_INPUTS)
def test_accuracy(eng, case, normalize):
    seed, T, W, span, gap, reach, d = case
    g, c, s, e = C.planted_talk(seed, T, W, span, gap, d)
    r = call(eng, [(g, c, s, e)], reach, normalize)
    check_track(f"{case[1:]} normalize={normalize}", r["tracks"][0], r["pitch"], g, c, s, e, reach, normalize)


# ------------------------------------------------------------------------------------------------ 2. the bridge to the clip form
def dense_of(band, start, reach, T):
    """band (W, pitch) with reach >= T -> the dense (W, T) matrix"""
    return np.stack([band[w, reach - int(start[w]):reach - int(start[w]) + T] for w in range(band.shape[0])])


# d = 64 is one k chunk pair below the chain cut of 128 terms, d = 192 ends its second chain off a cut; T = 33 / W = 33 put one frame and one
# word past a 32-lane half and a 32-word tile; (160, 96) is two frame blocks, the second partial, against three full word tiles.
# (The first two cases keep the ids they had before d became a parameter.)
@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("T,W,span,gap,reach,d", [pytest.param(300, 37, 6, 2, 400, 512, id="300-37-6-2-400"),
                                                  pytest.param(129, 128, 1, 0, 200, 512, id="129-128-1-0-200"),
                                                  (33, 33, 1, 0, 64, 64), (160, 96, 2, 1, 300, 192)])
def test_full_reach_gives_the_bits_of_attn_matrix(eng, T, W, span, gap, reach, d, normalize):
    g, c, s, e = C.planted_talk(5, T, W, span, gap, d)
    assert C.reach_mask(T, s, e, reach).all()                      # what the test is about: every word in reach of every frame
    r = call(eng, [(g, c, s, e)], reach, normalize)["tracks"][0]
    clip = clip_call(eng, [g], [c], normalize)
    A = dense_of(r["band"], s, reach, T)
    assert np.array_equal(bits(A), bits(clip["mats"][0]))
    assert np.array_equal(r["best_frame"], clip["frames"][0])
    assert np.array_equal(bits(r["best_score"]), bits(clip["scores"][0]))
    assert np.array_equal(r["frame_word"], np.argmax(A, axis=0)) and np.array_equal(r["frame_prob"], A.max(axis=0))


def test_more_than_128_candidates_is_undecided(eng):
    g, c, s, e = C.planted_talk(5, 129, 129, 1, 0)
    r = call(eng, [(g, c, s, e)], 200)["tracks"][0]                # returns JG_OK
    assert np.isnan(r["band"]).all() and np.all(r["best_frame"] == -1) and np.isnan(r["best_score"]).all()
    assert np.all(r["frame_word"] == -1) and np.isnan(r["frame_prob"]).all()
    # ... block by block: at reach 0 every block of the same track has at most 128 candidates and is decided
    r = call(eng, [(g, c, s, e)], 0)["tracks"][0]
    assert np.array_equal(r["best_frame"], np.arange(129)) and np.all(r["band"] == np.float32(1.0))
    # and Python restates the rule on the host
    with pytest.raises(ValueError, match="lower reach"):
        eng.attn_talk(g, c, [0, 129], [0, 129], s, e, reach=200)


# ------------------------------------------------------------------------------------------------ 3. reach = 0
def test_reach_zero(eng):
    T, W, span, gap = 135, 20, 5, 2
    g, c, s, e = C.planted_talk(30, T, W, span, gap, 64)
    out = call(eng, [(g, c, s, e)], 0)
    r = out["tracks"][0]
    assert out["pitch"] == span
    inside = (s[:, None] + np.arange(span)[None]) < T
    assert np.all(r["band"][inside] == np.float32(1.0)) and np.isnan(r["band"][~inside]).all()
    assert np.array_equal(r["best_frame"], s) and np.all(r["best_score"] == np.float32(1.0))
    want = np.full(T, -1)
    for w in range(W):
        want[s[w]:e[w] + 1] = w
    assert np.array_equal(r["frame_word"], want)
    assert np.all(r["frame_prob"][want >= 0] == np.float32(1.0)) and np.isnan(r["frame_prob"][want < 0]).all()


# ------------------------------------------------------------------------------------------------ 4. edges, in one batch
def edge_tracks():
    rng = np.random.default_rng(77)
    rows = lambda n: (rng.standard_normal((n, 64)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    I = lambda *v: np.array(v, np.int64)
    one = (rows(1), rows(2), I(0, 1), I(0, 3))                                   # a one-frame track
    empty = (rows(0), rows(3), I(0, 2, 4), I(1, 3, 5))                           # an empty track with words
    wordless = (rows(40), rows(0), I(), I())                                     # a track without words
    g, c = rows(50), rows(5)
    g[26] = g[27] = 3 * c[2]                     # two identical adjacent frame rows, on which the long word has its maximum
    #             cut at frame 0 | ......... | longer than the small band_pitch | ......... | starts beyond T
    main = (g, c, I(1, 6, 10, 24, 60), I(4, 27, 30, 36, 62))                     # (every frame in reach of word 2 has a second word)
    other = (rows(150), rows(9), np.arange(9) * 16, np.arange(9) * 16 + 9)       # a track of two blocks
    return [one, empty, wordless, main, other]


def test_edges_in_one_batch(eng):
    reach = 3
    tracks = edge_tracks()
    batch = call(eng, tracks, reach)
    pitch = batch["pitch"]
    assert pitch == 2 * reach + 22
    for i, (g, c, s, e) in enumerate(tracks):
        r = batch["tracks"][i]
        full = g.shape[0] > 0 and len(s) > 0
        P64 = C.talk64(g, c, s, e, reach, 1) if full else None
        B64 = C.band_of(P64, s, reach, pitch) if full else np.full((len(s), pitch), np.nan)
        # Tolerance: with normalised rows |x| <= 1 / 0.07 = 14.3, a 64-term fp32 dot product is off by a few ulp of 1 (6e-8) at most, so
        # x by about 14.3 x 4 x 6e-8 = 3.4e-6 absolute, which is the relative error of exp(x); 1e-4 leaves the softmax's own roundings
        # and a factor of ten
        assert np.array_equal(np.isnan(r["band"]), np.isnan(B64)), i
        assert np.allclose(r["band"], B64, rtol=1e-4, atol=0, equal_nan=True), i
        if full:
            check_argmax(f"edge track {i}", "words", P64, r["best_frame"], 0.0)
            check_argmax(f"edge track {i}", "frames", P64.T, r["frame_word"], 0.0)
        alone = call(eng, [tracks[i]], reach, pitch=pitch)["tracks"][0]          # each track alone gives the bits it gives in the batch
        assert same_bits(alone, r), i
    one, empty, wordless, main = (batch["tracks"][i] for i in range(4))
    assert one["frame_word"][0] in (0, 1) and not np.isnan(one["band"][1, 2])     # word 1 starts beyond the frame, within reach of it
    assert np.all(empty["best_frame"] == -1) and np.isnan(empty["band"]).all()
    assert np.all(wordless["frame_word"] == -1) and np.isnan(wordless["frame_prob"]).all()
    assert np.isnan(main["band"][0, :2]).all() and not np.isnan(main["band"][0, 2:10]).any()        # frames -2, -1 | 0 .. 7
    assert main["best_frame"][4] == -1 and np.isnan(main["band"][4]).all()                          # the word beyond T
    col = lambda f: np.array([bits(main["band"][w, f - (s - reach):][:1])[0] for w, s in ((1, 6), (2, 10), (3, 24))])
    assert np.array_equal(col(26), col(27)) and main["best_frame"][2] == 26                         # equal columns, the tie to the first
    assert main["frame_word"][26] == 2 and main["frame_word"][27] == 2
    assert bits(main["frame_prob"][26:27])[0] == bits(main["frame_prob"][27:28])[0]
    # a word longer than band_pitch keeps its first band_pitch frames; best_* still cover the whole range
    small = call(eng, tracks, reach, pitch=14)
    for i in range(len(tracks)):
        a, b = small["tracks"][i], batch["tracks"][i]
        assert np.array_equal(bits(a["band"]), bits(b["band"][:, :14])), i
        assert same_bits({k: a[k] for k in a if k != "band"}, {k: b[k] for k in b if k != "band"}), i
    assert small["tracks"][3]["best_frame"][2] == 26 > 10 - reach + 14
    # a track longer than max_frames is undecided as a whole, and its neighbours keep their bits
    cut = call(eng, tracks, reach, max_frames=50)
    u = cut["tracks"][4]
    assert np.isnan(u["band"]).all() and np.all(u["best_frame"] == -1) and np.isnan(u["best_score"]).all()
    assert np.all(u["frame_word"] == -1) and np.isnan(u["frame_prob"]).all()
    for i in range(4):
        assert same_bits(cut["tracks"][i], batch["tracks"][i]), i
    # every subset of the outputs gives the same bits
    for want in (("band",), ("best",), ("frames",)):
        part = call(eng, tracks, reach, want=want)
        for i in range(len(tracks)):
            assert all(np.array_equal(bits(v), bits(batch["tracks"][i][k])) for k, v in part["tracks"][i].items()), (want, i)


def test_python_entry_gives_the_same_bits(eng):
    from jegal_amd import metrics as M
    tracks = edge_tracks()[3:]
    batch = call(eng, tracks, 3)
    res = M.talk_heatmap([t[0] for t in tracks], [t[1] for t in tracks], [list(zip(t[2], t[3])) for t in tracks], reach=3, engine=eng)
    spots = M.spot_talk([t[0] for t in tracks], [t[1] for t in tracks], [list(zip(t[2], t[3])) for t in tracks], reach=3, engine=eng)
    for r, sp, want, t in zip(res, spots, batch["tracks"], tracks):
        assert np.array_equal(r["first_frame"], t[2] - 3)
        assert same_bits({k: r[k] for k in want}, want)
        assert sorted(sp) == ["best_frame", "best_score", "frame_prob", "frame_word"] and same_bits(sp, {k: want[k] for k in sp})


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(eng):
    g, c = torch.zeros(8, 64, device="cuda"), torch.zeros(2, 64, device="cuda")
    go, co = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([0, 8], [0, 2]))
    ws, we = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([0, 4], [3, 7]))
    outs = {k: torch.full((n,), NAN_BITS, dtype=torch.int32, device="cuda") for k, n in
            (("band", 2 * 6 + GUARD), ("bf", 2 + GUARD), ("bs", 2 + GUARD), ("fw", 8 + GUARD), ("fp", 8 + GUARD))}
    good = dict(g=g, go=go, n=1, rows=8, mf=8, c=c, co=co, nw=2, ws=ws, we=we, D=64, reach=1, temp=TEMP, pitch=6, **outs)
    odd_g, odd_c = torch.zeros(8 * 64 + 1, device="cuda")[1:], torch.zeros(2 * 64 + 1, device="cuda")[1:]      # 4 bytes off a 16-byte boundary
    bad = [dict(g=None), dict(go=None), dict(c=None), dict(co=None), dict(ws=None), dict(we=None),              # null operands
           dict(band=None, bf=None, bs=None, fw=None, fp=None),                                                  # no output at all
           dict(mf=0), dict(mf=2 ** 20 + 1), dict(reach=-1), dict(reach=1025), dict(D=96), dict(D=0), dict(temp=0.0), dict(temp=-1.0),
           dict(pitch=0), dict(pitch=-3), dict(nw=2, pitch=2 ** 30), dict(g=odd_g), dict(c=odd_c), dict(n=-1), dict(rows=-1), dict(nw=-1)]

    def run(a):
        return eng.lib.jg_attn_talk(eng.h, P(a["g"]), P(a["go"]), a["n"], a["rows"], a["mf"], P(a["c"]), P(a["co"]), a["nw"], P(a["ws"]), P(a["we"]),
                                    a["D"], a["reach"], a["temp"], 1, P(a["band"]), a["pitch"], P(a["bf"]), P(a["bs"]), P(a["fw"]), P(a["fp"]))
    eng._bind_stream()
    eng.profile(True)
    eng.profile_reset()
    try:
        for b in bad:
            assert run(dict(good, **b)) == -1, b
        assert run(dict(good, n=0)) == 0                                # no track: JG_OK, nothing launched
        assert all(n == 0 for _, n in eng.profile_get().values())
    finally:
        eng.profile(False)
    torch.cuda.synchronize()
    assert all(np.all(t.cpu().numpy() == NAN_BITS) for t in outs.values())
    # the largest legal values get past the checks (and the good call runs)
    for ok in (dict(reach=1024, pitch=2 * 1024 + 4), dict(reach=0, pitch=4), dict(mf=2 ** 20)):
        a = dict(good, **ok)
        if a["pitch"] != 6:
            a["band"] = torch.full((2 * a["pitch"] + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
        assert run(a) == 0, ok
    torch.cuda.synchronize()
    assert np.all(outs["band"].cpu().numpy()[12:] == NAN_BITS) and not np.any(outs["band"].cpu().numpy()[:12] == NAN_BITS)
