"""jg_jegal_gesture_tracks: gesture embeddings of tracks longer than the 500 rows of JEGAL's positional table (include/jegal_hip.h has the
window rule).  Expected values come from the oracle run on every span alone (jegal_oracle.jegal_forward_inference on span[None] with a
mask of ones, the core rows taken), never from the engine; the spans come from a restatement of the rule in this file, not from the
library's planner.  Tolerances are the project's own: 1e-3 rel-L2 in the default mode, 2e-5 in JG_PREC_FP32.
Smallest shapes that cross every edge: win 16, ctx 12 (spans up to 40 rows) on tracks of 1, 7, 16, 17, 40, 41 and 95 frames."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import jegal_oracle as O
from jegal_amd import synth

pytestmark = pytest.mark.gpu
TOL, AUD_TOL = 1e-3, 2e-5
WIN, CTX = 16, 12
TRACKS = [1, 7, 16, 17, 40, 41, 95]
JG_ERR_ARG, JG_ERR_STATE = -1, -3


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def windows_of(T, win, ctx):
    """The rule, restated: (span start, span end, core start, core end) of every window of a track of T frames."""
    return [(max(0, c0 - ctx), min(T, c0 + win + ctx), c0, min(c0 + win, T)) for c0 in range(0, T, win)]


def table_of(lengths, win, ctx):
    rows, base = [], 0
    for T in lengths:
        rows += [(base + s0, s1 - s0, c0 - s0, c1 - c0) for s0, s1, c0, c1 in windows_of(T, win, ctx)]
        base += T
    return np.asarray(rows, np.int32).reshape(-1, 4)


def oracle_track(jsd, feats, win, ctx, align=True):
    """(T,1024) -> (T,512): every span through the oracle as a clip of its own, its core rows kept."""
    out = torch.empty((feats.shape[0], 512))
    with torch.no_grad():
        for s0, s1, c0, c1 in windows_of(feats.shape[0], win, ctx):
            span = feats[s0:s1][None]
            if align:
                g = O.jegal_forward_inference(jsd, visual_feats=span, visual_mask=torch.ones(1, s1 - s0))[0]
            else:
                g = O.jegal_forward_gestures(jsd, span, torch.ones(1, 1, s1 - s0))[0]
            out[c0:c1] = g[c0 - s0:c1 - s0]
    return out


@pytest.fixture(scope="module")
def jsd():
    return O.tensors(synth.jegal_state_dict())


@pytest.fixture(scope="module")
def default():
    from jegal_amd._lib import Engine
    from jegal_amd.jegal import JEGAL
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = Engine.get("cuda:0")
    return e, JEGAL(engine=e).load_state_dict(synth.jegal_state_dict())


@pytest.fixture(scope="module")
def fp32():
    from jegal_amd._lib import Engine, PREC_FP32
    from jegal_amd.jegal import JEGAL
    e = Engine(0, precision=PREC_FP32)
    jg = JEGAL(engine=e).load_state_dict(synth.jegal_state_dict())
    yield e, jg
    e.close()


@pytest.fixture(scope="module")
def case(jsd):
    """The seven tracks and their oracle rows (computed once, never changed)."""
    rng = np.random.default_rng(1620)
    tracks = [torch.from_numpy(rng.standard_normal((t, 1024)).astype(np.float32)) for t in TRACKS]
    return tracks, [oracle_track(jsd, t, WIN, CTX) for t in tracks]


@pytest.fixture(scope="module")
def long_case(jsd):
    """One track of 1203 frames (over 500, no multiple of 120) at the defaults win 120, ctx 50: 11 spans of up to 220 rows."""
    rng = np.random.default_rng(1203)
    t = torch.from_numpy(rng.standard_normal((1203, 1024)).astype(np.float32))
    return t, oracle_track(jsd, t, 120, 50)


def run(e, tracks, win=WIN, ctx=CTX, **kw):
    feats = torch.cat(tracks).to(e.device)
    out = e.jegal_gesture_tracks(feats, [t.shape[0] for t in tracks], win=win, ctx=ctx, **kw).cpu()
    return list(torch.split(out, [t.shape[0] for t in tracks]))


# ------------------------------------------------------------------ parity
def test_parity_default_mode(default, case):
    e, _ = default
    tracks, ref = case
    out = run(e, tracks)
    whole = rel(torch.cat(out), torch.cat(ref))
    per = [rel(o, r) for o, r in zip(out, ref)]
    print(f"\ntracks {TRACKS} win {WIN} ctx {CTX}: whole {whole:.3e} | per track " + " ".join(f"{p:.2e}" for p in per), end="")
    assert whole < TOL
    for t, p in zip(TRACKS, per):
        if t >= 25:                     # the dataset's shortest clip; shorter tracks count in the whole-output figure
            assert p < TOL, (t, p)


def test_parity_fp32(fp32, case):
    e, _ = fp32
    tracks, ref = case
    per = [rel(o, r) for o, r in zip(run(e, tracks), ref)]
    print("\nfp32 per track " + " ".join(f"{p:.2e}" for p in per), end="")
    assert max(per) < AUD_TOL, per


@pytest.mark.parametrize("mode", ["default", "fp32"])
def test_over_length_track(request, long_case, mode):
    from jegal_amd._lib import JegalError
    e, jg = request.getfixturevalue(mode)
    t, ref = long_case
    out = jg.forward_gesture_tracks([t])          # the defaults: win 120, ctx 50
    assert len(out) == 1 and tuple(out[0].shape) == (1203, 512)
    r = rel(out[0], ref)
    worst = max(rel(out[0][c0:c1], ref[c0:c1]) for _, _, c0, c1 in windows_of(1203, 120, 50))
    print(f"\n1203 frames, {mode}: whole {r:.3e}, worst window {worst:.3e}", end="")
    tol = TOL if mode == "default" else AUD_TOL
    assert r < tol and worst < tol
    with pytest.raises(JegalError) as err:        # the clip entry still stops at the positional table
        e.jegal_gestures(t[None].to(e.device), align=True)
    assert err.value.code == JG_ERR_ARG


def test_single_window_tracks(default, fp32, jsd):
    """Tracks of at most win frames: one window each, the whole clip its span -- forward_gestures (+ align) on the clip itself."""
    lengths = [1, 7, 16, 9]
    rng = np.random.default_rng(16)
    tracks = [torch.from_numpy(rng.standard_normal((t, 1024)).astype(np.float32)) for t in lengths]
    with torch.no_grad():
        ref = [O.jegal_forward_inference(jsd, visual_feats=t[None], visual_mask=torch.ones(1, t.shape[0]))[0] for t in tracks]
    e, _ = default
    out = run(e, tracks)
    assert rel(torch.cat(out), torch.cat(ref)) < TOL
    e32, _ = fp32
    out32 = run(e32, tracks)
    padded, mask = torch.zeros((len(lengths), WIN, 1024)), torch.zeros((len(lengths), WIN))
    for i, t in enumerate(tracks):
        padded[i, :t.shape[0]], mask[i, :t.shape[0]] = t, 1
    clip = e32.jegal_gestures(padded.to(e32.device), mask.to(e32.device), align=True).cpu()
    for i, t in enumerate(lengths):
        assert rel(out32[i], ref[i]) < AUD_TOL, (t, rel(out32[i], ref[i]))
        assert rel(out32[i], clip[i, :t]) < AUD_TOL, (t, rel(out32[i], clip[i, :t]))


@pytest.mark.parametrize("mode", ["default", "fp32"])
def test_track_order_does_not_matter_under_poison(request, case, mode):
    """The same call with the tracks in another order: the same rows bit for bit, and no NaN although the workspace starts as NaN --
    an unwritten padding row or a wrong table index shows here."""
    e, _ = request.getfixturevalue(mode)
    tracks, ref = case
    order = [4, 0, 6, 2, 5, 1, 3]
    e.set_option("ws_poison", 1)
    try:
        a = run(e, tracks)
        b = run(e, [tracks[i] for i in order])
    finally:
        e.set_option("ws_poison", 0)
    assert all(torch.isfinite(x).all() for x in a + b)
    for j, i in enumerate(order):
        assert torch.equal(a[i], b[j]), (mode, TRACKS[i])
    assert rel(torch.cat(a), torch.cat(ref)) < (TOL if mode == "default" else AUD_TOL)


def test_normalize_and_align_bits(default, case, jsd):
    e, _ = default
    tracks, _ = case
    plain = torch.cat(run(e, tracks))
    unit = torch.cat(run(e, tracks, normalize=True))
    assert torch.equal(unit, e.l2norm(plain.to(e.device)).cpu())          # jg_l2norm of the same rows, bit for bit
    raw = run(e, tracks, align=False)
    ref = [oracle_track(jsd, t, WIN, CTX, align=False) for t in tracks]
    assert rel(torch.cat(raw), torch.cat(ref)) < TOL
    assert all(rel(o, r) < TOL for o, r, t in zip(raw, ref, TRACKS) if t >= 25)


def test_extract_gesture_track_from_frames(default, jsd):
    """Frames of one track -> unit rows: gestsync_clip on a batch of one, then the windows (win 2, ctx 1 on 5 frames: three windows)."""
    from jegal_amd.gestsync import GestSync
    e, _ = default
    gsd = synth.gestsync_state_dict(include_unused=False)
    GestSync(engine=e).load_state_dict(gsd)
    frames = synth.synth_frames(78, 1, 5)[0]
    out = e.extract_gesture_track(torch.from_numpy(frames).to(e.device), win=2, ctx=1).cpu()
    with torch.no_grad():
        f = O.gestsync_clip_feats(O.tensors(gsd), torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)))
    ref = O.l2_normalize(oracle_track(jsd, f, 2, 1))
    assert tuple(out.shape) == (5, 512) and rel(out, ref) < TOL, rel(out, ref)
    with pytest.raises(ValueError):
        e.extract_gesture_track(torch.from_numpy(frames[None]).to(e.device))


# ------------------------------------------------------------------ the two kernels, bit-exact against numpy
@pytest.mark.parametrize("n_windows,span_max,D", [(1, 1, 512), (1, 40, 512), (300, 40, 512), (300, 1, 512), (1, 500, 512), (300, 500, 64)])
def test_span_gather_check_point(default, n_windows, span_max, D):
    e, _ = default
    rng = np.random.default_rng(n_windows * 1000 + span_max)
    lens = rng.choice([1, span_max], n_windows)                         # span lengths 1 and span_max mixed
    if n_windows > 2:
        lens[2:n_windows:7] = rng.integers(1, span_max + 1, len(lens[2:n_windows:7]))
    rows = 2 * span_max + 3
    first = (rng.integers(0, 1 << 20, n_windows) % (rows - lens + 1)).astype(np.int32)
    table = np.stack([first, lens.astype(np.int32), np.zeros(n_windows, np.int32), lens.astype(np.int32)], 1)
    p32 = rng.standard_normal((rows, D)).astype(np.float32)
    pe = rng.standard_normal((500, D)).astype(np.float32)
    x32 = torch.full((n_windows, span_max, D), float("nan"), device=e.device)
    mask = torch.full((n_windows, span_max), float("nan"), device=e.device)
    e.debug_span_gather(torch.from_numpy(p32).to(e.device), torch.from_numpy(pe).to(e.device), torch.from_numpy(table).to(e.device),
                        n_windows, span_max, D, x32, mask)
    assert e.debug_last_kernel() == "span_gather_kernel"
    s = np.arange(span_max)
    live = s[None, :] < lens[:, None]
    want = np.where(live[:, :, None], p32[np.minimum(first[:, None] + s[None, :], rows - 1)] + pe[None, :span_max], np.float32(0))
    got, gm = x32.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))       # one fp32 add: bit for bit
    assert np.array_equal(gm, live.astype(np.float32))
    assert (got[~live] == 0).all() and (gm[~live] == 0).all()           # every padding element is zero and its mask 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_core_compact_check_point(default, dtype):
    e, _ = default
    lengths = [1, 16, 17, 33, 1, 95]                                    # cores of length 1 and of length win among them
    table = table_of(lengths, WIN, CTX)
    n_windows, span_max, total = len(table), int(table[:, 1].max()), sum(lengths)
    assert {1, WIN} <= set(table[:, 3].tolist()) and span_max == WIN + 2 * CTX
    rng = np.random.default_rng(33)
    x = torch.from_numpy(rng.standard_normal((n_windows, span_max, 512)).astype(np.float32)).to(dtype)
    out = torch.full((total + 5, 512), -7.5, dtype=dtype, device=e.device)
    e.debug_core_compact(x.to(e.device), torch.from_numpy(table).to(e.device), n_windows, span_max, 512, out)
    assert e.debug_last_kernel() == "core_compact_kernel"
    want = torch.full((total + 5, 512), -7.5, dtype=dtype)
    for w, (first, _, coff, clen) in enumerate(table.tolist()):
        want[first + coff:first + coff + clen] = x[w, coff:coff + clen]
    assert torch.equal(out.cpu(), want)                                 # a copy; only the sum T rows change
    assert (want[:total] != -7.5).any(dim=1).all() and (out.cpu()[total:] == -7.5).all()


def test_check_points_refuse_bad_arguments(default):
    from jegal_amd._lib import JegalError
    e, _ = default
    dev = e.device
    table = torch.from_numpy(table_of([40], WIN, CTX)).to(dev)
    n, S = 3, 40
    p32, pe = torch.zeros((40, 512), device=dev), torch.zeros((500, 512), device=dev)
    x32, mask = torch.full((n, S, 512), 3.0, device=dev), torch.full((n, S), 3.0, device=dev)
    x16, out = torch.zeros((n, S, 512), dtype=torch.float16, device=dev), torch.full((40, 512), 3.0, dtype=torch.float16, device=dev)
    bad_gather = [dict(p32=None), dict(pe=None), dict(table=None), dict(x32=None), dict(mask=None), dict(n=0), dict(S=0), dict(S=501), dict(D=0),
                  dict(D=510), dict(p32=p32.view(-1)[1:]), dict(x32=x32.view(-1)[1:]), dict(table=table.view(-1)[1:])]
    for change in bad_gather:
        a = {**dict(p32=p32, pe=pe, table=table, n=n, S=S, D=512, x32=x32, mask=mask), **change}
        with pytest.raises(JegalError) as err:
            e.debug_span_gather(a["p32"], a["pe"], a["table"], a["n"], a["S"], a["D"], a["x32"], a["mask"])
        assert err.value.code == JG_ERR_ARG, change
    bad_compact = [dict(x=None), dict(table=None), dict(out=None), dict(n=0), dict(S=0), dict(D=0), dict(D=6), dict(x=x16.view(-1)[1:]),
                   dict(out=out.view(-1)[1:]), dict(table=table.view(-1)[1:])]
    for change in bad_compact:
        a = {**dict(x=x16, table=table, n=n, S=S, D=512, out=out), **change}
        with pytest.raises(JegalError) as err:
            if a["x"] is None:
                e._ck(e.lib.jg_debug_core_compact(e.h, None, 2, ctypes.c_void_p(a["table"].data_ptr()), a["n"], a["S"], a["D"], ctypes.c_void_p(a["out"].data_ptr())))
            else:
                e.debug_core_compact(a["x"], a["table"], a["n"], a["S"], a["D"], a["out"])
        assert err.value.code == JG_ERR_ARG, change
    with pytest.raises(JegalError) as err:                              # an element size that is neither 2 nor 4
        e._ck(e.lib.jg_debug_core_compact(e.h, ctypes.c_void_p(x16.data_ptr()), 8, ctypes.c_void_p(table.data_ptr()), n, S, 512, ctypes.c_void_p(out.data_ptr())))
    assert err.value.code == JG_ERR_ARG
    e.sync()
    assert (x32 == 3.0).all() and (mask == 3.0).all() and (out == 3.0).all()       # nothing was enqueued


# ------------------------------------------------------------------ launches: the row-wise ends run once per track row
@pytest.mark.parametrize("mode", ["default", "fp32"])
def test_launch_counts(request, case, mode):
    """As many GEMM, attention and LayerNorm launches as ONE jg_jegal_gestures batch on the same handle -- the input projection and the
    output / align projections are launched once, on the track rows -- and two more `misc` launches (gather, compact), three with the
    l2norm."""
    e, _ = request.getfixturevalue(mode)
    tracks, _ = case

    def counts(fn):
        e.profile_reset()
        fn()
        return {k: v[1] for k, v in e.profile_get().items()}

    e.profile(True)
    try:
        clip = counts(lambda: e.jegal_gestures(torch.zeros((3, 40, 1024), device=e.device), torch.ones((3, 40), device=e.device), align=True))
        plain = counts(lambda: run(e, tracks))
        unit = counts(lambda: run(e, tracks, normalize=True))
    finally:
        e.profile(False)
        e.profile_reset()
    print(f"\n{mode}: clip batch {clip} | tracks {plain}", end="")
    assert clip["gemm"] == 29 and clip["attention"] == 6 and clip["layernorm"] == 14
    for stage in ("gemm", "attention", "layernorm"):
        assert plain[stage] == clip[stage] == unit[stage], stage
    assert plain["misc"] == clip["misc"] + 2 and unit["misc"] == clip["misc"] + 3
    assert all(plain[k] == clip[k] for k in plain if k not in ("gemm", "attention", "layernorm", "misc"))


# ------------------------------------------------------------------ errors
def raw_call(e, feats, offsets, n_tracks, win, ctx, out, align=1, normalize=0):
    off = None if offsets is None else (ctypes.c_int32 * len(offsets))(*offsets)
    e._bind_stream()
    return e.lib.jg_jegal_gesture_tracks(e.h, None if feats is None else ctypes.c_void_p(feats.data_ptr()), off, n_tracks, win, ctx, align, normalize,
                                         None if out is None else ctypes.c_void_p(out.data_ptr()))


def test_errors(default):
    from jegal_amd._lib import Engine
    e, _ = default
    feats = torch.zeros((57, 1024), device=e.device)
    out = torch.full((57, 512), 5.0, device=e.device)
    good = dict(feats=feats, offsets=[0, 40, 40, 57], n_tracks=3, win=WIN, ctx=CTX, out=out)
    bad = [dict(feats=None), dict(out=None), dict(offsets=None), dict(n_tracks=-1), dict(win=0), dict(ctx=-1), dict(win=16, ctx=243), dict(win=501, ctx=0),
           dict(offsets=[0, 40, 39, 57]), dict(offsets=[-1, 40, 40, 57]), dict(offsets=[1, 40, 40, 57])]
    for change in bad:
        assert raw_call(e, **{**good, **change}) == JG_ERR_ARG, change
    # more window rows than one call indexes: 5000 windows of 220 rows (refused before anything is read; the buffers are real all the same)
    big_f, big_o = torch.empty((600000, 1024), device=e.device), torch.full((600000, 512), 5.0, device=e.device)
    assert raw_call(e, big_f, [0, 600000], 1, 120, 50, big_o) == JG_ERR_ARG
    e.sync()
    assert (out == 5.0).all() and (big_o == 5.0).all()                  # nothing was enqueued
    del big_f, big_o
    assert raw_call(e, feats, [0], 0, WIN, CTX, out) == 0               # no tracks
    assert raw_call(e, None, None, 0, WIN, CTX, None) == 0
    assert raw_call(e, feats, [0, 0, 0], 2, WIN, CTX, out) == 0         # empty tracks only
    e.sync()
    assert (out == 5.0).all()
    assert raw_call(e, **good) == 0                                     # and the good call runs
    e.sync()
    assert torch.isfinite(out).all() and not (out == 5.0).all(dim=1).any()
    fresh = Engine(0)
    try:
        out.fill_(5.0)
        assert raw_call(fresh, **good) == JG_ERR_STATE                  # JEGAL weights never finalized
        fresh.sync()
        assert (out == 5.0).all()
    finally:
        fresh.close()


# ------------------------------------------------------------------ driver
def test_embed_tracks_driver_and_search_beyond_500_frames(default, tmp_path):
    from jegal_amd import drivers
    e, jg = default
    rng = np.random.default_rng(530)
    lengths = {"vidA/00000": 30, "vidA/00001": 530, "vidB/00000": 77}
    feats = {k: rng.standard_normal((t, 1024)).astype(np.float32) for k, t in lengths.items()}
    for k, f in feats.items():
        os.makedirs(tmp_path / "feats" / k.split("/")[0], exist_ok=True)
        np.save(tmp_path / "feats" / (k + ".npy"), f)
    argv = ["--checkpoint_path_jegal", "synthetic", "--feature_dir", str(tmp_path / "feats"), "--result_dir", str(tmp_path / "res")]
    assert drivers.cmd_embed_tracks(argv, engine=e, jegal=jg) == 0
    names = sorted(feats)
    want = jg.forward_gesture_tracks([torch.from_numpy(feats[k]) for k in names], normalize=True)
    embs = {}
    for k, w in zip(names, want):
        with open(tmp_path / "res" / "v" / (k.replace("/", "__") + ".pkl"), "rb") as f:
            d = pickle.load(f)
        assert d["content_emb"] is None and d["info"] == {"fname": k, "win": 120, "ctx": 50}
        assert d["gesture_emb"].dtype == np.float32 and np.array_equal(d["gesture_emb"], w.cpu().numpy())          # bit for bit
        assert np.allclose(np.linalg.norm(d["gesture_emb"], axis=1), 1.0, atol=1e-5)
        embs[k] = d["gesture_emb"]
    stamp = {k: os.path.getmtime(tmp_path / "res" / "v" / (k.replace("/", "__") + ".pkl")) for k in names}
    assert drivers.cmd_embed_tracks(argv + ["--rows_per_call", "100"], engine=e, jegal=jg) == 0                    # skip-if-exists
    assert stamp == {k: os.path.getmtime(tmp_path / "res" / "v" / (k.replace("/", "__") + ".pkl")) for k in names}
    # a query planted at frame 517 of the long track comes back from there
    os.makedirs(tmp_path / "query")
    with open(tmp_path / "query" / "planted.pkl", "wb") as f:
        pickle.dump({"gesture_emb": None, "content_emb": embs["vidA/00001"][517:518], "info": None}, f)
    assert drivers.cmd_search(["--path", str(tmp_path / "res" / "v"), "--query", str(tmp_path / "query" / "planted.pkl"), "--segment", "100",
                               "--topk", "5", "--res_dir", str(tmp_path / "out")], engine=e) == 0
    res = np.load(tmp_path / "out" / "search_planted.npz")
    assert str(res["names"][res["clip"][0, 0]]) == "vidA__00001" and int(res["frame"][0, 0]) == 517
    assert abs(float(res["score"][0, 0]) - 1.0) < 1e-5
