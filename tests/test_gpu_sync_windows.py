"""jg_sync_offset_windows through the C ABI (run with -m gpu): offsets, confidences, curves and the band of planted ragged batches against
the float64 statement of the contract (tests/sync_windows_cases.py), and the bit identities include/jegal_hip.h promises.

Offsets: the float64 arg-max on EVERY window -- tests/test_sync_windows_cpu.py proves each planted window decidable (float64 margin >= 1e-3).
Curve, conf and band: err(X) = max-abs distance of X from float64 pooled over the clips of one call; the kernels are held to
err(kernel) <= 4 x err(float32 numpy statement), the rule and the figure of tests/test_gpu_sync_offset.py.  The NaN patterns must be the
statement's.  Every output and the band lie between guard words that must survive, and are pre-filled with the guard pattern, so an element
that must not be written still shows it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sync_offset_cases as C
import sync_windows_cases as S

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
GUARD = 64
GUARD_BITS = 0x7FC0BEEF          # a quiet NaN with a payload, as int32
ARG = -1


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def offsets(xs):
    return np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.int64)


def call(eng, vids, auds, R, mo, win, hop, nwins, a_of=None, want_curve=True, want_band=True, expect=0, D=None, n=None, n_aud=None,
         max_rows=None, max_windows=None, n_vid_rows=None, misalign=False, null=()):
    """One jg_sync_offset_windows call -> dict(offset, conf, curve | None, band | None, written: per output the mask of the elements that
    no longer hold the guard pattern) on the host; guards checked.  n / n_aud / max_rows / max_windows / n_vid_rows override
    what the clips imply; null: names of pointer arguments to pass as NULL."""
    D = D or vids[0].shape[1]
    W = 2 * R + 1
    cat = lambda xs: torch.from_numpy(np.ascontiguousarray(np.concatenate(list(xs) + [np.zeros((4, xs[0].shape[1]), np.float32)]), np.float32)).cuda()
    v, a = cat(vids), cat(auds)
    if misalign:
        v = v.reshape(-1)[1:]
    vo, ao = offsets(vids), offsets(auds)
    wo = np.concatenate([[0], np.cumsum(nwins)]).astype(np.int64)
    n = len(vids) if n is None else n
    n_aud = len(auds) if n_aud is None else n_aud
    rows = int(sum(x.shape[0] for x in vids)) if n_vid_rows is None else n_vid_rows
    nwin = int(sum(nwins))
    dev = lambda x: torch.as_tensor(np.asarray(x, np.int32), device="cuda")
    vo_d, ao_d, wo_d = dev(vo), dev(ao), dev(wo)
    af_d = None if a_of is None else dev(a_of)
    buf = lambda m: torch.full((GUARD + m + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    band_rows = sum(x.shape[0] for x in vids)
    sizes = dict(curve=nwin * W, offset=nwin, conf=nwin, band=band_rows * W)
    bufs = {k: buf(m) for k, m in sizes.items()}
    at = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 4 * GUARD)
    if max_rows is None:
        max_rows = max([1] + [x.shape[0] for x in vids] + [x.shape[0] for x in auds])
    if max_windows is None:
        max_windows = max([1] + list(nwins))
    ptr = dict(vid=P(v), voff=P(vo_d), aud=P(a), aoff=P(ao_d), a_of=P(af_d), woff=P(wo_d), band=at("band") if want_band else None,
               curve=at("curve") if want_curve else None, offset=at("offset"), conf=at("conf"))
    for k in null:
        ptr[k] = None
    eng._bind_stream()
    rc = eng.lib.jg_sync_offset_windows(eng.h, ptr["vid"], ptr["voff"], n, rows, max_rows, ptr["aud"], ptr["aoff"], n_aud, ptr["a_of"], D, R, mo,
                                        win, hop, ptr["woff"], max_windows, ptr["band"], ptr["curve"], ptr["offset"], ptr["conf"])
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, b in host.items():
        assert (b[:GUARD] == GUARD_BITS).all() and (b[GUARD + sizes[k]:] == GUARD_BITS).all(), k + ": a guard word was overwritten"
    body = {k: b[GUARD:GUARD + sizes[k]] for k, b in host.items()}
    if expect != 0 or n <= 0:
        for k, b in body.items():
            assert (b == GUARD_BITS).all(), k + " was written"
        return None
    if not want_curve or "curve" in null:
        assert (body["curve"] == GUARD_BITS).all(), "the curve was written"
    if not want_band or "band" in null:
        assert (body["band"] == GUARD_BITS).all(), "the band was written"
    return dict(offset=body["offset"].copy(), conf=body["conf"].view(np.float32).copy(),
                curve=body["curve"].view(np.float32).reshape(nwin, W).copy() if want_curve else None,
                band=body["band"].view(np.float32).reshape(band_rows, W).copy() if want_band else None,
                written={k: b != GUARD_BITS for k, b in body.items()}, wo=wo, vo=vo)


def bits(x):
    return None if x is None else np.ascontiguousarray(x).view(np.int32)


def same_bits(a, b, keys=("offset", "conf", "curve", "band")):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        assert np.array_equal(bits(a[k]), bits(b[k])), k


@functools.lru_cache(maxsize=None)
def band_refs(D, R):
    """per clip of S.batch(D, R): (band float64, band float32) -- computed once, shared by the (win, hop) cases, never modified"""
    return tuple((S.band_ref(v, a, R), S.band_ref(v, a, R, np.float32)) for v, a in S.batch(D, R))


def check(name, got, clips, R, mo, win, hop, nwins, bands=None, max_rows=S.MAX_ROWS):
    """offsets and NaN patterns clip by clip; -> the errors (curve kernel, curve fp32 statement, conf .., band ..) pooled over the call"""
    err = np.zeros(6)
    for i, (v, a) in enumerate(clips):
        b64, b32 = bands[i] if bands else (S.band_ref(v, a, R), S.band_ref(v, a, R, np.float32))
        o64, c64, k64 = S.windows_ref(v, a, R, mo, win, hop, nwins[i], band=b64, max_rows=max_rows)
        _, c32, k32 = S.windows_ref(v, a, R, mo, win, hop, nwins[i], np.float32, band=b32, max_rows=max_rows)
        w0, w1 = int(got["wo"][i]), int(got["wo"][i + 1])
        of, co = got["offset"][w0:w1], got["conf"][w0:w1]
        assert np.array_equal(of, o64), (name, i, v.shape, a.shape, of, o64)
        assert np.array_equal(np.isnan(co), np.isnan(c64)), (name, i)
        ok = ~np.isnan(c64)
        if ok.any():
            err[2] = max(err[2], np.abs(co[ok] - c64[ok]).max())
            err[3] = max(err[3], np.abs(c32[ok].astype(np.float64) - c64[ok]).max())
        if got["curve"] is not None:
            cu = got["curve"][w0:w1]
            assert np.array_equal(np.isnan(cu), np.isnan(k64)), (name, i)
            ok = ~np.isnan(k64)
            if ok.any():
                err[0] = max(err[0], np.abs(cu[ok] - k64[ok]).max())
                err[1] = max(err[1], np.abs(k32[ok].astype(np.float64) - k64[ok]).max())
        if got["band"] is not None:
            v0 = int(got["vo"][i])
            bd = got["band"][v0:v0 + v.shape[0]]
            assert np.array_equal(np.isnan(bd), np.isnan(b64)), (name, i)
            ok = ~np.isnan(b64)
            if ok.any():
                err[4] = max(err[4], np.abs(bd[ok] - b64[ok]).max())
                err[5] = max(err[5], np.abs(b32[ok].astype(np.float64) - b64[ok]).max())
    return err


def hold(name, err):
    """the error rule, on the errors pooled over one call"""
    for j, part in enumerate(("curve", "conf", "band")):
        k, r = err[2 * j], err[2 * j + 1]
        print(f"{name}: {part} max-abs kernel {k:.3e} fp32 statement {r:.3e} ratio {k / max(r, 1e-30):.2f}")
    for j, part in enumerate(("curve", "conf", "band")):
        assert err[2 * j] <= 4 * err[2 * j + 1], (name, part, err[2 * j], err[2 * j + 1])


def split(clips):
    return [c[0] for c in clips], [c[1] for c in clips]


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("win,hop", S.WINHOP)
@pytest.mark.parametrize("D,R", C.SWEEP)
def test_planted_windows(eng, D, R, win, hop):
    """11 clips: Tv in 1, 31, 33, 150 x Ta = Tv, Tv + 3, Tv - 3, planted at -R, 0, R; windows of one row, windows that straddle a 32-row
    block edge (40, 24), windows aligned to it (32, 32), one window longer than the clip (200, 50), one window over all rows (0).  The band
    given and the band in the workspace: the same bits."""
    clips = S.batch(D, R)
    assert [c[0].shape[0] for c in clips] == [1, 1, 31, 31, 31, 33, 33, 33, 150, 150, 150]
    nwins = [S.n_windows(c[0].shape[0], win, hop) for c in clips]
    name = f"D={D} R={R} win={win} hop={hop}"
    got = call(eng, *split(clips), R, 1, win, hop, nwins)
    hold(name, check(name, got, clips, R, 1, win, hop, nwins, band_refs(D, R)))
    assert got["written"]["band"].all() and got["written"]["curve"].all()
    scratch = call(eng, *split(clips), R, 1, win, hop, nwins, want_band=False)
    same_bits(got, scratch)
    nocurve = call(eng, *split(clips), R, 1, win, hop, nwins, want_curve=False, want_band=False)
    same_bits(got, nocurve)


@pytest.mark.parametrize("D,R", C.SWEEP)
def test_one_window_gives_the_bits_of_sync_offset(eng, D, R):
    """win = 0, and win >= Tv with j = 0, on the 37 clips of sync_offset_cases.sweep_batch: offset, conf and curve bits of jg_sync_offset"""
    from test_gpu_sync_offset import call as call_offset
    clips = C.sweep_batch(D, R)
    of, co, cu = call_offset(eng, clips, R, 1)
    for win, hop in ((0, 1), (150, 7), (4000, 1)):
        got = call(eng, *split(clips), R, 1, win, hop, [1] * len(clips))
        assert np.array_equal(got["offset"], of) and np.array_equal(bits(got["conf"]), bits(co)) and np.array_equal(bits(got["curve"]), bits(cu)), (win, hop)
    clips, Rs, mo = C.special_clips()["short_min_overlap"]
    of, co, cu = call_offset(eng, clips, Rs, mo)
    got = call(eng, *split(clips), Rs, mo, 0, 1, [1] * len(clips))
    assert np.array_equal(got["offset"], of) and np.array_equal(bits(got["conf"]), bits(co)) and np.array_equal(bits(got["curve"]), bits(cu))


# ------------------------------------------------------------------------------------------------ bit identities
def test_the_same_rows_through_two_hops_give_the_same_bits(eng):
    """[48, 87] is window 2 of hop 24, window 3 of hop 16 and window 1 of hop 48; [144, 149] (cut at the clip's end) is window 6 of hop 24
    and window 3 of hop 48"""
    clips = S.batch(1024, 15)[8:9]
    res = {hop: call(eng, *split(clips), 15, 1, 40, hop, [n]) for hop, n in ((24, 7), (16, 10), (48, 4))}
    for (h0, j0), (h1, j1) in (((24, 2), (16, 3)), ((24, 2), (48, 1)), ((24, 6), (48, 3)), ((24, 4), (16, 6)), ((24, 0), (16, 0))):
        assert h0 * j0 == h1 * j1
        for k in ("offset", "conf", "curve"):
            assert np.array_equal(bits(res[h0][k][j0]), bits(res[h1][k][j1])), (h0, j0, h1, j1, k)
    same_bits(res[24], res[16], keys=("band",))


def test_poisoned_workspace_gives_the_same_bits(eng):
    clips = S.batch(64, 15)
    nwins = [S.n_windows(c[0].shape[0], 40, 24) for c in clips]
    ref = call(eng, *split(clips), 15, 1, 40, 24, nwins)
    eng.set_option("ws_poison", 1)
    try:
        poisoned = call(eng, *split(clips), 15, 1, 40, 24, nwins, want_band=False)
        given = call(eng, *split(clips), 15, 1, 40, 24, nwins)
    finally:
        eng.set_option("ws_poison", 0)
    same_bits(ref, poisoned)
    same_bits(ref, given)


def test_a_clip_gives_the_same_bits_alone_first_and_last(eng):
    clips = S.batch(1024, 15)
    probe, others = clips[9], [clips[2], clips[8], clips[5]]
    nw = lambda cs: [S.n_windows(c[0].shape[0], 40, 24) for c in cs]
    alone = call(eng, *split([probe]), 15, 1, 40, 24, nw([probe]))
    first = call(eng, *split([probe] + others), 15, 1, 40, 24, nw([probe] + others))
    last = call(eng, *split(others + [probe]), 15, 1, 40, 24, nw(others + [probe]))
    n, T = nw([probe])[0], probe[0].shape[0]
    for k in ("offset", "conf", "curve"):
        assert np.array_equal(bits(alone[k]), bits(first[k][:n])) and np.array_equal(bits(alone[k]), bits(last[k][-n:])), k
    assert np.array_equal(bits(alone["band"]), bits(first["band"][:T])) and np.array_equal(bits(alone["band"]), bits(last["band"][-T:]))


def test_tracks_that_share_an_audio_track(eng):
    """two video tracks that hold the same rows against ONE audio track through a_of (bit-equal results, the float64 result), a clip with
    another audio track between them; the audio tracks are stored in another order than the clips"""
    clips = S.batch(64, 15)
    v, a = clips[10]
    other, other_a = clips[8]
    vids, auds, a_of = [v, other, v.copy()], [other_a, a], [1, 0, 1]
    nwins = [S.n_windows(150, 40, 24)] * 3
    got = call(eng, vids, auds, 15, 1, 40, 24, nwins, a_of=a_of)
    n, T = nwins[0], 150
    for k in ("offset", "conf", "curve"):
        assert np.array_equal(bits(got[k][:n]), bits(got[k][2 * n:])), k
    assert np.array_equal(bits(got["band"][:T]), bits(got["band"][2 * T:]))
    pairs = [(v, a), (other, other_a), (v, a)]
    hold("shared audio", check("shared audio", got, pairs, 15, 1, 40, 24, nwins))
    # and the same clip with an audio track of its own (a_of NULL): the same bits
    own = call(eng, [v], [a], 15, 1, 40, 24, nwins[:1])
    for k in ("offset", "conf", "curve"):
        assert np.array_equal(bits(own[k]), bits(got[k][:n])), k


# ------------------------------------------------------------------------------------------------ drift, a long track
def test_drifting_clip(eng):
    p = S.DRIFT
    v, a = S.drift_clip()
    n = S.n_windows(p["Tv"], p["win"], p["hop"])
    got = call(eng, [v], [a], p["R"], 1, p["win"], p["hop"], [n])
    hold("drift", check("drift", got, [(v, a)], p["R"], 1, p["win"], p["hop"], [n]))
    before = [j for j in range(n) if j * p["hop"] + p["win"] - 1 < p["s"]]
    after = [j for j in range(n) if j * p["hop"] >= p["s"]]
    assert len(before) >= 2 and len(after) >= 2
    assert (got["offset"][before] == p["d0"]).all() and (got["offset"][after] == p["d1"]).all()


def test_long_track(eng):
    """8200 rows: beyond jg_sync_offset's limit; 257 row blocks, 324 windows"""
    p = S.LONG
    v, a = S.long_clip()
    n = S.n_windows(p["T"], p["win"], p["hop"])
    assert p["T"] > C.MAX_T and n == 324
    got = call(eng, [v], [a], p["R"], 1, p["win"], p["hop"], [n])
    hold("long", check("long", got, [(v, a)], p["R"], 1, p["win"], p["hop"], [n]))
    assert (got["offset"] == p["d0"]).all()
    one = call(eng, [v], [a], p["R"], 1, 0, 1, [1])
    hold("long, one window", check("long, one window", one, [(v, a)], p["R"], 1, 0, 1, [1]))
    same_bits(got, one, keys=("band",))


# ------------------------------------------------------------------------------------------------ undecided
def undecided(got, i):
    w0, w1 = int(got["wo"][i]), int(got["wo"][i + 1])
    return (got["offset"][w0:w1] == 0).all() and np.isnan(got["conf"][w0:w1]).all() and np.isnan(got["curve"][w0:w1]).all() and \
        got["written"]["offset"][w0:w1].all() and got["written"]["conf"][w0:w1].all() and got["written"]["curve"].reshape(-1, got["curve"].shape[1])[w0:w1].all()


def band_untouched(got, i, T):
    v0 = int(got["vo"][i])
    return not got["written"]["band"].reshape(-1, got["band"].shape[1])[v0:v0 + T].any()


def test_undecided_clips_between_good_ones(eng):
    """every clip that the offsets put outside the limits is undecided in all its windows, none of its band rows is written, and the good
    clips around it give the bits they give in a call of their own"""
    R, win, hop, D = 15, 40, 24, 64
    good = S.batch(D, R)
    g0, g1, g2 = good[8], good[4], good[10]
    rng = np.random.default_rng(5)
    rnd = lambda t: rng.standard_normal((t, D)).astype(np.float32)
    nw = lambda c: S.n_windows(c[0].shape[0], win, hop)
    ref = call(eng, *split([g0, g1, g2]), R, 1, win, hop, [nw(g0), nw(g1), nw(g2)])
    ref_rows = {0: (0, nw(g0)), 1: (nw(g0), nw(g0) + nw(g1)), 2: (nw(g0) + nw(g1), nw(g0) + nw(g1) + nw(g2))}

    def good_unchanged(got, where):
        for i, r in where.items():
            w0, w1 = int(got["wo"][i]), int(got["wo"][i + 1])
            for k in ("offset", "conf", "curve"):
                assert np.array_equal(bits(got[k][w0:w1]), bits(ref[k][ref_rows[r][0]:ref_rows[r][1]])), (i, k)

    # a track longer than max_rows (video, then audio), an empty video track, an empty audio track
    big_v, big_a = (rnd(200), rnd(150)), (rnd(150), rnd(200))
    empty_v, empty_a = (rnd(0), rnd(8)), (rnd(8), rnd(0))
    clips = [g0, big_v, g1, big_a, empty_v, empty_a, g2]
    nwins = [nw(g0), 3, nw(g1), 3, 2, 2, nw(g2)]
    got = call(eng, *split(clips), R, 1, win, hop, nwins, max_rows=150)
    for i in (1, 3, 4, 5):
        assert undecided(got, i) and band_untouched(got, i, clips[i][0].shape[0]), i
    good_unchanged(got, {0: 0, 2: 1, 6: 2})
    # a_of out of range (both sides)
    clips = [g0, g1, g2]
    nwins = [nw(c) for c in clips]
    for bad in (3, -1):
        got = call(eng, *split(clips), R, 1, win, hop, nwins, a_of=[0, bad, 2])
        assert undecided(got, 1) and band_untouched(got, 1, g1[0].shape[0])
        good_unchanged(got, {0: 0, 2: 2})
    # v0 + Tv > n_vid_rows: the last clip's rows end behind the rows the caller says vid has
    rows = sum(c[0].shape[0] for c in clips)
    got = call(eng, *split(clips), R, 1, win, hop, nwins, n_vid_rows=rows - 1)
    assert undecided(got, 2) and band_untouched(got, 2, g2[0].shape[0])
    good_unchanged(got, {0: 0, 1: 1})
    # more windows than max_windows: all of them undecided, however many
    got = call(eng, *split(clips), R, 1, win, hop, [nw(g0), 9, nw(g2)], max_windows=6)
    assert undecided(got, 1) and band_untouched(got, 1, g1[0].shape[0])
    good_unchanged(got, {0: 0, 2: 2})
    # windows that start at or beyond Tv are undecided alone (window 6 begins at row 144 of 150: a window; 7 and 8 begin at 168 and 192):
    # the clip's other windows and the other clips are the reference's
    got = call(eng, *split(clips), R, 1, win, hop, [nw(g0) + 3, nw(g1), nw(g2)])
    w1 = nw(g0)
    assert w1 == 6 and not np.isnan(got["conf"][w1]) and not np.isnan(got["curve"][w1][:R + 1]).any()
    assert (got["offset"][w1 + 1:w1 + 3] == 0).all() and np.isnan(got["conf"][w1 + 1:w1 + 3]).all() and np.isnan(got["curve"][w1 + 1:w1 + 3]).all()
    assert got["written"]["band"].all() and got["written"]["offset"].all() and got["written"]["conf"].all() and got["written"]["curve"].all()
    for k in ("offset", "conf", "curve"):
        assert np.array_equal(bits(got[k][:w1]), bits(ref[k][:w1])) and np.array_equal(bits(got[k][w1 + 3:]), bits(ref[k][w1:])), k
    # min_overlap larger than any overlap: every window undecided, the band is written all the same
    got = call(eng, *split(clips), R, 41, win, hop, nwins)
    assert all(undecided(got, i) for i in range(3)) and got["written"]["band"].all()
    same_bits(got, ref, keys=("band",))
    check("min_overlap 41", got, clips, R, 41, win, hop, nwins)
    # min_overlap that cuts some shifts only (the clip's last window is 30 rows long)
    got = call(eng, *split(clips), R, 35, win, hop, nwins)
    hold("min_overlap 35", check("min_overlap 35", got, clips, R, 35, win, hop, nwins))
    assert np.isnan(got["curve"]).any() and not np.isnan(got["curve"]).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_anything_is_written(eng):
    clips = S.batch(64, 1)[2:5]
    vids, auds = split(clips)
    nwins = [S.n_windows(c[0].shape[0], 8, 4) for c in clips]
    bad = lambda **kw: call(eng, vids, auds, kw.pop("R", 1), kw.pop("mo", 1), kw.pop("win", 8), kw.pop("hop", 4), nwins, expect=ARG, **kw) is None
    assert bad(R=65) and bad(R=-1) and bad(mo=0)
    assert bad(D=96) and bad(D=2048) and bad(D=-64)
    assert bad(n=-1) and bad(misalign=True)
    assert bad(win=-1) and bad(hop=0) and bad(hop=-3)
    assert bad(max_rows=0) and bad(max_rows=2 ** 20 + 1) and bad(max_windows=0) and bad(max_windows=2 ** 20 + 1)
    assert bad(n_vid_rows=-1) and bad(n_vid_rows=2 ** 40 // 3 + 1)
    assert bad(n_aud=2)                                            # without a_of: one audio track per clip
    assert bad(n_aud=0, a_of=[0, 0, 0])                            # clips, but no audio track
    for k in ("vid", "voff", "aud", "aoff", "woff", "offset", "conf"):
        assert bad(null=(k,)), k
    assert call(eng, vids, auds, 1, 1, 0, 0, [1, 1, 1]) is not None                # win == 0: hop is ignored
    assert call(eng, vids, auds, 1, 1, 8, 4, nwins, n=0, n_aud=0) is None          # nothing to do: JG_OK, nothing written


# ------------------------------------------------------------------------------------------------ Python entries
def test_python_entries(eng):
    from jegal_amd import metrics
    clips = S.batch(64, 15)
    vids, auds = split(clips)
    line = metrics.sync_timeline(vids, auds, win=40, hop=24, max_shift=15, engine=eng)
    nwins = [S.n_windows(v.shape[0], 40, 24) for v in vids]
    assert [len(t["offset"]) for t in line] == nwins and list(line[8]["start"]) == [0, 24, 48, 72, 96, 120]
    assert line[8]["offset"].dtype == np.int32 and line[8]["conf"].dtype == np.float32 and line[8]["curve"].shape == (6, 31)
    got = dict(offset=np.concatenate([t["offset"] for t in line]), conf=np.concatenate([t["conf"] for t in line]),
               curve=np.concatenate([t["curve"] for t in line]), band=None, wo=np.concatenate([[0], np.cumsum(nwins)]))
    hold("metrics.sync_timeline", check("metrics.sync_timeline", got, clips, 15, 1, 40, 24, nwins))
    dev = metrics.sync_timeline([torch.from_numpy(v).cuda() for v in vids], [torch.from_numpy(a).cuda() for a in auds], win=40, hop=24, engine=eng)
    assert all(np.array_equal(bits(d["curve"]), bits(t["curve"])) and np.array_equal(d["offset"], t["offset"]) for d, t in zip(dev, line))
    assert metrics.sync_timeline([], [], engine=eng) == []
    # win = 0 is metrics.sync_offset
    off, conf, curve = metrics.sync_offset(vids, auds, max_shift=15, engine=eng)
    one = metrics.sync_timeline(vids, auds, win=0, max_shift=15, engine=eng)
    assert all(o["offset"][0] == off[i] and bits(o["conf"])[0] == bits(conf)[i] and np.array_equal(bits(o["curve"][0]), bits(curve[i])) for i, o in enumerate(one))
    # which of three tracks is in sync with the audio: track 1 is planted, the others are independent noise
    v, a = clips[9]
    rng = np.random.default_rng(12)
    tracks = [rng.standard_normal(v.shape).astype(np.float32), v, rng.standard_normal((120, 64)).astype(np.float32)]
    speaker, table = metrics.sync_speaker(tracks, a, win=40, hop=24, max_shift=15, engine=eng)
    n = S.n_windows(150, 40, 24)
    assert speaker.shape == (n,) and table.shape == (n, 3) and speaker.dtype == np.int32
    assert (speaker == 1).all(), speaker                          # (every window of the planted track is decidable: test_sync_windows_cpu)
    assert np.isnan(table[-1, 2]) and not np.isnan(table[:-1, 2]).any()            # the short track has ended before the last window (lo = 120)
    want = np.concatenate([S.windows_ref(t, a, 15, 1, 40, 24, n)[1][:, None] for t in tracks], 1)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and np.nanmax(np.abs(table - want)) < 1e-5
    sp, tb = metrics.sync_speaker([tracks[0][:5]], a[:3], win=0, max_shift=2, min_overlap=9, engine=eng)
    assert list(sp) == [-1] and np.isnan(tb).all()                 # no shift with 9 pairs: nobody
    with pytest.raises(ValueError):
        eng.sync_offset_windows(torch.zeros(4, 96), torch.zeros(4, 96), [0, 4], [0, 4])
    with pytest.raises(ValueError):
        eng.sync_offset_windows(torch.zeros(4, 64), torch.zeros(4, 64), [0, 4], [0, 4], win=5, hop=0)
    off, conf, curve, w_off, band = eng.sync_offset_windows(torch.from_numpy(v), torch.from_numpy(a), [0, 150], [0, a.shape[0]], win=40, hop=24, want_band=True)
    assert tuple(band.shape) == (150, 31) and list(w_off) == [0, n] and np.array_equal(np.isnan(band.cpu().numpy()), np.isnan(S.band_ref(v, a, 15)))


def test_sync_offset_driver_over_time(tmp_path, capsys):
    """drivers sync_offset --win / several --frames = extract_clip_feats + extract_clip_audio_feats + metrics.sync_timeline / sync_speaker"""
    from jegal_amd import drivers, metrics, synth
    from jegal_amd._lib import Engine
    from jegal_amd.gestsync import GestSync
    e = Engine(0)
    try:
        gs = GestSync(engine=e).load_state_dict(synth.gestsync_state_dict(family="gauss"))
        T = 12
        frames = synth.synth_frames(9, 2, T)
        mel = np.random.default_rng(3).standard_normal((4 * T, 80)).astype(np.float32)
        np.save(tmp_path / "a.npy", frames[0])
        np.save(tmp_path / "b.npy", frames[1][:10])
        np.save(tmp_path / "mel.npy", mel)
        base = ["--checkpoint_path_gestsync", "synthetic", "--mel", str(tmp_path / "mel.npy"), "--max_shift", "3", "--res_dir", str(tmp_path)]
        assert drivers.cmd_sync_offset(base + ["--frames", str(tmp_path / "a.npy"), "--win", "5", "--hop", "3"], engine=e, gestsync=gs) == 0
        said = capsys.readouterr().out
        assert "AV offset:" in said and "WARNING: synthetic GestSync weights" in said and "over time (win 5 hop 3" in said
        got = np.load(tmp_path / "a.sync.npz")
        vid = gs.extract_clip_feats(torch.from_numpy(frames[0]).to(e.device))[0]
        aud = gs.extract_clip_audio_feats(torch.from_numpy(mel), T)[0]
        line = metrics.sync_timeline([vid], [aud], win=5, hop=3, max_shift=3, engine=e)[0]
        off, conf, curve = metrics.sync_offset([vid], [aud], 3, engine=e)
        assert list(got["start"]) == [0, 3, 6, 9] and np.array_equal(got["offset_t"], line["offset"])
        assert np.array_equal(bits(got["conf_t"]), bits(line["conf"])) and np.array_equal(bits(got["curve_t"]), bits(line["curve"]))
        assert got["offset"] == off[0] and np.array_equal(bits(got["curve"]), bits(curve[0])) and list(got["shifts"]) == list(range(-3, 4))
        # two candidate tracks against the one mel
        assert drivers.cmd_sync_offset(base + ["--frames", str(tmp_path / "a.npy"), "--frames", str(tmp_path / "b.npy"), "--win", "5", "--hop", "3"],
                                       engine=e, gestsync=gs) == 0
        said = capsys.readouterr().out
        assert said.count("AV offset:") == 2 and "in sync:" in said
        sp = np.load(tmp_path / "sync_speaker.npz")
        assert list(sp["tracks"]) == ["a", "b"] and sp["conf"].shape == (4, 2) and sp["speaker"].shape == (4,)
        assert np.load(tmp_path / "b.sync.npz")["offset_t"].shape == (3,)
        # without --win and with one --frames: the output of before (test_gpu_gestsync_audio.py holds it to the composition)
        assert drivers.cmd_sync_offset(base + ["--frames", str(tmp_path / "a.npy")], engine=e, gestsync=gs) == 0
        assert sorted(np.load(tmp_path / "a.sync.npz").files) == ["conf", "curve", "offset", "shifts"]
    finally:
        e.close()
