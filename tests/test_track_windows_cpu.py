"""jg_track_windows without a GPU: the window rule of long gesture tracks (include/jegal_hip.h) against a numpy restatement written
here, the properties that make it a cutting of a track (cores partition it in order, a core lies in its span, a span in its track),
counting mode against filling mode, and every argument error -- JG_ERR_ARG with the outputs untouched."""
import ctypes

import numpy as np
import pytest

JG_ERR_ARG = -1
I32P = ctypes.POINTER(ctypes.c_int32)
SENTINEL = -777


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    from jegal_amd._lib import load_library
    return load_library()


def restated(lengths, win, ctx):
    """The rule, restated: track of T frames -> ceil(T / win) windows, core [j win, min((j + 1) win, T)), span [max(0, j win - ctx),
    min(T, (j + 1) win + ctx)); rows global over the concatenated tracks."""
    rows, base = [], 0
    for T in lengths:
        for j in range(-(-T // win)):
            c0, c1 = j * win, min((j + 1) * win, T)
            s0, s1 = max(0, j * win - ctx), min(T, (j + 1) * win + ctx)
            rows.append((base + s0, s1 - s0, c0 - s0, c1 - c0))
        base += T
    t = np.asarray(rows, np.int32).reshape(-1, 4)
    return t, int(t[:, 1].max()) if len(t) else 0


def call(lib, offsets, n_tracks, win, ctx, cap=None, fill=True, n_ptr=True, s_ptr=True):
    """One raw call -> (rc, table, n_windows, span_max); table, n_windows and span_max start as SENTINEL."""
    off = None if offsets is None else (ctypes.c_int32 * max(len(offsets), 1))(*offsets)
    rows = 4096 if cap is None else max(cap, 1)
    table = np.full((rows, 4), SENTINEL, np.int32)
    n, s = ctypes.c_int(SENTINEL), ctypes.c_int(SENTINEL)
    rc = lib.jg_track_windows(off, n_tracks, win, ctx, table.ctypes.data_as(I32P) if fill else None, rows if cap is None else cap,
                              ctypes.byref(n) if n_ptr else None, ctypes.byref(s) if s_ptr else None)
    return rc, table, n.value, s.value


def offsets_of(lengths):
    return [0] + np.cumsum(lengths).tolist()


def check(lib, lengths, win, ctx):
    want, want_smax = restated(lengths, win, ctx)
    off = offsets_of(lengths)
    rc, _, n_count, s_count = call(lib, off, len(lengths), win, ctx, fill=False)
    assert rc == 0 and (n_count, s_count) == (len(want), want_smax), (lengths, win, ctx)
    rc, table, n, smax = call(lib, off, len(lengths), win, ctx, cap=n_count)          # a table of exactly the counted size
    assert rc == 0 and (n, smax) == (n_count, s_count)                                # counting mode agrees with filling mode
    got = table[:n]
    assert np.array_equal(got, want), (lengths, win, ctx)
    assert (table[n:] == SENTINEL).all()
    # the properties, from the table alone
    first, length, coff, clen = (got[:, i].astype(np.int64) for i in range(4))
    core0 = first + coff
    assert np.array_equal(core0, np.cumsum(clen) - clen)                              # cores partition the rows, in order
    assert int(clen.sum()) == sum(lengths) and (clen >= 1).all() and (clen <= win).all()
    assert (coff >= 0).all() and (coff + clen <= length).all()                       # a core lies inside its span
    assert (length <= win + 2 * ctx).all() and (coff <= ctx).all()
    track = np.searchsorted(np.asarray(off[1:]), core0, side="right")                # the track that holds the core
    t0, t1 = np.asarray(off)[track], np.asarray(off)[track + 1]
    assert (first >= t0).all() and (first + length <= t1).all()                      # a span lies inside its track
    assert smax == (length.max() if n else 0)
    per_track = np.bincount(track, minlength=len(lengths)) if n else np.zeros(len(lengths), int)
    assert np.array_equal(per_track, [-(-t // win) for t in lengths])                # ceil(T / win) windows; empty tracks have none


@pytest.mark.parametrize("win", [1, 2, 7, 16, 120])
def test_one_track_against_the_restatement(lib, win):
    for T in sorted({0, 1, win - 1, win, win + 1, 2 * win, 2 * win + 1}):
        for ctx in sorted({0, 1, T + 3, min(2 * win + 5, (500 - win) // 2)}):
            if win + 2 * ctx <= 500:
                check(lib, [T], win, ctx)


def test_the_limits_of_win_and_ctx(lib):
    for win, ctx in ((500, 0), (1, 0), (100, 200), (2, 249), (120, 50), (498, 1)):          # win + 2 ctx == 500 among them
        for lengths in ([0], [1], [win - 1], [win], [win + 1], [2 * win + 1], [1203], [3 * win + ctx + 1]):
            check(lib, lengths, win, ctx)


def test_fifty_mixed_tracks(lib):
    rng = np.random.default_rng(20)
    for win, ctx in ((16, 12), (120, 50), (7, 0), (1, 3), (500, 0)):
        lengths = rng.integers(0, 4 * win + 2, 50).tolist()
        lengths[3] = lengths[17] = 0
        lengths[5], lengths[6], lengths[7] = win, win + 1, win - 1
        check(lib, lengths, win, ctx)
    check(lib, [], 16, 12)                                                           # no tracks: no windows


def test_a_case_worked_by_hand(lib):
    # tracks of 5 and 3 frames, win 2, ctx 1: cores [0,2) [2,4) [4,5) | [5,7) [7,8); spans one frame wider where the track has one
    rc, table, n, smax = call(lib, [0, 5, 8], 2, 2, 1)
    assert rc == 0 and n == 5 and smax == 4
    assert table[:5].tolist() == [[0, 3, 0, 2], [1, 4, 1, 2], [3, 2, 1, 1], [5, 3, 0, 2], [6, 2, 1, 1]]
    # a track of at most win frames is one window whose span is the whole track
    rc, table, n, smax = call(lib, [0, 16], 1, 16, 12)
    assert rc == 0 and n == 1 and smax == 16 and table[0].tolist() == [0, 16, 0, 16]


def test_every_argument_error_leaves_the_outputs_untouched(lib):
    good = dict(offsets=[0, 40, 40, 57], n_tracks=3, win=16, ctx=12)
    assert call(lib, **good)[0] == 0
    bad = [dict(win=0), dict(win=-3), dict(ctx=-1), dict(win=16, ctx=243), dict(win=501, ctx=0), dict(win=2**31 - 1, ctx=2**30),
           dict(offsets=[-1, 40, 40, 57]), dict(offsets=[0, 40, 39, 57]), dict(offsets=[5, 4, 4, 4]), dict(offsets=[0, 40, 40, -57]),
           dict(n_tracks=-1), dict(offsets=None), dict(cap=4), dict(cap=0), dict(cap=-1), dict(n_ptr=False), dict(s_ptr=False)]
    for change in bad:
        rc, table, n, smax = call(lib, **{**good, **change})
        assert rc == JG_ERR_ARG, change
        assert (table == SENTINEL).all(), change
        assert n == SENTINEL and smax == SENTINEL, change
    assert call(lib, **{**good, "cap": 5})[0] == 0                                   # 3 + 0 + 2 windows fit exactly
    assert call(lib, **{**good, "cap": -1, "fill": False})[0] == 0                   # counting mode ignores cap
    rc, _, n, smax = call(lib, None, 0, 16, 12)                                      # no tracks need no offsets
    assert (rc, n, smax) == (0, 0, 0)


def test_python_layer(lib):
    from jegal_amd._lib import EXPORTS, Engine, JegalError, track_windows
    from jegal_amd.jegal import JEGAL
    for name in ("jg_track_windows", "jg_jegal_gesture_tracks", "jg_debug_span_gather", "jg_debug_core_compact"):
        assert name in EXPORTS
    for cls, names in ((Engine, ("track_windows", "jegal_gesture_tracks", "extract_gesture_track", "debug_span_gather", "debug_core_compact")),
                       (JEGAL, ("forward_gesture_tracks",))):
        for nm in names:
            assert callable(getattr(cls, nm)), (cls, nm)
    from jegal_amd.drivers import COMMANDS
    assert "embed_tracks" in COMMANDS
    lengths = [1, 7, 16, 17, 40, 41, 95]
    table, smax = Engine.track_windows(lengths, 16, 12)
    want, want_smax = restated(lengths, 16, 12)
    assert table.dtype == np.int32 and np.array_equal(table, want) and smax == want_smax == 40
    assert Engine.track_windows([1203], 120, 50)[1] == 220 and len(track_windows([1203], 120, 50)[0]) == 11
    for bad in ((0, 0), (16, -1), (400, 51)):
        with pytest.raises(JegalError) as e:
            track_windows(lengths, *bad)
        assert e.value.code == JG_ERR_ARG
    with pytest.raises(ValueError):
        track_windows([4, -1], 16, 12)
