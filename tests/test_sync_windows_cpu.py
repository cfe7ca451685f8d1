"""jg_sync_offset_windows without a GPU: the float64 and float32 numpy statements of its contract agree, the statement with win = 0 is
sync_offset_cases.sync_ref, the window-count rule, every planted window that tests/test_gpu_sync_windows.py runs is decidable (so that test
may demand the float64 arg-max of every window, none exempt), the checks Engine.sync_offset_windows makes before it needs a device, and the
built library's entry and kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import sync_offset_cases as C
import sync_windows_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def the_entry_exists():
    """the statements below are the contract of an entry: where the entry is missing they state nothing, and every test here fails"""
    from jegal_amd import metrics
    from jegal_amd._lib import EXPORTS, Engine
    assert "jg_sync_offset_windows" in EXPORTS and hasattr(Engine, "sync_offset_windows") and hasattr(metrics, "sync_timeline")


def test_statements_agree_and_every_planted_window_is_decidable():
    worst, n_win_total, undecided = np.inf, 0, 0
    cases = [(f"D={D} R={R} win={win} hop={hop}", S.batch(D, R), R, win, hop) for D, R in C.SWEEP for win, hop in S.WINHOP]
    p = S.DRIFT
    cases.append(("drift", [S.drift_clip()], p["R"], p["win"], p["hop"]))
    p = S.LONG
    cases.append(("long", [S.long_clip()], p["R"], p["win"], p["hop"]))
    for name, clips, R, win, hop in cases:
        for i, (v, a) in enumerate(clips):
            nw = S.n_windows(v.shape[0], win, hop)
            o64, c64, k64 = S.windows_ref(v, a, R, 1, win, hop, nw)
            o32, c32, k32 = S.windows_ref(v, a, R, 1, win, hop, nw, np.float32)
            assert np.array_equal(np.isnan(k64), np.isnan(k32)), (name, i)
            for j in range(nw):
                n_win_total += 1
                if np.isnan(k64[j]).all():          # (a window wholly behind the audio track: nothing to decide)
                    assert o64[j] == o32[j] == 0 and np.isnan(c64[j]) and np.isnan(c32[j]), (name, i, j)
                    undecided += 1
                    continue
                m = C.margin(k64[j])
                assert m >= S.MARGIN, (name, i, j, v.shape, a.shape, m)
                worst = min(worst, m)
                assert o64[j] == o32[j], (name, i, j)
                assert np.nanmax(np.abs(k64[j] - k32[j])) < 2e-6 and abs(c64[j] - c32[j]) < 4e-6, (name, i, j)
    print(f"{n_win_total} windows, {undecided} without any shift, smallest float64 margin {worst:.3e}")
    # (the windows without any shift are rows t >= Ta + R of the clips with Ta = Tv - 3 at R = 0 and 1, one row per window: all NaN by contract)
    assert undecided == 34


def test_the_statement_with_one_window_is_sync_ref():
    for D, R in ((64, 0), (64, 15), (64, 64), (1024, 15)):
        for v, a in S.batch(D, R) + C.sweep_batch(D, R)[:12]:
            o, c, k = C.sync_ref(v, a, R, 1)
            for win, hop in ((0, 1), (v.shape[0], 7), (v.shape[0] + 50, 1)):
                ow, cw, kw = S.windows_ref(v, a, R, 1, win, hop, 1)
                assert ow[0] == o and cw[0] == c and np.array_equal(kw[0], k, equal_nan=True)
    clips, R, mo = C.special_clips()["short_min_overlap"]
    for v, a in clips:
        o, c, k = C.sync_ref(v, a, R, mo)
        ow, cw, kw = S.windows_ref(v, a, R, mo, 0, 1, 1)
        assert ow[0] == o and cw[0] == c and np.array_equal(kw[0], k, equal_nan=True)


def test_the_statement_on_cases_worked_by_hand():
    e = np.eye(64, dtype=np.float32)
    # video rows e0 .. e5; audio: e0 e1 e2 at rows 1 .. 3 (shift +1), e3 e4 e5 at rows 2 .. 4 would collide: put them at shift -1 instead
    v = e[:6]
    a = np.stack([e[10], e[0], e[1], e[4], e[5], e[11], e[12]])          # rows 0 .. 2 match at +1; rows 4, 5 match at -1
    band = S.band_ref(v, a, 2)
    assert band.shape == (6, 5) and np.isnan(band[0, :2]).all() and np.isnan(band[5, 4]) and not np.isnan(band[5, 3])
    assert band[0, 3] == 1 and band[1, 3] == 1 and band[4, 1] == 1 and band[5, 1] == 1 and np.nansum(band) == 4
    o, c, k = S.windows_ref(v, a, 2, 1, 3, 3, 2)
    assert list(o) == [1, -1] and np.allclose(k[0], [0, 0, 0, 2 / 3, 0], equal_nan=False) and np.allclose(k[1], [0, 2 / 3, 0, 0, 0])
    # a window behind the track, and min_overlap: window 0 has 3 rows, shift -2 pairs only row 2
    o, c, k = S.windows_ref(v, a, 2, 2, 3, 3, 3)
    assert o[2] == 0 and np.isnan(c[2]) and np.isnan(k[2]).all() and np.isnan(k[0, 0]) and not np.isnan(k[0, 1])
    # limits
    o, c, k = S.windows_ref(e[:0], e[:3], 1, 1, 0, 1, 2)
    assert list(o) == [0, 0] and np.isnan(c).all() and np.isnan(k).all()
    o, c, k = S.windows_ref(e[:5], e[:5], 1, 1, 0, 1, 1, max_rows=4)
    assert o[0] == 0 and np.isnan(c[0])


def test_the_window_count_rule():
    from jegal_amd._lib import Engine
    for Tv in (1, 31, 33, 124, 125, 126, 150, 151, 8200):
        for win, hop in S.WINHOP + ((125, 25), (125, 1), (7, 100)):
            n = S.n_windows(Tv, win, hop)
            assert n == int(Engine.sync_window_counts([Tv], win, hop)[0])
            if not win or Tv <= win:
                assert n == 1
                continue
            assert (n - 1) * hop + win >= Tv          # the last window reaches the track's end ...
            assert (n - 2) * hop + win < Tv           # ... and the one before it does not: none is superfluous
            assert hop > win or (n - 1) * hop < Tv    # every window begins inside the track (hop > win leaves gaps: the rule counts on)
    p = S.LONG
    assert S.n_windows(p["T"], p["win"], p["hop"]) == 324


def test_drifting_clip_changes_its_offset_at_the_cut():
    p = S.DRIFT
    assert p["s"] % 32 != 0
    v, a = S.drift_clip()
    o, c, _ = S.windows_ref(v, a, p["R"], 1, p["win"], p["hop"], S.n_windows(p["Tv"], p["win"], p["hop"]))
    for j, off in enumerate(o):
        lo, hi = j * p["hop"], min(j * p["hop"] + p["win"], p["Tv"]) - 1
        if hi < p["s"]:
            assert off == p["d0"], (j, off)
        elif lo >= p["s"]:
            assert off == p["d1"], (j, off)
        else:
            assert off in (p["d0"], p["d1"]), (j, off)
    assert sum(1 for j in range(len(o)) if j * p["hop"] + p["win"] - 1 < p["s"]) >= 2 and (o == p["d1"]).sum() >= 2


def test_entries_exist_and_refuse_bad_arguments_before_they_need_a_device():
    from jegal_amd import metrics
    from jegal_amd._lib import _SIGS, EXPORTS, Engine
    assert len(_SIGS["jg_sync_offset_windows"]) == 21 and "jg_sync_offset_windows" in EXPORTS
    assert callable(metrics.sync_timeline) and callable(metrics.sync_speaker) and callable(Engine.sync_offset_windows)
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    v, a = torch.zeros(40, 64), torch.zeros(30, 64)
    good = dict(vid=v, aud=a, v_offsets=[0, 10, 40], a_offsets=[0, 12, 30], win=5, hop=2)
    bad = [dict(max_shift=65), dict(max_shift=-1), dict(min_overlap=0), dict(win=-1), dict(hop=0),
           dict(vid=torch.zeros(40, 96), aud=torch.zeros(30, 96)), dict(aud=torch.zeros(30, 128)), dict(vid=torch.zeros(40, 1088), aud=torch.zeros(30, 1088)),
           dict(a_offsets=[0, 30]),                                         # without a_of: one audio track per clip
           dict(a_of=[0, 2]), dict(a_of=[-1, 0]), dict(a_of=[0]),           # a_of outside the audio tracks / one entry per clip
           dict(v_offsets=[0, 10, 41]), dict(a_offsets=[0, 12, 31]), dict(v_offsets=[0, 0, 40]), dict(a_offsets=[0, 0, 30]),
           dict(n_windows=[3]), dict(n_windows=[0, 3]), dict(n_windows=[3, 2 ** 20 + 1])]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.sync_offset_windows(**dict(good, **kw))
    with pytest.raises(ValueError):                  # a track of more than 2^20 rows
        eng.sync_offset_windows(torch.zeros(2 ** 20 + 1, 64), a, [0, 2 ** 20 + 1], [0, 30], a_of=[0])
    if torch.cuda.is_available():
        return          # a device is present: there is no refusal to show
    x = np.zeros((4, 64), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.sync_timeline([x], [x])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.sync_speaker([x, x], x)


def test_library_exports_the_entry_and_its_kernels_do_not_spill():
    import __graft_entry__ as G
    G.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jegal_amd", "libjegal_hip.so"))
    assert hasattr(lib, "jg_sync_offset_windows")
    assert "jg_sync_offset_windows(" in open(os.path.join(ROOT, "include", "jegal_hip.h")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources()
    band = {k: v for k, v in res.items() if "sync_band_kernel" in k}
    wins = {k: v for k, v in res.items() if "sync_windows_kernel" in k}
    assert len(band) == 5 and len(wins) == 1                                 # 32 + 2R audio rows in 1..5 tiles of 32
    for name, r in list(band.items()) + list(wins.items()):
        assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds"] <= 64 * 1024, (name, r)
    # the band kernel holds what the offset kernel holds but the curve: the same parts, no more LDS
    offs = {k: v for k, v in res.items() if "sync_offset_kernel" in k}
    assert len(offs) == 5 and all(b < o for b, o in zip(sorted(v["lds"] for v in band.values()), sorted(v["lds"] for v in offs.values())))
