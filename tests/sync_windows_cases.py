"""jg_sync_offset_windows: the numpy statement of its contract (float64 = the reference, float32 = the yardstick of the error rule) and the
planted inputs of tests/test_gpu_sync_windows.py.  Imports without a GPU: tests/test_sync_windows_cpu.py checks the statements against
each other and against sync_offset_cases.sync_ref, and proves every planted window decidable.

The clips are sync_offset_cases.planted ones.  A window that holds no planted pair (the clip's tail when the planted shift points behind
the audio track's end) sees only chance cosines ~ N(0, 1 / D), and its two best shifts can come closer than MARGIN: the seeds of SEEDS
are the first of 0, 1, 2, ... for which EVERY window of EVERY (win, hop) of WINHOP has a float64 margin >= MARGIN, found with the float64
statement alone, never with the kernels (`python tests/sync_windows_cases.py` prints the table again)."""
import numpy as np

import sync_offset_cases as C

MAX_ROWS = 1 << 20
MARGIN = C.MARGIN
WINHOP = ((0, 1), (1, 1), (40, 24), (32, 32), (200, 50))


def n_windows(Tv, win, hop):
    """the windows that cover a track of Tv rows"""
    if not win or Tv <= win:
        return 1
    return -(-(Tv - win) // hop) + 1


def band_ref(v, a, R, dtype=np.float64):
    """band (Tv, 2R + 1): the cosine of video row t and audio row t + d at [t][d + R], NaN where t + d is outside the audio track; each entry
    from its two rows alone, evaluated row by row as sync_offset_cases.sync_ref does."""
    v, a = np.asarray(v, dtype), np.asarray(a, dtype)
    Tv, Ta = v.shape[0], a.shape[0]
    band = np.full((Tv, 2 * R + 1), np.nan, dtype)
    nv, na = np.linalg.norm(v, axis=1), np.linalg.norm(a, axis=1)
    for d in range(-R, R + 1):
        lo, hi = max(0, -d), min(Tv, Ta - d)
        if hi <= lo:
            continue
        dots = (v[lo:hi] * a[lo + d:hi + d]).sum(axis=1, dtype=dtype)
        band[lo:hi, d + R] = dots / np.maximum(nv[lo:hi] * na[lo + d:hi + d], dtype(1e-8))
    return band


def decide(curve, R, dtype):
    if np.isnan(curve).all():
        return 0, dtype(np.nan)
    return int(np.nanargmax(curve)) - R, dtype(np.nanmax(curve) - np.nanmedian(curve))


def windows_ref(v, a, R, min_overlap, win, hop, n_win, dtype=np.float64, band=None, max_rows=MAX_ROWS):
    """(offset (n_win,) int32, conf (n_win,), curve (n_win, 2R + 1)) of one clip as include/jegal_hip.h states them, evaluated in `dtype`.
    band: band_ref(v, a, R, dtype) if the caller has it already."""
    Tv, Ta = np.shape(v)[0], np.shape(a)[0]
    W = 2 * R + 1
    off, conf, curve = np.zeros(n_win, np.int32), np.full(n_win, np.nan, dtype), np.full((n_win, W), np.nan, dtype)
    if not (1 <= Tv <= max_rows and 1 <= Ta <= max_rows):
        return off, conf, curve
    if band is None:
        band = band_ref(v, a, R, dtype)
    need = max(min_overlap, 1)
    for j in range(n_win):
        lo = j * hop if win else 0
        hi = min(lo + win, Tv) if win else Tv
        if lo >= Tv:
            continue
        for d in range(-R, R + 1):
            t_lo, t_hi = max(lo, -d), min(hi, Ta - d)
            if t_hi - t_lo < need:
                continue
            # (a contiguous copy: the sum sync_ref takes of its cosines, bit for bit)
            curve[j, d + R] = np.ascontiguousarray(band[t_lo:t_hi, d + R]).sum(dtype=dtype) / dtype(t_hi - t_lo)
        off[j], conf[j] = decide(curve[j], R, dtype)
    return off, conf, curve


def drifting(rng, D, Tv, Ta, s, d0, d1):
    """planted at d0 up to frame s and at d1 from it on: two planted clips joined"""
    v0, a0 = C.planted(rng, D, Tv, Ta, d0)
    v1, a1 = C.planted(rng, D, Tv, Ta, d1)
    v = np.concatenate([v0[:s], v1[s:]])
    a = a0.copy()
    t = np.arange(s, Tv)
    ok = (t + d1 >= 0) & (t + d1 < Ta)
    a[t[ok] + d1] = a1[t[ok] + d1]
    return v, a


DRIFT = dict(D=64, R=15, Tv=150, Ta=150, s=70, d0=-3, d1=4, win=40, hop=12, seed=5)
LONG = dict(D=64, R=15, T=8200, d0=6, win=125, hop=25, seed=11)


def drift_clip():
    p = DRIFT
    return drifting(np.random.default_rng(p["seed"]), p["D"], p["Tv"], p["Ta"], p["s"], p["d0"], p["d1"])


def long_clip():
    p = LONG
    return C.planted(np.random.default_rng(p["seed"]), p["D"], p["T"], p["T"], p["d0"])


def shapes(R):
    """(Tv, Ta, d0) of the 11 clips of a batch: Tv in 1, 31, 33, 150 x Ta - Tv in 0, +3, -3 (Ta >= 1), planted at -R, 0, R in turn"""
    out = []
    for Tv in C.TV:
        for dT in (0, 3, -3):
            if Tv + dT >= 1:
                out.append((Tv, Tv + dT, (-R, 0, R)[len(out) % 3]))
    return out


def clip_margin(v, a, R):
    """the smallest float64 margin over every window of every (win, hop) of WINHOP"""
    band = band_ref(v, a, R)
    worst = np.inf
    for win, hop in WINHOP:
        _, _, curve = windows_ref(v, a, R, 1, win, hop, n_windows(v.shape[0], win, hop), band=band)
        worst = min([worst] + [C.margin(c) for c in curve])
    return worst


def find_seed(D, R, i, Tv, Ta, d0):
    for s in range(1000):
        v, a = C.planted(np.random.default_rng([D, R, i, s]), D, Tv, Ta, d0)
        if clip_margin(v, a, R) >= MARGIN:
            return s
    raise RuntimeError("no seed")


#: (D, R) -> the seed of each of the 11 clips of shapes(R)
SEEDS = {
    (64, 0): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (64, 1): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (64, 15): (0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    (64, 64): (0, 0, 0, 0, 0, 0, 4, 0, 3, 1, 0),
    (1024, 0): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (1024, 1): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (1024, 15): (0, 0, 3, 0, 1, 0, 3, 0, 0, 1, 0),
    (1024, 64): (0, 0, 1, 0, 0, 13, 2, 0, 22, 252, 0),
}


def batch(D, R):
    return [C.planted(np.random.default_rng([D, R, i, s]), D, Tv, Ta, d0) for i, ((Tv, Ta, d0), s) in enumerate(zip(shapes(R), SEEDS[(D, R)]))]


if __name__ == "__main__":
    for D, R in C.SWEEP:
        print(f"    ({D}, {R}): {tuple(find_seed(D, R, i, *s) for i, s in enumerate(shapes(R)))},")
