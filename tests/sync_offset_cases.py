"""jg_sync_offset: the numpy statement of its contract (float64 = the reference, float32 = the yardstick of the error rule) and the planted
inputs of tests/test_gpu_sync_offset.py.  Imports without a GPU: tests/test_sync_offset_cpu.py checks the statements against each other
and proves every planted clip decidable.

Planted clip: video rows ~ N(0, 1), audio row t + d0 = video row t + NOISE * N(0, 1) wherever that row exists, other audio rows N(0, 1):
the cosine of a matched pair is ~ 1 / sqrt(1 + NOISE^2) = 0.89, of any other pair ~ N(0, 1 / D).
"""
import numpy as np

MAX_T = 8192
NOISE = 0.5
MARGIN = 1e-3


def sync_ref(v, a, R, min_overlap, dtype=np.float64):
    """(offset, conf, curve (2R + 1,)) of one clip as include/jegal_hip.h states them, evaluated in `dtype`."""
    v, a = np.asarray(v, dtype), np.asarray(a, dtype)
    Tv, Ta = v.shape[0], a.shape[0]
    curve = np.full(2 * R + 1, np.nan, dtype)
    if not (1 <= Tv <= MAX_T and 1 <= Ta <= MAX_T):
        return 0, dtype(np.nan), curve
    nv, na = np.linalg.norm(v, axis=1), np.linalg.norm(a, axis=1)
    for d in range(-R, R + 1):
        lo, hi = max(0, -d), min(Tv, Ta - d)
        if hi - lo < max(min_overlap, 1):
            continue
        # (row by row, not a matrix product: a pair's value must be a function of its two rows, or duplicated rows would not tie)
        dots = (v[lo:hi] * a[lo + d:hi + d]).sum(axis=1, dtype=dtype)
        cos = dots / np.maximum(nv[lo:hi] * na[lo + d:hi + d], dtype(1e-8))
        curve[d + R] = cos.sum(dtype=dtype) / dtype(hi - lo)
    if np.isnan(curve).all():
        return 0, dtype(np.nan), curve
    return int(np.nanargmax(curve)) - R, dtype(np.nanmax(curve) - np.nanmedian(curve)), curve


def margin(curve):
    """float64 distance from the best shift to the best shift that is not EXACTLY equal to it (inf when there is none): duplicated rows
    make shifts bit-equal on purpose, and then the first one wins by contract."""
    c = curve[~np.isnan(curve)]
    if c.size == 0:
        return np.inf
    rest = c[c != c.max()]
    return np.inf if rest.size == 0 else float(c.max() - rest.max())


def planted(rng, D, Tv, Ta, d0):
    """d0 is clipped to the shifts for which the clip has a pair at all (-(Tv - 1) .. Ta - 1): a clip shorter than the shift asked for
    is planted at its farthest shift, where one pair matches."""
    d0 = int(np.clip(d0, -(Tv - 1), Ta - 1))
    v = rng.standard_normal((Tv, D)).astype(np.float32)
    a = rng.standard_normal((Ta, D)).astype(np.float32)
    t = np.arange(Tv)
    ok = (t + d0 >= 0) & (t + d0 < Ta)
    a[t[ok] + d0] = v[t[ok]] + NOISE * rng.standard_normal((int(ok.sum()), D)).astype(np.float32)
    return v, a


TV = (1, 31, 33, 150)
SWEEP = [(D, R) for D in (64, 1024) for R in (0, 1, 15, 64)]


def sweep_batch(D, R):
    """37 clips: Tv in TV x Ta - Tv in (0, +3, -3) x d0 in (-R, 0, R) (Ta >= 1; R = 0: d0 = 0 three times over, other seeds), filled up
    with clips of 64 rows (whole row blocks)."""
    rng = np.random.default_rng(1000 * D + R)
    clips = []
    for Tv in TV:
        for dT in (0, 3, -3):
            if Tv + dT < 1:
                continue
            for d0 in (-R, 0, R):
                clips.append(planted(rng, D, Tv, Tv + dT, d0))
    while len(clips) < 37:
        clips.append(planted(rng, D, 64, 64, (len(clips) % 3 - 1) * min(R, 7)))
    return clips[:37]


def special_clips():
    """name -> (clips, R, min_overlap), D = 64."""
    rng = np.random.default_rng(77)
    D = 64
    out = {}
    # Tv < R: min_overlap cuts the far shifts to NaN
    out["short_min_overlap"] = ([planted(rng, D, 5, 5, 1), planted(rng, D, 9, 12, -2)], 15, 3)
    # min_overlap larger than any overlap: no shift at all
    out["no_shift"] = ([planted(rng, D, 5, 5, 0), planted(rng, D, 4, 40, 3)], 15, 6)
    # a zero video row and a zero audio row: cosine 0 by the 1e-8 floor
    v, a = planted(rng, D, 40, 43, 2)
    v[7] = 0
    a[20] = 0
    out["zero_rows"] = ([(v, a)], 15, 1)
    # duplicated rows: audio rows of period 2 make shifts d and d + 2 bit-equal; shifts 0 and 2 are the maximum, 0 wins
    base = rng.standard_normal((2, D)).astype(np.float32)
    v = base[np.arange(6) % 2] + 0.25 * rng.standard_normal((6, D)).astype(np.float32)
    a = base[np.arange(12) % 2].copy()
    out["duplicates"] = ([(v, a)], 3, 6)
    # an oversized clip and an empty clip between good ones
    big = (rng.standard_normal((MAX_T + 1, D)).astype(np.float32), rng.standard_normal((40, D)).astype(np.float32))
    empty = (np.zeros((0, D), np.float32), rng.standard_normal((8, D)).astype(np.float32))
    empty_a = (rng.standard_normal((8, D)).astype(np.float32), np.zeros((0, D), np.float32))
    out["oversized_empty"] = ([planted(rng, D, 33, 33, 4), big, planted(rng, D, 31, 34, -4), empty, empty_a, planted(rng, D, 150, 147, 15)], 15, 1)
    return out
