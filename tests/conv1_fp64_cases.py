"""Operands, inputs, float64 reference, bounds and expected bits for the kernel-level checks of conv1 + BatchNorm + ReLU + max-pool
(tests/test_gpu_conv1_fp64.py runs them on the GPU, tests/test_conv1_cases_cpu.py checks this module without one).  No GPU code here.

The operation (gestsync.py:36-46): Conv3d(3 -> 64, k (5,7,7), s (1,3,3)) + BatchNorm(eval) + ReLU + MaxPool3d((1,3,3), (1,2,2)) of a
clip of T u8 frames (270 x 480 x 3) that is replicate-padded by `pad` frames at both ends: P = T + 2 pad - 4 positions per clip, position
p reads frames clamp(p + dt - pad, 0, T - 1), dt = 0..4, of ITS clip.  Output: pooled NHWC (B P, 43, 78, 64).

Operands that reach every kernel exactly (make_conv folds the BN scale s = g / sqrt(var + 1e-5f) in fp32, pack_matrix rounds to fp16 to
the nearest or with error diffusion, or to bf16):
  conv1.weight   m 2^-10, integer |m| <= 64, drawn independently per (out, in, kt, kh, kw)
  bn1.running_var 1, bn1.weight 2^k float32(sqrt(float32(1) + float32(1e-5))), k in -2..2 per channel: s = 2^k exactly
  conv1.bias, bn1.running_mean, bn1.bias   multiples of 2^-8 with |shift| <= 2, shift = (b - mu) s + be: every step exact in fp32
The folded weights w = m 2^(k-10) are exact in fp16 and bf16; 255 shift has up to 19 bits, so the hi+lo fp16 pair that carries the bias
through the direct kernel's GEMM (255 shift 2^-10, against a pad lane of 2^-14: shared.h) has a non-zero lo half in almost every
channel, and hi + lo == 255 shift 2^-10 exactly.
With u8 pixels n every product w n and every partial sum, in every order, is an integer below 2^24 in the channel's unit 2^(k-10)
(735 * 64 * 255 + 255 * 2 * 2^12 < 2^24): float64 evaluates the sum exactly and an fp32 accumulator has nothing to round.

Reference (float64, CPU): per distinct (frame, dt) one conv2d(frame, w[:, :, dt], stride 3); a position sums its five terms;
r = sum / 255 + shift; ReLU; max_pool2d(3, 2).  The same with |w| and |shift| gives the magnitudes S.

Tier A (every path):    |got - ref| <= maxpool(2 K u S) + 1 ulp16(ref), K = 737 (735 taps + the bias pair), u = 2^-24 -- the rule of
                        test_gpu_kernels_fp64.py; max-pool is 1-Lipschitz in the max norm, so the pooled bound is the pool of the bounds.
Tier B (direct kernel): the bits.  The kernel computes f16(max(fl32(A c), 0)) and then maxima of fp16 values, A = the exact sum
                        including 255 shift, c = float32(1.0f / 255.0f) (the powers of two in the launcher's scale and in the loader's
                        subnormals cancel exactly).  Over an all-zero patch that is f16(relu(fl32(255 shift c))): the constant of skipped tiles.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

IH, IW = 270, 480
CH, CW = 88, 158                    # conv rows / columns
PH, PW, OC = 43, 78, 64             # pooled rows / columns, channels
FRAME_BYTES = IH * IW * 3
ROW_BYTES = IW * 3
ROW_TILES, COL_TILES = 22, 5        # conv1_direct_kernel: tile rt reads the input band of rows 12 rt .. 12 rt + 15; 5 strips of 32 conv columns
K_TERMS = 737
U = 2.0 ** -24
C255 = np.float32(1.0) / np.float32(255.0)
MAX_PAD = 12

# ---- shapes (B, T, pad) -----------------------------------------------------------------------------------------------------------------
SHAPES = {
    "b1t1p2": (1, 1, 2),      # all five frames are frame 0; fewer strips than XCD ranges
    "b1t5p0": (1, 5, 0),      # no clamping at all
    "b2t2p2": (2, 2, 2),      # clip boundary inside the launch; per = 3, the last XCD ranges short or empty
    "b1t3p4": (1, 3, 4),      # every clamp pattern of a 3-frame clip; P = 7
    "b1t5p2": (1, 5, 2),      # P = 5, 25 strips: ranges of 4, the last one 1 strip long
    "b3t2p12": (3, 2, 12),    # 330 strips: more than CUs; P = 22; pad at the entry's limit
}
ZERO_FAMILIES = ("mask", "mask_jitter", "middle", "bottom", "black", "lone_byte_first", "lone_byte_last", "lone_byte_1424", "lone_byte_bandend",
                 "unread_rows")
ZERO_SHAPES = ("b1t3p4", "b3t2p12")
CASES = [(s, "dense") for s in SHAPES] + [(s, f) for s in ZERO_SHAPES for f in ZERO_FAMILIES]


def case_id(case):
    return f"{case[0]}-{case[1]}"


def positions(T, pad):
    return T + 2 * pad - 4


def frame_of(p, dt, T, pad):
    return min(max(p + dt - pad, 0), T - 1)


def clamp_patterns(T, pad):
    """The set of frame 5-tuples the positions of one clip read."""
    return {tuple(frame_of(p, dt, T, pad) for dt in range(5)) for p in range(positions(T, pad))}


def strips(B, T, pad):
    return B * positions(T, pad) * COL_TILES


def xcd_ranges(nstrips):
    """conv1_strips (conv1.hip): XCD x owns strips [x per, min((x + 1) per, nstrips)), per = ceil(nstrips / 8) -> lengths (0 for none)."""
    per = (nstrips + 7) >> 3
    return per, [max(min((x + 1) * per, nstrips) - x * per, 0) for x in range(8)]


def check_shape_properties(num_cu=None):
    """What the table of shapes promises of each; num_cu: the device's CU count where there is a device."""
    assert clamp_patterns(1, 2) == {(0,) * 5} and strips(1, 1, 2) == 5 and xcd_ranges(5)[1] == [1] * 5 + [0] * 3
    assert clamp_patterns(5, 0) == {(0, 1, 2, 3, 4)} and strips(1, 5, 0) == 5
    assert strips(2, 2, 2) == 20 and xcd_ranges(20) == (3, [3] * 6 + [2, 0])
    assert clamp_patterns(2, 2) == {(0, 0, 0, 1, 1), (0, 0, 1, 1, 1)}          # every position clamps at both ends of its 2-frame clip
    # a 3-frame clip: every monotone 5-tuple over {0,1,2} with steps <= 1 that the clamp can produce
    want = {(0, 0, 0, 0, 0), (0, 0, 0, 0, 1), (0, 0, 0, 1, 2), (0, 0, 1, 2, 2), (0, 1, 2, 2, 2), (1, 2, 2, 2, 2), (2, 2, 2, 2, 2)}
    assert clamp_patterns(3, 4) == want and positions(3, 4) == 7 and strips(1, 3, 4) == 35
    assert float(np.float32(1) / np.float32(7)) * 7 != 1.0                                         # decode()'s float32 1 / P is inexact
    assert positions(5, 2) == 5 and strips(1, 5, 2) == 25 and xcd_ranges(25) == (4, [4] * 6 + [1, 0])
    assert positions(2, 12) == 22 and strips(3, 2, 12) == 330 and SHAPES["b3t2p12"][2] == MAX_PAD
    if num_cu is not None:
        assert 330 > num_cu, "b3t2p12 must have more strips than the device has CUs (several strips per workgroup)"


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(seed=1):
    """-> dict: sd (the six net_vid.conv1.* / bn1.* tensors, float32 numpy), w (64,3,5,7,7) and shift (64) as float64 torch, k (64) int."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-64, 65, (OC, 3, 5, 7, 7))
    k = rng.integers(-2, 3, OC)
    b, mu = rng.integers(-32, 33, OC), rng.integers(-32, 33, OC)          # multiples of 2^-8 in [-1/8, 1/8]
    be = rng.integers(-256, 257, OC)                                      # ... in [-1, 1]
    q = np.sqrt(np.float32(1) + np.float32(1e-5)).astype(np.float32)
    sd = {
        "net_vid.conv1.weight": (m * 2.0 ** -10).astype(np.float32),
        "net_vid.conv1.bias": (b * 2.0 ** -8).astype(np.float32),
        "net_vid.bn1.weight": (np.float32(2.0) ** k.astype(np.float32) * q).astype(np.float32),
        "net_vid.bn1.bias": (be * 2.0 ** -8).astype(np.float32),
        "net_vid.bn1.running_mean": (mu * 2.0 ** -8).astype(np.float32),
        "net_vid.bn1.running_var": np.ones(OC, np.float32),
    }
    s = 2.0 ** k
    shift = (b - mu) * 2.0 ** -8 * s + be * 2.0 ** -8
    w = m * 2.0 ** -10 * s[:, None, None, None, None]
    return dict(sd=sd, w=torch.from_numpy(w), shift=torch.from_numpy(shift), k=k, unit=torch.from_numpy(2.0 ** (k - 10.0)))


def folded_fp32(sd):
    """make_conv's BN fold (linear.hip) in numpy float32 -> (s, shift); `contract`-proof: every step is exact for operands()."""
    g, var, b, mu, be = (sd["net_vid." + n] for n in ("bn1.weight", "bn1.running_var", "conv1.bias", "bn1.running_mean", "bn1.bias"))
    s = g / np.sqrt(var + np.float32(1e-5))
    assert s.dtype == np.float32
    return s, ((b - mu) * s + be).astype(np.float32)


def bias_pair(shift):
    """finalize_gestsync's hi+lo fp16 pair of 255 shift 2^-10 (CONV1_BIAS_PAIR_SCALE, shared.h), as float64: (v, hi, lo)."""
    v = shift.float() * np.float32(255.0) * np.float32(2.0 ** -10)
    hi = v.half()
    lo = (v - hi.float()).half()
    return v.double(), hi.double(), lo.double()


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
def probe_byte(r):
    """conv1_zero_scan_kernel's step 1 reads bytes [probe, probe + 16) of row r."""
    return ((r * 37) % 90) * 16


LONE = {    # variant -> (row, byte of the row); all rows are blanked by `mask` (< 110) and the byte lies outside the row's probe
    "lone_byte_first": (30, 0),            # byte 0: pixel 0, channel 0
    "lone_byte_last": (60, ROW_BYTES - 1),  # byte 1439: pixel 479, which no conv window reads (conv column 157 ends at pixel 477)
    "lone_byte_1424": (61, 1424),          # pixel 474, channel 2: the last pixel a pooled output reads; the last 16 bytes of the scan's row read
    "lone_byte_bandend": (51, 700),        # row 12 * 3 + 15: the last row of band 3 (and row 3 of band 4)
}
LONE_FRAME = 1                             # frame 1 of clip 0


def make_frames(shape, family):
    """(B, T, 270, 480, 3) u8, every byte uniform and independent, then the family's rows blanked."""
    B, T, pad = SHAPES[shape]
    rng = np.random.default_rng(sum(map(ord, shape)) * 7 + 3)
    x = rng.integers(0, 256, (B, T, IH, IW, 3), dtype=np.uint8)
    if family == "dense":
        pass
    elif family == "mask" or family in LONE:
        x[:, :, :110] = 0                                      # tiles 0..7 skipped, tile 8 (rows 96..111) partial
        if family in LONE:
            r, c = LONE[family]
            assert r < 110 and not probe_byte(r) <= c < probe_byte(r) + 16
            x[0, LONE_FRAME % T].reshape(IH, ROW_BYTES)[r, c] = 1
    elif family == "mask_jitter":
        for i in range(B * T):
            x[i // T, i % T, :(96, 110, 124)[i % 3]] = 0
    elif family == "middle":
        x[:, :, 120:168] = 0                                   # bands 10..12 zero under a non-zero band 9
    elif family in ("bottom", "unread_rows"):
        x[:, :, 200:] = 0
        if family == "unread_rows":
            x[:, :, 268:] = rng.integers(1, 256, (B, T, 2, IW, 3), dtype=np.uint8)      # no conv window reads rows 268, 269; no band holds them
    elif family == "black":
        x[min(1, B - 1)] = 0
    else:
        raise KeyError(family)
    return torch.from_numpy(x)


def zero_bands(frames):
    """(B, T) -> 22-bit masks as the scan should find them: bit rt = rows 12 rt .. 12 rt + 15 of the frame are zero."""
    rows = (frames.reshape(*frames.shape[:2], IH, -1) != 0).any(-1)
    return [[sum(1 << rt for rt in range(ROW_TILES) if not bool(rows[b, t, 12 * rt:12 * rt + 16].any())) for t in range(frames.shape[1])]
            for b in range(frames.shape[0])]


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def ulp16(x, bf=False):
    mant, lo = (7, -133) if bf else (10, -24)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -60)))
    return torch.exp2((e - mant).clamp_min(lo))


def _nhwc(t):
    return t.permute(1, 2, 0).contiguous()


def epilogue(val, mag, ops):
    """Exact sums (64, 88, 158) of one position -> ref, bound core (both pooled, float64), expected bits (int16), max |partial sum| in
    units, whether the sum including 255 shift is an fp32 value; all NHWC (43, 78, 64)."""
    shift = ops["shift"][:, None, None]
    A = val + 255.0 * shift                                           # exact: integers below 2^24 in the channel's unit
    units = float(((mag + 255.0 * shift.abs()) / ops["unit"][:, None, None]).max())
    fp32_exact = bool((A.float().double() == A).all())
    ref = F.max_pool2d((val / 255.0 + shift).clamp_min(0)[None], 3, 2)[0]
    core = F.max_pool2d((2 * K_TERMS * U * (mag / 255.0 + shift.abs()))[None], 3, 2)[0]
    x16 = (A.float() * torch.tensor(C255)).clamp_min(0).half()
    bits = F.max_pool2d(x16.float()[None], 3, 2)[0].half().view(torch.int16)
    return _nhwc(ref), _nhwc(core), _nhwc(bits), units, fp32_exact


def reference(frames, pad, ops=None):
    """-> dict(ref, core: float64 (B P, 43, 78, 64); bits: int16; units: max |partial sum| bound in units; fp32_exact)."""
    ops = ops or operands()
    B, T = frames.shape[:2]
    P = positions(T, pad)
    w = ops["w"]
    wk = torch.cat([w, w.abs()], 0).permute(2, 0, 1, 3, 4).reshape(5 * 2 * OC, 3, 7, 7)          # [dt][value | magnitude][in][kh][kw]
    ref = torch.empty((B * P, PH, PW, OC), dtype=torch.float64)
    core = torch.empty_like(ref)
    bits = torch.empty((B * P, PH, PW, OC), dtype=torch.int16)
    units, exact = 0.0, True
    for b in range(B):
        x = frames[b].permute(0, 3, 1, 2).double()
        per = [F.conv2d(x[t:t + 1], wk, stride=3)[0].view(5, 2 * OC, CH, CW) for t in range(T)]
        seen = {}
        for p in range(P):
            fs = tuple(frame_of(p, dt, T, pad) for dt in range(5))
            if fs not in seen:
                s = per[fs[0]][0] + per[fs[1]][1] + per[fs[2]][2] + per[fs[3]][3] + per[fs[4]][4]
                seen[fs] = epilogue(s[:OC], s[OC:], ops)
            r, c, bi, un, ex = seen[fs]
            ref[b * P + p], core[b * P + p], bits[b * P + p] = r, c, bi
            units, exact = max(units, un), exact and ex
    return dict(ref=ref, core=core, bits=bits, units=units, fp32_exact=exact)


def bound(d, bf=False):
    return d["core"] + ulp16(d["ref"], bf)


_CASE = {}


def case_data(case):
    """frames + reference of one case; those of the small shapes are kept for the session and shared between the tests that need them
    (a case of b3t2p12 holds 250 MB and is used by one test)."""
    if case in _CASE:
        return _CASE[case]
    shape, family = case
    frames = make_frames(shape, family)
    d = reference(frames, SHAPES[shape][2])
    d["frames"] = frames
    if d["ref"].shape[0] <= 8:
        _CASE[case] = d
    return d


def zero_patch_bits(ops=None):
    """f16(relu(fl32(255 shift c))) per channel (int16): every output over an all-zero patch."""
    ops = ops or operands()
    return ((255.0 * ops["shift"]).float() * torch.tensor(C255)).clamp_min(0).half().view(torch.int16)


def correctly_rounded_share(got16, ref, bf=False):
    """share of 16-bit outputs equal to the float64 reference rounded to the output type"""
    return float((got16.double() == ref.to(torch.bfloat16 if bf else torch.float16).double()).double().mean())


def describe_mismatch(ne):
    """Where a (N, 43, 78, 64) bool mask of differing elements sits: counts per position, pooled row, pooled column and channel group."""
    n = int(ne.sum())
    if n == 0:
        return "no mismatch"

    def top(dim, div=1):
        other = [d for d in range(4) if d != dim]
        c = ne.sum(other)
        if div > 1:
            c = c.view(-1, div).sum(1)
        idx = torch.argsort(c, descending=True)[:8]
        return f"{int((c > 0).sum())} of {c.numel()} hit, top " + " ".join(f"{int(i)}:{int(c[i])}" for i in idx if c[i] > 0)
    return (f"{n} of {ne.numel()} ({n / ne.numel():.4%}) differ | positions: {top(0)} | pooled rows: {top(1)} | pooled columns: {top(2)} | "
            f"channel groups of 8: {top(3, 8)}")
