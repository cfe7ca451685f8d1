"""Cases, float64 references and derived bounds for the two kernels of GestSync's audio stream (jegal_amd/csrc/gsa_kernels.hip).

Imports without a GPU: tests/test_gpu_gestsync_audio.py feeds the cases to jg_debug_gsa_conv1_pool / jg_debug_maxpool_2x3,
tests/test_gestsync_audio_cases_cpu.py feeds them to torch-float32 stand-ins and to planted defects.

conv1 + BatchNorm + ReLU + max-pool: a conv output is sum of nine fp32 products plus the shift; the kernel is documented to compute it as
one fmaf chain in fp32, so it errs by at most ~10 u times the sum of the magnitudes of its ten terms (u = 2^-24; nine roundings and
the add).  max and ReLU are 1-Lipschitz, so a pooled output errs by at most the largest bound among its nine conv outputs; an fp16
output adds one fp16 ulp of the reference.  The bound comes from this arithmetic, never from what the kernel returned.
The max-pool is exact: its output is one of its six inputs.
"""
import numpy as np
import torch

U = 2.0 ** -24
H, W, PH, PW, C = 80, 100, 19, 24, 64


def weights(seed=5):
    g = np.random.default_rng(seed)
    return (0.3 * g.standard_normal((C, 9))).astype(np.float32), (0.5 * g.standard_normal(C)).astype(np.float32)


def gather_windows(mel, T, valid=None):
    """The documented gather of the clip form: mel (B, Tm, 80) -> x (B T, 1, 80, 100), window t of clip b = mel rows
    clamp(4 (t - 12) + w, 0, valid[b] - 1), w = 0..99, transposed to (band, step)."""
    B, Tm, _ = mel.shape
    x = np.empty((B * T, 1, H, W), mel.dtype)
    for b in range(B):
        vt = Tm if valid is None else int(valid[b])
        for t in range(T):
            rows = np.clip(4 * (t - 12) + np.arange(W), 0, vt - 1)
            x[b * T + t, 0] = mel[b, rows].T
    return x


def conv1_pool_ref(x, w, shift):
    """x (N, 1, 80, 100) -> (reference (N, 19, 24, 64) float64 NHWC, bound of the same shape: 10 u sum |terms| of the worst conv output
    under each pooled one).  Conv rows 0..38 and columns 0..48 only: the pool reads no other."""
    x = np.asarray(x, np.float64)[:, 0]
    N = x.shape[0]
    xp = np.zeros((N, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    w64, s64 = np.asarray(w, np.float64).reshape(C, 3, 3), np.asarray(shift, np.float64)
    conv = np.zeros((N, 39, 49, C))
    mag = np.zeros((N, 39, 49, C))
    for kh in range(3):
        for kw in range(3):
            patch = xp[:, kh:kh + 77:2, kw:kw + 97:2]                         # rows 2r + kh, r < 39; columns 2q + kw, q < 49
            term = patch[..., None] * w64[None, None, None, :, kh, kw]
            conv += term
            mag += np.abs(term)
    conv += s64
    mag += np.abs(s64)
    ref = np.full((N, PH, PW, C), -np.inf)
    bound = np.zeros((N, PH, PW, C))
    for i in range(3):
        for j in range(3):
            ref = np.maximum(ref, conv[:, i:i + 37:2, j:j + 47:2])
            bound = np.maximum(bound, mag[:, i:i + 37:2, j:j + 47:2])
    return np.maximum(ref, 0.0), 10 * U * bound


def ulp16(ref):
    """one fp16 ulp at |ref| (normal range; 2^-24 below it)"""
    a = np.maximum(np.abs(ref), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def window_cases(seed=11):
    """x (N, 1, 80, 100): random windows, a constant window, and one window per corner with a lone non-zero value there (the two corners
    on band 79 / step 99 lie outside what the computed outputs read: those windows must come out as an all-zero input does)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((8, 1, H, W)).astype(np.float32)
    x[3] = np.float32(1.75)
    x[4:8] = 0
    for n, (h, w_) in zip(range(4, 8), ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        x[n, 0, h, w_] = np.float32(-3.5 if n % 2 else 2.5)
    return x


def clip_cases(seed=12):
    """[(mel (B, Tm, 80), T, valid or None)]: windows that start before row 0 (every t < 12 does) and windows that end past valid / Tm"""
    g = np.random.default_rng(seed)
    return [(g.standard_normal((2, 37, H)).astype(np.float32), 9, None),
            (g.standard_normal((2, 100, H)).astype(np.float32), 9, (100, 23)),
            (g.standard_normal((3, 60, H)).astype(np.float32), 14, (1, 60, 17))]


POOL_SHAPES = [(9, 5), (2, 3), (3, 4), (8, 7)]
POOL_C = (8, 256)


def pool_case(Hi, Wi, Ci, dtype, nimg=3, seed=13):
    g = torch.Generator().manual_seed(seed * 1000 + Hi * 100 + Wi * 10 + Ci)
    return (4 * torch.randn((nimg, Hi, Wi, Ci), generator=g)).to(dtype)


def pool_ref(x):
    """(nimg, H, W, C) -> (nimg, (H - 2) // 2 + 1, (W - 3) // 2 + 1, C): window (2, 3), stride (2, 2), exact in the input's type"""
    n, Hi, Wi, Ci = x.shape
    OH, OW = (Hi - 2) // 2 + 1, (Wi - 3) // 2 + 1
    out = torch.full((n, OH, OW, Ci), float("-inf"), dtype=torch.float64)
    for i in range(2):
        for j in range(3):
            out = torch.maximum(out, x[:, i:i + 2 * OH - 1:2, j:j + 2 * OW - 1:2].double())
    return out.to(x.dtype)
