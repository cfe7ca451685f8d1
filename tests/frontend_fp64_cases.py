"""Cases, float64 references and derived bounds for the front-end entries jg_logmel and jg_mask_resize[_packed] (jegal_amd/csrc/elementwise_f32.hip).

Imports without a GPU: tests/test_gpu_frontend_fp64.py feeds the cases to the public C ABI, tests/test_frontend_cases_cpu.py feeds them to a float32
numpy restatement of logmel_kernel and to planted defects.  u = 2^-24.

logmel.  Reference, float64 throughout: the signal reflect-padded by 256 samples, frame t = samples 160 t .. 160 t + 511 of it times a periodic
Hann(320) centred in 512 (offset 96), np.fft.rfft, the last of the 1 + n // 160 frames dropped, |X|, m64 = B |X| with the float32 basis B the
kernel receives.  The comparison is in the LINEAR mel domain, got_lin = exp(out) - 1e-20 in float64 -- in the log domain a quiet bin says
nothing about the arithmetic (its value is cancellation noise far below the bound of the loud bins next to it):

    |got_lin - m64| <= delta[t, m] = (sum_f B[m, f]) sqrt(2) (512 + c1) u sum_n |seg_t[n]|  +  (257 + c2 + |log M|) u M,     M = m64 + 1e-20

  first term, re and im of a bin (each; the magnitude of the error vector is sqrt(2) times that), in units of u sum_n |seg_t[n]|:
        512 terms accumulated in sequence                                                                             511
        a twiddle: the angle 2 pi n / 512 in fp32 (constant, product: <= 1.5 u of <= 2 pi = 9.4 u), sincosf <= 2 u, the product 1 u      12.4
        the window: the angle as above for 2 pi k / 320 (15.7 u with its two roundings), cosf 2 u, halved, two more roundings: |w^ - w| <= 10.4 u
        ABSOLUTELY, + 1 u for seg = w x.  The absolute part is 10.4 u |x_n|; it is counted against |seg| = w |x| through
        sum_{0 < w} |x_n| <= WIN_RATIO sum_n |seg_t[n]| with WIN_RATIO = 4, which the generator asserts for every frame of every signal
        (a flat envelope gives 2; w(96) = 0 exactly in both arithmetics, cos 0 = 1)                                    42.6
    => c1 = 56.
  second term, relative to M: mag = sqrtf(re^2 + im^2) 3 u; the mel sum: 257 products and 256 additions of non-negative terms, 257 u; + 1e-20: 1 u;
  logf to one ulp of its result = 2 u |log M|, of which the formula carries one |log M| and the other is <= 47 u (|log M| <= 46.1 from 1e-20 up to
  e^46); exp in float64 turns an absolute error of the logarithm into the same relative error.  => c2 = 3 + 1 + 47 = 51, + 1 for the second order: 52.
  Silence: every product is 0, the result is logf(1e-20f) in every element: within 2 ulp (2^-18 each) of log(1e-20).
The bound is loose by design (the float32 restatement stays below 1 % of it): it catches structure -- a dropped sample, a window shifted by one,
a wrong row stride --, not rounding.  Rounding is held by the tightness check: a signal's rel-L2 error in the linear domain against that of the
float32 restatement on the same signal.  The margin was to be 4 x, that of attn_matrix and sync_offset.  Measured on an MI355X: the kernel's
rel-L2 is 2.9e-7 .. 9.4e-7 on every noise signal, the 1 kHz tone and the impulse (1.3e-6 / 1.7e-6 on the bin-centred tone, where the restatement has 5e-7 /
1.4e-6), 1.1 .. 2.9 x the restatement's 2.2e-7 .. 5.1e-7 -- and 3.70, 4.94 and 6.51 x on three signals where the kernel is at its usual 7.6e-7 ..
1.1e-6 and the restatement happens to come out at 1.3e-7 .. 2.9e-7 (DC at full scale: two loud bins, the same in every frame; the one-frame clip).
No defect: at |log M| in 8 .. 16 one ulp of the fp32 OUTPUT is 9.5e-7 of the linear value, so a logarithm rounded correctly (numpy's, in the
restatement) leaves 0.29 ulp rms = 2.7e-7 and one accurate to an ulp (the device's logf) up to 0.58 ulp rms = 5.5e-7: both figures are the
output format's resolution, and the ratio of two of them on a handful of loud bins scatters.  So, as the issue that asked for this check
provides, TIGHT = 1.5 x the worst measured ratio = 1.5 x 6.51.

mask_resize.  Bit-exact against the oracle's integer restatement; this module restates the launcher's dispatch rule (mr_banded) and asserts which
kernel each size reaches.
"""
import numpy as np

from test_gpu_kernels_fp64 import U

LOGMEL_C1, LOGMEL_C2, WIN_RATIO = 56, 52, 4.0
TIGHT = 1.5 * 6.51          # (not the 4 x first asked for: measured, see above)
LOG_FLOOR = float(np.log(1e-20))
NOISE_N = (257, 320, 479, 480, 481, 1599, 1600)


def rng(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v) + 12345) % 2147483647
    return np.random.default_rng(s)


# ================================================================================================================================ logmel
def real_basis():
    from jegal_amd import audio
    return np.asarray(audio.mel_filterbank(), np.float32)


def synthetic_basis():
    """80 x 257: rows 0..4 one-hot on bins 0, 1, 128, 255 and 256 (a single DFT bin each; 256 is the one only thread 0's second pass computes),
    the others small and positive."""
    b = (rng(41).random((80, 257)) * 1e-3 + 1e-6).astype(np.float32)
    for row, f in enumerate(ONE_HOT_BINS):
        b[row] = 0
        b[row, f] = 1
    return b


ONE_HOT_BINS = (0, 1, 128, 255, 256)


def logmel_batches():
    """name -> (3, n) float32, int16 scale, a different signal in every row."""
    out = {}
    for n in NOISE_N:
        r = rng(42, n)
        out[f"noise{n}"] = np.stack([r.standard_normal(n) * a for a in (3000.0, 300.0, 9000.0)]).clip(-32768, 32767).astype(np.float32)
    n = 1600
    t = np.arange(n)
    imp = np.zeros(n)
    imp[800] = 32767
    out["tones_dc"] = np.stack([20000 * np.sin(2 * np.pi * 1000 * t / 16000), 32767 * np.cos(2 * np.pi * 32 * t / 512), np.full(n, 32767.0)]).astype(np.float32)
    out["impulse_silence_tiny"] = np.stack([imp, np.zeros(n), rng(43).standard_normal(n) * 1e-3]).astype(np.float32)
    return out


def frame_index(n, hop=160, clamp=False, keep_last=False):
    """Sample index of element k of frame t in the un-padded signal: (frames, 512).  Defects: another hop, clamped instead of reflected ends, the
    frames 1 .. n // 160 instead of 0 .. n // 160 - 1 (the last STFT frame kept, the first dropped)."""
    nf = n // 160
    idx = (np.arange(nf)[:, None] + (1 if keep_last else 0)) * hop + np.arange(512)[None] - 256
    if clamp:
        return idx.clip(0, n - 1)
    idx = np.abs(idx)
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
    assert n >= 257 and idx.min() >= 0 and idx.max() < n          # (keep_last reaches at most 160 nf + 255 <= n + 255: one reflection)
    return idx


def logmel_ref(wav, basis):
    """(B, n) float32 -> m64 (B, frames, 80), delta of the same shape, both float64."""
    B, n = wav.shape
    win = np.zeros(512)
    win[96:416] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(320) / 320)
    x = wav.astype(np.float64)[:, frame_index(n)]          # (B, frames, 512)
    seg = x * win
    sabs = np.abs(seg).sum(-1)
    inwin = np.abs(x[..., 97:416]).sum(-1)
    assert bool((inwin <= WIN_RATIO * sabs).all()), "the window's absolute error is counted against sum |seg| (module docstring)"
    mag = np.abs(np.fft.rfft(seg, axis=-1))
    b64 = basis.astype(np.float64)
    m = mag @ b64.T
    M = m + 1e-20
    delta = b64.sum(1)[None, None] * (np.sqrt(2) * (512 + LOGMEL_C1) * U * sabs[..., None]) + (257 + LOGMEL_C2 + np.abs(np.log(M))) * U * M
    return m, delta


def lin(out):
    """log-mel as the kernel returns it -> the linear mel domain, float64"""
    return np.exp(np.asarray(out, np.float64)) - 1e-20


def logmel_dft32(wav, win_off=96, hop=160, clamp=False, keep_last=False, stride=None):
    """The first half of a float32 numpy restatement of logmel_kernel: (B, n) -> magnitudes (B, frames, 257) float32, every operation in float32
    and the 512 terms of a bin accumulated in sequence.  Keyword arguments = the planted defects (`stride`: the row stride in samples)."""
    f = np.float32
    B, n = wav.shape
    k = np.arange(512)
    ang = f(6.283185307179586) * (k - win_off).astype(f) / f(320)
    win = np.where((k >= win_off) & (k < win_off + 320), f(0.5) - f(0.5) * np.cos(ang, dtype=f), f(0)).astype(f)
    tang = f(6.283185307179586) * k.astype(f) / f(512)
    tc, ts = np.cos(tang, dtype=f), np.sin(tang, dtype=f)
    idx = frame_index(n, hop, clamp, keep_last)
    flat = wav.reshape(-1)
    rows = [flat[(b * (stride or n) + idx).clip(0, flat.size - 1)] for b in range(B)]
    seg = (np.stack(rows) * win).astype(f).reshape(-1, 512)
    ph = (k[:, None] * np.arange(257)[None]) % 512
    re, im = np.zeros((seg.shape[0], 257), f), np.zeros((seg.shape[0], 257), f)
    for i in range(512):
        re += seg[:, i:i + 1] * tc[ph[i]][None]
        im -= seg[:, i:i + 1] * ts[ph[i]][None]
    return np.sqrt(re * re + im * im).reshape(B, -1, 257)


def logmel_mel32(mag, basis, drop_nyquist=False):
    """The second half: the mel sums in sequence and the logarithm, float32 -> (B, frames, 80).  Defect: bin 256 missing."""
    f = np.float32
    acc = np.zeros(mag.shape[:2] + (80,), f)
    for b in range(257 - (1 if drop_nyquist else 0)):
        acc += mag[..., b:b + 1] * basis[:, b][None, None]
    return np.log(acc + f(1e-20), dtype=f)


def logmel_fails(name, out, m, delta, wav):
    """The element-wise bound (and the silence rule) on one batch -> (worst observed / bound, list of failures)."""
    out = np.asarray(out, np.float64)
    fails, worst = [], 0.0
    for b in range(len(wav)):
        if not np.isfinite(out[b]).all():
            fails.append(f"{name} row {b}: not finite")
            continue
        if not wav[b].any():
            off = float(np.abs(out[b] - LOG_FLOOR).max()) / 2.0 ** -18
            if off > 2:
                fails.append(f"{name} row {b}: silence is {off:.2f} ulp from log(1e-20)")
            continue
        r = float((np.abs(lin(out[b]) - m[b]) / delta[b]).max())
        worst = max(worst, r)
        if r > 1:
            fails.append(f"{name} row {b}: observed/bound {r:.3f}")
    return worst, fails


def rel_l2(out_row, m_row):
    return float(np.linalg.norm(lin(out_row) - m_row) / np.linalg.norm(m_row))


# =========================================================================================================================== mask_resize
MR_SIZES = [(1, 1), (2, 3), (271, 481), (270, 1706), (270, 1707), (5, 4000), (2160, 480)]          # (H, W)
MR_T = 3
MR_RB, MR_SPAN_MAX = 6, 40 * 1024


def mr_banded(H, W, ptr=0):
    """launch_mask_resize's rule: the banded kernel stages the source rows a band of MR_RB output rows can touch, (MR_RB - 1) H / 270 + 3 of them,
    in LDS (+ 4 bytes for the dword alignment) and needs a source that starts on a dword; everything else takes the per-pixel kernel."""
    span_rows = (MR_RB - 1) * H // 270 + 3
    return span_rows * W * 3 + 4 <= MR_SPAN_MAX and W <= 32767 and ptr % 4 == 0


# 1706 | 1707 is the boundary at H = 270 (8 rows: 8 W 3 + 4 <= 40960); (5, 4000) stages 3 rows of 12 000 bytes and is the widest banded size;
# (2160, 480) would stage 43 rows and is generic
MR_KERNEL = {(1, 1): "band", (2, 3): "band", (271, 481): "band", (270, 1706): "band", (270, 1707): "generic", (5, 4000): "band", (2160, 480): "generic"}
for _hw in MR_SIZES:
    assert ("band" if mr_banded(*_hw) else "generic") == MR_KERNEL[_hw], _hw
    assert not mr_banded(*_hw, ptr=1)


def mr_masks(H):
    """two launches of T = 3 frames: every one of -1, 0, H // 3, H - 2, H - 1, H + 50"""
    return [np.asarray([-1, 0, H // 3], np.int32), np.asarray([H - 2, H - 1, H + 50], np.int32)]


def mr_frames(H, W):
    return rng(51, H, W).integers(0, 256, (MR_T, H, W, 3), dtype=np.uint8)


def mr_first_row(my, H):
    return (min(my + 1, H) if my >= 0 else 0)


def mr_pack(frames, mask_y):
    """The rows below each frame's mask back to back -> (packed bytes, int64 offsets); the last frame's rows end exactly at the last byte."""
    T, H, W, _ = frames.shape
    parts = [frames[f, mr_first_row(int(mask_y[f]), H):].reshape(-1) for f in range(T)]
    off = np.zeros(T, np.int64)
    off[1:] = np.cumsum([p.size for p in parts])[:-1]
    return np.concatenate(parts), off
