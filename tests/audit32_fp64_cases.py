"""Cases, float64 references and derived bounds for the fp32 audit kernels (jegal_amd/csrc/audit32.hip): the conv form of gemm32_kernel,
stack_frames32, maxpool32, group_mean32 and zero_tail32.

Imports without a GPU: tests/test_gpu_audit32_fp64.py feeds the cases to the jg_debug_* check points, tests/test_audit32_cases_cpu.py feeds
them to plain torch-float32 stand-ins and to planted defects, so that references and bounds are checked where no GPU is.  Every generator
is seeded and returns CPU tensors.  u = 2^-24.

Conv.  The weights are packed HERE, from tap_order as tests/test_gpu_conv_fp64.py restates it from common.h (k = t C + c, the taps t by
parity class for `reorder` layers of <= 32 taps, natural order otherwise), never by the library.  The reference is float64 F.conv2d on
exactly the fp32 operands, with scale, bias and ReLU / exact GELU in float64.  The weights are independent per tap, so a swapped tap or a
wrong image moves the result by O(|ref|).  Bounds, as for gemm32_case (tests/test_gpu_kernels_fp64.py), K = KH KW C:
  * element-wise  |got - ref| <= 2 K u (conv2d(|in|, |w|) |scale| + |bias|), x 1.13 + 4 u |ref| behind GELU (slope <= 1.13, erff a few ulp);
  * norm-wise     ||got - ref|| / ||ref|| <= 2 sqrt(K) u.
Guards: the input is [one NaN image | nimg images | one NaN image]; W holds NaN in the columns K .. ldw-1, in 16 extra rows and in the
w_off floats in front of it.

The launcher's rules, restated (launch_gemm32): the 128 x 128 tile when ceil(M / 128) ceil(N / 128) >= 384, else 64 x 64; the vector loader
when C % 4 == 0, ldw % 4 == 0 and both operand pointers are 16-byte aligned, else the scalar one.

Exact families (bits compared, no bounds): stack_frames32 (u8 / 255 in IEEE float32 division, float sources copied, lane 15 zero, the
frame index clamped to the clip), maxpool32 (3 x 3 / stride 2), zero_tail32 (rows from the halved length on are zero, every other row
keeps its bit pattern).  group_mean32 is bounded: float64 mean, |got - ref| <= (L + 1) u sum|x| / L (L additions and one division).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from elementwise_fp64_cases import NAN, STACK_PAD, STACK_T, bits, gen, nrnd, ratio, same_bits, stack_case, tail_len, zero_tail_case  # noqa: F401
from test_gpu_conv_fp64 import AUDIO11, AUDIO33, CONV1, CONV2, CONV3_ODD, CONV4, CONV5, geo, tap_order
from test_gpu_kernels_fp64 import U, urnd

GEO_KEYS = ("nimg", "H", "W", "C", "N", "KH", "KW", "SH", "SW", "PH", "PW", "reorder")


# ============================================================================================================================= conv
def tiles128(M, N):
    return -(-M // 128) * -(-N // 128)


def plan32(M, N, C, ldw, w_off=0, conv=1):
    """The instance launch_gemm32 picks for a conv launch whose input pointer is 16-byte aligned whenever C % 4 == 0."""
    vec = C % 4 == 0 and ldw % 4 == 0 and w_off % 4 == 0
    return f"gemm32_kernel<{conv},{int(vec)},{128 if tiles128(M, N) >= 384 else 64}>"


def out_hw(g):
    return (g["H"] + 2 * g["PH"] - g["KH"]) // g["SH"] + 1, (g["W"] + 2 * g["PW"] - g["KW"]) // g["SW"] + 1


def conv_M(g):
    oh, ow = out_hw(g)
    return g["nimg"] * oh * ow


C1_55 = geo(3, 7, 13, 1, 32, 5, 5, 1, 1, 2, 2, False)            # 7 x 13, M 273, K 25: the second k-step holds k = 16 .. 24 and a tail of zeros
C2_33 = geo(7, 11, 13, 2, 32, 3, 3, 2, 2, 1, 1, True)            # 6 x 7, M 294, K 18: the tap table in the scalar loader, two taps per quad
AUDIO_DEEP = geo(6, 9, 5, 512, 128, 3, 3, 1, 1, 1, 1, False)     # 9 x 5, M 270, K 4608: the audio stream's deepest layer
CONV5_N130 = dict(CONV5, N=130)                                  # N % 4 != 0: the scalar-store epilogue
THR_ABOVE = geo(43, 17, 17, 4, 512, 3, 3, 1, 1, 1, 1, False)     # M 12427: 98 x 4 = 392 tiles of 128 x 128
THR_BELOW = dict(THR_ABOVE, nimg=42)                             # M 12138: 95 x 4 = 380
THR_C1 = geo(43, 17, 17, 1, 512, 5, 5, 1, 1, 2, 2, False)        # the scalar loader on the 128 tile
CONV1_FORM = dict(CONV1, nimg=779)                               # M 49077, N 64: 384 x 1 tiles, half of every n-tile empty

# (name, geometry, options): act 0 none / 1 ReLU / 2 GELU; ldw default K + 8; w_off floats in front of W; ldc default N + 4.
# fmaxf turns a NaN that was read into 0, so every guard family has a case without ReLU.
SMALL_CASES = [
    ("conv1_natural", CONV1, dict(act=1, scale=True)),
    ("conv1_natural_norelu", CONV1, dict(act=0)),
    ("conv2_table", CONV2, dict(act=1)),
    ("conv2_table_norelu", CONV2, dict(act=0, scale=True)),
    ("conv3_oddw", CONV3_ODD, dict(act=1, scale=True)),
    ("conv3_oddw_norelu", CONV3_ODD, dict(act=0, bias=False)),
    ("conv4_stride12", CONV4, dict(act=0)),
    ("conv5_pad4", CONV5, dict(act=1)),
    ("conv5_pad4_gelu", CONV5, dict(act=2, scale=True)),
    ("audio_3x3_natural", AUDIO33, dict(act=1)),
    ("audio_1x1", AUDIO11, dict(act=0)),
    ("c1_5x5", C1_55, dict(act=0)),
    ("c1_5x5_relu", C1_55, dict(act=1, scale=True)),
    ("c2_3x3_table", C2_33, dict(act=0)),
    ("audio_deep_k4608", AUDIO_DEEP, dict(act=0, scale=True)),
    ("audio_deep_k4608_relu", AUDIO_DEEP, dict(act=1)),
    ("w_offset_scalar_loader", CONV5, dict(act=0, w_off=1, ldw_extra=1)),
    ("w_offset_scalar_loader_table", CONV2, dict(act=1, w_off=1, ldw_extra=1)),
    ("scalar_store_n130", CONV5_N130, dict(act=0, ldc_extra=1)),
    ("scalar_store_n130_relu", CONV5_N130, dict(act=1, ldc_extra=1, scale=True)),
]
PLANNER_CASES = [
    ("threshold_392_tiles", THR_ABOVE, dict(act=1, scale=True)),
    ("threshold_380_tiles", THR_BELOW, dict(act=0)),
    ("threshold_c1_392_tiles", THR_C1, dict(act=0)),
]
CONV1_FORM_CASES = [("conv1_form_n64_tile128", CONV1_FORM, dict(act=0))]
CONV_FAMILIES = dict(small=SMALL_CASES, planner=PLANNER_CASES, conv1_form=CONV1_FORM_CASES)
CONV32_INSTANCES = {"gemm32_kernel<1,1,64>", "gemm32_kernel<1,0,64>", "gemm32_kernel<1,1,128>", "gemm32_kernel<1,0,128>"}


def case_opts(g, o):
    """The options of a case with their defaults filled in."""
    K = g["KH"] * g["KW"] * g["C"]
    ldw = K + o.get("ldw_extra", 8)
    return dict(act=o.get("act", 0), scale=o.get("scale", False), bias=o.get("bias", True), w_off=o.get("w_off", 0), ldw=ldw,
                ldc=g["N"] + o.get("ldc_extra", 4), kname=plan32(conv_M(g), g["N"], g["C"], ldw, o.get("w_off", 0)))


def pack(w4, order):
    """Wpacked[o][t C + c] = w[o][c][kh_t][kw_t]"""
    return torch.cat([w4[:, :, kh, kw] for kh, kw in order], 1)


_DATA = {}


def conv32_data(g, seed=0):
    """Operands (fp32) and the float64 sums of one geometry, computed once and shared between its cases."""
    key = tuple(g[k] for k in GEO_KEYS) + (seed,)
    if key in _DATA:
        return _DATA[key]
    nimg, H, W, C, N, KH, KW, SH, SW, PH, PW, reorder = key[:-1]
    gn = gen(20, *key)
    K = KH * KW * C
    OH, OW = out_hw(g)
    M = nimg * OH * OW
    x = urnd(gn, (nimg, H, W, C)).float()
    w4 = (urnd(gn, (N, C, KH, KW)) / math.sqrt(K) * 2).float()              # independent per tap
    sc, bi = urnd(gn, (N,), 0.5, 1.5).float(), urnd(gn, (N,)).float()

    def conv(a, b):
        return F.conv2d(a.permute(0, 3, 1, 2), b, stride=(SH, SW), padding=(PH, PW)).permute(0, 2, 3, 1).reshape(M, N)
    inbuf = torch.full((nimg + 2, H, W, C), NAN, dtype=torch.float32)
    inbuf[1:nimg + 1] = x
    d = dict(M=M, K=K, OH=OH, OW=OW, x=x, w4=w4, wp=pack(w4, tap_order(KH, KW, SH, SW, reorder)), sc=sc, bi=bi, inbuf=inbuf,
             acc=conv(x.double(), w4.double()), mag=conv(x.double().abs(), w4.double().abs()))
    _DATA[key] = d
    return d


def w_buffer(d, ldw, w_off):
    """Flat fp32 buffer: w_off NaN floats, then [N + 16][ldw] with the packed rows in its corner and NaN everywhere else."""
    N, K = d["wp"].shape
    buf = torch.full((N + 16, ldw), NAN, dtype=torch.float32)
    buf[:N, :K] = d["wp"]
    return torch.cat([torch.full((w_off,), NAN, dtype=torch.float32), buf.reshape(-1)])


def conv32_expect(d, act, scale, bias):
    """-> (reference, element-wise bound, norm-wise bound)"""
    N, K = d["wp"].shape
    scd = d["sc"].double() if scale else torch.ones(N, dtype=torch.float64)
    bid = d["bi"].double() if bias else torch.zeros(N, dtype=torch.float64)
    v = d["acc"] * scd + bid
    eb = 2 * K * U * (d["mag"] * scd.abs() + bid.abs())
    if act == 1:
        v = v.clamp_min(0)
    elif act == 2:
        v = 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))
        eb = eb * 1.13 + 4 * U * v.abs()
    return v, eb, 2 * math.sqrt(K) * U


def conv32_ratio(got, v, eb, nb):
    """max(element-wise, norm-wise) observed / bound; inf when got is not finite"""
    got = got.double()
    if not bool(got.isfinite().all()):
        return float("inf")
    err = (got - v).abs()
    el = torch.where(err == 0, torch.zeros_like(err), err / eb)
    return max(float(el.max()), float((got - v).norm() / v.norm().clamp_min(1e-300)) / nb)


def epilogue32(y, d, act, scale, bias):
    """float32 epilogue of a stand-in: y (M, N) float32 sums"""
    if scale:
        y = y * d["sc"]
    if bias:
        y = y + d["bi"]
    if act == 1:
        y = y.clamp_min(0)
    elif act == 2:
        y = 0.5 * y * (1 + torch.erf(y * 0.70710678118654752))
    return y


def conv32_standin(g, d, act, scale, bias):
    """float32 F.conv2d over the weights un-packed from the test's own packing"""
    N, C, KH, KW = d["w4"].shape
    w4 = torch.empty_like(d["w4"])
    for t, (kh, kw) in enumerate(tap_order(KH, KW, g["SH"], g["SW"], g["reorder"])):
        w4[:, :, kh, kw] = d["wp"][:, t * C:(t + 1) * C]
    y = F.conv2d(d["x"].permute(0, 3, 1, 2), w4, stride=(g["SH"], g["SW"]), padding=(g["PH"], g["PW"])).permute(0, 2, 3, 1).reshape(d["M"], N)
    return epilogue32(y, d, act, scale, bias)


def patches(x, g, order=None, clamp_pad=False):
    """The implicit GEMM's A matrix (M, K) by explicit gathers, k = t C + c over `order` (default: the geometry's own).
    clamp_pad plants a defect: a tap outside the image reads the nearest pixel instead of zero."""
    nimg, H, W, C = x.shape
    OH, OW = out_hw(g)
    order = order or tap_order(g["KH"], g["KW"], g["SH"], g["SW"], g["reorder"])
    oh, ow = torch.arange(OH)[:, None], torch.arange(OW)[None, :]
    cols = []
    for kh, kw in order:
        ih, iw = oh * g["SH"] - g["PH"] + kh, ow * g["SW"] - g["PW"] + kw
        p = x[:, ih.clamp(0, H - 1), iw.clamp(0, W - 1)]                      # (nimg, OH, OW, C)
        if not clamp_pad:
            ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            p = torch.where(ok[None, :, :, None], p, torch.zeros_like(p))
        cols.append(p)
    return torch.cat(cols, -1).reshape(nimg * OH * OW, len(order) * C)


# ===================================================================================================================== exact families
# ---- stack_frames32 ------------------------------------------------------------------------------------------------------------------
def stack32_case(u8, B, T, H, W):
    """The stack_case sources with one more frame in front of and behind every clip: NaN for float sources, 255 - (the neighbouring
    frame) for u8, so a clamp that is off by one frame at either end changes every element it touches.  `offset`: the element of buf at
    which the clip's frame 0 starts (the pointer the kernel gets); strides in elements of buf."""
    c = stack_case(u8, B, T, H, W)
    src = c["src"]
    if u8:
        buf = torch.empty((B, T + 2, H, W, 3), dtype=torch.uint8)
        buf[:, 1:T + 1] = src
        buf[:, 0] = 255 - src[:, 0]
        buf[:, T + 1] = 255 - src[:, T - 1]
        st = H * W * 3
        return dict(buf=buf, offset=st, strides=((T + 2) * st, st, W * 3, 3, 1), framed=buf)
    Wp = W + 3
    buf = torch.full((B, 3, T + 2, H, Wp), NAN, dtype=torch.float32)
    buf[:, :, 1:T + 1] = src
    st = H * Wp
    return dict(buf=buf, offset=st, strides=(3 * (T + 2) * st, st, Wp, 1, (T + 2) * st), framed=buf[..., :W].permute(0, 2, 3, 4, 1))


def stack32_ref(c, u8, T, pad, lo=0, hi=None):
    """(B, P, H, W, 16) float32 from the framed logical view (B, T + 2, H, W, 3); lo / hi plant a wrong clamp (default 0 .. T - 1)."""
    hi = T - 1 if hi is None else hi
    fr = c["framed"].float()
    if u8:
        fr = torch.div(fr, torch.tensor(255.0, dtype=torch.float32))          # IEEE float32 division
    B, _, H, W, _ = fr.shape
    P = T + 2 * pad - 4
    out = torch.zeros((B, P, H, W, 16), dtype=torch.float32)
    for dt in range(5):
        f = (torch.arange(P) + dt - pad).clamp(lo, hi)
        out[..., dt * 3:dt * 3 + 3] = fr[:, f + 1]
    return out


def stack32_ref_loops(c, u8, T, pad):
    """The same by explicit loops in numpy, dividing by np.float32(255)."""
    fr = c["framed"].numpy().astype(np.float32)
    if u8:
        fr = fr / np.float32(255)
    B, _, H, W, _ = fr.shape
    P = T + 2 * pad - 4
    out = np.zeros((B, P, H, W, 16), np.float32)
    for b in range(B):
        for p in range(P):
            for dt in range(5):
                f = min(max(p + dt - pad, 0), T - 1)
                for ch in range(3):
                    out[b, p, :, :, dt * 3 + ch] = fr[b, f + 1, :, :, ch]
    return out


# ---- maxpool32 -------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(3, 7, 7, 4), (2, 8, 9, 8), (1, 3, 3, 4), (2, 19, 12, 256), (2, 10, 10, 256)]


def pool_case(nimg, H, W, C):
    """buf = [NaN image | nimg images | NaN image]; the last row / column of an even H / W, which no window reaches, holds NaN."""
    g = gen(21, nimg, H, W, C)
    x = urnd(g, (nimg, H, W, C), -4, 4).float()
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous()
    xdev = x.clone()
    xdev[:, 2 * OH + 1:] = NAN
    xdev[:, :, 2 * OW + 1:] = NAN
    buf = torch.full((nimg + 2, H, W, C), NAN, dtype=torch.float32)
    buf[1:nimg + 1] = xdev
    return dict(x=x, xdev=xdev, buf=buf, ref=ref, OH=OH, OW=OW, unread=(H - 2 * OH - 1, W - 2 * OW - 1))


def pool_ref_loops(x, shift=0):
    """Explicit loops in numpy; shift plants a window that starts `shift` columns to the right (reads wrap into the next row's memory
    as the kernel's address arithmetic would)."""
    a = x.numpy()
    nimg, H, W, C = a.shape
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    flat = np.concatenate([a.reshape(nimg, H * W, C), np.full((nimg, 4, C), np.nan, np.float32)], 1)
    out = np.empty((nimg, OH, OW, C), np.float32)
    for oh in range(OH):
        for ow in range(OW):
            win = [flat[:, (oh * 2 + kh) * W + ow * 2 + kw + shift] for kh in range(3) for kw in range(3)]
            out[:, oh, ow] = np.max(np.stack(win), 0)
    return out


# ---- zero_tail32 -----------------------------------------------------------------------------------------------------------------------
ZT_H, ZT_ROW_ELEMS, ZT_HALVINGS = (1, 5), (8, 1024, 1028), (0, 1, 2, 3)          # row_vec = row_elems / 4: 2, 256 (one pass of the block), 257


def zero_tail32_case(H, row_elems, halvings):
    """The zero_tail_case clip lengths (negative, 0, 1, exact, past the end, one row short) over rows of random non-zero bit patterns,
    NaN payloads included -> int32 (B, H, row_elems) before and after."""
    valid = zero_tail_case(H, 8, halvings, torch.float32)["valid"]
    g = gen(22, H, row_elems, halvings)
    x = torch.randint(-2 ** 31, 2 ** 31, (len(valid), H, row_elems), generator=g, dtype=torch.int64)
    x = torch.where(x == 0, torch.ones_like(x), x).to(torch.int32)
    ref = x.clone()
    for b, v in enumerate(valid):
        ref[b, tail_len(v, halvings):] = 0
    return dict(x=x, valid=valid, ref=ref)


# ================================================================================================================== bounded: group_mean32
GM_L, GM_D, GM_GROUPS = (1, 21, 150), (4, 1024), (1, 33)


def group_mean32_case(groups, L, D):
    """buf = [NaN group | groups x L rows | NaN group]"""
    g = gen(23, groups, L, D)
    x = nrnd(g, (groups * L, D)).float()
    xd = x.double().reshape(groups, L, D)
    buf = torch.full(((groups + 2) * L, D), NAN, dtype=torch.float32)
    buf[L:(groups + 1) * L] = x
    return dict(x=x, buf=buf, ref=xd.mean(1), bound=(L + 1) * U * xd.abs().sum(1) / L)
