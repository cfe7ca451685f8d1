"""Cases, float64 references and derived bounds for the element-wise and reduction kernels (jegal_amd/csrc/elementwise*.hip).

Imports without a GPU: tests/test_gpu_elementwise_fp64.py feeds the cases to the jg_debug_* check points, tests/test_elementwise_cases_cpu.py
feeds them to plain torch-float32 stand-ins and to planted defects, so that references and bounds are checked where no GPU is.

Every generator is seeded and returns CPU tensors holding exactly the values the kernel receives (16-bit operands are rounded here), the
float64 reference computed from those values, and the bound.  u = 2^-24; "+ ulp16" is one ulp of the reference in the build's 16-bit
type.  The bounds are derived from the arithmetic the kernels are documented to do, never from what a kernel returned:
  * an fp32 sum of n terms errs by at most ~n u times the sum of the magnitudes; the factor 2 covers the few roundings around it;
  * the bit-exact families have no bound: the reference repeats the kernel's one or two IEEE operations in torch float32.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from test_gpu_kernels_fp64 import U, dt16, ulp16, urnd

NAN = float("nan")
LN_STD, LN_ANNOTATED = 0, 1


def gen(*seed):
    """A generator seeded by the case's parameters, mixed arithmetically (the same cases under every interpreter)."""
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v) + 12345) % 2147483647
    return torch.Generator().manual_seed(s)


def nrnd(g, shape):
    return torch.randn(shape, generator=g, dtype=torch.float64)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got, ref):
    """Bit equality, NaN compared as NaN-ness only."""
    gn, rn = got.isnan(), ref.isnan()
    return bool((gn == rn).all()) and bool((bits(got)[~rn] == bits(ref)[~rn]).all())


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf when got is not finite; 0 / 0 counts as 0."""
    got = got.double()
    if not bool(got.isfinite().all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ================================================================================================================= bit-exact families
# ---- stack_frames ------------------------------------------------------------------------------------------------------------------
STACK_T, STACK_PAD = (1, 5, 6), (0, 2, 12)


def stack_case(u8, B, T, H, W, seed=1):
    """Source + element strides.  u8: channels-last (B,T,H,W,3).  float: channels-first (B,3,T,H,W+3) in [0,1] whose three extra columns
    per row are NaN (sh = W + 3): the kernel must not read them.  `frames` = the logical (B,T,H,W,3) view."""
    g = gen(seed, u8, B, T, H, W)
    if u8:
        src = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.int32).to(torch.uint8)
        return dict(src=src, frames=src, strides=(T * H * W * 3, H * W * 3, W * 3, 3, 1))
    src = torch.full((B, 3, T, H, W + 3), NAN, dtype=torch.float32)
    src[..., :W] = torch.rand((B, 3, T, H, W), generator=g)
    Wp = W + 3
    return dict(src=src, frames=src[..., :W].permute(0, 2, 3, 4, 1), strides=(3 * T * H * Wp, H * Wp, Wp, 1, T * H * Wp))


def stack_ref(frames, T, pad, d16):
    B, _, H, W, _ = frames.shape
    P = T + 2 * pad - 4
    out = torch.zeros((B, P, H, W, 16), dtype=d16)
    for dt in range(5):
        f = (torch.arange(P) + dt - pad).clamp(0, T - 1)
        out[..., dt * 3:dt * 3 + 3] = frames[:, f].float().to(d16)
    return out


def stack_ref_loops(frames, T, pad):
    """The same by explicit loops, in float32 numpy (the caller rounds)."""
    fr = frames.float().numpy()
    B, _, H, W, _ = fr.shape
    P = T + 2 * pad - 4
    out = np.zeros((B, P, H, W, 16), np.float32)
    for b in range(B):
        for p in range(P):
            for dt in range(5):
                f = min(max(p + dt - pad, 0), T - 1)
                for c in range(3):
                    out[b, p, :, :, dt * 3 + c] = fr[b, f, :, :, c]
    return out


# ---- window_gather -----------------------------------------------------------------------------------------------------------------
def tiled_index(m, n):
    """Element (row m, column n) of the tiled token plane (jegal_amd/csrc/common.h)."""
    return (m >> 7) * 65536 + (n >> 6) * 8192 + ((m & 127) >> 4) * 1024 + ((n & 63) >> 4) * 256 + (m & 15) * 16 + (n & 15)


GATHER_ROW_CASES = [(2, 5, Twin, L, D, shift) for Twin in (1, 3) for L in (1, 21) for shift in (0, 8, 30) for D in (4, 512)]
# M = B Twin L in {1, 15, 16, 17, 127, 129, 21 * 7}
GATHER_TILED_CASES = [(1, 1, 1), (1, 3, 5), (2, 2, 4), (1, 17, 1), (1, 127, 1), (1, 43, 3), (1, 7, 21)]


def gather_case(B, P, Twin, L, D, shift, seed=2):
    g = gen(seed, B, P, Twin, L, D, shift)
    return dict(conv=nrnd(g, (B, P, D)).float(), pe=nrnd(g, (L, D)).float())


def gather_rows(B, P, Twin, L, shift, lo=0, hi_off=1):
    """Source position of every output row (b, i, j); lo / hi_off plant a wrong clamp."""
    i = torch.arange(Twin)[:, None]
    j = torch.arange(L)[None, :]
    return (i + j - shift).clamp(lo, P - hi_off)


def gather_ref(c, B, P, Twin, L, shift, lo=0, hi_off=1):
    """fp32: one IEEE add per element, rows in (b, i, j) order -> (B Twin L, D)."""
    pp = gather_rows(B, P, Twin, L, shift, lo, hi_off)
    x = c["conv"][:, pp] + c["pe"][None, None]
    return x.reshape(B * Twin * L, -1)


def gather_ref_loops(c, B, P, Twin, L, shift):
    conv, pe = c["conv"].numpy(), c["pe"].numpy()
    out = np.empty((B * Twin * L, conv.shape[-1]), np.float32)
    for b in range(B):
        for i in range(Twin):
            for j in range(L):
                out[(b * Twin + i) * L + j] = conv[b, min(max(i + j - shift, 0), P - 1)] + pe[j]
    return out


def tiled_plane(x16, elems, fill_bits):
    """Row-major 16-bit (M, 512) -> the tiled plane of `elems` elements, everything else holding fill_bits."""
    M = x16.shape[0]
    plane = torch.full((elems,), fill_bits, dtype=torch.int16)
    m = torch.arange(M)[:, None]
    n = torch.arange(512)[None, :]
    plane[tiled_index(m, n).reshape(-1)] = bits(x16).reshape(-1)
    return plane


def tiled_plane_loops(x16, elems, fill_bits):
    src = bits(x16).numpy()
    plane = np.full(elems, fill_bits, np.int16)
    for m in range(src.shape[0]):
        base = (m // 128) * 65536 + ((m % 128) // 16) * 1024 + (m % 16) * 16
        for nb in range(8):
            for q in range(4):
                o = base + nb * 8192 + q * 256
                plane[o:o + 16] = src[m, nb * 64 + q * 16:nb * 64 + q * 16 + 16]
    return plane


# ---- cast --------------------------------------------------------------------------------------------------------------------------
def cast_values(n, seed=3):
    """fp32 inputs: +-0, target subnormals, halfway ties both ways (fp16 and bf16 spacing), overflow to inf, inf, NaN, then random."""
    sp = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25, 1.0001 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25,
          2.0 ** -130, 1.5 * 2.0 ** -133, 2.0 ** -134, 2.0 ** -140,
          1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -23,
          65504.0, 65519.9, 65520.0, -65520.0, 1e5, 3.3895e38, 3.4e38, float("inf"), -float("inf"), NAN]
    g = gen(seed, n)
    x = (nrnd(g, (n,)) * torch.exp2(urnd(g, (n,), -20, 17))).float()
    k = min(n, len(sp))
    if n < len(sp):          # the short case takes the harshest ones
        sp = [2.0 ** -25, 1 + 3 * 2.0 ** -11, 65520.0, NAN]
    x[:k] = torch.tensor(sp[:k], dtype=torch.float32)
    return x


def cast_ref_numpy(x, bf):
    """Second formulation: numpy for fp16, the integer round-to-nearest-even rule for bf16 -> int16 bits."""
    a = x.numpy()
    if not bf:
        with np.errstate(over="ignore"):
            return a.astype(np.float16).view(np.int16)
    b = a.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return r.view(np.int16)


# ---- zero_tail ---------------------------------------------------------------------------------------------------------------------
def tail_len(v, halvings):
    n = max(int(v), 0)
    for _ in range(halvings):
        n = (n - 1) // 2 + 1 if n > 0 else 0
    return n


def zero_tail_case(H, row_elems, halvings, d16, seed=4):
    valid = [-3, 0, 1, H * 2 ** halvings, H * 2 ** halvings + 7]
    if H > 1:
        valid.append((H - 1) * 2 ** halvings)          # one row short
    g = gen(seed, H, row_elems, halvings)
    x = urnd(g, (len(valid), H, row_elems), 0.5, 2.0).to(d16)          # never zero: a zeroed row shows
    ref = x.clone()
    for b, v in enumerate(valid):
        ref[b, tail_len(v, halvings):] = 0
    return dict(x=x, valid=valid, ref=ref)


# ---- xlmr_embed --------------------------------------------------------------------------------------------------------------------
XL_VOCAB, XL_MAXPOS, XL_PAD = 50, 40, 1


def xlmr_ids(L, seed=5):
    """Six sequences: no pad; pads at the start; inside; at the end; all pad; ids outside the vocabulary."""
    g = gen(seed, L)
    ids = torch.randint(2, XL_VOCAB, (6, L), generator=g, dtype=torch.int32)
    ids[1, :max(L // 3, 1)] = XL_PAD
    ids[2, L // 3:L // 3 + max(L // 4, 1)] = XL_PAD
    ids[2, L - 1 - L // 5] = XL_PAD
    ids[3, L - max(L // 2, 1):] = XL_PAD
    ids[4] = XL_PAD
    ids[5, ::2] = -7
    ids[5, 1::3] = XL_VOCAB + 4
    if L > 1:
        ids[5, -1] = XL_VOCAB
    return ids


def xlmr_tables(D, seed=6):
    g = gen(seed, D)
    return dict(word=nrnd(g, (XL_VOCAB, D)).float(), pos=nrnd(g, (XL_MAXPOS, D)).float(), type=nrnd(g, (D,)).float())


def xlmr_pid(ids, inclusive=True):
    nonpad = ids != XL_PAD
    cnt = nonpad.long().cumsum(1)
    if not inclusive:
        cnt = cnt - nonpad.long()
    return torch.where(nonpad, XL_PAD + cnt, torch.full_like(cnt, XL_PAD)).clamp(max=XL_MAXPOS - 1)


def xlmr_pid_loops(ids):
    out = np.zeros(ids.shape, np.int64)
    for b in range(ids.shape[0]):
        n = 0
        for t in range(ids.shape[1]):
            if int(ids[b, t]) != XL_PAD:
                n += 1
                out[b, t] = min(XL_PAD + n, XL_MAXPOS - 1)
            else:
                out[b, t] = XL_PAD
    return out


def xlmr_ref(ids, tb, inclusive=True):
    """fp32 (word[id] + type) + pos[pid], in that order -> (B L, D)."""
    idc = ids.long().clamp(0, XL_VOCAB - 1)
    v = (tb["word"][idc] + tb["type"]) + tb["pos"][xlmr_pid(ids, inclusive)]
    return v.reshape(-1, v.shape[-1])


def planes_ref(v, d16):
    hi = v.to(d16)
    lo = (v - hi.float()).to(d16)
    vd = v.double().reshape(v.shape[0], -1, 64)
    va = vd.abs()
    return dict(hi=hi, lo=lo, s1=vd.sum(-1), s2=(vd * vd).sum(-1), b1=2 * 64 * U * va.sum(-1), b2=2 * 64 * U * (va * va).sum(-1))


# ---- rc_bias: the clip means on {0, 1} operands ---------------------------------------------------------------------------------------
def rc_sample(rpc):
    """Rows of a clip of rpc rows that enter its mean: every row when rpc < 1024, else the 16-row runs (r >> 4) % 8 == 0."""
    r = torch.arange(rpc)
    return r if rpc < 1024 else r[((r >> 4) % 8) == 0]


def rc_rows_sampled(rpc):
    """The count, as the kernel's rc_rows_sampled computes it (second formulation of len(rc_sample))."""
    if rpc < 1024:
        return rpc
    return sum(min(rpc - r0, 16) for r0 in range(0, rpc, 128))


def rc_clip_rows(rpc_all, valid, c):
    rpc = rpc_all if valid is None else min(max(int(valid[c]), 1), rpc_all)
    return c * rpc_all + rc_sample(rpc)


# (rpc_all, nclips, valid)
RC_MEAN_CASES = [(r, 3, None) for r in (1, 15, 17, 259, 1023, 1024, 1030, 1157)] + [
    (21, 33, None), (21, 33, [0, 1, 21, 26] * 8 + [7]), (259, 3, [0, 1, 264]), (1030, 3, [1030, 1035, 1024]), (1100, 3, [1023, 1024, 1100]),
    (17, 3, [17, 0, 22])]


def rc_mean_case(rpc_all, nclips, valid, K, lda, seed=7):
    """A in {0, 1} (the fp32 sums are exact) with NaN in every row outside a clip's sample and in the columns K .. lda-1.
    mean16 = RNE16(float32(s) / float32(R)), fp16 (the run-time correction is an fp16-build path)."""
    g = gen(seed, rpc_all, nclips, K)
    M = nclips * rpc_all
    a01 = (torch.rand((M, K), generator=g) < 0.5).to(torch.float16)
    A = torch.full((M, lda), NAN, dtype=torch.float16)
    mean = torch.empty((nclips, K), dtype=torch.float16)
    for c in range(nclips):
        rows = rc_clip_rows(rpc_all, valid, c)
        A[rows, :K] = a01[rows]
        s = a01[rows].float().sum(0)
        mean[c] = (s / torch.tensor(float(len(rows)), dtype=torch.float32)).to(torch.float16)
    return dict(A=A, a01=a01, mean16=mean)


# ================================================================================================================== bounded families
# ---- layernorm ---------------------------------------------------------------------------------------------------------------------
LN_FAMILIES = ("normal", "offset", "small", "large")
LN_ROWS = (1, 5, 257)


def ln_input(family, rows, D, seed=8):
    """unit normal; per-row offset of about one sigma; scale 1e-3 (eps matters); scale 300 with offset 100."""
    g = gen(seed, LN_FAMILIES.index(family), rows, D)
    x = nrnd(g, (rows, D))
    if family == "offset":
        x = x + nrnd(g, (rows, 1))
    elif family == "small":
        x = x * 1e-3
    elif family == "large":
        x = x * 300 + 100
    return dict(x=x.float(), w=urnd(g, (D,), 0.5, 1.5).float() * (torch.rand(D, generator=g) < 0.5).double().mul(2).sub(1).float(),
                b=urnd(g, (D,)).float())


def ln_eval(x, w, b, flavour, relu, eps=None):
    """x (rows, D) float64 -> (y, xhat w, inv): nn.LayerNorm (biased variance, eps inside the root) or the annotated form (unbiased std + eps)."""
    D = x.shape[1]
    xc = x - x.mean(1, keepdim=True)
    ss = (xc * xc).sum(1, keepdim=True)
    if flavour == LN_STD:
        inv = 1 / torch.sqrt(ss / D + (1e-5 if eps is None else eps))
    else:
        inv = 1 / (torch.sqrt(ss / (D - 1)) + (1e-6 if eps is None else eps))
    xw = xc * inv * w
    y = xw + b
    return (y.clamp_min(0) if relu else y), xw, inv


def ln_case(c, flavour, relu, x64=None):
    """Reference, bounds, and the two defects the bounds must see, on the case's own operands.
    element-wise |got - ref| <= 2u (D mean_row|x| inv |w| + (D/2 + 4) |xhat w| + |ref|): the mean's error carried through, the relative error
    of the sum of squares, the last roundings.  norm-wise (fp32 output): ||got - ref|| / ||ref - b|| <= 2 sqrt(D) u."""
    x = c["x"].double() if x64 is None else x64
    w, b = c["w"].double(), c["b"].double()
    D = x.shape[1]
    ref, xw, inv = ln_eval(x, w, b, flavour, relu)
    bound = 2 * U * (D * x.abs().mean(1, keepdim=True) * inv * w.abs() + (D / 2 + 4) * xw.abs() + ref.abs())
    # other_flavour moves every case by ~1 / (2D) (1e-3 at D = 512) and is asserted everywhere.  other_eps is asserted where eps matters, the
    # "small" family only: at unit scale 1e-5 against 1e-6 moves the result by 4.5e-6 relative, below 5x the element bound (~3e-5 |xhat w|)
    # and below 10x the norm bound (2.7e-5), so no derived bound can see it there.
    other_flavour = ln_eval(x, w, b, 1 - flavour, relu)[0]
    other_eps = ln_eval(x, w, b, flavour, relu, eps=1e-6 if flavour == LN_STD else 1e-5)[0]
    return dict(ref=ref, bound=bound, nbound=2 * math.sqrt(D) * U, scale=(ref - b).norm(), other_flavour=other_flavour, other_eps=other_eps)


def ln_nrm(got, k):
    return float((got.double() - k["ref"]).norm() / k["scale"])


def ln_standin(c, flavour, relu, x32=None):
    """Plain torch float32, two passes."""
    x = c["x"] if x32 is None else x32
    D = x.shape[1]
    xc = x - x.mean(1, keepdim=True)
    ss = (xc * xc).sum(1, keepdim=True)
    inv = 1 / torch.sqrt(ss / D + 1e-5) if flavour == LN_STD else 1 / (torch.sqrt(ss / (D - 1)) + 1e-6)
    y = xc * inv * c["w"] + c["b"]
    return y.clamp_min(0) if relu else y


def planes_input(family, rows, d16, seed=9):
    """layernorm_planes: x = hi + lo (summed in float64), D = 768."""
    c = ln_input(family, rows, 768, seed)
    hi = c["x"].to(d16)
    lo = (c["x"] - hi.float()).to(d16)
    c.update(hi=hi, lo=lo, x64=hi.double() + lo.double())
    return c


# ---- ln_stats ----------------------------------------------------------------------------------------------------------------------
def ln_stats_case(rows, P, const_rows, seed=10):
    """fp32 partial (sum, sum of squares) per 64 columns, as the test feeds them; the kernel adds them in double, so the reference (float64
    over the SAME partials) differs by the final roundings only: |mean err| <= u |mean|, |rstd err| <= 4u rstd (var -> float, + eps, sqrt, 1/x).
    The first const_rows rows are constant: their variance is rounding noise of either sign around 0 and clamps at 0."""
    g = gen(seed, rows, P, const_rows)
    x = nrnd(g, (rows, P, 64)) * urnd(g, (rows, 1, 1), 0.1, 3.0) + nrnd(g, (rows, 1, 1))
    consts = [1.1, 0.7, 2.3, 1.9, 0.3, 2.9, 1.3, 0.9]
    for r in range(min(const_rows, rows)):
        x[r] = consts[r % 8]
    part = torch.stack([x.sum(-1), (x * x).sum(-1)], -1).float()
    n = P * 64
    s = part.double().sum(1)
    mean = s[:, 0] / n
    raw = s[:, 1] / n - mean * mean
    rstd = 1 / torch.sqrt(raw.clamp_min(0) + 1e-5)
    return dict(part=part, mean=mean, rstd=rstd, raw_var=raw, bmean=U * mean.abs(), brstd=4 * U * rstd)


def ln_stats_standin(c):
    """float32 instead of the kernel's double accumulation is too coarse for this bound by design; the stand-in is float64 sums + float32 ends."""
    n = c["part"].shape[1] * 64
    s = c["part"].double().sum(1)
    mean = s[:, 0] / n
    var = (s[:, 1] / n - mean * mean).clamp_min(0).float()
    return mean.float(), 1 / torch.sqrt(var + torch.tensor(1e-5, dtype=torch.float32))


# ---- group_mean --------------------------------------------------------------------------------------------------------------------
def group_mean_case(groups, L, D, d16, seed=11):
    g = gen(seed, groups, L, D)
    x = nrnd(g, (groups * L, D)).to(d16)
    xd = x.double().reshape(groups, L, D)
    ref = xd.mean(1)
    return dict(x=x, ref=ref, bound=2 * L * U * xd.abs().mean(1))          # + ulp16 at the comparison; L = 1 is exact


# ---- col_sum -----------------------------------------------------------------------------------------------------------------------
def col_sum_case(M, K, with_stats, seed=12):
    """Two calls on the same A into a pre-filled out: out = out0 + 2 sum.  Per call 2 M u sum_m |term| for the fp32 sums, plus 2u of the
    result for the `out[k] += s` step (one rounding of a value of the result's size, doubled like everything else)."""
    g = gen(seed, M, K, with_stats)
    A = nrnd(g, (M, K)).to(torch.float16)
    out0 = nrnd(g, (K,)).float()
    a = A.double()
    stats = None
    if with_stats:
        stats = torch.stack([nrnd(g, (M,)) * 0.3, urnd(g, (M,), 0.5, 2.0)], 1).float()
        a = (a - stats[:, :1].double()) * stats[:, 1:].double()
    s, mag = a.sum(0), a.abs().sum(0)
    ref1 = out0.double() + s
    ref2 = ref1 + s
    return dict(A=A, out0=out0, stats=stats, ref=ref2, bound=2 * (2 * M * U * mag) + 2 * U * (ref1.abs() + ref2.abs()))


# ---- rc_bias: the product ---------------------------------------------------------------------------------------------------------------
# (rpc_all, nclips, valid, K, N, tiled, bias)
RC_OUT_CASES = [(21, 33, None, 512, 96, 0, True), (21, 33, [0, 1, 21, 26] * 8 + [7], 512, 32, 1, True), (1030, 1, None, 2048, 32, 0, False),
                (1030, 1, [1027], 512, 96, 1, True), (259, 1, None, 2048, 96, 0, True)]


def rc_out_case(rpc_all, nclips, valid, K, N, bias, seed=13):
    """Random A (mean about 0.5), lo of about 2^-12.  ref = bias + lo . mean with the float64 mean over the sampled rows R;
    |got - ref| <= sum_k |lo| (|mean| 2^-11 + 2 R u mean|A|) + 2 K u sum_k |lo| |mean| + 2u |ref|:
    the mean's fp16 rounding and its fp32 sum, the product's fp32 sum, the last roundings."""
    g = gen(seed, rpc_all, nclips, K, N)
    M = nclips * rpc_all
    a = torch.rand((M, K), generator=g).to(torch.float16)
    lo = (nrnd(g, (N, K)) * 2.0 ** -12).to(torch.float16)
    bi = nrnd(g, (N,)).float() if bias else None
    A = torch.full((M, K), NAN, dtype=torch.float16)
    mean = torch.empty((nclips, K), dtype=torch.float64)
    mabs = torch.empty((nclips, K), dtype=torch.float64)
    R = torch.empty((nclips, 1), dtype=torch.float64)
    for c in range(nclips):
        rows = rc_clip_rows(rpc_all, valid, c)
        A[rows] = a[rows]
        mean[c] = a[rows].double().mean(0)
        mabs[c] = a[rows].double().abs().mean(0)
        R[c] = len(rows)
    lod = lo.double()
    corr = mean @ lod.T
    ref = corr + (bi.double() if bias else 0.0)
    la = lod.abs()
    bound = (mean.abs() * 2.0 ** -11 + 2 * R * U * mabs) @ la.T + 2 * K * U * (mean.abs() @ la.T) + 2 * U * ref.abs()
    return dict(A=A, a=a, lo=lo, bias=bi, ref=ref, bound=bound, corr=corr)


def rc_out_standin(c, rpc_all, nclips, valid, ignore_valid=False, drop_quarter=False):
    """float32: fp16 means of float32 sums, float32 product.  ignore_valid / drop_quarter: planted defects."""
    K = c["lo"].shape[1]
    out = []
    for cl in range(nclips):
        rows = rc_clip_rows(rpc_all, None if ignore_valid else valid, cl)
        m16 = (c["a"][rows].float().sum(0) / float(len(rows))).to(torch.float16).float()
        lo = c["lo"].float()
        if drop_quarter:
            lo = lo.clone()
            lo[:, 3 * K // 4:] = 0
        out.append(lo @ m16)
    out = torch.stack(out)
    return out + c["bias"] if c["bias"] is not None else out


# ---- pe_project --------------------------------------------------------------------------------------------------------------------
def pe_project_case(S, N, K, with_lo, with_bias, seed=14):
    g = gen(seed, S, N, K, with_lo, with_bias)
    pe = nrnd(g, (S, K)).float()
    w = nrnd(g, (N, K)) / math.sqrt(K)
    wh = w.to(torch.float16)
    wl = (w - wh.double()).to(torch.float16) if with_lo else None
    bi = nrnd(g, (N,)).float() if with_bias else None
    weff = wh.double() + (wl.double() if with_lo else 0.0)
    ref = pe.double() @ weff.T + (bi.double() if with_bias else 0.0)
    bound = 2 * K * U * (pe.double().abs() @ weff.abs().T) + (2 * U * bi.double().abs() if with_bias else 0.0)
    return dict(pe=pe, wh=wh, wl=wl, bias=bi, ref=ref, bound=bound)


def pe_project_standin(c):
    w = c["wh"].float() + (c["wl"].float() if c["wl"] is not None else 0.0)
    y = c["pe"] @ w.T
    return y + c["bias"] if c["bias"] is not None else y


# ---- audio_conv0 -------------------------------------------------------------------------------------------------------------------
AUDIO_TM, AUDIO_F = (1, 2, 3, 4, 7), (1, 5, 80)


def audio_valids(Tm):
    return [None, [Tm, 0, 2], [-3, Tm + 5, 1]]


def audio_conv0_case(Tm, F_, valid, with_lo, d16, seed=15):
    """B = 3.  mel carries NaN in the rows >= valid[b], the packed [32][32] weights (k = 5 kh + kw, kh along time) in the columns 25 .. 31.
    ref: float64 5x5 conv (pad 2) of the mel rounded to 16 bits and zeroed beyond valid, + bias, ReLU, rows >= valid exactly zero;
    |got - ref| <= 2 * 25 u (sum |x| |w| + |bias|)."""
    g = gen(seed, Tm, F_, with_lo, 0 if valid is None else sum(valid) + 100)
    B = 3
    mel = nrnd(g, (B, Tm, F_)).float() * 2
    w = nrnd(g, (32, 25)) / 5
    wh = torch.full((32, 32), NAN, dtype=d16)
    wh[:, :25] = w.to(d16)
    wl = None
    if with_lo:
        wl = torch.full((32, 32), NAN, dtype=d16)
        wl[:, :25] = (w - wh[:, :25].double()).to(d16)
    bi = nrnd(g, (32,)).float()
    Tv = [Tm] * B if valid is None else [min(max(v, 0), Tm) for v in valid]
    x = mel.to(d16).double()
    mel_dev = mel.clone()
    for b in range(B):
        x[b, Tv[b]:] = 0
        mel_dev[b, Tv[b]:] = NAN
    weff = (wh[:, :25].double() + (wl[:, :25].double() if with_lo else 0.0)).reshape(32, 1, 5, 5)
    acc = F.conv2d(x[:, None], weff, padding=2)
    mag = F.conv2d(x[:, None].abs(), weff.abs(), padding=2)
    ref = (acc + bi.double().view(1, 32, 1, 1)).clamp_min(0).permute(0, 2, 3, 1).contiguous()          # (B, Tm, F, 32)
    bound = (2 * 25 * U * (mag + bi.double().abs().view(1, 32, 1, 1))).permute(0, 2, 3, 1).contiguous()
    for b in range(B):
        ref[b, Tv[b]:] = 0
    return dict(mel=mel, mel_dev=mel_dev, wh=wh, wl=wl, bias=bi, ref=ref, bound=bound, Tv=Tv)


def audio_conv0_standin(c, d16, ignore_valid=False):
    B, Tm, _ = c["mel"].shape
    x = c["mel"].to(d16).float()
    Tv = [Tm] * B if ignore_valid else c["Tv"]
    for b in range(B):
        x[b, Tv[b]:] = 0
    w = c["wh"][:, :25].float() + (c["wl"][:, :25].float() if c["wl"] is not None else 0.0)
    y = (F.conv2d(x[:, None], w.reshape(32, 1, 5, 5), padding=2) + c["bias"].view(1, 32, 1, 1)).clamp_min(0).permute(0, 2, 3, 1).contiguous()
    for b in range(B):
        y[b, Tv[b]:] = 0
    return y


# ---- l2norm ------------------------------------------------------------------------------------------------------------------------
def l2norm_case(rows, D, seed=16):
    """x / max(||x||, 1e-12); one row is zero (-> 0).  |got - ref| <= (D/2 + 3) 2u |ref|."""
    g = gen(seed, rows, D)
    x = nrnd(g, (rows, D)).float()
    x[rows // 2] = 0 if rows > 1 else x[0]
    xd = x.double()
    ref = xd / xd.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return dict(x=x, ref=ref, bound=(D / 2 + 3) * 2 * U * ref.abs())


# ---- word_pool / pool_mean ---------------------------------------------------------------------------------------------------------
def pool_case(n, D, seed=17):
    """n consecutive segments of lengths 1, 2, 300, 1, 2 (cut to n) over a (sum, D) fp32 sequence; destination rows in reverse order.
    |got - ref| <= 2 len u mean|x|; a segment of length 1 is an exact copy."""
    lens = [1, 2, 300, 1, 2][:n]
    g = gen(seed, n, D)
    x = nrnd(g, (sum(lens), D)).float()
    off = [0]
    for ln in lens:
        off.append(off[-1] + ln)
    ref = torch.stack([x[off[i]:off[i + 1]].double().mean(0) for i in range(n)])
    bound = torch.stack([2 * lens[i] * U * x[off[i]:off[i + 1]].double().abs().mean(0) for i in range(n)])
    seg = [(off[i], off[i + 1], n - 1 - i) for i in range(n)]
    return dict(x=x, off=off, seg=seg, lens=lens, ref=ref, bound=bound)


def pool_standin(c):
    return torch.stack([c["x"][c["off"][i]:c["off"][i + 1]].mean(0) for i in range(len(c["lens"]))])
