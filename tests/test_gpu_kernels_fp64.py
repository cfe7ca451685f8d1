"""Kernel-level checks of the Linear GEMM, split-operand, fp32 and attention kernels against float64 (run with -m gpu).

Every case runs ONE launch through a production launcher (the jg_debug_* check points of include/jegal_hip.h, with the handle's
options picking the instance as in production) and compares it with float64 torch on the CPU applied to exactly the operands the kernel
received: 16-bit operands are exact in float64, hi+lo weights are summed in float64, the split-operand and fp32 GEMMs see their fp32 A.
The epilogue (scale, bias or per-clip bias, residual row m % res_mod, ReLU / exact GELU, LayerNorm) is applied in float64 too; the
result is rounded to the kernel's output type only where the comparison needs it.

Shapes are chosen to hit tails (M, N, K around the tile edges, K % 64 != 0, strided rows, clip boundaries inside 16-row blocks), not the
model.  Outputs carry >= 128 guard rows and ldc > N guard columns filled with a sentinel bit pattern, A / W carry NaN in the rows and
columns the kernel must not read: a store outside the result or a read outside the operand shows.  All of it stays inside allocations.

The bounds are derived, not measured (u = 2^-24, the fp32 unit roundoff):
  * element-wise, against gross defects (a wrong row or clip, NaN, a missed tile):
        |got - ref| <= 2 K u (|A| |W|^T |scale| + |bias| + |res|)  [+ 1 ulp of ref for 16-bit outputs]
    An fp32 sum of K terms errs by at most ~K u times the sum of their magnitudes; a factor 2 covers the epilogue's few extra
    roundings.  A wrong row / clip / tile is off by O(|ref|), i.e. by far more than K u |A||W| for any K used here (<= 3072: 2e-4).
  * norm-wise for fp32 outputs, against precision-path defects:  ||got - ref|| / ||ref|| <= 2 sqrt(K) u
    Zero-mean random operands make the rounding errors of the sum a random walk (sqrt(K) u).  A dropped lo half of the hi+lo weights
    or a dropped cross term of the split-operand GEMM costs ~2^-12 per product (~1e-4 norm-wise); every such case below computes that
    defect's error on its own operands and asserts it is >= 10x the bound (<= 6.6e-6 at K = 3072), so the bound can see it.
Each case prints observed / bound.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda"
GUARD_ROWS = 128
SENT16 = 0x7D5A            # fp16 / bf16 NaN bit pattern: a value no kernel computes
SENT32 = 0x7FBADBAD
NAN16 = 0x7E00             # the fp16 quiet NaN: what the parts of a tiled plane that no launch may read hold
RATIOS = {}                # family -> worst observed / bound (printed at the end of each test)


def note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio))


# ---- engines ------------------------------------------------------------------------------------------------------------------
_ENGINES = {}


def engine(prec=None, **opts):
    """A handle with exactly these options (everything else at its default), cached per option set."""
    from jegal_amd._lib import Engine
    key = (prec, tuple(sorted(opts.items())))
    if key not in _ENGINES:
        e = Engine(0, precision=prec)
        for k, v in opts.items():
            e.set_option(k, v)
        _ENGINES[key] = e
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def rejects(fn, *a, **kw):
    from jegal_amd._lib import JG_ERR_ARG, JegalError
    with pytest.raises(JegalError) as ei:
        fn(*a, **kw)
    return ei.value.code == JG_ERR_ARG


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def dt16(bf):
    return torch.bfloat16 if bf else torch.float16


def operand(x, ld, dtype, extra_rows=16):
    """x (rows, cols) -> device buffer [rows + extra_rows][ld] of dtype with NaN in every element outside x."""
    r, c = x.shape
    buf = torch.full((r + extra_rows, ld), float("nan"), dtype=dtype)
    buf[:r, :c] = x.to(dtype)
    return buf.to(DEV)


def guarded(rows, ld, dtype):
    """Output buffer [rows + GUARD_ROWS][ld] filled with the sentinel bit pattern."""
    if dtype == torch.float32:
        return torch.full((rows + GUARD_ROWS, ld), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full((rows + GUARD_ROWS, ld), SENT16, dtype=torch.int16, device=DEV).view(dtype)


def guards_intact(buf, rows, cols):
    b = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16).cpu()
    s = SENT32 if buf.dtype == torch.float32 else SENT16
    return bool((b[rows:] == s).all()) and bool((b[:rows, cols:] == s).all())


def ulp16(x, bf=False):
    """One ulp of |x| in fp16 (bf16): 2^(floor(log2|x|) - 10 (7)), at least the smallest subnormal step."""
    mant, lo = (7, -133) if bf else (10, -24)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -60)))
    return torch.exp2((e - mant).clamp_min(lo))


def urnd(g, shape, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def nrm_ratio(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


# ---- Linear GEMM (launch_gemm) ---------------------------------------------------------------------------------------------------
# every non-conv Linear instance launch_gemm can reach (the instance table of jegal_amd/csrc/gemm_plan.h): gemm_glds_kernel<W2,CONV,MI,WM,WN,LNF,SPR,XE,C32>, gemm_kernel<WM,WN,CONV,W2>
LINEAR_INSTANCES = {
    "gemm_glds_kernel<0,0,2,4,2,0,0,0,0>", "gemm_glds_kernel<1,0,2,4,2,0,0,0,0>",          # 128x128
    "gemm_glds_kernel<0,0,4,4,2,0,0,0,0>", "gemm_glds_kernel<1,0,4,4,2,0,0,0,0>",          # 256x128
    "gemm_glds_kernel<0,0,8,2,4,0,1,0,0>", "gemm_glds_kernel<0,0,8,2,4,0,0,0,0>",          # 256x256 (SPR: K <= 1024)
    "gemm_glds_kernel<0,0,8,1,8,1,0,0,0>",                                                 # residual + LayerNorm fused, 128x512
    # implicit-LayerNorm consumer (XE = 1) and producer (XE = 2) epilogues
    "gemm_glds_kernel<1,0,2,4,2,0,0,1,0>", "gemm_glds_kernel<1,0,4,4,2,0,0,1,0>", "gemm_glds_kernel<0,0,2,4,2,0,0,1,0>",
    "gemm_glds_kernel<0,0,8,2,4,0,1,1,0>", "gemm_glds_kernel<0,0,8,2,4,0,0,1,0>",
    "gemm_glds_kernel<1,0,2,4,2,0,0,2,0>", "gemm_glds_kernel<1,0,4,4,2,0,0,2,0>", "gemm_glds_kernel<0,0,2,4,2,0,0,2,0>",
    "gemm_glds_kernel<0,0,8,2,4,0,1,2,0>", "gemm_glds_kernel<0,0,8,2,4,0,0,2,0>",
    # register-staged: N <= 64 (4x1 waves) and whatever the LDS-DMA conditions reject (2x2), single / hi+lo weights
    "gemm_kernel<4,1,0,0>", "gemm_kernel<4,1,0,1>", "gemm_kernel<2,2,0,0>", "gemm_kernel<2,2,0,1>",
}
SEEN = set()


def planned(kw, opts=None):
    """The GEMM planner's answer for one debug_gemm_check argument set under these engine options: asked without a launch."""
    from jegal_amd._lib import gemm_plan
    return gemm_plan(num_cu=torch.cuda.get_device_properties(0).multi_processor_count, opts=opts, **kw)[0]


def gemm_case(name, M, N, K, *, w2=False, out="f32", lda=None, ldw=None, ldc=None, scale=False, bias=True, res=False, res_mod=0,
              relu=0, bias_clip=None, bf=False, opts=None, seed=0, tiled=False):
    """One plain / per-clip-bias Linear launch vs float64.  bias_clip = (rpc, nclips).  tiled: A is handed over as the tiled token plane
    (a_tiled; K = 512) of whole 128-row tiles plus one guard tile, with NaN bits in the rows >= M of the last tile and in the guard tile."""
    g = torch.Generator().manual_seed(seed)
    assert not tiled or (K == 512 and lda in (None, 512)), "the tiled token plane has 512 columns"
    lda, ldw = lda or K, ldw or K
    ldc = ldc or N + 8                                  # guard columns
    d16 = dt16(bf)
    a = urnd(g, (M, K)).to(d16).double()
    w = urnd(g, (N, K)) / math.sqrt(K) * 2
    wh = w.to(d16).double()
    wl = (w - wh).to(d16).double() if w2 else None
    weff = wh + (wl if w2 else 0.0)
    sc = urnd(g, (N,), 0.5, 1.5).float() if scale else None
    bi = urnd(g, (N,)).float() if bias else None
    rm = res_mod or M
    rs = urnd(g, (rm, N)).float() if res else None
    bc = None
    if bias_clip:
        rpc, ncl = bias_clip
        bc = (urnd(g, (ncl, N), -2, 2)).float()          # O(1) differences between the clips' vectors
    e = engine(prec=4 if bf else None, **(opts or {}))
    if tiled:
        from elementwise_fp64_cases import tiled_plane          # (imports this module: not at the top)
        A = tiled_plane(a.to(d16), (M + 127) // 128 * 65536 + 65536, NAN16).view(d16).to(DEV)
    else:
        A = operand(a, lda, d16)
    Wh = operand(wh, ldw, d16)
    Wl = operand(wl, ldw, d16) if w2 else None
    o32 = guarded(M, ldc, torch.float32) if out in ("f32", "both") else None
    o16 = guarded(M, ldc, d16) if out in ("f16", "both") else None
    kw = dict(A=A, lda=lda, Wh=Wh, ldw=ldw, M=M, N=N, K=K, relu=relu, ldc=ldc)
    if tiled:
        kw["a_tiled"] = 1
    if w2:
        kw["Wl"] = Wl
    if sc is not None:
        kw["scale"] = sc.to(DEV)
    if bc is not None:
        kw.update(bias_clip=bc.to(DEV), rpc=bias_clip[0], nclips=bias_clip[1])
    elif bi is not None:
        kw["bias"] = bi.to(DEV)
    if rs is not None:
        kw.update(res=rs.to(DEV), ldr=N, res_mod=res_mod)
    if o32 is not None:
        kw["out32"] = o32
    if o16 is not None:
        kw["out16"] = o16
    e.debug_gemm_check(**kw)
    torch.cuda.synchronize()
    kname = e.debug_last_kernel()
    assert kname == planned(kw, opts), f"{name}: launched {kname}, the planner says {planned(kw, opts)}"
    SEEN.add(kname)

    acc = a @ weff.T
    mag = a.abs() @ weff.abs().T
    if sc is not None:
        acc, mag = acc * sc.double(), mag * sc.double().abs()
    rows = torch.arange(M)
    if bc is not None:
        badd = bc.double()[torch.clamp(rows // bias_clip[0], max=bias_clip[1] - 1)]
    elif bi is not None:
        badd = bi.double().expand(M, N)
    else:
        badd = torch.zeros(M, N, dtype=torch.float64)
    radd = rs.double()[rows % rm] if rs is not None else torch.zeros(M, N, dtype=torch.float64)
    v = acc + badd + radd
    eb = 2 * K * U * (mag + badd.abs() + radd.abs())
    if relu == 1:
        v = v.clamp_min(0)
    elif relu == 2:
        v = 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))
        eb = eb * 1.13 + 4 * U * v.abs()             # GELU's slope is <= 1.13; erff adds a few ulp
    fails = []
    worst = 0.0
    for buf, is16 in ((o32, False), (o16, True)):
        if buf is None:
            continue
        if not guards_intact(buf, M, N):
            fails.append(f"{name}: guard {'16' if is16 else '32'} overwritten")
        got = buf[:M, :N].double().cpu()
        bound = eb + (ulp16(v, bf) if is16 else 0)
        r = float(((got - v).abs() / bound).max()) if got.isfinite().all() else float("inf")
        worst = max(worst, r)
        if not is16:
            nb = 2 * math.sqrt(K) * U
            rn = nrm_ratio(got, v) / nb
            worst = max(worst, rn)
            if w2:          # the defect this bound exists for: the lo half dropped
                drop = nrm_ratio(v - (a @ wl.T) * (sc.double() if sc is not None else 1), v)
                assert drop >= 10 * nb, f"{name}: bound {nb:.2e} too loose to see a dropped lo half ({drop:.2e})"
    note("linear", worst)
    print(f"{name:36s} {kname:40s} M={M} N={N} K={K} observed/bound {worst:.3f}")
    if worst > 1:
        fails.append(f"{name}: observed/bound {worst:.3f} ({kname})")
    return fails


# (name, M, N, K, kwargs): every instance, the tails of every dimension, every option of the GEMM dispatcher
GEMM_CASES = [
    ("staged_m1", 1, 128, 512, dict(out="f32", res=True)),
    ("staged_w2_m15_strided", 15, 384, 768, dict(w2=True, out="both", lda=776, ldc=392, scale=True)),
    ("narrow_m16", 16, 64, 1024, dict(out="f32", res=True, relu=1)),
    ("narrow_w2_k200", 17, 64, 200, dict(w2=True, out="f16")),
    ("staged_k80_resmod", 127, 512, 80, dict(out="both", res=True, res_mod=21, ldc=520)),
    ("staged_w2_nomulti128", 255, 192, 512, dict(w2=True, out="f32", relu=2)),
    ("glds_off", 257, 256, 512, dict(out="f32", opts=dict(gemm_glds=0))),
    ("t128", 128, 128, 64, dict(out="f32", opts=dict(gemm_tile=1))),
    ("t128_w2_mtail", 129, 768, 512, dict(w2=True, out="f32", res=True, opts=dict(gemm_tile=1))),
    ("t128_k3072", 129, 128, 3072, dict(w2=True, out="f32", opts=dict(gemm_tile=1))),
    ("t256x128_f16", 255, 1536, 1024, dict(out="f16", opts=dict(gemm_tile=2))),
    ("t256x128_w2_resmod", 257, 384, 768, dict(w2=True, out="both", res=True, res_mod=21, lda=784, ldc=392, opts=dict(gemm_tile=2))),
    ("t256x256_spr", 1023, 512, 512, dict(out="f16", scale=True, opts=dict(gemm_tile=3))),
    ("t256x256_k2048", 4800, 256, 2048, dict(out="f32", res=True, res_mod=4800 // 2, opts=dict(gemm_tile=3))),
    ("auto_jegal", 4800, 512, 512, dict(w2=True, out="f32", res=True, res_mod=100)),
    ("auto_big", 1024, 768, 768, dict(out="both", relu=1)),
    ("n2304_w2", 257, 2304, 512, dict(w2=True, out="f32", res=True, opts=dict(gemm_tile=2))),
    ("n2304_auto", 300, 2304, 768, dict(out="f16", scale=True)),
    ("persistent_off", 1023, 256, 512, dict(out="f32", opts=dict(gemm_persistent=0, gemm_tile=2))),
    ("counted_off_stagger", 1029, 512, 512, dict(out="f16", opts=dict(gemm_counted=0, gemm_stagger=500, num_cu=8))),
    ("stagger_off_numcu", 1029, 384, 512, dict(w2=True, out="f32", opts=dict(gemm_stagger=-1, num_cu=13))),
    ("small_big_off", 640, 512, 512, dict(out="f32", opts=dict(gemm_small_tile=0, gemm_big_tile=0))),
    ("numcu8_rounds", 1151, 256, 1024, dict(out="both", res=True, opts=dict(num_cu=8, gemm_tile=1))),
    # per-clip bias: clip boundaries inside 16-row blocks, tiles straddling them, the last clip's index clamped
    ("clip_rpc256", 640, 256, 512, dict(out="f16", bias_clip=(256, 2), opts=dict(gemm_tile=2))),
    ("clip_rpc257_t128", 811, 384, 512, dict(w2=True, out="f16", bias_clip=(257, 3), opts=dict(gemm_tile=1))),
    ("clip_rpc1029_big", 2100, 512, 512, dict(out="f16", bias_clip=(1029, 2), opts=dict(gemm_tile=3))),
    ("clip_rpc3150", 3150 * 2 + 17, 512, 512, dict(out="f16", relu=1, bias_clip=(3150, 2))),
]


def ln_fused_case(M, clip=None, seed=1, inplace=False):
    """Residual + LayerNorm fused (N = 512): the token plane in the tiled order of common.h, built here from that description.
    inplace: out16 is the res16 plane itself, as the fused transformer passes it; the reference keeps the host copy of the plane, the guard
    tile must keep the bits it was given, rows >= M inside the last 128-row tile are unspecified afterwards."""
    N, K = 512, 512
    g = torch.Generator().manual_seed(seed)
    e = engine()
    a = urnd(g, (M, K)).half().double()
    wh = (urnd(g, (N, K)) / math.sqrt(K) * 2).half().double()
    bias = urnd(g, (N,)).float()
    gam, bet = urnd(g, (N,), 0.5, 1.5).float(), urnd(g, (N,)).float()
    R = (M + 127) // 128
    m = np.arange(R * 128)[:, None]
    n = np.arange(N)[None, :]
    off16 = (m >> 7) * 65536 + (n >> 6) * 8192 + ((m & 127) >> 4) * 1024 + ((n & 63) >> 4) * 256 + (m & 15) * 16 + (n & 15)
    assert np.unique(off16).size == off16.size == R * 65536
    r16 = urnd(g, (R * 128, N), -2, 2).half()
    r16[M:] = float("nan")                                   # rows past M in the last tile: read, never part of a valid row
    res = r16.double()
    plane16 = torch.empty(R * 65536 + 65536, dtype=torch.float16)
    plane16[torch.from_numpy(off16.ravel())] = r16.ravel()
    plane16[R * 65536:] = float("nan")
    kw = dict(A=operand(a, K, torch.float16), lda=K, Wh=operand(wh, K, torch.float16), ldw=K, M=M, N=N, K=K, bias=bias.to(DEV),
              ln_w=gam.to(DEV), ln_b=bet.to(DEV), res16=plane16.to(DEV))
    out16 = kw["res16"] if inplace else torch.full((R * 65536 + 65536,), SENT16, dtype=torch.int16, device=DEV).view(torch.float16)
    guard_bits = plane16.view(torch.int16)[R * 65536:].clone() if inplace else torch.full((65536,), SENT16, dtype=torch.int16)
    kw["out16"] = out16
    rows = torch.arange(M)
    if clip:
        rpc, ncl = clip
        bc = urnd(g, (ncl, N), -2, 2).float()
        kw.update(bias_clip=bc.to(DEV), rpc=rpc, nclips=ncl)
        badd = bc.double()[torch.clamp(rows // rpc, max=ncl - 1)]
    else:
        badd = bias.double().expand(M, N)
    e.debug_gemm_check(**kw)
    torch.cuda.synchronize()
    kname = e.debug_last_kernel()
    assert kname == planned(kw), f"ln_fused M={M}: launched {kname}, the planner says {planned(kw)}"
    SEEN.add(kname)
    x = a @ wh.T + badd + res[:M]
    mu = x.mean(1, keepdim=True)
    sig = ((x - mu) ** 2).mean(1, keepdim=True).add(1e-5).sqrt()
    xh = (x - mu) / sig
    y = xh * gam.double() + bet.double()
    ex = 2 * K * U * ((a.abs() @ wh.abs().T) + badd.abs() + res[:M].abs())
    # LayerNorm of x + dx: the mean moves by <= max|dx|, sigma relatively by <= max|dx| / sigma, so
    # |dy| <= |gamma| (|dx| + max|dx| (1 + |xhat|)) / sigma, plus fp32 roundings of the statistics (~2^-20 |gamma xhat|)
    emax = ex.max(1, keepdim=True).values
    ey = gam.double().abs() * (ex + emax * (1 + xh.abs())) / sig + 2.0 ** -20 * (gam.double() * xh).abs() + 2 * U * y.abs()
    o16 = out16.cpu()
    got = o16[torch.from_numpy(off16[:M].ravel())].view(M, N).double()
    ratio = float(((got - y).abs() / (ey + ulp16(y))).max()) if got.isfinite().all() else float("inf")
    fails = []
    if not torch.equal(o16.view(torch.int16)[R * 65536:], guard_bits):
        fails.append("ln_fused: guard tile of out16 overwritten")
    note("ln_fused", ratio)
    print(f"ln_fused M={M} clip={clip}{' in place' if inplace else ''} {kname} observed/bound {ratio:.3f}")
    if ratio > 1:
        fails.append(f"ln_fused M={M} clip={clip}{' in place' if inplace else ''}: observed/bound {ratio:.3f}")
    return fails


def implicit_ln_case(mode, M, N, K, w2, tile, seed=2, inplace=False):
    """ln_mode 1 (consumer) / 2 (producer) of the implicit-LayerNorm token stream (GemmArgs::ln_mode, common.h).
    inplace (ln_mode 2): out16 is the xres_hi buffer and out_lo the xres_lo buffer, as engine::gemm passes them; their guard rows and guard
    columns must keep the (NaN) bits they were given, compared with a clone taken before the launch."""
    assert mode == 2 or not inplace
    g = torch.Generator().manual_seed(seed)
    e = engine(gemm_tile=tile)
    a = (urnd(g, (M, K)) + 0.5).half().double()              # un-normalised rows with a mean of their own
    w = urnd(g, (N, K)) / math.sqrt(K) * 2
    wh = w.half().double()
    wl = (w - wh).half().double() if w2 else None
    weff = wh + (wl if w2 else 0.0)
    ldc = N + 8
    kw = dict(A=operand(a, K, torch.float16), lda=K, Wh=operand(wh, K, torch.float16), ldw=K, M=M, N=N, K=K, ldc=ldc, ln_mode=mode)
    if w2:
        kw["Wl"] = operand(wl, K, torch.float16)
    bias = urnd(g, (N,)).float()
    acc = a @ weff.T
    mag = a.abs() @ weff.abs().T
    out16 = guarded(M, ldc, torch.float16)
    kw.update(bias=bias.to(DEV), out16=out16)
    fails = []
    if mode == 1:
        mean = a.mean(1).float()
        rstd = (1 / (a.var(1, unbiased=False) + 1e-5).sqrt()).float()
        c1 = weff.sum(1).float()                              # column sums of the folded weights
        kw.update(scale=c1.to(DEV), ln_stats=torch.stack([mean, rstd], 1).contiguous().to(DEV))
        r, mu = rstd.double()[:, None], mean.double()[:, None]
        v = r * (acc - mu * c1.double()) + bias.double()
        eb = 2 * K * U * (r * (mag + (mu * c1.double()).abs()) + bias.double().abs())
    else:
        xh = urnd(g, (M, N), -3, 3).half()
        xl = ((urnd(g, (M, N), -3, 3) - xh.double()) * 2.0 ** -11).half()
        xp = xh.double() + xl.double()
        mean = xp.mean(1).float()
        rstd = (1 / (xp.var(1, unbiased=False) + 1e-5).sqrt()).float()
        gam = urnd(g, (N,), 0.5, 1.5).float()
        xres_hi = operand(xh.double(), ldc, torch.float16, extra_rows=GUARD_ROWS if inplace else 16)
        xres_lo = operand(xl.double(), ldc, torch.float16, extra_rows=GUARD_ROWS if inplace else 16)
        if inplace:
            before = (xres_hi.clone(), xres_lo.clone())
            out16 = kw["out16"] = xres_hi
        lo = xres_lo if inplace else guarded(M, ldc, torch.float16)
        stat = guarded(M, N // 64 * 2, torch.float32)
        kw.update(scale=gam.to(DEV), ln_stats=torch.stack([mean, rstd], 1).contiguous().to(DEV), xres_hi=xres_hi, xres_lo=xres_lo, out_lo=lo,
                  stat_out=stat)
        nrm = gam.double() * rstd.double()[:, None] * (xp - mean.double()[:, None])
        v = acc + bias.double() + nrm
        eb = 2 * K * U * (mag + bias.double().abs() + nrm.abs())
    e.debug_gemm_check(**kw)
    torch.cuda.synchronize()
    kname = e.debug_last_kernel()
    assert kname == planned(kw, dict(gemm_tile=tile)), f"ln_mode {mode}: launched {kname}, the planner says {planned(kw, dict(gemm_tile=tile))}"
    SEEN.add(kname)
    hi = out16[:M, :N].double().cpu()
    ratio = float(((hi - v).abs() / (eb + ulp16(v))).max()) if hi.isfinite().all() else float("inf")
    def guards_kept(buf, was):          # in place: the rows >= M and the columns >= N hold what they held before the launch
        b, w = buf.view(torch.int16).cpu(), was.view(torch.int16).cpu()
        return torch.equal(b[M:], w[M:]) and torch.equal(b[:M, N:], w[:M, N:])
    if not (guards_kept(out16, before[0]) if inplace else guards_intact(out16, M, N)):
        fails.append(f"ln_mode {mode}: out16 guard overwritten")
    if mode == 2:
        got = hi + lo[:M, :N].double().cpu()
        ratio = max(ratio, float(((got - v).abs() / (eb + 2.0 ** -21 * v.abs() + 2.0 ** -24)).max()))
        s1 = v.view(M, N // 64, 64).sum(2)
        s2 = (v * v).view(M, N // 64, 64).sum(2)
        eb64 = eb.view(M, N // 64, 64)
        av = v.abs().view(M, N // 64, 64)
        gs = stat[:M, :N // 64 * 2].double().cpu().view(M, N // 64, 2)
        b1 = (eb64 + 64 * U * av).sum(2)
        b2 = (2 * av * eb64 + 64 * U * av * av).sum(2)
        ratio = max(ratio, float(((gs[..., 0] - s1).abs() / b1).max()), float(((gs[..., 1] - s2).abs() / b2).max()))
        if not (guards_kept(lo, before[1]) if inplace else guards_intact(lo, M, N)) or not guards_intact(stat, M, N // 64 * 2):
            fails.append("ln_mode 2: out_lo / stat_out guard overwritten")
    note(f"ln_mode{mode}", ratio)
    print(f"ln_mode={mode} M={M} N={N} K={K} w2={w2} tile={tile}{' in place' if inplace else ''} {kname} observed/bound {ratio:.3f}")
    if not ratio <= 1:
        fails.append(f"ln_mode {mode} M={M} N={N} w2={w2} tile={tile}{' in place' if inplace else ''}: observed/bound {ratio:.3f} ({kname})")
    return fails


def test_linear_gemm_kernels_vs_fp64_and_instance_coverage():
    fails = []
    for name, M, N, K, kw in GEMM_CASES:
        fails += gemm_case(name, M, N, K, **kw)
    for M, clip in ((1029, None), (1153, (300, 3)), (1100, (256, 4))):
        fails += ln_fused_case(M, clip)
    for mode in (1, 2):
        for w2, tile in ((True, 1), (True, 2), (False, 1), (False, 3)):
            fails += implicit_ln_case(mode, 257, 512, 512, w2, tile)
        fails += implicit_ln_case(mode, 1029, 768, 1024, False, 3)      # 256x256, K <= 1024: the SPR instance
        fails += implicit_ln_case(mode, 1029, 768, 2048, False, 3)      # K > 1024: the plain 256x256 instance
    print("worst observed/bound:", {k: round(v, 3) for k, v in RATIOS.items()})
    assert not fails, "\n".join(fails)
    missing, extra = LINEAR_INSTANCES - SEEN, SEEN - LINEAR_INSTANCES
    assert not missing and not extra, f"instances never run: {sorted(missing)}; not in the list: {sorted(extra)}"


def test_bf16_build_linear_reduced_grid():
    fails = []
    for name, M, N, K, kw in (("bf_staged", 17, 64, 200, dict(out="f16")), ("bf_t128_w2", 129, 384, 512, dict(w2=True, out="f32", opts=dict(gemm_tile=1))),
                              ("bf_t256", 1023, 512, 512, dict(out="both", res=True, res_mod=21)),
                              ("bf_big", 1029, 512, 2048, dict(out="f32", opts=dict(gemm_tile=3)))):
        fails += gemm_case(name, M, N, K, bf=True, **kw)
    assert not fails, "\n".join(fails)


def test_gemm_launcher_rejections():
    """Shapes the launchers refuse on purpose come back as JG_ERR_ARG (nothing is launched): pins the rules."""
    e = engine()
    z16 = torch.zeros(2048 * 1024, dtype=torch.float16, device=DEV)
    z32 = torch.zeros(2048 * 1024, dtype=torch.float32, device=DEV)
    base = dict(A=z16, lda=512, Wh=z16, ldw=512, M=256, N=256, K=512, ldc=256)
    bad = [
        dict(base, N=64, ldc=64, bias_clip=z32, rpc=256, nclips=1, out16=z16),          # per-clip bias: N = 64
        dict(base, bias_clip=z32, rpc=255, nclips=1, out16=z16),                         # rpc < 256
        dict(base, bias_clip=z32, rpc=256, nclips=1, out32=z32),                          # per-clip bias with an fp32 output
        dict(base, bias_clip=z32, rpc=256, nclips=1, out16=z16, res=z32, ldr=256),        # ... or a residual
        dict(base, M=1000, N=512, ldc=512, ln_w=z32, ln_b=z32, res16=z16, out16=z16),    # LayerNorm-fused with M < 1024
        dict(base, M=1024, N=384, ldc=384, ln_w=z32, ln_b=z32, res16=z16, out16=z16),    # ... with N != 512
        dict(base, ln_mode=1, ln_stats=z32, scale=z32, bias=z32, out16=z16, M=100),        # implicit LayerNorm: M < 128
        dict(base, ln_mode=1, ln_stats=z32, scale=z32, bias=z32, out32=z32),               # ... fp32 output
        dict(base, ln_mode=2, ln_stats=z32, scale=z32, bias=z32, out16=z16),               # producer without its planes
        dict(base, K=70, lda=72, ldw=72, out32=z32),                                      # register-staged: K % 8 != 0
        dict(base, M=100, lda=516, out32=z32),                                             # register-staged: lda % 8 != 0
        dict(base, out32=z32, ldc=258),                                                    # ldc % 4 != 0
    ]
    for kw in bad:
        assert rejects(e.debug_gemm_check, **kw), kw
        assert e.debug_last_kernel() == ""
        assert planned(kw) == "rejected", kw
    assert rejects(e.debug_gemm_x3, z32, 200, z16, z16, 200, 64, 128, 200, z32, 128)          # x3: K % 256 != 0
    assert rejects(e.debug_gemm_x3, z32, 256, z16, z16, 256, 64, 64, 256, z32, 64)            # x3: N % 128 != 0
    assert rejects(e.debug_attention_gather, z16, z16, 4, 8, 2, 8, 33, 8, z16)               # gather: S > 32
    # dk not 64 / 96: refused by jg_debug_attention's own argument check (launch_attention has no such rule to pin: it would fall to
    # the VALU kernel and return hipErrorInvalidValue there)
    assert rejects(e.debug_attention, z16, None, 2, 16, 8, 80, z16)


# ---- split-operand and fp32 GEMMs ------------------------------------------------------------------------------------------------
def x3_case(M, N, K, scale=1.0, res_mod=0, relu=0, lda=None, ldc=None, seed=3):
    g = torch.Generator().manual_seed(seed)
    e = engine()
    lda, ldc = lda or K, ldc or N
    a = (urnd(g, (M, K)) * scale).float().double()
    w = urnd(g, (N, K)) / math.sqrt(K) * 2
    wh = w.half().double()
    wl = (w - wh).half().double()
    bias = urnd(g, (N,)).float()
    rm = res_mod or M
    rs = urnd(g, (rm, N)).float() * scale
    out = guarded(M, ldc, torch.float32)
    e.debug_gemm_x3(operand(a, lda, torch.float32), lda, operand(wh, K, torch.float16), operand(wl, K, torch.float16), K, M, N, K, out, ldc,
                    bias=bias.to(DEV) * scale, res=rs.to(DEV), ldr=N, res_mod=res_mod, relu=relu)
    torch.cuda.synchronize()
    assert e.debug_last_kernel() == "gemm_x3_kernel"
    weff = wh + wl
    pre = a @ weff.T + bias.double() * scale + rs.double()[torch.arange(M) % rm]
    act = (lambda x: x.clamp_min(0)) if relu else (lambda x: x)
    v = act(pre)
    got = out[:M, :N].double().cpu()
    eb = 2 * K * U * (a.abs() @ weff.abs().T + abs(scale) * (bias.double().abs() + rs.double()[torch.arange(M) % rm].abs()))
    nb = 2 * math.sqrt(K) * U
    r_el = float(((got - v).abs() / eb).max()) if got.isfinite().all() else float("inf")
    r_n = nrm_ratio(got, v) / nb
    # the defects this bound exists for: the A-lo x W-hi cross term dropped (A rounded to fp16), the lo weights dropped
    ahi = a.half().double()
    for what, alt in (("cross term", pre - (a - ahi) @ weff.T), ("lo weights", pre - a @ wl.T)):
        d = nrm_ratio(act(alt), v)
        assert d >= 10 * nb, f"x3 bound {nb:.2e} too loose to see a dropped {what} ({d:.2e})"
    assert guards_intact(out, M, N)
    # the output error the loader's split alone causes on these operands (hi = fp16(a), lo = fp16(a - hi), emulated exactly)
    af = a.float()
    hi = af.half().float()
    split = (hi + (af - hi).half().float()).double()
    split_rel = nrm_ratio(pre - (a - split) @ weff.T, pre)
    return r_el, r_n, split_rel


def test_gemm_x3_vs_fp64():
    worst = 0.0
    for M, N, K, rm, relu, lda, ldc in ((1, 128, 256, 0, 0, None, None), (33, 512, 512, 21, 1, 516, 520), (1001, 512, 1024, 21, 0, None, None),
                                        (4817, 256, 512, 4800 // 2, 0, None, None), (129, 256, 3072, 0, 1, None, None)):
        r_el, r_n, _ = x3_case(M, N, K, res_mod=rm, relu=relu, lda=lda, ldc=ldc)
        print(f"gemm_x3 M={M} N={N} K={K} elementwise {r_el:.3f} normwise {r_n:.3f}")
        worst = max(worst, r_el, r_n)
    note("gemm_x3", worst)
    assert worst <= 1, worst


# Operand scale of the split A = fp16(a) + fp16(a - fp16(a)) (gemm_x3.hip): once |a| < ~2^-3 the lo half is subnormal in fp16 and carries
# an ABSOLUTE quantum of 2^-24 (error <= 2^-25 per element), so the norm-wise error of a row is ~2^-25 / rms(a): within the 2 sqrt(K) u
# bound while the rows' rms is >= ~2^-7 at K = 512; |a| >= 65520 overflows the hi half.
# The activations at the engine's gemm_x3 call sites (proj_ip_rgb on the GestSync features, the LayerNorm / ReLU outputs in front of
# proj_ip_rgb.3, proj_op_rgb, proj_op_text and the align MLPs, the fusion / align MLPs of the content path; the measured set also
# takes in the encoder feed-forward Linears as a wider envelope), measured on the CPU oracle over the six weight families by tools/x3_operand_range.py
# (profiles/x3_operand_range.json): per-row rms 0.69 .. ~9, max |a| 42.3; the split itself costs at most 0.018 of the bound there.
# The grid below -- uniform operands in +-2^s, row rms 2^s / sqrt 3 -- spans rms 0.009 .. 591 and |a| up to 1024, i.e. that range with
# margin on both sides, and holds the kernel to the fp32 bound over all of it.  No pre-scale of the split is needed at these call sites.
X3_GRID = [-6, 0, 6, 10]


@pytest.mark.parametrize("scale_log2", X3_GRID)
def test_gemm_x3_operand_scale_fp32_grade(scale_log2):
    r_el, r_n, _ = x3_case(257, 256, 512, scale=2.0 ** scale_log2, res_mod=0)
    print(f"gemm_x3 A scale 2^{scale_log2}: elementwise {r_el:.3f} normwise {r_n:.3f}")
    note("gemm_x3_scale", max(r_el, r_n))
    assert r_el <= 1 and r_n <= 1


def test_gemm_x3_grid_covers_the_measured_call_site_range():
    """The committed measurement of the call sites' activations lies inside the scale grid above (host-side check of the claim)."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "x3_operand_range.json")) as f:
        summ = json.load(f)["summary"]["with_ffn"]
    lo_rms, hi_abs = 2.0 ** min(X3_GRID) / math.sqrt(3), 2.0 ** max(X3_GRID)
    assert lo_rms <= summ["rms_min"] and summ["max_abs"] <= hi_abs, (summ, lo_rms, hi_abs)
    assert summ["worst_split_over_bound"] < 0.1


def test_gemm_x3_small_operands_absolute_quantum():
    """Documents the limit below the fp32-grade range (A uniform in +-2^-12, row rms 2^-12 / sqrt 3): there the split's subnormal lo half
    dominates.  Its error is emulated exactly on the same operands (split_rel); the kernel may add its fp32 accumulation error on top
    (2 sqrt(K) u) and nothing more.  At this scale split_rel (~2^-25 / (2^-12 / sqrt 3) / sqrt 3 = 2^-13) is of the order of a dropped
    cross term (~2^-12), so this case does not guard against that defect -- the fp32-grade cases above do."""
    M, N, K = 257, 256, 512
    r_el, r_n, split_rel = x3_case(M, N, K, scale=2.0 ** -12)
    nb = 2 * math.sqrt(K) * U
    rel = r_n * nb
    print(f"gemm_x3 A scale 2^-12: normwise {rel:.2e}, the split alone {split_rel:.2e} (+ fp32 bound {nb:.2e})")
    assert rel <= split_rel + nb


def gemm32_case(M, N, K, act, res_mod, lda, ldc, seed=4):
    g = torch.Generator().manual_seed(seed)
    e = engine()
    a = urnd(g, (M, K)).float().double()
    w = (urnd(g, (N, K)) / math.sqrt(K) * 2).float().double()
    sc = urnd(g, (N,), 0.5, 1.5).float()
    bias = urnd(g, (N,)).float()
    rm = res_mod or M
    rs = urnd(g, (rm, N)).float()
    out = guarded(M, ldc, torch.float32)
    e.debug_gemm32(operand(a, lda, torch.float32), lda, operand(w, K, torch.float32), K, M, N, K, out, ldc, scale=sc.to(DEV),
                   bias=bias.to(DEV), res=rs.to(DEV), ldr=N, res_mod=res_mod, act=act)
    torch.cuda.synchronize()
    kname = e.debug_last_kernel()
    radd = rs.double()[torch.arange(M) % rm]
    v = (a @ w.T) * sc.double() + bias.double() + radd
    eb = 2 * K * U * ((a.abs() @ w.abs().T) * sc.double() + bias.double().abs() + radd.abs())
    if act == 1:
        v = v.clamp_min(0)
    elif act == 2:
        v = 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))
        eb = eb * 1.13 + 4 * U * v.abs()
    got = out[:M, :N].double().cpu()
    r = max(float(((got - v).abs() / eb).max()) if got.isfinite().all() else float("inf"), nrm_ratio(got, v) / (2 * math.sqrt(K) * U))
    assert guards_intact(out, M, N)
    return r, kname


def test_gemm32_vs_fp64():
    worst, seen = 0.0, set()
    for M, N, K, act, rm, lda, ldc in ((1, 64, 80, 0, 0, 80, 64), (31, 130, 515, 1, 7, 517, 131), (255, 512, 1024, 2, 21, 1024, 516),
                                       (1029, 768, 768, 0, 100, 772, 768), (6400, 1024, 64, 1, 0, 64, 1024),
                                       (6400, 1024, 66, 0, 0, 67, 1024)):          # 400 tiles of 128 x 128 with K % 4 != 0 and lda % 4 != 0
        r, kname = gemm32_case(M, N, K, act, rm, lda, ldc)
        seen.add(kname)
        print(f"gemm32 M={M} N={N} K={K} act={act} {kname} observed/bound {r:.3f}")
        worst = max(worst, r)
    note("gemm32", worst)
    assert worst <= 1, worst
    assert {"gemm32_kernel<0,0,64>", "gemm32_kernel<0,1,64>", "gemm32_kernel<0,1,128>", "gemm32_kernel<0,0,128>"} == seen, seen


# ---- attention ------------------------------------------------------------------------------------------------------------------
# Bound for 16-bit outputs: |got - ref| <= 2^-9 max_j |v_j| per row (the max over the keys the reference weights, p_j > 0).
# The MFMA kernels round the probabilities once to the 16-bit type before P V (relative 2^-11 each: <= 2^-11 sum p_j |v_j|), normalise
# with the fp32 sum of the unrounded ones (another <= 2^-11 max|v|), and round the output once (<= 2^-11 |out| <= 2^-11 max|v|); the
# fp32 scores of 16-bit q, k (|q k| / sqrt(dk) <= 8 here) are good to ~1e-6.  3 x 2^-11 < 2^-9.  A masked key that leaks carries v = 1e4
# and a large score, so a leak costs O(1) max|v| -- far outside; a read beyond S meets NaN rows.  bf16: 2^-6 (8 bits instead of 11).
def attn_ref(q, k, v, mask, dk):
    """float64 softmax attention (masked_fill(mask == 0, -1e9)) -> (out, per query the max |v| over the keys it weights)."""
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) / math.sqrt(dk)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, -1e9)
    p = torch.softmax(s, -1)
    out = torch.einsum("bhqk,bhkd->bhqd", p, v)
    vm = ((p > 0) * v.abs().amax(-1)[:, :, None, :]).amax(-1)
    return out, vm


def attn_inputs(g, B, S, H, dk, mask_kind):
    D = H * dk
    q = urnd(g, (B, S, H, dk), 0, 1)
    k = urnd(g, (B, S, H, dk))
    v = urnd(g, (B, S, H, dk), -2, 2)
    mask = None
    if mask_kind:
        mask = torch.ones(B, S, dtype=torch.float64)
        for b in range(B):
            kind = b % 4
            if kind == 1:
                mask[b, max(1, (S * 2) // 3):] = 0                         # ragged padding
            elif kind == 2:
                mask[b] = 0
                mask[b, S // 2] = 1                                        # all but one key masked
            elif kind == 3:
                mask[b] = 0                                                # all keys masked: the mean of v over all S keys
            if kind in (1, 2):
                mk = mask[b] == 0
                k[b, mk] = 2.0                                             # large q.k on masked keys ...
                v[b, mk] = 1e4                                             # ... and a v that shows any leak
    return q, k, v, mask


def attention_case(e, B, S, H, dk, mask_kind, bf=False, fp32=False, seed=5):
    g = torch.Generator().manual_seed(seed + S)
    q, k, v, mask = attn_inputs(g, B, S, H, dk, mask_kind)
    dt = torch.float32 if fp32 else dt16(bf)
    qkv = torch.cat([q.reshape(B * S, H * dk), k.reshape(B * S, H * dk), v.reshape(B * S, H * dk)], 1).to(dt)
    ex = qkv.double()
    qe, ke, ve = (ex[:, i * H * dk:(i + 1) * H * dk].reshape(B, S, H, dk).permute(0, 2, 1, 3) for i in range(3))
    buf = torch.full((B * S + 64, 3 * H * dk), float("nan"), dtype=dt)        # rows beyond B*S: NaN
    buf[:B * S] = qkv
    out = guarded(B * S, H * dk, dt)
    km = mask.float().to(DEV) if mask is not None else None
    if fp32:
        e.debug_attention32(buf.to(DEV), km, B, S, H, dk, out)
    else:
        e.debug_attention(buf.to(DEV), km, B, S, H, dk, out)
    torch.cuda.synchronize()
    kname = e.debug_last_kernel()
    ref, vm = attn_ref(qe, ke, ve, mask, dk)
    ref = ref.permute(0, 2, 1, 3).reshape(B * S, H, dk)
    vm = vm.permute(0, 2, 1).reshape(B * S, H, 1)
    got = out[:B * S].double().cpu().view(B * S, H, dk)
    # fp32 (attention32): P V sums S terms (S u), the fp32 scores of |q|, |k| <= 1 err by <= dk^1.5 u, i.e. relatively in p
    tol = (2 * (S + dk + dk ** 1.5) * U if fp32 else 2.0 ** -6 if bf else 2.0 ** -9) * vm
    r = float(((got - ref).abs() / tol).max()) if got.isfinite().all() else float("inf")
    assert guards_intact(out, B * S, H * dk), (S, dk, kname)
    return r, kname


ATTN_S = [1, 2, 7, 16, 21, 24, 25, 31, 32, 33, 63, 64, 65, 128, 159, 160, 161, 200, 257, 512]


def test_attention_vs_fp64():
    e = engine()
    worst, seen, fails = 0.0, set(), []
    for S in ATTN_S:
        for dk, H, mk in ((64, 8, False), (64, 8, True), (96, 12, True), (96, 12, False)):
            B = 4 if mk else 2
            r, kname = attention_case(e, B, S, H, dk, mk)
            seen.add(kname)
            worst = max(worst, r)
            print(f"attention S={S} dk={dk} H={H} mask={mk} {kname} observed/bound {r:.3f}")
            if not r <= 1:
                fails.append(f"S={S} dk={dk} mask={mk} {kname}: {r:.3f}")
    note("attention", worst)
    assert not fails, fails
    want = {"attn_mfma_s32_kernel<0,24>", "attn_mfma_s32_kernel<0,32>", "attn_mfma_flash_kernel<64>", "attn_mfma_flash_kernel<96>",
            *[f"attn_mfma_kernel<{nb}>" for nb in range(1, 6)]}
    assert want == seen, seen ^ want


def test_attention_valu_fp32_and_bf16_vs_fp64():
    fails = []
    for label, e, kw, Ss in (("valu", engine(attn_mfma=0), {}, [1, 7, 21, 32, 33, 65, 161, 257]),
                              ("fp32", engine(), dict(fp32=True), [1, 21, 33, 160, 257]),
                              ("bf16", engine(prec=4), dict(bf=True), [7, 21, 32, 33, 160, 200])):
        worst = 0.0
        for S in Ss:
            for dk, H, mk in ((64, 8, True), (96, 12, True), (64, 8, False)):
                r, kname = attention_case(e, 4, S, H, dk, mk, **kw)
                worst = max(worst, r)
                print(f"attention[{label}] S={S} dk={dk} mask={mk} {kname} observed/bound {r:.3f}")
                if not r <= 1:
                    fails.append(f"{label} S={S} dk={dk} mask={mk} {kname}: {r:.3f}")
        note(f"attention_{label}", worst)
    assert not fails, fails


@pytest.mark.parametrize("S", [1, 7, 21, 24, 25, 32])
def test_attention_gather_vs_fp64(S):
    """Layer-0 gather form: token j of window (clip c, frame i) = row c*P + clamp(i + j - shift, 0, P - 1) of qkv_pos + row j of pe_qkv,
    summed in fp16 by the kernel (the operand the reference gets is that fp16 sum)."""
    e = engine()
    g = torch.Generator().manual_seed(6 + S)
    H, dk, Twin, P, shift, nclip = 8, 64, 5, 9, 12, 3
    D = H * dk
    B = nclip * Twin
    pos = urnd(g, (nclip * P, 3 * D)).half()
    pe = urnd(g, (S, 3 * D), -0.5, 0.5).half()
    rows = torch.tensor([[c * P + min(max(i + j - shift, 0), P - 1) for j in range(S)] for c in range(nclip) for i in range(Twin)])
    tok = (pos[rows] + pe[None]).reshape(B * S, 3 * D)                  # fp16 + fp16 -> fp16, as the kernel adds them
    out = guarded(B * S, D, torch.float16)
    posb = torch.full((nclip * P + 16, 3 * D), float("nan"), dtype=torch.float16)
    posb[:nclip * P] = pos
    e.debug_attention_gather(posb.to(DEV), pe.to(DEV), Twin, P, shift, B, S, H, out)
    torch.cuda.synchronize()
    assert e.debug_last_kernel() == f"attn_mfma_s32_kernel<1,{24 if S <= 24 else 32}>"
    ex = tok.double()
    qe, ke, ve = (ex[:, i * D:(i + 1) * D].reshape(B, S, H, dk).permute(0, 2, 1, 3) for i in range(3))
    ref, vm = attn_ref(qe, ke, ve, None, dk)
    ref = ref.permute(0, 2, 1, 3).reshape(B * S, H, dk)
    vm = vm.permute(0, 2, 1).reshape(B * S, H, 1)
    got = out[:B * S].double().cpu().view(B * S, H, dk)
    r = float(((got - ref).abs() / (2.0 ** -9 * vm)).max()) if got.isfinite().all() else float("inf")
    print(f"attention gather S={S} observed/bound {r:.3f}")
    note("attention_gather", r)
    assert guards_intact(out, B * S, D)
    assert r <= 1, r
