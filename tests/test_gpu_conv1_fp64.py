"""Kernel-level checks of conv1 + BatchNorm + ReLU + max-pool against float64, bit for bit on the fused u8 kernel (run with -m gpu).

Every launch goes through jg_debug_conv1_pool (include/jegal_hip.h), i.e. the production gs_conv1_stage: zero-band scan, then
conv1_direct_kernel, then conv1_edge_fix_kernel -- or, with conv1_direct = 0 or on a bf16 handle, stack + implicit GEMM + max-pool.
Operands, inputs, the float64 reference, the bounds and the expected bits come from tests/conv1_fp64_cases.py (its docstring has the
derivations; tests/test_conv1_cases_cpu.py checks it without a GPU).  The weights are loaded once per handle: the synthetic GestSync
checkpoint with the six net_vid.conv1.* / bn1.* tensors replaced by values that reach every kernel unchanged and make every sum exact.

Every output element of every case is checked:
  tier A (every path)      |got - ref| <= maxpool(2 K u S) + 1 ulp of ref, K = 737, u = 2^-24; observed / bound is printed per family
  tier B (direct kernel)   torch.equal on the bit patterns, for conv1_mfma16 = 0 / 1 x conv1_zero_skip = 0 / 1.  Outputs over all-zero
                           patches (skipped tiles, two-step zero tiles, the constant fill) follow the same formula, f16(relu(shift)).
Guards, all inside allocations: one frame of random non-zero bytes in front of and behind the clips (a read outside the clips changes
results by O(|ref|) instead of faulting); the result sits at a 16-byte-aligned offset inside a buffer of sentinel bits, the regions
before and after must come back untouched and no sentinel may remain inside the result (fill_all is true for this entry).

Tier B rests on an fp32 MFMA accumulation returning the exact sum when the exact sum and every partial sum are fp32 values.  Decision,
from the MI355X: it does, and tier B is asserted.  Evidence: the first run, against a kernel whose pad lane fed the bias pair the fp16
SUBNORMAL 2^-24, had 3.8 - 4.0 % of the elements of every dense case off, 91 % of them by one ulp, spread evenly over positions, pooled
rows and pooled columns -- but not over channels: 0 % in the 16 channels with floor(log2 |255 shift|) - k <= 4 (k: the channel's
weight-scale exponent), 0.4 - 19.5 % in every channel above that with a non-zero output.  The same launch with shift = 0, and with
255 shift = 0.996 (k-independent), matched in 100 % of the bits, in both MFMA forms.  So the sum is exact; the MFMA aligns the products
of a k-step by their operands' exponent FIELDS and keeps 24 bits below the largest, and a subnormal's field is that of 2^-14: the bias
product sat ten bits above its value and pushed the low bits of that step's pixel products out.  The kernel was fixed (the pad lane is
the normal 2^-14 and the pair holds 255 shift 2^-10: shared.h, CONV1_BIAS_ONE), after which every case matches bit for bit.
Measured there, per family, worst observed / bound of tier A: direct 0.32 - 0.45 (dense 0.319, mask 0.345, mask_jitter 0.451, middle
0.429, bottom 0.407, black 0.318, lone_byte_* 0.345 - 0.454, unread_rows 0.407), the implicit GEMM the same figures, bf16 0.466 (dense)
and 0.494 (mask); >= 99.9879 % of the fp16 outputs equal the correctly rounded reference (before the fix: 96.0 % on the direct kernel).

Seeded defects these tests were seen to fail on (each built into a scratch copy of the library, never committed; every access stays
inside the allocations; run on the shapes below b3t2p12; tier A: worst observed / bound, tier B: share of differing bits per launch):
  1. launch_conv1_edge_fix not called: all 14 cases with a non-black clip; tier A 860, tier B 0.8 - 1.4 % (pooled columns 15, 31, 47, 63)
  2. the carry is R3 alone in pool(): the same 14; tier A 1079, tier B 7.5 - 12.7 % (pooled rows 2 rt - 1)
  3. the upper temporal clamp of strip_setup is T - 2 for T >= 2: the 13 cases with T >= 2; tier A 3.6e6, tier B 34 - 81 %
  4. two (kh, kw) slots swapped when finalize_gestsync builds Wd: the 14; tier A 752, tier B 45 - 79 %
  5. skip_of(z) returns z: middle, bottom, unread_rows, lone_byte_first (a zero band under a non-zero one); tier A 1079, tier B up to 1.6 %
  6. step 2 of conv1_zero_scan_kernel skipped: lone_byte_first, lone_byte_1424, lone_byte_bandend; tier A 14, tier B 0.009 - 0.024 %
     (lone_byte_last cannot show it: its byte belongs to pixel 479, which no pooled output reads)
  7. the lo entry of the bias pair written as 0: the 14, by tier B alone: 7.9 - 13.3 % of the bits, tier A 0.85 at the most
"""
import ctypes

import pytest
import torch

import conv1_fp64_cases as C
import test_gpu_kernels_fp64 as K64
from test_gpu_kernels_fp64 import DEV, SENT16, engine, note, rejects, ulp16

pytestmark = pytest.mark.gpu

C.check_shape_properties(torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else None)

GUARD = 1 << 16                    # halves in front of and behind the result (128 KB: the offset stays 16-byte aligned)
DEFAULTS = dict(conv1_direct=1, conv1_mfma16=1, conv1_zero_skip=1)
_LOADED = set()
SHARES = {}                        # family -> lowest share of 16-bit outputs equal to the correctly rounded reference (recorded, not asserted)


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in K64._ENGINES.values():
        e.close()
    K64._ENGINES.clear()
    _LOADED.clear()
    C._CASE.clear()


def handle(bf=False):
    """The fp16 (default mode) or bf16 (precision 4) handle with the exact-sum conv1 weights, loaded once."""
    e = engine(prec=4 if bf else None)
    if id(e) not in _LOADED:
        from jegal_amd import synth
        sd = dict(synth.gestsync_state_dict(include_unused=False))
        sd.update(C.operands()["sd"])
        e.load_tensors(sd)
        e.finalize(1)
        _LOADED.add(id(e))
    return e


@pytest.fixture(scope="module")
def fp16_handle():
    return handle(False)


@pytest.fixture(scope="module")
def bf16_handle():
    return handle(True)


def guarded_input(frames):
    """[one frame of random non-zero bytes | the clips | one such frame] on the device -> (buffer, pointer to the clips)"""
    B, T = frames.shape[:2]
    g = torch.Generator().manual_seed(5)
    buf = torch.randint(1, 256, (B * T + 2, C.IH, C.IW, 3), generator=g, dtype=torch.uint8)
    buf[1:-1] = frames.reshape(B * T, C.IH, C.IW, 3)
    buf = buf.to(DEV)
    assert buf[1].data_ptr() % 16 == 0
    return buf, buf[1].data_ptr()


def sentinel_output(n):
    buf = torch.full((GUARD + n + GUARD,), SENT16, dtype=torch.int16, device=DEV)
    assert buf[GUARD:].data_ptr() % 16 == 0
    return buf


def run_entry(e, src_ptr, B, T, pad, out_ptr):
    e._bind_stream()
    e._ck(e.lib.jg_debug_conv1_pool(e.h, ctypes.c_void_p(src_ptr) if src_ptr else None, B, T, pad, ctypes.c_void_p(out_ptr) if out_ptr else None))


def launch(e, opts, src_ptr, B, T, pad, n):
    """One call of the entry under `opts` (restored afterwards) -> the result's bits (n int16 on the device), after the guard checks."""
    out = sentinel_output(n)
    try:
        for k, v in opts.items():
            e.set_option(k, v)
        run_entry(e, src_ptr, B, T, pad, out[GUARD:].data_ptr())
        torch.cuda.synchronize()
    finally:
        for k, v in DEFAULTS.items():
            e.set_option(k, v)
    assert bool((out[:GUARD] == SENT16).all()) and bool((out[GUARD + n:] == SENT16).all()), f"{opts}: a guard region of the output was written"
    got = out[GUARD:GUARD + n]
    left = int((got == SENT16).sum())
    assert left == 0, f"{opts}: {left} output elements were never written"
    return got


def tier_a(name, family, got16, ref, bnd, bf):
    """-> failure text or None; prints and records observed / bound and the correctly rounded share"""
    got = got16.view(torch.bfloat16 if bf else torch.float16).double()
    ratio = float(((got - ref).abs() / bnd).max()) if bool(got.isfinite().all()) else float("inf")
    share = C.correctly_rounded_share(got, ref, bf)
    note(family, ratio)
    SHARES[family] = min(SHARES.get(family, 1.0), share)
    print(f"{name:58s} tier A observed/bound {ratio:.3f}  correctly rounded {share:.4%}")
    if not ratio <= 1:
        bad = ((got - ref).abs() > bnd) | ~got.isfinite()
        return f"{name}: tier A observed/bound {ratio:.3f}: {C.describe_mismatch(bad.view(-1, C.PH, C.PW, C.OC).cpu())}"
    return None


def tier_b(name, got16, bits):
    """-> failure text or None"""
    if torch.equal(got16, bits):
        return None
    ne = (got16 != bits).view(-1, C.PH, C.PW, C.OC)
    one = int(((got16.int() - bits.int()).abs() == 1).sum())
    return f"{name}: tier B bits: {C.describe_mismatch(ne.cpu())} | {one} of them by one ulp"


DIRECT = [dict(conv1_mfma16=m, conv1_zero_skip=z) for m in (1, 0) for z in (1, 0)]


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_conv1_vs_fp64(case, fp16_handle):
    """The direct kernel in both MFMA forms with and without the zero-band skip (tiers A and B) and the implicit-GEMM formulation on
    the fp16 handle (tier A), all on the same input and against the same reference."""
    shape, family = case
    B, T, pad = C.SHAPES[shape]
    d = C.case_data(case)
    n = d["ref"].numel()
    ref, bnd, bits = d["ref"].reshape(-1).to(DEV), (d["core"] + ulp16(d["ref"])).reshape(-1).to(DEV), d["bits"].reshape(-1).to(DEV)
    src, ptr = guarded_input(d["frames"])
    fails = []
    for opts in DIRECT:
        name = f"{C.case_id(case)} direct mfma16={opts['conv1_mfma16']} zero_skip={opts['conv1_zero_skip']}"
        got = launch(fp16_handle, opts, ptr, B, T, pad, n)
        fails += [f for f in (tier_a(name, family, got, ref, bnd, False), tier_b(name, got, bits)) if f]
    for z in (1, 0):
        got = launch(fp16_handle, dict(conv1_direct=0, conv1_zero_skip=z), ptr, B, T, pad, n)
        fails += [f for f in (tier_a(f"{C.case_id(case)} implicit fp16 zero_skip={z}", family + "/implicit", got, ref, bnd, False),) if f]
    print("worst observed/bound so far:", {k: round(v, 3) for k, v in K64.RATIOS.items()})
    print("lowest correctly rounded share so far:", {k: round(v, 6) for k, v in SHARES.items()})
    del src
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", ["dense", "mask"])
def test_conv1_bf16_vs_fp64(family, bf16_handle):
    """The bf16 build runs conv1 as stack + implicit GEMM + max-pool whatever conv1_direct says: tier A with bf16 ulps."""
    case = ("b1t3p4", family)
    B, T, pad = C.SHAPES[case[0]]
    d = C.case_data(case)
    n = d["ref"].numel()
    ref, bnd = d["ref"].reshape(-1).to(DEV), (d["core"] + ulp16(d["ref"], bf=True)).reshape(-1).to(DEV)
    src, ptr = guarded_input(d["frames"])
    fails = []
    for opts in (dict(conv1_direct=1), dict(conv1_direct=0, conv1_zero_skip=0)):
        got = launch(bf16_handle, opts, ptr, B, T, pad, n)
        fails += [f for f in (tier_a(f"{C.case_id(case)} bf16 {opts}", family + "/bf16", got, ref, bnd, True),) if f]
    print("worst observed/bound so far:", {k: round(v, 3) for k, v in K64.RATIOS.items()})
    del src
    assert not fails, "\n".join(fails)


def test_conv1_entry_rejections(fp16_handle):
    """What the entry refuses comes back as JG_ERR_ARG and leaves the output untouched."""
    e = fp16_handle
    frames = C.make_frames("b1t1p2", "dense")
    src, ptr = guarded_input(frames.expand(1, 5, -1, -1, -1).contiguous())       # five frames: every refused shape below stays inside it
    n = 5 * C.PH * C.PW * C.OC
    out = sentinel_output(n)
    optr = out[GUARD:].data_ptr()
    for what, args in (("pad = 13", (ptr, 1, 1, 13, optr)), ("pad = -1", (ptr, 1, 5, -1, optr)), ("T + 2 pad = 4", (ptr, 1, 2, 1, optr)),
                       ("T + 2 pad = 4, T = 4", (ptr, 1, 4, 0, optr)), ("B = 0", (ptr, 0, 5, 0, optr)), ("null frames", (0, 1, 5, 0, optr)),
                       ("null output", (ptr, 1, 5, 0, 0))):
        assert rejects(run_entry, e, *args), what
        torch.cuda.synchronize()
        assert bool((out == SENT16).all()), f"{what}: a refused call wrote to the output"
    run_entry(e, ptr, 1, 5, 0, optr)                                              # the same buffers are accepted when the arguments are right
    torch.cuda.synchronize()
    assert not bool((out[GUARD:GUARD + C.PH * C.PW * C.OC] == SENT16).any()) and bool((out[GUARD + C.PH * C.PW * C.OC:] == SENT16).all())
