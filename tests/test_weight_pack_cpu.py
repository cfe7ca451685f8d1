"""Weight packing on the CPU (jegal_amd/csrc/weight_pack.h, asked through jg_debug_pack_conv / jg_debug_pack_round / jg_debug_conv1_panel /
jg_debug_bias_correction: no handle, no device) against tests/golden/weight_pack_cases.json: what pack_matrix, make_conv, the two folds of
finalize_xlmr, the panel loop of finalize_gestsync, the hand-written fold of net_aud.conv1 and apply_bias_corrections computed BEFORE
their arithmetic moved into that unit -- recorded by tools/weight_pack_recorder.cpp from a copy of the old expressions with the uploads
stubbed, never from the new functions.  Everything is compared as BITS.  A few float64 properties at the end say what the bits are
for; their bounds are derived in the tests' docstrings, and where a property and the recorded bits disagreed the bits would win."""
import json
import os

import numpy as np
import pytest

from jegal_amd import _lib
from jegal_amd._lib import PREC_BF16, PREC_FP32, JegalError, bias_correction, conv1_panel, pack_conv, pack_round, weight_form


@pytest.fixture(scope="module")
def cases(golden_dir):
    import __graft_entry__ as G
    G.build()
    return json.load(open(os.path.join(golden_dir, "weight_pack_cases.json")))


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def u16(bits):
    return np.array(bits, np.uint16)


def same_f32(got, want_bits):
    return np.array_equal(np.ascontiguousarray(got, np.float32).reshape(-1).view(np.uint32), np.array(want_bits, np.uint32))


def same_u16(got, want_bits):
    if want_bits is None or got is None:
        return want_bits is None and got is None
    return np.array_equal(np.asarray(got).reshape(-1), u16(want_bits))


def f16_value(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def pack_as_the_caller(c, w, b, N, K, keep32=False, group=0, **kw):
    """The rule as pack_host (linear.hip) derives it from the mode, the kind and the model; -> (packed, form, lo kept, uncalibrated, device32)"""
    form, lo_kept, uncal = weight_form(c["precision"], c["kind"], c["model"], keep32)
    device32 = c["precision"] == PREC_FP32 or bool(keep32)
    out = pack_round(w.reshape(N, K), b, bf16=c["precision"] == PREC_BF16, form=form, keep_lo=lo_kept, diffuse_group=group, device32=device32, **kw)
    return out, form, lo_kept, uncal, device32


def check_packed(c, out, form, uncal, device32):
    assert same_u16(out["hi"], c["hi"]), c
    assert same_u16(out["lo"], c["lo"]), c
    assert same_f32(out["bias"], c["bias"]), c
    assert _lib.WEIGHT_FORMS.index(form) == c["form"] and uncal == bool(c["uncalibrated"]) and device32 == bool(c["w32_kept"]), c
    assert (form == "bias_corrected") == bool(c["cal"]), c


def test_rounding_every_mode_kind_model(cases):
    """N = 3, K = 5 through every precision mode x layer kind x model x keep32: hi, lo (or none), bias, which fp32 copies are kept.  The
    inputs hold exact fp16 / bf16 ties, a value that rounds up into the next binade, fp16 subnormals, a residual whose lo is subnormal,
    both zeros and, for bf16, a quiet and a signalling NaN."""
    r = cases["round"]
    assert len(r["cases"]) == 7 * 4 * 3 * 2
    assert len({(c["precision"], c["kind"], c["model"], c["keep32"]) for c in r["cases"]}) == 168
    w16, wbf, b = f32(r["w16"]), f32(r["wbf"]), f32(r["bias"])
    assert np.isnan(wbf).sum() == 2 and (w16 == 0).sum() == 2 and np.signbit(w16[w16 == 0]).sum() == 1
    seen_lo = 0
    for c in r["cases"]:
        w = wbf if c["precision"] == PREC_BF16 else w16
        out, form, lo_kept, uncal, device32 = pack_as_the_caller(c, w, b, 3, 5, keep32=c["keep32"])
        check_packed(c, out, form, uncal, device32)
        if out["w32"] is not None:          # the fp32 copies are the matrix and the bias as given
            assert np.array_equal(out["w32"].reshape(-1).view(np.uint32), w.view(np.uint32)) and np.array_equal(out["b32"].view(np.uint32), b.view(np.uint32))
        seen_lo += out["lo"] is not None
    assert 0 < seen_lo < 168


def test_rounding_float64_properties(cases):
    """hi + lo: |w - (hi + lo)| <= max(2^-22 |w|, 2^-25) for |w| < 2^15.  hi = fp16(w) leaves a residual r with |r| <= 2^-11 |w| (or
    <= 2^-25 where hi is subnormal), exact in fp32; lo = fp16(r) leaves |r| 2^-11 <= 2^-22 |w| where lo is normal and at most half the
    smallest subnormal, 2^-25, where it is not.  Single fp16 is numpy's round-to-nearest-even."""
    w = np.concatenate([f32(cases["round"]["w16"]), np.random.default_rng(0).standard_normal(45).astype(np.float32) * np.float32(3.0)])
    w = w[np.abs(w) < 2.0 ** 15][:45].reshape(9, 5)
    out = pack_round(w, np.zeros(9, np.float32), form="split", keep_lo=True)
    assert np.array_equal(out["hi"], w.astype(np.float16).view(np.uint16))
    err = np.abs(w.astype(np.float64) - (f16_value(out["hi"]) + f16_value(out["lo"])))
    assert np.all(err <= np.maximum(2.0 ** -22 * np.abs(w.astype(np.float64)), 2.0 ** -25))


def test_diffusion_and_its_fallbacks(cases):
    """Error diffusion along the taps of one (channel, slot) chain: N = 2, slot 4, nine taps, two zero padding slots in the middle of a
    chain and a negative zero in another; K = 35 with group 4 and a hi+lo form must both fall back to round-to-nearest.
    Property: per chain |sum over taps of (w - hi)| <= 2^-10 max|w|.  The sum is the last carry, v - fp16(v) with v = w + carry, at most
    half an fp16 ulp of v: 2^-11 |v| <= 2^-11 (1 + 2^-11) max|w| in the normal range.  Padding slots are exactly (positive) zero."""
    d = cases["diffuse"]
    assert [(c["K"], c["group"]) for c in d] == [(36, 4), (35, 4), (36, 4)]
    for i, c in enumerate(d):
        w, b = f32(c["w"]), f32(c["b"])
        out, form, lo_kept, uncal, device32 = pack_as_the_caller(c, w, b, c["N"], c["K"], group=c["group"])
        check_packed(c, out, form, uncal, device32)
        nearest = w.astype(np.float16).view(np.uint16).reshape(c["N"], c["K"])
        if i == 0:
            assert form == "single" and (w == 0).sum() == 3 and not np.array_equal(out["hi"], nearest)        # diffusion did something
            assert np.all(out["hi"].reshape(-1)[w == 0] == 0)
            resid = (w.astype(np.float64) - f16_value(out["hi"]).reshape(-1)).reshape(c["N"], 9, 4).sum(axis=1)
            assert np.all(np.abs(resid) <= 2.0 ** -10 * np.abs(w).max())
        else:
            assert (form == "single") == (i == 1) and np.array_equal(out["hi"], nearest)


def conv_args(c):
    bn = tuple(f32(c[k]) for k in ("gamma", "beta", "mean", "var")) if "gamma" in c else None
    return f32(c["w"]).reshape(c["O"], c["I"], c["KT"], c["KH"], c["KW"]), f32(c["b"]), bn


def test_conv_matrix_and_shift(cases):
    """BatchNorm fold and tap layout of make_conv: natural order, parity-class order for strides (2, 2) and (1, 2), 7 x 7 with reorder
    (more than 32 taps: stays natural), the conv1 form (KT = 5, slot 16), kpad beyond the taps, Opad beyond O, no BatchNorm."""
    cs = {c["tag"]: c for c in cases["conv"]}
    assert sorted(cs) == sorted(["natural", "reorder_2x2", "reorder_1x2", "7x7_reorder_stays_natural", "conv1_form", "kpad", "opad", "no_bn"])
    got = {}
    for tag, c in cs.items():
        w, b, bn = conv_args(c)
        m, s = pack_conv(w, b, bn, slot=c["slot"], kpad=c["kpad"], Opad=c["Opad"], stride=(c["SH"], c["SW"]), reorder=c["reorder"])
        assert m.shape == (c["N"], c["K"]) and same_f32(m, c["matrix"]) and same_f32(s, c["shift"]), tag
        got[tag] = m
    assert (cs["conv1_form"]["K"], cs["kpad"]["K"], cs["opad"]["N"]) == (64, 32, 4)
    assert not np.array_equal(got["reorder_2x2"], got["reorder_1x2"]) and "gamma" not in cs["no_bn"]
    assert np.all(got["opad"][3] == 0) and f32(cs["opad"]["shift"])[3] == 0 and np.all(got["kpad"][:, 25:] == 0)
    assert np.all(got["conv1_form"].reshape(2, 4, 16)[:, :, 15] == 0)        # slot 16 holds KT I = 15 channels: the pad lane is zero
    # the layout in float64 terms, natural order: matrix[o][t slot + c] = w[o][c][0][kh][kw] * gamma / sqrt(var + 1e-5) to fp32 rounding
    c = cs["natural"]
    w, b, (g, be, mu, var) = conv_args(c)
    ref = (w[:, :, 0].astype(np.float64) * (g / np.sqrt(var.astype(np.float64) + 1e-5))[:, None, None, None]).transpose(0, 2, 3, 1).reshape(3, 18)
    assert np.allclose(got["natural"], ref, rtol=2.0 ** -21, atol=0)


def test_audio_conv1_is_the_conv_function(cases):
    """net_aud.conv1 (O = 64, 3 x 3, I = 1, slot 1) through the one conv function equals its former hand-written fold, bit for bit."""
    c = cases["audio_conv1"]
    bn = tuple(f32(c[k]) for k in ("gamma", "beta", "mean", "var"))
    m, s = pack_conv(f32(c["w"]).reshape(64, 1, 1, 3, 3), f32(c["b"]), bn, slot=1)
    assert m.shape == (64, 9) and same_f32(m, c["matrix"]) and same_f32(s, c["shift"])


def test_layernorm_folds_and_column_sums(cases):
    """Consumer fold W diag(gamma), b + W beta and the column sums of the weights as packed at N = 4, K = 6 in single fp16, hi + lo and
    bf16; the producer's b + beta.  float64: W diag(gamma) is the correctly rounded product (exact in float64, rounded once); the bias
    is summed in double and rounded once, so it lies within 2 fp32 ulp of the float64 value (half an ulp from the rounding, the rest is
    slack for the double sum's own 6 roundings of 2^-53 each)."""
    assert [c["precision"] for c in cases["ln_consumer"]] == [0, 1, PREC_BF16]
    for c in cases["ln_consumer"]:
        w, b, g, be = (f32(c[k]) for k in ("w", "b", "gamma", "beta"))
        form, lo_kept, _ = weight_form(c["precision"], c["kind"], c["model"])
        out = pack_round(w.reshape(4, 6), b, bf16=c["precision"] == PREC_BF16, form=form, keep_lo=lo_kept, ln=(g, be), device32=True)
        assert same_u16(out["hi"], c["hi"]) and same_u16(out["lo"], c["lo"]) and same_f32(out["bias"], c["bias"]), c["precision"]
        assert same_f32(out["c1h"], c["c1h"]) and same_f32(out["c1f"], c["c1f"]) and same_f32(out["w32"], c["w_folded"]), c["precision"]
        w64 = w.reshape(4, 6).astype(np.float64)
        assert np.array_equal(out["w32"], (w64 * g.astype(np.float64)).astype(np.float32))
        ref_b = b.astype(np.float64) + w64 @ be.astype(np.float64)
        assert np.all(np.abs(out["bias"].astype(np.float64) - ref_b) <= 2 * np.spacing(np.abs(ref_b).astype(np.float32)))
        if c["precision"] != PREC_BF16:          # the sums are of the packed values: exact in float64, rounded once
            hi, lo = f16_value(out["hi"]), f16_value(out["lo"]) if lo_kept else 0.0
            assert np.array_equal(out["c1h"], hi.sum(axis=1).astype(np.float32)) and np.array_equal(out["c1f"], (hi + lo).sum(axis=1).astype(np.float32))
        else:
            assert np.array_equal(out["c1h"], out["c1f"])
    p = cases["ln_producer"]
    out = pack_round(np.ones((4, 2), np.float32), f32(p["b"]), add_beta=f32(p["beta"]))
    assert same_f32(out["bias"], p["bias"])


def test_conv1_direct_panel(cases):
    """The slot-major panel from the HOST matrix: every Wd[s][o][e], e != bias lane, is W[o][16 s + e]; the bias lane of slots 0 / 1 holds
    the hi / lo fp16 pair of 255 shift 2^-10; the bias lane of slots 2 .. 48 holds what the old loop left there, W[o][16 s + 15].  The
    whole panel is pinned by the FNV-1a hash of the old loop's output."""
    p = cases["panel"]
    i = np.arange(64 * 784, dtype=np.uint64)
    hi = ((((i * np.uint64(40503)) & np.uint64(0xffffffff)) >> np.uint64(4)) & np.uint64(0xffff)).astype(np.uint16)
    hi[(hi & 0x7c00) == 0x7c00] &= 0xbfff
    slot, lane = (i % 784) // 16, i % 16
    hi[(lane == 15) & (slot != 5) & (slot != 40)] = 0
    hi = hi.reshape(64, 784)
    shift = f32(p["shift"])
    wd = conv1_panel(hi, shift)
    W = hi.reshape(64, 49, 16).transpose(1, 0, 2)
    assert np.array_equal(wd[:, :, :15], W[:, :, :15]) and np.array_equal(wd[2:, :, 15], W[2:, :, 15]) and wd[5, :, 15].any()
    v = (shift * np.float32(255.0)) * np.float32(2.0 ** -10)
    assert v.dtype == np.float32
    bias_hi = v.astype(np.float16)
    bias_lo = (v - bias_hi.astype(np.float32)).astype(np.float16)
    assert np.array_equal(wd[0, :, 15], bias_hi.view(np.uint16)) and np.array_equal(wd[1, :, 15], bias_lo.view(np.uint16))
    assert same_u16(wd[0, :, 15], p["bias_hi"]) and same_u16(wd[1, :, 15], p["bias_lo"])
    fnv = 0xcbf29ce484222325
    for byte in wd.astype("<u2").tobytes():
        fnv = ((fnv ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    assert f"{fnv:016x}" == p["fnv1a64"]


def test_bias_correction(cases):
    c = cases["bias_correction"]
    got = bias_correction(f32(c["w32"]).reshape(3, 5), f32(c["b32"]), f32(c["mu"]), c["rows"])
    assert same_f32(got, c["bias"])


def test_bad_arguments_are_rejected_and_nothing_is_written(cases):
    lib = _lib.load_library()
    w, b = np.ones((3, 5), np.float32), np.ones(3, np.float32)
    hi, lo, bias = np.full((3, 5), 0xabcd, np.uint16), np.full((3, 5), 0xabcd, np.uint16), np.full(3, 7.0, np.float32)
    wp, bp, hp, lp, op = (a.ctypes.data for a in (w, b, hi, lo, bias))

    def rnd(w=wp, b=bp, N=3, K=5, group=0, form=1, keep_lo=1, hi=hp, lo=lp, out=op):
        return lib.jg_debug_pack_round(w, b, N, K, 0, form, keep_lo, group, None, None, None, 0, hi, lo, out, None, None, None, None)
    assert rnd() == 0 and not (hi == 0xabcd).any()
    hi[:], lo[:], bias[:] = 0xabcd, 0xabcd, 7.0
    bad = [rnd(w=None), rnd(b=None), rnd(hi=None), rnd(out=None), rnd(lo=None), rnd(N=0), rnd(K=0), rnd(N=-3), rnd(K=-1), rnd(group=-1),
           rnd(form=4), rnd(form=-1), rnd(keep_lo=0)]          # (keep_lo = 0 with a lo buffer: the caller's rule and buffers disagree)
    assert bad == [_lib.JG_ERR_ARG] * len(bad)
    assert (hi == 0xabcd).all() and (lo == 0xabcd).all() and (bias == 7.0).all()
    with pytest.raises(JegalError):
        pack_round(w, b, diffuse_group=-1)
    # conv: null tensors, a BatchNorm given in part, sizes <= 0, channels that do not fit the slot, N / K that are not the layer's
    cw, cb = np.ones((3, 2, 1, 3, 3), np.float32), np.ones(3, np.float32)
    m, s = np.full((3, 18), 7.0, np.float32), np.full(3, 7.0, np.float32)

    def conv(w=cw.ctypes.data, b=cb.ctypes.data, g=None, O=3, I=2, slot=2, N=3, K=18, m=m.ctypes.data, s=s.ctypes.data):
        return lib.jg_debug_pack_conv(w, b, g, None, None, None, O, I, 1, 3, 3, slot, 0, 0, 1, 1, 0, N, K, m, s)
    assert conv() == 0 and not (m == 7.0).any()
    m[:], s[:] = 7.0, 7.0
    bad = [conv(w=None), conv(b=None), conv(m=None), conv(s=None), conv(g=cb.ctypes.data), conv(O=0), conv(I=0), conv(slot=1), conv(N=4), conv(K=17)]
    assert bad == [_lib.JG_ERR_ARG] * len(bad) and (m == 7.0).all() and (s == 7.0).all()
    panel = np.full((49, 64, 16), 0xabcd, np.uint16)
    ph, ps = np.zeros((64, 784), np.uint16), np.zeros(64, np.float32)
    assert lib.jg_debug_conv1_panel(None, ps.ctypes.data, panel.ctypes.data) == _lib.JG_ERR_ARG
    assert lib.jg_debug_conv1_panel(ph.ctypes.data, None, panel.ctypes.data) == _lib.JG_ERR_ARG
    assert lib.jg_debug_conv1_panel(ph.ctypes.data, ps.ctypes.data, None) == _lib.JG_ERR_ARG and (panel == 0xabcd).all()
    mu, nb = np.ones(5, np.float32), np.full(3, 7.0, np.float32)

    def bc(w=wp, b=bp, mu=mu.ctypes.data, rows=7, N=3, K=5, out=nb.ctypes.data):
        return lib.jg_debug_bias_correction(w, b, mu, rows, N, K, out)
    bad = [bc(w=None), bc(b=None), bc(mu=None), bc(out=None), bc(rows=0), bc(N=0), bc(K=0)]
    assert bad == [_lib.JG_ERR_ARG] * len(bad) and (nb == 7.0).all()
    assert bc() == 0 and not (nb == 7.0).any()
