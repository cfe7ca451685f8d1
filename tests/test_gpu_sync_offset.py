"""jg_sync_offset through the C ABI (run with -m gpu): offsets, confidences and curves of planted ragged batches against the float64
statement of the contract (tests/sync_offset_cases.py).

Offsets: the float64 arg-max on EVERY clip -- tests/test_sync_offset_cpu.py proves each planted clip decidable (float64 margin >= 1e-3).
Curve and conf: err(X) = max-abs distance of X from float64 pooled over the clips of one call; the kernel is held to
err(kernel) <= 4 x err(float32 numpy statement), the project's rule for jg_attn_matrix.  The NaN pattern must be the statement's.
Every output lies between guard words that must survive."""
import ctypes

import numpy as np
import pytest
import torch

import sync_offset_cases as C

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
GUARD = 64
GUARD_BITS = 0x7FC0BEEF          # a quiet NaN with a payload, as int32


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


def call(eng, clips, R, mo, want_curve=True, expect=0, D=None, n=None, misalign=False):
    """One jg_sync_offset call -> (offset (n,), conf (n,), curve (n, 2R + 1) | None) on the host; guards checked."""
    D = D or clips[0][0].shape[1]
    n = len(clips) if n is None else n
    W = 2 * R + 1
    cat = lambda xs: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs + [np.zeros((4, xs[0].shape[1]), np.float32)]), np.float32)).cuda()
    v, a = cat([c[0] for c in clips]), cat([c[1] for c in clips])
    if misalign:
        v = v.reshape(-1)[1:]
    off = lambda xs: torch.as_tensor(np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.int32), device="cuda")
    vo, ao = off([c[0] for c in clips]), off([c[1] for c in clips])
    nw = max(n, 0) * max(W, 0)
    curve = torch.full((GUARD + nw + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    offset = torch.full((GUARD + max(n, 0) + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    conf = torch.full((GUARD + max(n, 0) + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    at = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * GUARD)
    eng._bind_stream()
    rc = eng.lib.jg_sync_offset(eng.h, P(v), P(vo), P(a), P(ao), n, D, R, mo, at(curve) if want_curve else None, at(offset), at(conf))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    cu, of, co = curve.cpu().numpy(), offset.cpu().numpy(), conf.cpu().numpy()
    for name, buf, m in (("curve", cu, nw), ("offset", of, max(n, 0)), ("conf", co, max(n, 0))):
        assert (buf[:GUARD] == GUARD_BITS).all() and (buf[GUARD + m:] == GUARD_BITS).all(), name + ": a guard word was overwritten"
    if expect != 0 or n <= 0 or not want_curve:
        assert (cu == GUARD_BITS).all(), "the curve was written"
    if expect != 0 or n <= 0:
        assert (of == GUARD_BITS).all() and (co == GUARD_BITS).all()
        return None
    return of[GUARD:GUARD + n].copy(), co[GUARD:GUARD + n].view(np.float32).copy(), cu[GUARD:GUARD + nw].view(np.float32).reshape(n, W).copy() if want_curve else None


def check(name, got, clips, R, mo):
    of, co, cu = got
    e_k = e_r = c_k = c_r = 0.0
    for i, (v, a) in enumerate(clips):
        o64, c64, k64 = C.sync_ref(v, a, R, mo)
        _, c32, k32 = C.sync_ref(v, a, R, mo, np.float32)
        assert of[i] == o64, (name, i, v.shape, a.shape, int(of[i]), o64)
        if cu is not None:
            assert np.array_equal(np.isnan(cu[i]), np.isnan(k64)), (name, i)
        assert np.isnan(co[i]) == np.isnan(c64), (name, i)
        if np.isnan(c64):
            continue
        ok = ~np.isnan(k64)
        if cu is not None:
            e_k = max(e_k, float(np.abs(cu[i][ok] - k64[ok]).max()))
            e_r = max(e_r, float(np.abs(k32[ok].astype(np.float64) - k64[ok]).max()))
        c_k, c_r = max(c_k, abs(float(co[i]) - c64)), max(c_r, abs(float(c32) - c64))
    return e_k, e_r, c_k, c_r


def hold(name, errs, skip_exact=False):
    """the error rule on errors pooled over `errs` (one tuple per call of one input).  skip_exact: a part (curve, conf) in which the
    float32 statement happens to be exact gives no yardstick and is left to the pooled rule of the caller"""
    e_k, e_r, c_k, c_r = (max(e[j] for e in errs) for j in range(4))
    print(f"{name}: curve max-abs kernel {e_k:.3e} fp32 statement {e_r:.3e} ratio {e_k / max(e_r, 1e-30):.2f} | "
          f"conf kernel {c_k:.3e} fp32 statement {c_r:.3e} ratio {c_k / max(c_r, 1e-30):.2f}")
    if not (skip_exact and e_r == 0):
        assert e_k <= 4 * e_r, (name, "curve", e_k, e_r)
    if not (skip_exact and c_r == 0):
        assert c_k <= 4 * c_r, (name, "conf", c_k, c_r)


@pytest.mark.parametrize("D,R", C.SWEEP)
def test_planted_batches(eng, D, R):
    """37 clips: Tv in 1, 31, 33, 150; Ta = Tv, Tv + 3, Tv - 3; planted at -R, 0, R; and the first clip of every Tv alone (n_clips = 1)"""
    clips = C.sweep_batch(D, R)
    assert len(clips) == 37 and [clips[i][0].shape[0] for i in (0, 6, 15, 24)] == list(C.TV)
    batch = call(eng, clips, R, 1)
    hold(f"D={D} R={R} n=37", [check(f"D={D} R={R} n=37", batch, clips, R, 1)])
    for i in (0, 6, 15, 24):
        alone = call(eng, clips[i:i + 1], R, 1)
        check(f"D={D} R={R} clip {i} alone", alone, clips[i:i + 1], R, 1)          # offset and NaN pattern; the values: the batch's bits
        # a clip's result does not depend on the batch around it: the same bits
        assert alone[0][0] == batch[0][i] and alone[1].view(np.int32)[0] == batch[1].view(np.int32)[i]
        assert np.array_equal(alone[2].view(np.int32)[0], batch[2].view(np.int32)[i])


def test_a_clip_gives_the_same_bits_alone_first_and_last(eng):
    clips = C.sweep_batch(1024, 15)
    probe = clips[33]
    others = [clips[5], clips[20], clips[30]]
    res = [call(eng, [probe], 15, 1), call(eng, [probe] + others, 15, 1), call(eng, others + [probe], 15, 1)]
    picks = [(res[0], 0), (res[1], 0), (res[2], 3)]
    ref = None
    for r, i in picks:
        bits = (int(r[0][i]), int(r[1].view(np.int32)[i]), r[2].view(np.int32)[i].tobytes())
        ref = ref or bits
        assert bits == ref


def test_special_clips(eng):
    """Tv < R with min_overlap cutting shifts to NaN, no shift left at all, zero rows, duplicated rows, an oversized and two empty clips
    between good ones, each also without the curve.  The error rule holds per call (one input each), wherever the float32 statement has
    an error at all, and on the errors pooled over the calls (which covers a part in which a call's statement is exact)."""
    errs = []
    for name, (clips, R, mo) in sorted(C.special_clips().items()):
        errs.append(special(eng, name, clips, R, mo))
        hold(name, errs[-1:], skip_exact=True)
    hold("special clips", errs)


def special(eng, name, clips, R, mo):
    got = call(eng, clips, R, mo)
    errs = check(name, got, clips, R, mo)
    of, co, cu = got
    if name == "no_shift":
        assert (of == 0).all() and np.isnan(co).all() and np.isnan(cu).all()
    if name == "duplicates":          # shifts 0 and 2 are bit-equal maxima: the first wins
        assert of[0] == 0 and cu[0].view(np.int32)[R] == cu[0].view(np.int32)[R + 2] and cu[0].view(np.int32)[R + 1] == cu[0].view(np.int32)[R + 3]
    if name == "oversized_empty":
        for i in (1, 3, 4):
            assert of[i] == 0 and np.isnan(co[i]) and np.isnan(cu[i]).all()
        for i in (0, 2, 5):
            assert not np.isnan(co[i])
    # without the curve: the same offsets and confidences, bit for bit
    of2, co2, none = call(eng, clips, R, mo, want_curve=False)
    assert none is None and np.array_equal(of, of2) and np.array_equal(co.view(np.int32), co2.view(np.int32))
    return errs


def test_bad_arguments_are_refused_before_anything_is_written(eng):
    clips = C.sweep_batch(64, 1)[:3]
    ARG = -1
    assert call(eng, clips, 65, 1, expect=ARG) is None
    assert call(eng, clips, -1, 1, expect=ARG) is None
    assert call(eng, clips, 1, 0, expect=ARG) is None
    assert call(eng, clips, 1, 1, expect=ARG, D=96) is None
    assert call(eng, clips, 1, 1, expect=ARG, D=2048) is None
    assert call(eng, clips, 1, 1, expect=ARG, n=-1) is None
    assert call(eng, clips, 1, 1, expect=ARG, misalign=True) is None
    assert call(eng, clips, 1, 1, n=0) is None                      # nothing to do: JG_OK, nothing written
    v = torch.zeros((4, 64), device="cuda")
    o = torch.zeros(2, dtype=torch.int32, device="cuda")
    f = torch.zeros(2, device="cuda")
    for args in ((None, P(o), P(v), P(o), P(o), P(f)), (P(v), None, P(v), P(o), P(o), P(f)), (P(v), P(o), None, P(o), P(o), P(f)),
                 (P(v), P(o), P(v), None, P(o), P(f)), (P(v), P(o), P(v), P(o), None, P(f)), (P(v), P(o), P(v), P(o), P(o), None)):
        assert eng.lib.jg_sync_offset(eng.h, args[0], args[1], args[2], args[3], 1, 64, 1, 1, None, args[4], args[5]) == ARG


def test_python_entries(eng):
    from jegal_amd import metrics
    clips = C.sweep_batch(64, 15)[:12]
    off, conf, curve = metrics.sync_offset([c[0] for c in clips], [c[1] for c in clips], max_shift=15, engine=eng)
    assert off.dtype == np.int32 and conf.dtype == np.float32 and curve.shape == (12, 31)
    hold("metrics.sync_offset", [check("metrics.sync_offset", (off, conf, curve), clips, 15, 1)])
    dev = metrics.sync_offset([torch.from_numpy(c[0]).cuda() for c in clips], [torch.from_numpy(c[1]).cuda() for c in clips], engine=eng)
    assert np.array_equal(dev[0], off) and np.array_equal(dev[2].view(np.int32), curve.view(np.int32))
    assert metrics.sync_offset([], [], engine=eng)[2].shape == (0, 31)
    with pytest.raises(ValueError):
        eng.sync_offset(torch.zeros(4, 96), torch.zeros(4, 96), [0, 4], [0, 4])
    with pytest.raises(ValueError):
        eng.sync_offset(torch.zeros(4, 64), torch.zeros(4, 64), [0, 4], [0, 4], max_shift=65)
