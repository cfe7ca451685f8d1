"""GestSync's audio stream on the GPU (run with -m gpu): jg_gestsync_audio_windows against the real reference's forward_aud
(tests/golden/gestsync_audio.npz, tools/make_golden_gestsync_audio.py), the clip form against the window form, refusals, weight
finalisation, and the stream's two own kernels against float64 (tests/gestsync_audio_cases.py).

Parity: rel-L2 over the batch.  Default mode (JG_PREC_FP16_RC) <= 1e-3, the project's contract; JG_PREC_FP32 <= 2e-5, the audit mode's
bound against reference goldens.  Measured on MI355X (N = 1 / 3 / 29): see the prints; the figures are recorded in DESIGN.md section 5.
The rows of different windows are 0.93-0.996 correlated under the synthetic weights, so the error after subtracting the batch's mean row
is printed beside the raw one (not asserted)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gestsync_audio_cases as K
from jegal_amd import synth
from jegal_amd._lib import PREC_BF16, PREC_FP32, Engine, JegalError

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
ARG, STATE, WEIGHT = -1, -3, -4


@pytest.fixture(scope="module")
def sd():
    return synth.gestsync_state_dict(family="gauss")


def make_engine(sd, precision=None, which=8):
    e = Engine(0, precision=precision)
    e.load_tensors(sd)
    e.finalize(which)
    return e


@pytest.fixture(scope="module")
def eng(sd):
    e = make_engine(sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "gestsync_audio.npz"))
    x = np.random.default_rng(int(g["seed"])).standard_normal((29, 1, 80, 100)).astype(np.float32)
    assert g["out"].shape == (29, 1024) and (g["active"] > 0.2).all() and (g["active"] < 0.8).all()
    return x, g["out"].astype(np.float64)


def rel(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def bits(t):
    return t.cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize("mode,bound", [(None, 1e-3), (PREC_FP32, 2e-5)])
def test_forward_aud_matches_the_reference(sd, eng, golden, mode, bound):
    """N = 1, 3, 29: M = 1 / 3 / 29 rows for fc6 .. fc8, 45 / 135 / 1305 pixels for conv3 .. conv5 -- the register-staged and the LDS-DMA
    GEMM instances, both sides of the 1024-row line"""
    x, ref = golden
    e = eng if mode is None else make_engine(sd, mode)
    try:
        for N in (1, 3, 29):
            out = e.gestsync_audio_windows(torch.from_numpy(x[:N])).cpu().numpy().astype(np.float64)
            assert out.shape == (N, 1024) and np.isfinite(out).all()
            r = rel(out, ref[:N])
            c = rel(out - out.mean(0), ref[:N] - ref[:N].mean(0)) if N > 1 else float("nan")
            print(f"forward_aud mode {mode} N={N}: rel-L2 {r:.3e}   batch mean row removed: {c:.3e}")
            assert r <= bound, (mode, N, r)
    finally:
        if mode is not None:
            e.close()


def test_facade_forward_aud_and_finalize_bits(sd, golden):
    from jegal_amd.gestsync import GestSync
    x, ref = golden
    e = Engine(0)
    try:
        gs = GestSync(engine=e).load_state_dict(sd)                  # bits 0 and 3 in one finalize
        assert e.finalized == 9
        out = gs.forward_aud(torch.from_numpy(x[:3]))
        assert tuple(out.shape) == (3, 1024, 1)
        assert rel(out[:, :, 0].cpu().numpy().astype(np.float64), ref[:3]) <= 1e-3
        mel = torch.randn(1, 40, 80)
        assert tuple(gs.extract_clip_audio_feats(mel, 10).shape) == (1, 10, 1024)
        assert tuple(gs.extract_clip_audio_feats(mel[0], 10).shape) == (1, 10, 1024)
        # a checkpoint without audio keys: bit 0 alone still works, bit 3 fails strictly, the facade says what is missing
        video_only = synth.gestsync_state_dict(family="gauss", include_unused=False)
        gs2 = GestSync(engine=e).load_state_dict(video_only)
        assert tuple(gs2.extract_clip_feats(torch.from_numpy(synth.synth_frames(3, 1, 5)).to(e.device)).shape) == (1, 5, 1024)
        with pytest.raises(RuntimeError, match="no audio stream"):
            gs2.forward_aud(torch.from_numpy(x[:1]))
        e.load_tensors(video_only)
        with pytest.raises(JegalError, match="net_aud.conv1.weight") as err:
            e.finalize(8)
        assert err.value.code == WEIGHT
    finally:
        e.close()


def test_sync_offset_driver_is_the_composition(sd, tmp_path, capsys, golden_dir):
    """drivers sync_offset = extract_clip_feats + (log-mel | --mel) + extract_clip_audio_feats + metrics.sync_offset, written to .sync.npz"""
    from jegal_amd import drivers, metrics
    from jegal_amd.gestsync import GestSync
    e = Engine(0)
    try:
        gs = GestSync(engine=e).load_state_dict(sd)
        T = 30
        frames = synth.synth_frames(9, 1, T)[0]
        mel = np.random.default_rng(3).standard_normal((4 * T - 6, 80)).astype(np.float32)
        np.save(tmp_path / "clip.npy", frames)
        np.save(tmp_path / "clip_mel.npy", mel)
        ckpt = ["--checkpoint_path_gestsync", "synthetic"]
        assert drivers.cmd_sync_offset(ckpt + ["--frames", str(tmp_path / "clip.npy"), "--mel", str(tmp_path / "clip_mel.npy"), "--max_shift", "7",
                                               "--res_dir", str(tmp_path)], engine=e, gestsync=gs) == 0
        said = capsys.readouterr().out
        assert "AV offset:" in said and "WARNING: synthetic GestSync weights" in said and "MEANINGLESS" in said
        got = np.load(tmp_path / "clip.sync.npz")
        vid = gs.extract_clip_feats(torch.from_numpy(frames).to(e.device))[0]
        aud = gs.extract_clip_audio_feats(torch.from_numpy(mel), 29)[0]                    # ceil(114 / 4) audio windows
        off, conf, curve = metrics.sync_offset([vid], [aud], 7, engine=e)
        assert got["offset"] == off[0] and -7 <= int(got["offset"]) <= 7 and got["curve"].shape == (15,)
        assert np.array_equal(got["curve"].view(np.int32), curve[0].view(np.int32)) and got["conf"] == conf[0] and np.isfinite(got["conf"])
        assert list(got["shifts"]) == list(range(-7, 8))
        # --wav: the library's own log-mel front end in front of the same composition
        assert drivers.cmd_sync_offset(ckpt + ["--frames", str(tmp_path / "clip.npy"), "--wav", os.path.join(golden_dir, "sample1.wav"),
                                               "--res_dir", str(tmp_path / "w")], engine=e, gestsync=gs) == 0
        w = np.load(tmp_path / "w" / "clip.sync.npz")
        assert w["curve"].shape == (31,) and np.isfinite(w["conf"])
        with pytest.raises(SystemExit):                        # neither --wav nor --mel
            drivers.cmd_sync_offset(ckpt + ["--frames", str(tmp_path / "clip.npy")], engine=e, gestsync=gs)
        with pytest.raises(SystemExit):                        # the checkpoint is required: no silent synthetic default
            drivers.cmd_sync_offset(["--frames", str(tmp_path / "clip.npy"), "--mel", str(tmp_path / "clip_mel.npy")], engine=e, gestsync=gs)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ clip form against window form
def clip_inputs():
    g = np.random.default_rng(31)
    return g.standard_normal((2, 37, 80)).astype(np.float32), g.standard_normal((2, 100, 80)).astype(np.float32)


@pytest.mark.parametrize("Tm,valid", [(37, None), (100, None), (100, (100, 61)), (37, (5, 37))])
def test_clip_form_equals_window_form_bit_for_bit(eng, Tm, valid):
    """B = 2, T = 9: x built on the host with the documented gather; the two entries at equal N give equal bits"""
    mel = clip_inputs()[0 if Tm == 37 else 1]
    x = K.gather_windows(mel, 9, valid)
    a = eng.gestsync_audio_clip(torch.from_numpy(mel), 9, valid)
    b = eng.gestsync_audio_windows(torch.from_numpy(x))
    assert tuple(a.shape) == (2, 9, 1024)
    assert np.array_equal(bits(a).reshape(18, 1024), bits(b))


def test_a_clip_does_not_see_a_longer_neighbour_and_passes_repeat(eng):
    short, long_ = clip_inputs()
    g = np.random.default_rng(32)
    pad_a, pad_b = (np.concatenate([short[:1], g.standard_normal((1, 63, 80)).astype(np.float32)], 1) for _ in range(2))
    other = g.standard_normal((1, 100, 80)).astype(np.float32)
    r1 = eng.gestsync_audio_clip(torch.from_numpy(np.concatenate([pad_a, long_[:1]])), 9, (37, 100))
    r2 = eng.gestsync_audio_clip(torch.from_numpy(np.concatenate([pad_b, other])), 9, (37, 100))
    r3 = eng.gestsync_audio_clip(torch.from_numpy(short), 9)                      # the clip in a batch of its own length, same N
    assert np.array_equal(bits(r1)[0], bits(r2)[0]) and np.array_equal(bits(r1)[0], bits(r3)[0])
    assert not np.array_equal(bits(r1)[1], bits(r2)[1])
    # the workspace poisoned before the pass, and the pass twice in a row: the same bits
    eng.set_option("ws_poison", 1)
    try:
        p1 = eng.gestsync_audio_clip(torch.from_numpy(np.concatenate([pad_a, long_[:1]])), 9, (37, 100))
        p2 = eng.gestsync_audio_clip(torch.from_numpy(np.concatenate([pad_a, long_[:1]])), 9, (37, 100))
    finally:
        eng.set_option("ws_poison", 0)
    assert np.isfinite(p1.cpu().numpy()).all()
    assert np.array_equal(bits(p1), bits(r1)) and np.array_equal(bits(p2), bits(r1))


def test_more_windows_than_one_workspace_pass(eng):
    """B T = 4200 windows run as two workspace passes (4096 + 104: gestsync_audio.hip, GSA_PASS_WINDOWS), the second one with a window
    offset, its own upload of the lengths and its own part of the output.  A pass's GEMM instances depend on its size alone, so each pass
    equals, bit for bit, the window form on the same gathered windows; and the whole call agrees with the clips run as two halves (one
    pass each, other sizes: the planner may pick other instances) within the parity contract, also on the second pass's rows alone."""
    B, T, Tm, PASS = 28, 150, 600, 4096
    g = np.random.default_rng(41)
    mel = g.standard_normal((B, Tm, 80)).astype(np.float32)
    valid = [int(v) for v in g.integers(300, Tm + 1, B)]
    valid[-1] = 333                                                               # the last clip (second pass) ends well inside its rows
    whole = eng.gestsync_audio_clip(torch.from_numpy(mel), T, valid).reshape(B * T, 1024)
    x = torch.from_numpy(K.gather_windows(mel, T, valid)).cuda()
    first, second = eng.gestsync_audio_windows(x[:PASS]), eng.gestsync_audio_windows(x[PASS:])
    assert np.array_equal(bits(whole[:PASS]), bits(first)) and np.array_equal(bits(whole[PASS:]), bits(second))
    h = B // 2
    halves = torch.cat([eng.gestsync_audio_clip(torch.from_numpy(mel[:h]), T, valid[:h]),
                        eng.gestsync_audio_clip(torch.from_numpy(mel[h:]), T, valid[h:])]).reshape(B * T, 1024)
    w, s = whole.cpu().numpy().astype(np.float64), halves.cpu().numpy().astype(np.float64)
    assert np.isfinite(w).all()
    r_all, r_tail = rel(w, s), rel(w[PASS:], s[PASS:])
    print(f"4200 windows in two passes against two calls of 2100: rel-L2 {r_all:.3e}, rows of the second pass {r_tail:.3e}")
    assert r_all <= 1e-3 and r_tail <= 1e-3


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(sd, eng):
    x = torch.zeros((2, 1, 80, 100), device="cuda")
    mel = torch.zeros((2, 40, 80), device="cuda")
    out = torch.full((2 * 4 * 1024,), 7.0, device="cuda")
    L = eng.lib
    eng._bind_stream()
    v = lambda *a: (ctypes.c_int32 * len(a))(*a)
    assert L.jg_gestsync_audio_windows(eng.h, P(x), 0, P(out)) == ARG
    assert L.jg_gestsync_audio_windows(eng.h, P(x), -1, P(out)) == ARG
    assert L.jg_gestsync_audio_windows(eng.h, None, 2, P(out)) == ARG
    assert L.jg_gestsync_audio_windows(eng.h, P(x), 2, None) == ARG
    for B, Tm, T, val in ((0, 40, 4, None), (2, 0, 4, None), (2, 40, 0, None), (2, 40, 4, v(0, 40)), (2, 40, 4, v(40, 41))):
        assert L.jg_gestsync_audio_clip(eng.h, P(mel), B, Tm, T, val, P(out)) == ARG, (B, Tm, T)
    assert L.jg_gestsync_audio_clip(eng.h, None, 2, 40, 4, None, P(out)) == ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                   # nothing was enqueued
    fresh = Engine(0)
    try:
        fresh._bind_stream()
        assert L.jg_gestsync_audio_windows(fresh.h, P(x), 2, P(out)) == STATE
        assert L.jg_gestsync_audio_clip(fresh.h, P(mel), 2, 40, 4, None, P(out)) == STATE
    finally:
        fresh.close()
    bf = make_engine(sd, PREC_BF16)
    try:
        bf._bind_stream()
        assert L.jg_gestsync_audio_windows(bf.h, P(x), 2, P(out)) == STATE
        assert b"bf16" in L.jg_last_error(bf.h)
        with pytest.raises(JegalError):
            bf.gestsync_audio_clip(mel, 4)
    finally:
        bf.close()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ the stream's own kernels
GUARD = 2          # guard windows / images in front of and behind every output


def guarded(n, shape, dtype):
    buf = torch.full((n + 2 * GUARD,) + shape, 777.0, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_ok(buf, n):
    return bool((buf[:GUARD] == 777.0).all()) and bool((buf[GUARD + n:] == 777.0).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_gsa_conv1_pool_kernel_vs_fp64(eng, dtype):
    """both input forms, both output types; bound per element 10 u sum |terms| (+ one fp16 ulp for fp16 output)"""
    w, s = K.weights()
    wd, sdv = torch.from_numpy(w).cuda(), torch.from_numpy(s).cuda()
    cases = [("windows", K.window_cases(), None, None, None)]
    for mel, T, valid in K.clip_cases():
        cases.append((f"clip Tm={mel.shape[1]} T={T} valid={valid}", K.gather_windows(mel, T, valid), mel, T, valid))
    worst = 0.0
    for name, x, mel, T, valid in cases:
        ref, bound = K.conv1_pool_ref(x, w, s)
        if dtype == torch.float16:
            bound = bound + K.ulp16(ref)
        n = x.shape[0]
        buf, out = guarded(n, (19, 24, 64), dtype)
        if mel is None:
            eng.debug_gsa_conv1_pool(torch.from_numpy(x).cuda(), wd, sdv, out)
        else:
            eng.debug_gsa_conv1_pool(torch.from_numpy(mel).cuda(), wd, sdv, out, T=T, lengths=valid)
        torch.cuda.synchronize()
        kn = eng.debug_last_kernel()
        assert kn == "gsa_conv1_pool_kernel<{}> {}".format("f16" if dtype == torch.float16 else "float", "windows" if mel is None else "clip"), kn
        assert guards_ok(buf, n), name
        got = out.cpu().double().numpy()
        assert np.isfinite(got).all(), name
        err = np.abs(got - ref)
        r = float(np.where(err == 0, 0.0, err / bound).max())
        worst = max(worst, r)
        assert r <= 1.0, (name, r)
    print(f"gsa_conv1_pool {dtype}: worst error / bound {worst:.3f}")


def test_gsa_conv1_pool_rejections(eng):
    w, s = K.weights()
    wd, sdv = torch.from_numpy(w).cuda(), torch.from_numpy(s).cuda()
    x = torch.zeros((1, 1, 80, 100), device="cuda")
    out = torch.full((19 * 24 * 64 + 8,), 5.0, dtype=torch.float16, device="cuda")
    eng._bind_stream()
    L = eng.lib
    assert L.jg_debug_gsa_conv1_pool(eng.h, P(x), 0, 1, 0, 2, None, P(wd), P(sdv), P(out), 0) == ARG          # window form with T != 1
    assert L.jg_debug_gsa_conv1_pool(eng.h, P(x), 1, 1, 0, 1, None, P(wd), P(sdv), P(out), 0) == ARG          # clip form without rows
    assert L.jg_debug_gsa_conv1_pool(eng.h, P(x), 0, 1, 0, 1, None, None, P(sdv), P(out), 0) == ARG
    assert L.jg_debug_gsa_conv1_pool(eng.h, P(x), 0, 1, 0, 1, None, P(wd), P(sdv), ctypes.c_void_p(out.data_ptr() + 2), 0) == ARG
    assert L.jg_debug_gsa_conv1_pool(eng.h, P(x), 1, 1, 100, 1, (ctypes.c_int32 * 1)(101), P(wd), P(sdv), P(out), 0) == ARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_maxpool_2x3_is_exact(eng, dtype):
    for Hi, Wi in K.POOL_SHAPES:
        for Ci in K.POOL_C:
            x = K.pool_case(Hi, Wi, Ci, dtype)
            ref = K.pool_ref(x)
            buf, out = guarded(3, tuple(ref.shape[1:]), dtype)
            eng.debug_maxpool_2x3(x.cuda(), out)
            torch.cuda.synchronize()
            assert eng.debug_last_kernel() == "maxpool_2x3_s2_kernel<{}>".format("f16" if dtype == torch.float16 else "float")
            assert guards_ok(buf, 3), (Hi, Wi, Ci)
            assert torch.equal(out.cpu(), ref), (Hi, Wi, Ci)
    x = torch.zeros((1, 4, 4, 12), dtype=dtype, device="cuda")
    out = torch.zeros((1, 2, 1, 12), dtype=dtype, device="cuda")
    with pytest.raises(JegalError) as err:                 # C % 8
        eng.debug_maxpool_2x3(x, out)
    assert err.value.code == ARG
    with pytest.raises(JegalError):                        # narrower than the window
        eng.debug_maxpool_2x3(torch.zeros((1, 4, 2, 8), dtype=dtype, device="cuda"), out)
