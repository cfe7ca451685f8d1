"""Where a workspace pass begins (engine.h, begin_pass): every entry point that uses the stream-ordered arena takes it back to its start
in ONE place, which also fills it with NaN bytes under option ws_poison and clears the conv report (jg_debug_conv2_rowskip /
jg_debug_conv_rows), whose device words lie in the pass's workspace.

(1) Every such entry is reproducible under poison: without the option a stale or uninitialised read of the workspace returns the
previous identical run's bytes and is invisible; with it the read is NaN, so finite results that stay bit-identical from run to run
say that no kernel reads what its pass has not written.  Shapes on both sides of the 128-row line below which the planner leaves the
LDS-DMA GEMM kernel.  (tests/test_gpu_audit_fp32.py runs the JEGAL cases once more on the fp32 audit engine.)
(2) The conv report describes the last conv stack of the last call and reads 0 / 0 once another pass has begun or the stream was switched.
Default-mode engine, synthetic weights, through the C ABI."""
import numpy as np
import pytest
import torch

from jegal_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from jegal_amd._lib import Engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Engine.get("cuda:0")


@pytest.fixture(scope="module")
def models(engine):
    from jegal_amd.gestsync import GestSync
    from jegal_amd.jegal import JEGAL
    gs = GestSync(engine=engine).load_state_dict(synth.gestsync_state_dict(include_unused=False))
    jg = JEGAL(engine=engine).load_state_dict(synth.jegal_state_dict())
    return gs, jg


# ---- the cases: each builds its inputs once and returns call(engine) -> output tensor
def _masked(rng, B, L, D, tail):
    """(B, L, D) standard-normal rows and a (B, L) key mask with the last `tail` rows of clip 1 masked and zeroed (tail = 0: no mask)"""
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    if not tail:
        return torch.from_numpy(x).cuda(), None
    m = np.ones((B, L), np.float32)
    x[1, L - tail:] = 0
    m[1, L - tail:] = 0
    return torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda()


def _gestures(B, T, tail):
    feats, mask = _masked(np.random.default_rng(1000 + T), B, T, 1024, tail)
    return lambda e: e.jegal_gestures(feats, mask, align=True)


def _text(B, L, tail):
    states, mask = _masked(np.random.default_rng(2000 + L), B, L, 768, tail)
    return lambda e: e.jegal_text(states, mask)


def _audio(valid):
    mel = synth.synth_mel(31, 2, 64)
    for b, v in enumerate(valid or []):
        mel[b, v:] = 0                         # a zero-padded batch
    mel = torch.from_numpy(mel).cuda()
    return lambda e: e.jegal_audio(mel, valid_len=valid)


def _fuse(rows):
    fused = torch.from_numpy(np.random.default_rng(3000 + rows).standard_normal((rows, 512)).astype(np.float32)).cuda()
    return lambda e: e.fuse_content(fused)


def _windows(N):
    x = torch.from_numpy(np.random.default_rng(4000 + N).random((N, 3, 25, 270, 480), dtype=np.float32)).cuda()
    return lambda e: e.gestsync_windows(x)


CASES = {
    "gestures-1x25": lambda: _gestures(1, 25, 0),                 # 25 rows
    "gestures-2x70-masked": lambda: _gestures(2, 70, 9),          # 140 rows, the last 9 frames of clip 1 masked
    "text-2x33-masked": lambda: _text(2, 33, 5),                  # 66 rows, the last 5 tokens of clip 1 masked
    "text-4x40": lambda: _text(4, 40, 0),                         # 160 rows
    "audio-2x64": lambda: _audio(None),
    "audio-2x64-ragged": lambda: _audio([64, 37]),
    "fuse-5": lambda: _fuse(5),
    "fuse-300": lambda: _fuse(300),
    "windows-2": lambda: _windows(2),
}
JEGAL_SMALL = ("gestures-1x25", "text-2x33-masked", "audio-2x64", "audio-2x64-ragged", "fuse-5")      # the fp32 audit engine runs these as well


def assert_reproducible_under_poison(e, call):
    e.set_option("ws_poison", 0)
    ref = call(e).clone()
    assert torch.isfinite(ref).all()
    e.set_option("ws_poison", 1)
    try:
        for _ in range(3):
            assert torch.equal(call(e), ref)
    finally:
        e.set_option("ws_poison", 0)


@pytest.mark.parametrize("name", list(CASES))
def test_entry_is_reproducible_under_a_poisoned_workspace(engine, models, name):
    assert_reproducible_under_poison(engine, CASES[name]())


def test_conv_report_lives_until_the_next_pass(engine, models):
    """Two clips of 9 frames with rows 0..109 zero: every position's conv2 leaves out 6 rows.  The report is there after
    jg_extract_gesture -- whose JEGAL stage runs in the pass of its GestSync stage, behind its buffers, also when the pass is poisoned --
    and gone after a later call that begins a pass (jg_jegal_text), or after a call under another stream."""
    rng = np.random.default_rng(41)
    clips = rng.integers(1, 256, (2, 9, 270, 480, 3), dtype=np.uint8)
    clips[:, :, :110] = 0
    frames = torch.from_numpy(clips).cuda()
    states = torch.from_numpy(rng.standard_normal((1, 6, 768)).astype(np.float32)).cuda()
    none = ([0, 0, 0, 0], [0, 0, 0, 0])

    def report_is_there():
        computed, full = engine.debug_conv_rows()
        assert 0 < computed[0] < full[0]
        assert engine.debug_conv2_rowskip() == 6

    engine.set_option("dual_stream", 0)
    try:
        for poison in (0, 1):
            engine.set_option("ws_poison", poison)
            emb = engine.extract_gesture(frames)
            report_is_there()
            assert torch.isfinite(emb).all()
        engine.set_option("ws_poison", 0)
        engine.jegal_text(states)
        assert engine.debug_conv2_rowskip() == 0 and engine.debug_conv_rows() == none
        engine.extract_gesture(frames)
        report_is_there()
        with torch.cuda.stream(torch.cuda.Stream()):
            engine.l2norm(states)
        assert engine.debug_conv2_rowskip() == 0 and engine.debug_conv_rows() == none
    finally:
        engine.set_option("ws_poison", 0)
        engine.set_option("dual_stream", 1)
