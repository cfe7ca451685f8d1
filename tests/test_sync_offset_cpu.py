"""jg_sync_offset without a GPU: the float64 and float32 numpy statements of its contract agree on the planted inputs, every planted clip
is decidable (so tests/test_gpu_sync_offset.py may demand the float64 arg-max of every clip, none exempt), and the Python entries exist
and refuse loudly to run without a device."""
import numpy as np
import pytest
import torch

import sync_offset_cases as C


def all_cases():
    for D, R in C.SWEEP:
        yield f"sweep D={D} R={R}", C.sweep_batch(D, R), R, 1
    for name, (clips, R, mo) in C.special_clips().items():
        yield name, clips, R, mo


def test_statements_agree_and_every_planted_clip_is_decidable():
    worst_margin, n, total, no_shift = np.inf, 0, 0, 0
    for name, clips, R, mo in all_cases():
        total += len(clips)
        for i, (v, a) in enumerate(clips):
            o64, c64, k64 = C.sync_ref(v, a, R, mo)
            o32, c32, k32 = C.sync_ref(v, a, R, mo, np.float32)
            assert np.array_equal(np.isnan(k64), np.isnan(k32)), (name, i)
            if np.isnan(k64).all():
                assert o64 == o32 == 0 and np.isnan(c64) and np.isnan(c32), (name, i)
                no_shift += 1
                continue
            m = C.margin(k64)
            assert m >= C.MARGIN, (name, i, v.shape, a.shape, m)
            worst_margin = min(worst_margin, m)
            assert o64 == o32, (name, i)
            assert np.nanmax(np.abs(k64 - k32)) < 2e-6 and abs(c64 - c32) < 4e-6, (name, i)
            n += 1
    print(f"{n} decidable clips of {total}, {no_shift} without any shift, smallest float64 margin {worst_margin:.3e}")
    # every clip that the GPU test runs: the 37 of each sweep and the special ones; the five without a shift have nothing to decide
    assert total == 37 * len(C.SWEEP) + sum(len(c[0]) for c in C.special_clips().values()) and n + no_shift == total and no_shift == 5


def test_the_statement_on_cases_worked_by_hand():
    e = np.eye(64, dtype=np.float32)
    # video rows e0 e1 e2, audio rows x e0 e1 e2: the audio row of video row t is t + 1
    off, conf, curve = C.sync_ref(e[:3], np.concatenate([e[10:11], e[:3]]), 2, 1)
    assert off == 1 and np.allclose(curve, [0, 0, 0, 1, 0]) and conf == 1.0
    # min_overlap: shift -2 has 1 pair, -1 has 2, 0 .. 1 have 3, 2 has 2
    assert np.array_equal(np.isnan(C.sync_ref(e[:3], np.concatenate([e[10:11], e[:3]]), 2, 3)[2]), [True, True, False, False, True])
    # the median of an even count is the mean of the two middle entries; ties go to the first shift
    off, conf, curve = C.sync_ref(e[:2], e[:2] * 0, 1, 1)
    assert off == -1 and conf == 0.0 and np.array_equal(curve, [0, 0, 0])
    # limits: an empty or oversized stream
    for v, a in ((e[:0], e[:3]), (e[:3], e[:0]), (np.zeros((C.MAX_T + 1, 64), np.float32), e[:3])):
        off, conf, curve = C.sync_ref(v, a, 1, 1)
        assert off == 0 and np.isnan(conf) and np.isnan(curve).all()
    clips, R, mo = C.special_clips()["duplicates"]
    off, _, curve = C.sync_ref(*clips[0], R, mo)
    assert off == 0 and curve[R] == curve[R + 2] and curve[R + 1] == curve[R + 3] and curve[R] > curve[R + 1] and np.isnan(curve[:R]).all()


def test_entries_exist_and_refuse_without_a_gpu():
    from jegal_amd import metrics
    from jegal_amd._lib import EXPORTS, Engine
    from jegal_amd.gestsync import GestSync
    for name in ("jg_sync_offset", "jg_gestsync_audio_windows", "jg_gestsync_audio_clip", "jg_debug_gsa_conv1_pool", "jg_debug_maxpool_2x3"):
        assert name in EXPORTS
    for cls, names in ((GestSync, ("forward_aud", "extract_clip_audio_feats")),
                       (Engine, ("sync_offset", "gestsync_audio_windows", "gestsync_audio_clip"))):
        for nm in names:
            assert callable(getattr(cls, nm)), (cls, nm)
    assert callable(metrics.sync_offset)
    if torch.cuda.is_available():
        return          # a device is present: there is no refusal to show
    v = np.zeros((4, 64), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GestSync()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.sync_offset([v], [v])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine.get().sync_offset(v, v, [0, 4], [0, 4])
