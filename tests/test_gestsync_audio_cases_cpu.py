"""The cases of tests/gestsync_audio_cases.py checked where no GPU is: the float64 references agree with torch's own float32 layers within
the derived bounds, planted defects do not, and the documented window gather is what the references are built on."""
import numpy as np
import torch
import torch.nn.functional as F

import gestsync_audio_cases as K


def torch_conv1_pool(x, w, shift):
    """conv (3x3, stride 2, pad 1) + shift + ReLU + max-pool 3x3 / 2 in torch float32 -> NHWC"""
    y = F.conv2d(torch.from_numpy(x), torch.from_numpy(w).reshape(64, 1, 3, 3), torch.from_numpy(shift), stride=2, padding=1)
    return F.max_pool2d(torch.relu(y), 3, 2).permute(0, 2, 3, 1).numpy()


def worst(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    return float(np.where(err == 0, 0.0, err / bound).max())


def test_conv1_pool_reference_matches_torch_fp32_within_the_bound():
    w, s = K.weights()
    x = K.window_cases()
    ref, bound = K.conv1_pool_ref(x, w, s)
    got = torch_conv1_pool(x, w, s)
    assert got.shape == ref.shape == (8, 19, 24, 64)
    assert worst(got, ref, bound) <= 1.0
    # the lone values on band 79 / step 99 are never read: those windows equal an all-zero window, which is relu(shift) everywhere
    zero = np.broadcast_to(np.maximum(s.astype(np.float64), 0), ref[0].shape)
    for n in (5, 6, 7):
        assert np.array_equal(ref[n], zero)
    assert not np.array_equal(ref[4], zero)                 # the corner (0, 0) is read
    assert (bound > 0).all() and float(bound.max()) < 1e-4


def test_planted_defects_exceed_the_bound():
    w, s = K.weights()
    x = K.window_cases()[:3]
    ref, bound = K.conv1_pool_ref(x, w, s)
    w_bad = w.copy()
    w_bad[:, [1, 3]] = w_bad[:, [3, 1]]                     # taps (0, 1) and (1, 0) swapped: a transposed kernel
    assert worst(torch_conv1_pool(x, w_bad, s), ref, bound) > 100
    y = F.conv2d(torch.from_numpy(x), torch.from_numpy(w).reshape(64, 1, 3, 3), torch.from_numpy(s), stride=2, padding=1)
    no_relu = F.max_pool2d(y, 3, 2).permute(0, 2, 3, 1).numpy()
    assert worst(no_relu, ref, bound) > 100
    half = torch_conv1_pool(x, w, s).astype(np.float16).astype(np.float64)          # an fp16 output needs its ulp
    assert worst(half, ref, bound) > 1.0 and worst(half, ref, bound + K.ulp16(ref)) <= 1.0


def test_clip_form_is_the_documented_gather():
    for mel, T, valid in K.clip_cases():
        x = K.gather_windows(mel, T, valid)
        B, Tm, _ = mel.shape
        assert x.shape == (B * T, 1, 80, 100)
        for b in range(B):
            vt = Tm if valid is None else valid[b]
            assert np.array_equal(x[b * T + 0, 0, :, 0], mel[b, 0])                   # window 0 starts 48 rows before the clip: row 0
            assert np.array_equal(x[b * T + T - 1, 0, :, 99], mel[b, min(4 * (T - 13) + 99, vt - 1)])
            t = T - 1                                                                 # 4 (t - 12) + w inside the clip: the row itself
            ws = [w_ for w_ in range(100) if 0 <= 4 * (t - 12) + w_ < vt]
            for w_ in ws[:3]:
                assert np.array_equal(x[b * T + t, 0, :, w_], mel[b, 4 * (t - 12) + w_])
    # a clip's windows do not depend on what lies behind its own rows
    mel, T, valid = K.clip_cases()[1]
    other = mel.copy()
    other[1, valid[1]:] = 99.0
    assert np.array_equal(K.gather_windows(mel, T, valid)[T:], K.gather_windows(other, T, valid)[T:])


def test_maxpool_reference_is_torch_max_pool():
    for Hi, Wi in K.POOL_SHAPES:
        for Ci in K.POOL_C:
            for dt in (torch.float16, torch.float32):
                x = K.pool_case(Hi, Wi, Ci, dt)
                ref = K.pool_ref(x)
                got = F.max_pool2d(x.float().permute(0, 3, 1, 2), (2, 3), (2, 2)).permute(0, 2, 3, 1).to(dt)
                assert ref.shape == (3, (Hi - 2) // 2 + 1, (Wi - 3) // 2 + 1, Ci)
                assert torch.equal(ref, got)
    x = K.pool_case(9, 5, 8, torch.float32)
    assert not torch.equal(K.pool_ref(x), F.max_pool2d(x.permute(0, 3, 1, 2), (3, 3), (2, 2)).permute(0, 2, 3, 1))
