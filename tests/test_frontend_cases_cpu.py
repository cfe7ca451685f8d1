"""The cases of tests/frontend_fp64_cases.py checked against themselves, without a GPU.

logmel: the float64 reference agrees with the oracle's fp32 torch.stft statement where that can be told (noise, log domain); a float32 numpy
restatement of logmel_kernel (sequential DFT and mel sums, float32 window and twiddles) stays inside the derived linear-domain bound on every
signal and both bases, silence within 2 ulp of log(1e-20); and each planted defect of the restatement leaves the bound on at least one case:
    window offset 95 instead of 96; reflect replaced by clamp; bin 256 dropped; hop 159; the last frame kept instead of dropped (the first one
    goes); row stride 160 * frames instead of n_samples.
mask_resize: the launcher's dispatch rule as restated by the case module, the packed form's layout, and what the oracle must return whatever its
arithmetic: blanked frames, the rows of a frame without a face, a 1-pixel source.
"""
import numpy as np
import pytest
import torch

import frontend_fp64_cases as C
import jegal_oracle as O

MUTANTS = {"window_at_95": dict(win_off=95), "clamp_for_reflect": dict(clamp=True), "no_bin_256": dict(drop_nyquist=True), "hop_159": dict(hop=159),
           "last_frame_kept": dict(keep_last=True), "row_stride_160_frames": "stride"}


@pytest.fixture(scope="module")
def batches():
    return C.logmel_batches()


def test_logmel_reference_against_the_oracle(batches):
    basis = C.real_basis()
    for name in ("noise257", "noise481", "noise1600"):
        wav = batches[name]
        m, _ = C.logmel_ref(wav, basis)
        want = O.wav2filterbanks(torch.from_numpy(wav), torch.from_numpy(basis)).double().numpy()
        assert want.shape == m.shape == (3, wav.shape[1] // 160, 80)
        assert float(np.abs(np.log(m + 1e-20) - want).max()) < 2e-3, name
    for n in (160, 200, 256):          # what the entry now refuses, the reference's own front end cannot do either
        with pytest.raises(RuntimeError):
            O.wav2filterbanks(torch.zeros(1, n), torch.from_numpy(basis))


def test_logmel_restatement_inside_bound_and_mutants_outside(batches):
    bases = {"mel": C.real_basis(), "synthetic": C.synthetic_basis()}
    assert [int(np.flatnonzero(bases["synthetic"][r])[0]) for r in range(5)] == list(C.ONE_HOT_BINS) and bool((bases["synthetic"][5:] > 0).all())
    assert float(bases["mel"][:, 256].max()) == 0.0, "the Slaney bank ends at Nyquist: only the synthetic basis sees bin 256"
    caught = {m: 0 for m in MUTANTS}
    worst, strides = 0.0, 0
    for name, wav in batches.items():
        n = wav.shape[1]
        mag = C.logmel_dft32(wav)
        assert mag.shape == (3, n // 160, 257)
        mags = {}
        for mu, kw in MUTANTS.items():
            if kw == "stride":
                mags[mu] = C.logmel_dft32(wav, stride=160 * (n // 160))
                strides += n % 160 != 0
            elif "drop_nyquist" not in kw:
                mags[mu] = C.logmel_dft32(wav, **kw)
        for bname, basis in bases.items():
            m, delta = C.logmel_ref(wav, basis)
            r, fails = C.logmel_fails(name, C.logmel_mel32(mag, basis), m, delta, wav)
            print(f"logmel {name:22s} {bname:10s} restatement observed/bound {r:.5f}")
            assert fails == [], fails
            worst = max(worst, r)
            for mu in MUTANTS:
                out = C.logmel_mel32(mag, basis, drop_nyquist=True) if mu == "no_bin_256" else C.logmel_mel32(mags[mu], basis)
                caught[mu] += bool(C.logmel_fails(name, out, m, delta, wav)[1])
    print(f"logmel: float32 restatement, worst observed/bound {worst:.5f}; cases that caught each defect: {caught}")
    # (the largest figure is the impulse's silent frames: the fp32 rounding of log(1e-20) against the second term alone; signals stay below 0.01)
    assert worst < 0.1, "the restatement sits far inside: the bound is about structure"
    assert strides >= 4 and all(caught.values()), caught


def test_mask_resize_cases():
    assert C.mr_banded(270, 1706) and not C.mr_banded(270, 1707) and not C.mr_banded(270, 1706, ptr=1)
    assert sorted(int(v) for H in (9,) for m in C.mr_masks(H) for v in m) == [-1, 0, 3, 7, 8, 59]
    for H, W in [(1, 1), (2, 3), (5, 4000)]:
        fr = C.mr_frames(H, W)
        for my in C.mr_masks(H):
            ref = O.mask_resize_frames(fr, my)
            assert ref.shape == (3, 270, 480, 3) and ref.dtype == np.uint8
            packed, off = C.mr_pack(fr, my)
            assert packed.size == sum((H - C.mr_first_row(int(v), H)) * W * 3 for v in my) and off[0] == 0
            for f in range(3):
                row0 = C.mr_first_row(int(my[f]), H)
                assert np.array_equal(packed[off[f]:off[f] + (H - row0) * W * 3], fr[f, row0:].reshape(-1))
                if my[f] >= H - 1:
                    assert not ref[f].any()          # every source row blanked
                if my[f] < 0:
                    assert not ref[f, :111].any()
                    if (H, W) == (1, 1):
                        assert bool((ref[f, 111:] == fr[f, 0, 0]).all())          # a 1-pixel source: its colour everywhere
