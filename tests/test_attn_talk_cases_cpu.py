"""The inputs of tests/test_gpu_attn_talk.py are checked here, without a GPU: the float64 evaluation of the talk heat map
(tests/attn_talk_cases.py) equals the float64 formula of tests/test_gpu_attn_matrix.py once every word is in reach, and every accuracy input
has at least 90 % decidable words and frames (decidable as in that file: the float64 best beats the runner-up by more than 1e-3 relative),
so the exact arg-max assertions of the GPU tests bite.

Measured with this recipe (tests/attn_talk_cases.py: ACCURACY_INPUTS):
  (seed, T, W, span, gap, reach, D)       decidable words, normalize 1 / 0   decidable frames, 1 / 0   candidates per block
  (20, 700, 140, 4, 1, 40, 512)           0.979 / 0.986                      1.000 / 1.000             at most 43
  (21, 1000, 400, 2, 1, 25, 512)          1.000 / 0.991 (342 words in reach) 0.997 / 0.997             at most 60
  (30, 135, 20, 5, 2, 12, 64)             0.950 / 0.900                      1.000 / 1.000             at most 20
  (37, 135, 20, 5, 2, 12, 192)            0.950 / 0.900                      1.000 / 1.000             at most 20"""
import numpy as np
import pytest

import attn_talk_cases as C
from test_gpu_attn_matrix import ref64 as clip_ref64


def test_full_reach_is_the_clip_formula():
    for seed, (T, W, span, gap) in ((1, (300, 37, 6, 2)), (2, (129, 128, 1, 0))):
        g, c, s, e = C.planted_talk(seed, T, W, span, gap)
        for normalize in (1, 0):
            P = C.talk64(g, c, s, e, T, normalize)
            assert not np.isnan(P).any()
            assert np.array_equal(P, clip_ref64(g, c, normalize))
    # and a reach that cuts: a frame's probabilities sum to one over the words in reach of it, and are NaN elsewhere
    g, c, s, e = C.planted_talk(3, 135, 20, 5, 2)
    P = C.talk64(g, c, s, e, 12, 1)
    m = C.reach_mask(135, s, e, 12)
    assert np.array_equal(np.isnan(P), ~m)
    assert np.allclose(np.nansum(P, axis=0)[m.any(axis=0)], 1.0, rtol=0, atol=1e-12)
    assert P[0, 16] > 0 and np.isnan(P[0, 17])                      # word 0 ends at frame 4: in reach up to frame 16


@pytest.mark.parametrize("case", C.ACCURACY_INPUTS)
def test_gpu_inputs_are_decidable(case):
    seed, T, W, span, gap, reach, d = case
    g, c, s, e = C.planted_talk(seed, T, W, span, gap, d)
    cand = C.block_candidates(T, s, e, reach)
    print(f"{case}: candidates per block at most {cand.max()}, {(s < T).sum()} words fit")
    assert cand.max() <= C.MAX_BLOCK_W
    for normalize in (1, 0):
        P = C.talk64(g, c, s, e, reach, normalize)
        dw, hw = C.decidable(P, 1)
        df, hf = C.decidable(P, 0)
        assert hw.sum() == (s - reach < T).sum() and hf.all()         # (a word that starts less than reach behind the track has frames)
        print(f"{case} normalize={normalize}: decidable words {dw.sum() / hw.sum():.3f}, frames {df.sum() / hf.sum():.3f}")
        assert dw.sum() >= 0.9 * hw.sum() and df.sum() >= 0.9 * hf.sum()
        # the fp32 twin is a twin: the same entries, close to float64
        P32 = C.talk32(g, c, s, e, reach, normalize)
        assert np.array_equal(np.isnan(P32), np.isnan(P))
        ma, mr = C.err(P32, P)
        assert 0 < ma < 1e-5 and 0 < mr < 1e-4


def test_band_layout_and_best():
    g, c, s, e = C.planted_talk(4, 50, 6, 5, 2)
    P = C.talk64(g, c, s, e, 3, 1)
    pitch = C.band_pitch(s, e, 3)
    assert pitch == 11
    B = C.band_of(P, s, 3, pitch)
    assert np.isnan(B[0, :3]).all() and B[0, 3] == P[0, 0] and B[0, 10] == P[0, 7]      # word 0: frames -3 .. 7, cut at frame 0
    assert B[2, 0] == P[2, 11] and B[2, 10] == P[2, 21]
    bf, bs = C.word_best(P)
    for w in range(6):
        assert bf[w] == np.nanargmax(P[w]) and bs[w] == np.nanmax(P[w])
    fw, fp = C.frame_best(P)
    assert fw[0] == np.nanargmax(P[:, 0]) and fp[0] == np.nanmax(P[:, 0])
    assert fw[49] == -1 and np.isnan(fp[49])                        # the last word ends at frame 39: out of reach from 43 on
