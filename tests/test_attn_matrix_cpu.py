"""The host side of the attention-matrix feature without a GPU: metrics.attention_matrices, metrics.spot_words and the attn_matrix
driver reach the device only through engine.attn_matrix, so a stand-in engine whose attn_matrix is the oracle drives them here; plus the
argument checks Engine.attn_matrix makes before it needs a device."""
import pickle

import numpy as np
import pytest
import torch

import jegal_oracle as O
from jegal_amd import drivers, metrics as M, synth
from jegal_amd._lib import _SIGS, Engine


class OracleEngine:
    """attn_matrix with Engine.attn_matrix's contract, computed by the oracle on the host"""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def attn_matrix(self, gesture, content, g_offsets, c_offsets, temp=0.07, normalize=True, want_matrix=True):
        self.calls.append(dict(n=len(g_offsets) - 1, normalize=normalize, want_matrix=want_matrix))
        g, c = np.asarray(gesture, np.float32), np.asarray(content, np.float32)
        mats = []
        for i in range(len(g_offsets) - 1):
            gi, ci = g[g_offsets[i]:g_offsets[i + 1]], c[c_offsets[i]:c_offsets[i + 1]]
            if normalize:
                mats.append(O.attn_matrix(gi, ci, temp))
            else:
                mats.append(torch.softmax(torch.mm(torch.from_numpy(gi), torch.from_numpy(ci).t()) / temp, dim=1).numpy().T)
        a_off = np.zeros(len(mats) + 1, np.int64)
        a_off[1:] = np.cumsum([m.size for m in mats])
        A = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mats])) if want_matrix else None
        bf = torch.from_numpy(np.concatenate([np.argmax(m, axis=1) for m in mats]).astype(np.int32))
        bs = torch.from_numpy(np.concatenate([m.max(axis=1) for m in mats]).astype(np.float32))
        return A, a_off, bf, bs


@pytest.fixture(scope="module")
def planted():
    return synth.planted_spotting(9006, 20, n_frames=60, n_words=10, noise=2.0)


def test_attention_matrices_lists_and_concatenated(planted):
    gest, cont, _, _ = planted
    eng = OracleEngine()
    mats = M.attention_matrices(gest, cont, engine=eng)
    assert eng.calls == [dict(n=20, normalize=True, want_matrix=True)]              # one call for the batch
    for g, c, a in zip(gest, cont, mats):
        assert a.shape == (10, 60) and a.dtype == np.float32
        assert np.array_equal(a, O.attn_matrix(g, c))
    ragged_g, ragged_c = [gest[0][:7], gest[1], gest[2][:33]], [cont[0][:1], cont[1][:4], cont[2]]
    goff, coff = np.array([0, 7, 67, 100]), np.array([0, 1, 5, 15])
    cat = M.attention_matrices(torch.from_numpy(np.concatenate(ragged_g)), torch.from_numpy(np.concatenate(ragged_c)), engine=eng,
                               offsets=(goff, torch.from_numpy(coff)), normalize=False)
    assert eng.calls[-1] == dict(n=3, normalize=False, want_matrix=True)
    assert [a.shape for a in cat] == [(1, 7), (4, 60), (10, 33)]
    assert np.all(cat[0] == 1.0)
    assert M.attention_matrices([], [], engine=OracleEngine()) == []


def test_spot_words_equals_the_reference_spotting(planted):
    gest, cont, bounds, targets = planted
    eng = OracleEngine()
    spots = M.spot_words(gest, cont, engine=eng)
    assert eng.calls == [dict(n=20, normalize=True, want_matrix=False)]
    assert len(spots) == 20
    for g, c, wb, t, (frames, scores) in zip(gest, cont, bounds, targets, spots):
        assert frames.shape == (10,) and scores.shape == (10,)
        _, pred, score = O.spotting_correct(g, c, wb, t)
        assert frames[t] == pred and float(scores[t]) == score
        assert np.array_equal(frames, np.argmax(O.attn_matrix(g, c), axis=1))
    assert M.spot_words([], [], engine=OracleEngine()) == []


def test_driver_reads_both_info_schemas_and_writes_npz(planted, tmp_path):
    import pandas as pd
    gest, cont, bounds, _ = planted
    src, res = tmp_path / "pkl", tmp_path / "res"
    src.mkdir()
    for i in range(3):
        wb = [[f"w{i}_{j}", b[1], b[2]] for j, b in enumerate(bounds[i])]
        info = {"fname": f"c{i}", "word_boundaries": wb, "text": "t"} if i == 1 else pd.Series({"filename": f"v/{i}", "word_boundaries": str(wb)})
        with open(src / f"clip{i}.pkl", "wb") as f:
            pickle.dump({"gesture_emb": gest[i], "content_emb": cont[i], "info": info}, f)
    eng = OracleEngine()
    assert drivers.cmd_attn_matrix(["--path", str(src), "--res_dir", str(res)], engine=eng) == 0
    assert eng.calls == [dict(n=3, normalize=False, want_matrix=True)]              # plot_heatmap semantics by default, one call
    for i in range(3):
        z = np.load(res / f"clip{i}.attn.npz")
        assert sorted(z.files) == ["attn", "best_frame", "best_score", "words"]
        want = torch.softmax(torch.mm(torch.from_numpy(gest[i]), torch.from_numpy(cont[i]).t()) / 0.07, dim=1).numpy().T
        assert z["attn"].dtype == np.float32 and np.array_equal(z["attn"], want)
        assert list(z["words"]) == [f"w{i}_{j}" for j in range(10)]
        assert z["best_frame"].dtype == np.int32 and np.array_equal(z["best_frame"], np.argmax(want, axis=1))
        assert np.array_equal(z["best_score"], want.max(axis=1))
    assert drivers.cmd_attn_matrix(["--path", str(src / "clip1.pkl"), "--fname", "heat", "--res_dir", str(res), "--normalize", "1"], engine=eng) == 0
    assert eng.calls[-1] == dict(n=1, normalize=True, want_matrix=True)
    assert np.array_equal(np.load(res / "heat.attn.npz")["attn"], O.attn_matrix(gest[1], cont[1]))
    assert "attn_matrix" in drivers.COMMANDS
    with open(src / "clip2.pkl", "wb") as f:                                        # word boundaries that do not match the content rows
        pickle.dump({"gesture_emb": gest[2], "content_emb": cont[2][:4], "info": {"fname": "c2", "word_boundaries": bounds[2], "text": "t"}}, f)
    with pytest.raises(ValueError):
        drivers.cmd_attn_matrix(["--path", str(src / "clip2.pkl"), "--res_dir", str(res)], engine=eng)


def test_engine_attn_matrix_refuses_bad_arguments_before_it_needs_a_device():
    assert len(_SIGS["jg_attn_matrix"]) == 14
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    g, c = torch.zeros(20, 512), torch.zeros(6, 512)
    bad = [dict(g_offsets=[0, 20], c_offsets=[0, 3, 6]),                 # different clip counts
           dict(g_offsets=[0, 0, 20], c_offsets=[0, 3, 6]),              # a clip without frames
           dict(g_offsets=[0, 10, 20], c_offsets=[0, 6, 6]),             # a clip without words
           dict(g_offsets=[0, 10, 30], c_offsets=[0, 3, 6]),             # offsets beyond the rows
           dict(g_offsets=[0, 10, 20], c_offsets=[-1, 3, 6]),            # offsets before the rows
           dict(g_offsets=[0, 10, 20], c_offsets=[0, 3, 6], temp=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.attn_matrix(g, c, **kw)
    with pytest.raises(ValueError):
        eng.attn_matrix(torch.zeros(9000, 512), c, [0, 9000], [0, 6])    # more than 8192 frames
    with pytest.raises(ValueError):
        eng.attn_matrix(g, torch.zeros(1025, 512), [0, 20], [0, 1025])   # more than 1024 words
    with pytest.raises(ValueError):
        eng.attn_matrix(torch.zeros(20, 96), torch.zeros(6, 96), [0, 20], [0, 6])       # D % 64
    with pytest.raises(ValueError):
        eng.attn_matrix(g, torch.zeros(6, 256), [0, 20], [0, 6])         # different D
