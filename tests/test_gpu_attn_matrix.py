"""jg_attn_matrix through the C ABI (run with -m gpu): the gesture-word attention matrices A = softmax((G C^T) / 0.07, dim=1)^T of a ragged
batch, and every word's first arg-max frame, against a float64 evaluation of the same formula.

Error rule: err(X) = distance of X from the float64 matrices pooled over the clips of one input, as (max-abs, max relative error over
entries whose true value is >= 1e-3); the kernel is held to err(kernel) <= 4 x err(fp32 reference) in both parts, the fp32 reference
being O.attn_matrix (normalize=1), the same torch-fp32 formula without the normalisation (normalize=0), or the golden attn0.  The
reference's blocked fp32 sums and the MFMA's k-ordered fmaf chains differ only in summation order.  A CPU emulation of ONE 512-term
chain per element gave 1.1-2.1 x the reference's max-abs error on the planted clips and 0.9-3.9 x on the inputs of
test_path_boundaries; the kernel cuts the chain every 128 terms (0.3-1.0 x in the same emulation).  4 x leaves
room for the device expf.
Arg-max rule: a word is decidable if, in float64, its best frame beats the runner-up by more than 1e-3 relative; decidable words must
match the float64 arg-max exactly, the others must return a frame within 1e-3 relative of the best; every input has >= 95 % decidable
words (asserted)."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import jegal_oracle as O
from jegal_amd import synth

pytestmark = pytest.mark.gpu
TEMP = 0.07
REG_W = 128          # AM_REG_W of jegal_amd/csrc/spotting.hip: widest clip of the in-register form
FRAME_BLOCK = 128    # AM_FB: frames per workgroup


@pytest.fixture(scope="module")
def eng():
    from jegal_amd._lib import Engine
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ references
def ref64(g, c, normalize):
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    if normalize:
        g = g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-12)
        c = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)
    x = g @ c.T / TEMP
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).T


def ref32(g, c, normalize):
    if normalize:
        return O.attn_matrix(g, c, TEMP)
    gt, ct = torch.from_numpy(np.asarray(g, np.float32)), torch.from_numpy(np.asarray(c, np.float32))
    return torch.softmax(torch.mm(gt, ct.t()) / TEMP, dim=1).numpy().T


def err(mats, mats64):
    ma = mr = 0.0
    for a, r in zip(mats, mats64):
        d = np.abs(np.asarray(a, np.float64) - r)
        ma = max(ma, float(d.max()))
        big = r >= 1e-3
        if big.any():
            mr = max(mr, float((d[big] / r[big]).max()))
    return ma, mr


def check_errors(name, mats, mats32, mats64):
    k, r = err(mats, mats64), err(mats32, mats64)
    print(f"{name}: kernel max-abs {k[0]:.3e} rel {k[1]:.3e} | fp32 reference max-abs {r[0]:.3e} rel {r[1]:.3e} | "
          f"ratios {k[0] / max(r[0], 1e-30):.2f} {k[1] / max(r[1], 1e-30):.2f}")
    assert k[0] <= 4 * r[0] and k[1] <= 4 * r[1], (name, k, r)


def check_argmax(name, mats64, frames, min_share=0.95):
    n = dec = 0
    for a, f in zip(mats64, frames):
        for w in range(a.shape[0]):
            row = a[w]
            best = int(np.argmax(row))
            second = np.partition(row, -2)[-2] if row.size > 1 else -np.inf
            decidable = row[best] - second > 1e-3 * row[best]
            n += 1
            dec += bool(decidable)
            assert 0 <= f[w] < row.size, (name, w, f[w])
            if decidable:
                assert f[w] == best, (name, w, int(f[w]), best)
            else:
                assert row[f[w]] >= row[best] * (1 - 1e-3), (name, w, int(f[w]), best)
    print(f"{name}: {dec}/{n} decidable words")
    assert dec >= min_share * n, (name, dec, n)


# ------------------------------------------------------------------------------------------------ the C entry
NAN_BITS = 0x7FC0BEEF      # a quiet NaN with a payload, as int32
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def call(eng, gs, cs, normalize=1, want_a=True, want_best=True, gap=0, max_frames=None, expect=0):
    """One jg_attn_matrix call on the clips (gs[i] (T_i,D), cs[i] (W_i,D)).  A is pre-filled with a NaN pattern and laid out with
    `gap` unused elements behind every clip (and a guard of 64 at the end).  -> dict(mats, frames, scores, A (int32 view), spans)"""
    g = torch.from_numpy(np.ascontiguousarray(np.concatenate(gs), np.float32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(np.concatenate(cs), np.float32)).cuda()
    T, W = np.array([x.shape[0] for x in gs]), np.array([x.shape[0] for x in cs])
    goff, coff = np.concatenate([[0], np.cumsum(T)]), np.concatenate([[0], np.cumsum(W)])
    aoff = np.concatenate([[0], np.cumsum(T * W + gap)])
    A = torch.full((int(aoff[-1]) + 64,), NAN_BITS, dtype=torch.int32, device="cuda") if want_a else None
    bf = torch.full((int(coff[-1]),), -7, dtype=torch.int32, device="cuda") if want_best else None
    bs = torch.full((int(coff[-1]),), -7.0, dtype=torch.float32, device="cuda") if want_best else None
    go, co = (torch.as_tensor(v.astype(np.int32), device="cuda") for v in (goff, coff))
    ao = torch.as_tensor(aoff[:-1].astype(np.int64), device="cuda")
    eng._bind_stream()
    rc = eng.lib.jg_attn_matrix(eng.h, P(g), P(c), P(go), P(co), len(gs), g.shape[1], int(max_frames or T.max()), TEMP, normalize,
                                P(A), P(ao) if want_a else None, P(bf), P(bs))
    assert rc == expect, (rc, eng.lib.jg_last_error(eng.h))
    torch.cuda.synchronize()
    out = {"spans": [(int(aoff[i]), int(aoff[i] + T[i] * W[i])) for i in range(len(gs))], "coff": coff}
    if want_a:
        raw = A.cpu().numpy()
        out["A"] = raw
        out["mats"] = [raw[s:e].view(np.float32).reshape(W[i], T[i]) for i, (s, e) in enumerate(out["spans"])]
    if want_best:
        f, s = bf.cpu().numpy(), bs.cpu().numpy()
        out["frames"] = [f[coff[i]:coff[i + 1]] for i in range(len(gs))]
        out["scores"] = [s[coff[i]:coff[i + 1]] for i in range(len(gs))]
    return out


def check_input(eng, name, gs, cs, normalize):
    r = call(eng, gs, cs, normalize)
    m64 = [ref64(g, c, normalize) for g, c in zip(gs, cs)]
    check_errors(name, r["mats"], [ref32(g, c, normalize) for g, c in zip(gs, cs)], m64)
    check_argmax(name, m64, r["frames"])
    for a, f, s in zip(r["mats"], r["frames"], r["scores"]):        # best_score[w] is A[w][best_frame[w]] bit for bit
        assert np.array_equal(a[np.arange(a.shape[0]), f].view(np.int32), s.view(np.int32)), name
    return r


def scaled_rows(rng, n, d=512):
    return (rng.standard_normal((n, d)) * rng.uniform(0.1, 30, (n, 1))).astype(np.float32)


def unit_scaled_rows(rng, n, d=512):
    """rows of norm <= 1 (uniform in 0.3 .. 1): the un-normalised form is meant for stored, roughly normalised embeddings"""
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(0.3, 1.0, (n, 1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. reference golden
def test_reference_golden_and_spot(eng, golden_dir):
    gest, cont, bounds, targets = synth.planted_spotting(9006, 20, n_frames=60, n_words=10, noise=2.0)
    attn0 = np.load(os.path.join(golden_dir, "metrics.npz"))["attn0"]
    r0 = call(eng, gest[:1], cont[:1])
    m64 = [ref64(gest[0], cont[0], 1)]
    check_errors("golden clip 0", r0["mats"], [attn0], m64)
    check_argmax("golden clip 0", m64, r0["frames"], min_share=0.0)      # ten words: the share is asserted on the 20 clips below
    r = check_input(eng, "planted_spotting(9006) x 20", gest, cont, 1)
    assert np.array_equal(r["mats"][0].view(np.int32), r0["mats"][0].view(np.int32))
    goff = np.arange(21) * 60
    coff = np.arange(21) * 10
    pred, score = eng.spot(torch.from_numpy(np.concatenate(gest)), torch.from_numpy(np.concatenate(cont)), goff, coff, targets)
    pred, score = pred.cpu().numpy(), score.cpu().numpy()
    for i, t in enumerate(targets):
        assert r["frames"][i][t] == pred[i], (i, t)
        assert float(r["scores"][i][t]) == pytest.approx(float(score[i]), rel=1e-4)


# ------------------------------------------------------------------------------------------------ 2. tile edges, ragged, one call
EDGE_T = [1, 31, 32, 33, 64, 65, 150]
EDGE_W = [1, 5, 32, 33, 31, 64, 30]


@pytest.mark.parametrize("normalize", [1, 0])
def test_tile_edges_ragged(eng, normalize):
    rng = np.random.default_rng(3)
    make = scaled_rows if normalize else unit_scaled_rows
    gs = [make(rng, t) for t in EDGE_T]
    cs = [make(rng, w) for w in EDGE_W]
    r = check_input(eng, f"tile edges normalize={normalize}", gs, cs, normalize)
    assert np.all(r["mats"][0] == np.float32(1.0))                      # W = 1: the softmax over one word
    assert np.all(r["scores"][0] == np.float32(1.0)) and r["frames"][0][0] == 0


# ------------------------------------------------------------------------------------------------ 3. every path boundary
@pytest.mark.parametrize("T,W", [(40, REG_W - 1), (40, REG_W), (40, REG_W + 1),                       # in-register | wide form
                                 (FRAME_BLOCK - 1, 7), (FRAME_BLOCK, 7), (FRAME_BLOCK + 1, 7),        # one | two frame blocks
                                 (FRAME_BLOCK + 1, REG_W + 2),                                        # wide form over two blocks
                                 (8192, 40), (70, 1024)])                                             # the limits
def test_path_boundaries(eng, T, W):
    rng = np.random.default_rng(1000 * T + W)
    check_input(eng, f"T={T} W={W}", [scaled_rows(rng, T)], [scaled_rows(rng, W)], 1)


# ------------------------------------------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("W", [9, REG_W + 5])
@pytest.mark.parametrize("src,dst", [(3, 17), (20, 45), (100, 140)])     # within a 32-frame tile, across tiles, across frame blocks
def test_duplicate_frames_tie_to_the_first(eng, W, src, dst):
    rng = np.random.default_rng(7 + W)
    g, c = scaled_rows(rng, 150), scaled_rows(rng, W)
    g[src] = 3 * c[0]                                # word 0 has its maximum on the duplicated frame
    g[dst] = g[src]
    r = call(eng, [g], [c])
    a, f = r["mats"][0], r["frames"][0]
    assert np.array_equal(a[:, src].view(np.int32), a[:, dst].view(np.int32))
    at_dup = [w for w in range(W) if a[w].max() == a[w, src]]
    assert 0 in at_dup
    for w in range(W):
        assert f[w] == int(np.argmax(a[w])), w       # np.argmax: the first index on ties
    assert all(f[w] == src for w in at_dup)


# ------------------------------------------------------------------------------------------------ 5. bit-identity
@pytest.mark.parametrize("T,W", [(70, 12), (FRAME_BLOCK + 30, REG_W + 9)])
def test_bit_identity_across_neighbours_and_modes(eng, T, W):
    rng = np.random.default_rng(11)
    x = (scaled_rows(rng, T), scaled_rows(rng, W))
    n1 = (scaled_rows(rng, 33), scaled_rows(rng, 140))
    n2 = (scaled_rows(rng, 200), scaled_rows(rng, 3))
    bits = lambda r, i: (r["mats"][i].view(np.int32).copy(), r["frames"][i].copy(), r["scores"][i].view(np.int32).copy())
    alone = call(eng, [x[0]], [x[1]])
    a0, f0, s0 = bits(alone, 0)
    assert np.array_equal(a0[np.arange(W), f0], s0)
    for order, pos in (((x, n1, n2), 0), ((n1, n2, x), 2), ((n1, x, n2), 1), ((n2, x, n1), 1)):
        r = call(eng, [o[0] for o in order], [o[1] for o in order])
        a, f, s = bits(r, pos)
        assert np.array_equal(a, a0) and np.array_equal(f, f0) and np.array_equal(s, s0), pos
    r = call(eng, [n1[0], x[0]], [n1[1], x[1]], want_a=False)                      # A == NULL: best_* only
    assert np.array_equal(r["frames"][1], f0) and np.array_equal(r["scores"][1].view(np.int32), s0)
    r = call(eng, [n1[0], x[0]], [n1[1], x[1]], want_best=False)                   # the matrix only
    assert np.array_equal(r["mats"][1].view(np.int32), a0)
    eng.set_option("ws_poison", 1)
    try:
        r = call(eng, [n2[0], x[0]], [n2[1], x[1]])
    finally:
        eng.set_option("ws_poison", 0)
    a, f, s = bits(r, 1)
    assert np.array_equal(a, a0) and np.array_equal(f, f0) and np.array_equal(s, s0)


# ------------------------------------------------------------------------------------------------ 6. nothing else is written
def test_nothing_outside_the_clips_is_written(eng):
    rng = np.random.default_rng(5)
    Ts, Ws = [33, 33, 33, 1], [5, 33, REG_W + 1, 2]
    gs, cs = [scaled_rows(rng, t) for t in Ts], [scaled_rows(rng, w) for w in Ws]
    r = call(eng, gs, cs, gap=3)
    inside = np.zeros(r["A"].size, bool)
    for s, e in r["spans"]:                          # (T = 33 and gaps of 3: rows start at odd element offsets)
        inside[s:e] = True
    assert np.all(r["A"][~inside] == NAN_BITS)
    assert (~inside).sum() == 3 * len(Ts) + 64
    assert not np.isnan(r["A"][inside].view(np.float32)).any()
    check_errors("gapped layout", r["mats"], [ref32(g, c, 1) for g, c in zip(gs, cs)], [ref64(g, c, 1) for g, c in zip(gs, cs)])


# ------------------------------------------------------------------------------------------------ 7. limits
def test_limits_and_argument_errors(eng):
    rng = np.random.default_rng(9)
    gs, cs = [scaled_rows(rng, t) for t in (40, 50, 17)], [scaled_rows(rng, w) for w in (6, 4, 9)]
    r = call(eng, gs, cs, max_frames=40)             # the middle clip is longer than max_frames
    assert np.all(r["frames"][1] == -1) and np.isnan(r["scores"][1]).all()
    s, e = r["spans"][1]
    assert np.all(r["A"][s:e] == NAN_BITS)
    ok = call(eng, [gs[0], gs[2]], [cs[0], cs[2]])
    for i, j in ((0, 0), (2, 1)):
        assert np.array_equal(r["mats"][i].view(np.int32), ok["mats"][j].view(np.int32))
        assert np.array_equal(r["frames"][i], ok["frames"][j]) and np.array_equal(r["scores"][i].view(np.int32), ok["scores"][j].view(np.int32))
    check_errors("neighbours of a rejected clip", [r["mats"][0], r["mats"][2]], [ref32(gs[i], cs[i], 1) for i in (0, 2)],
                 [ref64(gs[i], cs[i], 1) for i in (0, 2)])
    # Python refuses what the host can see
    for Tn, Wn in ((9000, 4), (10, 1025)):
        with pytest.raises(ValueError):
            eng.attn_matrix(torch.zeros(Tn, 512), torch.zeros(Wn, 512), [0, Tn], [0, Wn])
    # content rows in front of the first clip: best_* stay indexed like the content rows
    cat_g, cat_c = torch.from_numpy(np.concatenate([gs[0], gs[2]])), torch.from_numpy(np.concatenate([cs[1], cs[0], cs[2]]))
    _, _, bf2, bs2 = eng.attn_matrix(cat_g, cat_c, [0, 40, 57], [4, 10, 19])
    bf2, bs2 = bf2.cpu().numpy(), bs2.cpu().numpy()
    assert np.all(bf2[:4] == -1) and np.isnan(bs2[:4]).all()
    assert np.array_equal(bf2[4:], np.concatenate(ok["frames"])) and np.array_equal(bs2[4:].view(np.int32), np.concatenate(ok["scores"]).view(np.int32))
    # every JG_ERR_ARG case returns it and launches nothing
    g, c = torch.zeros(8, 512, device="cuda"), torch.zeros(2, 512, device="cuda")
    go, co = (torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([0, 8], [0, 2]))
    ao = torch.zeros(1, dtype=torch.int64, device="cuda")
    A = torch.full((16,), NAN_BITS, dtype=torch.int32, device="cuda")
    bf, bs = torch.full((2,), -7, dtype=torch.int32, device="cuda"), torch.full((2,), -7.0, device="cuda")
    good = dict(g=g, c=c, go=go, co=co, n=1, D=512, mf=8, temp=TEMP, A=A, ao=ao, bf=bf, bs=bs)
    odd = torch.zeros(8 * 512 + 1, device="cuda")[1:]                   # 4 bytes off a 16-byte boundary
    bad = [dict(g=None), dict(c=None), dict(go=None), dict(co=None), dict(ao=None), dict(A=None, bf=None, bs=None),
           dict(mf=0), dict(mf=8193), dict(D=96), dict(D=0), dict(temp=0.0), dict(temp=-1.0), dict(g=odd), dict(c=odd)]
    eng._bind_stream()
    eng.profile(True)
    eng.profile_reset()
    try:
        for b in bad:
            a = dict(good, **b)
            rc = eng.lib.jg_attn_matrix(eng.h, P(a["g"]), P(a["c"]), P(a["go"]), P(a["co"]), a["n"], a["D"], a["mf"], a["temp"], 1,
                                        P(a["A"]), P(a["ao"]), P(a["bf"]), P(a["bs"]))
            assert rc == -1, (b, rc)
        assert all(n == 0 for _, n in eng.profile_get().values())
    finally:
        eng.profile(False)
    torch.cuda.synchronize()
    assert np.all(A.cpu().numpy() == NAN_BITS) and np.all(bf.cpu().numpy() == -7) and np.all(bs.cpu().numpy() == -7.0)


# ------------------------------------------------------------------------------------------------ 8. driver
def test_driver_writes_the_matrices(eng, tmp_path):
    import pandas as pd
    from jegal_amd import drivers, metrics as M
    gest, cont, bounds, _ = synth.planted_spotting(77, 3, n_frames=41, n_words=6, noise=1.5)
    src, res = tmp_path / "pkl", tmp_path / "res"
    src.mkdir()
    for i in range(3):
        wb = [[f"word{i}_{j}", b[1], b[2]] for j, b in enumerate(bounds[i])]
        info = pd.Series({"filename": f"vid/{i:05d}", "word_boundaries": str(wb)}) if i != 1 else {"fname": "clip1", "word_boundaries": wb, "text": "x"}
        with open(src / f"clip{i}.pkl", "wb") as f:
            pickle.dump({"gesture_emb": gest[i], "content_emb": cont[i], "info": info}, f)
    assert drivers.cmd_attn_matrix(["--path", str(src), "--res_dir", str(res)], engine=eng) == 0
    want = M.attention_matrices(gest, cont, normalize=False, engine=eng)
    for i in range(3):
        z = np.load(res / f"clip{i}.attn.npz")
        assert z["attn"].dtype == np.float32 and z["attn"].shape == (6, 41)
        assert np.array_equal(z["attn"], want[i])
        assert list(z["words"]) == [f"word{i}_{j}" for j in range(6)]
        assert np.array_equal(z["best_frame"], np.argmax(z["attn"], axis=1))
        assert np.array_equal(z["best_score"], z["attn"].max(axis=1))
    check_errors("driver", want, [ref32(g, c, 0) for g, c in zip(gest, cont)], [ref64(g, c, 0) for g, c in zip(gest, cont)])
    # a single file, with plot_heatmap's --fname, through the command table
    assert drivers.main(["attn_matrix", "--path", str(src / "clip1.pkl"), "--fname", "heat", "--res_dir", str(res), "--normalize", "1"]) == 0
    z = np.load(res / "heat.attn.npz")
    assert np.array_equal(z["attn"], M.attention_matrices(gest[1:2], cont[1:2], normalize=True, engine=eng)[0])
