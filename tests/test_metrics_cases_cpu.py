"""The cases of tests/metrics_fp64_cases.py checked against themselves, without a GPU, and the argument checks of the Engine's metric wrappers.

For jg_sim_rank, jg_spot and jg_asd:
  (a) the float64 reference agrees with the oracle's fp32 statements (O.compute_metrics, O.attn_matrix, O.asd_predictions) on the cases that
      are not degenerate for those (no empty candidate list, nothing zero or tiny);
  (b) a plain float32 numpy statement of the kernel's arithmetic stays inside every bound, and every margin condition holds (the generators
      assert them, for every clip and query: nothing is excluded);
  (c) each planted defect of that statement fails at least one case:
        rank:  `>` changed to `>=`; ties without the partner itself; the last tile's column guard dropped (the gallery padded with zero scores
               to a multiple of 64); the diagonal taken at column i instead of row_offset + i
        spot:  last arg-max instead of first; softmax over W - 1 words; rows not normalised; the first index of a lane's strided scan lost
        asd:   seven candidates considered; last arg-max; eps on each norm instead of on their product
So a GPU failure of tests/test_gpu_metrics_fp64.py points at the kernel, not at a reference or at a bound that float32 cannot meet.

Engine.asd / sim_rank / pool_mean / logmel refuse bad shapes, counts and host offsets with ValueError before they need a handle or a device.
"""
import numpy as np
import pytest
import torch

import jegal_oracle as O
import metrics_fp64_cases as C
from jegal_amd import metrics as M
from jegal_amd._lib import Engine


# ================================================================================================================================ rank
def scores32(e1, e2):
    """float32 dot products, one k-ascending chain per element: a score depends on its two rows alone, as in the kernel"""
    acc = np.zeros((e1.shape[0], e2.shape[0]), np.float32)
    for k in range(e1.shape[1]):
        acc += e1[:, k:k + 1] * e2[None, :, k]
    return acc


RANK_MUTANTS = {"ge": dict(gt=np.greater_equal), "ties_without_self": dict(count_self=False), "no_column_guard": dict(pad_to=64),
                "diag_at_i": dict(diag_at_i=True)}


def test_rank_exact_reference_standin_and_mutants():
    caught = {m: 0 for m in RANK_MUTANTS}
    zero_queries = 0
    for shape in C.RANK_EXACT_SHAPES:
        n_local, n_total, row_offset, D = shape
        c = C.rank_exact_case(*shape)
        s32 = scores32(c["e1"], c["e2"])
        assert np.array_equal(s32.astype(np.int64), c["s"]), shape          # (b) every fp32 partial sum is exact
        rank, ties = C.rank_counts(s32, row_offset)
        assert np.array_equal(rank, c["rank"]) and np.array_equal(ties, c["ties"]), shape
        assert int(c["ties"].min()) >= 1 and int((c["rank"] + c["ties"]).max()) <= n_total
        zero_queries += c["zero_query"] is not None
        if n_local == n_total and row_offset == 0:          # (a) the oracle ranks a square matrix by its diagonal
            assert O.compute_metrics(s32) == M.metrics_from_ranks(c["rank"], c["ties"]), shape
        for name, kw in RANK_MUTANTS.items():
            r, t = C.rank_counts(s32, row_offset, **kw)
            caught[name] += not (np.array_equal(r, c["rank"]) and np.array_equal(t, c["ties"]))
    assert zero_queries >= 3
    assert all(caught.values()), caught
    assert caught["ge"] == caught["ties_without_self"] == len(C.RANK_EXACT_SHAPES)


def test_rank_float_interval():
    c = C.rank_float_case()
    n_local, n_total, row_offset, D = C.RANK_FLOAT_SHAPE
    s32 = scores32(c["e1"], c["e2"])
    rank, ties = C.rank_counts(s32, row_offset)
    assert C.rank_interval_fails(c, rank, ties) == []
    width = c["hi"] - c["lo"] - 1 - c["copies"]
    print(f"rank float: undecided scores per query, max {int(width.max())}, mean {float(width.mean()):.3f}")
    assert int(width.max()) <= 2, "the interval decides all but a handful of scores"
    # the interval sees the defects: another diagonal, no column guard (d < 0 for about half of the queries), ties without the partner's copies
    for kw in (dict(diag_at_i=True), dict(pad_to=64), dict(gt=np.greater_equal)):
        assert C.rank_interval_fails(c, *C.rank_counts(s32, row_offset, **kw)), kw
    assert C.rank_interval_fails(c, rank, np.ones_like(ties))


# ================================================================================================================================ spot
SPOT_MUTANTS = {"last_argmax": dict(last=True), "w_minus_1_words": dict(drop_word=True), "not_normalised": dict(normalise=False),
                "lane_first_lost": dict(lane_last=True)}


def spot_fails(clip, pred, score):
    if pred != clip["pred"]:
        return [f"pred {pred} != {clip['pred']}"]
    if clip["W"] == 1:
        return [] if score == 1.0 else [f"score {score} != 1.0"]
    r = abs(score - clip["p"]) / clip["bound"]
    return [] if r <= 1 else [f"observed/bound {r:.3f}"]


def test_spot_reference_standin_and_mutants():
    caught = {m: 0 for m in SPOT_MUTANTS}
    clips = C.spot_cases()
    assert {(c["T"], c["W"], c["D"]) for c in clips} == set(C.SPOT_SHAPES)
    pos, ties = C.spot_tie_cases()
    assert pos == [20, 21, 23, 84, 85, 129]
    worst = 0.0
    for c in clips + ties:
        a = O.attn_matrix(c["g"], c["c"])[c["target"]]          # (a)
        assert int(np.argmax(a)) == c["pred"] and abs(float(a[c["pred"]]) - c["p"]) <= 1e-4 * c["p"], (c["T"], c["W"], c["D"])
        pred, score = C.spot32(c["g"], c["c"], c["target"])          # (b)
        assert spot_fails(c, pred, score) == [], (c["T"], c["W"], c["D"], c["target"], spot_fails(c, pred, score))
        if c["W"] > 1:
            worst = max(worst, abs(score - c["p"]) / c["bound"])
        for name, kw in SPOT_MUTANTS.items():          # (c)
            caught[name] += bool(spot_fails(c, *C.spot32(c["g"], c["c"], c["target"], **kw)))
    print(f"spot: float32 statement, worst observed/bound {worst:.4f}")
    assert all(caught.values()), caught
    for tg_clips in (ties[:6], ties[6:]):          # the six clips of a target: pred walks through the positions, one score
        got = [C.spot32(c["g"], c["c"], c["target"]) for c in tg_clips]
        assert [p for p, _ in got] == pos and len({s for _, s in got}) == 1
    clips, flags = C.spot_mixed_batch()
    assert [c["T"] for c in clips] == [9, 0, 70, 4, 6, 5, 8193] and [c["W"] for c in clips][3] == 0 and clips[4]["target"] == clips[4]["W"]
    assert flags == [not ("pred" in c) for c in clips]


# ================================================================================================================================= asd
ASD_MUTANTS = {"seven_candidates": dict(limit=7), "last_argmax": dict(last=True), "eps_on_each_norm": dict(eps_each=True)}


def test_asd_reference_standin_and_mutants():
    caught = {m: 0 for m in ASD_MUTANTS}
    counts, ns, ds, kinds = set(), set(), set(), set()
    for n, D, P in C.ASD_BATCHES:
        b = C.asd_batch(n, D, P)
        counts |= set(P)
        ns.add(n)
        ds.add(D)
        kinds |= set(b["kinds"])
        for i in range(n):
            q, cand = b["q"][i], b["cands"][i]
            want = b["pred"][i].tolist()
            if b["plain"][i]:          # (a)
                assert O.asd_predictions(q, cand) == want, (n, D, i)
            assert C.asd32(q, cand) == want, (n, D, i, b["kinds"][i])          # (b)
            for name, kw in ASD_MUTANTS.items():          # (c)
                caught[name] += C.asd32(q, cand, **kw) != want
            if len(cand) == 0:
                assert want == [-1, -1, -1]
            if b["kinds"][i] == "zero_query":
                assert want == [0, 0, 0]
            if b["kinds"][i] == "zero_cand_wins":
                assert want[1:] == [2, 2]
            if b["kinds"][i] == "dup13":
                assert want == [1, 1, 1]
            if b["kinds"][i] == "dup35":
                assert want == [1, 3, 3]
    assert counts == {0, 1, 2, 3, 4, 5, 6, 7, 9} and ns == {1, 4, 5, 9} and ds == {1, 64, 100, 512, 1024}
    assert kinds >= set(C.ASD_SPECIAL.values())
    assert all(caught.values()), caught


# ====================================================================================================================== Engine's checks
def test_engine_metric_wrappers_refuse_bad_arguments_before_they_need_a_device():
    eng = Engine.__new__(Engine)          # no handle, no device: every check below comes before either is touched
    q, cand = torch.zeros(4, 128), torch.zeros(9, 128)
    bad_asd = [dict(query=torch.zeros(128), cand=cand, c_offsets=[0, 9]),                       # not (rows, D)
               dict(query=q, cand=torch.zeros(9, 64), c_offsets=[0, 2, 4, 6, 9]),               # different D
               dict(query=q, cand=cand, c_offsets=[0, 2, 4, 9]),                                # n offsets: the kernel would read past them
               dict(query=q, cand=cand, c_offsets=[0, 2, 4, 6, 8, 9]),
               dict(query=q, cand=cand, c_offsets=torch.tensor([0, 2, 4, 9], dtype=torch.int32)),
               dict(query=q, cand=cand, c_offsets=[0, 4, 2, 6, 9]),                             # decreasing
               dict(query=q, cand=cand, c_offsets=[0, 2, 4, 6, 10]),                            # past the candidates
               dict(query=q, cand=cand, c_offsets=[-1, 2, 4, 6, 9]),
               dict(query=q, cand=cand, c_offsets=[[0, 2, 4, 6, 9]]),
               dict(query=q, cand=cand, c_offsets=[0.0, 2.0, 4.0, 6.0, 9.0])]
    for kw in bad_asd:
        with pytest.raises(ValueError):
            eng.asd(**kw)
    e1, e2 = torch.zeros(5, 128), torch.zeros(20, 128)
    bad_rank = [dict(e1=torch.zeros(128), e2=e2), dict(e1=e1, e2=torch.zeros(20, 64)), dict(e1=torch.zeros(5, 96), e2=torch.zeros(20, 96)),
                dict(e1=torch.zeros(5, 0), e2=torch.zeros(20, 0)), dict(e1=e1, e2=e2, row_offset=-1), dict(e1=e1, e2=e2, row_offset=16),
                dict(e1=e2, e2=e1)]
    for kw in bad_rank:
        with pytest.raises(ValueError):
            eng.sim_rank(**kw)
    x = torch.zeros(9, 100)
    bad_pool = [dict(x=torch.zeros(100), offsets=[0, 1]), dict(x=x, offsets=[]), dict(x=x, offsets=[0, 5, 3, 9]), dict(x=x, offsets=[0, 10]),
                dict(x=x, offsets=[-2, 9]), dict(x=x, offsets=torch.zeros(2, 2, dtype=torch.int32)), dict(x=x, offsets=[0.5, 9.0])]
    for kw in bad_pool:
        with pytest.raises(ValueError):
            eng.pool_mean(**kw)
    mb = torch.zeros(80, 257)
    bad_mel = [dict(wav=torch.zeros(1600), mel_basis=mb), dict(wav=torch.zeros(0, 1600), mel_basis=mb), dict(wav=torch.zeros(2, 1600), mel_basis=mb.T),
               dict(wav=torch.zeros(2, 1600), mel_basis=torch.zeros(80, 256))]
    for kw in bad_mel:
        with pytest.raises(ValueError):
            eng.logmel(**kw)
    for n in (0, 159, 160, 200, 256):
        with pytest.raises(ValueError, match="reflect padding needs more than 256 samples"):
            eng.logmel(torch.zeros(2, n), mb)
    # what is in order gets past the checks: the next thing the wrappers touch is the handle this stand-in lacks
    for call in (lambda: eng.asd(q, cand, [0, 2, 4, 6, 9]), lambda: eng.asd(q, cand, torch.tensor([0, 2, 4, 6, 9])),
                 lambda: eng.sim_rank(e1, e2, 15), lambda: eng.pool_mean(x, np.asarray([0, 0, 9])), lambda: eng.logmel(torch.zeros(2, 257), mb)):
        with pytest.raises(AttributeError):
            call()
