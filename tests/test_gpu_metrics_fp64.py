"""jg_sim_rank, jg_spot and jg_asd against float64 at their edges (run with -m gpu).

Every case is ONE production launch through the public C ABI (e._ck(e.lib.jg_...): the Engine's wrappers would refuse some of the arguments
tried here).  Cases, references, bounds and margin conditions come from tests/metrics_fp64_cases.py, where tests/test_metrics_cases_cpu.py
checks them without a GPU.  Outputs are pre-filled with a sentinel bit pattern and carry guard rows; inputs are framed with NaN rows.  rank, ties
and every arg-max must be EXACT; the spotting score is bounded: observed / bound is printed per clip and asserted <= 1.

Measured on an MI355X: sim_rank equal to the int64 counts at every exact shape, and inside the interval for all 70 queries of the float shape (one
rank above the certain count, at most one undecided score per query); spot pred exact everywhere, the six copies of a winner bit-equal, worst
observed / bound of the score 0.0011 (T 67, W 65, D 100); asd exact for every query.  ("Float64 checks of the first-generation entries".)
"""
import ctypes

import numpy as np
import pytest
import torch

import metrics_fp64_cases as C
import test_gpu_kernels_fp64 as K64
from test_gpu_kernels_fp64 import DEV, SENT32, engine, guarded, guards_intact, note, rejects

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in K64._ENGINES.values():
        e.close()
    K64._ENGINES.clear()


def framed(x):
    """float32 rows on the device inside a buffer with 64 NaN elements in front and behind (the start stays 16-byte aligned)"""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    flat = torch.full((x.numel() + 128,), NAN, dtype=torch.float32)
    flat[64:64 + x.numel()] = x.reshape(-1)
    return flat.to(DEV)[64:64 + x.numel()].view(x.shape)


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.int32), device=DEV)


def iguard(rows, cols=1):
    """int32 output [rows + guard][cols] filled with the sentinel"""
    return guarded(rows, cols, torch.float32).view(torch.int32)


def iguards_intact(buf, rows, cols=1):
    return guards_intact(buf.view(torch.float32), rows, cols)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def refused(e, rc):
    """the return code of a C entry is JG_ERR_ARG (through the Engine's own check of return codes)"""
    return rejects(e._ck, rc)


def report(family, fails):
    print(f"worst observed/bound, {family}: {K64.RATIOS.get(family, 0.0):.4f}")
    assert not fails, "\n".join(fails)


# ============================================================================================================================== sim_rank
def sim_rank(e, c, n_local, n_total, row_offset, D):
    e1, e2 = framed(c["e1"]), framed(c["e2"])
    rank, ties = iguard(n_local), iguard(n_local)
    e._bind_stream()
    e._ck(e.lib.jg_sim_rank(e.h, P(e1), P(e2), n_local, n_total, row_offset, D, P(rank), P(ties)))
    torch.cuda.synchronize()
    assert iguards_intact(rank, n_local) and iguards_intact(ties, n_local), (n_local, n_total, row_offset, D)
    return rank[:n_local, 0].cpu().numpy().astype(np.int64), ties[:n_local, 0].cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("shape", C.RANK_EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sim_rank_exact(shape):
    e = engine()
    c = C.rank_exact_case(*shape)
    rank, ties = sim_rank(e, c, *shape)
    bad = [(i, int(rank[i]), int(c["rank"][i]), int(ties[i]), int(c["ties"][i])) for i in range(shape[0]) if rank[i] != c["rank"][i] or ties[i] != c["ties"][i]]
    assert not bad, f"(query, rank, want, ties, want): {bad[:8]}"
    if c["zero_query"] is not None:
        assert rank[c["zero_query"]] == 0 and ties[c["zero_query"]] == shape[1]


def test_sim_rank_float_interval():
    e = engine()
    c = C.rank_float_case()
    rank, ties = sim_rank(e, c, *C.RANK_FLOAT_SHAPE)
    fails = C.rank_interval_fails(c, rank, ties)
    undecided = c["hi"] - c["lo"] - 1 - c["copies"]
    print(f"sim_rank float: {int((rank != c['lo']).sum())} of {len(rank)} ranks above the certain count, at most {int(undecided.max())} undecided scores per query")
    assert not fails, "\n".join(fails)


def test_sim_rank_rejections_and_empty():
    e = engine()
    c = C.rank_exact_case(5, 200, 195, 1024)
    e1, e2 = framed(c["e1"]), framed(c["e2"])
    rank, ties = iguard(5), iguard(5)
    e._bind_stream()
    for n_local, n_total, row_offset, D in ((5, 200, 195, 1000), (5, 200, 195, 32), (5, 200, -1, 1024), (5, 200, 196, 1024), (5, 4, 0, 1024)):
        assert refused(e, e.lib.jg_sim_rank(e.h, P(e1), P(e2), n_local, n_total, row_offset, D, P(rank), P(ties))), (n_local, n_total, row_offset, D)
    assert e.lib.jg_sim_rank(e.h, P(e1), P(e2), 0, 200, 0, 1024, P(rank), P(ties)) == 0          # no query: nothing to do
    torch.cuda.synchronize()
    assert iguards_intact(rank, 0) and iguards_intact(ties, 0), "a refused or empty call writes nothing"


# ================================================================================================================================== spot
def spot(e, batch, n=None):
    """One jg_spot launch over a batch (metrics_fp64_cases.spot_batch) -> (pred int64, score float32 as numpy)"""
    n = len(batch["target"]) if n is None else n
    g, c = framed(batch["g"]), framed(batch["c"])
    goff, coff, target = i32(batch["goff"]), i32(batch["coff"]), i32(batch["target"])
    pred, score = iguard(n), guarded(n, 1, torch.float32)
    e._bind_stream()
    e._ck(e.lib.jg_spot(e.h, P(g), P(c), P(goff), P(coff), P(target), n, batch["D"], C.TEMP, P(pred), P(score)))
    torch.cuda.synchronize()
    assert iguards_intact(pred, n) and guards_intact(score, n, 1)
    return pred[:n, 0].cpu().numpy().astype(np.int64), score[:n, 0].cpu().numpy()


def spot_check(clip, pred, score, what):
    if pred != clip["pred"]:
        return [f"spot {what}: pred {pred}, float64 says {clip['pred']}"]
    if clip["W"] == 1:
        return [] if score == 1.0 else [f"spot {what}: score {score!r} with one word, must be 1.0"]
    r = abs(float(score) - clip["p"]) / clip["bound"] if np.isfinite(score) else float("inf")
    note("spot", r)
    print(f"spot               {what:60s} observed/bound {r:.4f}")
    return [] if r <= 1 else [f"spot {what}: observed/bound {r:.4f}"]


@pytest.mark.parametrize("shape", C.SPOT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spot_shapes(shape):
    """every target of the shape in one launch (the clips of a launch share D)"""
    e = engine()
    T, W, D = shape
    clips = [C.spot_clip(T, W, D, tg, zero_rows=(T, W) == (130, 5)) for tg in C.spot_targets(W)]
    pred, score = spot(e, C.spot_batch(clips))
    fails = []
    for k, c in enumerate(clips):
        fails += spot_check(c, int(pred[k]), score[k], f"T {T} W {W} D {D} target {c['target']}")
    report("spot", fails)


def test_spot_ties_first_frame_and_equal_bits():
    e = engine()
    pos, clips = C.spot_tie_cases()
    pred, score = spot(e, C.spot_batch(clips))
    fails = []
    for k, c in enumerate(clips):
        fails += spot_check(c, int(pred[k]), score[k], f"copies at {pos[k % 6:]} target {c['target']}")
    assert pred.tolist() == pos + pos, "the first of the copies"
    for half in (score[:6], score[6:]):          # a copy computes the same bits in whichever wave, lane and pass of the lane scan it lies
        assert len(set(half.view(np.int32).tolist())) == 1, half.tolist()
    assert score[0] != score[6], "the second target is another column"
    report("spot", fails)


def test_spot_mixed_batch_flags_and_neighbours():
    e = engine()
    clips, flags = C.spot_mixed_batch()
    pred, score = spot(e, C.spot_batch(clips))
    fails = []
    for k, (c, bad) in enumerate(zip(clips, flags)):
        if bad:
            assert pred[k] == -1 and np.isnan(score[k]), (k, pred[k], score[k])
            continue
        fails += spot_check(c, int(pred[k]), score[k], f"mixed batch, clip {k}")
        p1, s1 = spot(e, C.spot_batch([c]))          # the same clip alone
        assert p1[0] == pred[k] and s1.view(np.int32)[0] == score.view(np.int32)[k], (k, p1, s1, pred[k], score[k])
    b = C.spot_batch(clips[:1])
    pred0, score0 = spot(e, b, n=0)          # n = 0: returns 0, writes nothing (the guards of spot() cover all of both outputs)
    assert pred0.size == 0 and score0.size == 0
    report("spot", fails)


# =================================================================================================================================== asd
@pytest.mark.parametrize("n,D,counts", C.ASD_BATCHES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_asd(n, D, counts):
    e = engine()
    b = C.asd_batch(n, D, counts)
    q = framed(b["q"])
    cand = framed(b["cand"] if len(b["cand"]) else np.zeros((1, D), np.float32))
    coff = i32(b["coff"])
    pred = iguard(n, 3)
    e._bind_stream()
    e._ck(e.lib.jg_asd(e.h, P(q), P(cand), P(coff), n, D, C.TEMP, P(pred)))
    torch.cuda.synchronize()
    assert iguards_intact(pred, n, 3)
    got = pred[:n].cpu().numpy()
    bad = [(i, b["kinds"][i], counts[i], got[i].tolist(), b["pred"][i].tolist()) for i in range(n) if got[i].tolist() != b["pred"][i].tolist()]
    assert not bad, f"(query, kind, candidates, got, float64): {bad}"
    for i, cnt in enumerate(counts):
        if cnt >= 7:
            assert 6 not in got[i], "only the first six candidates count"
    assert e.lib.jg_asd(e.h, P(q), P(cand), P(coff), 0, D, C.TEMP, P(pred[n:])) == 0          # n = 0
    torch.cuda.synchronize()
    assert iguards_intact(pred, n, 3)
    assert int(pred.view(torch.int32)[n, 0]) == SENT32
