"""The host side of the top-k retrieval feature without a GPU: metrics.retrieve and the retrieve driver reach the device only through
engine.l2norm / pool_mean / sim_topk / sim_rank, so a stand-in engine that computes them with numpy drives them here; plus the argument
checks Engine.sim_topk makes before it needs a device, and the two-rank sharded path of metrics.retrieve under gloo."""
import pickle
import textwrap

import numpy as np
import pytest
import torch

from jegal_amd import drivers, metrics as M, synth
from jegal_amd._lib import _SIGS, EXPORTS, Engine
from test_host_cpu import ROOT, _run_two_ranks


class NumpyEngine:
    """l2norm / pool_mean / sim_topk / sim_rank with the Engine's contracts, computed on the host"""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def l2norm(self, x):
        x = torch.as_tensor(x, dtype=torch.float32)
        return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)

    def pool_mean(self, x, offsets):
        return torch.stack([x[offsets[i]:offsets[i + 1]].mean(0) for i in range(len(offsets) - 1)])

    def sim_topk(self, queries, gallery, k, gallery_offset=0, merge_into=None):
        self.calls.append(dict(n=queries.shape[0], m=gallery.shape[0], k=k))
        assert merge_into is None
        return topk_reference(queries.numpy(), gallery.numpy(), k, gallery_offset)

    def sim_rank(self, e1, e2, row_offset=0):
        s = scores(e1.numpy(), e2.numpy())
        d = s[np.arange(s.shape[0]), row_offset + np.arange(s.shape[0])][:, None]
        return torch.from_numpy((s > d).sum(1).astype(np.int32)), torch.from_numpy((s == d).sum(1).astype(np.int32))


def scores(q, g):
    """float64 dot products rounded to fp32: what any exact-enough fp32 kernel returns, whatever its blocking"""
    return (np.asarray(q, np.float64) @ np.asarray(g, np.float64).T).astype(np.float32)


def topk_reference(q, g, k, offset=0):
    s = scores(q, g)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    idx = np.full((q.shape[0], k), -1, np.int32)
    score = np.full((q.shape[0], k), -np.inf, np.float32)
    idx[:, :order.shape[1]] = order + offset
    score[:, :order.shape[1]] = np.take_along_axis(s, order, axis=1)
    return torch.from_numpy(idx), torch.from_numpy(score)


@pytest.fixture(scope="module")
def planted():
    return synth.planted_retrieval(9107, 37)


def test_retrieve_lists_and_tensors(planted):
    g, c = planted
    eng = NumpyEngine()
    idx, score = M.retrieve(c * 2.5, g * 0.3, k=5, engine=eng)                      # un-normalised means in
    assert eng.calls == [dict(n=37, m=37, k=5)]                                     # one sim_topk call per direction
    assert idx.shape == (37, 5) and idx.dtype == np.int32 and score.shape == (37, 5) and score.dtype == np.float32
    want = np.argsort(-scores(c, g), axis=1, kind="stable")[:, :5]
    assert np.array_equal(idx, want)
    assert np.allclose(score, np.take_along_axis(c @ g.T, want, axis=1), atol=1e-6)
    idx2, score2 = M.retrieve([row for row in c], torch.from_numpy(g), k=5, engine=eng)      # a list of rows, a tensor
    assert np.array_equal(idx2, want) and eng.calls[-1] == dict(n=37, m=37, k=5)
    few_i, few_s = M.retrieve(c[:4], g[:3], k=5, engine=eng)                        # fewer gallery rows than k: -1 / -inf behind them
    assert np.all(few_i[:, 3:] == -1) and np.all(np.isneginf(few_s[:, 3:])) and np.all(few_i[:, :3] >= 0)


def write_pkls(path, g, c, frames=6):
    """one feature .pkl per clip: frame-level embeddings whose temporal means are multiples of the planted rows"""
    rng = np.random.default_rng(3)
    names = []
    for i in range(g.shape[0]):
        wobble = rng.standard_normal((frames, 1)).astype(np.float32) * 0.1
        feat = {"gesture_emb": g[i] * (1 + wobble), "content_emb": c[i] * (2 + wobble[:4]), "info": {"fname": f"c{i}"}}
        names.append(f"vid{i:03d}__t")
        with open(path / (names[-1] + ".pkl"), "wb") as f:
            pickle.dump(feat, f)
    return names


def test_retrieve_driver_writes_npz(planted, tmp_path, capsys):
    g, c = planted
    src, res = tmp_path / "pkl", tmp_path / "res"
    src.mkdir()
    names = write_pkls(src, g, c)
    eng = NumpyEngine()
    assert "retrieve" in drivers.COMMANDS
    assert drivers.cmd_retrieve(["--path", str(src), "--topk", "5", "--res_dir", str(res)], engine=eng) == 0
    assert sorted(p.name for p in res.iterdir()) == ["retrieve_c2g.npz", "retrieve_g2c.npz"]
    assert eng.calls == [dict(n=37, m=37, k=5)] * 2
    assert len([l for l in capsys.readouterr().out.splitlines() if "retrieval:" in l]) == 2          # one line per direction
    for d in ("c2g", "g2c"):
        z = np.load(res / f"retrieve_{d}.npz")
        assert sorted(z.files) == ["idx", "names", "rank", "score"]
        assert list(z["names"]) == names
        assert z["idx"].dtype == np.int32 and z["idx"].shape == (37, 5)
        assert z["score"].dtype == np.float32 and z["score"].shape == (37, 5)
        assert z["rank"].dtype == np.int32 and z["rank"].shape == (37,)
        for i in range(37):                                  # rank and idx agree: the partner is in the list iff fewer than K rows beat it
            pos = np.flatnonzero(z["idx"][i] == i)
            assert (len(pos) == 1) == (z["rank"][i] < 5), (d, i)
            if len(pos):
                assert np.sum(z["score"][i] > z["score"][i, pos[0]]) == z["rank"][i]
    a, b = np.load(res / "retrieve_c2g.npz")["idx"], np.load(res / "retrieve_g2c.npz")["idx"]
    assert not np.array_equal(a, b)                          # (the two directions are different questions)
    res1 = tmp_path / "one"
    assert drivers.cmd_retrieve(["--path", str(src), "--direction", "g2c", "--topk", "50", "--res_dir", str(res1)], engine=eng) == 0
    assert [p.name for p in res1.iterdir()] == ["retrieve_g2c.npz"]
    z = np.load(res1 / "retrieve_g2c.npz")                   # --topk larger than N
    assert z["idx"].shape == (37, 50) and np.all(z["idx"][:, 37:] == -1) and np.all(np.isneginf(z["score"][:, 37:]))
    assert np.all(np.sort(z["idx"][:, :37], axis=1) == np.arange(37))
    assert np.array_equal(z["idx"][:, :5], b)
    with pytest.raises(SystemExit):
        drivers.cmd_retrieve(["--path", str(src), "--topk", "129"], engine=eng)
    with pytest.raises(SystemExit):
        drivers.cmd_retrieve(["--path", str(tmp_path / "res")], engine=eng)          # no .pkl there


def test_engine_sim_topk_refuses_bad_arguments_before_it_needs_a_device():
    assert len(_SIGS["jg_sim_topk"]) == 11 and "jg_sim_topk" in EXPORTS
    eng = Engine.__new__(Engine)                     # no handle, no device: every check below comes before either is touched
    q, g = torch.zeros(20, 512), torch.zeros(30, 512)
    ok_i, ok_s = torch.zeros(20, 5, dtype=torch.int32), torch.zeros(20, 5)
    bad = [dict(queries=torch.zeros(512), gallery=g, k=5),                          # not (rows, D)
           dict(queries=q, gallery=torch.zeros(30, 256), k=5),                      # different D
           dict(queries=torch.zeros(20, 96), gallery=torch.zeros(30, 96), k=5),     # D % 64
           dict(queries=torch.zeros(20, 0), gallery=torch.zeros(30, 0), k=5),       # D = 0
           dict(queries=q, gallery=g, k=0), dict(queries=q, gallery=g, k=129),
           dict(queries=q, gallery=g, k=5, gallery_offset=-1),
           dict(queries=q, gallery=g, k=5, gallery_offset=2 ** 31 - 30),            # gallery_offset + rows > INT32_MAX
           dict(queries=q, gallery=g, k=5, merge_into=ok_i),                        # not a pair
           dict(queries=q, gallery=g, k=5, merge_into=(ok_i, ok_s[:, :4])),         # shapes
           dict(queries=q, gallery=g, k=5, merge_into=(ok_i[:19], ok_s[:19])),
           dict(queries=q, gallery=g, k=5, merge_into=(ok_i.to(torch.int64), ok_s)),        # dtypes
           dict(queries=q, gallery=g, k=5, merge_into=(ok_i, ok_s.to(torch.float64))),
           dict(queries=q, gallery=g, k=5, merge_into=(ok_s, ok_i))]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.sim_topk(**kw)


_WORKER = textwrap.dedent(r"""
    import os, sys
    import numpy as np, torch
    for p in ("tests", "oracle", ""):
        sys.path.insert(0, os.path.join({root!r}, p))
    from jegal_amd import dist as jdist, metrics as M, synth
    from test_sim_topk_cpu import NumpyEngine, topk_reference
    jdist.init_from_env("gloo")
    assert jdist.world_size() == 2
    N = 101
    g, c = synth.planted_retrieval(5, N)
    g[7] = g[3]
    lo, hi = jdist.shard_range(N)                      # ragged: 51 + 50 rows
    eng = NumpyEngine()
    idx, score = M.retrieve(c[lo:hi], g[lo:hi], k=7, engine=eng)
    assert eng.calls == [dict(n=hi - lo, m=N, k=7)]    # this rank's queries against the assembled gallery
    want_i, want_s = topk_reference(eng.l2norm(c).numpy(), eng.l2norm(g).numpy(), 7)
    assert idx.shape == (N, 7) and idx.dtype == np.int32 and score.dtype == np.float32
    assert np.array_equal(idx, want_i.numpy()), "idx"  # global gallery rows, all ranks' queries in rank order
    assert np.array_equal(score, want_s.numpy()), "score"
    assert np.array_equal(M.partner_ranks(c[lo:hi], g[lo:hi], engine=eng), eng.sim_rank(eng.l2norm(c), eng.l2norm(g))[0].numpy())
    jdist.barrier()
    print("rank", jdist.rank(), "ok")
    """)


def test_two_rank_gloo_sharded_retrieve(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    for attempt in range(3):                         # a rendezvous port lost to another process is retried, a failed assertion is not
        outs = _run_two_ranks(script)
        if all(rc == 0 for rc, _ in outs):
            break
        text = "\n".join(o for _, o in outs)
        if "AssertionError" in text or attempt == 2:
            raise AssertionError(text)
    for rc, out in outs:
        assert " ok" in out
