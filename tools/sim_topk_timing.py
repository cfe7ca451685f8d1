"""Time jg_sim_topk next to jg_sim_rank and next to the route without it (torch.mm + torch.topk, which writes the N x N matrix) on
synth.planted_retrieval(1237, N), rows normalised on the engine, device-resident.  GPU only, no fallback.
Each iteration runs every variant back to back, each call between its own pair of device events, so the variants alternate in one
process and every iteration is one comparison.  --baseline-lib: another build of libjegal_hip.so (the parent commit's, when kernels are
to be compared across builds): every jg_ variant then runs from both libraries, this build's call and the other's next to each other, the
other's jg_sim_rank is the yardstick, and the result carries the other's figures ("baseline"), the per-iteration ratios this build /
other ("over_baseline") and the other's spread: max / min - 1 over the iterations of its variant / its own jg_sim_rank.
FLOPs come from the shapes: 2 N^2 D; roof 157 TFLOP/s (fp32 MFMA).
The flush model is host arithmetic on the first --model-blocks workgroups (64 query rows each): with the threshold of a row = its k-th
best score over the tiles before, per 64-column tile the number of scores that pass it (= keys queued; the flush inserts those that still beat the running threshold) and the rows with a
non-empty queue (= row flushes).
  python tools/sim_topk_timing.py [--iters 30] [--n 10000] [--baseline-lib PATH] [--out profiles/sim_topk_timing.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jegal_amd import synth  # noqa: E402
from jegal_amd._lib import Engine  # noqa: E402

MFMA32_FLOPS = 157.0e12
KS = (1, 10, 50, 128)
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def summarise(ms, flop):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()), "share_of_fp32_mfma_roof": flop / MFMA32_FLOPS * 1e3 / med}


def flush_model(q, g, k, blocks):
    """per workgroup (mean over `blocks` of them): keys queued per row, row flushes, tiles in which any row flushed"""
    ins, rowfl, tiles = [], [], []
    ntiles = -(-g.shape[0] // 64)
    for b in range(blocks):
        s = q[b * 64:(b + 1) * 64].astype(np.float64) @ g.astype(np.float64).T
        best = np.full((s.shape[0], k), -np.inf)
        n_ins = n_rows = n_tiles = 0
        for t in range(ntiles):
            st = s[:, t * 64:(t + 1) * 64]
            passed = st > best[:, :1]                      # best is kept ascending: column 0 is the k-th best so far
            n_ins += int(passed.sum())
            n_rows += int(passed.any(axis=1).sum())
            n_tiles += int(passed.any())
            best = np.sort(np.concatenate([best, np.where(passed, st, -np.inf)], axis=1), axis=1)[:, -k:]
        ins.append(n_ins / s.shape[0])
        rowfl.append(n_rows)
        tiles.append(n_tiles)
    return {"keys_queued_per_row": float(np.mean(ins)), "row_flushes_per_workgroup": float(np.mean(rowfl)),
            "tiles_with_a_flush_per_workgroup": float(np.mean(tiles)), "tiles": ntiles, "blocks_modelled": blocks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--model-blocks", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_topk_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sim_topk_timing needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng._bind_stream()
    lib, h = eng.lib, eng.h
    N, D = args.n, 512
    ge, ce = synth.planted_retrieval(1237, N)
    q, g = eng.l2norm(torch.from_numpy(ce)), eng.l2norm(torch.from_numpy(ge))
    rank = torch.empty(N, dtype=torch.int32, device="cuda")
    ties = torch.empty(N, dtype=torch.int32, device="cuda")
    outs = {k: (torch.empty((N, k), dtype=torch.int32, device="cuda"), torch.empty((N, k), dtype=torch.float32, device="cuda")) for k in KS}

    libs = {"": (lib, h)}                                  # variant name prefix -> (library, handle)
    if args.baseline_lib:
        base_lib = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        base_h = ctypes.c_void_p()
        assert base_lib.jg_create(0, ctypes.byref(base_h)) == 0
        for fn in ("jg_sim_rank", "jg_sim_topk", "jg_set_stream"):
            getattr(base_lib, fn).argtypes = getattr(lib, fn).argtypes
        assert base_lib.jg_set_stream(base_h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        libs["baseline/"] = (base_lib, base_h)

    def sim_rank(l, lh):
        assert l.jg_sim_rank(lh, P(q), P(g), N, N, 0, D, P(rank), P(ties)) == 0

    def topk(l, lh, k):
        assert l.jg_sim_topk(lh, P(q), P(g), N, N, D, k, 0, 0, P(outs[k][0]), P(outs[k][1])) == 0

    torch_out = {}

    def torch_route():
        torch_out["r"] = torch.topk(torch.mm(q, g.t()), 10, dim=1)

    jg = [("jg_sim_rank", sim_rank)] + [(f"jg_sim_topk_k{k}", (lambda l, lh, k=k: topk(l, lh, k))) for k in KS]
    # the other build's call first: what is left in `outs` and compared with torch below is this build's
    variants = [(pre + name, (lambda fn=fn, pre=pre: fn(*libs[pre]))) for name, fn in jg for pre in reversed(list(libs))]
    variants.append(("torch_mm_topk_k10", torch_route))
    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(args.iters):
        evs = []
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in evs:
            times[name].append(e0.elapsed_time(e1))
    flop = 2.0 * N * N * D
    res = {"input": f"synth.planted_retrieval(1237, {N}), D = {D}, rows normalised by jg_l2norm", "iters": args.iters, "flop": flop,
           "fp32_mfma_flop_per_s": MFMA32_FLOPS, "jg_sim_rank_from": os.path.basename(args.baseline_lib) if args.baseline_lib else "this build"}

    def ratio(a, b):
        r = np.asarray(times[a]) / np.asarray(times[b])
        return {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}

    yard = "baseline/jg_sim_rank" if args.baseline_lib else "jg_sim_rank"
    for name, _ in variants:
        if name.startswith("baseline/"):
            continue
        res[name] = summarise(times[name], flop)
        if name != "jg_sim_rank":
            res[name]["over_jg_sim_rank"] = ratio(name, yard)
        if "baseline/" + name in times:
            base = summarise(times["baseline/" + name], flop)
            base["over_jg_sim_rank"] = ratio("baseline/" + name, yard)
            base["spread"] = base["over_jg_sim_rank"]["max"] / base["over_jg_sim_rank"]["min"] - 1.0
            res[name]["baseline"] = base
            res[name]["over_baseline"] = ratio(name, "baseline/" + name)
    # what the device route and the torch route agree on: the share of equal neighbours at k = 10 (their summation orders differ)
    res["k10_indices_equal_to_torch_share"] = float((outs[10][0].cpu() == torch_out["r"].indices.cpu().to(torch.int32)).float().mean())
    qh, gh = q.cpu().numpy(), g.cpu().numpy()
    res["flush_model"] = {f"k{k}": flush_model(qh, gh, k, args.model_blocks) for k in KS}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if args.baseline_lib:
        base_lib.jg_destroy.argtypes = [ctypes.c_void_p]
        base_lib.jg_destroy(base_h)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
