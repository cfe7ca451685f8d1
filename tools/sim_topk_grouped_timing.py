"""Time jg_sim_topk_grouped next to jg_sim_topk on the workload it is for: a corpus of --clips clips x --frames frames (D = 512, unit rows,
neighbouring frames of a clip nearly equal: a random walk around the clip's own direction), --queries unit query rows (noisy copies of
corpus frames), k = 10.  GPU only, no fallback.  Variants, run back to back in every iteration, each call between its own pair of device
events:
  jg_sim_topk                 the same tile loop over the same frame rows without grouping: the yardstick (unchanged from the parent commit)
  grouped_per_clip            jg_sim_topk_grouped, one group per clip: what metrics.search runs
  grouped_per_row             groups of one row: jg_sim_topk's result through the grouped epilogue and flush
  grouped_one_group           one group over everything: the list never fills, every score is queued and replaces the champion or is dropped
--baseline-lib: another build of libjegal_hip.so (the parent commit's, when kernels are to be compared across builds): every variant then
runs from both libraries, this build's call and the other's next to each other, and so does the other's jg_sim_rank on the same rows; the
result carries the other's figures ("baseline"), the per-iteration ratios this build / other ("over_baseline") and the other's spread:
max / min - 1 over the iterations of its variant / its own jg_sim_rank.
FLOPs come from the shapes: 2 Q N D; roof 157 TFLOP/s (fp32 MFMA).
The queue model is arithmetic on the first workgroup's 64 query rows (torch, on the device, from the matrix the kernels never write): per
64-row tile, with the threshold of a row = its k-th best score (rows) or k-th best group champion (groups) over the tiles before, the keys
that pass it (= keys queued = insertions attempted) and the rows with a non-empty queue (= row flushes).
  python tools/sim_topk_grouped_timing.py [--iters 10] [--clips 4000] [--frames 150] [--queries 1000] [--baseline-lib PATH]
         [--out profiles/sim_topk_grouped_timing.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jegal_amd._lib import Engine  # noqa: E402

MFMA32_FLOPS = 157.0e12
K = 10
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def summarise(ms, flop):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()), "share_of_fp32_mfma_roof": flop / MFMA32_FLOPS * 1e3 / med}


def queue_model(q64, g, k, group_of_row, n_groups):
    """first workgroup: keys queued per row, row flushes, tiles with a flush.  group_of_row: (N,) int64 device tensor, or None (every row
    its own group: the running k best rows)"""
    s = q64 @ g.t()                                                # (64, N): this model's matrix, not the kernels'
    rows, N = s.shape
    ntiles = -(-N // 64)
    queued = flushes = tiles = 0
    if group_of_row is None:
        best = torch.full((rows, k), float("-inf"), device=s.device)
    else:
        champ = torch.full((rows, n_groups), float("-inf"), device=s.device)
    for t in range(ntiles):
        st = s[:, t * 64:(t + 1) * 64]
        if group_of_row is None:
            thr = best[:, -1:]
        else:
            thr = torch.topk(champ, min(k, n_groups), dim=1).values[:, -1:] if n_groups >= k else torch.full((rows, 1), float("-inf"), device=s.device)
        passed = st > thr
        queued += int(passed.sum())
        flushes += int(passed.any(dim=1).sum())
        tiles += int(passed.any())
        if group_of_row is None:
            best = torch.topk(torch.cat([best, st], dim=1), k, dim=1).values
        else:
            gid = group_of_row[t * 64:(t + 1) * 64].unsqueeze(0).expand(rows, -1)
            champ.scatter_reduce_(1, gid, st, reduce="amax")
    return {"keys_queued_per_row": queued / rows, "row_flushes_per_workgroup": flushes, "tiles_with_a_flush_per_workgroup": tiles, "tiles": ntiles}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=4000)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_topk_grouped_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sim_topk_grouped_timing needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng._bind_stream()
    lib, h = eng.lib, eng.h
    C, T, Q, D = args.clips, args.frames, args.queries, 512
    N = C * T
    gen = torch.Generator(device="cuda").manual_seed(20260)
    g = torch.randn((C, 1, D), generator=gen, device="cuda") + torch.cumsum(0.05 * torch.randn((C, T, D), generator=gen, device="cuda"), dim=1)
    g = eng.l2norm(g.reshape(N, D))
    pick = torch.randint(0, N, (Q,), generator=gen, device="cuda")
    q = eng.l2norm(g[pick] + 0.05 * torch.randn((Q, D), generator=gen, device="cuda"))
    offs = {"grouped_per_clip": torch.arange(0, N + 1, T, dtype=torch.int32, device="cuda"),
            "grouped_per_row": torch.arange(0, N + 1, dtype=torch.int32, device="cuda"),
            "grouped_one_group": torch.tensor([0, N], dtype=torch.int32, device="cuda")}
    names = ["jg_sim_topk"] + list(offs)
    outs = {n: (torch.empty((Q, K), dtype=torch.int32, device="cuda"), torch.empty((Q, K), dtype=torch.float32, device="cuda")) for n in names}
    libs = {"": (lib, h)}                                          # variant name prefix -> (library, handle)
    if args.baseline_lib:
        base_lib = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        base_h = ctypes.c_void_p()
        assert base_lib.jg_create(0, ctypes.byref(base_h)) == 0
        for fn in ("jg_sim_rank", "jg_sim_topk", "jg_sim_topk_grouped", "jg_set_stream"):
            getattr(base_lib, fn).argtypes = getattr(lib, fn).argtypes
        assert base_lib.jg_set_stream(base_h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        libs["baseline/"] = (base_lib, base_h)
        rank = torch.empty(Q, dtype=torch.int32, device="cuda")
        ties = torch.empty(Q, dtype=torch.int32, device="cuda")

    def run(name):
        l, lh = libs["baseline/" if name.startswith("baseline/") else ""]
        name = name.replace("baseline/", "")
        if name == "jg_sim_rank":
            rc = l.jg_sim_rank(lh, P(q), P(g), Q, N, 0, D, P(rank), P(ties))
        elif name == "jg_sim_topk":
            rc = l.jg_sim_topk(lh, P(q), P(g), Q, N, D, K, 0, 0, P(outs[name][0]), P(outs[name][1]))
        else:
            rc = l.jg_sim_topk_grouped(lh, P(q), P(g), Q, N, D, K, P(offs[name]), offs[name].numel() - 1, 0, 0, P(outs[name][0]), P(outs[name][1]))
        assert rc == 0, name

    # the other build's call first: what is left in `outs` and checked below is this build's
    runs = [pre + n for n in names for pre in reversed(list(libs))] + (["baseline/jg_sim_rank"] if args.baseline_lib else [])
    for _ in range(args.warmup):
        for n in runs:
            run(n)
    torch.cuda.synchronize()
    times = {n: [] for n in runs}
    for _ in range(args.iters):
        evs = []
        for n in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(n)
            e1.record()
            evs.append((n, e0, e1))
        torch.cuda.synchronize()
        for n, e0, e1 in evs:
            times[n].append(e0.elapsed_time(e1))
    flop = 2.0 * Q * N * D
    res = {"input": f"{C} clips x {T} frames, D = {D}, unit rows (random walk per clip), {Q} query rows = noisy corpus frames, k = {K}",
           "iters": args.iters, "flop": flop, "fp32_mfma_flop_per_s": MFMA32_FLOPS, "workgroups": -(-Q // 64), "tiles_per_workgroup": -(-N // 64)}
    yard = np.asarray(times["jg_sim_topk"])

    def ratio(a, b):
        r = np.asarray(times[a]) / np.asarray(times[b])
        return {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}

    for n in names:
        res[n] = summarise(times[n], flop)
        if args.baseline_lib:
            base = summarise(times["baseline/" + n], flop)
            base["over_jg_sim_rank"] = ratio("baseline/" + n, "baseline/jg_sim_rank")
            base["spread"] = base["over_jg_sim_rank"]["max"] / base["over_jg_sim_rank"]["min"] - 1.0
            res[n]["baseline"] = base
            res[n]["over_baseline"] = ratio(n, "baseline/" + n)
        if n != "jg_sim_topk":
            r = np.asarray(times[n]) / yard
            res[n]["over_jg_sim_topk"] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}
            res[n]["extra_ms_over_jg_sim_topk_median"] = float(np.median(np.asarray(times[n]) - yard))
    # what the variants must agree on: groups of one row are jg_sim_topk; every per-clip champion is a frame of its clip, clips distinct
    ti, ts = outs["jg_sim_topk"]
    ri, rs = outs["grouped_per_row"]
    res["per_row_equals_jg_sim_topk"] = bool(torch.equal(ti, ri) and torch.equal(ts.view(torch.int32), rs.view(torch.int32)))
    ci, cs = outs["grouped_per_clip"]
    clip = torch.div(ci, T, rounding_mode="floor")
    res["per_clip_rows_in_distinct_clips"] = bool((torch.sort(clip, dim=1).values.diff(dim=1) > 0).all())
    res["per_clip_best_equals_jg_sim_topk_best"] = bool(torch.equal(ci[:, 0], ti[:, 0]) and torch.equal(cs[:, 0].view(torch.int32), ts[:, 0].view(torch.int32)))
    res["distinct_clips_in_jg_sim_topk_top10_mean"] = float(torch.tensor([len(set(r.tolist())) for r in torch.div(ti, T, rounding_mode="floor").cpu()], dtype=torch.float32).mean())
    oi, _ = outs["grouped_one_group"]
    res["one_group_returns_one_row"] = bool((oi[:, 0] == ti[:, 0]).all() and (oi[:, 1:] == -1).all())
    if not args.no_model:
        q64 = q[:64]
        res["queue_model_first_workgroup"] = {
            "jg_sim_topk / grouped_per_row": queue_model(q64, g, K, None, N),
            "grouped_per_clip": queue_model(q64, g, K, torch.arange(N, device="cuda") // T, C),
            "grouped_one_group": queue_model(q64, g, K, torch.zeros(N, dtype=torch.int64, device="cuda"), 1)}
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
