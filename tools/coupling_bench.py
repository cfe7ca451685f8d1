"""Time jg_sim_coupling on the late-interaction evaluation of N utterances against N clips: --words words per utterance (default 8) and
--frames frames per clip (default 150), D = 512, unit rows (neighbouring frames of a clip nearly equal), one group per clip, k = 10, for
N in --clips (default 500, 2000, 10000).  GPU only, no fallback.  Data is device resident; every call runs between its own pair of device
events after --warmup untimed rounds; the variants alternate inside every iteration, so drift hits all of them alike:
  coupling_f32          jg_sim_coupling, JG_F32 gallery, slices = 0 (the plan: `plan`), lists only
  coupling_f32_pair     ... and the dense (N, N) output
  coupling_f16          JG_F16 gallery (the same rows rounded to fp16), lists only
  coupling_f16_pair     ... and the dense output
  torch                 the composition on the same device where its (N words) x (N frames) matrix fits in --torch-bytes: words @ gallery.T,
                        a max per clip by reshape, a mean per query; where it does not fit, that is recorded in place of a time
Reported per variant: median, min and max over the iterations, the exact-fp32 work 2 (N words) (N frames) D over the median as TFLOP/s, and
the per-iteration ratio to `torch` (median, min, max: the spread).  The results are checked while they are there: the lists of the pair
and the list-only variants must be equal bit for bit, the lists must be the top k of the dense output, and the dense output must agree
with torch's to the fp32 chains' bound (D + words) 2^-24.
  python tools/coupling_bench.py [--clips 500 2000 10000] [--iters 10 5 2] [--warmup 1] [--out profiles/coupling_bench.json]
--ordered: jg_sim_ordered against jg_sim_coupling on the same data, lists only, both gallery types, the four calls alternating inside
every iteration, --windows windows (default 3) of warm-up and iterations each; per variant the median of every window, and the
per-iteration ratio ordered / coupling.  --parent-results FILES: result files this tool wrote from ANOTHER build's tree (the parent
commit's, run in between on the same machine) whose coupling_f32 / coupling_f16 medians are recorded next to this build's.
--align: jg_sim_align alone for the first 10 utterances x k = 10 of the same corpus, ordered and not: a cost per returned result.
Both write into --out (default profiles/ordered_bench.json), each under its own key, keeping what the other left there."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jegal_amd._lib import Engine, coupling_plan  # noqa: E402

K, D = 10, 512
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def make_case(eng, N, W, T):
    """-> (g32, g16, words, w_off (host), g_off (device)): N clips of T unit frames (a random walk per clip), N utterances of W words"""
    gen = torch.Generator(device="cuda").manual_seed(20262 + N)
    g = torch.randn((N, 1, D), generator=gen, device="cuda") + torch.cumsum(0.05 * torch.randn((N, T, D), generator=gen, device="cuda"), dim=1)
    g32 = eng.l2norm(g.reshape(N * T, D))
    del g
    # utterance i: W frames of clip i with noise, so the partner ranks high as it would after training
    pick = (torch.arange(N, device="cuda")[:, None] * T + torch.randint(0, T, (N, W), generator=gen, device="cuda")).reshape(-1)
    words = eng.l2norm(g32[pick] + 0.05 * torch.randn((N * W, D), generator=gen, device="cuda"))
    return (g32, g32.half(), words, np.arange(0, N * W + 1, W, dtype=np.int32), torch.arange(0, N * T + 1, T, dtype=torch.int32, device="cuda"))


def timed_rounds(names, run, warmup, iters):
    """warmup untimed rounds, then iters rounds of every name in turn between its own events -> {name: [ms]}"""
    for _ in range(warmup):
        for n in names:
            run(n)
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(iters):
        evs = []
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(n)
            e1.record()
            evs.append((n, e0, e1))
        torch.cuda.synchronize()
        for n, e0, e1 in evs:
            times[n].append(e0.elapsed_time(e1))
    return times


def ordered_modes(args, eng):
    """--ordered and --align (the module docstring)"""
    lib, h = eng.lib, eng.h
    W, T = args.words, args.frames
    out = args.out or os.path.join(ROOT, "profiles", "ordered_bench.json")
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["input"] = f"N utterances x {W} words against N clips x {T} frames, D = {D}, unit rows (random walk per clip), one group per clip, k = {K}"
    res["num_cu"] = torch.cuda.get_device_properties(0).multi_processor_count
    parent = [json.load(open(f)) for f in args.parent_results]
    for ci, N in enumerate(args.clips):
        iters = args.iters[min(ci, len(args.iters) - 1)]
        g32, g16, words, w_off, g_off = make_case(eng, N, W, T)
        wo = w_off.ctypes.data_as(ctypes.c_void_p)
        if args.ordered:
            names = ["ordered_f32", "coupling_f32", "ordered_f16", "coupling_f16"]
            outs = {n: (torch.empty((N, K), dtype=torch.int32, device="cuda"), torch.empty((N, K), dtype=torch.float32, device="cuda")) for n in names}

            def run(name):
                i, s = outs[name]
                f16 = "f16" in name
                entry = lib.jg_sim_ordered if name.startswith("ordered") else lib.jg_sim_coupling
                rc = entry(h, P(words), wo, N, P(g16 if f16 else g32), int(f16), N * T, D, K, P(g_off), N, 0, 0, 0, P(i), P(s), None, N)
                assert rc == 0, (name, rc, lib.jg_last_error(h))

            # (a run appends its windows to those an earlier run left in --out: runs of another build's tree may lie in between)
            case = res.get("ordered", {}).get(f"N={N}") or {"iters_per_window": iters, "warmup_per_window": args.warmup, "word_rows": N * W,
                                                             "frame_rows": N * T, "windows": [], "ratio_samples": {"f32": [], "f16": []}}
            ratios = case["ratio_samples"]
            for _ in range(args.windows):
                times = timed_rounds(names, run, args.warmup, iters)
                case["windows"].append({n: stats(times[n]) for n in names})
                for t in ratios:
                    ratios[t] += (np.asarray(times["ordered_" + t]) / np.asarray(times["coupling_" + t])).tolist()
            for t, r in ratios.items():
                case[f"ordered_over_coupling_{t}"] = {"median": float(np.median(r)), "min": float(np.min(r)), "max": float(np.max(r))}
            if parent:
                case["parent_build_windows"] = [{n: p["cases"][f"N={N}"][n] for n in ("coupling_f32", "coupling_f16")} for p in parent
                                                if f"N={N}" in p.get("cases", {})]
            case["best_ordered_score_never_above_best_coupling_score"] = bool((outs["ordered_f32"][1][:, 0] <= outs["coupling_f32"][1][:, 0]).all())
            case["partner_is_first_share"] = {n: float((outs[n][0][:, 0] == torch.arange(N, device="cuda")).float().mean()) for n in ("ordered_f32", "coupling_f32")}
            res.setdefault("ordered", {})[f"N={N}"] = case
            print(f"ordered N={N}: " + json.dumps(case), flush=True)
        if args.align:
            nq = min(10, N)
            idx, sc = torch.empty((nq, K), dtype=torch.int32, device="cuda"), torch.empty((nq, K), dtype=torch.float32, device="cuda")
            frames, fs = torch.empty((nq, K, W), dtype=torch.int32, device="cuda"), torch.empty((nq, K), dtype=torch.float32, device="cuda")
            case = {"queries": nq, "k": K, "iters": iters, "frame_rows": N * T}
            for ordered in (1, 0):
                entry = lib.jg_sim_ordered if ordered else lib.jg_sim_coupling
                rc = entry(h, P(words), wo, nq, P(g32), 0, N * T, D, K, P(g_off), N, 0, 0, 0, P(idx), P(sc), None, nq)
                assert rc == 0, (rc, lib.jg_last_error(h))

                def run(name):
                    rc = lib.jg_sim_align(h, P(words), wo, nq, P(g16 if "f16" in name else g32), int("f16" in name), N * T, D, P(g_off), N, 0, P(idx),
                                          K, ordered, P(frames), W, P(fs))
                    assert rc == 0, (name, rc, lib.jg_last_error(h))
                tag = "ordered" if ordered else "unordered"
                times = timed_rounds([f"align_{tag}_f32", f"align_{tag}_f16"], run, args.warmup, max(iters, 5))
                for n, ms in times.items():
                    case[n] = stats(ms)
                run(f"align_{tag}_f32")
                torch.cuda.synchronize()
                case[f"{tag}_scores_equal_the_scoring_entry"] = bool(torch.equal(fs.view(torch.int32), sc.view(torch.int32)))
                case[f"{tag}_every_word_has_a_frame"] = bool((frames >= 0).all())
            res.setdefault("align", {})[f"N={N}"] = case
            print(f"align N={N}: " + json.dumps(case), flush=True)
        del g32, g16, words
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    eng.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[500, 2000, 10000])
    ap.add_argument("--iters", type=int, nargs="+", default=[10, 5, 2], help="one count per entry of --clips (the last one repeats)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--words", type=int, default=8)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--torch-bytes", type=float, default=64e9, help="the largest (N words) x (N frames) fp32 matrix the torch composition may write")
    ap.add_argument("--out", default=None, help="default: profiles/coupling_bench.json, or profiles/ordered_bench.json with --ordered / --align")
    ap.add_argument("--ordered", action="store_true", help="time jg_sim_ordered against jg_sim_coupling instead")
    ap.add_argument("--align", action="store_true", help="time jg_sim_align for 10 queries x k = 10 instead")
    ap.add_argument("--windows", type=int, default=3, help="--ordered: windows of warm-up and iterations")
    ap.add_argument("--parent-results", nargs="*", default=[], help="--ordered: result files of this tool from another build's tree")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coupling_bench needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng._bind_stream()
    if args.ordered or args.align:
        return ordered_modes(args, eng)
    args.out = args.out or os.path.join(ROOT, "profiles", "coupling_bench.json")
    lib, h = eng.lib, eng.h
    W, T = args.words, args.frames
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"input": f"N utterances x {W} words against N clips x {T} frames, D = {D}, unit rows (random walk per clip), one group per clip, k = {K}",
           "warmup": args.warmup, "num_cu": num_cu, "cases": {}}
    for ci, N in enumerate(args.clips):
        iters = args.iters[min(ci, len(args.iters) - 1)]
        gen = torch.Generator(device="cuda").manual_seed(20262 + N)
        g = torch.randn((N, 1, D), generator=gen, device="cuda") + torch.cumsum(0.05 * torch.randn((N, T, D), generator=gen, device="cuda"), dim=1)
        g32 = eng.l2norm(g.reshape(N * T, D))
        del g
        g16 = g32.half()
        # utterance i: W frames of clip i with noise, so the partner ranks high as it would after training
        pick = (torch.arange(N, device="cuda")[:, None] * T + torch.randint(0, T, (N, W), generator=gen, device="cuda")).reshape(-1)
        words = eng.l2norm(g32[pick] + 0.05 * torch.randn((N * W, D), generator=gen, device="cuda"))
        w_off = np.arange(0, N * W + 1, W, dtype=np.int32)
        g_off = torch.arange(0, N * T + 1, T, dtype=torch.int32, device="cuda")
        flop = 2.0 * (N * W) * (N * T) * D
        matrix_bytes = 4.0 * (N * W) * (N * T)
        names = ["coupling_f32", "coupling_f32_pair", "coupling_f16", "coupling_f16_pair"]
        with_torch = matrix_bytes <= args.torch_bytes
        if with_torch:
            names.append("torch")
        outs = {n: (torch.empty((N, K), dtype=torch.int32, device="cuda"), torch.empty((N, K), dtype=torch.float32, device="cuda"),
                    torch.empty((N, N), dtype=torch.float32, device="cuda") if n.endswith("_pair") else None) for n in names if n != "torch"}
        dense = {}

        def run(name):
            if name == "torch":
                dense["torch"] = (words @ g32.t()).view(N * W, N, T).amax(dim=2).view(N, W, N).mean(dim=1)
                return
            i, s, p = outs[name]
            f16 = "f16" in name
            rc = lib.jg_sim_coupling(h, P(words), w_off.ctypes.data_as(ctypes.c_void_p), N, P(g16 if f16 else g32), int(f16), N * T, D, K, P(g_off), N,
                                     0, 0, 0, P(i), P(s), P(p), N)
            assert rc == 0, (name, rc, lib.jg_last_error(h))

        for _ in range(args.warmup):
            for n in names:
                run(n)
        torch.cuda.synchronize()
        times = {n: [] for n in names}
        for _ in range(iters):
            evs = []
            for n in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(n)
                e1.record()
                evs.append((n, e0, e1))
            torch.cuda.synchronize()
            for n, e0, e1 in evs:
                times[n].append(e0.elapsed_time(e1))
        tfq, slices, rows_per_slice, ws = coupling_plan(w_off, N * T, K, num_cu)
        case = {"iters": iters, "word_rows": N * W, "frame_rows": N * T, "exact_fp32_flop": flop, "torch_matrix_bytes": matrix_bytes,
                "plan (query tiles, slices, rows per slice, list bytes)": [len(tfq) - 1, slices, rows_per_slice, ws]}
        for n in names:
            case[n] = stats(times[n])
            case[n]["tflops_at_median"] = flop / (case[n]["median_ms"] * 1e-3) / 1e12
            if with_torch:
                r = np.asarray(times[n]) / np.asarray(times["torch"])
                case[n]["over_torch"] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}
        if not with_torch:
            case["torch"] = f"not run: its matrix of {matrix_bytes / 1e9:.1f} GB does not fit (--torch-bytes {args.torch_bytes / 1e9:.0f} GB)"
        same = lambda a, b: bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
        case["lists_equal_with_and_without_pair"] = same(outs["coupling_f32"], outs["coupling_f32_pair"]) and same(outs["coupling_f16"], outs["coupling_f16_pair"])
        pair = outs["coupling_f32_pair"][2].t()                              # (N queries, N groups)
        top = torch.topk(pair, K, dim=1)
        case["list_scores_are_the_top_k_of_pair"] = bool(torch.equal(top.values.view(torch.int32), outs["coupling_f32_pair"][1].view(torch.int32)))
        case["partner_is_first_share"] = float((outs["coupling_f32"][0][:, 0] == torch.arange(N, device="cuda")).float().mean())
        if with_torch:
            err = float((pair - dense["torch"]).abs().max())
            case["max_abs_difference_to_torch"] = err
            case["bound (D + words) 2^-24, doubled for torch's own chain"] = 2 * (D + W) * 2.0 ** -24
            case["within_bound"] = err <= 2 * (D + W) * 2.0 ** -24
        res["cases"][f"N={N}"] = case
        print(f"N={N}: " + json.dumps(case), flush=True)
        del outs, dense, g32, g16, words
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
