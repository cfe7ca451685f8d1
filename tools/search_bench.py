"""Time jg_sim_search next to jg_sim_topk_grouped on the search the README leads with: a corpus of --clips clips x --frames frames (D = 512,
unit rows, neighbouring frames of a clip nearly equal), one group per clip, k = 10, for --queries query rows each (default 1, 64, 1024:
a word, a query file's worth, a batch).  GPU only, no fallback.  Data is device resident; every call runs between its own pair of device
events after --warmup untimed rounds; the variants alternate inside every iteration, so drift hits all of them alike:
  grouped            jg_sim_topk_grouped: ceil(Q / 64) workgroups, each walking the whole gallery
  search_f32         jg_sim_search, JG_F32 gallery, slices = 0 (the planner's cut: `plan`)
  search_f16         jg_sim_search, JG_F16 gallery (the same rows rounded to fp16), slices = 0
  search_f32_s<N>    with --slices N [N ..]: forced cuts, to see where the planner's constants stand
--baseline-lib: another build of libjegal_hip.so (the parent commit's): its jg_sim_topk_grouped runs as `baseline/grouped` next to the others.
Reported per variant: median, min and max over the iterations, and the per-iteration ratio to `grouped` (median, min, max: the spread).
The results are checked while they are there: search_f32 must equal grouped bit for bit, search_f16 the grouped call on the widened rows.
  python tools/search_bench.py [--iters 10] [--warmup 2] [--clips 4000] [--frames 150] [--queries 1 64 1024] [--slices ...]
         [--baseline-lib PATH] [--out profiles/search_bench.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jegal_amd._lib import Engine, JegalError, search_plan  # noqa: E402

K, D = 10, 512
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=4000)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--slices", type=int, nargs="*", default=[])
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_bench needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng._bind_stream()
    lib, h = eng.lib, eng.h
    C, T = args.clips, args.frames
    N = C * T
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    gen = torch.Generator(device="cuda").manual_seed(20261)
    g = torch.randn((C, 1, D), generator=gen, device="cuda") + torch.cumsum(0.05 * torch.randn((C, T, D), generator=gen, device="cuda"), dim=1)
    g32 = eng.l2norm(g.reshape(N, D))
    del g
    g16 = g32.half()
    off = torch.arange(0, N + 1, T, dtype=torch.int32, device="cuda")
    base = None
    if args.baseline_lib:
        base_lib = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        base_h = ctypes.c_void_p()
        assert base_lib.jg_create(0, ctypes.byref(base_h)) == 0
        for fn in ("jg_sim_topk_grouped", "jg_set_stream"):
            getattr(base_lib, fn).argtypes = getattr(lib, fn).argtypes
        assert base_lib.jg_set_stream(base_h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        base = (base_lib, base_h)
    res = {"input": f"{C} clips x {T} frames = {N} rows, D = {D}, unit rows (random walk per clip), one group per clip, k = {K}",
           "iters": args.iters, "warmup": args.warmup, "num_cu": num_cu, "cases": {}}
    for Q in args.queries:
        pick = torch.randint(0, N, (Q,), generator=gen, device="cuda")
        q = eng.l2norm(g32[pick] + 0.05 * torch.randn((Q, D), generator=gen, device="cuda"))
        cuts = []
        for s in args.slices:                            # (a cut whose lists exceed the cap is refused: left out here, by the planner's word)
            try:
                search_plan(Q, N, K, num_cu, s)
                cuts.append(s)
            except JegalError:
                print(f"Q={Q}: slices={s} is refused (lists beyond the cap): left out", flush=True)
        names = (["baseline/grouped"] if base else []) + ["grouped", "search_f32", "search_f16"] + [f"search_f32_s{s}" for s in cuts]
        outs = {n: (torch.empty((Q, K), dtype=torch.int32, device="cuda"), torch.empty((Q, K), dtype=torch.float32, device="cuda")) for n in names}

        def run(name):
            i, s = outs[name]
            if name == "baseline/grouped":
                rc = base[0].jg_sim_topk_grouped(base[1], P(q), P(g32), Q, N, D, K, P(off), C, 0, 0, P(i), P(s))
            elif name == "grouped":
                rc = lib.jg_sim_topk_grouped(h, P(q), P(g32), Q, N, D, K, P(off), C, 0, 0, P(i), P(s))
            else:
                f16 = name == "search_f16"
                forced = int(name.rsplit("_s", 1)[1]) if "_s" in name else 0
                rc = lib.jg_sim_search(h, P(q), Q, P(g16 if f16 else g32), int(f16), N, D, K, P(off), C, 0, 0, forced, P(i), P(s))
            assert rc == 0, (name, rc)

        for _ in range(args.warmup):
            for n in names:
                run(n)
        torch.cuda.synchronize()
        times = {n: [] for n in names}
        for _ in range(args.iters):
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
        yard = np.asarray(times["grouped"])
        case = {"plan (slices, rows per slice, list bytes)": list(search_plan(Q, N, K, num_cu)), "workgroups_of_grouped": -(-Q // 64)}
        for n in names:
            case[n] = stats(times[n])
            r = np.asarray(times[n]) / yard
            case[n]["over_grouped"] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}
        same = lambda a, b: bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
        case["search_f32_equals_grouped"] = all(same(outs[n], outs["grouped"]) for n in names if n.startswith("search_f32"))
        if base:
            case["grouped_equals_baseline"] = same(outs["grouped"], outs["baseline/grouped"])
        wide = (torch.empty_like(outs["grouped"][0]), torch.empty_like(outs["grouped"][1]))
        assert lib.jg_sim_topk_grouped(h, P(q), P(g16.float()), Q, N, D, K, P(off), C, 0, 0, P(wide[0]), P(wide[1])) == 0
        case["search_f16_equals_grouped_on_widened_rows"] = same(outs["search_f16"], wide)
        case["search_f16_clips_equal_to_f32_share"] = float((torch.div(outs["search_f16"][0], T, rounding_mode="floor")
                                                             == torch.div(outs["grouped"][0], T, rounding_mode="floor")).float().mean())
        res["cases"][f"Q={Q}"] = case
        print(f"Q={Q}: " + json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if base:
        base[0].jg_destroy.argtypes = [ctypes.c_void_p]
        base[0].jg_destroy(base[1])
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
