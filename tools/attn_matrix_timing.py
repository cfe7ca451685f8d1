"""Time jg_attn_matrix next to jg_spot on BASELINE config 5 (synth.planted_spotting(1238, 4000): 4000 clips of 150 frames x 30 words,
device-resident and concatenated), plus one clip of 8192 frames x 64 words (the frame split).  GPU only, no fallback.
Each iteration runs jg_spot, jg_attn_matrix with A == NULL and jg_attn_matrix with the matrix back to back, every call between its own
pair of device events, so the variants alternate in one process and every iteration is one comparison pair.
Traffic and FLOPs come from the shapes: reads (sum T + sum W) * D * 4 bytes, writes sum W*T * 4 bytes (the matrix form only),
2 * sum T*W * D FLOP; roofs 8 TB/s and 157 TFLOP/s (fp32 MFMA); share = the larger of the two bounds over the measured time.
  python tools/attn_matrix_timing.py [--iters 60] [--clips 4000] [--out profiles/attn_matrix_timing.json]"""
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

HBM_BPS, MFMA32_FLOPS = 8.0e12, 157.0e12
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def bounds(sum_t, sum_w, sum_wt, d, with_matrix):
    rd, wr, fl = (sum_t + sum_w) * d * 4, sum_wt * 4 if with_matrix else 0, 2 * sum_wt * d
    t_mem, t_flop = (rd + wr) / HBM_BPS, fl / MFMA32_FLOPS
    return {"read_bytes": rd, "write_bytes": wr, "flop": fl, "bound": "memory" if t_mem >= t_flop else "compute",
            "bound_ms": 1e3 * max(t_mem, t_flop)}


def summarise(ms, b):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return dict(b, median_ms=med, min_ms=float(ms.min()), max_ms=float(ms.max()), share_of_bound=b["bound_ms"] / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clips", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_matrix_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_matrix_timing needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng._bind_stream()
    lib, h = eng.lib, eng.h

    def clips(gest, cont):
        T, W = np.array([x.shape[0] for x in gest]), np.array([x.shape[0] for x in cont])
        d = dict(g=torch.from_numpy(np.concatenate(gest)).cuda(), c=torch.from_numpy(np.concatenate(cont)).cuda(), n=len(gest), T=T, W=W)
        d["go"] = torch.as_tensor(np.concatenate([[0], np.cumsum(T)]).astype(np.int32), device="cuda")
        d["co"] = torch.as_tensor(np.concatenate([[0], np.cumsum(W)]).astype(np.int32), device="cuda")
        d["ao"] = torch.as_tensor(np.concatenate([[0], np.cumsum(T * W)])[:-1].astype(np.int64), device="cuda")
        d["A"] = torch.empty(int((T * W).sum()), dtype=torch.float32, device="cuda")
        d["bf"] = torch.empty(int(W.sum()), dtype=torch.int32, device="cuda")
        d["bs"] = torch.empty(int(W.sum()), dtype=torch.float32, device="cuda")
        return d

    gest, cont, _, targets = synth.planted_spotting(1238, args.clips)
    big = clips(gest, cont)
    tg = torch.as_tensor(np.asarray(targets, np.int32), device="cuda")
    pred = torch.empty(big["n"], dtype=torch.int32, device="cuda")
    score = torch.empty(big["n"], dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(0)
    long = clips([rng.standard_normal((8192, 512)).astype(np.float32)], [rng.standard_normal((64, 512)).astype(np.float32)])

    def attn(d, with_matrix):
        rc = lib.jg_attn_matrix(h, P(d["g"]), P(d["c"]), P(d["go"]), P(d["co"]), d["n"], 512, int(d["T"].max()), 0.07, 1,
                                P(d["A"]) if with_matrix else None, P(d["ao"]) if with_matrix else None, P(d["bf"]), P(d["bs"]))
        assert rc == 0, lib.jg_last_error(h)

    def spot():
        rc = lib.jg_spot(h, P(big["g"]), P(big["c"]), P(big["go"]), P(big["co"]), P(tg), big["n"], 512, 0.07, P(pred), P(score))
        assert rc == 0, lib.jg_last_error(h)

    variants = [("jg_spot", spot), ("attn_matrix_null", lambda: attn(big, False)), ("attn_matrix_full", lambda: attn(big, True)),
                ("attn_matrix_full_8192x64", lambda: attn(long, True))]
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
    # the two entries agree on the target words (same arg-max; jg_spot's own summation order in the score)
    co = big["co"].cpu().numpy()[:-1] + np.asarray(targets)
    same = bool(np.array_equal(big["bf"].cpu().numpy()[co], pred.cpu().numpy()))
    st, sw, swt = int(big["T"].sum()), int(big["W"].sum()), int((big["T"] * big["W"]).sum())
    res = {"input": f"synth.planted_spotting(1238, {args.clips}): {args.clips} clips x 150 frames x 30 words, D = 512", "iters": args.iters,
           "roofs": {"hbm_bytes_per_s": HBM_BPS, "fp32_mfma_flop_per_s": MFMA32_FLOPS},
           "jg_spot": summarise(times["jg_spot"], bounds(st, sw, swt, 512, False)),
           "attn_matrix_null": summarise(times["attn_matrix_null"], bounds(st, sw, swt, 512, False)),
           "attn_matrix_full": summarise(times["attn_matrix_full"], bounds(st, sw, swt, 512, True)),
           "attn_matrix_full_8192x64": summarise(times["attn_matrix_full_8192x64"], bounds(8192, 64, 8192 * 64, 512, True)),
           "target_frames_equal_jg_spot": same}
    ratios = np.asarray(times["jg_spot"]) / np.asarray(times["attn_matrix_null"])
    res["spot_over_null"] = {"median": float(np.median(ratios)), "min": float(ratios.min()), "max": float(ratios.max()),
                             "null_faster_in_every_pair": bool((ratios > 1).all())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0 if res["spot_over_null"]["null_faster_in_every_pair"] else 1


if __name__ == "__main__":
    sys.exit(main())
