"""Time jg_asd_windows next to the routes that exist without it, on the same device-resident inputs: 4000 scenes x 6 tracks x 150 frames
x 30 words (word j on frames 5 j .. 5 j + 3), D = 512.  GPU only, no fallback.
Modes and their yardsticks:
  clip level       jg_pool_mean twice (tracks, utterances) + torch cosine_similarity + softmax
  win 25 / hop 5   torch unfold(...).mean over the frames, a (windows x words) averaging matrix for q, cosine_similarity, softmax
  win 25 / hop 1   the same
The torch route forms full windows only, so the entry is asked for the same ones ((150 - 25) / hop + 1 per scene).  Each iteration runs
every variant back to back, each call between its own pair of device events, so the variants alternate in one process and every iteration
is one comparison.  The memory bound comes from the shapes: the bytes that must be read once (every gesture and content row) over 8 TB/s.
  python tools/asd_windows_timing.py [--iters 10] [--scenes 4000] [--out profiles/asd_windows_timing.json]"""
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

HBM_BYTES_PER_S = 8.0e12
P, T, W, D, WIN, TEMP = 6, 150, 30, 512, 25, 0.07
PTR = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def summarise(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asd_windows_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("asd_windows_timing needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng._bind_stream()
    lib, h = eng.lib, eng.h
    N = args.scenes
    gen = torch.Generator(device="cuda").manual_seed(1237)
    g = torch.randn((N * P * T, D), generator=gen, device="cuda") / D ** 0.5
    c = torch.nn.functional.normalize(torch.randn((N * W, D), generator=gen, device="cuda"), dim=-1)
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32), device="cuda")
    goff, coff, soff, trk = i32(np.arange(N * P + 1) * T), i32(np.arange(N + 1) * W), i32(np.arange(N + 1) * P), i32(np.arange(N * P))
    ws = i32(np.tile(5 * np.arange(W), N))
    we = i32(np.tile(5 * np.arange(W) + 3, N))
    modes = {"clip_level": (0, 1, 1), "win25_hop5": (WIN, 5, (T - WIN) // 5 + 1), "win25_hop1": (WIN, 1, T - WIN + 1)}
    bufs = {}
    for name, (win, hop, nw) in modes.items():
        bufs[name] = dict(wo=i32(np.arange(N + 1) * nw), po=torch.arange(N, device="cuda", dtype=torch.int64) * (nw * P),
                          prob=torch.empty(N * nw * P, device="cuda"), pred=torch.empty(N * nw, dtype=torch.int32, device="cuda"))

    def entry(name):
        win, hop, nw = modes[name]
        b = bufs[name]
        rc = lib.jg_asd_windows(h, PTR(g), PTR(goff), N * P, PTR(c), PTR(coff), PTR(ws), PTR(we), PTR(trk), PTR(soff), N, D, win, hop,
                                PTR(b["wo"]), PTR(b["po"]), nw, TEMP, PTR(b["prob"]), None, PTR(b["pred"]))
        assert rc == 0, lib.jg_last_error(h)

    route_out = {}

    def clip_route():
        gm = eng.pool_mean(g, goff).view(N, P, D)
        qm = eng.pool_mean(c, coff)
        cos = torch.nn.functional.cosine_similarity(qm[:, None, :], gm, dim=-1)
        route_out["clip_level"] = torch.softmax(cos / TEMP, dim=1)

    avg = {}
    for name, (win, hop, nw) in modes.items():
        if win:
            lo = hop * np.arange(nw)[:, None]
            m = ((5 * np.arange(W)[None] + 3 >= lo) & (5 * np.arange(W)[None] <= lo + win - 1)).astype(np.float32)
            avg[name] = torch.as_tensor(m / m.sum(axis=1, keepdims=True), device="cuda")         # (windows, words): every window has a word

    def window_route(name):
        win, hop, nw = modes[name]
        gw = g.view(N, P, T, D).unfold(2, win, hop).mean(-1)                       # (N, P, windows, D)
        q = torch.matmul(avg[name], c.view(N, W, D))                               # (N, windows, D)
        cos = torch.nn.functional.cosine_similarity(q[:, None], gw, dim=-1)        # (N, P, windows)
        route_out[name] = torch.softmax(cos / TEMP, dim=1).transpose(1, 2)

    variants = []
    for name in modes:
        variants.append((f"jg_asd_windows_{name}", (lambda name=name: entry(name))))
        variants.append((f"route_without_{name}", clip_route if name == "clip_level" else (lambda name=name: window_route(name))))
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
    once = 4.0 * D * (N * P * T + N * W)
    res = {"input": f"{N} scenes x {P} tracks x {T} frames x {W} words, D = {D}, N(0, 1/D) frames, unit-norm words on frames 5j .. 5j+3",
           "iters": args.iters, "bytes_read_once": once, "hbm_bytes_per_s": HBM_BYTES_PER_S, "memory_bound_ms": once / HBM_BYTES_PER_S * 1e3}
    for name, (win, hop, nw) in modes.items():
        a, b = np.asarray(times[f"jg_asd_windows_{name}"]), np.asarray(times[f"route_without_{name}"])
        r = a / b
        prob = bufs[name]["prob"].view(N, nw, P)
        res[name] = {"win": win, "hop": hop, "windows_per_scene": nw, "jg_asd_windows": summarise(a), "route_without": summarise(b),
                     "entry_over_route": {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())},
                     "entry_over_memory_bound": float(np.median(a)) / res["memory_bound_ms"],
                     "max_abs_prob_difference_to_route": float((prob - route_out[name].reshape(N, nw, P)).abs().max())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
