"""Time jg_attn_talk on one talk: a 30 000-frame track with 3 000 words (word j on frames 10 j .. 10 j + 7) at reach 110, D = 512,
device-resident.  GPU only, no fallback.  Yardstick: jg_attn_matrix on the same rows cut into clips of 220 frames, each with the words
that begin inside it (137 clips of about 22 words: what the clip form can say about a talk).  Each iteration runs the variants back to
back, every call between its own pair of device events, so they alternate in one process and every iteration is one comparison.
The two do not compute the same thing -- per frame the talk form's softmax runs over about 23 words in reach, the clip form's over the 22
words of its clip, and the talk form also labels every frame -- so the ratio says what the feature costs, not which kernel is better.
Traffic and FLOPs of the talk form from the shapes: every block of 128 frames reads its 128 frame rows and its candidates' rows
((128 + 2 reach + 8) / 10 of them), and writes its band entries.
  python tools/attn_talk_timing.py [--iters 60] [--out profiles/attn_talk_timing.json]"""
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

P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
T, W, SPAN, STEP, REACH, CLIP, D = 30000, 3000, 8, 10, 110, 220, 512


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_talk_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_talk_timing needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng._bind_stream()
    lib, h = eng.lib, eng.h
    rng = np.random.default_rng(0)
    unit = lambda n: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.standard_normal((n, D)))
    g, c = torch.from_numpy(unit(T)).cuda(), torch.from_numpy(unit(W)).cuda()
    start = np.arange(W, dtype=np.int32) * STEP
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32), device="cuda")
    ws, we, go, co = i32(start), i32(start + SPAN - 1), i32([0, T]), i32([0, W])
    pitch = 2 * REACH + SPAN
    band = torch.empty((W, pitch), dtype=torch.float32, device="cuda")
    bf, bs = torch.empty(W, dtype=torch.int32, device="cuda"), torch.empty(W, dtype=torch.float32, device="cuda")
    fw, fp = torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty(T, dtype=torch.float32, device="cuda")
    # the clip form: frames cut every CLIP, each clip with the words that begin inside it
    cg = np.minimum(np.arange(0, T + CLIP, CLIP), T)
    cg = cg[:int(np.argmax(cg == T)) + 1]
    cw = np.searchsorted(start, cg, side="left")
    n_clips = len(cg) - 1
    cgo, cco = i32(cg), i32(cw)
    cT, cW = np.diff(cg), np.diff(cw)
    ao = torch.as_tensor(np.concatenate([[0], np.cumsum(cT * cW)])[:-1].astype(np.int64), device="cuda")
    A = torch.empty(int((cT * cW).sum()), dtype=torch.float32, device="cuda")
    cbf, cbs = torch.empty(W, dtype=torch.int32, device="cuda"), torch.empty(W, dtype=torch.float32, device="cuda")

    def talk(with_band):
        rc = lib.jg_attn_talk(h, P(g), P(go), 1, T, T, P(c), P(co), W, P(ws), P(we), D, REACH, 0.07, 0, P(band) if with_band else None, pitch,
                              P(bf), P(bs), P(fw), P(fp))
        assert rc == 0, lib.jg_last_error(h)

    def clip(with_matrix):
        rc = lib.jg_attn_matrix(h, P(g), P(c), P(cgo), P(cco), n_clips, D, CLIP, 0.07, 0, P(A) if with_matrix else None,
                                P(ao) if with_matrix else None, P(cbf), P(cbs))
        assert rc == 0, lib.jg_last_error(h)

    variants = [("attn_talk_band", lambda: talk(True)), ("attn_matrix_clips_full", lambda: clip(True)),
                ("attn_talk_no_band", lambda: talk(False)), ("attn_matrix_clips_null", lambda: clip(False))]
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
    blocks = -(-T // 128)
    cand = (128 + 2 * REACH + SPAN) / STEP
    res = {"input": f"one track of {T} frames x {W} words (word j on frames {STEP} j .. {STEP} j + {SPAN - 1}), reach {REACH}, D = {D}, normalize 0",
           "yardstick": f"jg_attn_matrix on the same rows as {n_clips} clips of {CLIP} frames with the words that begin inside each",
           "iters": args.iters,
           "talk_shape": {"blocks_of_128_frames": blocks, "candidates_per_block": cand, "read_bytes": int(blocks * (128 + cand) * D * 4),
                          "band_bytes": int(W * pitch * 4), "flop": int(2 * blocks * 128 * cand * D)},
           "decided_words": int((bf.cpu().numpy() >= 0).sum()), "decided_frames": int((fw.cpu().numpy() >= 0).sum())}
    for name in times:
        res[name] = stats(times[name])
    r = np.asarray(times["attn_talk_band"]) / np.asarray(times["attn_matrix_clips_full"])
    res["talk_band_over_clips_full"] = {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
