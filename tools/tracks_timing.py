"""Time jg_jegal_gesture_tracks against the only way to embed a long track without it: the same spans, cut and padded by the caller,
through jg_jegal_gestures as one (n_windows, span_max) batch with a key mask (the caller then keeps the core rows).  Both on HIP events
around a window of calls on the engine's stream, alternating, after a warm-up of both shapes; the batch side is timed WITHOUT the
gathering of its input and the stripping of its output.  Seeded synthetic weights (timing does not depend on the weights' values).

    python tools/tracks_timing.py [--iters 10] [--repeats 3] [--precision 5]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("one track of 8192 frames", [8192]), ("64 tracks of 1000 frames", [1000] * 64)]


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--min_ms", type=float, default=500.0, help="shortest timed window; the calls per window grow to fill it")
    p.add_argument("--win", type=int, default=120)
    p.add_argument("--ctx", type=int, default=50)
    p.add_argument("--precision", type=int, default=None)
    args = p.parse_args()
    from jegal_amd import synth
    from jegal_amd._lib import Engine
    from jegal_amd.jegal import JEGAL
    eng = Engine(0, precision=args.precision)
    JEGAL(engine=eng).load_state_dict(synth.jegal_state_dict())
    for name, lengths in CASES:
        rows = sum(lengths)
        table, span_max = eng.track_windows(lengths, args.win, args.ctx)
        nw = len(table)
        feats = torch.randn((rows, 1024), device=eng.device, generator=torch.Generator(eng.device).manual_seed(rows))
        # the caller-side batch: span rows gathered, zero padded, with their mask
        idx = torch.zeros((nw, span_max), dtype=torch.long)
        mask = torch.zeros((nw, span_max))
        for w, (first, length, _, _) in enumerate(table.tolist()):
            idx[w, :length] = torch.arange(first, first + length)
            mask[w, :length] = 1
        mask = mask.to(eng.device)
        batch = feats[idx.to(eng.device)] * mask[:, :, None]

        def tracks():
            return eng.jegal_gesture_tracks(feats, lengths, win=args.win, ctx=args.ctx, align=True)

        def padded():
            return eng.jegal_gestures(batch, mask, align=True)

        a, b = tracks(), padded()
        core = torch.cat([b[w, coff:coff + clen] for w, (_, _, coff, clen) in enumerate(table.tolist())])
        diff = float((a - core).norm() / core.norm())
        for _ in range(2):
            tracks(), padded()
        torch.cuda.synchronize()
        iters = max(args.iters, int(np.ceil(args.min_ms / timed_ms(padded, 3))))          # a timed window of at least min_ms
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(timed_ms(tracks, iters))
            tb.append(timed_ms(padded, iters))
        fmt = lambda v: "/".join(f"{x:.2f}" for x in v)
        print(f"{name} (win {args.win}, ctx {args.ctx}: {nw} windows x {span_max} = {nw * span_max} window rows for {rows} track rows, precision mode "
              f"{eng.precision}):")
        print(f"  jg_jegal_gesture_tracks   {fmt(ta)} ms per call ({args.repeats} windows of {iters} calls)  median {np.median(ta):.2f} ms = "
              f"{rows / np.median(ta) * 1e3:,.0f} track rows/s")
        print(f"  padded jg_jegal_gestures  {fmt(tb)} ms per call  median {np.median(tb):.2f} ms = {rows / np.median(tb) * 1e3:,.0f} track rows/s"
              f"   ratio {np.median(tb) / np.median(ta):.3f}")
        print(f"  core rows of the two: rel-L2 {diff:.2e}; workspace {eng.workspace_bytes() / 2**20:.0f} MiB")
    eng.close()


if __name__ == "__main__":
    main()
