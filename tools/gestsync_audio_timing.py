"""Time GestSync's audio stream and the offset search on device-resident inputs.  GPU only, no fallback.
  jg_gestsync_audio_clip   32 clips x 150 windows (mel (32, 600, 80)): per call between two device events, and per stage with the
                           engine's stage profile; beside it the FLOP count of the shapes (as computed: channels padded to 256 / 512;
                           and unpadded) and the bytes of the activations, and jg_gestsync_clip (the video stream) for the same clips
  jg_sync_offset           4000 clips x 150 x 1024 rows per stream, R = 15, against the bytes that must be read once over 8 TB/s
  jg_sync_offset_windows   alternated with jg_sync_offset in the same loop, on the same device-resident rows (win = 0, the band in the
                           workspace: the two entries then give the same bits): (a) ONE clip of 8192 x 1024 rows at R = 15 and R = 64 -- one
                           workgroup for jg_sync_offset, 256 row blocks for the band grid; (b) 4000 clips x 150 rows at R = 15, where the
                           band is an extra 74 MB write and read.  And what only the new entry does: (a) with win = 125, hop = 25, and one
                           track of 2^17 rows (win = 0; win = 125, hop = 25)
Every iteration runs the variants back to back, each between its own pair of events.
  python tools/gestsync_audio_timing.py [--iters 10] [--out profiles/gestsync_audio_timing.json]"""
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

HBM_BYTES_PER_S = 8.0e12
PTR = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
B, T, TM = 32, 150, 600


def summarise(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def window_flops(padded):
    """2 x multiply-adds of one window: conv1 as computed (39 x 49 conv outputs under the pool, each pooled output recomputing its 9), the
    implicit GEMMs over M x N x K, the three Linears"""
    c2o, c3o = (256, 512) if padded else (192, 384)
    layers = [(19 * 24 * 9 if padded else 39 * 49, 64, 9), (19 * 12, c2o, 9 * 64), (45, c3o, 9 * c2o), (45, 256, 9 * c3o), (45, 256, 9 * 256),
              (1, 512, 2048), (1, 512, 512), (1, 1024, 512)]
    return 2.0 * sum(m * n * k for m, n, k in layers)


def window_bytes():
    """fp16 activations written and read once each + the window's own 8000 fp32 values + the fp32 row out"""
    acts = 19 * 24 * 64 + 19 * 12 * 256 + 45 * 256 + 45 * 512 + 45 * 256 + 45 * 256 + 8 * 256 + 512 + 512
    return 2 * 2 * acts + 4 * 8000 + 4 * 1024


def sync_windows_variants(eng, vid, aud, gen, N, D):
    """[(name, callable, description)]: jg_sync_offset and jg_sync_offset_windows on the same rows.  vid / aud: the 4000 x 150 rows of the
    batch case; their first 8192 rows are the one long clip; the 2^17-row track is made here."""
    LONG, HUGE = 8192, 1 << 17
    hv = torch.randn((HUGE, D), generator=gen, device="cuda")
    ha = hv + 0.5 * torch.randn((HUGE, D), generator=gen, device="cuda")
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32), device="cuda")
    out = []

    def old(name, v, a, rows, clips, R, what):
        off = i32(np.arange(clips + 1) * rows)
        curve = torch.empty((clips, 2 * R + 1), device="cuda")
        offset, conf = torch.empty(clips, dtype=torch.int32, device="cuda"), torch.empty(clips, device="cuda")

        def fn():
            rc = eng.lib.jg_sync_offset(eng.h, PTR(v), PTR(off), PTR(a), PTR(off), clips, D, R, 1, PTR(curve), PTR(offset), PTR(conf))
            assert rc == 0, eng.lib.jg_last_error(eng.h)
        out.append((name, fn, dict(what, entry="jg_sync_offset", result=(offset, conf, curve))))

    def new(name, v, a, rows, clips, R, win, hop, what):
        n_win = int(Engine.sync_window_counts([rows], win, hop)[0])
        off, woff = i32(np.arange(clips + 1) * rows), i32(np.arange(clips + 1) * n_win)
        curve = torch.empty((clips * n_win, 2 * R + 1), device="cuda")
        offset, conf = torch.empty(clips * n_win, dtype=torch.int32, device="cuda"), torch.empty(clips * n_win, device="cuda")

        def fn():
            rc = eng.lib.jg_sync_offset_windows(eng.h, PTR(v), PTR(off), clips, clips * rows, rows, PTR(a), PTR(off), clips, None, D, R, 1, win, hop,
                                                PTR(woff), n_win, None, PTR(curve), PTR(offset), PTR(conf))
            assert rc == 0, eng.lib.jg_last_error(eng.h)
        out.append((name, fn, dict(what, entry="jg_sync_offset_windows", win=win, hop=hop, windows_per_clip=n_win,
                                   band_bytes=4 * clips * rows * (2 * R + 1), result=(offset, conf, curve))))

    for R in (15, 64):
        what = dict(case=f"a_R{R}", input=f"1 clip x {LONG} rows x {D}, R = {R}")
        old(f"a_R{R}_jg_sync_offset", vid, aud, LONG, 1, R, what)
        new(f"a_R{R}_jg_sync_offset_windows", vid, aud, LONG, 1, R, 0, 1, what)
    what = dict(case="b", input=f"{N} clips x 150 rows x {D}, R = 15")
    old("b_jg_sync_offset", vid, aud, 150, N, 15, what)
    new("b_jg_sync_offset_windows", vid, aud, 150, N, 15, 0, 1, what)
    new("a_R15_win125_hop25", vid, aud, LONG, 1, 15, 125, 25, dict(case="a_timeline", input=f"1 clip x {LONG} rows x {D}, R = 15"))
    new("track_2p17_one_window", hv, ha, HUGE, 1, 15, 0, 1, dict(case="track_2p17", input=f"1 track x {HUGE} rows x {D}, R = 15"))
    new("track_2p17_win125_hop25", hv, ha, HUGE, 1, 15, 125, 25, dict(case="track_2p17_timeline", input=f"1 track x {HUGE} rows x {D}, R = 15"))
    return out


def sync_windows_report(times, cases):
    info = {name: what for name, _, what in cases}
    rep = {}
    for name, what in info.items():
        rep[name] = dict({k: v for k, v in what.items() if k != "result"}, per_call=summarise(times[name]))
    for case in ("a_R15", "a_R64", "b"):
        o, n = f"{case}_jg_sync_offset", f"{case}_jg_sync_offset_windows"
        # the two entries promise the same bits for one window over all rows
        for x, y in zip(info[o]["result"], info[n]["result"]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), case
        a, b = np.asarray(times[o]), np.asarray(times[n])
        rep[case + "_old_over_new"] = {"median_of_ratios": float(np.median(a / b)), "min": float((a / b).min()), "max": float((a / b).max())}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sync_clips", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gestsync_audio_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gestsync_audio_timing needs the GPU: there is nothing to time without it")
    eng = Engine(0)
    eng.load_tensors(synth.gestsync_state_dict())
    eng.finalize(9)
    gen = torch.Generator(device="cuda").manual_seed(4242)
    mel = torch.randn((B, TM, 80), generator=gen, device="cuda")
    frames = torch.from_numpy(synth.synth_frames(5, 1, T)).to(eng.device).expand(B, -1, -1, -1, -1).contiguous()
    N, D, R = args.sync_clips, 1024, 15
    vid = torch.randn((N * T, D), generator=gen, device="cuda")
    aud = vid + 0.5 * torch.randn((N * T, D), generator=gen, device="cuda")
    off = torch.as_tensor((np.arange(N + 1) * T).astype(np.int32), device="cuda")
    curve = torch.empty((N, 2 * R + 1), device="cuda")
    offset, conf = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, device="cuda")

    def sync():
        rc = eng.lib.jg_sync_offset(eng.h, PTR(vid), PTR(off), PTR(aud), PTR(off), N, D, R, 1, PTR(curve), PTR(offset), PTR(conf))
        assert rc == 0, eng.lib.jg_last_error(eng.h)

    variants = [("jg_gestsync_audio_clip", lambda: eng.gestsync_audio_clip(mel, T)), ("jg_gestsync_clip", lambda: eng.gestsync_clip(frames)),
                ("jg_sync_offset", sync)]
    windows_cases = sync_windows_variants(eng, vid, aud, gen, N, D)
    variants += [(name, fn) for name, fn, _ in windows_cases]
    eng._bind_stream()
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
    assert int((offset == 0).sum()) == N, "the planted offset 0 was not found everywhere"
    # per stage: every launch between two events (the launches no longer run back to back: a split of the time, not a second timing)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(args.iters):
        eng.gestsync_audio_clip(mel, T)
    stages = {k: {"ms_per_call": ms / args.iters, "launches_per_call": n // args.iters} for k, (ms, n) in eng.profile_get().items() if n}
    eng.profile(False)
    a = summarise(times["jg_gestsync_audio_clip"])
    windows = B * T
    once = 4.0 * D * 2 * N * T
    s = summarise(times["jg_sync_offset"])
    res = {"audio_clip": {"input": f"{B} clips x {T} windows, mel ({B}, {TM}, 80), synthetic gauss weights, default precision mode",
                          "iters": args.iters, "per_call": a, "per_stage": stages,
                          "gflop_per_window_unpadded": window_flops(False) / 1e9, "gflop_per_window_as_computed": window_flops(True) / 1e9,
                          "tflops_as_computed": window_flops(True) * windows / (a["median_ms"] * 1e-3) / 1e12,
                          "activation_bytes_per_window": window_bytes(),
                          "memory_bound_ms": window_bytes() * windows / HBM_BYTES_PER_S * 1e3,
                          "video_stream_same_clips": summarise(times["jg_gestsync_clip"])},
           "sync_offset": {"input": f"{N} clips x {T} rows x {D} per stream, R = {R}, planted at 0", "per_call": s, "bytes_read_once": once,
                           "hbm_bytes_per_s": HBM_BYTES_PER_S, "memory_bound_ms": once / HBM_BYTES_PER_S * 1e3,
                           "entry_over_memory_bound": s["median_ms"] / (once / HBM_BYTES_PER_S * 1e3)}}
    res["sync_offset_windows"] = sync_windows_report(times, windows_cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
