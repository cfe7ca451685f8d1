"""Benchmark: clips/s of JEGAL gesture-embedding extraction (BASELINE.json metric).

Workload (BASELINE.json configs[1]): per GPU a batch of 32 synthetic clips of
150 frames x 270x480x3 uint8 (face rows zeroed), resident in HBM; one step = frames -> GestSync
(conv stack de-duplicated over windows, transformer, ff_vid, mean) -> JEGAL gesture encoder ->
align MLP -> L2-normalise -> (32,150,512).  Weak scaling: every rank has its own 32 clips, no
collective on the data path.

`value` is measured with the engine's default scheduling: every batch runs as two parts on two internal HIP streams
(option dual_stream, bit-identical results).

A plain run does only what the headline needs: set-up, warm-up, the timed steps, --dump-outputs, the JSON line.  --full
measures everything else after the timed loop, in the same process: the `roofline*` objects and `stage_ms_per_step` (HIP events
around the kernels of steps on ONE stream: a kernel's roofline is a property of the kernel running alone), the secondary
measurements (--no-extras leaves them out: live parity against the fp32 audit engine, dense / mask-jitter / sustained /
`single_stream` loops, the config-4 retrieval evaluation -- seed-1237 gallery of 10 000 clips, queries sharded ceil(N/G) per rank,
gallery assembled by an all-gather: RCCL over xGMI -- and config-5 spotting, whose results must equal the single-rank ones,
config 3, the PCIe-inclusive legs, the other precision modes in fresh child processes) and the CPU baseline (--no-cpu-baseline
leaves it out).

Usage: python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full [--no-extras] [--no-cpu-baseline]]
  --dump-outputs DIR: rank 0 writes what the LAST timed step returned (the (clips,150,512) fp32 gesture embeddings) to
  DIR/gesture_embeddings.npy; the inputs are seeded, so two builds run with the same arguments can be compared output for output.
  N > 1 without a torchrun environment: this process starts N fresh rank processes itself (it makes no GPU
  call before or after doing so) and relays rank 0's JSON line.  Under `python -m torch.distributed.run
  --nproc-per-node N bench.py --gpus N ...` the ranks come from the environment; WORLD_SIZE != N is an error.
Prints ONE JSON line (rank 0).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CLIPS, FRAMES = 32, 150
DUMP_MAX_BYTES = 64 << 20          # --dump-outputs: larger outputs are cut to a seeded sample of whole clips
# ---- algorithmic work per clip (never padded K or tile waste).  SURVEY counts 170 window-de-duplicated
# conv positions per 150-frame clip; the engine evaluates the 154 DISTINCT ones (positions 0..8 and T+11..T+19 of the
# edge-padded clip see five copies of one frame), and every utilisation figure below is priced on those 154.
POS_SURVEY, POS_EXEC = 170, 154
CONV1_GFLOP_PER_CLIP = POS_EXEC * 13904 * 64 * 735 * 2 / 1e9                       # 201.5
CONV_REST_GFLOP_PER_CLIP = (333.8 - 222.4) * POS_EXEC / POS_SURVEY                 # conv2..fc6: 100.9
CONV2_GFLOP_PER_CLIP = 51.5 * POS_EXEC / POS_SURVEY                                # 46.7 of the 100.9; rows read from the const chain are not counted
CONV3_GFLOP_PER_CLIP = 19.1 * POS_EXEC / POS_SURVEY
CONV4_GFLOP_PER_CLIP = 20.1 * POS_EXEC / POS_SURVEY
CONV5_GFLOP_PER_CLIP = 20.1 * POS_EXEC / POS_SURVEY
LINEAR_GFLOP_PER_CLIP = 131.1      # GestSync transformer + ff_vid (124.7) + JEGAL gesture + align (6.4)
# The synthetic clips carry the reference's face mask (rows 0..109 zero).  conv1 skips all-zero
# input tiles: 8 of the 22 row tiles of every strip (input rows 12*rt .. 12*rt+15 <= 109).  The roofline prices the
# kernel on the FLOPs it EXECUTES; the same launch is timed once more on frames without a zero row (`dense_input`).
CONV1_EXECUTED_TILE_FRACTION = 14.0 / 22.0
MFMA_PEAK_TFLOPS = 2500.0          # dense fp16/bf16 (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0
# algorithmic HBM bytes of the conv stack per clip (uint8 input): 154 x 5... the u8 frames are read once
# (150 x 388.8 KB = 58.3 MB), every inter-layer activation is written once and read once in fp16.
CONV_ALGO_BYTES_PER_CLIP = (FRAMES * 270 * 480 * 3 +
                            2 * 2 * POS_EXEC * (43 * 78 * 64 + 20 * 37 * 128 + 10 * 19 * 256 + 2 * 10 * 10 * 256 + 4 * 4 * 256) +
                            4 * POS_EXEC * 512)
CONV1_ALGO_BYTES_PER_CLIP = FRAMES * 270 * 480 * 3 + 2 * POS_EXEC * 43 * 78 * 64


def load_traffic():
    """Per-launch HBM traffic of the dominant kernel from the committed counter passes (profiles/r2_pmc_summary.json,
    written by tools/pmc_summary.py from separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` runs of this
    command).  None when the summary is absent."""
    for name in ("r6_pmc_summary.json", "r5_pmc_summary.json", "r4_pmc_summary.json", "r3_pmc_summary.json", "r2_pmc_summary.json"):          # the newest committed counter passes
        p = os.path.join(ROOT, "profiles", name)
        if os.path.exists(p):
            break
    else:
        return None, "no committed counter summary (profiles/r3_pmc_summary.json)"
    d = json.load(open(p))
    k = d.get("conv1_direct_kernel")
    if not k:
        return None, f"conv1_direct_kernel missing from profiles/{name}"
    return k["hbm_bytes_per_launch"], f"profiles/{name}: " + k.get("note", "")


def load_sq_counters():
    """SQ / GRBM counters of the dominant kernel from the committed passes (profiles/r4_sq_summary.json, written by tools/sq_summary.py
    from `rocprofv3 --pmc` runs of this command: tools/profile_sq.sh): MFMA-pipe busy fraction of the kernel's cycles, the clock
    GRBM_GUI_ACTIVE implies for the dispatch, LDS bank-conflict share.  None when no summary is committed."""
    for name in ("r6_sq_summary.json", "r5_sq_summary.json", "r4_sq_summary.json", "r4a_sq_summary.json"):
        p = os.path.join(ROOT, "profiles", name)
        if os.path.exists(p):
            k = json.load(open(p)).get("conv1_direct_kernel")
            if k:
                return {"mfma_busy": k.get("mfma_busy_frac"), "clock_ghz_under_pmc": k.get("clock_ghz_under_pmc"),
                        "lds_conflict_frac": k.get("lds_conflict_frac"), "lds_active_frac_of_kernel": k.get("lds_active_frac_of_kernel"),
                        "source": f"profiles/{name} (SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs over GRBM_GUI_ACTIVE / 8 XCDs, one 32-clip launch under rocprofv3 --pmc)"}
    return None


def cpu_baseline(clips_u8, n_windows=96):
    """The reference's algorithm via the oracle port on the host cores, bounded sample: the first `n_windows` windows
    of each of TWO seed-1234 clips through the naive per-window fp32 conv stack (batches of 48 windows, as
    inference_embs.py:499) + the JEGAL gesture branch, extrapolated to whole clips; next to it the window-de-duplicated
    variant of the same port on the same two clips (whole clips)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import jegal_oracle as O
    from jegal_amd import synth
    cores = min(os.cpu_count() or 1, 64)     # more threads than this slows the small JEGAL matmuls down
    torch.set_num_threads(cores)
    gsd = O.tensors(synth.gestsync_state_dict(include_unused=False))
    jsd = O.tensors(synth.jegal_state_dict())
    t_win = t_j = t_dd = 0.0
    n_clips = len(clips_u8)
    with torch.no_grad():
        for clip in clips_u8:
            f01 = torch.from_numpy(clip.astype(np.float32) / np.float32(255.0))
            vol = O.pad_clip(f01).permute(3, 0, 1, 2)
            t0 = time.perf_counter()
            parts = []
            for s0 in range(0, n_windows, 48):
                xs = torch.stack([vol[:, i:i + 25] for i in range(s0, min(n_windows, s0 + 48))])
                parts.append(O.gestsync_forward_vid(gsd, xs).mean(-1))
            feats = torch.cat(parts)
            t_win += time.perf_counter() - t0
            vis = feats[None].repeat(1, FRAMES // n_windows + 1, 1)[:, :FRAMES]
            t0 = time.perf_counter()
            O.l2_normalize(O.jegal_forward_inference(jsd, visual_feats=vis, visual_mask=torch.ones(1, FRAMES)))
            t_j += time.perf_counter() - t0
            t0 = time.perf_counter()
            fd = O.gestsync_clip_feats(gsd, f01)
            O.l2_normalize(O.jegal_forward_inference(jsd, visual_feats=fd[None], visual_mask=torch.ones(1, FRAMES)))
            t_dd += time.perf_counter() - t0
    per_clip = (t_win * FRAMES / n_windows + t_j) / n_clips
    return {"value": 1.0 / per_clip, "unit": "clips/s", "cores": cores, "kind": "port",
            "sample": f"{n_windows} of 150 windows of each of {n_clips} seed-1234 clips through the reference algorithm (naive per-window "
                      f"fp32 conv stack, batches of 48: {t_win:.1f} s) + JEGAL gesture branch ({t_j * 1e3:.0f} ms), extrapolated to whole clips",
            "dedup_variant": {"value": n_clips / t_dd, "unit": "clips/s",
                              "what": f"same port with the conv stack evaluated once per padded-clip position (exact), {n_clips} whole clips in {t_dd:.1f} s"}}


CONTENT_GFLOP_PER_CLIP = 2.15 + 0.52 + 0.02       # JEGAL audio CNN / text encoder (L = 12) / fusion + align (W = 10)


def config3(eng, jg, dev, steps, warmup=3, clips=64):
    """BASELINE configs[2] / SURVEY 8d config 3: B = 64 tri-modal (seeds 1234 / 1235 / 1236) end to end on one GPU:
    frames -> GestSync features -> JEGAL.forward_inference(visual, text, audio) -> L2-normalised (gesture, content).
    Returns clips/s of the whole vta step, per-branch milliseconds (torch events on the engine's stream) and the content
    path's share."""
    import numpy as np
    import torch
    from jegal_amd import synth
    B, T, W = clips, FRAMES, 10
    frames = torch.from_numpy(synth.synth_frames(1234, B, T)).to(dev)
    mel = torch.from_numpy(synth.synth_mel(1235, B, 4 * T)).to(dev)
    states, tmask, ids, offs = synth.synth_text(1236, B, W)
    wbs = synth.synth_boundaries(B, W)
    tbatch = [[w[0] for w in wb] for wb in wbs]
    st_d, tm_d = torch.from_numpy(states).to(dev), torch.from_numpy(tmask.astype(np.float32)).to(dev)
    vmask = torch.ones((B, T), dtype=torch.float32, device=dev)
    pack = (st_d, tm_d, tbatch, ids, offs)

    def step():
        feats = eng.gestsync_clip(frames)
        g, c = jg.forward_inference(visual_feats=feats, visual_mask=vmask, text=pack, audio=mel, word_boundaries=wbs)
        return eng.l2norm(g.reshape(B * T, 512)), eng.l2norm(c.reshape(-1, 512))

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g, c = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(g).all() and torch.isfinite(c).all()

    # per-branch times: the same calls bracketed with events (the host-side segment logic of the word pooling is inside
    # its bracket: it is part of what a caller waits for)
    from jegal_amd.jegal import audio_word_segments, text_word_segments
    names = ["gestsync_features", "jegal_gesture_encoder", "audio_cnn", "text_encoder", "word_pool_fusion", "l2norm"]
    acc = {n: 0.0 for n in names}
    reps = 5
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        feats = eng.gestsync_clip(frames)
        ev[1].record()
        gest = eng.jegal_gestures(feats, vmask, align=True)
        ev[2].record()
        aud = eng.jegal_audio(mel)
        ev[3].record()
        sub = eng.jegal_text(st_d, tm_d)
        ev[4].record()
        t_segs, _ = text_word_segments(ids, offs, tbatch)
        a_segs = audio_word_segments(wbs, aud.shape[1])
        fused = torch.zeros((B, W, 512), dtype=torch.float32, device=dev)
        jg._pool(aud, a_segs, 0, fused, list(range(B)))
        jg._pool(sub, t_segs, 256, fused, list(range(B)))
        cont = eng.fuse_content(fused)
        ev[5].record()
        eng.l2norm(gest.reshape(B * T, 512)); eng.l2norm(cont.reshape(-1, 512))
        ev[6].record()
        torch.cuda.synchronize()
        for i, n in enumerate(names):
            acc[n] += ev[i].elapsed_time(ev[i + 1]) / reps
    content_ms = acc["audio_cnn"] + acc["text_encoder"] + acc["word_pool_fusion"]
    total_ms = dt / steps * 1e3
    return {"workload": "BASELINE configs[2]: synthetic batch=64 vta (frames seed 1234, mel seed 1235 (64,600,80), text states seed 1236 "
                        "(64,12,768), W = 10 words), resident in HBM, one GPU",
            "value": B * steps / dt, "unit": "clips/s", "ms_per_step": total_ms, "steps": steps, "clips": B,
            "branch_ms": {k: round(v, 3) for k, v in acc.items()},
            "content_path_ms": round(content_ms, 3), "content_path_share_of_step": content_ms / total_ms,
            "content_path_mfma_frac": CONTENT_GFLOP_PER_CLIP * B / max(content_ms, 1e-9) / MFMA_PEAK_TFLOPS,
            "note": "branch_ms: torch events around the library calls in a separate pass; content path = audio CNN + text encoder + "
                    "word pooling (host segment logic included) + fusion / align MLPs"}


def dump_outputs(path, emb):
    """Write the timed path's output (numpy float32, clips first) as path/gesture_embeddings.npy.  Over DUMP_MAX_BYTES a fixed
    seeded sample of clips is written instead, with their indices in path/gesture_embeddings_clip_index.npy (float64)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    per_clip = emb[0].nbytes
    if emb.nbytes > DUMP_MAX_BYTES:
        keep = np.sort(np.random.default_rng(0).choice(emb.shape[0], DUMP_MAX_BYTES // per_clip, replace=False))
        emb = emb[keep]
        np.save(os.path.join(path, "gesture_embeddings_clip_index.npy"), keep.astype(np.float64))
    np.save(os.path.join(path, "gesture_embeddings.npy"), np.ascontiguousarray(emb, dtype=np.float32))


def launch_ranks(args, argv, timeout_s=1800.0):
    """--gpus N > 1 outside torchrun: start N fresh rank processes (one per GPU).  This parent never touches the GPU.
    Watchdog: the children are polled; when one exits non-zero (e.g. before the rendezvous) the others are terminated instead
    of being left to wait for the process-group timeout, and the whole job has an overall time limit."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    import threading
    out_chunks = []
    reader = threading.Thread(target=lambda: out_chunks.append(procs[0].stdout.read()), daemon=True)     # rank 0's pipe must keep draining
    reader.start()
    deadline = time.monotonic() + timeout_s
    why = None
    while True:
        rcs = [p.poll() for p in procs]
        if all(rc is not None for rc in rcs):
            break
        if any(rc not in (None, 0) for rc in rcs):
            why = "a rank failed"
        elif time.monotonic() > deadline:
            why = f"no result after {timeout_s:.0f} s"
        if why:
            for p in procs:                      # exactly the processes started above
                if p.poll() is None:
                    p.terminate()
            t_kill = time.monotonic() + 10.0
            for p in procs:
                try:
                    p.wait(timeout=max(0.1, t_kill - time.monotonic()))
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            break
        time.sleep(0.2)
    reader.join(timeout=10.0)
    rcs = [p.returncode for p in procs]
    sys.stdout.write(b"".join(out_chunks).decode())
    sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad or why:
        sys.stderr.write(f"bench.py: {why or 'ranks failed'}; (rank, exit code): {bad}\n")
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=150, help="timed steps (default 150 ~ 2 s of sustained work)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clips", type=int, default=CLIPS)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--precision", type=int, default=5, help="0 fp16, 1 hi+lo Linear weights, 2 hi+lo everywhere, 3 bias-corrected fp16 (opt-in: needs a calibration), 4 bf16 (reported mode: outside the 1e-3 contract), 5 run-time corrected fp16 (the library default: calibration-free), 6 fp32 audit mode (~50 clips/s: use --steps 2 --warmup 1)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed loop also measure the roofline / per-stage figures, the secondary measurements and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary measurements (dense conv1, sustained loop, PCIe stream, retrieval)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only for --oversubscribe)")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="testing aid: allow more ranks than GPUs (ranks share devices round-robin; forces backend gloo; flagged in the output)")
    ap.add_argument("--extra-streams", type=int, default=0, help="robustness experiment: the application owns this many other (used) streams before the engine exists")
    ap.add_argument("--opt", action="append", default=[], help="engine option name=int (tuning experiments)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's embeddings (rank 0) to DIR/gesture_embeddings.npy, float32, at most 64 MB")
    ap.add_argument("--only", default=None, choices=["config3"], help="run just one secondary measurement (for rocprofv3 summaries) and print its object")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        return launch_ranks(args, sys.argv[1:])
    if env_world is not None and int(env_world) != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world}: launch with --nproc-per-node {args.gpus}")

    import jegal_amd
    jegal_amd.want_hw_queues()          # before the first HIP call: the streamed (PCIe-inclusive) leg runs five streams
    import numpy as np
    import torch
    from jegal_amd import synth
    from jegal_amd import dist as jdist

    ndev = torch.cuda.device_count()
    if ndev < 1:
        sys.exit("bench.py: no HIP device visible (jegal_amd has no CPU path)")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > ndev and not args.oversubscribe:
        sys.exit(f"bench.py: --gpus {args.gpus} but only {ndev} device(s) visible (use --oversubscribe only to test the launcher)")
    oversub = args.gpus > ndev
    backend = "gloo" if oversub else args.backend
    local_dev = local % ndev
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    if args.gpus > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            torch.distributed.init_process_group(backend="nccl", device_id=dev)
        else:
            torch.distributed.init_process_group(backend=backend)
    rank, world = jdist.rank(), jdist.world_size()
    assert world == args.gpus, (world, args.gpus)

    from jegal_amd._lib import Engine
    from jegal_amd.gestsync import GestSync
    from jegal_amd.jegal import JEGAL
    extra_streams = []
    for _ in range(args.extra_streams):          # each one used once, so the runtime has bound it to a hardware queue
        st = torch.cuda.Stream(device=local_dev)
        with torch.cuda.stream(st):
            torch.zeros(1, device=f"cuda:{local_dev}").add_(1)
        extra_streams.append(st)
    torch.cuda.synchronize(local_dev)
    eng = Engine(local_dev, precision=args.precision)
    eng.set_chunk(args.chunk)
    for o in args.opt:
        k, v = o.split("=")
        eng.set_option(k, int(v))
    GestSync(engine=eng).load_state_dict(synth.gestsync_state_dict(include_unused=False))
    jg_model = JEGAL(engine=eng).load_state_dict(synth.jegal_state_dict())
    if args.only == "config3":
        print(json.dumps({"config3": config3(eng, jg_model, dev, max(3, min(args.steps, 20)))}))
        return

    frames_host = synth.synth_frames(1234 + rank, args.clips, FRAMES)
    frames = torch.from_numpy(frames_host).to(dev)
    out = torch.empty((args.clips, FRAMES, 512), dtype=torch.float32, device=dev)

    def sync_all():
        torch.cuda.synchronize()
        jdist.barrier()
        torch.cuda.synchronize()

    def timed_loop(n, src=None, engine=None):
        src = frames if src is None else src
        engine = eng if engine is None else engine
        sync_all()
        t0 = time.perf_counter()
        for _ in range(n):
            engine.extract_gesture(src, out)
        sync_all()
        mine = time.perf_counter() - t0
        tmax = torch.tensor([mine], dtype=torch.float64, device=dev)
        jdist.all_reduce_max(tmax)
        per_rank, _ = jdist.all_gather_rows(torch.tensor([[mine]], dtype=torch.float64, device=dev))      # a straggler shows up here
        timed_loop.per_rank_s = [float(v) for v in per_rank.flatten().cpu()]
        return float(tmax.item())

    for _ in range(args.warmup):
        eng.extract_gesture(frames, out)
    dt = timed_loop(args.steps)
    per_rank_ms = [v / args.steps * 1e3 for v in timed_loop.per_rank_s]
    assert torch.isfinite(out).all(), "non-finite embeddings"
    # the measurements below reuse `out`: keep the last timed step's result now
    timed_out = out.cpu().numpy() if args.dump_outputs and rank == 0 else None

    # ---- --full: per-kernel timing with HIP events on the launch stream (dominant kernel: conv1)
    # (1) the dominant kernel alone: only the conv1 launch carries events, the rest of the step runs back to back as in the
    # timed loop; (2) every launch bracketed, for the per-stage table (each bracket adds ~10 us of idle time around its launch).
    # Each block starts with untimed steps: the all-reduce / host work since the timed loop left the GPU idle for milliseconds,
    # and the first steps after an idle period run at ramping clocks (the first conv1 launch measured 4.3 ms against 3.5 ms in
    # the loop, rocprofv3 kernel trace of this very command).
    nprof = 5

    # The timed loop runs every batch as two parts on two internal streams (option dual_stream: one part's next kernel fills the
    # partly empty last round of the other's); a kernel's own roofline is a property of the kernel running ALONE, so the
    # profiled steps run on one stream (dual_stream=0) -- there the launch covers all 32 clips and nothing shares the CUs.
    dual = not any(o.replace(" ", "") == "dual_stream=0" for o in args.opt)

    def profiled(only=None, src=None):
        src = frames if src is None else src
        eng.set_option("dual_stream", 0)
        eng.profile(True, only=only)
        for _ in range(3):
            eng.extract_gesture(src, out)
        eng.profile_reset()
        for _ in range(nprof):
            eng.extract_gesture(src, out)
        p = eng.profile_get()
        eng.profile(False)
        eng.set_option("dual_stream", 1 if dual else 0)
        return p

    if args.full:
        c1_ms, c1_n = profiled(only="conv1")["conv1"]
        prof = profiled()
        conv2_rows_skipped = eng.debug_conv2_rowskip()          # min over the positions, of 20 output rows ("conv2_row_skip", bit-identical)
        conv_rows, conv_rows_full = eng.debug_conv_rows()       # output pixels conv2 .. conv5 computed / would compute without the skip

    extras = {}
    extras_on = args.full and not args.no_extras
    if extras_on and rank == 0 and args.precision != 6:
        # Parity of THIS run's embeddings, measured live (round 6): two of the timed clips once more on a JG_PREC_FP32 audit engine (exact-fp32
        # MFMAs, fp32 activations: the reference's CPU arithmetic on the device, itself 1e-6 from the CPU oracle -- tests/test_gpu_audit_fp32.py,
        # and from the cpu_baseline port below on the same clips) and the rel-L2 / max-abs of the timed mode against it
        try:
            from jegal_amd._lib import PREC_FP32
            e32 = Engine(local_dev, precision=PREC_FP32)
            try:
                GestSync(engine=e32).load_state_dict(synth.gestsync_state_dict(include_unused=False))
                JEGAL(engine=e32).load_state_dict(synth.jegal_state_dict())
                eng.extract_gesture(frames, out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref32 = e32.extract_gesture(frames[:2]).double()
                torch.cuda.synchronize()
                t32 = time.perf_counter() - t0
                got = out[:2].double()
                extras["audit"] = {"engine": "JG_PREC_FP32 (audit mode)", "clips": 2,
                                   "gesture_rel_l2": float((got - ref32).norm() / ref32.norm()),
                                   "gesture_max_abs": float((got - ref32).abs().max()), "tolerance": 1e-3,
                                   "audit_clips_per_s": 2.0 / t32}
            finally:
                e32.close()
        except Exception as exc:  # noqa: BLE001
            extras["audit"] = {"error": repr(exc)[:200]}
    if extras_on:
        # the same step on frames with no zero rows (timing only): every conv1 tile is computed
        dense = torch.randint(0, 256, frames.shape, dtype=torch.uint8, device=dev)
        dprof = profiled(only="conv1", src=dense)
        del dense
        extras["dense_ms"], extras["dense_n"] = dprof["conv1"]
        # robustness of the headline to the mask: the same timed loop on (a) clips whose mask height is drawn per
        # frame from 80..140 rows (the reference's rectangle follows the chin; every position skips what ITS frames allow) and
        # (b) clips without any zero row (nothing is skipped anywhere)
        fj = torch.from_numpy(synth.synth_frames(1234 + rank, args.clips, FRAMES, mask_jitter=(80, 140))).to(dev)
        for _ in range(3):
            eng.extract_gesture(fj, out)
        extras["jitter_s"] = timed_loop(args.steps, fj)
        eng.set_option("dual_stream", 0)
        eng.extract_gesture(fj, out)
        extras["jitter_rows"] = eng.debug_conv_rows()
        eng.set_option("dual_stream", 1 if dual else 0)
        del fj
        fd = torch.randint(1, 256, frames.shape, dtype=torch.uint8, device=dev)
        for _ in range(3):
            eng.extract_gesture(fd, out)
        extras["dense_s"] = timed_loop(args.steps, fd)
        del fd
        # sustained rate: whatever K the driver asked for, also run ~2.5 s of back-to-back steps (clocks settle)
        per = dt / max(args.steps, 1)
        n_sus = max(args.steps, int(2.5 / max(per, 1e-4)))
        extras["sustained_steps"], extras["sustained_s"] = n_sus, timed_loop(n_sus)
        if dual:                                # the same loop with every batch on ONE stream, for reference
            eng.set_option("dual_stream", 0)
            for _ in range(3):
                eng.extract_gesture(frames, out)
            extras["single_stream_s"] = timed_loop(args.steps)
            eng.set_option("dual_stream", 1)
        # config 4: sharded retrieval evaluation with the gallery all-gather
        from jegal_amd import metrics as M
        N = 10000
        ge, ce = synth.planted_retrieval(1237, N)
        lo, hi = jdist.shard_range(N)
        q_dev, g_dev = torch.from_numpy(ce[lo:hi]).to(dev), torch.from_numpy(ge[lo:hi]).to(dev)
        M.retrieval_metrics(q_dev, g_dev, engine=eng)                    # warm-up (RCCL connection set-up)
        sync_all()
        t0 = time.perf_counter()
        m_sharded = M.retrieval_metrics(q_dev, g_dev, engine=eng)
        sync_all()
        tm = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        jdist.all_reduce_max(tm)
        extras["retrieval"] = {"n": N, "ms": float(tm.item()) * 1e3, "metrics": m_sharded}
        # config 5: spotting over 4 000 clips (W = 30), clips sharded ceil(N/G) per rank, two counters all-reduced
        NS = 4000
        sg, sc, sb, stg = synth.planted_spotting(1238, NS)
        lo5, hi5 = jdist.shard_range(NS)
        M.spotting_accuracy(sg[lo5:hi5], sc[lo5:hi5], sb[lo5:hi5], stg[lo5:hi5], engine=eng)       # warm-up
        sync_all()
        t0 = time.perf_counter()
        acc5 = M.spotting_accuracy(sg[lo5:hi5], sc[lo5:hi5], sb[lo5:hi5], stg[lo5:hi5], engine=eng)
        sync_all()
        tm5 = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        jdist.all_reduce_max(tm5)
        # the same with the rank's block already on the device (what is left is jg_spot + the host-side window check + the reduction)
        g5 = torch.from_numpy(np.concatenate(sg[lo5:hi5])).to(dev)
        c5d = torch.from_numpy(np.concatenate(sc[lo5:hi5])).to(dev)
        off5 = (M._offsets(sg[lo5:hi5]), M._offsets(sc[lo5:hi5]))
        sync_all()
        t0 = time.perf_counter()
        acc5r = M.spotting_accuracy(g5, c5d, sb[lo5:hi5], stg[lo5:hi5], engine=eng, offsets=off5)
        sync_all()
        tm5r = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        jdist.all_reduce_max(tm5r)
        assert acc5r == acc5
        del g5, c5d
        extras["spotting"] = {"n": NS, "words": 30, "ms": float(tm5.item()) * 1e3, "ms_device_resident": float(tm5r.item()) * 1e3, "accuracy": acc5,
                              "what": "BASELINE configs[4]: seed-1238 planted clips, clips sharded over the ranks, (correct, total) all-reduced; "
                                      "ms includes the host-side concatenation and the pageable upload of the rank's 1.2 GB block, ms_device_resident starts from the concatenated block in HBM"}
        if rank == 0:
            p5, s5 = eng.spot(torch.from_numpy(np.concatenate(sg)), torch.from_numpy(np.concatenate(sc)), M._offsets(sg), M._offsets(sc), stg)
            c5, n5 = M.spotting_counts(p5.cpu().numpy(), s5.cpu().numpy(), sb, stg)
            assert acc5 == 100.0 * c5 / n5, ("sharded spotting accuracy differs from the single-rank result", acc5, c5, n5)
            extras["spotting"]["equals_single_rank"] = True
        del sg, sc
        if rank == 0:
            r_all, t_all = eng.sim_rank(eng.l2norm(torch.from_numpy(ce).to(dev)), eng.l2norm(torch.from_numpy(ge).to(dev)))
            m_single = M.metrics_from_ranks(r_all.cpu().numpy(), t_all.cpu().numpy())
            assert m_single == m_sharded, ("sharded retrieval metrics differ from the single-rank result", m_single, m_sharded)
            extras["retrieval"]["equals_single_rank"] = True
            if world == 1:
                extras["config3"] = config3(eng, jg_model, dev, max(3, min(args.steps, 20)))
            # PCIe-inclusive rate (host-resident clips -> pinned buffers -> H2D under compute -> D2H), never `value`
            if world == 1:
                from jegal_amd.extract import GestureStreamer
                st = GestureStreamer(eng, args.clips, FRAMES)
                for s_ in range(2):
                    st.h_in[s_].numpy()[:] = frames_host
                nb = 6
                for _ in st.run_filled(lambda buf, k: args.clips if k < 2 else 0):
                    pass
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = 0
                for _, emb in st.run_filled(lambda buf, k: args.clips if k < nb else 0):
                    got += emb.shape[0]
                extras["pcie_clips_per_s"] = got / (time.perf_counter() - t0)
                del st
                # the same with only the rows below each clip's mask crossing the link (GestureStreamer(masked=True))
                st = GestureStreamer(eng, args.clips, FRAMES, masked=True)
                for s_ in range(2):
                    for b in range(args.clips):
                        st.packer[s_].add(frames_host[b], 110)
                for _ in st.run_filled(lambda pk, k: args.clips if k < 2 else 0):
                    pass
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got, emb_m = 0, None
                for _, emb in st.run_filled(lambda pk, k: args.clips if k < nb else 0):
                    got += emb.shape[0]
                    emb_m = emb
                extras["pcie_masked_clips_per_s"] = got / (time.perf_counter() - t0)
                extras["pcie_masked_bytes"] = st.packer[0].used
                eng.extract_gesture(frames, out)
                assert np.array_equal(emb_m, out.cpu().numpy()), "masked upload differs from the resident path"
                del st
                # source-resolution upload: the decoder's 228x314 frames (reference samples/sample1.avi, inference_embs.py:255-276
                # resizes them to 270x480 on the host) with their mask rows; mask + resize run on the device in front of the batch's compute (jg_mask_resize_packed)
                SH, SW = 228, 314
                rng_s = np.random.default_rng(4321)
                src = rng_s.integers(0, 256, (args.clips, FRAMES, SH, SW, 3), dtype=np.uint8)
                my_src = int(round(109 * SH / 270.0))                      # the 110-row mask of the synthetic crops at source scale
                st = GestureStreamer(eng, args.clips, FRAMES, source_hw=(SH, SW))
                for s_ in range(2):
                    for b in range(args.clips):
                        st.packer[s_].add(src[b], my_src)
                for _ in st.run_filled(lambda pk, k: args.clips if k < 2 else 0):
                    pass
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got, emb_s = 0, None
                stamps = []
                for _, emb in st.run_filled(lambda pk, k: args.clips if k < nb else 0):
                    got += emb.shape[0]
                    emb_s = emb
                    stamps.append((time.perf_counter() - t0) * 1e3)
                extras["pcie_source_clips_per_s"] = got / (time.perf_counter() - t0)
                print("source-resolution stream: batch completion times (ms) " + " ".join(f"{x:.1f}" for x in stamps), file=sys.stderr)
                extras["pcie_source_bytes"] = st.packer[0].used
                crops = torch.stack([eng.mask_resize(torch.from_numpy(src[b]), [my_src] * FRAMES) for b in range(args.clips)])
                eng.extract_gesture(crops, out)
                torch.cuda.synchronize()
                assert np.array_equal(emb_s, out.cpu().numpy()), "source-resolution upload differs from load_rgb_masked_frames + the resident path"
                extras["pcie_source_hw"] = [SH, SW]
                del st, crops, src
        # The same timed loop in the other precision treatments a driver can select: `value` is the calibration-FREE
        # run-time corrected mode (5: per-clip E[x] from the clip's own rows -- what the CLI drivers give a checkpoint they have never
        # seen); 3 = corrections folded into the biases by a calibration pass (the library default for the seeded weights), 1 = hi+lo
        # Linear weights.  Each mode runs this very script in a FRESH child process (--full --no-extras: weights, warm-up, the timed loop, the
        # bracketed stage table): a second engine inside this process would share the runtime's hardware queues with the streams the
        # measurements above created, and its two lanes then serialise (measured: 13.8 ms instead of 11.9 for mode 3).
        if world == 1:
            extras["precision_modes"] = {}
            for mode, name in ((5, "rc"), (3, "bc"), (1, "w2")):
                if mode == args.precision:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--precision", str(mode), "--full", "--no-extras", "--no-cpu-baseline", "--steps", str(args.steps),
                       "--warmup", str(max(3, args.warmup)), "--clips", str(args.clips), "--chunk", str(args.chunk)]
                for o in args.opt:
                    cmd += ["--opt", o]
                try:
                    cp = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                    d2 = json.loads(cp.stdout.strip().splitlines()[-1])
                    extras["precision_modes"][name] = {"precision_mode": mode, "value": d2["value"], "ms_per_step": d2["ms_per_step"],
                                                       "stage_ms_per_step": d2["stage_ms_per_step"],
                                                       "roofline_linear_gemms_frac": d2["roofline_linear_gemms"]["frac"],
                                                       "roofline_conv1_frac": d2["roofline"]["frac"]}
                except Exception as exc:          # the headline must not depend on a secondary measurement
                    extras["precision_modes"][name] = {"precision_mode": mode, "error": repr(exc)[:200]}
    jdist.barrier()

    if rank == 0:
        clips_total = args.clips * world * args.steps
        value = clips_total / dt
        zskip = not any(o.replace(" ", "") == "conv1_zero_skip=0" for o in args.opt)
        res = {
            "metric": "clips/sec (T=150 frames, 270x480) embedding extraction", "value": value, "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "ms_per_step_per_rank": [round(v, 4) for v in per_rank_ms],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16" if args.precision == 4 else ("f32" if args.precision == 6 else "f16"),
            "data": "synthetic", "full": args.full,
            "config": {"workload": "BASELINE configs[1]: synthetic batch=32 gesture-only (GestSync conv + JEGAL gesture encoder), "
                                   "uint8 150x270x480x3 clips resident in HBM, seeded synthetic weights",
                       "clips_per_gpu": args.clips, "frames": FRAMES, "precision_mode": args.precision, "chunk": args.chunk,
                       "conv1_zero_tile_skip": zskip, "dual_stream": dual,
                       "parallelism": f"clip-sharded x{world}, no data-path collective" + (" (OVERSUBSCRIBED: ranks share GPUs, gloo)" if oversub else "")},
        }
        if args.full:
            c1_avg_s = (c1_ms / max(c1_n, 1)) * 1e-3
            clips_per_launch = args.clips * nprof / max(c1_n, 1)
            exec_frac = CONV1_EXECUTED_TILE_FRACTION if zskip else 1.0
            achieved = CONV1_GFLOP_PER_CLIP * exec_frac * clips_per_launch / c1_avg_s / 1e3 if c1_avg_s > 0 else 0.0
            traffic, traffic_note = load_traffic()
            # executed share of conv2 .. conv5: every position leaves out its own position-independent leading rows (ConvGeom::rowmap)
            cfrac = [conv_rows[l] / conv_rows_full[l] if conv_rows_full[l] else 1.0 for l in range(4)]
            layer_gflop = [CONV2_GFLOP_PER_CLIP, CONV3_GFLOP_PER_CLIP, CONV4_GFLOP_PER_CLIP, CONV5_GFLOP_PER_CLIP]
            conv_rest_exec = CONV_REST_GFLOP_PER_CLIP - sum(g * (1.0 - f) for g, f in zip(layer_gflop, cfrac))
            exec_gflop_clip = CONV1_GFLOP_PER_CLIP * exec_frac + conv_rest_exec + LINEAR_GFLOP_PER_CLIP
            pooled_rows_written = 43 - 2 * max(int(conv2_rows_skipped or 0), 0) if zskip else 43
            exec_bytes_launch = (FRAMES * 270 * 480 * 3 * exec_frac + 2 * POS_EXEC * pooled_rows_written * 78 * 64) * clips_per_launch
            stage = {k: v[0] / nprof for k, v in prof.items()}
            conv_ms = stage["conv1"] + stage["conv1_aux"] + stage["maxpool"] + stage["conv2-fc6+audio_cnn"] + stage["stack_frames"]
            lin_ms = stage["gemm"] + stage["attention"] + stage["layernorm"]
            res.update({
                "roofline": {"bound": "mfma", "kernel": "conv1_direct_kernel (u8 frames -> conv1+BN+ReLU+maxpool, 154 distinct positions/clip)",
                             "achieved": achieved, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / MFMA_PEAK_TFLOPS,
                             "traffic": traffic * clips_per_launch / 32.0 if traffic else None, "traffic_note": traffic_note,
                             # bytes the launch has to move for the work it EXECUTES: the frame rows of the executed input tiles (the all-zero
                             # bands are read by the scan kernel, not by this one) + the pooled rows conv2 will read (conv2's row skip leaves
                             # the first 2 x s2 pooled rows of every position unwritten); `traffic` / this >= 1 is the re-read / write amplification
                             "algorithmic_bytes_per_launch": exec_bytes_launch,
                             "algorithmic_bytes_per_launch_unskipped": CONV1_ALGO_BYTES_PER_CLIP * clips_per_launch,
                             "traffic_over_algorithmic": (traffic * clips_per_launch / 32.0) / exec_bytes_launch if traffic else None,
                             "hbm_frac_of_peak": exec_bytes_launch / c1_avg_s / 1e9 / HBM_PEAK_GBS if c1_avg_s > 0 else None,
                             "launch_ms": c1_avg_s * 1e3, "launches_per_step": c1_n / nprof,
                             "counters": load_sq_counters(),
                             "executed_tile_fraction": exec_frac,
                             "timing_note": "the kernel timed ALONE: these steps run on one stream (dual_stream=0, one launch = all clips); in the timed "
                                            "loop the batch runs as two parts on two streams and its two conv1 launches share the CUs with the other part's kernels",
                             "flops_note": "achieved = EXECUTED algorithmic FLOPs / launch time (HIP events on the launch stream, mean of "
                                           f"{c1_n} launches): all-zero input tiles (the face-mask rows, 8 of 22 row tiles of the synthetic clips) are not counted",
                             # whole path, priced consistently on executed work (154 positions, executed conv1 tiles)
                             "whole_path": {"executed_gflop_per_clip": exec_gflop_clip,
                                            "frac": value / world * exec_gflop_clip / 1e3 / MFMA_PEAK_TFLOPS}},
                # SURVEY 8d asks for BOTH fractions on the conv extractor: algorithmic HBM bytes of the whole conv stack / its time
                "roofline_conv_stack": {"bound": "mfma", "ms_per_step": conv_ms,
                                        "mfma_frac": (CONV1_GFLOP_PER_CLIP * exec_frac + conv_rest_exec) * args.clips / max(conv_ms, 1e-9) / MFMA_PEAK_TFLOPS,
                                        "conv2_rows_skipped_min": conv2_rows_skipped,
                                        "computed_row_fraction": {f"conv{l + 2}": round(cfrac[l], 4) for l in range(4)},
                                        "flops_note": "executed FLOPs: conv1 tiles over all-zero input and the leading conv2 .. conv5 output rows that do "
                                                      "not depend on the position (read from images computed once per weight load) are not counted",
                                        "algorithmic_bytes_per_step": CONV_ALGO_BYTES_PER_CLIP * args.clips,
                                        "achieved_gbs": CONV_ALGO_BYTES_PER_CLIP * args.clips / max(conv_ms, 1e-9) / 1e6,
                                        "hbm_frac": CONV_ALGO_BYTES_PER_CLIP * args.clips / max(conv_ms, 1e-9) / 1e6 / HBM_PEAK_GBS,
                                        "note": "the conv stack is MFMA-bound (620 FLOP/B): the HBM fraction is reported because north_star asks for it, not because it is the roof"},
                # attention + MLP blocks: every Linear GEMM, attention and LayerNorm launch of a step (algorithmic FLOPs only:
                # the hi+lo weight split of precision mode 1 is NOT counted as work)
                "roofline_linear_gemms": {"bound": "mfma", "kernel": "all Linear GEMM + attention + LayerNorm launches of one step",
                                          "achieved": LINEAR_GFLOP_PER_CLIP * args.clips / max(lin_ms, 1e-9), "peak": MFMA_PEAK_TFLOPS,
                                          "unit": "TFLOP/s", "frac": LINEAR_GFLOP_PER_CLIP * args.clips / max(lin_ms, 1e-9) / MFMA_PEAK_TFLOPS,
                                          "ms_per_step": lin_ms, "gemm_only_ms": stage["gemm"], "launches_per_step": prof["gemm"][1] / nprof},
                "stage_ms_per_step": {k: round(v, 3) for k, v in stage.items()},
            })
        if "dense_ms" in extras:
            d1 = extras["dense_ms"] / max(extras["dense_n"], 1) * 1e-3
            da = CONV1_GFLOP_PER_CLIP * clips_per_launch / d1 / 1e3 if d1 > 0 else 0.0
            res["roofline"]["dense_input"] = {"what": "same launch on uniform-noise frames without zero rows (timing only): every tile computed",
                                              "launch_ms": d1 * 1e3, "achieved": da, "frac": da / MFMA_PEAK_TFLOPS}
            jr, jf = extras["jitter_rows"]
            res["value_jitter_mask"] = {"value": args.clips * world * args.steps / extras["jitter_s"], "unit": "clips/s",
                                        "ms_per_step": extras["jitter_s"] / args.steps * 1e3,
                                        "computed_row_fraction": {f"conv{l + 2}": round(jr[l] / jf[l], 4) if jf[l] else 1.0 for l in range(4)},
                                        "what": "the same timed loop on the same clips with the mask height drawn per frame from 80..140 rows "
                                                "(seed fixed; inference_embs.py:264-270 blanks rows 0..y2+15 per frame)"}
            res["value_dense"] = {"value": args.clips * world * args.steps / extras["dense_s"], "unit": "clips/s",
                                  "ms_per_step": extras["dense_s"] / args.steps * 1e3,
                                  "what": "the same timed loop on uniform-noise clips without any zero row: no conv1 tile and no conv2..conv5 row is skipped"}
            res["sustained"] = {"steps": extras["sustained_steps"], "seconds": extras["sustained_s"],
                                "value": args.clips * world * extras["sustained_steps"] / extras["sustained_s"], "unit": "clips/s"}
            if "single_stream_s" in extras:
                res["single_stream"] = {"ms_per_step": extras["single_stream_s"] / args.steps * 1e3,
                                        "value": args.clips * world * args.steps / extras["single_stream_s"], "unit": "clips/s",
                                        "what": "the same timed loop with dual_stream=0 (every batch on one stream); stage_ms_per_step and the roofline objects are measured in this mode"}
            res["retrieval_config4"] = extras["retrieval"]
            res["spotting_config5"] = extras["spotting"]
            if "config3" in extras:
                res["config3"] = extras["config3"]
            if "audit" in extras:
                res["config"]["parity_of_this_run"] = extras["audit"]
            # the driver keeps `config` whole (other top-level keys are reduced to their names): the numbers a reader of the headline needs
            res["config"]["value_is"] = "masked synthetic clips (rows 0..109 zero, BASELINE configs[1]), precision mode JG_PREC_FP16_RC, two lanes"
            res["config"]["same_loop_other_inputs_clips_per_s"] = {"dense_frames_no_zero_row": round(res["value_dense"]["value"], 1),
                                                                   "mask_height_jitter_80_140": round(res["value_jitter_mask"]["value"], 1)}
            if extras.get("precision_modes"):
                res["config"]["same_loop_other_precision_modes_clips_per_s"] = {k: round(v["value"], 1) for k, v in extras["precision_modes"].items() if "value" in v}
            if extras.get("precision_modes"):
                res["precision_modes"] = dict(extras["precision_modes"],
                                              what="the SAME timed loop (same clips, steps, two lanes) in the other precision treatments: `value` above is "
                                                   "JG_PREC_FP16_RC (per-clip run-time correction, calibration-free: the library default and what the "
                                                   "CLI drivers run every checkpoint in); bc = JG_PREC_FP16_BC (corrections folded into the biases by a "
                                                   "calibration pass: opt-in, here with its built-in clips), "
                                                   "w2 = JG_PREC_FP16_W2 (hi+lo Linear weights, calibration-free)")
            if "pcie_clips_per_s" in extras:
                res["pcie_inclusive"] = {"value": extras["pcie_clips_per_s"], "unit": "clips/s",
                                         "what": "host-resident clips -> pinned buffers -> H2D under compute -> embeddings back on the host (GestureStreamer); never `value`"}
            if "pcie_masked_clips_per_s" in extras:
                res["pcie_inclusive"]["masked_upload"] = {
                    "value": extras["pcie_masked_clips_per_s"], "unit": "clips/s", "bytes_per_batch": extras["pcie_masked_bytes"],
                    "bytes_per_batch_dense": args.clips * FRAMES * 270 * 480 * 3, "equals_resident_path": True,
                    "what": "only the rows below each clip's face mask cross the link (GestureStreamer(masked=True)), jg_unpack_masked rebuilds the batch on the device"}
            if "pcie_source_clips_per_s" in extras:
                res["pcie_inclusive"]["source_res"] = {
                    "value": extras["pcie_source_clips_per_s"], "unit": "clips/s", "source_hw": extras["pcie_source_hw"],
                    "bytes_per_batch": extras["pcie_source_bytes"], "bytes_per_batch_dense": args.clips * FRAMES * 270 * 480 * 3,
                    "equals_resident_path": True,
                    "what": "decoder-resolution frames (228x314 as in the reference's samples/sample1.avi), only the source rows below each frame's mask "
                            "cross the link (GestureStreamer(source_hw=...)); face mask + cv2-style bilinear resize to 270x480 on the device "
                            "(jg_mask_resize_packed); bit-identical to load_rgb_masked_frames + the resident path"}
        if args.full and not args.no_cpu_baseline and world == 1:
            res["cpu_baseline"] = cpu_baseline(frames_host[:2])
        else:
            res["cpu_baseline"] = None
        if timed_out is not None:
            dump_outputs(args.dump_outputs, timed_out)
        print(json.dumps(res))
    jdist.barrier()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
