"""Launch counts, workspace and output bits of the model graphs (jegal.hip, gestsync.hip, xlmr.hip), for comparing two builds of
libjegal_hip.so after a change to the host code that strings the launches together:

    python tools/model_graph_digest.py [LIB.so] [--golden OUT.json]     (default: jegal_amd/libjegal_hip.so; once per library, each run
                                                                         a fresh process)
    python tools/model_graph_digest.py --compare OLD.jsonl NEW.jsonl

Every entry that runs a transformer or JEGAL graph, on synth.py weights and fixed-seed inputs, in every arithmetic it can run in (the
16-bit modes, the split-operand ends, the fp32 audit stages and audit_jegal_parts), at shapes either side of the 128-row GEMM line and
with B < 8 (no call splits into lanes).  One JSON line per case: the case, the launches per profiling stage (Engine.profile_get), the
workspace bytes and the SHA-256 of the output bytes.  --golden writes the launch counts alone (tests/golden/model_graph_launches.json,
tests/test_gpu_model_graphs.py: counts do not depend on the compiler).  --compare: every case of OLD is in NEW with equal launch counts,
an equal digest and no more workspace."""
import hashlib, json, os, sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import jegal_amd._lib as L
from jegal_amd import synth

GS, JG, XL = 1, 2, 4            # jg_finalize_weights masks
# a handle per set of weights: precision, options set before the weights are finalized, models
CONFIGS = {
    "rc": (L.PREC_FP16_RC, {}, GS | JG | XL),
    "rc_aw": (L.PREC_FP16_RC, {"audit_weights": 1}, GS | JG | XL),
    "w2": (L.PREC_FP16_W2, {}, GS | JG),
    "fp16": (L.PREC_FP16, {}, JG),
    "bf16": (L.PREC_BF16, {}, GS | JG),
    "fp32": (L.PREC_FP32, {}, JG),
    "rc_fold0": (L.PREC_FP16_RC, {"xlmr_fold": 0}, XL),
    "rc_aw_fold0": (L.PREC_FP16_RC, {"audit_weights": 1, "xlmr_fold": 0}, XL),
}
RUNTIME = {"audit_stages": 0, "audit_jegal_parts": 0, "jegal_fp32_ends": 1}       # per-case options and their defaults
GESTURE_SHAPES = ((1, 33), (2, 70))


def engine(config):
    prec, opts, models = CONFIGS[config]
    e = L.Engine(0, precision=prec)
    for k, v in opts.items():
        e.set_option(k, v)
    from jegal_amd.gestsync import GestSync
    from jegal_amd.jegal import JEGAL
    from jegal_amd.xlmr import XLMRoberta
    if models & GS:
        GestSync(engine=e).load_state_dict(synth.gestsync_state_dict(include_unused=False))
    if models & JG:
        JEGAL(engine=e).load_state_dict(synth.jegal_state_dict())
    if models & XL:
        XLMRoberta(engine=e).load_state_dict(synth.xlmr_state_dict())
    return e


def gesture_inputs(B, T, ragged):
    feats = np.random.default_rng(1000 + T).standard_normal((B, T, 1024)).astype(np.float32)
    mask = np.ones((B, T), np.float32)
    if ragged:
        mask[B - 1, 3 * T // 4:] = 0
        feats[B - 1, 3 * T // 4:] = 0
    return torch.from_numpy(feats).cuda(), torch.from_numpy(mask).cuda() if ragged else None


def gestures(B, T, align, ragged):
    def run(e):
        feats, mask = gesture_inputs(B, T, ragged)
        return e.jegal_gestures(feats, mask, align=align)
    return f"jegal_gestures B{B} T{T} align{align} ragged{ragged}", run


def audio(ragged):
    def run(e):
        mel, valid = synth.synth_mel(77, 3, 40), (40, 17, 4)
        for b, v in enumerate(valid if ragged else ()):
            mel[b, v:] = 0
        return e.jegal_audio(torch.from_numpy(mel).cuda(), valid_len=valid if ragged else None)
    return f"jegal_audio B3 Tm40 ragged{ragged}", run


def text(e):
    st = torch.from_numpy(np.random.default_rng(7).standard_normal((2, 33, 768)).astype(np.float32))
    m = torch.ones(2, 33)
    m[1, 20:] = 0
    return e.jegal_text(st.cuda(), m.cuda())


def fuse(e):
    return e.fuse_content(torch.from_numpy(np.random.default_rng(8).standard_normal((70, 512)).astype(np.float32)).cuda())


def xlmr(e):
    ids, mask = synth.xlmr_inputs(5, 2, 33)
    return e.xlmr_encode(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda())


def clip(B, T):
    return f"gestsync_clip B{B} T{T}", lambda e: e.gestsync_clip(torch.from_numpy(synth.synth_frames(611, B, T)).cuda())


def windows(e):
    vol = torch.from_numpy(synth.synth_frames(612, 1, 27)[0].astype(np.float32) / np.float32(255.0)).permute(3, 0, 1, 2)
    return e.gestsync_windows(torch.stack([vol[:, i:i + 25] for i in range(3)]).cuda())


def cases(config):
    """[(case name, per-case options, run(engine) -> output tensor)] of one handle"""
    models = CONFIGS[config][2]
    aw = config.startswith("rc_aw")
    out = []

    def add(named, **opts):
        name, run = named
        out.append((f"{config}/{name}" + "".join(f" {k}={v}" for k, v in opts.items()), opts, run))

    if models & JG:
        gest = [gestures(B, T, a, r) for B, T in GESTURE_SHAPES for a in (0, 1) for r in (0, 1)]
        for g in gest:
            if aw:
                add(g, audit_stages=4)
                for parts in (1, 2, 4, 8, 15):
                    add(g, audit_jegal_parts=parts)
            else:
                add(g)
                if config == "rc":
                    add(g, jegal_fp32_ends=0)
    if config in ("rc", "bf16", "rc_aw"):
        for named in (audio(0), audio(1), ("jegal_text B2 L33", text), ("fuse_content rows70", fuse)):
            if aw:
                add(named, audit_stages=8)
            elif config == "rc" or named[0].startswith("jegal_audio"):
                add(named)
        if config == "rc":
            add(("jegal_text B2 L33", text), jegal_fp32_ends=0)
            add(("fuse_content rows70", fuse), jegal_fp32_ends=0)
    if models & XL:
        add(("xlmr_encode B2 L33", xlmr), **({"audit_stages": 16} if aw else {}))
    if models & GS:
        stage = {"audit_stages": 2} if aw else {}
        add(clip(1, 30), **stage)           # fewer than 1024 tokens: the unfused plan in every mode
        add(clip(2, 10), **stage)
        add(clip(1, 50), **stage)           # the fused plan where the mode has one (12 LayerNorm launches become none)
        if config in ("rc", "rc_aw"):
            add(("gestsync_windows N3", windows), **stage)
    return out


def run_config(config, e=None):
    """-> [{case, launches, workspace_bytes, sha256}] of one handle's cases"""
    own = e is None
    e = e or engine(config)
    recs = []
    try:
        e.profile(True)
        for name, opts, run in cases(config):
            for k, v in {**RUNTIME, **opts}.items():
                e.set_option(k, v)
            e.profile_reset()
            y = run(e)
            launches = {k: n for k, (_, n) in e.profile_get().items() if n}
            sha = hashlib.sha256(y.contiguous().cpu().numpy().tobytes()).hexdigest()
            recs.append(dict(case=name, launches=launches, workspace_bytes=e.workspace_bytes(), sha256=sha))
        for k, v in RUNTIME.items():
            e.set_option(k, v)
        e.profile(False)
    finally:
        if own:
            e.close()
    return recs


def compare(old, new):
    a, b = ({r["case"]: r for r in map(json.loads, open(p))} for p in (old, new))
    bad = [c for c in a if c not in b or a[c]["launches"] != b[c]["launches"] or a[c]["sha256"] != b[c]["sha256"]
           or b[c]["workspace_bytes"] > a[c]["workspace_bytes"]]
    for c in bad:
        print("DIFFERS", json.dumps(a[c]), json.dumps(b.get(c)))
    print(f"{len(a)} cases in OLD, {len(b)} in NEW: {len(a) - len(bad)} with equal launches and digest and no more workspace, {len(bad)} differ")
    return 1 if bad or len(a) != len(b) else 0


def main():
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        sys.exit(compare(args[1], args[2]))
    golden = None
    if "--golden" in args:
        i = args.index("--golden")
        golden = args[i + 1]
        del args[i:i + 2]
    if args:
        L.LIB_PATH = os.path.abspath(args[0])
    recs = []
    for config in CONFIGS:
        for r in run_config(config):
            print(json.dumps(r), flush=True)
            recs.append(r)
    if golden:
        json.dump({r["case"]: r["launches"] for r in recs}, open(golden, "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
