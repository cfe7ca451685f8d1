"""Activation range at the split-operand GEMM's call sites (gemm_x3, option jegal_fp32_ends), on the CPU oracle.

gemm_x3 splits its fp32 A in the loader as hi = fp16(a), lo = fp16(a - hi).  Below |a| ~ 2^-3 the lo half is an fp16 subnormal with an
absolute quantum of 2^-24, so how close the split is to fp32 depends on the activations' scale.  This tool runs the oracle's JEGAL
forward passes (GestSync features of synthetic clips -> gesture branch; synthetic text states + mel -> content path) with the seeded
weights of the six weight families of tests/test_gpu_weight_families.py, captures the A operand of every Linear the engine runs on
gemm_x3, and reports per call site:
  * the per-row rms of A (min / median) and max |A|,
  * split_rel: ||(A - (hi + lo)) W^T|| / ||A W^T + b||, the output error the split itself causes on these very activations,
    next to the norm-wise bound 2 sqrt(K) 2^-24 of tests/test_gpu_kernels_fp64.py.

    python tools/x3_operand_range.py [--T 40] [--out profiles/x3_operand_range.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import jegal_oracle as O  # noqa: E402
from jegal_amd import synth  # noqa: E402

FAMILIES = [("gauss", 0), ("gauss", 1), ("gauss", 2), ("heavy", 0), ("sharp2", 0), ("sharp", 0)]
# Linears on gemm_x3 in the fp16 modes (jegal.hip: jegal_input / jegal_tail / jegal_text / fuse_content in the split-operand arithmetic, Arith<float>{x3}); the encoder
# feed-forward ones are not, and are measured as a wider envelope (rows marked ffn_x3_only, summary "with_ffn")
X3_SITES = ["proj_ip_rgb.0", "proj_ip_rgb.3", "proj_op_rgb", "proj_op_align_gesture.0", "proj_op_align_gesture.2", "proj_op_text",
            "proj_op_fusion_content.0", "proj_op_fusion_content.2", "proj_op_align_content.0", "proj_op_align_content.2"]
FFN_SITES = [f"encoder_rgb.layers.{l}.feed_forward.w_{i}" for l in range(6) for i in (1, 2)]


def split_x3(a):
    hi = a.half().float()
    lo = (a - hi).half().float()
    return hi + lo


def measure(T=40, B=2, W=10):
    rows = {}
    frames = synth.synth_frames(1234, B, T)
    mel = synth.synth_mel(1235, B, 600)                # 150 audio steps: the word boundaries of synth_boundaries reach step 145
    states, tmask, ids, offs = synth.synth_text(1236, B, W)
    wbs = synth.synth_boundaries(B, W)
    pack = (torch.from_numpy(states), torch.from_numpy(tmask), [[w[0] for w in wb] for wb in wbs], ids, offs)
    lin0 = O.F.linear
    for name, off in FAMILIES:
        fam = f"{name}+{off}"
        gt = O.tensors(synth.gestsync_state_dict(seed=synth.GESTSYNC_SEED + off, include_unused=False, family=name))
        jt = O.tensors(synth.jegal_state_dict(seed=synth.JEGAL_SEED + off, family=name))
        names = {v.data_ptr(): k[:-len(".weight")] for k, v in jt.items() if k.endswith(".weight")}
        seen = {}

        def rec(x, w, b=None):
            site = names.get(w.data_ptr())
            if site in X3_SITES or site in FFN_SITES:
                a = x.reshape(-1, x.shape[-1]).float()
                a = a[a.abs().amax(1) > 0]                       # all-zero padding rows carry no error
                y = lin0(a, w, b)
                err = (a - split_x3(a)) @ w.t()
                st = seen.setdefault(site, {"rms": [], "maxabs": 0.0, "err2": 0.0, "ref2": 0.0, "K": a.shape[1]})
                st["rms"].append(a.pow(2).mean(1).sqrt())
                st["maxabs"] = max(st["maxabs"], float(a.abs().max()))
                st["err2"] += float(err.double().pow(2).sum())
                st["ref2"] += float(y.double().pow(2).sum())
            return lin0(x, w, b)

        O.F.linear = rec
        try:
            with torch.no_grad():
                for b in range(B):
                    f = O.gestsync_clip_feats(gt, torch.from_numpy(frames[b].astype(np.float32) / np.float32(255.0)))
                    O.jegal_forward_inference(jt, visual_feats=f[None], visual_mask=torch.ones(1, T))
                O.jegal_forward_inference(jt, text=pack, audio=torch.from_numpy(mel), audio_mask=None, word_boundaries=wbs)
        finally:
            O.F.linear = lin0
        for site, st in seen.items():
            r = torch.cat(st["rms"])
            rows[f"{fam}/{site}"] = dict(K=st["K"], rows=int(r.numel()), rms_min=float(r.min()), rms_median=float(r.median()),
                                         max_abs=st["maxabs"], split_rel=math.sqrt(st["err2"] / st["ref2"]),
                                         bound=2 * math.sqrt(st["K"]) * 2.0 ** -24, ffn_x3_only=site in FFN_SITES)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rows = measure(a.T)
    for k, v in rows.items():
        print(f"{k:55s} K={v['K']:5d} rms {v['rms_min']:.3e} .. median {v['rms_median']:.3e}  max|a| {v['max_abs']:.3e}  "
              f"split_rel {v['split_rel']:.2e} (bound {v['bound']:.2e})")
    core = [v for v in rows.values() if not v["ffn_x3_only"]]
    allv = list(rows.values())
    summary = dict(rms_min=min(v["rms_min"] for v in core), max_abs=max(v["max_abs"] for v in core),
                   worst_split_over_bound=max(v["split_rel"] / v["bound"] for v in core),
                   with_ffn=dict(rms_min=min(v["rms_min"] for v in allv), max_abs=max(v["max_abs"] for v in allv),
                                 worst_split_over_bound=max(v["split_rel"] / v["bound"] for v in allv)))
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(T=a.T, summary=summary, sites=rows), f, indent=1)


if __name__ == "__main__":
    main()
