"""Bit identity and launch time of the attention kernels, for comparing two builds of libjegal_hip.so:

    python tools/attn_digest.py [LIB.so]          (default: jegal_amd/libjegal_hip.so; once per library, each in a fresh process)

Runs the fixed-seed inputs of tests/test_gpu_kernels_fp64.py -- the grid of test_attention_vs_fp64 (ATTN_S x four (dk, H, mask)
combinations), the bf16 sizes of test_attention_valu_fp32_and_bf16_vs_fp64 and the six gather sizes -- through debug_attention /
debug_attention_gather and prints one JSON line per case: the kernel, the SHA-256 of the output bytes and the median of 20 timed
launches after 3 warm-ups (device events).  Equal digests case by case = the two builds compute the same bits."""
import hashlib, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import jegal_amd._lib as L
if len(sys.argv) > 1:
    L.LIB_PATH = os.path.abspath(sys.argv[1])
import test_gpu_kernels_fp64 as T           # the tests' own input generators: same seeds, same operands


def report(e, case, launch, out, rows):
    for _ in range(3):
        launch()
    ms = []
    for _ in range(20):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        launch()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    sha = hashlib.sha256(out[:rows].contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()
    print(json.dumps(dict(case=case, kernel=e.debug_last_kernel(), sha256=sha, median_us=round(1e3 * statistics.median(ms), 2))), flush=True)


def dense(e, B, S, H, dk, mk, bf):
    q, k, v, mask = T.attn_inputs(torch.Generator().manual_seed(5 + S), B, S, H, dk, mk)
    qkv = torch.cat([x.reshape(B * S, H * dk) for x in (q, k, v)], 1).to(T.dt16(bf)).to(T.DEV)
    km = mask.float().to(T.DEV) if mask is not None else None
    out = torch.zeros((B * S, H * dk), dtype=T.dt16(bf), device=T.DEV)
    report(e, f"{'bf16' if bf else 'fp16'} S={S} dk={dk} H={H} mask={int(mk)}", lambda: e.debug_attention(qkv, km, B, S, H, dk, out), out, B * S)


def gather(e, S):
    g = torch.Generator().manual_seed(6 + S)
    H, dk, Twin, P, shift, nclip = 8, 64, 5, 9, 12, 3
    B, D = nclip * Twin, H * dk
    pos = T.urnd(g, (nclip * P, 3 * D)).half().to(T.DEV)
    pe = T.urnd(g, (S, 3 * D), -0.5, 0.5).half().to(T.DEV)
    out = torch.zeros((B * S, D), dtype=torch.float16, device=T.DEV)
    report(e, f"gather S={S}", lambda: e.debug_attention_gather(pos, pe, Twin, P, shift, B, S, H, out), out, B * S)


def main():
    e, ebf = T.engine(), T.engine(prec=4)
    for S in T.ATTN_S:
        for dk, H, mk in ((64, 8, False), (64, 8, True), (96, 12, True), (96, 12, False)):
            dense(e, 4 if mk else 2, S, H, dk, mk, False)
    for S in (7, 21, 32, 33, 160, 200):
        for dk, H, mk in ((64, 8, True), (96, 12, True), (64, 8, False)):
            dense(ebf, 4, S, H, dk, mk, True)
    for S in (1, 7, 21, 24, 25, 32):
        gather(e, S)


if __name__ == "__main__":
    main()
