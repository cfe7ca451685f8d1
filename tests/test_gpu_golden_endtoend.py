"""GPU parity tests (run with -m gpu on the MI355X box).  Everything goes through the C ABI
(libjegal_hip.so via ctypes); expected values come from tests/golden (outputs of the REAL
reference) and from the CPU oracle on the same seeded inputs.

Tolerance (BASELINE north_star): embeddings within 1e-3 relative (rel-L2 per clip matrix) of the
fp32 reference, plus max-abs <= 1e-3 on unit-norm rows.  Intermediate tensors use the same bound.
"""
import os

import numpy as np
import pytest
import torch

import jegal_oracle as O
from jegal_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-3


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def engine():
    from jegal_amd._lib import Engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Engine.get("cuda:0")


@pytest.fixture(scope="module")
def models(engine):
    from jegal_amd.gestsync import GestSync
    from jegal_amd.jegal import JEGAL
    gs = GestSync(engine=engine).load_state_dict(synth.gestsync_state_dict())     # incl. unused audio/LSTM keys
    jg = JEGAL(engine=engine).load_state_dict(synth.jegal_state_dict())
    return gs, jg


@pytest.fixture(scope="module")
def oracle_sd():
    return O.tensors(synth.gestsync_state_dict(include_unused=False)), O.tensors(synth.jegal_state_dict())


def _golden_windows(g):
    frames = synth.synth_frames(int(g["seed"]), 1, int(g["T"]))[0]
    f01 = O.pad_clip(torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)))
    vol = f01.permute(3, 0, 1, 2)
    return frames, torch.stack([vol[:, i:i + 25] for i in range(f01.shape[0] - 24)])


def test_strict_load_rejects_missing_key(engine):
    from jegal_amd._lib import Engine, JegalError
    from jegal_amd.gestsync import GestSync
    e2 = Engine(0)
    sd = synth.gestsync_state_dict(include_unused=False)
    del sd["net_vid.bn3.running_var"]
    with pytest.raises(JegalError, match="missing weight"):
        GestSync(engine=e2).load_state_dict(sd)
    e2.close()


def test_conv1_pool_kernel(models, golden_dir, oracle_sd):
    """conv1+BN+ReLU+maxpool: fused u8 kernel and the stack+implicit-GEMM formulation, against the
    reference golden slice and the full oracle tensor.
    (The kernel-level check, element by element against float64 and bit for bit: tests/test_gpu_conv1_fp64.py.)"""
    gs, _ = models
    gsd, _ = oracle_sd
    g = np.load(os.path.join(golden_dir, "gestsync_clip.npz"))
    frames = synth.synth_frames(int(g["seed"]), 1, int(g["T"]))[0]
    f01 = O.pad_clip(torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)))
    with torch.no_grad():
        ref = O.vgg_vid(gsd, f01.permute(3, 0, 1, 2).unsqueeze(0)[:, :, :9], upto="conv1")[0]     # (64,5,43,78)
    ref = ref.permute(1, 2, 3, 0).numpy()                                                          # (5,43,78,64)
    outs = {}
    for direct in (1, 0):
        gs.engine.set_option("conv1_direct", direct)
        out = gs.engine.debug_conv1_pool(torch.from_numpy(frames)[None].cuda(), 12).float().cpu().numpy()
        outs[direct] = out
        assert out.shape == (26, 43, 78, 64)
        assert rel(out[0].transpose(2, 0, 1)[:, ::6, ::6], g["conv1_pool_t0"]) < TOL
        assert rel(out[:5], ref) < TOL, f"direct={direct}"
        print(f"conv1 direct={direct}: rel {rel(out[:5], ref):.3e} max-abs {np.abs(out[:5] - ref).max():.3e}")
    gs.engine.set_option("conv1_direct", 1)
    d = np.abs(outs[1] - outs[0])
    print("direct vs stack: max", d.max(), "rel", rel(outs[1], outs[0]))
    assert rel(outs[1], outs[0]) < 3e-4          # both round the same fp32 sums to fp16


def test_forward_vid_matches_reference_golden(models, golden_dir):
    gs, _ = models
    g = np.load(os.path.join(golden_dir, "gestsync_clip.npz"))
    _, x = _golden_windows(g)
    out, out_conv = gs.forward_vid(x[:2].cuda(), return_feats=True)
    assert out.shape == (2, 1024, 21) and out_conv.shape == (2, 512, 21)
    assert rel(out_conv, g["out_conv"][:2]) < TOL
    assert rel(out, g["out_full"]) < TOL


def test_clip_features_match_reference_golden(models, golden_dir):
    gs, _ = models
    g = np.load(os.path.join(golden_dir, "gestsync_clip.npz"))
    frames, x = _golden_windows(g)
    feats_u8 = gs.extract_clip_feats(torch.from_numpy(frames).cuda())[0]
    assert rel(feats_u8, g["feats"]) < TOL
    # fused u8 conv1 kernel vs the stack_frames + implicit-GEMM formulation: same fp16 operands,
    # only the fp32 accumulation order differs
    gs.engine.set_option("conv1_direct", 0)
    feats_v0 = gs.extract_clip_feats(torch.from_numpy(frames).cuda())[0]
    gs.engine.set_option("conv1_direct", 1)
    assert rel(feats_u8, feats_v0) < 1e-3
    # edge de-duplication (T+4 instead of T+20 conv positions) is bit-identical
    gs.engine.set_option("edge_dedup", 0)
    feats_all = gs.extract_clip_feats(torch.from_numpy(frames).cuda())[0]
    gs.engine.set_option("edge_dedup", 1)
    assert torch.equal(feats_all, feats_u8)
    f01 = torch.from_numpy(frames.astype(np.float32) / np.float32(255.0)).cuda()
    feats_f32 = gs.extract_clip_feats(f01)[0]
    assert rel(feats_f32, g["feats"]) < TOL
    # drop-in window path == de-duplicated clip path (size-independent property)
    win = gs.forward_vid(x.cuda()).mean(-1)
    assert rel(win, feats_f32) < 5e-4


def _gesture_inputs():
    rng = np.random.default_rng(9002)
    vf = rng.standard_normal((2, 40, 1024)).astype(np.float32)
    vf[1, 30:] = 0
    vm = np.ones((2, 40), np.float32)
    vm[1, 30:] = 0
    return torch.from_numpy(vf), torch.from_numpy(vm)


def test_jegal_gesture_golden(models, golden_dir):
    _, jg = models
    g = np.load(os.path.join(golden_dir, "jegal_gesture.npz"))
    vf, vm = _gesture_inputs()
    out = jg.forward_inference(visual_feats=vf.cuda(), visual_mask=vm.cuda())
    fg = jg.forward_gestures(vf.cuda(), vm.cuda().unsqueeze(1))
    # padded query rows of clip 1 are computed by the reference too; compare everything
    assert rel(fg, g["fwd_gestures"]) < TOL
    assert rel(out, g["gesture"]) < TOL


AUDIO_WB = [[["a", 3, 9], ["b", 10, 10], ["c", 12, 30]], [["d", 0, 5], ["e", 6, 20]]]


def test_jegal_audio_golden(models, golden_dir):
    _, jg = models
    g = np.load(os.path.join(golden_dir, "jegal_audio.npz"))
    mel = torch.from_numpy(synth.synth_mel(int(g["seed"]), 2, 160)).cuda()
    fa = jg.forward_audio(mel)
    assert fa.shape == g["fwd_audio"].shape
    assert rel(fa, g["fwd_audio"]) < TOL
    c = jg.forward_inference(audio=mel, audio_mask=torch.ones(2, 40), word_boundaries=AUDIO_WB)
    assert c.shape == g["content"].shape
    assert rel(c, g["content"]) < TOL
    # padded word row of clip 1 is NOT masked out by the reference (zero input row -> bias path)
    assert float(c[1, 2].abs().max()) > 0


def _text_pack(g):
    tbatch = [["w0", "w1", "w2", "w3"], ["x0", "x1", "x2"]]
    return (torch.from_numpy(g["states"]), torch.from_numpy(g["mask"]), tbatch, torch.from_numpy(g["ids"]), torch.from_numpy(g["offsets"]))


def test_jegal_text_golden(models, golden_dir):
    _, jg = models
    g = np.load(os.path.join(golden_dir, "jegal_text.npz"))
    ft = jg.forward_text(torch.from_numpy(g["states"]).cuda(), torch.from_numpy(g["mask"]).cuda().unsqueeze(1))
    assert rel(ft, g["fwd_text"]) < TOL
    c = jg.forward_inference(text=_text_pack(g))
    assert c.shape == g["content"].shape
    assert rel(c, g["content"]) < TOL
    # same result through a text_encoder callable (the get_roberta_embeddings hook)
    jg.text_encoder = lambda text: _text_pack(g)
    c2 = jg.forward_inference(text=["w0 w1 w2 w3", "x0 x1 x2"])
    jg.text_encoder = None
    assert torch.equal(c, c2)


def test_jegal_vta_golden(models, golden_dir):
    _, jg = models
    g = np.load(os.path.join(golden_dir, "jegal_vta.npz"))
    gt = np.load(os.path.join(golden_dir, "jegal_text.npz"))
    vf, vm = _gesture_inputs()
    wb2 = [[["w0", 2, 6], ["w1", 7, 12], ["w2", 13, 13], ["w3", 15, 30]], [["x0", 1, 4], ["x1", 5, 9], ["x2", 10, 22]]]
    mel = torch.from_numpy(synth.synth_mel(9003, 2, 160)).cuda()
    ge, ce = jg.forward_inference(visual_feats=vf.cuda(), visual_mask=vm.cuda(), text=_text_pack(gt), audio=mel,
                                  audio_mask=torch.ones(2, 40), word_boundaries=wb2)
    assert rel(ge, g["gesture"]) < TOL
    assert rel(ce, g["content"]) < TOL
    # round 4: the engine keeps one workspace arena per stream (jg_set_stream).  Two callers on two un-synchronised streams, their
    # calls interleaved call by call, must get what each gets alone (before, the second call re-used the arena the first one's
    # kernels were still working in).
    vf2 = torch.flip(vf, dims=[1]).contiguous().cuda()
    ge_b, ce_b = jg.forward_inference(visual_feats=vf2, visual_mask=vm.cuda(), text=_text_pack(gt), audio=mel * 0.5 + 4.0,
                                      audio_mask=torch.ones(2, 40), word_boundaries=wb2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(4):
        with torch.cuda.stream(s1):
            o1 = jg.forward_inference(visual_feats=vf.cuda(), visual_mask=vm.cuda(), text=_text_pack(gt), audio=mel,
                                      audio_mask=torch.ones(2, 40), word_boundaries=wb2)
        with torch.cuda.stream(s2):
            o2 = jg.forward_inference(visual_feats=vf2, visual_mask=vm.cuda(), text=_text_pack(gt), audio=mel * 0.5 + 4.0,
                                      audio_mask=torch.ones(2, 40), word_boundaries=wb2)
        outs.append((o1, o2))
    torch.cuda.synchronize()
    for o1, o2 in outs:
        assert torch.equal(o1[0], ge) and torch.equal(o1[1], ce) and torch.equal(o2[0], ge_b) and torch.equal(o2[1], ce_b)


def test_error_behaviour(models):
    _, jg = models
    mel = torch.from_numpy(synth.synth_mel(1, 1, 160)).cuda()
    with pytest.raises(IndexError):            # empty audio slice, as jegal.py:239
        jg.forward_inference(audio=mel, audio_mask=torch.ones(1, 40), word_boundaries=[[["a", 0, 3], ["b", 100, 120]]])
    with pytest.raises(RuntimeError):          # no text encoder configured
        jg.forward_inference(text=["hello world"])
    from jegal_amd._lib import JegalError
    with pytest.raises(JegalError):            # T beyond the PE table (modules.py:136)
        jg.forward_gestures(torch.zeros(1, 501, 1024).cuda())


def test_l2norm_and_metrics_golden(engine, golden_dir):
    from jegal_amd import metrics as M
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    ge, ce = synth.planted_retrieval(9005, 64)
    ge[7] = ge[3]
    x = torch.randn(37, 512)
    assert rel(engine.l2norm(x.cuda()), O.l2_normalize(x)) < 1e-6
    m = M.retrieval_metrics(ce, ge, engine=engine)
    for k in ("R5", "R10", "R25", "R50", "MR"):
        assert m[k] == float(g[k]), (k, m)
    assert m["R1"] == O.compute_metrics(g["sim"])["R1"]
    gest, cont, bounds, targets = synth.planted_spotting(9006, 20, n_frames=60, n_words=10, noise=2.0)
    acc = M.spotting_accuracy(gest, cont, [str(b) for b in bounds], targets, engine=engine)
    assert acc == pytest.approx(float(g["spot_acc"]))
    for P in (2, 4, 6):
        ref = int(np.argmax(g[f"asd{P}"]))
        pred = engine.asd(torch.from_numpy(ce[:1]), torch.from_numpy(ge[:6]), [0, 6]).cpu().numpy()
        assert pred[0, (P // 2) - 1] == ref
    vl = M.video_level(engine, gest)
    ref = np.stack([x.mean(axis=0) for x in gest])
    assert rel(vl, ref) < 1e-6


def test_retrieval_config4_scale(engine):
    """BASELINE configs[3] metric parity: N=10k planted gallery; identical R@K / MR to the oracle."""
    from jegal_amd import metrics as M
    N = 10000
    ge, ce = synth.planted_retrieval(1237, N)
    m = M.retrieval_metrics(ce, ge, engine=engine)
    sim = O.similarity_matrix(ce, ge).numpy()
    ref = O.compute_metrics(sim)
    assert m == ref, (m, ref)
    # sharded form: 8 contiguous query blocks against the full gallery give the same ranks
    e1, e2 = engine.l2norm(torch.from_numpy(ce)), engine.l2norm(torch.from_numpy(ge))
    full_rank, full_ties = engine.sim_rank(e1, e2)
    per = -(-N // 8)
    parts = [engine.sim_rank(e1[r * per:(r + 1) * per], e2, r * per) for r in range(8)]
    assert torch.equal(torch.cat([p[0] for p in parts]), full_rank)
    assert torch.equal(torch.cat([p[1] for p in parts]), full_ties)


def test_spotting_config5_scale(engine):
    """BASELINE configs[4]: 4000 clips, T=150, W=30 -> accuracy identical to the oracle."""
    from jegal_amd import metrics as M
    gest, cont, bounds, targets = synth.planted_spotting(1238, 4000)
    acc = M.spotting_accuracy(gest, cont, bounds, targets, engine=engine)
    ref = O.spotting_accuracy(gest, cont, bounds, targets)
    assert acc == pytest.approx(ref)
    assert 10.0 < acc < 90.0


def test_gesture_only_full_length_vs_oracle(engine, models, oracle_sd):
    """BASELINE configs[1] at full clip length (T=150): 2 clips of the seed-1234 batch against the CPU
    oracle end to end (frames -> unit-norm gesture embedding)."""
    gsd, jsd = oracle_sd
    T = 150
    frames = synth.synth_frames(1234, 2, T)
    emb = engine.extract_gesture(torch.from_numpy(frames).cuda()).cpu()
    assert emb.shape == (2, T, 512)
    assert torch.allclose(emb.norm(dim=-1), torch.ones(2, T), atol=1e-5)
    with torch.no_grad():
        for b in range(2):
            f = O.gestsync_clip_feats(gsd, torch.from_numpy(frames[b].astype(np.float32) / np.float32(255.0)))
            ref = O.l2_normalize(O.jegal_forward_inference(jsd, visual_feats=f[None], visual_mask=torch.ones(1, T))[0])
            r = rel(emb[b], ref)
            mx = float((emb[b] - ref).abs().max())
            print(f"clip {b}: rel-L2 {r:.3e} max-abs {mx:.3e}")
            assert r < TOL and mx < TOL


def test_logmel_frontend(engine):
    """STFT + mel + log on the GPU vs torch.stft on the CPU (same mel basis; the basis itself restates
    librosa's published algorithm and is unpinned).  Sizes of the reference's samples: 34691 samples -> 216 frames."""
    from jegal_amd import audio
    rng = np.random.default_rng(3)
    wav = (rng.standard_normal((2, 34691)) * 3000).astype(np.float32)
    wav[1] *= np.linspace(0.0, 1.0, 34691, dtype=np.float32)
    feats, _, _, mb = audio.wav2filterbanks(torch.from_numpy(wav).cuda(), engine=engine)
    assert feats.shape == (2, 216, 80)
    ref = O.wav2filterbanks(wav, mb.cpu())
    assert float((feats.cpu() - ref).abs().max()) < 2e-3
    assert rel(feats, ref) < 1e-5
    basis = audio.mel_filterbank()
    assert basis.shape == (80, 257) and (basis >= 0).all() and (basis.sum(1) > 0).all()
    # the CNN consumes it: 216 mel frames -> 54 audio steps
    assert engine.audio_len(216) == 54
    # BASELINE configs[0] plumbing: the reference's own samples/sample1.wav (data fixture) -> 216 log-mel frames
    wav1 = audio.load_wav(os.path.join(os.path.dirname(__file__), "golden", "sample1.wav")).astype("float32")
    assert wav1.shape == (34691,)
    f1, _, _, _ = audio.wav2filterbanks(torch.from_numpy(wav1)[None].cuda(), engine=engine)
    assert f1.shape == (1, 216, 80)
    assert rel(f1, O.wav2filterbanks(wav1[None], mb.cpu())) < 1e-5
    # ... and against the reference's own wav2filterbanks output for that file (tests/golden/logmel_sample1.npz, make_golden.py logmel)
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "logmel_sample1.npz"))["features"]
    assert rel(f1[0], gold) < 1e-5 and float(np.abs(f1[0].cpu().numpy() - gold).max()) < 2e-3


def test_precision_modes(oracle_sd):
    """hi+lo (W2) and bias-corrected (default) weights both hold the 1e-3 bound on a fresh clip; plain fp16
    is measurably worse (it is what the two remedies exist for); re-calibrating on real clips keeps the bound."""
    from jegal_amd._lib import Engine, PREC_FP16, PREC_FP16_W2, PREC_FP16_BC
    from jegal_amd.gestsync import GestSync
    from jegal_amd.jegal import JEGAL
    gsd, jsd = oracle_sd
    T = 20
    frames = synth.synth_frames(4242, 1, T)
    with torch.no_grad():
        f = O.gestsync_clip_feats(gsd, torch.from_numpy(frames[0].astype(np.float32) / np.float32(255.0)))
        ref = O.l2_normalize(O.jegal_forward_inference(jsd, visual_feats=f[None], visual_mask=torch.ones(1, T))[0])
    err = {}
    for mode in (PREC_FP16, PREC_FP16_W2, PREC_FP16_BC):
        e = Engine(0, precision=mode)
        GestSync(engine=e).load_state_dict(synth.gestsync_state_dict(include_unused=False))
        JEGAL(engine=e).load_state_dict(synth.jegal_state_dict())
        err[mode] = rel(e.extract_gesture(torch.from_numpy(frames).cuda())[0], ref)
        if mode == PREC_FP16_BC:
            e.calibrate(torch.from_numpy(synth.synth_frames(99, 2, 12)).cuda())       # user-supplied calibration clips
            err["recal"] = rel(e.extract_gesture(torch.from_numpy(frames).cuda())[0], ref)
        e.close()
    print("precision modes:", err)
    assert err[PREC_FP16_W2] < TOL and err[PREC_FP16_BC] < TOL and err["recal"] < TOL
    assert err[PREC_FP16_BC] < err[PREC_FP16]


def test_batch32_properties(engine, models):
    """Full BASELINE batch (32 x 150 frames): finite, unit-norm, deterministic, and independent of
    batch composition/chunking (clip b of the batch == the same clip run alone)."""
    T = 150
    frames = torch.from_numpy(synth.synth_frames(1234, 32, T)).cuda()
    a = engine.extract_gesture(frames)
    b = engine.extract_gesture(frames)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert torch.allclose(a.norm(dim=-1), torch.ones(32, T, device=a.device), atol=1e-5)
    solo = engine.extract_gesture(frames[5:6])
    assert rel(solo[0], a[5]) < 1e-5
    engine.set_chunk(3)
    c = engine.extract_gesture(frames[:7])
    engine.set_chunk(32)
    assert rel(c, a[:7]) < 1e-5


def test_vta_config3_full_batch(engine, models, oracle_sd):
    """BASELINE configs[2]: batch 64, tri-modal (mel (64,600,80) ~ N(8,2.5), text states
    (64,12,768), 10 words with boundaries [w_i, 15i, 15i+10]).  Shapes / finiteness on the whole batch, content
    and gesture embeddings of 2 clips against the oracle."""
    gs, jg = models
    _, jsd = oracle_sd
    B, T, W = 64, 150, 10
    frames = torch.from_numpy(synth.synth_frames(1234, B, T)).cuda()
    feats = torch.cat([gs.extract_clip_feats(frames[i:i + 32]) for i in range(0, B, 32)])
    mel = synth.synth_mel(1235, B, 4 * T)
    states, tmask, ids, offs = synth.synth_text(1236, B, W)
    wbs = synth.synth_boundaries(B, W)
    tbatch = [[w[0] for w in wb] for wb in wbs]
    pack = (torch.from_numpy(states), torch.from_numpy(tmask), tbatch, ids, offs)
    g, c = jg.forward_inference(visual_feats=feats, visual_mask=torch.ones(B, T), text=pack, audio=torch.from_numpy(mel),
                                audio_mask=torch.ones(B, T), word_boundaries=wbs)
    assert g.shape == (B, T, 512) and c.shape == (B, W, 512)
    assert torch.isfinite(g).all() and torch.isfinite(c).all()
    gn, cn = engine.l2norm(g), engine.l2norm(c)
    for b in (0, 63):
        p1 = (states[b:b + 1], tmask[b:b + 1], tbatch[b:b + 1], ids[b:b + 1], offs[b:b + 1])
        with torch.no_grad():
            rg, rc = O.jegal_forward_inference(jsd, visual_feats=feats[b:b + 1].cpu(), visual_mask=torch.ones(1, T), text=p1,
                                               audio=torch.from_numpy(mel[b:b + 1]), audio_mask=None, word_boundaries=wbs[b:b + 1])
        eg, ec = rel(gn[b], O.l2_normalize(rg[0])), rel(cn[b], O.l2_normalize(rc[0]))
        print(f"vta clip {b}: gesture rel {eg:.3e} content rel {ec:.3e}")
        assert eg < TOL and ec < TOL


def test_ragged_batch_padding(models):
    """Zero-padded clips + key mask (dataset.py:336-340 contract): valid rows of a padded batch equal
    the clip run alone."""
    _, jg = models
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.standard_normal((1, 50, 1024)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.standard_normal((1, 31, 1024)).astype(np.float32)).cuda()
    batch = torch.zeros(2, 50, 1024, device="cuda")
    batch[0] = a[0]
    batch[1, :31] = b[0]
    mask = torch.ones(2, 50, device="cuda")
    mask[1, 31:] = 0
    out = jg.forward_inference(visual_feats=batch, visual_mask=mask)
    solo_b = jg.forward_inference(visual_feats=b, visual_mask=torch.ones(1, 31, device="cuda"))
    solo_a = jg.forward_inference(visual_feats=a, visual_mask=torch.ones(1, 50, device="cuda"))
    rb, ra = rel(out[1, :31], solo_b[0]), rel(out[0], solo_a[0])
    print('ragged rel', rb, ra)
    assert rb < 1e-5 and ra < 1e-5, (rb, ra)


def test_repeated_runs_are_bit_identical(engine, models):
    """No atomics, no data-dependent scheduling: the same batch gives the same bits every time (guards the hand-rolled
    waits/barriers of the persistent kernels -- a race shows up here as a flaky mismatch).  Large enough for the fused
    GEMM+LayerNorm path (M = 4*60*21 tokens >= 1024) and for zero-tile skipping in conv1."""
    eng = engine
    frames = torch.from_numpy(synth.synth_frames(4242, 4, 60)).cuda()
    ref = eng.extract_gesture(frames).clone()
    assert torch.isfinite(ref).all()
    for _ in range(4):
        assert torch.equal(eng.extract_gesture(frames), ref)
