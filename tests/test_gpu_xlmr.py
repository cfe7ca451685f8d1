"""XLM-RoBERTa text front end on the HIP engine, through the C ABI (jg_xlmr_encode).

Reference call site: models/jegal.py:116-129 (``mroberta(input_ids, attention_mask=text_mask).last_hidden_state``).  The model is
third-party (transformers); parity is pinned against transformers.XLMRobertaModel with seeded weights (tests/golden/xlmr.npz)."""
import os

import numpy as np
import pytest
import torch

import jegal_oracle as O
from jegal_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-3        # relative L2 over the valid token rows (rows have unit-order LayerNorm scale)


def rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def xlmr():
    from jegal_amd._lib import Engine
    from jegal_amd.xlmr import XLMRoberta
    eng = Engine(0)
    m = XLMRoberta(engine=eng).load_state_dict({"roberta." + k: v for k, v in synth.xlmr_state_dict().items()})
    yield m
    eng.close()


def test_xlmr_matches_transformers_golden(xlmr, golden_dir):
    g = np.load(os.path.join(golden_dir, "xlmr.npz"))
    out = xlmr(torch.from_numpy(g["input_ids"]), attention_mask=torch.from_numpy(g["attention_mask"])).last_hidden_state.cpu()
    ref = torch.from_numpy(g["last_hidden_state"])
    m = torch.from_numpy(g["attention_mask"]).bool()
    e = rel(out[m], ref[m])
    print("xlmr vs transformers golden: rel-L2 %.3e, max-abs %.3e" % (e, float((out[m] - ref[m]).abs().max())))
    assert e < TOL
    out1 = xlmr(torch.from_numpy(g["input_ids"][:1])).last_hidden_state.cpu()
    assert rel(out1, torch.from_numpy(g["last_hidden_state_nomask"])) < TOL


@pytest.mark.parametrize("B,L", [(1, 3), (2, 33), (5, 70), (2, 200), (1, 512), (103, 160)])      # (103, 160): two lanes of 8 160 / 8 320 rows -- 256x256 tiles, the last one partial along M
def test_xlmr_lengths_vs_oracle(xlmr, B, L):
    """Short, odd and long sequences (attn_mfma_kernel up to 160 tokens, attn_mfma_flash_kernel<64> beyond; 512 = the position table's limit),
    ragged padding, against the fp32 restatement."""
    ids, mask = synth.xlmr_inputs(100 + L, B, L)
    sd = synth.xlmr_state_dict()
    with torch.no_grad():
        ref = O.xlmr_forward(sd, ids, mask)
    out = xlmr(torch.from_numpy(ids).cuda(), attention_mask=torch.from_numpy(mask).cuda()).last_hidden_state.cpu()
    m = torch.from_numpy(mask).bool()
    e = rel(out[m], ref[m])
    print(f"B={B} L={L}: rel-L2 {e:.3e}")
    assert torch.isfinite(out).all() and e < TOL


def test_xlmr_properties_and_errors(xlmr):
    ids, mask = synth.xlmr_inputs(7, 4, 40)
    a = xlmr(ids, attention_mask=mask).last_hidden_state
    b = xlmr(ids, attention_mask=mask).last_hidden_state
    assert torch.equal(a, b)                                         # deterministic
    # a sample's valid rows do not depend on what else is in the batch, nor on how much padding follows
    one = xlmr(ids[2:3], attention_mask=mask[2:3]).last_hidden_state
    n = int(mask[2].sum())
    assert rel(one[0, :n].cpu(), a[2, :n].cpu()) < 1e-5
    with pytest.raises(ValueError):
        xlmr(ids[0])                                                  # not (B, L)
    with pytest.raises(ValueError):
        xlmr(ids, attention_mask=mask[:, :10])
    with pytest.raises(RuntimeError):
        xlmr(np.ones((1, 600), np.int32))                             # beyond the position table


def test_xlmr_implicit_layernorm_and_lanes(xlmr):
    """Round 4: the default pass never materialises a LayerNorm (option xlmr_fold: un-normalised hi + lo token planes, LayerNorm
    folded into the consumer GEMMs / recomputed in the producer epilogues, xlmr.hip:xlmr_encode_folded) and runs a batch as two
    half batches on two streams.  Both against the explicit-LayerNorm pass (xlmr_fold=0) and the fp32 restatement; the lanes
    must not change a bit; hi+lo (default) and single-fp16 (calibrated) weights alike."""
    from jegal_amd._lib import Engine
    from jegal_amd.xlmr import XLMRoberta
    sd = synth.xlmr_state_dict()
    ids, mask = synth.xlmr_inputs(31, 16, 40)                         # ragged padding; 2 x 320 rows: both lanes above the 256-row minimum
    with torch.no_grad():
        ref = O.xlmr_forward(sd, ids, mask)
    m = torch.from_numpy(mask).bool()
    ids_d, mask_d = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    eng0 = Engine(0)
    eng0.set_option("xlmr_fold", 0)
    plain = XLMRoberta(engine=eng0).load_state_dict(sd)
    try:
        for calibrated in (False, True):
            if calibrated:
                xlmr.calibrate(ids_d[:4], mask_d[:4])
                plain.calibrate(ids_d[:4], mask_d[:4])
            a = xlmr(ids_d, attention_mask=mask_d).last_hidden_state
            xlmr.engine.set_option("dual_stream", 0)
            b = xlmr(ids_d, attention_mask=mask_d).last_hidden_state
            xlmr.engine.set_option("dual_stream", 1)
            assert torch.equal(a, b)
            c = plain(ids_d, attention_mask=mask_d).last_hidden_state
            ea, ec, eac = rel(a.cpu()[m], ref[m]), rel(c.cpu()[m], ref[m]), rel(a.cpu()[m], c.cpu()[m])
            print(f"calibrated={calibrated}: implicit LN vs oracle {ea:.3e}, explicit LN vs oracle {ec:.3e}, implicit vs explicit {eac:.3e}")
            assert ea < TOL and ec < TOL and eac < TOL
    finally:
        eng0.close()
        xlmr.load_state_dict({"roberta." + k: v for k, v in sd.items()})          # back to the un-calibrated weights for the tests below


@pytest.mark.parametrize("mode,bound", [("PREC_FP16", 2e-3), ("PREC_FP16_W2", 1e-3), ("PREC_BF16", 3e-2)])
def test_xlmr_other_precision_modes_run_the_implicit_layernorm_path(mode, bound):
    """The implicit-LayerNorm GEMM instances exist in every build (single fp16, hi+lo, the bf16 re-build with bf16 token planes): plain
    fp16 and bf16 are reported modes (outside the 1e-3 contract), W2 meets it."""
    import jegal_amd._lib as L
    from jegal_amd.xlmr import XLMRoberta
    sd = synth.xlmr_state_dict()
    ids, mask = synth.xlmr_inputs(41, 6, 50)
    with torch.no_grad():
        ref = O.xlmr_forward(sd, ids, mask)
    eng = L.Engine(0, precision=getattr(L, mode))
    try:
        out = XLMRoberta(engine=eng).load_state_dict(sd)(torch.from_numpy(ids).cuda(), attention_mask=torch.from_numpy(mask).cuda()).last_hidden_state.cpu()
    finally:
        eng.close()
    m = torch.from_numpy(mask).bool()
    e = rel(out[m], ref[m])
    print(f"{mode}: XLM-R (implicit LayerNorm) vs the fp32 restatement: rel-L2 {e:.3e}")
    assert torch.isfinite(out).all() and e < bound


class StubTokenizer:
    """HuggingFace-fast-tokenizer calling convention (is_split_into_words, offsets, padding) over a toy vocabulary: every word
    becomes one or two sub-word ids; <s> = 0, </s> = 2, <pad> = 1 as in xlm-roberta (the real sentencepiece model is not
    available offline)."""

    def __call__(self, text_batch, return_tensors="pt", padding=True, is_split_into_words=True, return_offsets_mapping=True):
        rows = []
        for words in text_batch:
            ids, offs = [0], [(0, 0)]
            for w in words:
                h = sum(ord(c) * (i + 7) for i, c in enumerate(w))
                pieces = 1 + (len(w) > 4)
                cut = len(w) // 2 if pieces == 2 else len(w)
                ids.append(3 + h % 900); offs.append((0, cut))
                if pieces == 2:
                    ids.append(3 + (h * 31 + 5) % 900); offs.append((cut, len(w)))
            ids.append(2); offs.append((0, 0))
            rows.append((ids, offs))
        L = max(len(r[0]) for r in rows)
        input_ids = torch.ones(len(rows), L, dtype=torch.long)
        mask = torch.zeros(len(rows), L, dtype=torch.long)
        offsets = torch.zeros(len(rows), L, 2, dtype=torch.long)
        for b, (ids, offs) in enumerate(rows):
            input_ids[b, :len(ids)] = torch.tensor(ids)
            mask[b, :len(ids)] = 1
            offsets[b, :len(ids)] = torch.tensor(offs)
        return {"input_ids": input_ids, "attention_mask": mask, "offset_mapping": offsets}


def test_text_to_content_embedding_end_to_end(xlmr):
    """jegal.py:116-129 + 377-420 with the engine in place of the CPU mroberta: sentences -> tokenizer (host) -> XLM-RoBERTa (engine)
    -> JEGAL text encoder + word pooling + fusion/align (engine) -> word-level content embeddings; against the same JEGAL path fed
    with the fp32 restatement's hidden states."""
    from jegal_amd.jegal import JEGAL
    from jegal_amd.xlmr import roberta_embeddings
    text = ["so we went over there yesterday", "and then it suddenly stopped working", "hello"]
    tok = StubTokenizer()
    jg = JEGAL(engine=xlmr.engine, text_encoder=lambda t: roberta_embeddings(xlmr, tok, t))
    jg.load_state_dict(synth.jegal_state_dict())
    c = jg.forward_inference(text=text)
    pack = roberta_embeddings(xlmr, tok, text)
    with torch.no_grad():
        states = O.xlmr_forward(synth.xlmr_state_dict(), pack[3].numpy(), pack[1].numpy())
    c_ref = jg.forward_inference(text=(states, pack[1], pack[2], pack[3], pack[4]))
    assert c.shape == c_ref.shape and c.shape[0] == 3 and c.shape[2] == 512
    e = rel(c.cpu(), c_ref.cpu())
    print("content embeddings, engine XLM-R vs oracle XLM-R hidden states: rel-L2 %.3e" % e)
    assert e < TOL
    # and the whole chain against the ORACLE end to end (round 3: the comparison above shares the engine's JEGAL half): fp32
    # restatement of XLM-R -> fp32 restatement of JEGAL text encoder + word pooling + fusion / align, per clip over its real words
    jsd = O.tensors(synth.jegal_state_dict())
    with torch.no_grad():
        c_orc = O.jegal_forward_inference(jsd, text=(states, pack[1], pack[2], pack[3], pack[4]))
    nwords = [len(t.split(" ")) for t in text]
    for b, w in enumerate(nwords):
        eb = rel(xlmr.engine.l2norm(c[b, :w]).cpu(), O.l2_normalize(c_orc[b, :w]))
        print("clip %d (%d words): engine chain vs oracle chain rel-L2 %.3e" % (b, w, eb))
        assert eb < TOL


def test_xlmr_12_layers_matches_transformers_golden(golden_dir):
    """the 12-layer model was only checked by a tool.  Full depth of xlm-roberta-base against transformers itself
    (tests/golden/xlmr12.npz, generated by oracle/make_golden.py xlmr), default precision mode (bias-corrected single-fp16 weights,
    calibrated on built-in token ids)."""
    from jegal_amd._lib import Engine
    from jegal_amd.xlmr import XLMRoberta
    g = np.load(os.path.join(golden_dir, "xlmr12.npz"))
    eng = Engine(0)
    m = XLMRoberta(engine=eng).load_state_dict(synth.xlmr_state_dict(layers=12))
    out = m(torch.from_numpy(g["input_ids"]).cuda(), attention_mask=torch.from_numpy(g["attention_mask"]).cuda()).last_hidden_state.cpu()
    ref = torch.from_numpy(g["last_hidden_state"])
    mk = torch.from_numpy(g["attention_mask"]).bool()
    e = rel(out[mk], ref[mk])
    print("xlmr 12 layers vs transformers golden: rel-L2 %.3e, max-abs %.3e" % (e, float((out[mk] - ref[mk]).abs().max())))
    eng.close()
    assert e < TOL


def test_xlmr_calibration_is_explicit_and_holds_on_other_token_distributions():
    """in the default precision mode the XLM-R Linears were bias-corrected single fp16, calibrated implicitly on
    uniform-random ids without padding -- and every check drew its ids from that same distribution.  Now: (1) after
    load_state_dict the encoder runs hi+lo (calibration-free); (2) calibrate(ids, mask) is explicit; (3) a calibration on UNIFORM
    unpadded ids is tested on a DIFFERENT distribution -- heavily skewed ids (90 % of the tokens from 20 ids), ragged padding --
    and (4) a calibration on the skewed padded ids themselves; all within 1e-3 of the fp32 restatement, errors printed."""
    from jegal_amd._lib import Engine
    from jegal_amd.xlmr import XLMRoberta
    eng = Engine(0)
    sd = synth.xlmr_state_dict()
    m = XLMRoberta(engine=eng).load_state_dict({"roberta." + k: v for k, v in sd.items()})
    rng = np.random.default_rng(99)
    B, L = 6, 48
    ids = np.where(rng.random((B, L)) < 0.9, rng.integers(3, 23, (B, L)), rng.integers(3, 1000, (B, L))).astype(np.int64)
    lens = [48, 9, 30, 17, 48, 5]
    mask = np.zeros((B, L), np.int64)
    for b, l in enumerate(lens):
        ids[b, 0], ids[b, l - 1] = 0, 2
        ids[b, l:] = 1
        mask[b, :l] = 1
    with torch.no_grad():
        ref = O.xlmr_forward(sd, ids, mask)
    mm = torch.from_numpy(mask).bool()
    ids_d, mask_d = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    res = {}
    res["hi+lo (default, uncalibrated)"] = rel(m(ids_d, attention_mask=mask_d).last_hidden_state.cpu()[mm], ref[mm])
    m.calibrate()                                                       # built-in: uniform ids, no padding
    res["calibrated on uniform unpadded ids"] = rel(m(ids_d, attention_mask=mask_d).last_hidden_state.cpu()[mm], ref[mm])
    m.calibrate(ids_d, mask_d)                                          # the caller's own tokens
    res["calibrated on these ids"] = rel(m(ids_d, attention_mask=mask_d).last_hidden_state.cpu()[mm], ref[mm])
    print("\nXLM-R, skewed + padded ids vs the fp32 restatement:", {k: f"{v:.2e}" for k, v in res.items()})
    for k, v in res.items():
        assert v < TOL, (k, v)
    eng.close()
    # calibration outside mode 3 is an error, not a silent no-op
    from jegal_amd._lib import JegalError, PREC_FP16_W2
    e2 = Engine(0, precision=PREC_FP16_W2)
    m2 = XLMRoberta(engine=e2).load_state_dict({"roberta." + k: v for k, v in sd.items()})
    with pytest.raises(JegalError):
        m2.calibrate()
    e2.close()


def test_xlmr_calibration_on_one_short_sentence_ignores_the_padding_rows():
    """batches of fewer than 128 tokens run padded to 128 rows; the calibration pass used to average those padding rows
    (bias values, rstd = 316 after the first producer epilogue) into E[x].  Calibrating on ONE 20-token sentence must give the
    corrections of the same sentence repeated 8 times (160 rows, no padding): identical E[x] up to summation order."""
    from jegal_amd._lib import Engine
    from jegal_amd.xlmr import XLMRoberta
    sd = synth.xlmr_state_dict()
    ids, mask = synth.xlmr_inputs(77, 1, 20)
    test_ids, test_mask = synth.xlmr_inputs(78, 4, 40)
    with torch.no_grad():
        ref = O.xlmr_forward(sd, test_ids, test_mask)
    mm = torch.from_numpy(test_mask).bool()
    outs = {}
    for name, rep in (("one sentence (20 rows, padded to 128)", 1), ("the sentence x 8 (160 rows)", 8)):
        eng = Engine(0)
        m = XLMRoberta(engine=eng).load_state_dict({"roberta." + k: v for k, v in sd.items()})
        m.calibrate(torch.from_numpy(np.repeat(ids, rep, 0)).cuda(), torch.from_numpy(np.repeat(mask, rep, 0)).cuda())
        outs[name] = m(torch.from_numpy(test_ids).cuda(), attention_mask=torch.from_numpy(test_mask).cuda()).last_hidden_state.cpu()
        eng.close()
        e = rel(outs[name][mm], ref[mm])
        print(f"\ncalibrated on {name}: rel-L2 vs the fp32 restatement {e:.3e}", end="")
        assert e < TOL
    a, b = outs.values()
    assert rel(a[mm], b[mm]) < 2e-5


def test_dataset_driver_runs_xlmr_on_the_engine_batch_invariant(tmp_path, monkeypatch):
    """`extract_jegal_embs --modalities t --xlmr_checkpoint ... --tokenizer ...`: phrases from the csv -> tokenizer (host; a stub with
    the HuggingFace calling convention, the sentencepiece model is not available offline) -> XLM-RoBERTa on the engine -> JEGAL
    text encoder -> word pooling -> fusion, eight sentences of 1..9 words in ONE padded batch.  Every .pkl must be what the oracle
    chain (fp32 XLM-R restatement + fp32 JEGAL restatement) gives for that sentence ALONE (models/jegal.py:116-129,168-171;
    evaluation/extract_jegal_embs.py:141 runs batch_size=1)."""
    import pickle
    import pandas as pd
    from jegal_amd import drivers
    monkeypatch.setattr(drivers, "_load_tokenizer", lambda name: StubTokenizer())
    phrases = ["hello", "so we went over there yesterday", "and then it suddenly stopped working", "two words", "a b c d e f g h i",
               "extraordinarily long wordforms everywhere", "yes", "the quick brown fox jumps"]
    rows = []
    for i, ph in enumerate(phrases):
        wb = [[w, 5 * j, 5 * j + 4] for j, w in enumerate(ph.split(" "))]
        rows.append({"video_id": f"vid{i}", "filename": f"vid{i}/00000", "phrase": ph, "word_boundaries": str(wb), "target_word_boundary": str(wb[0])})
    csv = str(tmp_path / "avs.csv")
    pd.DataFrame(rows).to_csv(csv, index=False)
    res_dir = str(tmp_path / "res")
    assert drivers.main(["extract_jegal_embs", "--file_path", csv, "--checkpoint_path", "synthetic", "--res_dir", res_dir, "--video_dir", str(tmp_path),
                         "--feature_dir", str(tmp_path), "--modalities", "t", "--xlmr_checkpoint", "synthetic", "--tokenizer", "stub", "--batch_size", "8"]) == 0
    jsd = O.tensors(synth.jegal_state_dict())
    xsd = synth.xlmr_state_dict()
    tok = StubTokenizer()
    worst = 0.0
    for i, ph in enumerate(phrases):
        got = pickle.load(open(os.path.join(res_dir, "t", f"vid{i}__00000.pkl"), "rb"))["content_emb"]
        enc = tok([ph.split(" ")])
        with torch.no_grad():
            states = O.xlmr_forward(xsd, enc["input_ids"].numpy(), enc["attention_mask"].numpy())
            ref = O.l2_normalize(O.jegal_forward_inference(jsd, text=(states, enc["attention_mask"], [ph.split(" ")], enc["input_ids"], enc["offset_mapping"]))[0]).numpy()
        assert got.shape == ref.shape == (len(ph.split(" ")), 512)
        worst = max(worst, float(np.linalg.norm(got - ref) / np.linalg.norm(ref)))
    print(f"\nphrases -> XLM-R on the engine -> content embeddings, 8 ragged sentences in one batch vs the oracle on each alone: rel-L2 {worst:.2e}")
    assert worst < TOL


def test_xlmr_is_reproducible_under_a_poisoned_workspace():
    """Round 6.  In steady state an uninitialised or stale read of the workspace returns the PREVIOUS identical run's value and stays
    invisible; with option ws_poison the arena is filled with NaN bytes before every call, so run-to-run bit-identity becomes a
    real test.  With two parts in flight (the default) 10-40 % of such runs used to differ on some sequences
    (tools/experiments/xlmr_race/xl_poison_probe.py) -- a packed-fp32 instruction of the implicit-LayerNorm consumer's epilogue read
    one operand as 0 in lanes 48-63 while the other part's attention kernel issued MFMAs on the same SIMD
    (tools/experiments/pk_opsel_mfma/repro.hip); the library is built without packed-fp32 instructions since.  Two parts must equal one."""
    from jegal_amd._lib import Engine
    from jegal_amd.xlmr import XLMRoberta
    eng = Engine(0)
    try:
        m = XLMRoberta(engine=eng).load_state_dict(synth.xlmr_state_dict(layers=2))
        for B, L in ((64, 32), (24, 40)):
            ids, mask = synth.xlmr_inputs(3, B, L)
            ids_d, mask_d = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
            eng.set_option("ws_poison", 0)
            eng.set_option("xlmr_lanes", 1)
            base = m(ids_d, attention_mask=mask_d).last_hidden_state.clone()
            assert torch.isfinite(base).all()
            eng.set_option("ws_poison", 1)
            for lanes in (2, 1, 4):
                eng.set_option("xlmr_lanes", lanes)
                for it in range(40 if lanes == 2 else 8):
                    eng.set_option("gemm_tile", it & 3)
                    out = m(ids_d, attention_mask=mask_d).last_hidden_state
                    assert torch.equal(out, base), (B, L, lanes, it)
    finally:
        eng.set_option("gemm_tile", 0)
        eng.close()


def test_two_handles_on_two_streams_do_not_disturb_each_other():
    """Two handles, two streams (the second of high priority, so the runtime gives it a hardware queue of its own and the two passes
    really overlap), the second trailing the first by a varying delay: each must return what it returns alone.  This is the
    application-level form of the round-6 finding -- 16-48 % of such runs differed at the unlucky delays
    (tools/experiments/xlmr_race/two_handles_sweep.sh) before the packed-fp32 instructions were taken out of the build."""
    from jegal_amd._lib import Engine
    from jegal_amd.xlmr import XLMRoberta
    sd = synth.xlmr_state_dict(layers=2)
    engs, xls, ins, streams, base = [], [], [], [], []
    try:
        for k in range(2):
            e = Engine(0)
            e.set_option("xlmr_lanes", 1)
            engs.append(e)
            xls.append(XLMRoberta(engine=e).load_state_dict(sd))
            ids, mask = synth.xlmr_inputs(3 + k, 32, 32)
            ins.append((torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()))
            streams.append(torch.cuda.Stream(priority=-1 if k else 0))
        torch.cuda.synchronize()
        for k in range(2):
            base.append(xls[k](ins[k][0], attention_mask=ins[k][1]).last_hidden_state.clone())
            torch.cuda.synchronize()
        for delay in (40_000, 160_000, 0, 100_000):                 # shader cycles; 40 000 and 160 000 were the worst before
            for it in range(40):
                outs = [None, None]
                gate = torch.cuda.Event()
                torch.cuda._sleep(3_000_000)                         # both passes queue up behind this and start together
                gate.record()
                for k in ((0, 1) if it & 1 else (1, 0)):
                    with torch.cuda.stream(streams[k]):
                        streams[k].wait_event(gate)
                        if k == 1 and delay:
                            torch.cuda._sleep(delay)
                        outs[k] = xls[k](ins[k][0], attention_mask=ins[k][1]).last_hidden_state
                torch.cuda.synchronize()
                for k in range(2):
                    assert torch.equal(outs[k], base[k]), (delay, it, k)
    finally:
        for e in engs:
            e.close()
