"""Command-line drivers mirroring the reference's hot-path scripts.

    python -m jegal_amd.drivers extract_gestsync_feats ...   # preprocess/extract_gestsync_feats.py
    python -m jegal_amd.drivers extract_jegal_embs ...       # evaluation/extract_jegal_embs.py
    python -m jegal_amd.drivers evaluate_retrieval --path D  # evaluation/evaluate_retrieval.py
    python -m jegal_amd.drivers evaluate_spotting  --path D  # evaluation/evaluate_spotting.py
    python -m jegal_amd.drivers evaluate_asd --path D --file avs_asd.csv   # evaluation/evaluate_asd.py
    python -m jegal_amd.drivers inference_embs ...            # inference_embs.py (single clip -> <fname>.pkl)
    python -m jegal_amd.drivers attn_matrix --path F|D        # utils/plot_heatmap.py without the rendering (-> <name>.attn.npz)
    python -m jegal_amd.drivers retrieve --path D [--topk 10] # the retrieval evaluate_retrieval.py grades (-> retrieve_<direction>.npz)
    python -m jegal_amd.drivers search --path D --query F.pkl [--level word|phrase|coupling|ordered] [--align]   # which clips gesture a word, and at which frame (-> search_<F>.npz)
    python -m jegal_amd.drivers asd --path D --file avs_asd.csv [--win N --hop M]   # the detection evaluate_asd.py grades (-> asd.npz)
    python -m jegal_amd.drivers sync_offset --checkpoint_path_gestsync CKPT --frames F.npy --wav F.wav [--mel F.npy] [--max_shift 15]   # audio-visual offset of a clip (-> <name>.sync.npz)
        [--win 125 --hop 25]   # the offset over time (start, offset_t, conf_t, curve_t);  several --frames: which track is in sync with the audio, per window
    python -m jegal_amd.drivers embed_tracks --checkpoint_path_jegal CKPT --feature_dir D --result_dir R [--win 120 --ctx 50]   # gesture embeddings of tracks of any length (-> R/v/<vid>__<track>.pkl)

Same flags, file naming and on-disk formats as the reference.  What is upstream of the hot path is
NOT rebuilt: video decoding / mediapipe masking (the drivers read already masked 270x480 crops as
``<frames_dir>/<vid>/<track>.npy`` uint8 (T,270,480,3)) and XLM-RoBERTa's tokenizer; audio is read as the reference reads it
(``<video_dir>/<file>.wav`` -> log-mel on the GPU, or a precomputed ``<file>.mel.npy`` (4T,80) fp32); XLM-RoBERTa states come from
``--text_states_dir`` (``<vid>__<track>.npz`` holding states/mask/ids/offsets) or a ``text_encoder`` passed from Python.
Run under ``torchrun`` to shard over GPUs (contiguous blocks, extract_gestsync_feats.py:366-370).
"""
import argparse
import ast
import glob
import os
import pickle
import sys

import numpy as np
import torch

from . import dist as jdist
from . import extract
from . import metrics as M
from . import synth
from ._metric_entries import COUPLING_MAX_W


def load_checkpoint(path, kind):
    """inference_embs.py:92-119: torch.load(path)['state_dict'] with 'module.' stripped.
    path == 'synthetic' gives the seeded synthetic weights (no checkpoints ship with the reference)."""
    if path == "synthetic":
        return synth.gestsync_state_dict() if kind == "gestsync" else synth.jegal_state_dict()
    ckpt = torch.load(path, map_location="cpu")
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    return {k.replace("module.", ""): v for k, v in sd.items()}


def _add_precision_args(p):
    p.add_argument("--precision", type=int, default=None, choices=[0, 1, 2, 3, 5, 6],
                   help="engine precision mode (include/jegal_hip.h); default: 5 (run-time corrected fp16: per-clip, calibration-free), "
                        "or 3 (bias-corrected fp16, ~3 %% faster) when --calibrate_frames is given; 6 = the fp32 audit mode (exact-fp32 "
                        "MFMAs, fp32 activations: the reference's CPU arithmetic, ~50x slower)")
    p.add_argument("--calibrate_frames", default=None,
                   help=".npy of masked uint8 crops (B,T,270,480,3) or (T,270,480,3): re-run the precision-mode-3 calibration on them")


#: engine precision mode (include/jegal_hip.h) a driver selects unless calibration clips are supplied: the library's default,
#: calibration-free by construction.  tests/test_gpu_weight_families.py holds THIS mode to 1e-3 on every weight family.
REAL_CHECKPOINT_PRECISION = 5          # PREC_FP16_RC: per-clip run-time correction (round 5; rounds 3-4: 1 = PREC_FP16_W2, 1.4x slower)


def pick_precision(args, checkpoints, can_calibrate=True):
    """Every checkpoint -- the seeded synthetic one included -- runs the library's default, the calibration-free run-time corrected
    mode (E[x] per clip from the clip's own rows, JG_PREC_FP16_RC; held to 1e-3 on every weight family by
    tests/test_gpu_weight_families.py).  The bias-corrected mode (JG_PREC_FP16_BC: the same term folded into the biases once, ~3 %
    faster) is chosen only when the caller supplies calibration clips AND the command can run the
    calibration on them (can_calibrate: it needs the GestSync model, frames -> features -> JEGAL); its built-in calibration on
    synthetic clips was only ever validated on the seeded weights."""
    from ._lib import PREC_FP16_BC
    if getattr(args, "precision", None) is not None:
        return args.precision
    calibrated = bool(getattr(args, "calibrate_frames", None)) and can_calibrate
    return PREC_FP16_BC if calibrated else REAL_CHECKPOINT_PRECISION


def _models(args, need_gestsync=False, need_jegal=False):
    from ._lib import Engine, PREC_FP16_BC
    from .gestsync import GestSync
    from .jegal import JEGAL
    jdist.init_from_env()
    if torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    eng = Engine.get()
    prec = pick_precision(args, [getattr(args, "checkpoint_path_gestsync", None) if need_gestsync else None,
                                 getattr(args, "checkpoint_path", None) if need_jegal else None], can_calibrate=need_gestsync)
    if getattr(args, "calibrate_frames", None) and not need_gestsync:
        print("Note: --calibrate_frames needs the GestSync model and is ignored by this command (precision mode {})".format(prec))
    if eng.finalized == 0:
        eng.set_precision(prec)
    elif (need_gestsync or need_jegal) and eng.precision != prec:
        raise RuntimeError("this process already holds an engine finalized in precision mode {}; mode {} was asked for "
                           "(close the engine or start a new process)".format(eng.precision, prec))
    gs = jg = None
    if need_gestsync:
        gs = GestSync(engine=eng).load_state_dict(load_checkpoint(args.checkpoint_path_gestsync, "gestsync"))
    if need_jegal:
        jg = JEGAL(engine=eng).load_state_dict(load_checkpoint(args.checkpoint_path, "jegal"))
    if getattr(args, "calibrate_frames", None) and prec == PREC_FP16_BC and need_gestsync:
        clips = np.load(args.calibrate_frames)
        eng.calibrate(torch.from_numpy(clips if clips.ndim == 5 else clips[None]).to(eng.device))
    return eng, gs, jg


def _engine(engine, args):
    """the Engine a command runs on: the caller's, or this process's"""
    return engine if engine is not None else _models(args)[0]


# --------------------------------------------------------------------------- feature files
def _load_pkl(fn):
    with open(fn, "rb") as f:
        return pickle.load(f)


def _base_name(fn):
    """a file's name without its directory and its extension"""
    return os.path.basename(fn).rsplit(".", 1)[0]


def _feature_words(ft):
    """the words of a feature dict, from its info (the csv row, a pandas Series, or inference_embs' {fname, word_boundaries, text}); None where
    it holds no boundaries"""
    info = ft.get("info")
    return M.word_bounds(info["word_boundaries"])[0] if info is not None and "word_boundaries" in info else None


def _check_topk(topk):
    if not 1 <= topk <= 128:
        raise SystemExit("--topk must be 1..128")


def _gesture_content(out, has_visual, has_content):
    """JEGAL.forward_inference's return value -> (gesture | None, content | None): both when it was given frames and text or audio"""
    if has_visual and has_content:
        return out
    return (out, None) if has_visual else (None, out)


def _wav_mel(wav_fn, eng):
    """a 16 kHz mono .wav -> its (1, Tm, 80) log-mel on the engine's device (jg_logmel)"""
    from . import audio as jaudio
    wav = torch.from_numpy(np.asarray(jaudio.load_wav(wav_fn)).astype(np.float32))
    return jaudio.wav2filterbanks(wav[None].to(eng.device), engine=eng)[0]


def _run_groups(groups, run_group, save, label):
    """Run every group of items in one call of run_group(group) -> one result per item; a group that raises is run again item by item, so
    that one bad file does not take its neighbours down (a group of one is not retried).  save(result, item) stores one result, under its
    own try (per-file try/except as in the reference, extract_gestsync_feats.py:347-351).  Every failure prints ``Error: <e> | <label>:
    <item[1]>``.  -> (saved, err)"""
    saved = err = 0
    for group in groups:
        try:
            results = run_group(group)
        except Exception as e:
            if len(group) == 1:
                err += 1
                print("Error: ", e, " | {}: ".format(label), group[0][1])
                continue
            results = []
            for item in group:
                try:
                    results.append(run_group([item])[0])
                except Exception as e1:
                    results.append(None)
                    err += 1
                    print("Error: ", e1, " | {}: ".format(label), item[1])
        for result, item in zip(results, group):
            if result is None:
                continue
            try:
                save(result, item)
                saved += 1
            except Exception as e:
                err += 1
                print("Error: ", e, " | {}: ".format(label), item[1])
    return saved, err


# --------------------------------------------------------------------------- extract_gestsync_feats
def cmd_extract_gestsync_feats(argv):
    p = argparse.ArgumentParser(prog="extract_gestsync_feats")
    p.add_argument("--checkpoint_path_gestsync", required=True)
    p.add_argument("--frames_dir", required=True, help="<vid>/<track>.npy masked uint8 crops (T,270,480,3)")
    p.add_argument("--result_dir", required=True)
    p.add_argument("--batch_size", type=int, default=48, help="accepted for compatibility; windows are never materialised")
    p.add_argument("--clips_per_batch", type=int, default=16, help="clips of similar length processed per engine call (padded to the longest with its last frame: exact)")
    p.add_argument("--frames_per_batch", type=int, default=4800, help="upper bound on clips x longest clip per engine call (workspace / host memory bound)")
    p.add_argument("--rank", type=int, default=None)
    p.add_argument("--nshard", type=int, default=None)
    _add_precision_args(p)
    args = p.parse_args(argv)
    eng, gs, _ = _models(args, need_gestsync=True)
    files = sorted(glob.glob(os.path.join(args.frames_dir, "*", "*.npy")))
    lo, hi = jdist.shard_range(len(files), args.rank, args.nshard)
    print("Total videos: {} | Start : End = {} : {}".format(len(files), lo, hi))
    saved = err = 0
    todo = []
    for f in files[lo:hi]:
        out = os.path.join(args.result_dir, f.split("/")[-2], os.path.basename(f))
        if os.path.exists(out):                      # resume: skip-if-exists (extract_gestsync_feats.py:281-284)
            saved += 1
            continue
        todo.append((f, out))
    # Clips of different lengths go through the engine in batches: a clip padded with copies of its LAST frame gives, for its own
    # T frames, exactly the windows of the reference's edge padding (inference_embs.py:283 replicates the last frame 12 times;
    # window t only reaches frame t+12) - so a batch is padded to its longest clip, the first T_i rows of clip i are kept, and
    # the GEMMs see several clips at once instead of one.  Files are sorted by length to keep the padding small.  A batch is
    # bounded by clips AND by padded frames (--frames_per_batch): the engine's workspace grows with clips x Tmax (about 2.9 MB per
    # conv position) and the host array with 388 KB per frame, so long tracks go through in small groups or alone, as the
    # reference's one-video-at-a-time loop bounds them (extract_gestsync_feats.py:314-344).
    def clip_len(f):
        try:
            m = np.load(f, mmap_mode="r")
            if m.dtype != np.uint8:
                return -2
            return m.shape[0] if m.ndim == 4 and tuple(m.shape[1:]) == (270, 480, 3) and m.shape[0] > 0 else -1
        except Exception:
            return -1
    sized = sorted(((clip_len(f), f, out) for f, out in todo), key=lambda x: x[0])
    for T_bad, f, _ in [x for x in sized if x[0] <= 0]:
        err += 1
        print("Error: ", "expected uint8 crops" if T_bad == -2 else "expected a (T,270,480,3) uint8 .npy", " | Video file: ", f)
    sized = [x for x in sized if x[0] > 0]

    def run_group(group):
        """Features of a group of clips (padded to its longest); returns the list of (T,1024) arrays."""
        Tmax = max(t for t, _, _ in group)
        batch = np.empty((len(group), Tmax, 270, 480, 3), np.uint8)
        for i, (t, f, _) in enumerate(group):
            fr = np.load(f)
            batch[i, :t] = fr
            batch[i, t:] = fr[t - 1]
        # (the lengths keep each clip's run-time precision correction on its OWN frames: rows < t are those of the clip alone -- bit for bit
        # from 49 frames on, within the contract below: include/jegal_hip.h, jg_gestsync_clip_ragged)
        feats = gs.extract_clip_feats(torch.from_numpy(batch).to(eng.device), lengths=[t for t, _, _ in group]).cpu().numpy()
        return [feats[i, :t] for i, (t, _, _) in enumerate(group)]

    def save_one(feat, item):
        os.makedirs(os.path.dirname(item[2]), exist_ok=True)
        np.save(item[2], feat)

    nb, fmax = max(1, args.clips_per_batch), max(1, args.frames_per_batch)
    groups, s0 = [], 0
    while s0 < len(sized):
        s1 = s0 + 1                                   # sorted by length: the last clip of a group is its longest
        while s1 < len(sized) and s1 - s0 < nb and (s1 - s0 + 1) * sized[s1][0] <= fmax:
            s1 += 1
        groups.append(sized[s0:s1])
        s0 = s1
    done, failed = _run_groups(groups, run_group, save_one, "Video file")
    print("No of files saved = {} | Err = {}".format(saved + done, err + failed))
    return 0


# --------------------------------------------------------------------------- extract_jegal_embs
def _load_tokenizer(name):
    """The reference's module global `tokenizer = AutoTokenizer.from_pretrained("xlm-roberta-base")` (models/jegal.py:13): third-party,
    host side.  `name` is a HuggingFace name or a local directory (no network on the GPU boxes: pass a directory)."""
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(name)


def _load_xlmr(eng, path):
    """`mroberta = XLMRobertaModel.from_pretrained("xlm-roberta-base")` (models/jegal.py:14) on the engine: `path` = a state_dict of
    transformers.XLMRobertaModel (torch.save) or 'synthetic' (seeded test weights, reduced vocabulary)."""
    from .xlmr import XLMRoberta
    sd = synth.xlmr_state_dict() if path == "synthetic" else torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    return XLMRoberta(engine=eng).load_state_dict({k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()})


def _load_text_pack(path):
    z = np.load(path, allow_pickle=True)
    return z["states"], z["mask"], z["ids"], z["offsets"]


def cmd_extract_jegal_embs(argv):
    import pandas as pd
    p = argparse.ArgumentParser(prog="extract_jegal_embs")
    p.add_argument("--file_path", required=True)
    p.add_argument("--checkpoint_path", required=True)
    p.add_argument("--res_dir", required=True)
    p.add_argument("--video_dir", required=True)
    p.add_argument("--feature_dir", required=True)
    p.add_argument("--text_states_dir", default=None, help="precomputed XLM-RoBERTa states <vid>__<track>.npz (states, mask, ids, offsets)")
    p.add_argument("--xlmr_checkpoint", default=None, help="state_dict of transformers.XLMRobertaModel (or 'synthetic'): run XLM-RoBERTa on the engine "
                                                           "from the csv's phrases, as models/jegal.py:116-129 does on the CPU; needs --tokenizer")
    p.add_argument("--tokenizer", default=None, help="HuggingFace tokenizer name or local directory (models/jegal.py:13: xlm-roberta-base)")
    p.add_argument("--modalities", default="vta", choices=["vta", "vt", "va", "ta", "v", "t", "a"])
    p.add_argument("--batch_size", type=int, default=16, help="clips per engine call (the reference: 1; results are those of batch size 1 whatever this is)")
    _add_precision_args(p)
    args = p.parse_args(argv)
    eng, _, jg = _models(args, need_jegal=True)
    xlmr = tok = None
    if "t" in args.modalities and args.xlmr_checkpoint:
        if not args.tokenizer:
            raise SystemExit("--xlmr_checkpoint needs --tokenizer (a HuggingFace name or a local tokenizer directory)")
        xlmr, tok = _load_xlmr(eng, args.xlmr_checkpoint), _load_tokenizer(args.tokenizer)
    df = pd.read_csv(args.file_path)
    print("Total files: {}".format(len(df)))
    res_dir = os.path.join(args.res_dir, args.modalities)
    os.makedirs(res_dir, exist_ok=True)
    lo, hi = jdist.shard_range(len(df))
    mod = args.modalities
    saved = 0
    rows = [df.iloc[i] for i in range(lo, hi)]
    for s in range(0, len(rows), args.batch_size):
        batch = []
        for row in rows[s:s + args.batch_size]:
            item = {"row": row, "file": row.filename}
            if "v" in mod:
                fn = os.path.join(args.feature_dir, row.filename + ".npy")
                if not os.path.exists(fn):
                    print("Visual feats file does not exist: ", fn)
                    continue
                item["feats"] = np.load(fn).astype(np.float32)
                if item["feats"].ndim != 2 or item["feats"].shape[1] != 1024:
                    continue
            if "a" in mod:
                # the reference's dataset reads <video_dir>/<file>.wav and computes the log-mel itself (dataset.py:229-235,279-298);
                # a precomputed <file>.mel.npy (4T,80) takes precedence, else the .wav goes through the GPU front end (jg_logmel)
                fn = os.path.join(args.video_dir, row.filename + ".mel.npy")
                wav_fn = os.path.join(args.video_dir, row.filename + ".wav")
                if os.path.exists(fn):
                    item["mel"] = np.load(fn).astype(np.float32)
                elif os.path.exists(wav_fn):
                    try:
                        item["mel"] = _wav_mel(wav_fn, eng)[0].cpu().numpy()
                    except Exception:                      # dataset.py:296-298: a wav that cannot be read drops the sample
                        print("Error loading audio, check the file: ", wav_fn)
                        continue
                else:
                    print("Audio file does not exist: ", wav_fn)
                    continue
            if "a" in mod and item["mel"].shape[0] < 4:
                # under 4 mel frames (< 40 ms) the audio CNN has no output step: the reference's per-sample run raises inside its word
                # pooling and the sample is skipped (jegal.py:230-239; the engine's ragged batch call rejects such a clip, and one
                # bad clip must not abort the other fifteen of the batch)
                print("Audio too short ({} mel frames), skipping: {}".format(item["mel"].shape[0], row.filename))
                continue
            if "t" in mod and xlmr is None:
                fn = os.path.join(args.text_states_dir or args.video_dir, row.filename.replace("/", "__") + ".npz")
                if not os.path.exists(fn):
                    print("Text states file does not exist: ", fn)
                    continue
                item["text"] = _load_text_pack(fn)
            batch.append(item)
        if not batch:
            continue
        n = len(batch)
        vis = mask = audio = text = None
        wbs = [M.boundary_list(it["row"].word_boundaries) for it in batch] if mod != "v" else None
        if "v" in mod:                                # pad_sequence + mask (dataset.py:336-340)
            T = max(it["feats"].shape[0] for it in batch)
            vis = torch.zeros((n, T, 1024))
            mask = torch.zeros((n, T))
            for i, it in enumerate(batch):
                t = it["feats"].shape[0]
                vis[i, :t] = torch.from_numpy(it["feats"])
                mask[i, :t] = 1
        if "a" in mod:
            Tm = max(it["mel"].shape[0] for it in batch)
            audio = torch.zeros((n, Tm, 80))
            for i, it in enumerate(batch):
                audio[i, :it["mel"].shape[0]] = torch.from_numpy(it["mel"])
        if "t" in mod and xlmr is not None:
            # phrases -> tokenizer (host) -> XLM-RoBERTa on the engine: get_roberta_embeddings (models/jegal.py:116-129) for the whole
            # batch; the key padding mask and the position ids from the non-pad tokens keep every clip's rows independent of the padding
            from .xlmr import roberta_embeddings
            text = roberta_embeddings(xlmr, tok, [str(it["row"].phrase) for it in batch])
        elif "t" in mod:
            L = max(it["text"][0].shape[0] for it in batch)
            st = np.zeros((n, L, 768), np.float32)
            tm = np.zeros((n, L), np.int64)
            ids = np.ones((n, L), np.int64)
            offs = np.zeros((n, L, 2), np.int64)
            for i, it in enumerate(batch):
                l = it["text"][0].shape[0]
                st[i, :l], tm[i, :l], ids[i, :l], offs[i, :l] = it["text"]
            tbatch = [str(it["row"].phrase).split(" ") for it in batch]
            text = (torch.from_numpy(st), torch.from_numpy(tm), tbatch, ids, offs)
        am = alens = None
        if audio is not None:
            alens = [it["mel"].shape[0] for it in batch]
            am = torch.zeros((n, eng.audio_len(audio.shape[1])))
            for i, l in enumerate(alens):
                am[i, :l // 4] = 1                    # dataset.py:291 (unused by the model, kept for the signature)
        # per_clip=True: the reference runs this script with batch_size=1 (extract_jegal_embs.py:141), so a clip's result must not
        # depend on the clips it happens to be batched with here -- the last word's text range ends at the clip's own token
        # count and the audio conv stack sees every clip's own zero padding (jegal_amd/jegal.py, jg_jegal_audio_ragged)
        out = jg.forward_inference(visual_feats=vis, visual_mask=mask, text=text, audio=audio, audio_mask=am, word_boundaries=wbs,
                                   audio_lens=alens, per_clip=True)
        gesture, content = _gesture_content(out, vis is not None, text is not None or audio is not None)
        for i, it in enumerate(batch):
            g = c = None
            if gesture is not None:                   # strip padded query rows
                g = eng.l2norm(gesture[i, :it["feats"].shape[0]]).cpu().numpy()
            if content is not None:                   # strip padded word rows
                c = eng.l2norm(content[i, :len(wbs[i])]).cpu().numpy()
            with open(extract.pkl_name(res_dir, it["file"]), "wb") as f:
                pickle.dump({"gesture_emb": g, "content_emb": c, "info": it["row"]}, f)
            saved += 1
    print("Saved {} files".format(saved))
    print("Saved JEGAL features at: ", res_dir)
    return 0


# --------------------------------------------------------------------------- evaluators
def _load_pkls(path):
    files = sorted(glob.glob("{}/*.pkl".format(path)))
    print("No of files = ", len(files))
    return files, [_load_pkl(fn) for fn in files]


_RETRIEVAL_LINE = "R@1: {:.2f} - R@5: {:.2f} - R@10: {:.2f} - R@25: {:.2f} - R@50: {:.2f} | Median R: {:.1f}"


def cmd_evaluate_retrieval(argv, engine=None):
    """evaluate_retrieval.py.  --score coupling: the same two lines with the late-interaction score (every word's best frame in the clip,
    metrics.coupling_retrieval_metrics) in place of the cosine of the pooled vectors; --score ordered: that score with the words taking
    frames in word order (jg_sim_ordered); either in one process only.  engine: the Engine to run on (default: this process's)."""
    p = argparse.ArgumentParser(prog="evaluate_retrieval")
    p.add_argument("--path", required=True)
    p.add_argument("--score", default="pooled", choices=["pooled", "coupling", "ordered"],
                   help="pooled: the cosine of the clip-level means, as the reference; coupling: every word's best frame (late interaction); "
                        "ordered: the same with the words' frames in word order")
    args = p.parse_args(argv)
    eng = _engine(engine, args)
    if args.score != "pooled" and jdist.world_size() > 1:
        raise SystemExit("--score {} runs in one process: it is not sharded over ranks".format(args.score))
    _, feats = _load_pkls(args.path)
    if args.score != "pooled":
        both = M.coupling_retrieval_metrics([f["content_emb"] for f in feats], [f["gesture_emb"] for f in feats], engine=eng,
                                            **({"ordered": True} if args.score == "ordered" else {}))
        res = {"Content to Gesture": both["c2g"], "Gesture to Content": both["g2c"]}
        for name, m in res.items():
            print("{} Retrieval scores:".format(name))
            print(_RETRIEVAL_LINE.format(m["R1"] * 100, m["R5"] * 100, m["R10"] * 100, m["R25"] * 100, m["R50"] * 100, m["MR"]))
        return res
    lo, hi = jdist.shard_range(len(feats))
    g = M.video_level(eng, [f["gesture_emb"] for f in feats[lo:hi]])
    c = M.video_level(eng, [f["content_emb"] for f in feats[lo:hi]])
    res = {}
    for name, (a, b) in (("Content to Gesture", (c, g)), ("Gesture to Content", (g, c))):
        m = M.retrieval_metrics(a, b, engine=eng)
        res[name] = m
        if jdist.rank() == 0:
            print("{} Retrieval scores:".format(name))
            print(_RETRIEVAL_LINE.format(m["R1"] * 100, m["R5"] * 100, m["R10"] * 100, m["R25"] * 100, m["R50"] * 100, m["MR"]))
    return res


def cmd_evaluate_spotting(argv):
    p = argparse.ArgumentParser(prog="evaluate_spotting")
    p.add_argument("--path", required=True)
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--frame_threshold", type=int, default=9)
    args = p.parse_args(argv)
    eng, _, _ = _models(args)
    _, feats = _load_pkls(args.path)
    lo, hi = jdist.shard_range(len(feats))
    feats = feats[lo:hi]
    acc = M.spotting_accuracy([f["gesture_emb"] for f in feats], [f["content_emb"] for f in feats],
                              [f["info"]["word_boundaries"] for f in feats],
                              [f["info"]["target_word_boundary"] for f in feats],
                              thresh=args.threshold, frame_thresh=args.frame_threshold, engine=eng)
    if jdist.rank() == 0:
        print("Word Spotting Accuracy: {}".format(acc))
    return acc


def cmd_evaluate_asd(argv):
    import pandas as pd
    p = argparse.ArgumentParser(prog="evaluate_asd")
    p.add_argument("--path", required=True)
    p.add_argument("--file", required=True)
    args = p.parse_args(argv)
    eng, _, _ = _models(args)
    df = pd.read_csv(args.file)
    print("Total files: {}".format(len(df)))

    def load(fname):
        fn = extract.pkl_name(args.path, fname)
        return _load_pkl(fn) if os.path.exists(fn) else None

    queries, cands = [], []
    lo, hi = jdist.shard_range(len(df))           # queries sharded over the ranks (contiguous blocks), counters all-reduced
    for i in range(lo, hi):
        row = df.iloc[i]
        q = load(row.filename)
        if q is None:
            continue
        cs = [np.asarray(q["gesture_emb"], np.float32).mean(axis=0)]
        for neg in ast.literal_eval(row.neg_files):
            d = load(neg)
            if d is not None:
                cs.append(np.asarray(d["gesture_emb"], np.float32).mean(axis=0))
        queries.append(np.asarray(q["content_emb"], np.float32).mean(axis=0))
        cands.append(np.stack(cs))
    a2, a4, a6 = M.asd_accuracy(np.stack(queries) if queries else np.zeros((0, 512), np.float32), cands, engine=eng)
    total = M.reduce_counts([len(queries)], eng.device)[0]
    if jdist.rank() == 0:
        print("Total videos evaluated: {}".format(total))
        for k, a in ((2, a2), (4, a4), (6, a6)):
            print("{} spk: Acc: {:.3f}".format(k, a))
    return a2, a4, a6


def cmd_attn_matrix(argv, engine=None):
    """utils/plot_heatmap.py without the matplotlib rendering: the gesture-word attention matrix of one feature .pkl, or of every .pkl of
    a directory (one jg_attn_matrix call for all of them).  Per clip ``<res_dir>/<name>.attn.npz`` = {attn (W,T) float32, words,
    best_frame (W,) int32, best_score (W,) float32}; <name> is --fname for a single file (plot_heatmap's flag), the .pkl's own name
    otherwise.  --normalize 0 (default) is what plot_heatmap.py computes on the stored, already normalised embeddings; 1 re-normalises the
    rows first (evaluate_spotting.py:39-57).  engine: the Engine to run on (default: this process's)."""
    p = argparse.ArgumentParser(prog="attn_matrix")
    p.add_argument("--path", required=True, help="a JEGAL feature .pkl, or a directory of them")
    p.add_argument("--fname", default=None, help="name of the output for a single .pkl (default: the .pkl's name)")
    p.add_argument("--res_dir", default=".")
    p.add_argument("--normalize", type=int, default=0, choices=[0, 1])
    p.add_argument("--temp", type=float, default=0.07)
    args = p.parse_args(argv)
    if os.path.isdir(args.path):
        files, feats = _load_pkls(args.path)
        names = [_base_name(f) for f in files]
    else:
        feats = [_load_pkl(args.path)]
        names = [args.fname or _base_name(args.path)]
    if not feats:
        raise SystemExit("no .pkl under {}".format(args.path))
    words = [_feature_words(ft) for ft in feats]
    eng = _engine(engine, args)
    mats, best = M.attn_call([np.asarray(ft["gesture_emb"], np.float32) for ft in feats],
                             [np.asarray(ft["content_emb"], np.float32) for ft in feats],
                             args.temp, bool(args.normalize), eng, None, True)          # matrices and best_* from ONE call
    os.makedirs(args.res_dir, exist_ok=True)
    for name, a, w, (bf, bs) in zip(names, mats, words, best):
        M.check_word_count(len(w), a.shape[0], name)
        out = os.path.join(args.res_dir, name + ".attn.npz")
        np.savez(out, attn=a, words=np.asarray(w), best_frame=bf, best_score=bs)
        print("Attn mtx: ", a.shape, " -> ", out)
    return 0


RETRIEVE_DIRECTIONS = {"c2g": ("Content to Gesture", "content_emb", "gesture_emb"), "g2c": ("Gesture to Content", "gesture_emb", "content_emb")}


def cmd_retrieve(argv, engine=None):
    """The retrieval that evaluate_retrieval only grades: for every clip of a directory of feature .pkl files (loaded, pooled and sharded as
    evaluate_retrieval does) the --topk best clips of the other modality.  Rank 0 writes ``<res_dir>/retrieve_<direction>.npz`` = {names (N,):
    the .pkl base names = the gallery order, idx (N,K) int32 gallery rows best first (-1 where N < K), score (N,K) float32, rank (N,)
    int32: jg_sim_rank's rank of the clip's own partner from the same normalised rows}.  engine: the Engine to run on (default: this
    process's)."""
    p = argparse.ArgumentParser(prog="retrieve")
    p.add_argument("--path", required=True, help="a directory of JEGAL feature .pkl files")
    p.add_argument("--topk", type=int, default=10, help="gallery clips kept per query (1..128)")
    p.add_argument("--direction", default="both", choices=["c2g", "g2c", "both"])
    p.add_argument("--res_dir", default=".")
    args = p.parse_args(argv)
    _check_topk(args.topk)
    eng = _engine(engine, args)
    files, feats = _load_pkls(args.path)
    if not feats:
        raise SystemExit("no .pkl under {}".format(args.path))
    names = np.asarray([_base_name(f) for f in files])
    lo, hi = jdist.shard_range(len(feats))
    pooled = {key: M.video_level(eng, [f[key] for f in feats[lo:hi]]) for key in ("gesture_emb", "content_emb")}
    res = {}
    for d in (["c2g", "g2c"] if args.direction == "both" else [args.direction]):
        title, qk, gk = RETRIEVE_DIRECTIONS[d]
        idx, score = M.retrieve(pooled[qk], pooled[gk], k=args.topk, engine=eng)
        rank = M.partner_ranks(pooled[qk], pooled[gk], engine=eng)
        res[d] = dict(names=names, idx=idx, score=score, rank=rank)
        if jdist.rank() == 0:
            os.makedirs(args.res_dir, exist_ok=True)
            out = os.path.join(args.res_dir, "retrieve_{}.npz".format(d))
            np.savez(out, **res[d])
            print("{} retrieval: top-{} of {} clips, own partner ranked under {} for {} -> {}".format(
                title, args.topk, len(names), args.topk, int(np.sum(rank < args.topk)), out))
    return 0


def _corpus_clips(path):
    """the corpus under `path`: (names (N,): the .pkl base names in sorted order = the clip numbering, [gesture_emb (T_i, D) float32])"""
    files, feats = _load_pkls(path)
    feats = [(fn, ft) for fn, ft in zip(files, feats) if ft.get("gesture_emb") is not None]
    if not feats:
        raise SystemExit("no .pkl with gesture_emb under {}".format(path))
    return (np.asarray([_base_name(fn) for fn, _ in feats]),
            [np.asarray(ft["gesture_emb"], np.float32) for _, ft in feats])


def cmd_index(argv, engine=None):
    """Prepare a corpus for search --index: every gesture_emb of the .pkl files under --path (names and clip numbering as search --path
    has them), the rows L2-normalised (--normalize 1) and rounded to --dtype, written as one .npz (metrics.Corpus).  float16 halves the
    file, the upload and the device memory; the search then scores the rows as stored.  engine: the Engine to run on."""
    p = argparse.ArgumentParser(prog="index")
    p.add_argument("--path", required=True, help="a directory of JEGAL feature .pkl files: the corpus")
    p.add_argument("--out", required=True, help="the corpus file to write (.npz)")
    p.add_argument("--dtype", default="float16", choices=["float16", "float32"])
    p.add_argument("--normalize", type=int, default=1, choices=[0, 1], help="1: unit rows (cosine similarity); 0: the rows as stored")
    args = p.parse_args(argv)
    names, clips = _corpus_clips(args.path)
    eng = _engine(engine, args) if engine is not None or args.normalize else None
    corpus = M.Corpus.build(clips, names=names, dtype=args.dtype, normalize=bool(args.normalize), engine=eng)
    out = args.out if args.out.endswith(".npz") else args.out + ".npz"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    corpus.save(out)
    print("index: {} clips, {} rows x {} {} -> {}".format(len(names), corpus.rows.shape[0], corpus.rows.shape[1], args.dtype, out))
    return 0


def cmd_search(argv, engine=None):
    """For this word, or this phrase, which clips of a corpus gesture it, and at which frame: the query rows are the --query .pkl's
    content_emb rows (--level word: one query per word) or their mean (--level phrase: one query), the gallery is every gesture_emb row of
    the .pkl files under --path, a clip scores as its best frame (metrics.search, jg_sim_topk_grouped).  --segment N: runs of N frames
    score on their own, so a long clip can come back with several moments.  Writes ``<res_dir>/search_<query name>.npz`` = {words (Q,): the
    query's words (phrase: the words joined), names (N,): the .pkl base names = the clip numbering, clip (Q,K) int32, frame (Q,K) int32:
    the frame inside the clip, score (Q,K) float32; -1 / -1 / -inf where fewer than K groups exist} and prints one line per query row.
    --index FILE instead of --path: the corpus is one written by the index command (metrics.Corpus, jg_sim_search): prepared once, maybe
    in 16 bits, the same output.  --level coupling: the query's words stay separate rows of ONE query of at most 64 words, and a clip (or
    segment) scores as the mean over the words of each word's best frame in it (metrics.search_phrases, jg_sim_coupling); the .npz also
    holds start (1,K) = the first frame of the returned group inside its clip, and `frame` repeats it.  --level ordered: as coupling, with
    the words taking frames of the group in word order (jg_sim_ordered).  --align (coupling and ordered): the .npz also holds word_frame
    (1,K,W) int32, the frame inside the returned clip that every word took (jg_sim_align), and the printed line shows each word with its
    frame.  engine: the Engine to run on (default: this process's)."""
    p = argparse.ArgumentParser(prog="search", description="Single process: sharding over ranks is not built for this command.")
    p.add_argument("--path", default=None, help="a directory of JEGAL feature .pkl files: the corpus (or --index)")
    p.add_argument("--index", default=None, help="a corpus written by the index command, instead of --path: prepared once, maybe in 16 bits")
    p.add_argument("--query", required=True, help="a JEGAL feature .pkl whose content_emb rows are the query")
    p.add_argument("--level", default="word", choices=["word", "phrase", "coupling", "ordered"])
    p.add_argument("--align", action="store_true", help="--level coupling / ordered: also the frame every word took in each returned clip")
    p.add_argument("--topk", type=int, default=10, help="clips (or segments) kept per query row (1..128)")
    p.add_argument("--segment", type=int, default=0, help="frames per group; 0: a clip is one group")
    p.add_argument("--normalize", type=int, default=1, choices=[0, 1], help="1: cosine similarity (rows re-normalised); 0: the rows as stored")
    p.add_argument("--max_rows", type=int, default=None, help="gallery rows on the device at a time (default: all)")
    p.add_argument("--res_dir", default=".")
    args = p.parse_args(argv)
    _check_topk(args.topk)
    if args.segment < 0:
        raise SystemExit("--segment must be >= 0")
    if (args.path is None) == (args.index is None):
        raise SystemExit("exactly one of --path and --index")
    qf = _load_pkl(args.query)
    if qf.get("content_emb") is None:
        raise SystemExit("{} holds no content_emb".format(args.query))
    queries = np.asarray(qf["content_emb"], np.float32)
    words = _feature_words(qf)
    if words is None:
        words = ["word{}".format(i) for i in range(len(queries))]
    M.check_word_count(len(words), len(queries), args.query)
    if args.level == "phrase":
        queries, words = queries.mean(axis=0, keepdims=True), [" ".join(words)]
    coupling = args.level in ("coupling", "ordered")
    if args.align and not coupling:
        raise SystemExit("--align goes with --level coupling or --level ordered")
    more = {}                                    # (keywords only where asked for: an engine or a corpus of before is called as before)
    if args.level == "ordered":
        more["order"] = True
    if args.align:
        more["align"] = True
    word_list = list(words)
    if coupling:                                 # the words stay separate rows of ONE query
        if not 1 <= len(queries) <= COUPLING_MAX_W:
            raise SystemExit("--level {} takes a query of 1..{} words, not {}".format(args.level, COUPLING_MAX_W, len(queries)))
        queries, words = [queries], [" ".join(words)]
    if args.index is not None:                   # (its rows were normalised, or not, when it was built: --normalize is about the query)
        corpus = M.Corpus.load(args.index)
        names = corpus.names
        eng = _engine(engine, args)
        clip, frame, score, *rest = (corpus.search_phrases if coupling else corpus.search)(
            queries, k=args.topk, segment=args.segment, normalize=bool(args.normalize), engine=eng, max_rows=args.max_rows, **more)
    else:
        names, clips = _corpus_clips(args.path)
        eng = _engine(engine, args)
        clip, frame, score, *rest = (M.search_phrases if coupling else M.search)(
            queries, clips, k=args.topk, segment=args.segment, normalize=bool(args.normalize), engine=eng, max_rows=args.max_rows, **more)
    os.makedirs(args.res_dir, exist_ok=True)
    out = os.path.join(args.res_dir, "search_{}.npz".format(_base_name(args.query)))
    if coupling:                                 # a group comes back, not a frame: `frame` is its first one, under both names
        np.savez(out, words=np.asarray(words), names=names, clip=clip, start=frame, frame=frame, score=score,
                 **({"word_frame": rest[0]} if args.align else {}))
    else:
        np.savez(out, words=np.asarray(words), names=names, clip=clip, frame=frame, score=score)
    for i, w in enumerate(words):
        hits = ["{}@{} ({:.3f})".format(names[c], f, s) for c, f, s in zip(clip[i][:3], frame[i][:3], score[i][:3]) if c >= 0]
        if args.align:                           # ... and every word with the frame it took
            hits = ["{} [{}]".format(h, " ".join("{}@{}".format(wd, t) for wd, t in zip(word_list, rest[0][i][r]))) for r, h in enumerate(hits)]
        print("search: \"{}\" -> {} of {} clips: {}".format(w, int(np.sum(clip[i] >= 0)), len(names), ", ".join(hits) or "nothing"))
    print("search: {} query rows x top-{} -> {}".format(len(words), args.topk, out))
    return 0


def cmd_asd(argv, engine=None):
    """The detection that evaluate_asd only grades: for every row of the csv whose feature .pkl exists, the probability that each of its
    candidates -- the query clip first, then its neg_files that exist, as evaluate_asd builds the list -- gestures to the query's speech.
    Writes ``<res_dir>/asd.npz`` = {names (N,): the queries' .pkl base names, cand_names (sum P,), cand_offsets (N + 1,), prob (sum P,)
    float32: query i's probabilities are prob[cand_offsets[i] : cand_offsets[i + 1]], pred (N,) int32: the winner's place in the list (0 =
    the query's own clip)}.  With --win also the timeline of every query, ``<res_dir>/<name>.asd.npz`` = {candidates (P,), start (n_win,)
    int32, prob (n_win, P) float32, pred (n_win,) int32}: windows of --win frames, --hop apart, on the query's word boundaries.  A clip
    that is a candidate of many queries is on the device once.  engine: the Engine to run on (default: this process's)."""
    import pandas as pd
    p = argparse.ArgumentParser(prog="asd", description="Single process: sharding over ranks is not built for this command.")
    p.add_argument("--path", required=True, help="a directory of JEGAL feature .pkl files")
    p.add_argument("--file", required=True, help="the csv of evaluate_asd: filename, neg_files")
    p.add_argument("--win", type=int, default=None, help="frames per window: also write every query's timeline (1..8192)")
    p.add_argument("--hop", type=int, default=5, help="frames between window starts")
    p.add_argument("--temp", type=float, default=0.07)
    p.add_argument("--res_dir", default=".")
    args = p.parse_args(argv)
    if args.win is not None and (not 1 <= args.win <= 8192 or args.hop < 1):
        raise SystemExit("--win must be 1..8192 and --hop >= 1")
    df = pd.read_csv(args.file)
    print("Total files: {}".format(len(df)))
    stem = lambda fname: _base_name(extract.pkl_name("", fname))
    feats, track_of, tracks = {}, {}, []

    def load(fname):
        if fname not in feats:
            fn = extract.pkl_name(args.path, fname)
            feats[fname] = None
            if os.path.exists(fn):
                feats[fname] = _load_pkl(fn)
                track_of[fname] = len(tracks)
                tracks.append(np.asarray(feats[fname]["gesture_emb"], np.float32))
        return feats[fname]

    names, cand_names, contents, bounds, trk, s_off = [], [], [], [], [], [0]
    for i in range(len(df)):
        row = df.iloc[i]
        q = load(row.filename)
        if q is None:
            continue
        cands = [row.filename] + [neg for neg in ast.literal_eval(row.neg_files) if load(neg) is not None]
        if len(cands) > 64:
            raise SystemExit("{}: {} candidates; jg_asd_windows takes at most 64 per query".format(row.filename, len(cands)))
        names.append(stem(row.filename))
        cand_names.append([stem(c) for c in cands])
        contents.append(np.asarray(q["content_emb"], np.float32))
        bounds.append(q["info"]["word_boundaries"])
        trk += [track_of[c] for c in cands]
        s_off.append(len(trk))
    if not names:
        raise SystemExit("no query of {} has a .pkl under {}".format(args.file, args.path))
    eng = _engine(engine, args)
    g, c = M.cat_rows(tracks), M.cat_rows(contents)
    goff, coff = M.offsets_of(tracks), M.offsets_of(contents)
    prob, _, pred, _, _ = eng.asd_windows(g, goff, c, coff, trk, s_off, win=0, temp=args.temp)
    os.makedirs(args.res_dir, exist_ok=True)
    out = os.path.join(args.res_dir, "asd.npz")
    pred = M.to_host(pred).astype(np.int32)
    np.savez(out, names=np.asarray(names), cand_names=np.asarray([c for cs in cand_names for c in cs]), cand_offsets=np.asarray(s_off, np.int64),
             prob=M.to_host(prob), pred=pred)
    print("ASD: {} queries, own clip chosen for {} -> {}".format(len(names), int(np.sum(pred == 0)), out))
    if args.win is not None:
        start, end = M.batch_bounds(bounds, contents, names)
        prob, p_off, pred, w_off, _ = eng.asd_windows(g, goff, c, coff, trk, s_off, win=args.win, hop=args.hop, temp=args.temp,
                                                      word_start=start, word_end=end)
        prob, pred = M.to_host(prob), M.to_host(pred)
        for i, name in enumerate(names):
            w = M.span(w_off, i)
            n_win = w.stop - w.start
            np.savez(os.path.join(args.res_dir, name + ".asd.npz"), candidates=np.asarray(cand_names[i]),
                     start=M.window_starts(n_win, args.win, args.hop), prob=prob[M.span(p_off, i)].reshape(n_win, len(cand_names[i])),
                     pred=pred[w].astype(np.int32))
        print("ASD timelines: win {} hop {} -> {}/<name>.asd.npz".format(args.win, args.hop, args.res_dir))
    return 0


SYNC_OFFSET_NOTE = ("The released GestSync checkpoint was trained on its authors' own mel normalisation, which is not in the reference tree: "
                    "--wav goes through this library's log-mel front end (JEGAL's), whose parity with GestSync's is unpinned -- pass the "
                    "authors' mel with --mel for a real checkpoint.  Parity of the network itself is pinned (GestSync.forward_aud).")


def _sync_streams(args, engine, gestsync):
    """What both forms of sync_offset start from: the synthetic-weights warning, the models, the (T,1024) video rows of every --frames
    file and the (Ta,1024) audio rows of the one --wav / --mel -> (engine, [video rows], audio rows), on the device."""
    if args.checkpoint_path_gestsync == "synthetic":
        print("WARNING: synthetic GestSync weights: their window embeddings are 0.93-0.996 correlated whatever the input, so the offset "
              "and confidence below are MEANINGLESS as a sync measurement; pass a trained checkpoint.")
    if gestsync is None:
        engine, gestsync, _ = _models(args, need_gestsync=True)
    eng = engine if engine is not None else gestsync.engine
    vids = []
    for path in args.frames:
        frames = np.load(path)
        if frames.ndim != 4 or tuple(frames.shape[1:]) != (270, 480, 3) or frames.dtype != np.uint8:
            raise ValueError("--frames must hold (T,270,480,3) uint8 masked crops")
        vids.append(gestsync.extract_clip_feats(torch.from_numpy(frames).to(eng.device))[0])
    if args.mel is not None:
        mel = torch.from_numpy(np.load(args.mel).astype(np.float32))
        if mel.dim() != 2 or mel.shape[1] != 80 or mel.shape[0] < 1:
            raise ValueError("--mel must hold (Tm,80) mel rows")
        mel = mel[None].to(eng.device)
    else:
        mel = _wav_mel(args.wav, eng)
    T = max(int(v.shape[0]) for v in vids)
    Ta = max(1, min(T, -(-int(mel.shape[1]) // 4)))            # audio windows: one per frame the mel covers
    return eng, vids, gestsync.extract_clip_audio_feats(mel, Ta)[0]


def _sync_offset_over_time(args, engine, gestsync):
    """sync_offset with --win (the offset as a function of time: metrics.sync_timeline) and / or several --frames (which track is in sync
    with the audio: metrics.sync_speaker); every track's ``<name>.sync.npz`` gains start, offset_t, conf_t, curve_t beside the clip-level
    offset, conf, curve, shifts."""
    eng, vids, aud = _sync_streams(args, engine, gestsync)
    hop = args.hop if args.hop > 0 else max(1, args.win // 5)
    Ta = int(aud.shape[0])
    n = len(vids)
    clip = M.sync_timeline(vids, [aud], win=0, max_shift=args.max_shift, min_overlap=args.min_overlap, audio_of=[0] * n, engine=eng)
    line = M.sync_timeline(vids, [aud], win=args.win, hop=hop, max_shift=args.max_shift, min_overlap=args.min_overlap, audio_of=[0] * n,
                           engine=eng)
    os.makedirs(args.res_dir, exist_ok=True)
    shifts = np.arange(-args.max_shift, args.max_shift + 1, dtype=np.int32)
    for f, v, c, t in zip(args.frames, vids, clip, line):
        out = os.path.join(args.res_dir, _base_name(f) + ".sync.npz")
        np.savez(out, offset=c["offset"][0], conf=c["conf"][0], curve=c["curve"][0], shifts=shifts, start=t["start"], offset_t=t["offset"],
                 conf_t=t["conf"], curve_t=t["curve"])
        print("AV offset: {} frames   confidence: {:.4f}   ({} video / {} audio windows) -> {}".format(
            int(c["offset"][0]), float(c["conf"][0]), int(v.shape[0]), Ta, out))
        ok = ~np.isnan(t["conf"])
        if ok.any():                    # confident: at least half the best window's confidence
            ok &= np.nan_to_num(t["conf"], nan=-np.inf) >= 0.5 * np.nanmax(t["conf"])
        if ok.any():
            o = t["offset"][ok]
            step = np.abs(np.diff(t["offset"].astype(np.int64))) if len(t["offset"]) > 1 else np.zeros(0, np.int64)
            at = int(t["start"][1 + int(np.argmax(step))]) if step.size and step.max() > 0 else -1
            print("  over time (win {} hop {}, {} windows): median offset {:g}, min {} / max {} over the {} confident windows{}".format(
                args.win, hop, len(t["offset"]), float(np.median(o)), int(o.min()), int(o.max()), int(ok.sum()),
                ", largest change at frame {}".format(at) if at >= 0 else ", no change"))
        else:
            print("  over time (win {} hop {}): no window with a shift".format(args.win, hop))
    if n > 1:
        speaker, conf = M.sync_speaker(vids, aud, win=args.win, hop=hop, max_shift=args.max_shift, min_overlap=args.min_overlap, engine=eng)
        names = [_base_name(f) for f in args.frames]
        start = M.window_starts(len(speaker), args.win, hop)
        for j, s in enumerate(speaker):
            print("  window {} (frame {}): in sync: {}".format(j, start[j], names[s] if s >= 0 else "-"))
        np.savez(os.path.join(args.res_dir, "sync_speaker.npz"), tracks=np.asarray(names), speaker=speaker, conf=conf, start=start)
    return 0


def cmd_sync_offset(argv, engine=None, gestsync=None):
    """Audio-visual offset of one clip: the thin composition of GestSync.extract_clip_feats (frames -> (T,1024)), the log-mel front end
    (--wav, Engine.logmel) or a caller's mel (--mel: (4T,80) fp32, time-major, 4 mel steps per frame), GestSync.extract_clip_audio_feats
    (mel -> (T,1024)) and metrics.sync_offset.  Prints the offset in frames (d > 0: the audio matching frame t is found d frames later,
    i.e. the audio track lags) and the confidence; writes ``<res_dir>/<name>.sync.npz`` = {offset, conf, curve (2 max_shift + 1,),
    shifts}.  --win N [--hop M]: the offset over time as well (_sync_offset_over_time: metrics.sync_timeline); --frames given several
    times: candidate tracks against the one audio, the in-sync track per window (metrics.sync_speaker).  Without either: the output of
    before, byte for byte."""
    p = argparse.ArgumentParser(prog="sync_offset", epilog=SYNC_OFFSET_NOTE)
    p.add_argument("--checkpoint_path_gestsync", required=True,
                   help="GestSync checkpoint with its audio stream; 'synthetic' = the seeded test weights, whose embeddings carry NO sync "
                        "signal (the result then only shows that the path runs)")
    p.add_argument("--frames", required=True, action="append",
                   help=".npy of masked uint8 crops (T,270,480,3); several --frames: candidate tracks of one scene against the one --wav / --mel")
    p.add_argument("--wav", default=None, help="16 kHz mono .wav of the clip (log-mel on the GPU). " + SYNC_OFFSET_NOTE)
    p.add_argument("--mel", default=None, help=".npy (Tm,80) fp32 time-major mel of the clip, 4 steps per frame: used instead of --wav")
    p.add_argument("--max_shift", type=int, default=15)
    p.add_argument("--min_overlap", type=int, default=1)
    p.add_argument("--win", type=int, default=0, help="frames per window of the offset timeline (0: one offset for the clip)")
    p.add_argument("--hop", type=int, default=0, help="frames between window starts (default: win / 5)")
    p.add_argument("--res_dir", default=".")
    _add_precision_args(p)
    args = p.parse_args(argv)
    if (args.wav is None) == (args.mel is None):
        raise SystemExit("sync_offset: give --wav or --mel (one of them)")
    if args.win < 0 or args.hop < 0:
        raise SystemExit("sync_offset: --win and --hop must be >= 0")
    if args.win > 0 or len(args.frames) > 1:
        return _sync_offset_over_time(args, engine, gestsync)
    eng, (vid,), aud = _sync_streams(args, engine, gestsync)
    T, Ta = int(vid.shape[0]), int(aud.shape[0])
    off, conf, curve = M.sync_offset([vid], [aud], args.max_shift, args.min_overlap, engine=eng)
    os.makedirs(args.res_dir, exist_ok=True)
    out = os.path.join(args.res_dir, _base_name(args.frames[0]) + ".sync.npz")
    np.savez(out, offset=off[0], conf=conf[0], curve=curve[0], shifts=np.arange(-args.max_shift, args.max_shift + 1, dtype=np.int32))
    print("AV offset: {} frames   confidence: {:.4f}   ({} video / {} audio windows) -> {}".format(int(off[0]), float(conf[0]), T, Ta, out))
    return 0


def cmd_embed_tracks(argv, engine=None, jegal=None):
    """Gesture embeddings of whole tracks, however long: reads the ``<feature_dir>/<vid>/<track>.npy`` (T,1024) GestSync features that
    extract_gestsync_feats writes, runs JEGAL.forward_gesture_tracks on them (windows of --win emitted frames with --ctx frames of context
    on both sides: include/jegal_hip.h, jg_jegal_gesture_tracks) and writes ``<result_dir>/v/<vid>__<track>.pkl`` = {"gesture_emb": (T,512)
    unit rows, "content_emb": None, "info": {"fname", "win", "ctx"}} -- the file search, asd and spot_talk read.  Tracks are packed into
    engine calls of at most --rows_per_call frames (a longer track goes alone); a track's rows do not depend on what it is packed with.
    engine / jegal: an Engine and a loaded JEGAL to run on (default: this process's, loaded from --checkpoint_path_jegal)."""
    p = argparse.ArgumentParser(prog="embed_tracks")
    p.add_argument("--checkpoint_path_jegal", required=True)
    p.add_argument("--feature_dir", required=True, help="<vid>/<track>.npy GestSync features (T,1024)")
    p.add_argument("--result_dir", required=True)
    p.add_argument("--win", type=int, default=120, help="frames a window emits")
    p.add_argument("--ctx", type=int, default=50, help="frames of context a window sees on each side (win + 2 ctx <= 500).  The defaults make spans of "
                                                       "at most 220 frames, the longest clip of the training lists: a choice, not a measured optimum")
    p.add_argument("--rows_per_call", type=int, default=16384, help="frames per engine call (bounds the workspace: ~25 KB per frame at the defaults)")
    p.add_argument("--rank", type=int, default=None)
    p.add_argument("--nshard", type=int, default=None)
    _add_precision_args(p)
    args = p.parse_args(argv)
    if args.win < 1 or args.ctx < 0 or args.win + 2 * args.ctx > 500:
        raise SystemExit("embed_tracks: need --win >= 1, --ctx >= 0 and win + 2 ctx <= 500")
    if jegal is None:
        ns = argparse.Namespace(checkpoint_path=args.checkpoint_path_jegal, precision=args.precision, calibrate_frames=args.calibrate_frames)
        engine, _, jegal = _models(ns, need_jegal=True)
    res_dir = os.path.join(args.result_dir, "v")
    os.makedirs(res_dir, exist_ok=True)
    files = sorted(glob.glob(os.path.join(args.feature_dir, "*", "*.npy")))
    lo, hi = jdist.shard_range(len(files), args.rank, args.nshard)
    print("Total tracks: {} | Start : End = {} : {}".format(len(files), lo, hi))
    saved = err = 0
    todo = []
    for f in files[lo:hi]:
        fname = f.split("/")[-2] + "/" + os.path.basename(f)[:-len(".npy")]
        out = extract.pkl_name(res_dir, fname)
        if os.path.exists(out):                      # resume: skip-if-exists, as extract_gestsync_feats
            saved += 1
            continue
        try:
            feats = np.load(f)
            if feats.ndim != 2 or feats.shape[1] != 1024 or feats.shape[0] < 1:
                raise ValueError("expected a (T,1024) feature .npy, got {}".format(feats.shape))
            todo.append((np.ascontiguousarray(feats, np.float32), fname, out))
        except Exception as e:
            err += 1
            print("Error: ", e, " | Feature file: ", f)

    def run_group(group):
        embs = jegal.forward_gesture_tracks([torch.from_numpy(ft) for ft, _, _ in group], win=args.win, ctx=args.ctx, normalize=True)
        return [e.cpu().numpy() for e in embs]

    def save_one(emb, item):
        with open(item[2], "wb") as f:
            pickle.dump({"gesture_emb": emb, "content_emb": None, "info": {"fname": item[1], "win": args.win, "ctx": args.ctx}}, f)

    cap = max(1, args.rows_per_call)
    groups, s0 = [], 0
    while s0 < len(todo):
        s1, rows = s0 + 1, todo[s0][0].shape[0]
        while s1 < len(todo) and rows + todo[s1][0].shape[0] <= cap:
            rows += todo[s1][0].shape[0]
            s1 += 1
        groups.append(todo[s0:s1])
        s0 = s1
    done, failed = _run_groups(groups, run_group, save_one, "Track")
    print("No of files saved = {} | Err = {}".format(saved + done, err + failed))
    print("Saved JEGAL gesture embeddings at: ", res_dir)
    return 0


SPOT_TALK_NOTE = ("--reach 110 is half the longest clip of the training lists (220 frames): every frame sees the words a clip of that length "
                  "centred on it would contain.  It is a choice, not a measured optimum: no trained checkpoint was available to tune it on.")


def cmd_spot_talk(argv, engine=None):
    """The gesture-word heat map of a whole talk, and its word spotting: --gesture is the track's .pkl as embed_tracks writes it (gesture_emb
    (T,512), any T up to 2^20); the words come from --content, one feature .pkl whose content_emb rows and info["word_boundaries"] are on
    the track's frame axis, or from --utterances, a csv with the columns filename and start_frame: every row names an utterance-level
    feature .pkl under --path (``a/b`` -> ``a__b.pkl``, as extract_jegal_embs names them; inference_embs --modalities ta writes the same
    from wav and text alone) and the frame of the talk at which it begins (metrics.talk_words).  One jg_attn_talk call.  Writes
    ``<res_dir>/<name>.talk.npz`` = {words (W,), word_start, word_end (W,) int32, first_frame (W,) int32, band (W, 2 reach + longest word)
    float32: band[w][j] = the probability of word w at frame first_frame[w] + j, NaN outside the track or its reach; best_frame (W,) int32,
    best_score (W,) float32; frame_word (T,) int32, frame_prob (T,) float32}; --band 0 leaves first_frame and band out.  <name> is the
    gesture .pkl's own name.  engine: the Engine to run on (default: this process's)."""
    p = argparse.ArgumentParser(prog="spot_talk", description=SPOT_TALK_NOTE)
    p.add_argument("--gesture", required=True, help="the track's .pkl (embed_tracks): gesture_emb (T,512)")
    p.add_argument("--content", default=None, help="a feature .pkl with content_emb (W,512) and word boundaries on the track's frame axis")
    p.add_argument("--utterances", default=None, help="a csv (filename, start_frame) of utterance-level feature .pkl files under --path")
    p.add_argument("--path", default=None, help="the directory of the --utterances files")
    p.add_argument("--reach", type=int, default=110, help="frames around a word within which it competes for a frame.  " + SPOT_TALK_NOTE)
    p.add_argument("--temp", type=float, default=0.07)
    p.add_argument("--normalize", type=int, default=0, choices=[0, 1], help="1: re-normalise the rows first (evaluate_spotting.py:39-57)")
    p.add_argument("--band", type=int, default=1, choices=[0, 1], help="0: best_* and frame_* only")
    p.add_argument("--res_dir", default=".")
    args = p.parse_args(argv)
    if (args.content is None) == (args.utterances is None) or (args.utterances is not None and args.path is None):
        raise SystemExit("spot_talk: give --content C.pkl, or --utterances LIST.csv with --path DIR")

    track = _load_pkl(args.gesture)
    if track.get("gesture_emb") is None:
        raise SystemExit("{} holds no gesture_emb".format(args.gesture))
    gesture = np.asarray(track["gesture_emb"], np.float32)
    if args.content is not None:
        ft = _load_pkl(args.content)
        if ft.get("content_emb") is None:
            raise SystemExit("{} holds no content_emb".format(args.content))
        content, bounds = M.talk_words([ft], [0])
    else:
        import pandas as pd
        df = pd.read_csv(args.utterances)
        stem = lambda fname: "__".join(str(fname).split("/")) + ("" if str(fname).endswith(".pkl") else ".pkl")
        content, bounds = M.talk_words([_load_pkl(os.path.join(args.path, stem(f))) for f in df.filename], [int(s) for s in df.start_frame])
    eng = _engine(engine, args)
    call = M.talk_heatmap if args.band else M.spot_talk
    r = call(gesture, content, bounds, reach=args.reach, temp=args.temp, normalize=bool(args.normalize), engine=eng)
    os.makedirs(args.res_dir, exist_ok=True)
    out = os.path.join(args.res_dir, _base_name(args.gesture) + ".talk.npz")
    np.savez(out, words=np.asarray([b[0] for b in bounds]), word_start=np.asarray([b[1] for b in bounds], np.int32),
             word_end=np.asarray([b[2] for b in bounds], np.int32), **r)
    print("Talk heat map: {} frames, {} words, reach {} -> {}".format(gesture.shape[0], len(bounds), args.reach, out))
    return 0


COMMANDS = {
    "spot_talk": cmd_spot_talk,
    "embed_tracks": cmd_embed_tracks,
    "sync_offset": cmd_sync_offset,
    "attn_matrix": cmd_attn_matrix,
    "retrieve": cmd_retrieve,
    "search": cmd_search,
    "index": cmd_index,
    "asd": cmd_asd,
    "extract_gestsync_feats": cmd_extract_gestsync_feats,
    "extract_jegal_embs": cmd_extract_jegal_embs,
    "evaluate_retrieval": cmd_evaluate_retrieval,
    "evaluate_spotting": cmd_evaluate_spotting,
    "evaluate_asd": cmd_evaluate_asd,
}
COMMANDS["inference_embs"] = lambda argv: cmd_inference_embs(argv)      # (defined below)


# --------------------------------------------------------------------------- inference_embs
def cmd_inference_embs(argv):
    """inference_embs.py (the reference's single-clip driver, :526-646 + the __main__ checks :648-685): one clip in, one
    ``<res_dir>/<fname>.pkl`` = {"gesture_emb" (T,512) | None, "content_emb" (W,512) | None, "info": {fname, word_boundaries, text}} out.

    Upstream of the hot path and NOT rebuilt: video decoding, the mediapipe face mesh and WhisperX.  So --video_path is a ``.npy``:
    the decoded frames (T,H,W,3) uint8 at source resolution with --mask_y (per frame: last blanked source row = chin y2 + 15, or -1
    for "no face", inference_embs.py:264-270; a ``.npy`` of T ints or one int) -- the face rectangle, the cv2-style resize to
    270 x 480, /255 and the +-12 frame edge padding then run on the GPU -- or already masked (T,270,480,3) crops (no --mask_y).
    --audio_path is a 16 kHz mono ``.wav`` (log-mel on the GPU); --text_path the reference's text-file grammar (:288-377); word
    boundaries must come from it (the WhisperX fallback of :589-601 is upstream).  Text needs XLM-RoBERTa states: --xlmr_checkpoint +
    --tokenizer (encoder on the engine, models/jegal.py:116-129) or --text_states (.npz: states, mask, ids, offsets).

    All seven --modalities work (the reference unpacks two return values and indexes word_boundaries[0] unconditionally, so only
    'vta' / 'vt' / 'va' survive there): outputs follow JEGAL.forward_inference's own return convention (:377-415)."""
    p = argparse.ArgumentParser(prog="inference_embs")
    p.add_argument("--checkpoint_path_gestsync", required=True)
    p.add_argument("--checkpoint_path_jegal", required=True)
    p.add_argument("--modalities", default="vta", choices=["vta", "vt", "va", "ta", "v", "t", "a"])
    p.add_argument("--video_path", default=None, help=".npy of frames: (T,H,W,3) uint8 source frames (with --mask_y) or masked (T,270,480,3) crops")
    p.add_argument("--mask_y", default=None, help=".npy of T ints or one int: last blanked source row per frame (chin y2 + 15; -1 = no face)")
    p.add_argument("--text_path", default=None)
    p.add_argument("--audio_path", default=None)
    p.add_argument("--res_dir", required=True)
    p.add_argument("--text_states", default=None, help="precomputed XLM-RoBERTa states (.npz: states, mask, ids, offsets) for --text_path's words")
    p.add_argument("--xlmr_checkpoint", default=None)
    p.add_argument("--tokenizer", default=None)
    _add_precision_args(p)
    p.add_argument("--audit", action="store_true",
                   help="run the clip a second time in the fp32 audit mode (precision 6, a second engine with the same checkpoints) and print "
                        "the rel-L2 / max-abs of the embeddings above against it: the 1e-3 contract checked on YOUR clip and checkpoint, where "
                        "no CPU reference is at hand (a network that amplifies operand rounding beyond it shows up here; DESIGN.md section 3)")
    args = p.parse_args(argv)
    mod = args.modalities
    for m, arg in (("v", "video_path"), ("a", "audio_path")):                # inference_embs.py:650-664
        if m in mod and getattr(args, arg) is None:
            raise ValueError(f"--{arg} must be specified when modality '{m}' is used.")
    if "t" in mod and args.text_path is None and args.audio_path is None:
        raise ValueError("For modality 't', you must specify either --text_path or --audio_path (since text can be extracted from audio).")
    if mod != "v" and args.text_path is None:
        raise SystemExit("word boundaries come from --text_path here (the reference's WhisperX fallback, inference_embs.py:589-601, is upstream of the hot path)")
    if "t" in mod and not (args.text_states or (args.xlmr_checkpoint and args.tokenizer)):
        raise SystemExit("modality 't' needs --text_states or --xlmr_checkpoint with --tokenizer")
    ns = argparse.Namespace(checkpoint_path_gestsync=args.checkpoint_path_gestsync, checkpoint_path=args.checkpoint_path_jegal,
                            precision=args.precision, calibrate_frames=args.calibrate_frames)
    eng, gs, jg = _models(ns, need_gestsync="v" in mod, need_jegal=True)
    os.makedirs(args.res_dir, exist_ok=True)
    gesture, content, fname, wbs, text_strs = _inference_embs_clip(args, mod, eng, gs, jg, verbose=True)
    if args.audit:
        rep = audit_against_fp32(args, mod, gesture, content)
        print("Audit (fp32 engine, same clip and checkpoints): " + "; ".join(
            f"{k} rel-L2 {v['rel_l2']:.2e} max-abs {v['max_abs']:.2e}" for k, v in rep.items()))
        bad = [k for k, v in rep.items() if not (v["rel_l2"] < 1e-3 and v["max_abs"] < 1e-3)]
        if bad:
            print("WARNING: " + ", ".join(bad) + " exceed(s) the 1e-3 contract in precision mode {}: this checkpoint amplifies fp16 operand "
                  "rounding (DESIGN.md section 3, `sharp` family); use --precision 6 for the embeddings themselves.".format(eng.precision))
    print("------------------------------------------------")
    feat = {"gesture_emb": gesture, "content_emb": content,
            "info": {"fname": fname, "word_boundaries": None if wbs is None else wbs[0], "text": None if text_strs is None else text_strs[0]}}
    output_fname = os.path.join(args.res_dir, fname + ".pkl")
    with open(output_fname, "wb") as f:
        pickle.dump(feat, f)
    print("Saved the embeddings: ", output_fname)
    return 0


def audit_against_fp32(args, mod, gesture, content):
    """--audit: the same clip through a second engine in JG_PREC_FP32 (exact-fp32 MFMAs, fp32 activations end to end: the arithmetic of the
    reference's CPU path, inference_embs.py:497) with the same checkpoints -> {"gesture" | "content": {"rel_l2", "max_abs"}} of the
    embeddings passed in against it."""
    from ._lib import Engine, PREC_FP32
    from .gestsync import GestSync
    from .jegal import JEGAL
    e32 = Engine(torch.cuda.current_device(), precision=PREC_FP32)
    try:
        gs32 = GestSync(engine=e32).load_state_dict(load_checkpoint(args.checkpoint_path_gestsync, "gestsync")) if "v" in mod else None
        jg32 = JEGAL(engine=e32).load_state_dict(load_checkpoint(args.checkpoint_path_jegal, "jegal"))
        g32, c32, _, _, _ = _inference_embs_clip(args, mod, e32, gs32, jg32, verbose=False)
    finally:
        e32.close()
    rep = {}
    for name, a, b in (("gesture", gesture, g32), ("content", content, c32)):
        if a is not None:
            a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
            rep[name] = {"rel_l2": float(np.linalg.norm(a64 - b64) / max(np.linalg.norm(b64), 1e-30)), "max_abs": float(np.abs(a64 - b64).max())}
    return rep


def _inference_embs_clip(args, mod, eng, gs, jg, verbose=True):
    """frames / wav / text of one clip -> (gesture (T,512) | None, content (W,512) | None, fname, word boundaries, text): extract_embs of
    inference_embs.py:526-646 on `eng`."""
    say = print if verbose else (lambda *a, **k: None)
    vis = mask = text = audio = am = wbs = None
    fname = None
    text_strs = None
    if args.video_path is not None and "v" in mod:
        frames = np.load(args.video_path)
        if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
            raise ValueError("--video_path must hold (T,H,W,3) uint8 frames")
        if args.mask_y is not None:
            my = np.load(args.mask_y) if args.mask_y.endswith(".npy") else np.full(frames.shape[0], int(args.mask_y))
            crops = eng.mask_resize(torch.from_numpy(frames), np.asarray(my, np.int32).reshape(-1))
        else:
            if tuple(frames.shape[1:3]) != (270, 480):
                raise ValueError("frames that are not 270x480 need --mask_y (source-resolution path)")
            crops = torch.from_numpy(frames).to(eng.device)
        say("Input masked frames: ", tuple(crops.shape))
        say("Extracting pre-trained GestSync features...")
        vis = gs.extract_clip_feats(crops)                                   # (1,T,1024): get_gestsync_feats (:476-522)
        mask = torch.ones(vis.shape[:2], device=vis.device)
        fname = os.path.basename(args.video_path).split(".")[0]
        say("Input visual features: ", tuple(vis.shape))
    if args.text_path is not None:
        text_strs, wbs = extract.load_text(args.text_path)
        if fname is None:
            fname = os.path.basename(args.text_path).split(".")[0]
    if args.audio_path is not None and "a" in mod:
        say("Loading audio...")
        audio = _wav_mel(args.audio_path, eng)                               # load_audio (:440-475)
        say("Input audio mel: ", tuple(audio.shape))
        am = torch.ones((1, audio.shape[1] // 4), device=eng.device)
    if fname is None and args.audio_path is not None:
        fname = os.path.basename(args.audio_path).split(".")[0]
    if "t" in mod:
        if args.text_states:
            st, tm, ids, offs = _load_text_pack(args.text_states)
            st, tm, ids, offs = (np.asarray(x) for x in (st, tm, ids, offs))
            if st.ndim == 2:
                st, tm, ids, offs = st[None], tm[None], ids[None], offs[None]
            text = (torch.from_numpy(st.astype(np.float32)), torch.from_numpy(tm), [text_strs[0].split(" ")], ids, offs)
        else:
            from .xlmr import roberta_embeddings
            text = roberta_embeddings(_load_xlmr(eng, args.xlmr_checkpoint), _load_tokenizer(args.tokenizer), text_strs)
    say("Extracting JEGAL embeddings...")
    say("------------------------------------------------")
    out = jg.forward_inference(visual_feats=vis, visual_mask=mask, text=text, audio=audio, audio_mask=am,
                               word_boundaries=wbs if mod != "v" else None)
    gesture, content = _gesture_content(out, vis is not None, text is not None or audio is not None)
    if gesture is not None:
        gesture = eng.l2norm(gesture[0]).cpu().numpy()                       # F.normalize(p=2, dim=-1), [0], .cpu().numpy() (:629-637)
        say("Extracted gesture embeddings: ", gesture.shape)
    if content is not None:
        content = eng.l2norm(content[0]).cpu().numpy()
        say("Extracted content embeddings: ", content.shape)
    return gesture, content, fname, wbs, text_strs


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    from . import want_hw_queues
    want_hw_queues()            # an application may shape its own process: before the first HIP call (no-op when the caller already set it)
    if not argv or argv[0] not in COMMANDS:
        print(__doc__)
        return 2
    res = COMMANDS[argv[0]](argv[1:])
    return 0 if not isinstance(res, int) else res


if __name__ == "__main__":
    sys.exit(main())
