"""GestSync feature extractor, both streams -- MI355X engine behind the reference's interface.

Mirrors ``models/gestsync.py`` of the reference: ``GestSync()`` (no ctor args, :9),
``forward_vid(x, return_feats=False)`` (:148-162), ``forward_aud(x)`` (:164-168), ``load_state_dict`` with the
reference's keys (the audio stream is packed when the state dict carries it; the LSTM / logits_scale / fc tensors,
which no forward uses, are accepted and ignored).  All tensor math runs in libjegal_hip; there is no PyTorch fallback.
"""
import torch

from ._lib import Engine


class GestSync:
    def __init__(self, device=None, engine=None):
        self.engine = engine if engine is not None else Engine.get(device)
        self._loaded = False
        self._audio = False

    # nn.Module-style plumbing so reference drivers (inference_embs.py:655-668) read the same
    def cuda(self, device=None):
        return self

    def eval(self):
        return self

    def load_state_dict(self, state_dict, strict=True):
        sd = {k.replace("module.", ""): v for k, v in state_dict.items()}
        self.engine.load_tensors(sd)
        # the audio stream (bit 3) with the video stream, in ONE finalize: the staged tensors are cleared behind it
        self._audio = "net_aud.conv1.weight" in sd
        self.engine.finalize(1 | (8 if self._audio else 0))     # raises on any missing key of a stream it packs (strict)
        self._loaded = True
        return self

    def _check(self):
        if not self._loaded:
            raise RuntimeError("GestSync: call load_state_dict() first")

    def forward_vid(self, x, return_feats=False):
        """x (N,3,25,270,480) float -> (N,1024,21) [, out_conv (N,512,21)]  (gestsync.py:148-162)."""
        self._check()
        with torch.no_grad():
            return self.engine.gestsync_windows(x, return_feats=return_feats)

    def _check_audio(self):
        self._check()
        if not self._audio:
            raise RuntimeError("GestSync: the loaded state dict had no audio stream (net_aud.* / ff_aud.*)")

    def forward_aud(self, x):
        """x (N,1,80,100) float (mel band x 100 mel steps = 25 frames) -> (N,1024,1)  (gestsync.py:164-168)."""
        self._check_audio()
        with torch.no_grad():
            return self.engine.gestsync_audio_windows(x).unsqueeze(-1)

    def extract_clip_audio_feats(self, mel, T, lengths=None):
        """mel (B,Tm,80) time-major log-mel (Engine.logmel; 4 mel steps per video frame) -> (B,T,1024): the audio twin of
        extract_clip_feats -- window t covers mel rows 4(t-12) .. 4(t-12)+99, clamped to the clip's own rows, as the video windows are
        edge-padded by 12 frames.  lengths (optional): each clip's own mel rows in a padded batch."""
        self._check_audio()
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        with torch.no_grad():
            return self.engine.gestsync_audio_clip(mel, T, lengths)

    def extract_clip_feats(self, frames, lengths=None):
        """frames (B,T,270,480,3) uint8 (or float in [0,1]) -> (B,T,1024): the padded/windowed loop of
        inference_embs.py:283,476-522 with the conv stack de-duplicated across windows.  lengths (optional): each clip's own
        frame count in a batch padded to T with copies of the clips' last frames (Engine.gestsync_clip)."""
        self._check()
        if frames.dim() == 4:
            frames = frames.unsqueeze(0)
        with torch.no_grad():
            return self.engine.gestsync_clip(frames, lengths)

    __call__ = forward_vid
