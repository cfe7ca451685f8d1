"""ctypes binding of libjegal_hip.so (include/jegal_hip.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded,
importing the engine raises.  PyTorch is used only for device memory and streams; every
tensor op of the hot path runs inside the library.
"""
import ctypes
import os

import numpy as np
import torch  # imported first so libamdhip64.so.7 resolves to the runtime torch already loaded

from . import _abi
from ._check_entries import CheckPoints, ConvCheck, ConvShape, GemmCheck
from ._metric_entries import MetricEntries, _ptr, _shape

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libjegal_hip.so")

# include/jegal_hip.h is the only declaration of the ABI: signatures, structs and enum values come from _abi's parse of it
_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
JG_F32, JG_F16, JG_I64, JG_U8, JG_ERR_ARG = (_abi.CONSTANTS[k] for k in ("JG_F32", "JG_F16", "JG_I64", "JG_U8", "JG_ERR_ARG"))
PREC_FP16, PREC_FP16_W2, PREC_FP16_W2_ALL, PREC_FP16_BC, PREC_BF16, PREC_FP16_RC, PREC_FP32 = (
    _abi.CONSTANTS["JG_PREC_" + k] for k in ("FP16", "FP16_W2", "FP16_W2_ALL", "FP16_BC", "BF16", "FP16_RC", "FP32"))
AUDIT_CONV, AUDIT_GESTSYNC, AUDIT_JEGAL, AUDIT_CONTENT, AUDIT_XLMR = 1, 2, 4, 8, 16      # option audit_stages (include/jegal_hip.h)
STAGES = ["stack_frames", "conv1", "maxpool", "conv2-fc6+audio_cnn", "gemm", "attention", "layernorm", "misc", "conv1_aux"]
assert len(STAGES) == _abi.CONSTANTS["JG_ST_COUNT"], "STAGES needs one label per JG_ST_* stage of include/jegal_hip.h"

_SIGS = {name: args for name, (res, args) in _abi.FUNCTIONS.items() if res is _I}      # the entries that return a status
EXPORTS = sorted(_abi.FUNCTIONS)

_lib = None


def load_library():
    """Load libjegal_hip.so or raise.  No fallback by design."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C jegal_amd/csrc`).  jegal_amd has no CPU/PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _abi.FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def gemm_plan(num_cu=256, lanes_active=False, opts=None, conv=None, a_tiled=False, **fields):
    """The GEMM planner's answer (jg_debug_gemm_plan) -> (instance name or "rejected", grid, lds bytes, stagger).  Needs no Engine and no
    GPU.  fields: those of jg_gemm_check, as for Engine.debug_gemm_check; of a pointer field only its presence counts, so a tensor or
    True stands for "set" (None / False / 0: NULL).  a_tiled: A is the tiled token plane (debug_gemm_check's a_tiled field, passed with the
    other fields, lands here: the planner plans exactly what that call launches).  opts: engine options (gemm_*, lane_walk*; "num_cu" overrides num_cu, "debug_lanes" overrides
    lanes_active, as the handle options of those names do for the check points); conv: dict of the jg_conv_shape fields."""
    lib = load_library()
    c = GemmCheck()
    ptr_fields = {k for k, t in GemmCheck._fields_ if t is _P}
    for k, v in fields.items():
        if k in ptr_fields:
            v = 1 if isinstance(v, torch.Tensor) or bool(v) else None
        setattr(c, k, v)
    opts = dict(opts or {})
    num_cu = opts.pop("num_cu", num_cu)
    lanes_active = opts.pop("debug_lanes", lanes_active)
    names = (ctypes.c_char_p * max(len(opts), 1))(*[k.encode() for k in opts])
    values = (_I * max(len(opts), 1))(*[int(v) for v in opts.values()])
    cs = ConvShape(**{k: int(v) for k, v in conv.items()}) if conv is not None else None
    name = ctypes.create_string_buffer(128)
    grid, lds, stagger = _I(), _I(), _I()
    rc = lib.jg_debug_gemm_plan(ctypes.byref(c), ctypes.byref(cs) if cs is not None else None, int(bool(a_tiled)), int(num_cu), int(bool(lanes_active)),
                                names, values, len(opts), name, 128, ctypes.byref(grid), ctypes.byref(lds), ctypes.byref(stagger))
    if rc != 0:
        raise JegalError(f"jg_debug_gemm_plan: bad arguments or unknown option ({rc})", rc)
    return name.value.decode(), grid.value, lds.value, stagger.value


def search_plan(n_queries, n_gallery, k, num_cu=256, slices=0):
    """The cut jg_sim_search makes (jg_debug_search_plan) -> (slices, rows per slice, bytes of the slices' lists).  Needs no Engine and no
    GPU; JegalError where jg_sim_search refuses the counts."""
    s, r, b = _I(), _I(), ctypes.c_int64()
    rc = load_library().jg_debug_search_plan(int(n_queries), int(n_gallery), int(k), int(num_cu), int(slices), ctypes.byref(s), ctypes.byref(r),
                                             ctypes.byref(b))
    if rc != 0:
        raise JegalError(f"jg_debug_search_plan: bad arguments ({rc})", rc)
    return s.value, r.value, b.value


def coupling_plan(w_offsets, n_gallery, k, num_cu=256, slices=0):
    """The plan jg_sim_coupling makes (jg_debug_coupling_plan) for queries of the word rows w_offsets (queries + 1 host entries) ->
    (tile_first_query: int32 array of tiles + 1 entries, slices, rows per slice, bytes of the slices' lists).  Needs no Engine and no
    GPU; JegalError where jg_sim_coupling refuses the offsets or the counts."""
    import numpy as np
    off = np.ascontiguousarray(np.asarray(w_offsets).reshape(-1), np.int32)
    tfq = np.zeros(max(off.size, 1), np.int32)
    t, s, r, b = _I(), _I(), _I(), ctypes.c_int64()
    rc = load_library().jg_debug_coupling_plan(off.ctypes.data_as(_P) if off.size else None, off.size - 1, int(n_gallery), int(k), int(num_cu),
                                               int(slices), tfq.ctypes.data_as(_P), ctypes.byref(t), ctypes.byref(s), ctypes.byref(r),
                                               ctypes.byref(b))
    if rc != 0:
        raise JegalError(f"jg_debug_coupling_plan: bad arguments ({rc})", rc)
    return tfq[:t.value + 1].copy(), s.value, r.value, b.value


WEIGHT_FORMS = ["single", "split", "bias_corrected", "runtime_corrected"]      # enum WeightForm (jegal_amd/csrc/weight_form.h)


def weight_form(precision, kind, model, keep32=False):
    """Which weights a packed layer's GEMM runs with (jg_debug_weight_form) -> (form name, lo kept on the device, starts uncalibrated).
    kind: 0 conv, 1 gesture, 2 content, 3 XLM-R; model: 1 GestSync, 2 JEGAL, 3 XLM-R.  Needs no Engine and no GPU."""
    form, lo, unc = _I(), _I(), _I()
    rc = load_library().jg_debug_weight_form(int(precision), int(kind), int(model), int(bool(keep32)), ctypes.byref(form), ctypes.byref(lo), ctypes.byref(unc))
    if rc != 0:
        raise JegalError(f"jg_debug_weight_form: bad arguments ({rc})", rc)
    return WEIGHT_FORMS[form.value], bool(lo.value), bool(unc.value)


def gemm_runs_lo(form, uncalibrated=False, calibrating=False, clip_bias=False):
    """Whether a GEMM on a layer of this form (a name of WEIGHT_FORMS) takes the lo operand (jg_debug_gemm_runs_lo)."""
    lo = _I()
    rc = load_library().jg_debug_gemm_runs_lo(WEIGHT_FORMS.index(form), int(bool(uncalibrated)), int(bool(calibrating)), int(bool(clip_bias)), ctypes.byref(lo))
    if rc != 0:
        raise JegalError(f"jg_debug_gemm_runs_lo: bad arguments ({rc})", rc)
    return bool(lo.value)


def _host(a, dtype):
    """a host array of `dtype`, C-contiguous, or None -> (array kept alive by the caller, pointer or None)"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data


def pack_conv(w, bias, bn=None, *, slot, kpad=0, Opad=0, stride=(1, 1), reorder=False):
    """A conv layer's folded matrix and shift (jg_debug_pack_conv): w (O, I, KT, KH, KW) fp32, bias (O,), bn = (gamma, beta, mean, var) or
    None -> (matrix (N, K) fp32, shift (N,)).  Needs no Engine and no GPU."""
    w = np.ascontiguousarray(w, np.float32)
    O, I, KT, KH, KW = w.shape
    N, K = max(O, Opad), kpad if kpad > 0 else KH * KW * slot
    keep = [_host(x, np.float32) for x in (bias,) + (tuple(bn) if bn is not None else (None,) * 4)]
    matrix, shift = np.empty((N, K), np.float32), np.empty(N, np.float32)
    rc = load_library().jg_debug_pack_conv(w.ctypes.data, *[p for _, p in keep], O, I, KT, KH, KW, int(slot), int(kpad), int(Opad), int(stride[0]),
                                           int(stride[1]), int(bool(reorder)), N, K, matrix.ctypes.data, shift.ctypes.data)
    if rc != 0:
        raise JegalError(f"jg_debug_pack_conv: bad arguments ({rc})", rc)
    return matrix, shift


def pack_round(w, bias, *, bf16=False, form="single", keep_lo=False, diffuse_group=0, ln=None, add_beta=None, device32=False):
    """A layer packed under a rounding rule (jg_debug_pack_round): w (N, K) fp32, bias (N,); ln = (gamma, beta) packs it as that LayerNorm's
    consumer, add_beta as a producer -> dict of hi / lo (uint16 bit patterns; lo None unless keep_lo), bias, c1h / c1f (None without ln),
    w32 / b32 (None unless device32 or the form keeps them).  Needs no Engine and no GPU."""
    w = np.ascontiguousarray(w, np.float32)
    N, K = w.shape
    keep = [_host(x, np.float32) for x in (bias,) + (tuple(ln) if ln is not None else (None, None)) + (add_beta,)]
    keeps32 = bool(device32) or form == "bias_corrected"
    out = dict(hi=np.empty((N, K), np.uint16), lo=np.empty((N, K), np.uint16) if keep_lo else None, bias=np.empty(N, np.float32),
               c1h=np.empty(N, np.float32) if ln is not None else None, c1f=np.empty(N, np.float32) if ln is not None else None,
               w32=np.empty((N, K), np.float32) if keeps32 else None, b32=np.empty(N, np.float32) if keeps32 else None)
    rc = load_library().jg_debug_pack_round(w.ctypes.data, keep[0][1], N, K, int(bool(bf16)), WEIGHT_FORMS.index(form), int(bool(keep_lo)),
                                            int(diffuse_group), keep[1][1], keep[2][1], keep[3][1], int(bool(device32)),
                                            *[v.ctypes.data if v is not None else None for v in out.values()])
    if rc != 0:
        raise JegalError(f"jg_debug_pack_round: bad arguments ({rc})", rc)
    return out


def conv1_panel(hi, shift):
    """conv1's slot-major panel for the direct kernel (jg_debug_conv1_panel): hi (64, 784) uint16 bit patterns, shift (64,) -> (49, 64, 16) uint16."""
    hi, shift = np.ascontiguousarray(hi, np.uint16), np.ascontiguousarray(shift, np.float32)
    if hi.shape != (64, 784) or shift.shape != (64,):
        raise ValueError("conv1_panel: hi (64, 784), shift (64,)")
    panel = np.empty((49, 64, 16), np.uint16)
    rc = load_library().jg_debug_conv1_panel(hi.ctypes.data, shift.ctypes.data, panel.ctypes.data)
    if rc != 0:
        raise JegalError(f"jg_debug_conv1_panel: bad arguments ({rc})", rc)
    return panel


def bias_correction(w32, b32, mu, rows):
    """The calibrated bias of a bias-corrected layer (jg_debug_bias_correction): w32 (N, K), b32 (N,), mu (K,) column sums over `rows` rows."""
    w32, b32, mu = (np.ascontiguousarray(x, np.float32) for x in (w32, b32, mu))
    N, K = w32.shape
    bias = np.empty(N, np.float32)
    rc = load_library().jg_debug_bias_correction(w32.ctypes.data, b32.ctypes.data, mu.ctypes.data, int(rows), N, K, bias.ctypes.data)
    if rc != 0:
        raise JegalError(f"jg_debug_bias_correction: bad arguments ({rc})", rc)
    return bias


class JegalError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def _track_offsets(lengths):
    """Lengths of tracks -> the (n + 1) int32 row offsets jg_track_windows / jg_jegal_gesture_tracks take."""
    lens = [int(x) for x in lengths]
    if any(t < 0 for t in lens) or sum(lens) > 2**31 - 1:
        raise ValueError("track lengths must be >= 0 and sum to less than 2^31 rows")
    return (ctypes.c_int32 * (len(lens) + 1))(*np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int32))


def track_windows(lengths, win, ctx):
    """The window rule of long gesture tracks (jg_track_windows, include/jegal_hip.h) -> (table, span_max): table (n_windows, 4) int32 =
    (span first row, span length, core offset inside the span, core length) per window, rows counted over the concatenated tracks.
    Needs no Engine and no GPU."""
    lib = load_library()
    off = _track_offsets(lengths)
    n, smax = _I(), _I()
    rc = lib.jg_track_windows(off, len(off) - 1, int(win), int(ctx), None, 0, ctypes.byref(n), ctypes.byref(smax))
    if rc != 0:
        raise JegalError(f"jg_track_windows: bad arguments (need win >= 1, ctx >= 0, win + 2 ctx <= 500) ({rc})", rc)
    table = np.zeros((n.value, 4), np.int32)
    rc = lib.jg_track_windows(off, len(off) - 1, int(win), int(ctx), table.ctypes.data, n.value,
                              ctypes.byref(n), ctypes.byref(smax))
    if rc != 0:
        raise JegalError(f"jg_track_windows failed ({rc})", rc)
    return table, smax.value


class Engine(MetricEntries, CheckPoints):
    """One jg_handle on one GPU.  Not thread-safe; one per process/GPU.  The metric entries (pool_mean .. asd_windows) are
    MetricEntries' (_metric_entries.py), the kernel check points (debug_*) CheckPoints' (_check_entries.py)."""

    _cache = {}

    @classmethod
    def get(cls, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("jegal_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if idx not in cls._cache:
            cls._cache[idx] = cls(idx)
        return cls._cache[idx]

    def __init__(self, device_index=0, precision=None):
        self.lib = load_library()
        self.device = torch.device("cuda", device_index)
        torch.cuda.init()
        with torch.cuda.device(self.device):
            torch.zeros(1, device=self.device)          # make sure the HIP context exists
        h = _P()
        rc = self.lib.jg_create(device_index, ctypes.byref(h))
        if rc != 0:
            raise JegalError(f"jg_create({device_index}) failed with {rc}")
        self.h = h
        self.precision = PREC_FP16_RC              # the library's default (jg_handle::precision)
        if precision is not None:
            self.set_precision(precision)
        self.finalized = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.jg_destroy(self.h)
            self.h = None
            for k, v in list(Engine._cache.items()):
                if v is self:
                    del Engine._cache[k]

    def _ck(self, rc):
        if rc != 0:
            raise JegalError(f"libjegal_hip error {rc}: {self.lib.jg_last_error(self.h).decode()}", rc)

    def _bind_stream(self):
        self._ck(self.lib.jg_set_stream(self.h, _P(torch.cuda.current_stream(self.device).cuda_stream)))

    def _call(self, name, *args):
        """One entry on the current stream: tensors go by device pointer, None and scalars as they are; a status other than 0 raises."""
        self._bind_stream()
        self._ck(getattr(self.lib, name)(self.h, *[_ptr(a) if isinstance(a, torch.Tensor) else a for a in args]))

    # ---- weights
    def set_precision(self, mode):
        self._ck(self.lib.jg_set_precision(self.h, mode))
        self.precision = int(mode)

    def set_option(self, name, value):
        self._ck(self.lib.jg_set_option(self.h, name.encode(), int(value)))

    def set_chunk(self, clips):
        self._ck(self.lib.jg_set_chunk(self.h, int(clips)))

    def load_tensors(self, state_dict):
        for name, val in state_dict.items():
            if isinstance(val, torch.Tensor):
                val = val.detach().cpu().numpy()
            arr = np.asarray(val)
            if arr.dtype == np.float16:
                code = JG_F16
            elif arr.dtype == np.int64:
                code = JG_I64
            else:
                arr = arr.astype(np.float32, copy=False)
                code = JG_F32
            arr = np.ascontiguousarray(arr)
            shape = (ctypes.c_int64 * max(arr.ndim, 1))(*arr.shape)
            self._ck(self.lib.jg_load_tensor(self.h, name.encode(), arr.ctypes.data_as(_P), shape, arr.ndim, code))

    def finalize(self, which, clear_staged=True):
        """jg_finalize_weights; the Python facades load one model's state_dict and finalize it at once, so whatever that
        finalize did not consume (lstm.* of a GestSync checkpoint; net_aud.* / ff_aud.* unless bit 3, value 8, is in `which`) is dropped
        afterwards.  which: 1 GestSync video stream, 2 JEGAL, 4 XLM-RoBERTa, 8 GestSync audio stream."""
        with torch.cuda.device(self.device):
            self._ck(self.lib.jg_finalize_weights(self.h, which))
        if clear_staged:
            self._ck(self.lib.jg_clear_staged_tensors(self.h))
        self.finalized |= which

    # ---- helpers
    def _f32(self, t):
        return torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()

    def _i32(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.int32).contiguous()
        return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.int32)), device=self.device)

    def sync(self):
        self._ck(self.lib.jg_sync(self.h))

    def calibrate(self, frames=None):
        """Re-run the bias-correction calibration (precision mode 3) on real clips (B,T,270,480,3);
        None = the built-in deterministic synthetic clips used by finalize()."""
        self._bind_stream()
        if frames is None:
            self._ck(self.lib.jg_calibrate_gesture(self.h, None, JG_U8, 0, 0))
            return
        frames, code, B, T = self._frames_arg(frames)
        self._ck(self.lib.jg_calibrate_gesture(self.h, _ptr(frames), code, B, T))

    def _frames_arg(self, frames):
        """Validate a clip batch and put it on this engine's device: (B,T,270,480,3) uint8 (decoded video) or
        floating point in [0,1].  Returns (contiguous device tensor, dtype code, B, T).  A wrong shape would hand the
        conv1 kernel a raw pointer it reads 270x480x3 bytes per frame from, so it is rejected here."""
        if not isinstance(frames, torch.Tensor):
            frames = torch.as_tensor(frames)
        if frames.dim() != 5 or tuple(frames.shape[2:]) != (270, 480, 3):
            raise ValueError(f"frames must be (B,T,270,480,3), got {tuple(frames.shape)}")
        if frames.shape[0] == 0 or frames.shape[1] == 0:
            raise ValueError("frames must hold at least one clip of at least one frame")
        frames = frames.to(self.device)
        if frames.dtype == torch.uint8:
            code = JG_U8
        elif frames.dtype.is_floating_point:
            frames, code = frames.to(torch.float32), JG_F32
        else:
            raise ValueError(f"frames must be uint8 or floating point, got {frames.dtype}")
        return frames.contiguous(), code, frames.shape[0], frames.shape[1]

    def _out_arg(self, out, shape):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
                or tuple(out.shape) != tuple(shape) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(shape)} on {self.device}")
        return out

    # ---- GestSync
    def gestsync_clip(self, frames, lengths=None):
        """frames (B,T,270,480,3) uint8 or float32 cuda tensor -> (B,T,1024) fp32.  lengths (B ints, optional): frames of each clip
        that are its own in a batch padded to T with copies of the clips' last frames (jg_gestsync_clip_ragged): rows t < lengths[b]
        of clip b are then what the clip gives alone, whatever T is (bit for bit for clips of >= 49 frames; a shorter clip alone takes
        the unfused plan and agrees within the contract, include/jegal_hip.h)."""
        self._bind_stream()
        frames, code, B, T = self._frames_arg(frames)
        out = torch.empty((B, T, 1024), dtype=torch.float32, device=self.device)
        if lengths is None:
            self._ck(self.lib.jg_gestsync_clip(self.h, _ptr(frames), code, B, T, _ptr(out)))
            return out
        v = [int(x) for x in lengths]
        if len(v) != B:
            raise ValueError("lengths needs one entry per clip")
        self._ck(self.lib.jg_gestsync_clip_ragged(self.h, _ptr(frames), code, B, T, (ctypes.c_int32 * B)(*v), _ptr(out)))
        return out

    def gestsync_windows(self, x, return_feats=False):
        self._bind_stream()
        x = self._f32(x)
        if tuple(x.shape[1:]) != (3, 25, 270, 480):
            raise ValueError(f"x must be (N,3,25,270,480), got {tuple(x.shape)}")
        N = x.shape[0]
        out = torch.empty((N, 1024, 21), dtype=torch.float32, device=self.device)
        oc = torch.empty((N, 512, 21), dtype=torch.float32, device=self.device) if return_feats else None
        self._ck(self.lib.jg_gestsync_windows(self.h, _ptr(x), N, _ptr(out), _ptr(oc)))
        return (out, oc) if return_feats else out

    def gestsync_audio_windows(self, x):
        """jg_gestsync_audio_windows, GestSync.forward_aud's arithmetic: x (N,1,80,100) (mel band x mel step) -> (N,1024) fp32.  Needs
        finalize bit 3 (value 8)."""
        self._bind_stream()
        x = self._f32(x)
        if x.dim() != 4 or tuple(x.shape[1:]) != (1, 80, 100) or x.shape[0] < 1:
            raise ValueError(f"x must be (N,1,80,100) with N >= 1, got {tuple(x.shape)}")
        N = x.shape[0]
        out = torch.empty((N, 1024), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_gestsync_audio_windows(self.h, _ptr(x), N, _ptr(out)))
        return out

    def gestsync_audio_clip(self, mel, T, lengths=None):
        """jg_gestsync_audio_clip: mel (B,Tm,80) time-major (Engine.logmel's layout) -> (B,T,1024): window t = mel rows 4(t-12) .. 4(t-12)+99,
        clamped to the clip's own rows.  lengths (B ints, optional): mel rows of each clip that are its own in a padded batch."""
        self._bind_stream()
        mel = self._f32(mel)
        if mel.dim() != 3 or mel.shape[2] != 80 or mel.shape[0] < 1 or mel.shape[1] < 1 or int(T) < 1:
            raise ValueError(f"mel must be (B,Tm,80) with B, Tm, T >= 1, got {tuple(mel.shape)}, T = {T}")
        B, Tm = mel.shape[0], mel.shape[1]
        v = None
        if lengths is not None:
            v = [int(x) for x in lengths]
            if len(v) != B:
                raise ValueError("lengths needs one entry per clip")
            v = (ctypes.c_int32 * B)(*v)
        out = torch.empty((B, int(T), 1024), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_gestsync_audio_clip(self.h, _ptr(mel), B, Tm, int(T), v, _ptr(out)))
        return out

    def extract_gesture(self, frames, out=None):
        """frames -> unit-norm gesture embedding (B,T,512), one library call."""
        self._bind_stream()
        frames, code, B, T = self._frames_arg(frames)
        if T > 500:
            raise ValueError("clips are limited to 500 frames (JEGAL's positional table, modules.py:136)")
        out = self._out_arg(out, (B, T, 512))
        self._ck(self.lib.jg_extract_gesture(self.h, _ptr(frames), code, B, T, _ptr(out)))
        return out

    # ---- JEGAL
    def jegal_gestures(self, feats, mask=None, align=False):
        self._bind_stream()
        feats = self._f32(feats)
        B, T, D = feats.shape
        if D != 1024:
            raise ValueError("visual feats must have 1024 channels")
        m = None if mask is None else self._f32(mask).reshape(B, T)
        out = torch.empty((B, T, 512), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_jegal_gestures(self.h, _ptr(feats), _ptr(m), B, T, int(bool(align)), _ptr(out)))
        return out

    @staticmethod
    def track_windows(lengths, win, ctx):
        """The window table of a set of tracks, (n, 4) int32, and span_max (the module's track_windows; no device involved)."""
        return track_windows(lengths, win, ctx)

    def jegal_gesture_tracks(self, feats, lengths, win=120, ctx=50, align=True, normalize=False):
        """Gesture embeddings of tracks of ANY length (jg_jegal_gesture_tracks): feats (sum T, 1024), the tracks' GestSync features back to
        back, lengths = frames per track -> (sum T, 512) on the device, row for row.  A track is encoded in windows: every `win` frames are
        emitted from a span that reaches `ctx` frames further on both sides (win + 2 ctx <= 500, the positional table); a track of at
        most `win` frames is one window, i.e. exactly jegal_gestures on that clip (include/jegal_hip.h has the rule).
        The defaults give spans of at most 220 frames, the longest clip of the reference's dataset lists (dataset/avs_*.csv), i.e. what the
        model was trained on.  That is a choice from the dataset's lengths, not a measured optimum: no trained checkpoint is available
        to tune win / ctx on retrieval quality."""
        self._bind_stream()
        feats = self._f32(feats)
        off = _track_offsets(lengths)
        rows = int(off[len(off) - 1])
        if feats.dim() != 2 or feats.shape[1] != 1024 or feats.shape[0] != rows:
            raise ValueError(f"feats must be (sum of lengths = {rows}, 1024), got {tuple(feats.shape)}")
        out = torch.empty((rows, 512), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_jegal_gesture_tracks(self.h, _ptr(feats), off, len(off) - 1, int(win), int(ctx), int(bool(align)), int(bool(normalize)),
                                                  _ptr(out)))
        return out

    def extract_gesture_track(self, frames, win=120, ctx=50):
        """One track of frames (T,270,480,3), T unbounded -> unit-norm gesture embeddings (T,512): gestsync_clip on the track as a batch of
        one, then jegal_gesture_tracks(normalize=True).  (extract_gesture is the one-call form for clips of at most 500 frames.)"""
        if not isinstance(frames, torch.Tensor):
            frames = torch.as_tensor(frames)
        if frames.dim() != 4:
            raise ValueError(f"frames must be one track (T,270,480,3), got {tuple(frames.shape)}")
        feats = self.gestsync_clip(frames[None])[0]
        return self.jegal_gesture_tracks(feats, [feats.shape[0]], win=win, ctx=ctx, align=True, normalize=True)

    def audio_len(self, Tm):
        return int(self.lib.jg_audio_len(int(Tm)))

    def jegal_audio(self, mel, valid_len=None):
        """mel (B,Tm,80) -> (B, audio_len(Tm), 256).  valid_len (B ints, optional): mel frames each clip of a zero-padded batch
        really holds -- rows t < audio_len(valid_len[b]) of clip b then equal the clip run alone (jg_jegal_audio_ragged)."""
        self._bind_stream()
        mel = self._f32(mel)
        B, Tm, F = mel.shape
        if F != 80:
            raise ValueError("mel must have 80 bands")
        out = torch.empty((B, self.audio_len(Tm), 256), dtype=torch.float32, device=self.device)
        if valid_len is None:
            self._ck(self.lib.jg_jegal_audio(self.h, _ptr(mel), B, Tm, _ptr(out)))
            return out
        v = [int(x) for x in valid_len]
        if len(v) != B:
            raise ValueError("valid_len needs one entry per clip")
        self._ck(self.lib.jg_jegal_audio_ragged(self.h, _ptr(mel), B, Tm, (ctypes.c_int32 * B)(*v), _ptr(out)))
        return out

    def mask_resize(self, frames_u8, mask_y):
        """load_rgb_masked_frames (inference_embs.py:235-276) minus /255 and the edge pad: (T,H,W,3) uint8 source frames,
        mask_y (T,) int (last blanked source row = y2+15, or -1 for "no face") -> (T,270,480,3) uint8 masked crops."""
        self._bind_stream()
        frames_u8 = frames_u8.to(self.device).contiguous()
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
            raise ValueError("frames must be uint8 (T,H,W,3)")
        T, H, W, _ = frames_u8.shape
        my = torch.as_tensor(mask_y, dtype=torch.int32).to(self.device).contiguous()
        if my.numel() != T:
            raise ValueError("mask_y needs one entry per frame")
        out = torch.empty((T, 270, 480, 3), dtype=torch.uint8, device=self.device)
        self._ck(self.lib.jg_mask_resize(self.h, _ptr(frames_u8), T, H, W, _ptr(my), _ptr(out)))
        return out

    def unpack_masked(self, packed, row0, offsets, dst):
        """packed uint8 (bytes,) / row0 int32 (F,) / offsets int64 (F,) device tensors -> dst (F,270,480,3) uint8 (written in place).
        offsets must be multiples of 16; the kernel writes a frame as zeros instead of reading it when its metadata points outside
        `packed` (row0 outside 0..270, misaligned / negative offset, rows past the end)."""
        self._bind_stream()
        F = row0.numel()
        if (packed.dtype != torch.uint8 or row0.dtype != torch.int32 or offsets.dtype != torch.int64 or dst.dtype != torch.uint8
                or offsets.numel() != F or dst.numel() != F * 270 * 480 * 3 or not dst.is_contiguous() or not packed.is_contiguous()):
            raise ValueError("unpack_masked: packed uint8, row0 int32 (F), offsets int64 (F), dst uint8 (F,270,480,3)")
        self._ck(self.lib.jg_unpack_masked(self.h, _ptr(packed), packed.numel(), _ptr(row0), _ptr(offsets), F, _ptr(dst)))
        return dst

    def mask_resize_packed(self, packed, offsets, mask_y, H, W, dst):
        """Source-resolution frames with only the rows below each frame's mask shipped (jg_mask_resize_packed): packed uint8 (bytes,),
        offsets int64 (F,), mask_y int32 (F,) device tensors -> dst (F,270,480,3) uint8 (written in place)."""
        self._bind_stream()
        F = mask_y.numel()
        if (packed.dtype != torch.uint8 or mask_y.dtype != torch.int32 or offsets.dtype != torch.int64 or dst.dtype != torch.uint8
                or offsets.numel() != F or dst.numel() != F * 270 * 480 * 3 or not dst.is_contiguous() or not packed.is_contiguous()):
            raise ValueError("mask_resize_packed: packed uint8, offsets int64 (F), mask_y int32 (F), dst uint8 (F,270,480,3)")
        self._ck(self.lib.jg_mask_resize_packed(self.h, _ptr(packed), packed.numel(), _ptr(offsets), F, int(H), int(W), _ptr(mask_y), _ptr(dst)))
        return dst

    def logmel(self, wav, mel_basis):
        """wav (B,n) fp32 (int16 scale), n >= 257 -> log-mel (B, n//160, 80)."""
        ws, ms = _shape(wav), _shape(mel_basis)
        if len(ws) != 2 or ws[0] < 1 or ms != (80, 257):
            raise ValueError("wav must be (B, n) with B >= 1, mel_basis (80, 257)")
        if ws[1] < 257:
            raise ValueError("reflect padding needs more than 256 samples")
        self._bind_stream()
        wav = self._f32(wav)
        mb = self._f32(mel_basis)
        B, n = wav.shape
        out = torch.empty((B, n // 160, 80), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_logmel(self.h, _ptr(wav), B, n, _ptr(mb), _ptr(out)))
        return out

    def jegal_text(self, states, mask=None):
        self._bind_stream()
        states = self._f32(states)
        B, L, D = states.shape
        if D != 768:
            raise ValueError("text states must have 768 channels")
        m = None if mask is None else self._f32(mask).reshape(B, L)
        out = torch.empty((B, L, 256), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_jegal_text(self.h, _ptr(states), _ptr(m), B, L, _ptr(out)))
        return out

    def xlmr_encode(self, input_ids, attention_mask=None):
        """XLM-RoBERTa last_hidden_state: input_ids / attention_mask (B,L) int -> (B,L,768) fp32 (jg_xlmr_encode)."""
        self._bind_stream()
        ids = self._i32(input_ids)
        if ids.ndim != 2:
            raise ValueError("input_ids must be (B, L)")
        B, L = ids.shape
        m = None
        if attention_mask is not None:
            m = self._i32(attention_mask)
            if tuple(m.shape) != (B, L):
                raise ValueError("attention_mask must have the shape of input_ids")
        out = torch.empty((B, L, 768), dtype=torch.float32, device=self.device)
        self._ck(self.lib.jg_xlmr_encode(self.h, _ptr(ids), _ptr(m), B, L, _ptr(out)))
        return out

    def calibrate_xlmr(self, input_ids=None, attention_mask=None):
        """Precision mode 3: switch the XLM-RoBERTa Linears from hi+lo to bias-corrected single fp16, calibrated on these token ids
        ((B,L) ints; None = built-in uniform-random ids, validated on seeded test weights only)."""
        self._bind_stream()
        if input_ids is None:
            self._ck(self.lib.jg_calibrate_xlmr(self.h, None, None, 0, 0))
            return
        ids = self._i32(input_ids)
        if ids.ndim != 2:
            raise ValueError("input_ids must be (B, L)")
        m = None if attention_mask is None else self._i32(attention_mask)
        if m is not None and tuple(m.shape) != tuple(ids.shape):
            raise ValueError("attention_mask must have the shape of input_ids")
        self._ck(self.lib.jg_calibrate_xlmr(self.h, _ptr(ids), _ptr(m), ids.shape[0], ids.shape[1]))

    def word_pool(self, seq, segments, dst, dst_col):
        """seq (rows,D) fp32; segments int (n,3) = (start,end_excl,dst_row); dst (rows_out, ld) fp32."""
        self._bind_stream()
        seg = self._i32(segments).reshape(-1, 3)
        if seg.shape[0] == 0:
            return
        self._ck(self.lib.jg_word_pool(self.h, _ptr(seq), seq.shape[-1], _ptr(seg), seg.shape[0], _ptr(dst), dst.shape[-1], dst_col))

    def fuse_content(self, fused):
        self._bind_stream()
        fused = self._f32(fused)
        rows = fused.numel() // 512
        out = torch.empty_like(fused)
        self._ck(self.lib.jg_fuse_content(self.h, _ptr(fused), rows, _ptr(out)))
        return out

    def l2norm(self, x):
        self._bind_stream()
        x = self._f32(x)
        out = torch.empty_like(x)
        D = x.shape[-1]
        self._ck(self.lib.jg_l2norm(self.h, _ptr(x), _ptr(out), x.numel() // D, D))
        return out

    # ---- profiling
    # ---- multi-GPU exchange on RCCL through the C ABI (jegal_amd/dist.py uses torch.distributed for the same exchange)
    @staticmethod
    def comm_unique_id():
        """rank 0: a 128-byte RCCL id for the launcher to hand to every rank."""
        buf = ctypes.create_string_buffer(128)
        rc = load_library().jg_comm_get_unique_id(buf)
        if rc != 0:
            raise JegalError(f"jg_comm_get_unique_id failed with {rc} (librccl.so not loadable?)")
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        with torch.cuda.device(self.device):
            self._ck(self.lib.jg_comm_init(self.h, bytes(unique_id), int(rank), int(world)))
        self.comm_world = int(world)

    def comm_destroy(self):
        self._ck(self.lib.jg_comm_destroy(self.h))
        self.comm_world = 1

    def allgather(self, x):
        """(n, ...) per rank -> (world * n, ...) in rank order (ncclAllGather on the engine's stream)."""
        self._bind_stream()
        x = x.to(self.device).contiguous()
        out = torch.empty((getattr(self, "comm_world", 1) * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=self.device)
        self._ck(self.lib.jg_allgather(self.h, _ptr(x), _ptr(out), x.numel() * x.element_size()))
        return out

    def allreduce_sum_i64(self, counts):
        self._bind_stream()
        t = torch.as_tensor(counts, dtype=torch.int64).to(self.device).contiguous().clone()
        self._ck(self.lib.jg_allreduce_sum_i64(self.h, _ptr(t), t.numel()))
        return t

    def profile(self, on, only=None):
        """on: bracket every launch with HIP events; only="conv1": bracket just that stage (the rest of the step runs back to back)."""
        self._ck(self.lib.jg_profile_enable(self.h, 2 + STAGES.index(only) if (on and only) else int(bool(on))))

    def profile_reset(self):
        self._ck(self.lib.jg_profile_reset(self.h))

    def profile_get(self):
        res = {}
        for i, name in enumerate(STAGES):
            ms, n = ctypes.c_double(), ctypes.c_int64()
            self._ck(self.lib.jg_profile_get(self.h, i, ctypes.byref(ms), ctypes.byref(n)))
            res[name] = (ms.value, n.value)
        return res

    def workspace_bytes(self):
        return int(self.lib.jg_workspace_bytes(self.h))
