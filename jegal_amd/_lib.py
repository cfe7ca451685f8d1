"""ctypes binding of libjegal_hip.so (include/jegal_hip.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded,
importing the engine raises.  PyTorch is used only for device memory and streams; every
tensor op of the hot path runs inside the library.
"""
import ctypes
import os

import numpy as np
import torch  # imported first so libamdhip64.so.7 resolves to the runtime torch already loaded

from ._metric_entries import MetricEntries, _ptr, _shape

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libjegal_hip.so")

JG_F32, JG_F16, JG_I64, JG_U8 = 0, 1, 2, 3
PREC_FP16, PREC_FP16_W2, PREC_FP16_W2_ALL, PREC_FP16_BC, PREC_BF16, PREC_FP16_RC, PREC_FP32 = 0, 1, 2, 3, 4, 5, 6
AUDIT_CONV, AUDIT_GESTSYNC, AUDIT_JEGAL, AUDIT_CONTENT, AUDIT_XLMR = 1, 2, 4, 8, 16      # option audit_stages (include/jegal_hip.h)
STAGES = ["stack_frames", "conv1", "maxpool", "conv2-fc6+audio_cnn", "gemm", "attention", "layernorm", "misc", "conv1_aux"]

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
JG_ERR_ARG = -1


class GemmCheck(ctypes.Structure):
    """struct jg_gemm_check (include/jegal_hip.h): operands of one jg_debug_gemm_check launch."""
    _fields_ = [("A", _P), ("lda", _L), ("Wh", _P), ("Wl", _P), ("ldw", _L), ("M", _I), ("N", _I), ("K", _I),
                ("scale", _P), ("bias", _P), ("bias_clip", _P), ("rpc", _I), ("nclips", _I),
                ("res", _P), ("ldr", _L), ("res_mod", _I), ("relu", _I), ("out32", _P), ("out16", _P), ("ldc", _L),
                ("ln_w", _P), ("ln_b", _P), ("res16", _P),
                ("ln_mode", _I), ("ln_stats", _P), ("xres_hi", _P), ("xres_lo", _P), ("out_lo", _P), ("stat_out", _P),
                ("a_tiled", _I)]
class ConvCheck(ctypes.Structure):
    """struct jg_conv_check (include/jegal_hip.h): operands of one jg_debug_conv_check launch."""
    _fields_ = [("in_", _P)] + [(k, _I) for k in ("nimg", "H", "W", "C", "KH", "KW", "SH", "SW", "PH", "PW", "reorder")] + [
        ("Wh", _P), ("Wl", _P), ("ldw", _L), ("N", _I), ("K", _I), ("scale", _P), ("bias", _P), ("relu", _I),
        ("out32", _P), ("out16", _P), ("ldc", _L), ("s2_host", ctypes.POINTER(ctypes.c_int32)), ("op", _I), ("const_in", _P)]
class ConvShape(ctypes.Structure):
    """struct jg_conv_shape (include/jegal_hip.h): the part of a conv geometry the GEMM planner reads."""
    _fields_ = [(k, _I) for k in ("H", "W", "C", "KH", "KW", "PH", "PW", "tap_table", "rowmap", "const_in")]


_SIGS = {
    "jg_create": [_I, ctypes.POINTER(_P)],
    "jg_destroy": [_P],
    "jg_set_stream": [_P, _P],
    "jg_set_precision": [_P, _I],
    "jg_set_chunk": [_P, _I],
    "jg_set_option": [_P, ctypes.c_char_p, _I],
    "jg_sync": [_P],
    "jg_load_tensor": [_P, ctypes.c_char_p, _P, ctypes.POINTER(ctypes.c_int64), _I, _I],
    "jg_finalize_weights": [_P, _I],
    "jg_clear_staged_tensors": [_P],
    "jg_calibrate_gesture": [_P, _P, _I, _I, _I],
    "jg_gestsync_clip": [_P, _P, _I, _I, _I, _P],
    "jg_gestsync_clip_ragged": [_P, _P, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _P],
    "jg_gestsync_windows": [_P, _P, _I, _P, _P],
    "jg_gestsync_audio_windows": [_P, _P, _I, _P],
    "jg_gestsync_audio_clip": [_P, _P, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _P],
    "jg_debug_gsa_conv1_pool": [_P, _P, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _P, _P, _P, _I],
    "jg_debug_maxpool_2x3": [_P, _P, _I, _I, _I, _I, _P, _I],
    "jg_sync_offset": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "jg_sync_offset_windows": [_P, _P, _P, _I, _L, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P],
    "jg_debug_conv1_pool": [_P, _P, _I, _I, _I, _P],
    "jg_debug_gemm": [_P, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_double)],
    "jg_debug_gemm_ex": [_P, _P, _P, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_double)],
    "jg_debug_conv2_rowskip": [_P, ctypes.POINTER(ctypes.c_int)],
    "jg_debug_gemm_check": [_P, _P],
    "jg_debug_conv_check": [_P, _P],
    "jg_debug_maxpool": [_P, _P, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _I, _P, _P],
    "jg_debug_conv_rowmaps": [_P, ctypes.POINTER(ctypes.c_int32), _I, ctypes.POINTER(_I), ctypes.POINTER(_I), _I, ctypes.POINTER(_P), ctypes.POINTER(_P),
                              ctypes.POINTER(ctypes.c_int32)],
    "jg_debug_gemm_plan": [_P, _P, _I, _I, _I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_I), _I, ctypes.c_char_p, _I,
                           ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)],
    "jg_debug_weight_form": [_I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)],
    "jg_debug_gemm_runs_lo": [_I, _I, _I, _I, ctypes.POINTER(_I)],
    "jg_debug_pack_conv": [_P] * 6 + [_I] * 13 + [_P, _P],
    "jg_debug_pack_round": [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I] + [_P] * 7,
    "jg_debug_conv1_panel": [_P, _P, _P],
    "jg_debug_bias_correction": [_P, _P, _P, _L, _I, _I, _P],
    "jg_debug_gemm32": [_P, _P, _L, _P, _L, _I, _I, _I, _P, _P, _P, _L, _I, _I, _P, _L],
    "jg_debug_conv32": [_P, _P] + [_I] * 11 + [_P, _L, _I, _P, _P, _I, _P, _L],
    "jg_debug_gemm_x3": [_P, _P, _L, _P, _P, _L, _I, _I, _I, _P, _P, _L, _I, _I, _P, _L],
    "jg_debug_attention": [_P, _P, _P, _I, _I, _I, _I, _P],
    "jg_debug_attention_gather": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "jg_debug_attention32": [_P, _P, _P, _I, _I, _I, _I, _P],
    "jg_debug_stack_frames": [_P, _P, _I, _L, _L, _L, _L, _L, _L, _I, _I, _I, _I, _I, _P],
    "jg_debug_window_gather": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P],
    "jg_debug_layernorm": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    "jg_debug_layernorm_planes": [_P, _P, _P, _P, _P, _I, _I, _P],
    "jg_debug_group_mean": [_P, _P, _I, _I, _I, _P],
    "jg_debug_cast": [_P, _P, _P, _L],
    "jg_debug_audio_conv0": [_P, _P, _I, _I, _I, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_int32), _I],
    "jg_debug_zero_tail": [_P, _P, ctypes.POINTER(ctypes.c_int32), _I, _I, _I, _I, _L],
    "jg_debug_stack_frames32": [_P, _P, _I, _L, _L, _L, _L, _L, _L, _I, _I, _I, _I, _I, _P],
    "jg_debug_maxpool32": [_P, _P, _I, _I, _I, _I, _P],
    "jg_debug_group_mean32": [_P, _P, _I, _I, _I, _P],
    "jg_debug_zero_tail32": [_P, _P, ctypes.POINTER(ctypes.c_int32), _I, _I, _I, _I, _L],
    "jg_debug_xlmr_embed": [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "jg_debug_xlmr_embed_planes": [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "jg_debug_ln_stats": [_P, _P, _I, _I, _P],
    "jg_debug_mask_i32_f32": [_P, _P, _P, _L],
    "jg_debug_transpose_tokens": [_P, _P, _I, _I, _I, _P],
    "jg_debug_pe_project": [_P, _P, _I, _P, _P, _P, _I, _I, _P],
    "jg_debug_broadcast_channels": [_P, _P, _I, _P, _L],
    "jg_debug_col_sum": [_P, _P, _L, _I, _I, _P, _L, _P, _P],
    "jg_debug_rc_bias": [_P, _P, _L, _L, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _I, _P, _P, _I, _I, _P, _L, _P],
    "jg_debug_last_kernel": [_P, ctypes.c_char_p, _I],
    "jg_debug_conv_rows": [_P, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)],
    "jg_jegal_gestures": [_P, _P, _P, _I, _I, _I, _P],
    "jg_track_windows": [ctypes.POINTER(ctypes.c_int32), _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _I, ctypes.POINTER(_I), ctypes.POINTER(_I)],
    "jg_jegal_gesture_tracks": [_P, _P, ctypes.POINTER(ctypes.c_int32), _I, _I, _I, _I, _I, _P],
    "jg_debug_span_gather": [_P, _P, _P, _P, _I, _I, _I, _P, _P],
    "jg_debug_core_compact": [_P, _P, _I, _P, _I, _I, _I, _P],
    "jg_jegal_audio": [_P, _P, _I, _I, _P],
    "jg_jegal_audio_ragged": [_P, _P, _I, _I, ctypes.POINTER(ctypes.c_int32), _P],
    "jg_audio_len": [_I],
    "jg_logmel": [_P, _P, _I, _I, _P, _P],
    "jg_mask_resize": [_P, _P, _I, _I, _I, _P, _P],
    "jg_unpack_masked": [_P, _P, ctypes.c_int64, _P, _P, _I, _P],
    "jg_mask_resize_packed": [_P, _P, ctypes.c_int64, _P, _I, _I, _I, _P, _P],
    "jg_jegal_text": [_P, _P, _P, _I, _I, _P],
    "jg_xlmr_encode": [_P, _P, _P, _I, _I, _P],
    "jg_calibrate_xlmr": [_P, _P, _P, _I, _I],
    "jg_word_pool": [_P, _P, _I, _P, _I, _P, _I, _I],
    "jg_fuse_content": [_P, _P, _I, _P],
    "jg_l2norm": [_P, _P, _P, _I, _I],
    "jg_extract_gesture": [_P, _P, _I, _I, _I, _P],
    "jg_pool_mean": [_P, _P, _P, _I, _I, _P],
    "jg_sim_rank": [_P, _P, _P, _I, _I, _I, _I, _P, _P],
    "jg_sim_topk": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P],
    "jg_sim_topk_grouped": [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P],
    "jg_sim_search": [_P, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P],
    "jg_debug_search_plan": [_I, _I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_int64)],
    "jg_sim_coupling": [_P, _P, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, ctypes.c_int64],
    "jg_debug_coupling_plan": [_P, _I, _I, _I, _I, _I, _P, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_int64)],
    "jg_group_of_rows": [_P, _P, _L, _P, _I, _I, _P, _P],
    "jg_spot": [_P, _P, _P, _P, _P, _P, _I, _I, ctypes.c_float, _P, _P],
    "jg_attn_matrix": [_P, _P, _P, _P, _P, _I, _I, _I, ctypes.c_float, _I, _P, _P, _P, _P],
    "jg_attn_talk": [_P, _P, _P, _I, _L, _I, _P, _P, _I, _P, _P, _I, _I, ctypes.c_float, _I, _P, _I, _P, _P, _P, _P],
    "jg_asd": [_P, _P, _P, _P, _I, _I, ctypes.c_float, _P],
    "jg_asd_windows": [_P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I, ctypes.c_float, _P, _P, _P],
    "jg_comm_get_unique_id": [ctypes.c_char_p],
    "jg_comm_init": [_P, ctypes.c_char_p, _I, _I],
    "jg_comm_destroy": [_P],
    "jg_allgather": [_P, _P, _P, ctypes.c_int64],
    "jg_allreduce_sum_i64": [_P, _P, _I],
    "jg_profile_enable": [_P, _I],
    "jg_profile_get": [_P, _I, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)],
    "jg_profile_reset": [_P],
}
EXPORTS = sorted(list(_SIGS) + ["jg_last_error", "jg_stage_name", "jg_workspace_bytes"])

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
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _I
    lib.jg_last_error.argtypes = [_P]
    lib.jg_last_error.restype = ctypes.c_char_p
    lib.jg_stage_name.argtypes = [_I]
    lib.jg_stage_name.restype = ctypes.c_char_p
    lib.jg_workspace_bytes.argtypes = [_P]
    lib.jg_workspace_bytes.restype = ctypes.c_int64
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
    rc = lib.jg_track_windows(off, len(off) - 1, int(win), int(ctx), table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n.value,
                              ctypes.byref(n), ctypes.byref(smax))
    if rc != 0:
        raise JegalError(f"jg_track_windows failed ({rc})", rc)
    return table, smax.value


class Engine(MetricEntries):
    """One jg_handle on one GPU.  Not thread-safe; one per process/GPU.  The metric entries (pool_mean .. asd_windows) are
    MetricEntries' (_metric_entries.py)."""

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

    def debug_gemm(self, M, N, K, mode=0, iters=10, a16=None, w16=None):
        """ms per launch of the production GEMM; a16 (M,K) / w16 (N,K): optional fp16 cuda operands (else constant fill)."""
        self._bind_stream()
        ms = ctypes.c_double()
        for t, shp in ((a16, (M, K)), (w16, (N, K))):
            if t is not None and (t.dtype != torch.float16 or tuple(t.shape) != shp or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"debug_gemm operand must be a contiguous fp16 {shp} tensor on {self.device}")
        self._ck(self.lib.jg_debug_gemm_ex(self.h, _ptr(a16), _ptr(w16), M, N, K, mode, iters, ctypes.byref(ms)))
        return ms.value

    # ---- kernel check points (include/jegal_hip.h): one production launch on caller-owned device tensors, asynchronous on the
    # engine's stream; a shape the launcher rejects raises JegalError with .code == JG_ERR_ARG.  debug_last_kernel() names the instance.
    def debug_gemm_check(self, **kw):
        """Linear GEMM (launch_gemm): keyword arguments are the fields of jg_gemm_check; tensors are passed by pointer."""
        self._bind_stream()
        c = GemmCheck()
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                if v.device != self.device:
                    raise ValueError(f"debug_gemm_check: {k} must be on {self.device}")
                v = v.data_ptr()
            setattr(c, k, v)
        self._ck(self.lib.jg_debug_gemm_check(self.h, ctypes.byref(c)))

    def debug_conv_check(self, **kw):
        """Implicit-GEMM convolution (launch_gemm, conv): keyword arguments are the fields of jg_conv_check (`in_` for its `in`); tensors are
        passed by pointer, s2_host is a sequence of nimg ints (or None)."""
        self._bind_stream()
        c = ConvCheck()
        s2 = kw.pop("s2_host", None)
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                if v.device != self.device:
                    raise ValueError(f"debug_conv_check: {k} must be on {self.device}")
                v = v.data_ptr()
            setattr(c, "in_" if k == "in" else k, v)
        if s2 is not None:
            s2 = [int(x) for x in s2]
            if len(s2) != c.nimg:
                raise ValueError("debug_conv_check: s2_host needs one entry per image")
            keep = (ctypes.c_int32 * len(s2))(*s2)
            c.s2_host = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int32))
        self._ck(self.lib.jg_debug_conv_check(self.h, ctypes.byref(c)))

    def debug_maxpool(self, x, out, s2_host=None, in_op=0, const_in=None):
        """3x3 / stride 2 max-pool (launch_maxpool3x3s2): x (nimg,H,W,C) 16-bit NHWC -> out (nimg,(H-3)//2+1,(W-3)//2+1,C), written in place.
        s2_host (nimg ints) / in_op / const_in (H,W,C): input rows below conv_skip_decode(s2, in_op) come from const_in."""
        self._bind_stream()
        nimg, H, W, C = x.shape
        s2 = None
        if s2_host is not None:
            s2 = [int(v) for v in s2_host]
            if len(s2) != nimg:
                raise ValueError("debug_maxpool: s2_host needs one entry per image")
            s2 = (ctypes.c_int32 * nimg)(*s2)
        self._ck(self.lib.jg_debug_maxpool(self.h, _ptr(x), nimg, H, W, C, s2, int(in_op), _ptr(const_in), _ptr(out)))

    def debug_conv_rowmaps(self, s2_host, layers, fill=-1):
        """Compaction maps of conv layers op = 0 .. len(layers)-1 (launch_conv_rowmaps) for the per-image counts s2_host; layers: (OH, OW) per layer.
        -> per layer (map int32 [NF*OH*OW], prefilled with `fill`: only the first `total` entries are written; base int32 [NF+1]; total)."""
        self._bind_stream()
        s2 = np.ascontiguousarray(np.asarray(s2_host, np.int32))
        NF, nl = int(s2.size), len(layers)
        maps = [np.full(NF * oh * ow, fill, np.int32) for oh, ow in layers]
        bases = [np.full(NF + 1, fill, np.int32) for _ in layers]
        totals = np.full(max(nl, 1), fill, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        OH = (_I * max(nl, 1))(*[oh for oh, _ in layers])
        OW = (_I * max(nl, 1))(*[ow for _, ow in layers])
        mp = (_P * max(nl, 1))(*[m.ctypes.data for m in maps])
        bp = (_P * max(nl, 1))(*[b.ctypes.data for b in bases])
        self._ck(self.lib.jg_debug_conv_rowmaps(self.h, s2.ctypes.data_as(i32p), NF, OH, OW, nl, mp, bp, totals.ctypes.data_as(i32p)))
        return [(maps[l], bases[l], int(totals[l])) for l in range(nl)]

    def debug_gemm32(self, A, lda, W, ldw, M, N, K, out, ldc, scale=None, bias=None, res=None, ldr=0, res_mod=0, act=0):
        self._bind_stream()
        self._ck(self.lib.jg_debug_gemm32(self.h, _ptr(A), lda, _ptr(W), ldw, M, N, K, _ptr(scale), _ptr(bias), _ptr(res), ldr, res_mod, act,
                                          _ptr(out), ldc))

    def debug_conv32(self, x, nimg, H, W, C, KH, KW, SH, SW, PH, PW, reorder, Wt, ldw, N, out, ldc, scale=None, bias=None, act=0):
        """fp32 implicit-GEMM convolution (launch_gemm32, conv): x (nimg,H,W,C) fp32 NHWC, Wt [N][ldw] fp32 in ConvGeom's tap order."""
        self._bind_stream()
        self._ck(self.lib.jg_debug_conv32(self.h, _ptr(x), nimg, H, W, C, KH, KW, SH, SW, PH, PW, int(reorder), _ptr(Wt), ldw, N, _ptr(scale),
                                          _ptr(bias), act, _ptr(out), ldc))

    def debug_gemm_x3(self, A, lda, Wh, Wl, ldw, M, N, K, out, ldc, bias=None, res=None, ldr=0, res_mod=0, relu=0):
        self._bind_stream()
        self._ck(self.lib.jg_debug_gemm_x3(self.h, _ptr(A), lda, _ptr(Wh), _ptr(Wl), ldw, M, N, K, _ptr(bias), _ptr(res), ldr, res_mod, relu,
                                           _ptr(out), ldc))

    def debug_attention(self, qkv, keymask, B, S, H, dk, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_attention(self.h, _ptr(qkv), _ptr(keymask), B, S, H, dk, _ptr(out)))

    def debug_attention_gather(self, qkv_pos, pe_qkv, Twin, P, shift, B, S, H, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_attention_gather(self.h, _ptr(qkv_pos), _ptr(pe_qkv), Twin, P, shift, B, S, H, _ptr(out)))

    def debug_attention32(self, qkv, keymask, B, S, H, dk, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_attention32(self.h, _ptr(qkv), _ptr(keymask), B, S, H, dk, _ptr(out)))

    # ---- check points of the element-wise and reduction launchers (include/jegal_hip.h): device tensors by pointer, sizes as given -- the
    # library validates them and raises JegalError(.code == JG_ERR_ARG) before anything is enqueued; `valid`: a sequence of host ints or None
    @staticmethod
    def _valid_arg(valid):
        if valid is None:
            return None, 0
        v = [int(x) for x in valid]
        return (ctypes.c_int32 * max(len(v), 1))(*v), len(v)

    def debug_stack_frames(self, src, strides, B, T, pad, H, W, dst):
        """strides = (sb, st, sh, sw, sc) in elements of src (uint8 or float32)."""
        self._bind_stream()
        sb, st, sh, sw, sc = (int(x) for x in strides)
        self._ck(self.lib.jg_debug_stack_frames(self.h, _ptr(src), int(src.dtype == torch.uint8), sb, st, sh, sw, sc, src.numel(), B, T, pad, H, W, _ptr(dst)))

    def debug_window_gather(self, conv, pe, B, P, Twin, L, D, shift, tiled, x32, x16):
        self._bind_stream()
        self._ck(self.lib.jg_debug_window_gather(self.h, _ptr(conv), _ptr(pe), B, P, Twin, L, D, shift, int(bool(tiled)), _ptr(x32), _ptr(x16)))

    def debug_layernorm(self, x, w, b, rows, D, flavour, relu, out32=None, out16=None):
        self._bind_stream()
        self._ck(self.lib.jg_debug_layernorm(self.h, _ptr(x), _ptr(w), _ptr(b), rows, D, flavour, relu, _ptr(out32), _ptr(out16)))

    def debug_layernorm_planes(self, hi, lo, w, b, rows, D, out32):
        self._bind_stream()
        self._ck(self.lib.jg_debug_layernorm_planes(self.h, _ptr(hi), _ptr(lo), _ptr(w), _ptr(b), rows, D, _ptr(out32)))

    def debug_group_mean(self, x, groups, L, D, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_group_mean(self.h, _ptr(x), groups, L, D, _ptr(out)))

    def debug_cast(self, x, out, n):
        self._bind_stream()
        self._ck(self.lib.jg_debug_cast(self.h, _ptr(x), _ptr(out), n))

    def debug_audio_conv0(self, mel, B, Tm, F, wh, wl, bias, out, valid=None):
        self._bind_stream()
        v, n = self._valid_arg(valid)
        self._ck(self.lib.jg_debug_audio_conv0(self.h, _ptr(mel), B, Tm, F, _ptr(wh), _ptr(wl), _ptr(bias), _ptr(out), v, n))

    def debug_zero_tail(self, x, valid, halvings, B, H, row_elems):
        self._bind_stream()
        v, n = self._valid_arg(valid)
        self._ck(self.lib.jg_debug_zero_tail(self.h, _ptr(x), v, n, halvings, B, H, row_elems))

    # the fp32 clones of the audit mode (audit32.hip)
    def debug_stack_frames32(self, src, strides, B, T, pad, H, W, dst):
        self._bind_stream()
        sb, st, sh, sw, sc = (int(x) for x in strides)
        u8, elems = (int(src.dtype == torch.uint8), src.numel()) if src is not None else (0, 0)
        self._ck(self.lib.jg_debug_stack_frames32(self.h, _ptr(src), u8, sb, st, sh, sw, sc, elems, B, T, pad, H, W, _ptr(dst)))

    def debug_maxpool32(self, x, out):
        """x (nimg,H,W,C) fp32 NHWC -> out (nimg,(H-3)//2+1,(W-3)//2+1,C), written in place."""
        self._bind_stream()
        nimg, H, W, C = x.shape
        self._ck(self.lib.jg_debug_maxpool32(self.h, _ptr(x), nimg, H, W, C, _ptr(out)))

    def debug_group_mean32(self, x, groups, L, D, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_group_mean32(self.h, _ptr(x), groups, L, D, _ptr(out)))

    def debug_zero_tail32(self, x, valid, halvings, B, H, row_elems):
        self._bind_stream()
        v, n = self._valid_arg(valid)
        self._ck(self.lib.jg_debug_zero_tail32(self.h, _ptr(x), v, n, halvings, B, H, row_elems))

    def debug_xlmr_embed(self, ids, B, L, D, pad_id, vocab, maxpos, word, pos, type_, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_xlmr_embed(self.h, _ptr(ids), B, L, D, pad_id, vocab, maxpos, _ptr(word), _ptr(pos), _ptr(type_), _ptr(out)))

    def debug_xlmr_embed_planes(self, ids, B, L, D, pad_id, vocab, maxpos, word, pos, type_, hi, lo, part):
        self._bind_stream()
        self._ck(self.lib.jg_debug_xlmr_embed_planes(self.h, _ptr(ids), B, L, D, pad_id, vocab, maxpos, _ptr(word), _ptr(pos), _ptr(type_), _ptr(hi),
                                                     _ptr(lo), _ptr(part)))

    def debug_ln_stats(self, part, rows, P, stats):
        self._bind_stream()
        self._ck(self.lib.jg_debug_ln_stats(self.h, _ptr(part), rows, P, _ptr(stats)))

    def debug_mask_i32_f32(self, x, out, n):
        self._bind_stream()
        self._ck(self.lib.jg_debug_mask_i32_f32(self.h, _ptr(x), _ptr(out), n))

    def debug_transpose_tokens(self, x, N, L, D, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_transpose_tokens(self.h, _ptr(x), N, L, D, _ptr(out)))

    def debug_pe_project(self, pe, S, Wh, Wl, bias, N, K, out):
        self._bind_stream()
        self._ck(self.lib.jg_debug_pe_project(self.h, _ptr(pe), S, _ptr(Wh), _ptr(Wl), _ptr(bias), N, K, _ptr(out)))

    def debug_broadcast_channels(self, v, C, out, pixels):
        self._bind_stream()
        self._ck(self.lib.jg_debug_broadcast_channels(self.h, _ptr(v), C, _ptr(out), pixels))

    def debug_col_sum(self, A, lda, M, K, scratch, out, stats=None):
        self._bind_stream()
        self._ck(self.lib.jg_debug_col_sum(self.h, _ptr(A), lda, M, K, _ptr(scratch), scratch.numel(), _ptr(out), _ptr(stats)))

    def debug_rc_bias(self, A, lda, tiled, nclips, rpc, lo, bias, N, K, scratch, out, valid=None):
        """scratch: float32, at least nclips * K elements; its first nclips * K fp16 values are the clip means afterwards."""
        self._bind_stream()
        v, n = self._valid_arg(valid)
        self._ck(self.lib.jg_debug_rc_bias(self.h, _ptr(A), lda, A.numel(), int(bool(tiled)), nclips, rpc, v, n, _ptr(lo), _ptr(bias), N, K, _ptr(scratch),
                                           scratch.numel(), _ptr(out)))

    def debug_last_kernel(self):
        buf = ctypes.create_string_buffer(128)
        self._ck(self.lib.jg_debug_last_kernel(self.h, buf, 128))
        return buf.value.decode()

    def debug_conv2_rowskip(self):
        """Leading conv2 output rows per image that the last conv stack copied instead of computing ("conv2_row_skip")."""
        rows = ctypes.c_int()
        self._ck(self.lib.jg_debug_conv2_rowskip(self.h, ctypes.byref(rows)))
        return rows.value

    def debug_conv_rows(self):
        """(computed, full) output pixels of conv2 .. conv5 in the last conv stack (per-position row skip)."""
        c, f = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
        self._ck(self.lib.jg_debug_conv_rows(self.h, c, f))
        return list(c), list(f)

    def debug_conv1_pool(self, frames_u8, pad):
        """conv1+BN+ReLU+maxpool only: (B,T,270,480,3) u8 -> (B*(T+2*pad-4),43,78,64) fp16 NHWC."""
        self._bind_stream()
        frames_u8 = frames_u8.to(self.device).contiguous()
        B, T = frames_u8.shape[:2]
        out = torch.empty((B * (T + 2 * pad - 4), 43, 78, 64), dtype=torch.float16, device=self.device)
        self._ck(self.lib.jg_debug_conv1_pool(self.h, _ptr(frames_u8), B, T, pad, _ptr(out)))
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

    def debug_gsa_conv1_pool(self, src, w, shift, out, T=None, lengths=None):
        """One launch of gsa_conv1_pool_kernel: src (N,1,80,100) (T None) or mel (B,Tm,80) with T windows per clip; w (64,9) / shift (64,) fp32
        device tensors; out (windows,19,24,64) fp16 or fp32, written in place."""
        self._bind_stream()
        clip = T is not None
        B, Tm = (src.shape[0], src.shape[1]) if clip else (src.shape[0], 0)
        v = None if lengths is None else (ctypes.c_int32 * B)(*[int(x) for x in lengths])
        self._ck(self.lib.jg_debug_gsa_conv1_pool(self.h, _ptr(src), int(clip), B, Tm, int(T) if clip else 1, v, _ptr(w), _ptr(shift), _ptr(out),
                                                  int(out.dtype == torch.float32)))

    def debug_maxpool_2x3(self, x, out):
        """One launch of maxpool_2x3_s2_kernel: x (nimg,H,W,C) fp16 or fp32 NHWC -> out (nimg,(H-2)//2+1,(W-3)//2+1,C), written in place."""
        self._bind_stream()
        nimg, H, W, C = x.shape
        self._ck(self.lib.jg_debug_maxpool_2x3(self.h, _ptr(x), nimg, H, W, C, _ptr(out), int(x.dtype == torch.float32)))

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

    def debug_span_gather(self, p32, pe, table, n_windows, span_max, D, x32, mask):
        self._bind_stream()
        self._ck(self.lib.jg_debug_span_gather(self.h, _ptr(p32), _ptr(pe), _ptr(table), n_windows, span_max, D, _ptr(x32), _ptr(mask)))

    def debug_core_compact(self, x, table, n_windows, span_max, D, out):
        """x (n_windows, span_max, D) of 2- or 4-byte elements; out rows of the same type, written in place."""
        self._bind_stream()
        self._ck(self.lib.jg_debug_core_compact(self.h, _ptr(x), x.element_size(), _ptr(table), n_windows, span_max, D, _ptr(out)))

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
