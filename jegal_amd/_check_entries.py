"""The kernel check points of the engine (jg_debug_*, include/jegal_hip.h) as a class that Engine (_lib.py) inherits from, with the
structs two of them take.  A check point is one production launch on caller-owned device tensors, asynchronous on the engine's stream;
a shape the launcher rejects raises JegalError with .code == JG_ERR_ARG.  debug_last_kernel() names the instance."""
import ctypes

import numpy as np
import torch

from . import _abi

_P = ctypes.c_void_p
_I = ctypes.c_int


class GemmCheck(ctypes.Structure):
    """struct jg_gemm_check (include/jegal_hip.h): operands of one jg_debug_gemm_check launch."""
    _fields_ = _abi.STRUCTS["jg_gemm_check"]
class ConvCheck(ctypes.Structure):
    """struct jg_conv_check (include/jegal_hip.h): operands of one jg_debug_conv_check launch (`in_` for its `in`)."""
    _fields_ = _abi.STRUCTS["jg_conv_check"]
class ConvShape(ctypes.Structure):
    """struct jg_conv_shape (include/jegal_hip.h): the part of a conv geometry the GEMM planner reads."""
    _fields_ = _abi.STRUCTS["jg_conv_shape"]


def _i32_array(values, n=None):
    """Host ints -> a ctypes int32 array (n entries when the caller knows the count); None stays None."""
    if values is None:
        return None
    v = [int(x) for x in values]
    return (ctypes.c_int32 * (len(v) if n is None else n))(*v)


class CheckPoints:
    """Engine's debug_* methods.  Uses Engine's handle (lib, h, device) and helpers (_call, _ck, _bind_stream)."""

    def debug_gemm(self, M, N, K, mode=0, iters=10, a16=None, w16=None):
        """ms per launch of the production GEMM; a16 (M,K) / w16 (N,K): optional fp16 cuda operands (else constant fill)."""
        ms = ctypes.c_double()
        for t, shp in ((a16, (M, K)), (w16, (N, K))):
            if t is not None and (t.dtype != torch.float16 or tuple(t.shape) != shp or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"debug_gemm operand must be a contiguous fp16 {shp} tensor on {self.device}")
        self._call("jg_debug_gemm_ex", a16, w16, M, N, K, mode, iters, ctypes.byref(ms))
        return ms.value

    def _check_struct(self, c, kw, who):
        """Keyword arguments -> the fields of c; tensors, which must live on the engine's device, by pointer."""
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                if v.device != self.device:
                    raise ValueError(f"{who}: {k} must be on {self.device}")
                v = v.data_ptr()
            setattr(c, "in_" if k == "in" else k, v)
        return c

    def debug_gemm_check(self, **kw):
        """Linear GEMM (launch_gemm): keyword arguments are the fields of jg_gemm_check; tensors are passed by pointer."""
        self._call("jg_debug_gemm_check", ctypes.byref(self._check_struct(GemmCheck(), kw, "debug_gemm_check")))

    def debug_conv_check(self, **kw):
        """Implicit-GEMM convolution (launch_gemm, conv): keyword arguments are the fields of jg_conv_check (`in_` for its `in`); tensors are
        passed by pointer, s2_host is a sequence of nimg ints (or None)."""
        s2 = kw.pop("s2_host", None)
        c = self._check_struct(ConvCheck(), kw, "debug_conv_check")
        if s2 is not None:
            keep = _i32_array(s2)
            if len(keep) != c.nimg:
                raise ValueError("debug_conv_check: s2_host needs one entry per image")
            c.s2_host = ctypes.cast(keep, _P)
        self._call("jg_debug_conv_check", ctypes.byref(c))

    def debug_maxpool(self, x, out, s2_host=None, in_op=0, const_in=None):
        """3x3 / stride 2 max-pool (launch_maxpool3x3s2): x (nimg,H,W,C) 16-bit NHWC -> out (nimg,(H-3)//2+1,(W-3)//2+1,C), written in place.
        s2_host (nimg ints) / in_op / const_in (H,W,C): input rows below conv_skip_decode(s2, in_op) come from const_in."""
        nimg, H, W, C = x.shape
        s2 = _i32_array(s2_host)
        if s2 is not None and len(s2) != nimg:
            raise ValueError("debug_maxpool: s2_host needs one entry per image")
        self._call("jg_debug_maxpool", x, nimg, H, W, C, s2, int(in_op), const_in, out)

    def debug_conv_rowmaps(self, s2_host, layers, fill=-1):
        """Compaction maps of conv layers op = 0 .. len(layers)-1 (launch_conv_rowmaps) for the per-image counts s2_host; layers: (OH, OW) per layer.
        -> per layer (map int32 [NF*OH*OW], prefilled with `fill`: only the first `total` entries are written; base int32 [NF+1]; total)."""
        s2 = np.ascontiguousarray(np.asarray(s2_host, np.int32))
        NF, nl = int(s2.size), len(layers)
        maps = [np.full(NF * oh * ow, fill, np.int32) for oh, ow in layers]
        bases = [np.full(NF + 1, fill, np.int32) for _ in layers]
        totals = np.full(max(nl, 1), fill, np.int32)
        OH = (_I * max(nl, 1))(*[oh for oh, _ in layers])
        OW = (_I * max(nl, 1))(*[ow for _, ow in layers])
        mp = (_P * max(nl, 1))(*[m.ctypes.data for m in maps])
        bp = (_P * max(nl, 1))(*[b.ctypes.data for b in bases])
        self._call("jg_debug_conv_rowmaps", s2.ctypes.data, NF, OH, OW, nl, mp, bp, totals.ctypes.data)
        return [(maps[l], bases[l], int(totals[l])) for l in range(nl)]

    def debug_gemm32(self, A, lda, W, ldw, M, N, K, out, ldc, scale=None, bias=None, res=None, ldr=0, res_mod=0, act=0):
        self._call("jg_debug_gemm32", A, lda, W, ldw, M, N, K, scale, bias, res, ldr, res_mod, act, out, ldc)

    def debug_conv32(self, x, nimg, H, W, C, KH, KW, SH, SW, PH, PW, reorder, Wt, ldw, N, out, ldc, scale=None, bias=None, act=0):
        """fp32 implicit-GEMM convolution (launch_gemm32, conv): x (nimg,H,W,C) fp32 NHWC, Wt [N][ldw] fp32 in ConvGeom's tap order."""
        self._call("jg_debug_conv32", x, nimg, H, W, C, KH, KW, SH, SW, PH, PW, int(reorder), Wt, ldw, N, scale, bias, act, out, ldc)

    def debug_gemm_x3(self, A, lda, Wh, Wl, ldw, M, N, K, out, ldc, bias=None, res=None, ldr=0, res_mod=0, relu=0):
        self._call("jg_debug_gemm_x3", A, lda, Wh, Wl, ldw, M, N, K, bias, res, ldr, res_mod, relu, out, ldc)

    def debug_attention(self, qkv, keymask, B, S, H, dk, out):
        self._call("jg_debug_attention", qkv, keymask, B, S, H, dk, out)

    def debug_attention_gather(self, qkv_pos, pe_qkv, Twin, P, shift, B, S, H, out):
        self._call("jg_debug_attention_gather", qkv_pos, pe_qkv, Twin, P, shift, B, S, H, out)

    def debug_attention32(self, qkv, keymask, B, S, H, dk, out):
        self._call("jg_debug_attention32", qkv, keymask, B, S, H, dk, out)

    # ---- check points of the element-wise and reduction launchers (include/jegal_hip.h): device tensors by pointer, sizes as given -- the
    # library validates them and raises JegalError(.code == JG_ERR_ARG) before anything is enqueued; `valid`: a sequence of host ints or None
    @staticmethod
    def _valid_arg(valid):
        if valid is None:
            return None, 0
        v = [int(x) for x in valid]
        return _i32_array(v, max(len(v), 1)), len(v)

    def debug_stack_frames(self, src, strides, B, T, pad, H, W, dst):
        """strides = (sb, st, sh, sw, sc) in elements of src (uint8 or float32)."""
        sb, st, sh, sw, sc = (int(x) for x in strides)
        self._call("jg_debug_stack_frames", src, int(src.dtype == torch.uint8), sb, st, sh, sw, sc, src.numel(), B, T, pad, H, W, dst)

    def debug_window_gather(self, conv, pe, B, P, Twin, L, D, shift, tiled, x32, x16):
        self._call("jg_debug_window_gather", conv, pe, B, P, Twin, L, D, shift, int(bool(tiled)), x32, x16)

    def debug_layernorm(self, x, w, b, rows, D, flavour, relu, out32=None, out16=None):
        self._call("jg_debug_layernorm", x, w, b, rows, D, flavour, relu, out32, out16)

    def debug_layernorm_planes(self, hi, lo, w, b, rows, D, out32):
        self._call("jg_debug_layernorm_planes", hi, lo, w, b, rows, D, out32)

    def debug_group_mean(self, x, groups, L, D, out):
        self._call("jg_debug_group_mean", x, groups, L, D, out)

    def debug_cast(self, x, out, n):
        self._call("jg_debug_cast", x, out, n)

    def debug_audio_conv0(self, mel, B, Tm, F, wh, wl, bias, out, valid=None):
        self._call("jg_debug_audio_conv0", mel, B, Tm, F, wh, wl, bias, out, *self._valid_arg(valid))

    def debug_zero_tail(self, x, valid, halvings, B, H, row_elems):
        self._call("jg_debug_zero_tail", x, *self._valid_arg(valid), halvings, B, H, row_elems)

    # the fp32 clones of the audit mode (audit32.hip)
    def debug_stack_frames32(self, src, strides, B, T, pad, H, W, dst):
        sb, st, sh, sw, sc = (int(x) for x in strides)
        u8, elems = (int(src.dtype == torch.uint8), src.numel()) if src is not None else (0, 0)
        self._call("jg_debug_stack_frames32", src, u8, sb, st, sh, sw, sc, elems, B, T, pad, H, W, dst)

    def debug_maxpool32(self, x, out):
        """x (nimg,H,W,C) fp32 NHWC -> out (nimg,(H-3)//2+1,(W-3)//2+1,C), written in place."""
        nimg, H, W, C = x.shape
        self._call("jg_debug_maxpool32", x, nimg, H, W, C, out)

    def debug_group_mean32(self, x, groups, L, D, out):
        self._call("jg_debug_group_mean32", x, groups, L, D, out)

    def debug_zero_tail32(self, x, valid, halvings, B, H, row_elems):
        self._call("jg_debug_zero_tail32", x, *self._valid_arg(valid), halvings, B, H, row_elems)

    def debug_xlmr_embed(self, ids, B, L, D, pad_id, vocab, maxpos, word, pos, type_, out):
        self._call("jg_debug_xlmr_embed", ids, B, L, D, pad_id, vocab, maxpos, word, pos, type_, out)

    def debug_xlmr_embed_planes(self, ids, B, L, D, pad_id, vocab, maxpos, word, pos, type_, hi, lo, part):
        self._call("jg_debug_xlmr_embed_planes", ids, B, L, D, pad_id, vocab, maxpos, word, pos, type_, hi, lo, part)

    def debug_ln_stats(self, part, rows, P, stats):
        self._call("jg_debug_ln_stats", part, rows, P, stats)

    def debug_mask_i32_f32(self, x, out, n):
        self._call("jg_debug_mask_i32_f32", x, out, n)

    def debug_transpose_tokens(self, x, N, L, D, out):
        self._call("jg_debug_transpose_tokens", x, N, L, D, out)

    def debug_pe_project(self, pe, S, Wh, Wl, bias, N, K, out):
        self._call("jg_debug_pe_project", pe, S, Wh, Wl, bias, N, K, out)

    def debug_broadcast_channels(self, v, C, out, pixels):
        self._call("jg_debug_broadcast_channels", v, C, out, pixels)

    def debug_col_sum(self, A, lda, M, K, scratch, out, stats=None):
        self._call("jg_debug_col_sum", A, lda, M, K, scratch, scratch.numel(), out, stats)

    def debug_rc_bias(self, A, lda, tiled, nclips, rpc, lo, bias, N, K, scratch, out, valid=None):
        """scratch: float32, at least nclips * K elements; its first nclips * K fp16 values are the clip means afterwards."""
        self._call("jg_debug_rc_bias", A, lda, A.numel(), int(bool(tiled)), nclips, rpc, *self._valid_arg(valid), lo, bias, N, K, scratch,
                   scratch.numel(), out)

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
        frames_u8 = frames_u8.to(self.device).contiguous()
        B, T = frames_u8.shape[:2]
        out = torch.empty((B * (T + 2 * pad - 4), 43, 78, 64), dtype=torch.float16, device=self.device)
        self._call("jg_debug_conv1_pool", frames_u8, B, T, pad, out)
        return out

    def debug_gsa_conv1_pool(self, src, w, shift, out, T=None, lengths=None):
        """One launch of gsa_conv1_pool_kernel: src (N,1,80,100) (T None) or mel (B,Tm,80) with T windows per clip; w (64,9) / shift (64,) fp32
        device tensors; out (windows,19,24,64) fp16 or fp32, written in place."""
        clip = T is not None
        B, Tm = (src.shape[0], src.shape[1]) if clip else (src.shape[0], 0)
        self._call("jg_debug_gsa_conv1_pool", src, int(clip), B, Tm, int(T) if clip else 1, _i32_array(lengths, B), w, shift, out,
                   int(out.dtype == torch.float32))

    def debug_maxpool_2x3(self, x, out):
        """One launch of maxpool_2x3_s2_kernel: x (nimg,H,W,C) fp16 or fp32 NHWC -> out (nimg,(H-2)//2+1,(W-3)//2+1,C), written in place."""
        nimg, H, W, C = x.shape
        self._call("jg_debug_maxpool_2x3", x, nimg, H, W, C, out, int(x.dtype == torch.float32))

    def debug_span_gather(self, p32, pe, table, n_windows, span_max, D, x32, mask):
        self._call("jg_debug_span_gather", p32, pe, table, n_windows, span_max, D, x32, mask)

    def debug_core_compact(self, x, table, n_windows, span_max, D, out):
        """x (n_windows, span_max, D) of 2- or 4-byte elements; out rows of the same type, written in place."""
        self._call("jg_debug_core_compact", x, x.element_size(), table, n_windows, span_max, D, out)
