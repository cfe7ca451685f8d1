"""jegal_amd/_abi.py, the parse of include/jegal_hip.h that the ctypes binding is built from: signatures and struct layouts pinned by
hand from the header's text, and the parser's refusal of whatever its grammar does not cover.  No library, no device."""
import ctypes
import os
import subprocess
import sys

import pytest

from jegal_amd import _abi

P, I, L, F, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_char_p


def test_signatures_are_the_headers():
    fn = _abi.FUNCTIONS
    assert len(fn) >= 108 and all(name.startswith("jg_") for name in fn)
    assert fn["jg_sim_coupling"][1][-1] is L and len(fn["jg_sim_coupling"][1]) == 18            # int64_t pair_ld
    assert fn["jg_spot"][1][8] is F and fn["jg_spot"][1][6:8] == [I, I]                         # int n_clips, int D, float temp
    assert fn["jg_debug_bias_correction"] == (I, [P, P, P, L, I, I, P])
    assert fn["jg_attn_talk"][1][:6] == [P, P, P, I, L, I] and fn["jg_attn_talk"][1][13] is F
    assert fn["jg_create"] == (I, [I, P]) and fn["jg_audio_len"] == (I, [I])                     # jg_handle** is a plain pointer
    assert fn["jg_set_option"] == (I, [P, S, I])
    assert fn["jg_debug_gemm_plan"][1] == [P, P, I, I, I, P, P, I, S, I, P, P, P]                # const char* const* is no string
    assert fn["jg_workspace_bytes"] == (L, [P])
    assert fn["jg_last_error"] == (S, [P]) and fn["jg_stage_name"] == (S, [I])
    assert sorted(n for n, (res, _) in fn.items() if res is not I) == ["jg_last_error", "jg_stage_name", "jg_workspace_bytes"]


def test_constants_are_the_headers():
    c = _abi.CONSTANTS
    assert (c["JG_OK"], c["JG_ERR_ARG"], c["JG_ERR_WEIGHT"]) == (0, -1, -4)
    assert [c[k] for k in ("JG_F32", "JG_F16", "JG_I64", "JG_U8")] == [0, 1, 2, 3]
    assert c["JG_PREC_FP16"] == 0 and c["JG_PREC_FP16_RC"] == 5 and c["JG_PREC_FP32"] == 6
    assert c["JG_ST_STACK"] == 0 and c["JG_ST_CONV1"] == 1 and c["JG_ST_CONV1_AUX"] == 8 and c["JG_ST_COUNT"] == 9    # continue from the one before
    assert c["JG_TRACKS_MAX_WINDOW_ROWS"] == 1048575 and c["JG_COMM_ID_BYTES"] == 128


def test_struct_layouts_are_the_headers():
    from jegal_amd._check_entries import ConvCheck, ConvShape, GemmCheck
    assert [len(_abi.STRUCTS[k]) for k in ("jg_gemm_check", "jg_conv_shape", "jg_conv_check")] == [30, 10, 26]
    assert GemmCheck._fields_[1] == ("lda", L) and GemmCheck.lda.offset == 8 and GemmCheck.M.offset == 40
    assert GemmCheck._fields_[-1] == ("a_tiled", I)
    assert ctypes.sizeof(ConvShape) == 40 and all(t is I for _, t in ConvShape._fields_)
    assert ConvCheck._fields_[0] == ("in_", P) and ConvCheck.nimg.offset == 8
    assert dict(ConvCheck._fields_)["s2_host"] is P and dict(ConvCheck._fields_)["ldw"] is L


@pytest.mark.parametrize("text", [
    "int jg_x(jg_handle* h, double scale);",                          # a parameter type without a rule
    "int jg_x(jg_handle* h, unsigned n);",
    "int jg_x(jg_handle* h, int shape[4]);",                          # the grammar has no arrays ...
    "int jg_x(jg_handle* h, void (*done)(int));",                     # ... and no function pointers
    "int jg_x(jg_handle* h, int);",                                   # a parameter without a name
    "double jg_x(jg_handle* h);",
    "enum { JG_A = 1, JG_B = JG_A + 1 };",                            # an enumerator that is no integer literal
    "enum { JG_A = 1.5 };",
    "#define JG_LIMIT (1 << 20)\n",
    "typedef struct jg_s { int a; double b; } jg_s;",
    "typedef struct jg_s { const float* a, b; } jg_s;",
    "static inline int jg_x(int a) { return a; }",
])
def test_what_the_grammar_cannot_read_raises(text):
    with pytest.raises(ValueError, match="jegal_hip.h"):
        _abi.parse("int jg_ok(jg_handle* h, int64_t n);\n" + text + "\nint jg_after(float x);\n")


def test_the_offender_is_named_and_a_good_header_parses():
    with pytest.raises(ValueError, match="jg_bad"):
        _abi.parse("int jg_bad(void (*done)(int));")
    fn, st, c = _abi.parse("/* int jg_not(int a); */ #define JG_N 0x10\nenum { JG_A = -2, JG_B, };\n"
                           "typedef struct jg_s { const void* in; int a, b; int64_t n; } jg_s;\n"
                           "const char* jg_name(const jg_s* s, const char* const* names, char* buf, float t); // int jg_nor(int a);\n")
    assert fn == {"jg_name": (S, [P, P, S, F])} and c == {"JG_N": 16, "JG_A": -2, "JG_B": -1}
    assert st == {"jg_s": [("in_", P), ("a", I), ("b", I), ("n", L)]}


def test_abi_needs_neither_torch_nor_the_library():
    code = "import sys; sys.modules['torch'] = None; sys.modules['numpy'] = None; import jegal_amd._abi as a; print(len(a.FUNCTIONS))"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(_abi.HEADER_PATH)))
    assert out.returncode == 0 and int(out.stdout) == len(_abi.FUNCTIONS), out.stderr
