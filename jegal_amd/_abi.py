"""The C ABI as include/jegal_hip.h declares it, read once: the header is the only declaration of an entry's types, of the check-point
structs and of the enum values, and _lib.py builds its ctypes binding from what this module parses.

Pure Python, no torch, no library, no device.  The parser knows a small grammar -- prototypes `ret jg_name(type name, ...);`, `typedef
struct name { fields } name;`, anonymous enums, integer `#define JG_*` -- and fails closed: whatever it cannot read raises ValueError
when the package is imported, nothing is skipped.
"""
import ctypes
import keyword
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jegal_hip.h")

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"


def ctype_of(ctype):
    """A C type as written (`int`, `const float*`, `const char* const*`) -> its ctypes type.  The one rule for parameters, struct fields
    and returns: int / int64_t / float by value, `char*` of any constness c_char_p, every other pointer c_void_p."""
    words = ctype.replace("*", " * ").split()
    base = [w for w in words if w not in ("const", "*")]
    stars = words.count("*")
    if len(base) != 1 or not re.fullmatch(r"[A-Za-z_]\w*", base[0]) or (stars == 0 and base[0] not in _SCALARS):
        raise ValueError(f"include/jegal_hip.h: no ctypes rule for the type `{ctype.strip()}`")
    if stars == 0:
        return _SCALARS[base[0]]
    return ctypes.c_char_p if (stars == 1 and base[0] == "char") else ctypes.c_void_p


def _declarations(text, sep, where):
    """`type name` declarations separated by `sep`, a type shared by `type a, b, c` (scalars only) -> [(name, ctypes type)]."""
    out = []
    for decl in (d.strip() for d in text.split(sep)):
        if not decl:
            continue
        first, *more = [p.strip() for p in decl.split(",")]
        m = re.fullmatch(r"(.*[\w*])\s*\b([A-Za-z_]\w*)", first, re.S)
        if not m or not all(re.fullmatch(r"[A-Za-z_]\w*", p) for p in more) or (more and "*" in m.group(1)):
            raise ValueError(f"include/jegal_hip.h: cannot read the declaration `{decl}` of {where}")
        out += [(name, ctype_of(m.group(1))) for name in [m.group(2)] + more]
    return out


def _integer(value, where):
    if not re.fullmatch(_INT, value.strip()):
        raise ValueError(f"include/jegal_hip.h: {where} is not an integer literal: `{value.strip()}`")
    return int(value.strip(), 0)


def parse(text):
    """Header text -> (functions {name: (restype, [argtypes])}, structs {name: [(field, ctype)]}, constants {name: int})."""
    functions, structs, constants = {}, {}, {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#\s*ifdef\s+__cplusplus\b.*?^[ \t]*#\s*endif\b[^\n]*", " ", text, flags=re.S | re.M)      # extern "C" { and its }

    def define(m):
        if m.group(1).startswith("JG_"):
            constants[m.group(1)] = _integer(m.group(2), f"#define {m.group(1)}")
        return " "
    text = re.sub(r"^[ \t]*#\s*define\s+(\w+)\b([^\n]*)", define, text, flags=re.M)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)

    def enum(m):
        value = -1
        for item in (i.strip() for i in m.group(1).split(",")):
            if not item:
                continue
            name, eq, v = (p.strip() for p in item.partition("="))
            if not re.fullmatch(r"[A-Za-z_]\w*", name):
                raise ValueError(f"include/jegal_hip.h: cannot read the enumerator `{item}`")
            value = _integer(v, f"enumerator {name}") if eq else value + 1
            constants[name] = value
        return " "
    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)

    def struct(m):
        if m.group(1) != m.group(3):
            raise ValueError(f"include/jegal_hip.h: struct {m.group(1)} is typedef'd as {m.group(3)}")
        structs[m.group(1)] = [(n + "_" if keyword.iskeyword(n) else n, t) for n, t in _declarations(m.group(2), ";", f"struct {m.group(1)}")]
        return " "
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", " ", text)                                                    # opaque handle types

    for stmt in (s.strip() for s in text.split(";")):
        if not stmt:
            continue
        m = re.fullmatch(r"([\w\s*]*[\w*])\s*\b(jg_[a-z0-9_]+)\s*\(([^()]*)\)", stmt)
        if not m:
            name = re.search(r"jg_[a-z0-9_]+(?=\s*\()", stmt)
            raise ValueError("include/jegal_hip.h: cannot read " + (f"the prototype of {name.group(0)}" if name else f"`{stmt[:80]}`"))
        functions[m.group(2)] = (ctype_of(m.group(1)), [t for _, t in _declarations(m.group(3), ",", m.group(2))])
    return functions, structs, constants


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} not found: jegal_amd binds libjegal_hip.so from the header's declarations and keeps no copy of "
                           "them; the package needs include/ next to it, as in the source tree.")
    with open(HEADER_PATH) as f:
        return f.read()


FUNCTIONS, STRUCTS, CONSTANTS = parse(_read_header())
