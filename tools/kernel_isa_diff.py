#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code of two builds of libjegal_hip.so: what a refactor of a kernel has to show.

    python tools/kernel_isa_diff.py OLD.so NEW.so [--strict] [--rename OLDNAME=NEWNAME ...]

For every kernel it says whether the instruction stream is identical (addresses, comments, labels and directives stripped); for the
ones that differ it prints old -> new: instruction count, vgpr / sgpr count, VGPR / SGPR spills, scratch and LDS bytes
(tools/kernel_resources.py) and the number of MFMA, LDS-DMA, s_barrier and global-store instructions.  Exit status 1 if the kernel
name sets differ; with --strict also if any kernel differs.  --rename: a kernel that the refactor renamed (names without the parameter
list, as in 'sim_topk_grouped_kernel<64>=sim_topk_kernel<64, true>'); OLD's kernel is compared with, and reported as, NEW's."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, MAGIC, kernel_resources  # noqa: E402

COUNTED = (("mfma", r"v_mfma"), ("lds_dma", r"global_load_lds"), ("barrier", r"s_barrier\b"), ("gstore", r"global_store"),
           ("global_load", r"global_load_(?!lds)"))
META = ("vgpr", "sgpr", "spill", "sgpr_spill", "scratch", "lds")


def streams(lib, kernels):
    """{demangled kernel name: [instruction text]} of the kernels named in `kernels` (kernel_resources(lib)) in the library's code objects"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):
            e = starts[i + 1] if i + 1 < len(starts) else len(blob)
            part, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.co")
            open(part, "wb").write(blob[s:e])
            r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                f"--input={part}", f"--output={co}", "--unbundle"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
            raw, cur = {}, None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = raw.setdefault(m.group(1), [])
                    continue
                ins = re.sub(r"<[^>]*>", "", line.split("//")[0]).strip()
                if cur is not None and ins and not ins.startswith(".") and not ins.endswith(":"):
                    cur.append(ins)
            dem = subprocess.run(["c++filt"], input="\n".join(raw), capture_output=True, text=True).stdout.split("\n")
            for name, d in zip(raw, dem):
                if d.strip() in kernels:
                    ins = raw[name]
                    while ins and ins[-1] in ("s_nop 0", "s_code_end"):     # the padding behind the LAST kernel of a code object is not part of it
                        ins.pop()
                    out[d.strip()] = ins
    return out


def compare(so, sn, mo, mn, out=print):
    """Print the report for old / new streams (so, sn) and metadata (mo, mn); returns (names of the kernels that differ, name sets equal)."""
    for k in sorted(set(so) ^ set(sn)):
        out(("only in OLD: " if k in so else "only in NEW: ") + k)
    differ = [k for k in sorted(set(so) & set(sn)) if so[k] != sn[k] or mo[k] != mn[k]]
    for k in differ:
        out("DIFFERS  " + k + ("   (same instruction stream, other metadata)" if so[k] == sn[k] else ""))
        rows = [("instructions", len(so[k]), len(sn[k]))] + [(f, mo[k][f], mn[k][f]) for f in META]
        rows += [(n, sum(1 for x in so[k] if re.match(p, x)), sum(1 for x in sn[k] if re.match(p, x))) for n, p in COUNTED]
        out("    " + "  ".join(f"{n} {a}" if a == b else f"{n} {a} -> {b}" for n, a, b in rows))
    out(f"{len(so)} kernels in OLD, {len(sn)} in NEW: {len(set(so) & set(sn)) - len(differ)} identical, {len(differ)} differ")
    return differ, set(so) == set(sn)


def bare(name):
    """a demangled kernel name without its return type and parameter list"""
    return name.split("(")[0].replace("void ", "").strip()


def main(argv):
    strict = "--strict" in argv
    renames = dict(argv[i + 1].split("=", 1) for i, a in enumerate(argv) if a == "--rename")
    old_lib, new_lib = [a for i, a in enumerate(argv) if a not in ("--strict", "--rename") and (i == 0 or argv[i - 1] != "--rename")]
    mo, mn = kernel_resources(old_lib), kernel_resources(new_lib)
    so, sn = streams(old_lib, mo), streams(new_lib, mn)
    for old, new in renames.items():
        (ko,), (kn,) = [k for k in so if bare(k) == old], [k for k in sn if bare(k) == new]
        print(f"renamed: {old} -> {new}")
        so[kn], mo[kn] = so.pop(ko), mo.pop(ko)
    differ, same_names = compare(so, sn, mo, mn)
    return 1 if not same_names or (strict and differ) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
