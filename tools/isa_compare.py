#!/usr/bin/env python3
"""Compare the device assembly of two builds, function by function.

    tools/isa_compare.py --emit DIR [FILE.hip ...]   compile csrc/*.hip (or the named files) to DIR/*.s, device side only,
                                                     with the flags of csrc/Makefile
    tools/isa_compare.py OLD_DIR NEW_DIR             compare the *.s files the two directories share

A function's body is the text from its label to its .Lfunc_end, without comments, debug / ident lines and the numbering of
local labels; a kernel's resources are five values of its metadata record.  Prints one line per file and the names of the
functions whose body or resources differ (with the size of the body's diff); exit status 1 if any does.  A refactoring that
only moves inline code between sources should leave every function as it was.
"""
import difflib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "genomics_general_amd", "csrc")
FLAGS = "-O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -x hip --offload-arch=gfx950 --cuda-device-only -S".split()
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def emit(out_dir, files):
    os.makedirs(out_dir, exist_ok=True)
    files = files or sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = [(f, subprocess.Popen([hipcc, *FLAGS, os.path.basename(f), "-o", os.path.abspath(os.path.join(out_dir, os.path.basename(f)[:-4] + ".s"))],
                                 cwd=CSRC)) for f in files]
    bad = [f for f, p in jobs if p.wait() != 0]
    if bad:
        sys.exit("failed: " + " ".join(bad))


def functions(text):
    """name -> normalised body lines"""
    out, name, body = {}, None, []
    types = set(re.findall(r"^\t\.type\t(\S+),@function", text, re.M))
    for line in text.split("\n"):
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
            if m and m.group(1) in types:
                name, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name] = body
            name = None
            continue
        line = line.split(";")[0].rstrip()
        if not line or re.match(r"^\s*\.(loc|file|ident|cfi_\w+)\b", line):
            continue
        body.append(re.sub(r"\.L(BB|tmp|Ltmp)\d+_", r".L\1_", line))
    return out


def resources(text):
    """kernel name -> the five resource values of its metadata record"""
    m = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.target:", text, re.M | re.S)
    out = {}
    for rec in re.split(r"^  - ", m.group(1) if m else "", flags=re.M)[1:]:
        fields = dict(re.findall(r"^(?:    )?(\.\w+):\s+(\S+)$", rec, re.M))         # the record's own keys: four spaces (none on its first line)
        out[fields[".name"]] = tuple(fields.get(k) for k in RESOURCES)
    return out


def compare(old_dir, new_dir):
    names = sorted(set(os.listdir(old_dir)) & set(os.listdir(new_dir)))
    names = [n for n in names if n.endswith(".s")]
    differ = 0
    for n in names:
        old, new = open(os.path.join(old_dir, n)).read(), open(os.path.join(new_dir, n)).read()
        fo, fn, ro, rn = functions(old), functions(new), resources(old), resources(new)
        lines = []
        for f in sorted(set(fo) | set(fn)):
            kind = "kernel" if f in ro or f in rn else "function"
            if f not in fo or f not in fn:
                lines.append("  %s %s: only in %s" % (kind, f, "OLD" if f in fo else "NEW"))
            elif fo[f] != fn[f]:
                d = [x for x in difflib.unified_diff(fo[f], fn[f], lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---")]
                lines.append("  %s %s: body differs, %d of %d lines (-%d +%d)" % (kind, f, len(d), len(fo[f]), sum(x[0] == "-" for x in d),
                                                                                 sum(x[0] == "+" for x in d)))
            if f in ro and f in rn and ro[f] != rn[f]:
                lines.append("  kernel %s: resources differ: %s" % (f, ", ".join("%s %s -> %s" % (k[1:], a, b) for k, a, b in zip(RESOURCES, ro[f], rn[f]) if a != b)))
        print("%s: %d kernels, %d functions, %s" % (n, len(rn), len(fn), "%d differ" % len(lines) if lines else "identical"))
        for x in lines:
            print(x)
        differ += len(lines)
    print("total: %d files, %d differences" % (len(names), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--emit":
        emit(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) == 3:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
