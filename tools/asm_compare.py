#!/usr/bin/env python3
"""Compares the device assembly of two builds function by function (profiles/*/asm_compare.txt).

    make -C learned_quantization_amd/csrc asm          # at the parent commit and at this one; keep the gfx950 .s of each
    python3 tools/asm_compare.py PARENT.s THIS.s [--rename PARENT_NAME=THIS_NAME ...]

A function's instruction stream is what is left of its body once labels, comments and the directives that only carry
addresses or sizes are gone; local labels that instructions name (branch targets) are renumbered in order of first use, so
that a function which merely moved inside the file compares equal.  The kernel descriptor (.amdhsa_* lines: registers, LDS,
scratch) counts as part of its function.  Runs on the CPU; exit status 1 when a function differs or is missing.
"""
import re
import sys

SKIP = re.compile(r"\.(p2align|size|type|globl|weak|protected|hidden|section|text|loc|file|cfi_\w+|ident|addrsig\w*|end_amdhsa_kernel|amdhsa_kernel|set)\b")
LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")


def functions(path):
    """{name: normalized stream} of every function (label opened by `.type name,@function`) and its kernel descriptor."""
    out, name, want = {}, None, set()
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:
            want.add(m.group(1))
            continue
        m = re.match(r"([^\s:]+):$", line)
        if m and m.group(1) in want:
            name = m.group(1)
            out[name] = []
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
            out.setdefault(name, [])
            continue
        if re.match(r"\s*\.(Lfunc_end\d+:|end_amdhsa_kernel)", line):
            name = None
            continue
        if name is None or line.endswith(":") or SKIP.match(line.strip()):
            continue
        out[name].append(" ".join(line.split()))
    norm = {}
    for fn, lines in out.items():
        seen = {}
        norm[fn] = "\n".join(LOCAL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), ln) for ln in lines)
    return norm


def renamed(fns, pairs):
    """``fns`` with every parent name of ``pairs`` replaced by this build's name, in the keys and inside the streams (a kernel that
    became an instantiation of a template keeps its stream but not its mangled name)."""
    for old, new in pairs:
        if old not in fns:
            sys.exit(f"--rename: no function {old} in the parent")
        fns = {(new if k == old else k): v.replace(old, new) for k, v in fns.items()}
    return fns


def main():
    args = sys.argv[1:]
    pairs = []
    while "--rename" in args:      # --rename PARENT_NAME=THIS_NAME, any number of times
        i = args.index("--rename")
        pairs.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = renamed(functions(args[0]), pairs), functions(args[1])
    for old, new in pairs:
        print(f"renamed: {old} -> {new}")
    same = sorted(f for f in a if f in b and a[f] == b[f])
    diff = sorted(f for f in a if f in b and a[f] != b[f])
    missing = sorted(f for f in a if f not in b)
    new = sorted(f for f in b if f not in a)
    print(f"parent functions {len(a)}, this {len(b)}, identical instruction streams {len(same)}, different {len(diff)}, "
          f"missing {len(missing)}, new {len(new)}")
    for title, names in (("different", diff), ("missing", missing), ("new", new)):
        for f in names:
            print(f"{title}: {f}")
    return 1 if diff or missing else 0


if __name__ == "__main__":
    sys.exit(main())
