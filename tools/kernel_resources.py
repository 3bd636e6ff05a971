#!/usr/bin/env python3
"""Tabulates the compiler's resource report of two builds kernel by kernel (profiles/*/kernel_resources.txt).

    make -C learned_quantization_amd/csrc asm 2> REPORT      # at the parent commit and at this one (-Rpass-analysis=kernel-resource-usage)
    python3 tools/kernel_resources.py PARENT_REPORT THIS_REPORT 'k_group_batch<' 'k_group_(affine_)?(cols|rows)<' 'k_group_batch_affine<'

Each further argument is a regular expression on the demangled kernel name and opens a group of the table.  Per kernel: VGPRs,
AGPRs, SGPRs, LDS bytes per block, scratch bytes per lane and the occupancy in waves per SIMD, of the parent and of this build.
Runs on the CPU; exit status 1 when a kernel of the parent is missing or has other figures in this build, or a kernel has scratch.
"""
import re
import shutil
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs", "TotalSGPRs"), ("LDS", "LDS Size [bytes/block]"),
          ("scratch", "ScratchSize [bytes/lane]"), ("waves", "Occupancy [waves/SIMD]"))


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if tool is None or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {n: re.sub(r"^void |\(.*$|lq::", "", d) for n, d in zip(names, out)}


def report(path):
    """{demangled kernel name: {field: int}}"""
    raw, name = {}, None
    for line in open(path, errors="replace"):
        if "remark:" not in line:      # "FILE:L:C: remark: ..." or, with -save-temps, "remark: FILE:L:C: ..."
            continue
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            raw[name] = {}
            continue
        m = re.search(r":\s+([A-Za-z][^:]*): (\d+) \[-Rpass-analysis", line)
        if m and name is not None:
            raw[name][m.group(1)] = int(m.group(2))
    names = demangle(list(raw))
    return {names[n]: v for n, v in raw.items()}


def row(figures):
    if figures is None:
        return "-".rjust(sum(max(5, len(head)) + 1 for head, _ in FIELDS) - 1)
    return " ".join(f"{figures[key]:>{max(5, len(head))}}" for head, key in FIELDS)


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    parent, this = report(sys.argv[1]), report(sys.argv[2])
    head = " ".join(f"{h:>{max(5, len(h))}}" for h, _ in FIELDS)
    bad = 0
    for pattern in sys.argv[3:]:
        print(f"-- {pattern}")
        print(f"{'kernel':<46} | parent: {head} |   this: {head} |")
        for k in sorted(n for n in set(parent) | set(this) if re.search(pattern, n)):
            a, b = parent.get(k), this.get(k)
            verdict = "new" if a is None else ("missing" if b is None else ("identical" if a == b else "DIFFERENT"))
            if verdict in ("missing", "DIFFERENT") or (b or a)["ScratchSize [bytes/lane]"]:
                bad = 1
            print(f"{k:<46} |         {row(a)} |         {row(b)} | {verdict}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
