#!/usr/bin/env python3
"""The traced launches of tests/test_gpu_group_forms.py next to what tests/_group_forms.py::launch_shape predicts.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 -m pytest -q -m gpu tests/test_gpu_group_forms.py
    python3 tools/group_forms_trace.py DIR > profiles/group_forms/kernel_coverage.txt

Part 1: the group-wise instantiations the library ships (tools/kernel_coverage.py: the device stubs of liblq_hip.so) and how often the
run launched each.  Part 2: ``test_forms`` runs first and launches, per (case, variant) in table order, forward, backward, forward,
backward of the single-tensor kernels; these are the first k_group_cols / k_group_rows launches of the trace by start time.  Each is
printed with its kernel and grid (in blocks) next to the prediction; a disagreement means the restatement is wrong.
Exit status 1 on an unlaunched group instantiation or a disagreement."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kernel_coverage import norm, shipped                      # noqa: E402
from _group_forms import VARIANTS, form_variants, launch_shape  # noqa: E402

FAMILIES = ("lq::k_group_cols<", "lq::k_group_rows<", "lq::k_group_batch<")


def launches(path):
    rows = []
    for d, _, fs in os.walk(path):
        for f in fs:
            if f.endswith("kernel_trace.csv"):
                with open(os.path.join(d, f), newline="") as fh:
                    for r in csv.DictReader(fh):
                        k = norm(r["Kernel_Name"])
                        if k.startswith(FAMILIES):
                            grid = tuple(int(r["Grid_Size_" + a]) // max(int(r["Workgroup_Size_" + a]), 1) for a in "XYZ")
                            rows.append((int(r["Start_Timestamp"]), k, grid))
    return [(k, g) for _, k, g in sorted(rows)]


def predicted(case, variant, bwd):
    _, rounding = VARIANTS[variant]
    d = launch_shape(*case)
    rne = int(rounding == "nearest")
    if d["form"].startswith("cols"):
        v, tx = (4, 16) if d["form"] == "cols4" else (1, 64)
        return f"lq::k_group_cols<{rne},{int(bwd)},{v},{tx}>", (d["tiles"], d["grid_y"], 1 if bwd else d["nz"])
    return f"lq::k_group_rows<{rne},{int(bwd)},{4 if d['form'] == 'rows4' else 1}>", (d["blocks"], 1, 1)


def main():
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    run = launches(sys.argv[1])
    ship = sorted(k for k in shipped() if k.startswith(FAMILIES))
    count = {}
    for k, _ in run:
        count[k] = count.get(k, 0) + 1
    missing = [k for k in ship if k not in count]
    print(f"# group-wise instantiations: {len(ship)} shipped, {len(ship) - len(missing)} launched by tests/test_gpu_group_forms.py "
          f"({len(run)} launches)")
    for k in ship:
        print(f"{count.get(k, 0):6d}  {k}")
    print("#\n# test_forms: traced launch | predicted by launch_shape (grid in blocks, x y z)")
    single = [(k, g) for k, g in run if not k.startswith("lq::k_group_batch<")]
    bad, i = 0, 0
    for case, variant in form_variants():
        d = launch_shape(*case)
        extra = (f"team {d['team']}, {d['dead']} dead teams" if "team" in d else
                 f"trips {d['trips']}, nz {d['nz']}{' (capped)' if d['capped'] else ''}, {d['dead']} dead lanes")
        print(f"# {case} {variant}: {d['form']}, nb {d['nb']}, last group {d['last']}, {extra}")
        for bwd in (False, True, False, True):
            want = predicted(case, variant, bwd)
            got = single[i] if i < len(single) else ("(no launch)", ())
            ok = got == want
            bad += not ok
            print(f"  {'AGREE    ' if ok else 'DIFFERENT'} {got[0]} {got[1]} | {want[0]} {want[1]}")
            i += 1
    print(f"# disagreements: {bad}; group instantiations never launched: {len(missing)}")
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main())
