#!/usr/bin/env python3
"""Diff the kernels a rocprofv3 kernel trace saw against the kernels of the `make asm` listings (tests/kernel_matrix.py).

    make -C cuda-nbody_amd/csrc asm
    rocprofv3 --kernel-trace --stats -M -f csv -d TRACE_DIR -- python -m pytest tests/test_kernel_matrix.py -m gpu
    python tools/kernel_matrix_trace.py TRACE_DIR profiles/kernel_matrix_trace.txt

Reads every *kernel_trace.csv under TRACE_DIR (kernel names mangled or demangled), counts the dispatches per kernel, and writes the summary:
which compiled, reachable, shape-dispatched kernels the run never launched (there must be none), the UNREACHABLE ones, and the kernels
outside the shape-dispatched families that this module happens to launch or not.  Exits 1 when a reachable shape-dispatched kernel is
missing from the trace."""
import csv
import glob
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kernel_matrix as km  # noqa: E402

CSRC = os.path.join(ROOT, "cuda-nbody_amd", "csrc")


def traced_kernels(trace_dir):
    """Counter of (name, template arguments) over every dispatch of the trace; names that are not this project's kernels under None"""
    seen, foreign = Counter(), Counter()
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = (row.get("Kernel_Name") or row.get("Name") or "").strip()
                if name.endswith(".kd"):
                    name = name[:-3]
                kernel = km.parse_symbol(name) if name.startswith("_ZN2nb12_GLOBAL__N_1") else km.parse_demangled(name)
                if kernel is None:
                    foreign[name] += 1
                else:
                    seen[kernel] += 1
    return files, seen, foreign


def main(trace_dir, out_path):
    listed = []
    for name in km.LISTINGS:
        with open(os.path.join(CSRC, name)) as f:
            listed += km.listed_kernels(f.read())
    listed = list(dict.fromkeys(listed))  # a kernel two listings share as text (km.SHARED_TEXT) has one name in a trace: counted once
    files, seen, foreign = traced_kernels(trace_dir)
    unreachable = {u.kernel: u.reason for u in km.UNREACHABLE}
    dispatched = [k for k in listed if k[0] in km.FAMILIES]
    reachable = [k for k in dispatched if k not in unreachable]
    missing = [k for k in reachable if seen[k] == 0]
    others = [k for k in listed if k[0] not in km.FAMILIES]
    lines = ["kernel matrix: the kernels of a rocprofv3 --kernel-trace run of `pytest tests/test_kernel_matrix.py -m gpu` against the listings of `make asm`",
             f"trace files read: {len(files)}; dispatches of this project's kernels: {sum(seen.values())}; distinct kernels traced: {len(seen)}",
             f"kernels in the {len(km.LISTINGS)} registered listings: {len(listed)}; of shape-dispatched families: {len(dispatched)}; of these reachable: {len(reachable)}, UNREACHABLE: {len(dispatched) - len(reachable)}",
             f"compiled, reachable, shape-dispatched kernels missing from the trace: {len(missing)}"]
    lines += [f"    MISSING {km.kernel_name(k)}" for k in missing]
    lines += ["", "traced kernels that no listing holds: " + str(len([k for k in seen if k not in set(listed)]))]
    lines += [f"    {km.kernel_name(k)}" for k in seen if k not in set(listed)]
    lines += ["", "UNREACHABLE (tests/kernel_matrix.py), dispatches in the trace:"]
    lines += [f"    {seen[k]:6d}  {km.kernel_name(k)}: {why}" for k, why in unreachable.items()]
    lines += ["", "dispatches per shape-dispatched kernel:"]
    lines += [f"    {seen[k]:6d}  {km.kernel_name(k)}" for k in sorted(reachable, key=km.kernel_name)]
    lines += ["", "the other kernels (each named with its own test in tests/kernel_matrix.py OTHER), dispatches in this run:"]
    lines += [f"    {seen[k]:6d}  {km.kernel_name(k)}" for k in sorted(others, key=km.kernel_name)]
    if foreign:
        lines += ["", "dispatches of kernels from outside the project: " + ", ".join(f"{n} x {c}" for n, c in foreign.most_common(8))]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:5 + len(missing)]))
    return 1 if missing or any(seen[k] for k in unreachable) else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
