#!/usr/bin/env python3
"""Acceleration, jerk and potential at points of the caller's own (nb_field_eval_f32, include/nbody_hip_field.h) by the number of
targets, next to nb_hermite_eval_f32 and the one-sided FAST step (nb_integrate_f32 without a workspace) timed in the same process.
One JSON line per point: fp32, N = 65 536 and 262 144 sources, M = 1, 128, 1 024, 8 192 and N targets (M < N: points off the sources,
nobody excluded; M = N: targets == sources, self_index = arange), without and with the jerk: microseconds per call (median of
--repeats single calls, device events), interactions per second (N * M per call), the geometry the plan query reports, the ratio to
the yardstick of the same N scaled by M / N (the one-sided step without the jerk, nb_hermite_eval_f32 with it) and that ratio over
the issue-cost model of the loops as compiled (13 packed + 2 v_rsq_f32 per packed pair against the step's 11 + 2; 27 + 2 against
hermite_eval's 25 + 2; a packed op every 4.08 and a v_rsq_f32 every 8.3 SIMD cycles: DESIGN.md 5.9).  M = N is also timed without
self_index: what the MASK form of the loop costs.

The library measured is the one NBODY_HIP_FIELD_LIB names (default: the package's), so builds with another workgroup target
(make -C cuda-nbody_amd/csrc EXP=-DNB_FIELD_TARGET=1024 ...) are timed by the same script; `ranges` in each line says what J it chose.

Kernel times come from one separate run under the profiler, with the program after `--`:
    rocprofv3 --kernel-trace --stats -d DIR -o field -- python tools/field_bench.py --calls 5 --sequence DIR/sequence.json
    python tools/field_bench.py --summarise DIR --out profiles/field_kernel_stats.csv
--calls K issues every point K times and nothing else (no events, no yardsticks); --sequence records the order of the points, which
--summarise lays over the field_* dispatches of the trace, in order: median, smallest and largest time of field_eval and of
field_finish per point.

  python tools/field_bench.py [--repeats 9] [--label TEXT] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

SOURCES = (65536, 262144)
PK_CYCLES, RSQ_CYCLES = 4.08, 8.3
MODEL_PLAIN = (13 * PK_CYCLES + 2 * RSQ_CYCLES) / (11 * PK_CYCLES + 2 * RSQ_CYCLES)
MODEL_JERK = (27 * PK_CYCLES + 2 * RSQ_CYCLES) / (25 * PK_CYCLES + 2 * RSQ_CYCLES)


def targets_of(n):
    return (1, 128, 1024, 8192, n)


def cloud(n, dtype, seed=1):
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3], pos[:, 3], vel[:, :3] = rng.standard_normal((n, 3)), 1.0 / n, rng.standard_normal((n, 3)) * 0.3
    return pos, vel


def median_ms(pkg, fn, repeats):
    fn(), fn()
    times = []
    for _ in range(repeats):
        pkg.check(pkg.lib().nb_device_synchronize(), "nb_device_synchronize")
        start, stop = pkg.Event(), pkg.Event()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_ms(stop))
    return sorted(times)[len(times) // 2]


class Points:
    """the device arrays of one N: the sources, M <= 8 192 points off them, and one probe for every M"""

    def __init__(self, pkg, n):
        self.pkg, self.n, dtype = pkg, n, np.float32
        self.pos, self.vel = cloud(n, dtype)
        self.eps2 = dtype(0.01)
        self.probe = pkg.FieldProbe(n, n, dtype, softening_sq=self.eps2)
        self.probe._src.upload(self.pos), self.probe._src_vel.upload(self.vel)
        off, off_vel = cloud(8192, dtype, 2)
        self.probe._tgt.upload(off), self.probe._tgt_vel.upload(off_vel)
        self.probe._self.upload(np.arange(n, dtype=np.uint32))

    def call(self, m, jerk, exclude=True):
        p = self.probe
        own = m == self.n  # targets == sources, self_index = arange
        p.enqueue(p._src, p._src if own else p._tgt, p._src_vel if jerk else None, (p._src_vel if own else p._tgt_vel) if jerk else None, p._self if own and exclude else None,
                  num_targets=m, jerks=jerk)

    def free(self):
        self.probe.free()


def timed_points(pkg, n, repeats):
    dtype = np.float32
    points = Points(pkg, n)
    lib = pkg.lib()
    pkg.set_softening_squared(points.eps2)
    shared = pkg.HermiteSystem(n, dtype, softening_sq=points.eps2)
    shared.set_state(points.pos, points.vel)
    t_hermite = median_ms(pkg, shared.eval, repeats)
    shared.free()
    here, other, velocities = pkg.DeviceBuffer(points.pos.nbytes), pkg.DeviceBuffer(points.pos.nbytes), pkg.DeviceBuffer(points.pos.nbytes)
    here.upload(points.pos), velocities.upload(points.vel)
    state = {"read": here.ptr.value, "write": other.ptr.value}

    def euler():
        pkg.check(lib.nb_integrate_f32(state["write"], state["read"], velocities.ptr, np.float32(1e-4), np.float32(1.0), n, 256, pkg.NB_MODE_FAST, None), "nb_integrate")
        state["read"], state["write"] = state["write"], state["read"]

    t_euler = median_ms(pkg, euler, repeats)
    for buf in (here, other, velocities):
        buf.free()
    for m in targets_of(n):
        for jerk in (False, True):
            t = median_ms(pkg, lambda: points.call(m, jerk), repeats)
            plan = pkg.field_plan(n, m, dtype)
            yardstick, model = (t_hermite, MODEL_JERK) if jerk else (t_euler, MODEL_PLAIN)
            ratio = t / (yardstick * m / n)
            row = {"precision": "fp32", "num_sources": n, "num_targets": m, "jerk": jerk, "tiles": plan.tiles, "ranges": plan.ranges, "groups": plan.groups,
                   "waves_per_group": plan.waves_per_group, "launches": plan.launches, "call_us": round(t * 1e3, 2), "interactions_per_s": float(n) * m / (t * 1e-3),
                   "yardstick": "nb_hermite_eval_f32" if jerk else "nb_integrate_f32 one-sided", "yardstick_us": round(yardstick * 1e3, 2),
                   "fraction_of_yardstick": t / yardstick, "ratio_per_interaction": ratio, "model": round(model, 4), "ratio_over_model": ratio / model}
            if m == n:
                bare = median_ms(pkg, lambda: points.call(m, jerk, exclude=False), repeats)
                row["call_us_without_self_index"] = round(bare * 1e3, 2)
                row["mask_form_cost"] = (t - bare) / bare
            yield row
    points.free()


def issue_only(pkg, calls, sequence_file):
    """every point `calls` times, nothing else: the run the profiler traces"""
    sequence = []
    for n in SOURCES:
        points = Points(pkg, n)
        for m in targets_of(n):
            for jerk in (False, True):
                plan = pkg.field_plan(n, m, np.float32)
                for _ in range(calls):
                    points.call(m, jerk)
                sequence.append({"num_sources": n, "num_targets": m, "jerk": jerk, "calls": calls, "launches": plan.launches})
        pkg.check(pkg.lib().nb_device_synchronize(), "nb_device_synchronize")
        points.free()
    with open(sequence_file, "w") as fh:
        json.dump(sequence, fh)


def summarise(directory, out):
    """lay the recorded sequence over the field_* dispatches of the kernel trace, in start order"""
    with open(os.path.join(directory, "sequence.json")) as fh:
        sequence = json.load(fh)
    traces = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    if not traces:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    with open(traces[-1], newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "field_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    at, lines = 0, []
    for point in sequence:
        times = {"field_eval": [], "field_finish": []}
        for _ in range(point["calls"]):
            for kernel in ("field_eval", "field_finish")[:point["launches"]]:
                row = rows[at]
                at += 1
                if kernel not in row["Kernel_Name"]:
                    raise SystemExit(f"dispatch {at} is {row['Kernel_Name']}, expected {kernel}: the trace does not follow the sequence")
                times[kernel].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        for kernel, t in times.items():
            if t:
                t.sort()
                lines.append((kernel, point["num_sources"], point["num_targets"], int(point["jerk"]), len(t), t[len(t) // 2], t[0], t[-1]))
    if at != len(rows):
        raise SystemExit(f"{len(rows) - at} field_* dispatches beyond the sequence")
    with open(out, "w", newline="") as fh:
        writer = csv.writer(fh, quoting=csv.QUOTE_NONNUMERIC)
        writer.writerow(("Name", "NumSources", "NumTargets", "Jerk", "Calls", "MedianNs", "MinNs", "MaxNs"))
        writer.writerows(lines)
    print(f"{len(lines)} lines -> {out}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--label", default="", help="copied into every line (e.g. the workgroup target of the library measured)")
    ap.add_argument("--out", help="also append the JSON lines to this file (with --summarise: the CSV to write)")
    ap.add_argument("--calls", type=int, default=0, help="issue every point this many times and nothing else (the profiler's run)")
    ap.add_argument("--sequence", help="with --calls: where to record the order of the points")
    ap.add_argument("--summarise", metavar="DIR", help="DIR holds sequence.json and the profiler's kernel trace: write the per-point kernel times to --out")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.out or os.path.join("profiles", "field_kernel_stats.csv"))
        return
    pkg = entry.load_package()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
    if args.calls:
        issue_only(pkg, args.calls, args.sequence or "sequence.json")
        return
    for n in SOURCES:
        for row in timed_points(pkg, n, args.repeats):
            row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **({"label": args.label} if args.label else {}), **row}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
