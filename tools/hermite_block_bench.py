#!/usr/bin/env python3
"""Block steps of the Hermite scheme (nb_hermite_block_step_*, include/nbody_hip_hermite_block.h) by the number of active bodies, next to
the shared step (nb_hermite_step_*) timed in the same process -- and, next to each, the same point of the 6th-order block library
(nb_hermite6_block_step_*, include/nbody_hip_hermite6_block.h; "library": "hermite6_block" in its lines, its shared step nb_hermite6_step_*).
One JSON line per point:

  steps     fp32 at 65 536 and 262 144 bodies, n_act = 1, 128, 1 024, 8 192, N (hand-made levels: n_act bodies one level deeper than
            the rest, put back before every timed step): microseconds per block step (median of --repeats single steps, device events)
            and interactions per second (n_act * N per step).
  cluster   fp64, 16 384 bodies with four hard binaries (separation 0.001, mass 4/N each), eps^2 = 1e-8, to t = 1/8: wall clock and
            relative energy error (nb_energy_f64) of the block run (eta 0.02, 30 levels; 6th order: eta 0.2) and of shared-step runs of
            256 ... 4 096 steps.
  binary    fp64, the 256-body binary system of tests/test_hermite_block.py to t = 1: wall clock, block steps and energy error of both
            block libraries (4th order eta 0.02, 6th order eta 0.2).

The library measured is the one NBODY_HIP_HERMITE_BLOCK_LIB names (default: the package's), so builds with another workgroup target
(make -C cuda-nbody_amd/csrc EXP=-DNB_BLOCK_TARGET=1024 ...) are timed by the same script; `ranges` in each line says what J it chose.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/hermite_block_bench.py --only steps`.

  python tools/hermite_block_bench.py [--only steps|cluster|binary] [--repeats 9] [--label TEXT] [--out FILE]
(the lines of the 6th-order library are kept in profiles/hermite6_block_bench.jsonl)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402


def cloud(n, dtype, seed=1):
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3], pos[:, 3], vel[:, :3] = rng.standard_normal((n, 3)), 1.0 / n, rng.standard_normal((n, 3)) * 0.3
    return pos, vel


def median_ms(pkg, fn, prepare, repeats):
    for _ in range(2):
        prepare(), fn()
    times = []
    for _ in range(repeats):
        prepare()
        pkg.check(pkg.lib().nb_device_synchronize(), "nb_device_synchronize")
        start, stop = pkg.Event(), pkg.Event()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_ms(stop))
    return sorted(times)[len(times) // 2]


def libraries(pkg):
    """(name in the lines, block class, its eta, shared-step class, plan query) of the two block libraries"""
    return (("hermite_block", pkg.HermiteBlockSystem, 0.02, pkg.HermiteSystem, pkg.hermite_block_plan),
            ("hermite6_block", pkg.Hermite6BlockSystem, 0.2, pkg.Hermite6System, pkg.hermite6_block_plan))


def step_points(pkg, n, repeats, library):
    name, block_class, eta, shared_class, plan_of = library
    dtype = np.float32
    pos, vel = cloud(n, dtype)
    eps2, dt = dtype(0.01), 1e-3
    shared = shared_class(n, dtype, softening_sq=eps2)
    shared.set_state(pos, vel)
    shared.eval()
    t_shared = median_ms(pkg, lambda: shared.step(dtype(dt)), lambda: None, repeats)
    shared.free()
    for n_act in (1, 128, 1024, 8192, n):
        system = block_class(n, dtype, softening_sq=eps2, eta=eta, eta_start=0.01, dt_max=dt, max_level=8)
        system.set_state(pos, vel)
        system.init()
        levels = np.zeros(n, np.int32)
        levels[np.arange(n_act) * (n // n_act)] = 8 if n_act < n else 0
        ticks = np.zeros(n, np.uint64)

        def rewind():
            system._levels.upload(levels), system._ticks.upload(ticks)

        t = median_ms(pkg, system.step, rewind, repeats)
        assert system.status().last_active == n_act
        plan = plan_of(n, n_act, dtype)
        system.free()
        yield {"kind": "step", "library": name, "precision": "fp32", "num_bodies": n, "num_active": n_act, "tiles": plan.tiles, "ranges": plan.ranges, "groups": plan.groups,
               "launch_groups": plan.launch_groups, "launches": plan.launches, "block_step_us": round(t * 1e3, 2), "shared_step_us": round(t_shared * 1e3, 2),
               "interactions_per_s": float(n_act) * n / (t * 1e-3), "shared_interactions_per_s": float(n) * n / (t_shared * 1e-3)}


def cluster_points(pkg):
    n, dtype, eps2, t_end = 16384, np.float64, 1e-8, 0.125
    pos, vel = cloud(n, dtype, 7)
    sep, m = 0.001, 4.0 / n
    for b in range(4):  # bodies 2b, 2b+1: a circular binary about body 2b's place and velocity
        i, j = 2 * b, 2 * b + 1
        c, cv = pos[i, :3].copy(), vel[i, :3].copy()
        pos[i, 3] = pos[j, 3] = m
        pos[i, :3], pos[j, :3] = c + [sep / 2, 0, 0], c - [sep / 2, 0, 0]
        orbit = np.sqrt(m / (2 * sep))
        vel[i, :3], vel[j, :3] = cv + [0, orbit, 0], cv - [0, orbit, 0]
    pkg.set_softening_squared(float(eps2))
    e0 = None
    for line in block_runs(pkg, "cluster", pos, vel, eps2, t_end, t_end):
        e0 = line.pop("_e0")
        yield line
    for steps in (256, 1024, 4096):
        shared = pkg.HermiteSystem(n, dtype, softening_sq=eps2)
        shared.set_state(pos, vel)
        shared.synchronize()
        begin = time.perf_counter()
        shared.eval()
        for _ in range(steps):
            shared.step(t_end / steps)
        shared.synchronize()
        wall = time.perf_counter() - begin
        e1 = pkg.energy(shared._pos.ptr, shared._vel.ptr, n, dtype)["total"]
        shared.free()
        yield {"kind": "cluster", "run": f"shared {steps} steps", "num_bodies": n, "wall_s": round(wall, 4), "relative_energy_error": abs((e1 - e0) / e0), "evaluations_of_n2": steps}


def block_runs(pkg, kind, pos, vel, eps2, t_end, dt_max):
    """one line per block library: the run to t_end timed on the host (init and every block step), its counters and its energy error"""
    n, dtype = pos.shape[0], pos.dtype
    for name, block_class, eta, _, _ in libraries(pkg):
        block = block_class(n, dtype, softening_sq=eps2, eta=eta, eta_start=0.01, dt_max=dt_max, max_level=30)
        block.set_state(pos, vel)
        e0 = pkg.energy(block._pos.ptr, block._vel.ptr, n, dtype)["total"]
        block.synchronize()
        begin = time.perf_counter()
        block.init()
        status = block.advance(t_end, batch=64)
        block.synchronize()
        wall = time.perf_counter() - begin
        block.sync()
        p, v = block.snapshot_ptrs()
        e1 = pkg.energy(p, v, n, dtype)["total"]
        block.free()
        yield {"kind": kind, "library": name, "run": f"block eta {eta}", "num_bodies": n, "wall_s": round(wall, 4), "relative_energy_error": abs((e1 - e0) / e0),
               "block_steps": status.block_steps, "evaluations_of_n2": status.body_steps / n, "deepest_level": status.deepest_level, "_e0": e0}


def binary_points(pkg):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_hermite_block import BINARY_DT_MAX, BINARY_EPS2, binary_cloud  # noqa: E402, PLC0415

    pos, vel = binary_cloud()
    pkg.set_softening_squared(float(BINARY_EPS2))
    for line in block_runs(pkg, "binary", pos, vel, BINARY_EPS2, 1.0, BINARY_DT_MAX):
        del line["_e0"]
        yield line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=("steps", "cluster", "binary"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--label", default="", help="copied into every line (e.g. the workgroup target of the library measured)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")

    def rows():
        if args.only in (None, "steps"):
            for n in (65536, 262144):
                for library in libraries(pkg):
                    yield from step_points(pkg, n, args.repeats, library)
        if args.only in (None, "cluster"):
            yield from cluster_points(pkg)
        if args.only in (None, "binary"):
            yield from binary_points(pkg)

    for row in rows():
        row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **({"label": args.label} if args.label else {}), **row}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
