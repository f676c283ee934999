#!/usr/bin/env python3
"""Ensemble throughput (nb_ensemble_integrate_*, include/nbody_hip_ensemble.h) against the same work as B back-to-back single-system
nb_integrate_* calls on one stream.  One JSON line per point:

  fp32 FAST at (N, B) = (256, 1024), (1024, 256), (4096, 64), (16384, 16); fp64 FAST and fp32 STRICT at (1024, 256).

Times come from device events after a warm-up, over at least --seconds of timed steps.  Share of peak: 20 flop per interaction at
157.3 TFLOP/s (fp32) and 30 at 78.6 TFLOP/s (fp64), as DESIGN.md counts them.  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/ensemble_bench.py`.

  python tools/ensemble_bench.py [--seconds 0.25] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

POINTS = [(np.float32, 1, 256, 1024), (np.float32, 1, 1024, 256), (np.float32, 1, 4096, 64), (np.float32, 1, 16384, 16),
          (np.float64, 1, 1024, 256), (np.float32, 0, 1024, 256)]
PEAK = {np.float32: (20, 157.3e12), np.float64: (30, 78.6e12)}


def timed_ms(pkg, fn, seconds):
    """ms per call of fn(): warm-up, then repeated until `seconds` of device time have passed (events around the whole run)"""
    for _ in range(3):
        fn()
    pkg.check(pkg.lib().nb_device_synchronize())
    reps = 1
    while True:
        start, stop = pkg.Event(), pkg.Event()
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_ms(stop)
        if ms >= 1e3 * seconds:
            return ms / reps, reps
        reps = max(reps * 2, int(reps * 1.2e3 * seconds / max(ms, 1e-3)))


def point(pkg, oracle, dtype, mode, n, b, seconds):
    f32 = dtype == np.float32
    scalar = np.float32 if f32 else float
    oracle.srand(1)
    p, v = oracle.randomise(1, n, 1.54, 8.0, dtype)
    pos, vel = np.tile(p, b), np.tile(v, b)
    bufs = [pkg.DeviceBuffer(pos.nbytes) for _ in range(3)]
    bufs[0].upload(pos)
    bufs[2].upload(vel)
    s = dtype(np.float32(0.1))
    eps2 = s * s
    lib, ens = pkg.lib(), pkg.ensemble_lib()
    (lib.nb_set_softening_sq_f32 if f32 else lib.nb_set_softening_sq_f64)(scalar(eps2))
    integ = ens.nb_ensemble_integrate_f32 if f32 else ens.nb_ensemble_integrate_f64
    single = lib.nb_integrate_f32 if f32 else lib.nb_integrate_f64
    stride = 4 * n * np.dtype(dtype).itemsize
    dt, damp = scalar(dtype(np.float32(0.016))), scalar(dtype(1.0))
    new, old, v_ = (x.ptr.value for x in bufs)

    def ensemble():
        pkg.check(integ(new, old, v_, n, b, dt, damp, scalar(eps2), None, mode, None), "nb_ensemble_integrate")

    def singles():
        for k in range(b):
            pkg.check(single(new + k * stride, old + k * stride, v_ + k * stride, dt, damp, n, 256, mode, None), "nb_integrate")

    t_ens, reps_ens = timed_ms(pkg, ensemble, seconds)
    t_seq, reps_seq = timed_ms(pkg, singles, seconds)
    for x in bufs:
        x.free()
    inter = float(b) * n * n
    flop, peak = PEAK[dtype]
    plan = pkg.ensemble_plan(n, b, dtype)
    return {"precision": "fp32" if f32 else "fp64", "mode": "fast" if mode == 1 else "strict", "num_bodies": n, "num_systems": b,
            "plan": {"bodies_per_lane": plan.bodies_per_lane, "waves_per_group": plan.waves_per_group, "groups_per_system": plan.groups_per_system,
                     "grid_blocks": plan.grid_blocks},
            "ensemble_ms": round(t_ens, 5), "ensemble_steps_timed": reps_ens,
            "sequential_ms": round(t_seq, 5), "sequential_rounds_timed": reps_seq,
            "interactions_per_s": inter / (t_ens * 1e-3), "sequential_interactions_per_s": inter / (t_seq * 1e-3),
            "share_of_peak": round(inter / (t_ens * 1e-3) * flop / peak, 4), "sequential_share_of_peak": round(inter / (t_seq * 1e-3) * flop / peak, 4),
            "speedup": round(t_seq / t_ens, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=0.25, help="timed device time per measurement (default 0.25)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    args = ap.parse_args()
    pkg, O = entry.load_package(), entry.load_oracle()
    oracle = O.Oracle()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
    for dtype, mode, n, b in POINTS:
        row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **point(pkg, oracle, dtype, mode, n, b, args.seconds)}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
