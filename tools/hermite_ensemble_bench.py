#!/usr/bin/env python3
"""Hermite ensemble throughput (nb_hermite_ensemble_*, include/nbody_hip_hermite_ensemble.h).  One JSON line per point:

  fixed step   one nb_hermite_ensemble_step_* of B systems of N bodies against B back-to-back nb_hermite_step_* calls on one stream and
               against one nb_ensemble_integrate_* FAST step of the same systems (the first-order step; the issue-cost model of DESIGN.md
               5.6 puts a Hermite step at 1.93 of it): fp32 at (N, B) = (256, 1024), (1024, 256), (4096, 64), (16384, 16); fp64 at (1024, 256).
  adaptive     B = 64 clouds of 1 024 bodies with one hard binary each (bodies 0 and 1, DESIGN.md 5.7's) to t = 1/8, eta 0.02: wall clock
               of begin + batches of nb_hermite_ensemble_advance_* with a 64-byte status read per batch, against the same 64 runs driven
               one after another through nb_hermite_step_* / nb_hermite_timestep_* with a host read of dt per step.

Times of the fixed steps come from device events after a warm-up, over at least --seconds of timed steps.

  python tools/hermite_ensemble_bench.py [--seconds 0.25] [--out FILE] [--skip-adaptive]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

POINTS = [(np.float32, 256, 1024), (np.float32, 1024, 256), (np.float32, 4096, 64), (np.float32, 16384, 16), (np.float64, 1024, 256)]
ISSUE_MODEL = (25 * 4.08 + 2 * 8.3) / (11 * 4.08 + 2 * 8.3)


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


def cloud(n, dtype, seed):
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3], vel[:, :3], pos[:, 3] = rng.standard_normal((n, 3)), rng.standard_normal((n, 3)) * 0.3, 1.0 / n
    return pos, vel


def fixed_point(pkg, dtype, n, b, seconds):
    f32 = dtype == np.float32
    scalar, sfx = (np.float32, "f32") if f32 else (float, "f64")
    clouds = [cloud(n, dtype, 100 + s) for s in range(b)]
    pos, vel = np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds])
    eps2, dt = dtype(0.01), dtype(1e-3)
    system = pkg.HermiteEnsemble(n, b, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    system.eval()
    lib, solo, first = pkg.lib(), pkg.hermite_lib(), pkg.ensemble_lib()
    solo_step = getattr(solo, "nb_hermite_step_" + sfx)
    euler = getattr(first, "nb_ensemble_integrate_" + sfx)
    stride = 4 * n * np.dtype(dtype).itemsize
    p, v, a, j, ws = (x.ptr.value for x in (system._pos, system._vel, system._acc, system._jerk, system._workspace))
    other = pkg.DeviceBuffer(pos.nbytes)

    def ensemble():
        system.step(dt)

    def solos():
        for k in range(b):
            pkg.check(solo_step(p + k * stride, p + k * stride, v + k * stride, a + k * stride, j + k * stride, ws + 2 * k * stride, 2 * stride, n, scalar(dt), scalar(eps2), None),
                      "nb_hermite_step")

    def first_order():
        pkg.check(euler(other.ptr, p, v, n, b, scalar(dt), scalar(1.0), scalar(eps2), None, pkg.NB_MODE_FAST, None), "nb_ensemble_integrate")

    t_ens, reps_ens = timed_ms(pkg, ensemble, seconds)
    t_solo, reps_solo = timed_ms(pkg, solos, seconds)
    t_euler, _ = timed_ms(pkg, first_order, seconds)
    pkg.check(lib.nb_device_synchronize())
    other.free(), system.free()
    inter = float(b) * n * n
    plan = pkg.hermite_ensemble_plan(n, b, dtype)
    return {"kind": "fixed", "precision": "fp32" if f32 else "fp64", "num_bodies": n, "num_systems": b,
            "plan": {"bodies_per_lane": plan.bodies_per_lane, "waves_per_group": plan.waves_per_group, "groups_per_system": plan.groups_per_system, "grid_blocks": plan.grid_blocks},
            "ensemble_step_ms": round(t_ens, 5), "ensemble_steps_timed": reps_ens, "solo_steps_ms": round(t_solo, 5), "solo_rounds_timed": reps_solo,
            "interactions_per_s": inter / (t_ens * 1e-3), "solo_interactions_per_s": inter / (t_solo * 1e-3), "speedup_over_solo": round(t_solo / t_ens, 2),
            "first_order_ensemble_ms": round(t_euler, 5), "ratio_to_first_order": round(t_ens / t_euler, 3), "issue_model": round(ISSUE_MODEL, 3)}


def binary_cloud(n, seed):
    """a cloud with bodies 0 and 1 made a circular binary of separation 0.01 and four times the mass each"""
    pos, vel = cloud(n, np.float64, seed)
    sep, m = 0.01, 4 * pos[0, 3]
    pos[0, 3] = pos[1, 3] = m
    c, cv = pos[0, :3].copy(), vel[0, :3].copy()
    pos[0, :3], pos[1, :3] = c + [sep / 2, 0, 0], c - [sep / 2, 0, 0]
    orbit = np.sqrt(m / (2 * sep))
    vel[0, :3], vel[1, :3] = cv + [0, orbit, 0], cv - [0, orbit, 0]
    return pos, vel


def adaptive_point(pkg, dtype=np.float64, n=1024, b=64, t_end=0.125, eta=0.02, batch=64):
    clouds = [binary_cloud(n, 200 + s) for s in range(b)]
    pos, vel = np.stack([c[0] for c in clouds]).astype(dtype), np.stack([c[1] for c in clouds]).astype(dtype)
    eps2 = dtype(1e-6)
    sync = lambda: pkg.check(pkg.lib().nb_device_synchronize())  # noqa: E731
    system = pkg.HermiteEnsemble(n, b, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    sync()
    start = time.perf_counter()
    system.begin(eta)
    calls = 0
    while True:
        system.advance(t_end, eta, calls=batch)
        calls += batch
        status = system.status()
        if status.done + status.stalled == status.systems:
            break
    t_ensemble = time.perf_counter() - start
    steps = system.clocks()["steps"].astype(int)
    system.free()
    solo = pkg.HermiteSystem(n, dtype, softening_sq=eps2)
    solo_steps = []
    sync()
    start = time.perf_counter()
    for s in range(b):
        solo.set_state(pos[s], vel[s])
        solo.eval()
        t, count = 0.0, 0
        while t < t_end:
            dt = min(float(solo.suggested_dt(eta)), t_end - t)  # (a host read per step)
            solo.step(dt)
            t, count = t + dt, count + 1
        solo_steps.append(count)
    sync()
    t_solo = time.perf_counter() - start
    solo.free()
    return {"kind": "adaptive", "precision": "fp32" if dtype == np.float32 else "fp64", "num_bodies": n, "num_systems": b, "t_end": t_end, "eta": eta, "batch": batch,
            "ensemble_wall_s": round(t_ensemble, 4), "ensemble_calls": calls, "steps_fewest": int(steps.min()), "steps_median": int(np.median(steps)), "steps_most": int(steps.max()),
            "steps_total": int(steps.sum()), "done": status.done, "stalled": status.stalled,
            "solo_wall_s": round(t_solo, 4), "solo_steps_total": int(sum(solo_steps)), "speedup_over_solo": round(t_solo / t_ensemble, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=0.25, help="timed device time per measurement (default 0.25)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    ap.add_argument("--skip-adaptive", action="store_true", help="only the fixed-step points")
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
    rows = [lambda d=dtype, n=n, b=b: fixed_point(pkg, d, n, b, args.seconds) for dtype, n, b in POINTS]
    if not args.skip_adaptive:
        rows.append(lambda: adaptive_point(pkg))
    for make in rows:
        row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **make()}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
