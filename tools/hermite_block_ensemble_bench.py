#!/usr/bin/env python3
"""Block time steps of many systems in one call (nb_hermite_block_ensemble_*, include/nbody_hip_hermite_block_ensemble.h) against the solo
library (nb_hermite_block_*) in the same process.  One JSON line per point:

  call   one nb_hermite_block_ensemble_step_* of B systems of N bodies with n_act bodies due in each, against the B nb_hermite_block_step_*
         calls it replaces, back to back on one stream ON THE SAME ARRAYS (system s of the ensemble's arrays, one solo workspace): fp32,
         (N, B, n_act) in {256, 1 024, 16 384} x {1, 16, 64, 256} x {1, 128, N}.  The schedule (levels and ticks) is put back before every
         timed call, outside the timed region; device events; the median of --samples calls after a warm-up.  The row also holds the solo
         geometry (tiles, J), the workgroups launched and working, and the bytes of partial planes written and read per call.
  run    B = 64 clouds of 256 bodies with one hard binary each (DESIGN.md 5.7's cloud, other seeds) to t = 1, fp64, eta 0.02: the wall clock
         of HermiteBlockEnsemble.advance (batches of 64 calls and one summary, 64 bytes read per batch) against the 64
         HermiteBlockSystem.advance runs one after the other, and the relative energy errors of both through nb_energy_f64 on the synced
         snapshots -- which the bit-identity makes equal.

  python tools/hermite_block_ensemble_bench.py [--order {4,6}] [--samples 9] [--out FILE] [--skip-run] [--only-run] [--point N,B,N_ACT]

--point restricts the single-call points to one (what a `rocprofv3 --kernel-trace --stats` run of its own traces).

--order 6 measures the 6th-order library (nb_hermite6_block_ensemble_*, include/nbody_hip_hermite6_block_ensemble.h) at the same points
against nb_hermite6_block_step_*, and the whole run (eta 0.2) against the 64 Hermite6BlockSystem.advance runs; every `call` row then also
holds the 4th-order ensemble call at the same point (fourth_ensemble_call_us, ratio_over_fourth), and the `run` row the 4th-order block
ensemble's run at eta 0.02 (fourth_*).  Its results go to profiles/hermite6_block_ensemble_bench.jsonl (--out)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

SIZES, SYSTEMS = (256, 1024, 16384), (1, 16, 64, 256)
MAX_LEVEL, DT_MAX = 8, 1.0 / 64


def cloud(n, dtype, seed):
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3], vel[:, :3], pos[:, 3] = rng.standard_normal((n, 3)), rng.standard_normal((n, 3)) * 0.3, 1.0 / n
    return pos, vel


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


def median_ms(pkg, fn, prepare, samples):
    for _ in range(2):
        prepare(), fn()
    times = []
    for _ in range(samples):
        prepare()
        pkg.check(pkg.lib().nb_device_synchronize())
        start, stop = pkg.Event(), pkg.Event()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_ms(stop))
    return float(np.median(times)), float(min(times))


def libraries(pkg, order):
    """(ensemble class, solo class, solo library, its prefix, ensemble plan, solo workspace query, state arrays, eta) of an order"""
    if order == 6:
        return (pkg.Hermite6BlockEnsemble, pkg.Hermite6BlockSystem, pkg.hermite6_block_lib, "nb_hermite6_block_", pkg.hermite6_block_ensemble_plan,
                pkg.hermite6_block_workspace_bytes, ("pos", "vel", "acc", "jerk", "snap", "crackle"), 0.2)
    return (pkg.HermiteBlockEnsemble, pkg.HermiteBlockSystem, pkg.hermite_block_lib, "nb_hermite_block_", pkg.hermite_block_ensemble_plan, pkg.hermite_block_workspace_bytes,
            ("pos", "vel", "acc", "jerk"), 0.02)


def call_point(pkg, n, b, n_act, samples, order=4, dtype=np.float32):
    """n_act bodies of every system at the deepest level, due at tick 1; the others at level 0 (all of them due when n_act = N: level 0, tick 0)"""
    size = np.dtype(dtype).itemsize
    scalar = np.float32 if dtype == np.float32 else float
    sfx = "f32" if dtype == np.float32 else "f64"
    ensemble_class, _, solo_lib, prefix, ensemble_plan, solo_workspace_bytes, arrays, eta = libraries(pkg, order)
    params = pkg.HermiteBlockParams(eta, 0.01, DT_MAX, MAX_LEVEL, 0)
    one = cloud(n, dtype, 300)
    pos, vel = np.stack([one[0]] * b), np.stack([one[1]] * b)
    eps2 = dtype(0.01)
    ensemble = ensemble_class(n, b, dtype, params, eps2)
    ensemble.set_state(pos, vel)
    ensemble.init()
    levels = np.zeros((b, n), np.int32)
    if n_act < n:
        levels[:, ::n // n_act][:, :n_act] = MAX_LEVEL
    ticks = np.zeros((b, n), np.uint64)

    def rewind():
        ensemble._levels.upload(levels), ensemble._ticks.upload(ticks)

    solo_step = getattr(solo_lib(), prefix + "step_" + sfx)
    solo_ws_bytes = solo_workspace_bytes(n, dtype)
    solo_ws = pkg.DeviceBuffer(solo_ws_bytes)
    base = {name: getattr(ensemble, "_" + name).ptr.value for name in (*arrays, "ticks", "levels", "status")}
    per_body = dict(**{name: 4 * size for name in arrays}, ticks=8, levels=4)

    def solos():
        for s in range(b):
            at = [base[name] + s * n * per_body[name] for name in (*arrays, "ticks", "levels")]
            pkg.check(solo_step(*at, base["status"] + 64 * s, solo_ws.ptr, solo_ws_bytes, n, scalar(eps2), ctypes.byref(params), float("inf"), None), prefix + "step")

    t_ens, t_ens_min = median_ms(pkg, ensemble.step, rewind, samples)
    active = sorted({s.last_active for s in ensemble.statuses()})
    t_solo, t_solo_min = median_ms(pkg, solos, rewind, samples)
    active_solo = sorted({s.last_active for s in ensemble.statuses()})
    assert active == active_solo == [n_act], (active, active_solo, n_act)
    plan = ensemble_plan(n, b, n_act, dtype)
    solo_ws.free(), ensemble.free()
    fourth = {}
    if order == 6:  # the 4th-order ensemble call at the same point, in the same process
        other = pkg.HermiteBlockEnsemble(n, b, dtype, pkg.HermiteBlockParams(0.02, 0.01, DT_MAX, MAX_LEVEL, 0), eps2)
        other.set_state(pos, vel)
        other.init()
        t_fourth, _ = median_ms(pkg, other.step, lambda: (other._levels.upload(levels), other._ticks.upload(ticks)), samples)
        other.free()
        fourth = {"fourth_ensemble_call_us": round(t_fourth * 1e3, 2), "ratio_over_fourth": round(t_ens / t_fourth, 2)}
    return {"kind": "call", "order": order, **fourth, "precision": "fp32" if dtype == np.float32 else "fp64", "num_bodies": n, "num_systems": b, "num_active": n_act, "samples": samples,
            "ensemble_call_us": round(t_ens * 1e3, 2), "ensemble_call_min_us": round(t_ens_min * 1e3, 2), "solo_calls_us": round(t_solo * 1e3, 2), "solo_calls_min_us": round(t_solo_min * 1e3, 2),
            "speedup_over_solo": round(t_solo / t_ens, 2), "interactions_per_s": float(b) * n_act * n / (t_ens * 1e-3),
            "plan": {"waves_per_group": plan.waves_per_group, "tiles": plan.tiles, "ranges": plan.ranges, "groups_working_per_system": plan.groups,
                     "groups_launched_per_system": plan.groups_per_system, "eval_grid": plan.eval_grid, "step_launches": plan.step_launches, "solo_launches": 6 * b,
                     "partial_bytes_per_call": 2 * plan.partial_bytes * b}}


def run_point(pkg, order=4, n=256, b=64, t_end=1.0, batch=64):
    dtype, eps2 = np.float64, 1e-8
    ensemble_class, solo_class, _, _, _, _, _, eta = libraries(pkg, order)
    clouds = [binary_cloud(n, 1992 + s) for s in range(b)]
    pos, vel = np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds])
    params = pkg.HermiteBlockParams(eta, 0.01, 0.125, 30, 0)
    sync = lambda: pkg.check(pkg.lib().nb_device_synchronize())  # noqa: E731
    pkg.set_softening_squared(eps2)
    stride = 4 * n * 8

    def energies(p, v):
        return np.array([pkg.energy(p.value + s * stride, v.value + s * stride, n, dtype)["total"] for s in range(b)])

    ensemble = ensemble_class(n, b, dtype, params, eps2)
    ensemble.set_state(pos, vel)
    start_energy = energies(ensemble._pos.ptr, ensemble._vel.ptr)
    sync()
    start = time.perf_counter()
    ensemble.init()
    summary = ensemble.advance(t_end, batch)
    sync()
    t_ensemble = time.perf_counter() - start
    ensemble.sync()
    end_energy = energies(*ensemble.snapshot_ptrs())
    steps = np.array([s.block_steps for s in ensemble.statuses()])
    snapshot = ensemble.snapshot()
    ensemble.free()

    fourth = {}
    if order == 6:  # the 4th-order block ensemble on the same clouds, at the eta that matches (include/nbody_hip_hermite6_block.h)
        other = pkg.HermiteBlockEnsemble(n, b, dtype, pkg.HermiteBlockParams(0.02, 0.01, 0.125, 30, 0), eps2)
        other.set_state(pos, vel)
        sync()
        start = time.perf_counter()
        other.init()
        other_summary = other.advance(t_end, batch)
        sync()
        t_other = time.perf_counter() - start
        other.sync()
        other_err = np.abs((energies(*other.snapshot_ptrs()) - start_energy) / start_energy)
        other.free()
        fourth = {"fourth_eta": 0.02, "fourth_ensemble_wall_s": round(t_other, 4), "fourth_block_steps_total": int(other_summary.block_steps),
                  "fourth_body_steps_total": int(other_summary.body_steps), "fourth_energy_error_median": float(np.median(other_err)), "fourth_energy_error_max": float(other_err.max())}

    solo = solo_class(n, dtype, softening_sq=eps2, eta=eta, eta_start=0.01, dt_max=0.125, max_level=30)
    solo_steps, solo_energy, same = [], [], True
    t_solo = 0.0
    for s in range(b):
        solo.set_state(pos[s], vel[s])
        sync()
        start = time.perf_counter()
        solo.init()
        status = solo.advance(t_end, batch)
        sync()
        t_solo += time.perf_counter() - start
        solo_steps.append(status.block_steps)
        p, v = solo.snapshot()
        same = same and p.tobytes() == snapshot[0][s].tobytes() and v.tobytes() == snapshot[1][s].tobytes()
        solo_energy.append(pkg.energy(*solo.snapshot_ptrs(), n, dtype)["total"])
    solo.free()
    err = np.abs((end_energy - start_energy) / start_energy)
    solo_err = np.abs((np.array(solo_energy) - start_energy) / start_energy)
    return {"kind": "run", "order": order, **fourth, "precision": "fp64", "num_bodies": n, "num_systems": b, "t_end": t_end, "eta": eta, "batch": batch,
            "ensemble_wall_s": round(t_ensemble, 4), "solo_wall_s": round(t_solo, 4), "speedup_over_solo": round(t_solo / t_ensemble, 2),
            "block_steps_fewest": int(steps.min()), "block_steps_median": int(np.median(steps)), "block_steps_most": int(steps.max()), "block_steps_total": int(summary.block_steps),
            "solo_block_steps_total": int(sum(solo_steps)), "body_steps_total": int(summary.body_steps), "deepest_level": int(summary.deepest_level),
            "energy_error_median": float(np.median(err)), "energy_error_max": float(err.max()), "solo_energy_error_max": float(solo_err.max()),
            "energy_errors_equal_solo": bool((err == solo_err).all()), "snapshots_equal_solo": bool(same)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--order", type=int, choices=(4, 6), default=4, help="4: nb_hermite_block_ensemble_* (default); 6: nb_hermite6_block_ensemble_*")
    ap.add_argument("--samples", type=int, default=9, help="timed calls per measurement (default 9)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    ap.add_argument("--skip-run", action="store_true", help="only the single-call points")
    ap.add_argument("--only-run", action="store_true", help="only the whole run")
    ap.add_argument("--point", help="N,B,N_ACT: only this single-call point")
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
    rows = []
    if not args.only_run:
        points = [tuple(int(v) for v in args.point.split(","))] if args.point else [(n, b, a) for n in SIZES for b in SYSTEMS for a in (1, 128, n)]
        rows += [lambda n=n, b=b, a=a: call_point(pkg, n, b, a, args.samples, args.order) for n, b, a in points]
    if not args.skip_run:
        rows.append(lambda: run_point(pkg, args.order))
    for make in rows:
        row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **make()}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
