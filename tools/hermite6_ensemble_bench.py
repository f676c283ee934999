#!/usr/bin/env python3
"""6th-order Hermite ensemble throughput (nb_hermite6_ensemble_*, include/nbody_hip_hermite6_ensemble.h).  One JSON line per point:

  fixed step   one nb_hermite6_ensemble_step_* of B systems of N bodies against B back-to-back nb_hermite6_step_* calls on one stream and
               against one nb_hermite_ensemble_step_* (the 4th-order step of the same systems; the issue-cost model of DESIGN.md 5.13 puts
               a 6th-order step at 1.76 of it): fp32 at (N, B) = (256, 1024), (1024, 256), (4096, 64), (16384, 16); fp64 at (1024, 256).
  adaptive     B = 64 clouds of 1 024 bodies with one hard binary each (bodies 0 and 1, DESIGN.md 5.7's) to t = 1/8, fp64: wall clock and
               steps of begin + batches of nb_hermite6_ensemble_advance_* at eta 0.025 with a 64-byte status read per batch, against the
               4th-order ensemble's run of the same systems at eta 0.02, with the relative energy error (numpy fp64) of both.
  eta          (--eta-table, CPU only, no library) the table behind the default eta: an fp64 numpy restatement of both schemes on DESIGN.md
               5.7's 256-body cloud with one hard binary, softening^2 1e-8, to t = 1/8, with a shared adaptive step.

Times of the fixed steps come from device events after a warm-up, over at least --seconds of timed steps.

  python tools/hermite6_ensemble_bench.py [--seconds 0.25] [--out FILE] [--skip-adaptive] [--eta-table [--seeds 1992,1993]]"""
import argparse
import json
import os
import sys
import time

import numpy as np

POINTS = [(np.float32, 256, 1024), (np.float32, 1024, 256), (np.float32, 4096, 64), (np.float32, 16384, 16), (np.float64, 1024, 256)]
ISSUE_MODEL = (47 * 4.08 + 2 * 8.3) / (25 * 4.08 + 2 * 8.3)
ETA4, ETA6 = 0.02, 0.025
ETAS = (0.8, 0.4, 0.2, 0.1, 0.05, 0.025, 0.0125)


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
    system = pkg.Hermite6Ensemble(n, b, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    system.eval()
    fourth = pkg.HermiteEnsemble(n, b, dtype, softening_sq=eps2)
    fourth.set_state(pos, vel)
    fourth.eval()
    solo_step = getattr(pkg.hermite6_lib(), "nb_hermite6_step_" + sfx)
    stride = 4 * n * np.dtype(dtype).itemsize
    p, v, a, j, s, c, ws = (x.ptr.value for x in (system._pos, system._vel, system._acc, system._jerk, system._snap, system._crackle, system._workspace))

    def ensemble():
        system.step(dt)

    def solos():
        for k in range(b):
            at = k * stride
            pkg.check(solo_step(p + at, p + at, v + at, a + at, j + at, s + at, c + at, ws + 3 * at, 3 * stride, n, scalar(dt), scalar(eps2), None), "nb_hermite6_step")

    def fourth_order():
        fourth.step(dt)

    t_ens, reps_ens = timed_ms(pkg, ensemble, seconds)
    t_solo, reps_solo = timed_ms(pkg, solos, seconds)
    t_fourth, _ = timed_ms(pkg, fourth_order, seconds)
    pkg.check(pkg.lib().nb_device_synchronize())
    system.free(), fourth.free()
    inter = float(b) * n * n
    plan = pkg.hermite6_ensemble_plan(n, b, dtype)
    return {"kind": "fixed", "precision": "fp32" if f32 else "fp64", "num_bodies": n, "num_systems": b,
            "plan": {"bodies_per_lane": plan.bodies_per_lane, "waves_per_group": plan.waves_per_group, "groups_per_system": plan.groups_per_system, "grid_blocks": plan.grid_blocks},
            "ensemble_step_ms": round(t_ens, 5), "ensemble_steps_timed": reps_ens, "solo_steps_ms": round(t_solo, 5), "solo_rounds_timed": reps_solo,
            "interactions_per_s": inter / (t_ens * 1e-3), "solo_interactions_per_s": inter / (t_solo * 1e-3), "speedup_over_solo": round(t_solo / t_ens, 2),
            "fourth_order_ensemble_ms": round(t_fourth, 5), "ratio_to_fourth_order": round(t_ens / t_fourth, 3), "issue_model": round(ISSUE_MODEL, 3)}


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


def energy(x, v, m, eps2):
    d = x[None] - x[:, None]
    s = np.sqrt((d * d).sum(axis=2) + eps2)
    return 0.5 * (m * (v * v).sum(axis=1)).sum() - (m[:, None] * m[None] / s)[np.triu_indices(len(m), 1)].sum()


def adaptive_point(pkg, dtype=np.float64, n=1024, b=64, t_end=0.125, batch=64):
    clouds = [binary_cloud(n, 200 + s) for s in range(b)]
    pos, vel = np.stack([c[0] for c in clouds]).astype(dtype), np.stack([c[1] for c in clouds]).astype(dtype)
    eps2 = dtype(1e-6)
    sync = lambda: pkg.check(pkg.lib().nb_device_synchronize())  # noqa: E731
    start_energy = np.array([energy(pos[s, :, :3], vel[s, :, :3], pos[s, :, 3], float(eps2)) for s in range(b)])
    row = {"kind": "adaptive", "precision": "fp32" if dtype == np.float32 else "fp64", "num_bodies": n, "num_systems": b, "t_end": t_end, "batch": batch}
    for name, cls, eta in (("hermite6", pkg.Hermite6Ensemble, ETA6), ("hermite", pkg.HermiteEnsemble, ETA4)):
        system = cls(n, b, dtype, softening_sq=eps2)
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
        wall = time.perf_counter() - start
        steps = system.clocks()["steps"].astype(int)
        p, v = system.get_positions(), system.get_velocities()
        system.free()
        end_energy = np.array([energy(p[s, :, :3], v[s, :, :3], p[s, :, 3], float(eps2)) for s in range(b)])
        error = np.abs((end_energy - start_energy) / start_energy)
        row[name] = {"eta": eta, "wall_s": round(wall, 4), "calls": calls, "steps_fewest": int(steps.min()), "steps_median": int(np.median(steps)), "steps_most": int(steps.max()),
                     "steps_total": int(steps.sum()), "done": status.done, "stalled": status.stalled, "energy_error_median": float(np.median(error)), "energy_error_worst": float(error.max())}
    row["wall_ratio_fourth_over_sixth"] = round(row["hermite"]["wall_s"] / row["hermite6"]["wall_s"], 2)
    return row


# ---------------------------------------------------------------------------------------------------------------- the eta table (numpy, fp64)
def evaluate(x, v, b, m, eps2):
    """a, jerk [, snap if b is given] of every body: the formulas of include/nbody_hip_hermite6.h"""
    r, w = x[None] - x[:, None], v[None] - v[:, None]
    s2 = (r * r).sum(axis=2) + eps2
    k = m[None] * s2 ** -1.5
    np.fill_diagonal(k, 0.0)
    alpha = (r * w).sum(axis=2) / s2
    jp = w - 3 * alpha[..., None] * r
    a, j = (k[..., None] * r).sum(axis=1), (k[..., None] * jp).sum(axis=1)
    if b is None:
        return a, j
    d = b[None] - b[:, None]
    beta = ((w * w).sum(axis=2) + (r * d).sum(axis=2)) / s2 + alpha ** 2
    return a, j, (k[..., None] * (d - 6 * alpha[..., None] * jp - 3 * beta[..., None] * r)).sum(axis=1)


def norm(q):
    return np.sqrt((q * q).sum(axis=1))


def numpy_run4(pos, vel, eps2, t_end, eta):
    """the 4th-order scheme of include/nbody_hip_hermite.h with dt = eta min |a| / |jerk|: (relative energy error, steps)"""
    x, v, m = pos[:, :3].copy(), vel[:, :3].copy(), pos[:, 3].copy()
    e0 = energy(x, v, m, eps2)
    a, j = evaluate(x, v, None, m, eps2)
    t, steps = 0.0, 0
    while t < t_end:
        dt = min(eta * (norm(a) / norm(j)).min(), t_end - t)
        xp, vp = x + dt * (v + dt / 2 * (a + dt / 3 * j)), v + dt * (a + dt / 2 * j)
        a1, j1 = evaluate(xp, vp, None, m, eps2)
        v1 = v + dt / 2 * (a + a1) + dt * dt / 12 * (j - j1)
        x = x + dt / 2 * (v + v1) + dt * dt / 12 * (a - a1)
        v, a, j, t, steps = v1, a1, j1, t + dt, steps + 1
    return abs((energy(x, v, m, eps2) - e0) / e0), steps


def numpy_run6(pos, vel, eps2, t_end, eta):
    """the 6th-order scheme of include/nbody_hip_hermite6.h with dt = eta sqrt(min (|a||s| + |j|^2) / (|j||c| + |s|^2))"""
    x, v, m = pos[:, :3].copy(), vel[:, :3].copy(), pos[:, 3].copy()
    e0 = energy(x, v, m, eps2)
    a, j = evaluate(x, v, None, m, eps2)
    a, j, s = evaluate(x, v, a, m, eps2)
    c = np.zeros_like(a)
    t, steps = 0.0, 0
    while t < t_end:
        na, nj, ns, nc = norm(a), norm(j), norm(s), norm(c)
        h = min(eta * np.sqrt(((na * ns + nj * nj) / (nj * nc + ns * ns)).min()), t_end - t)
        xp = x + h * (v + h / 2 * (a + h / 3 * (j + h / 4 * (s + h / 5 * c))))
        vp = v + h * (a + h / 2 * (j + h / 3 * (s + h / 4 * c)))
        ap = a + h * (j + h / 2 * (s + h / 3 * c))
        a1, j1, s1 = evaluate(xp, vp, ap, m, eps2)
        v1 = v + h / 2 * (a + a1) - h * h / 10 * (j1 - j) + h ** 3 / 120 * (s + s1)
        x = x + h / 2 * (v + v1) - h * h / 10 * (a1 - a) + h ** 3 / 120 * (j + j1)
        c = (60 * (a1 - a - j * h - s * h * h / 2) - 36 * (j1 - j - s * h) * h + 9 * (s1 - s) * h * h) / h ** 3
        v, a, j, s, t, steps = v1, a1, j1, s1, t + h, steps + 1
    return abs((energy(x, v, m, eps2) - e0) / e0), steps


def eta_table(seeds, etas=ETAS, n=256, eps2=1e-8, t_end=0.125):
    for seed in seeds:
        pos, vel = binary_cloud(n, seed)
        error4, steps4 = numpy_run4(pos, vel, eps2, t_end, ETA4)
        yield {"kind": "eta", "seed": seed, "order": 4, "eta": ETA4, "energy_error": error4, "steps": steps4}
        for eta in etas:
            error6, steps6 = numpy_run6(pos, vel, eps2, t_end, eta)
            yield {"kind": "eta", "seed": seed, "order": 6, "eta": eta, "energy_error": error6, "steps": steps6, "half_the_error_in_fewer_steps": bool(error6 <= error4 / 2 and steps6 < steps4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=0.25, help="timed device time per measurement (default 0.25)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    ap.add_argument("--skip-adaptive", action="store_true", help="only the fixed-step points")
    ap.add_argument("--eta-table", action="store_true", help="only the numpy table behind the default eta (no GPU, no library)")
    ap.add_argument("--seeds", default="1992", help="--eta-table: the seeds of the cloud, comma-separated (default 1992, DESIGN.md 5.7's)")
    args = ap.parse_args()
    if args.eta_table:
        rows = eta_table([int(s) for s in args.seeds.split(",")])
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import __graft_entry__ as entry
        pkg = entry.load_package()
        pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
        makers = [lambda d=dtype, n=n, b=b: fixed_point(pkg, d, n, b, args.seconds) for dtype, n, b in POINTS]
        if not args.skip_adaptive:
            makers.append(lambda: adaptive_point(pkg))
        rows = (make() for make in makers)
    for made in rows:
        line = json.dumps({"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **made})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
