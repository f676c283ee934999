#!/usr/bin/env python3
"""The neighbour survey and the neighbour lists (nb_neighbour_survey_f32 / nb_neighbour_lists_f32, include/nbody_hip_neighbour.h)
next to the one-sided FAST step of the product (nb_integrate_f32 without a workspace) timed in the same process.  One JSON line per
point: fp32 at 16 384, 65 536 and 262 144 bodies; the survey without and with potentials; the lists at a mean of about 20 entries
(radius_sq = (0.35 (5000 / N)^(1/3))^2 on a standard normal cloud).

Times come from device events after a warm-up, over at least --seconds of timed calls.  `model` is the issue-cost ratio of the fp32
loops as compiled (survey: 6 packed + 7 other vector operations per packed pair of bodies i and body j, with potentials 8 + 7 and
2 v_rsq_f32, against 11 packed + 2 v_rsq_f32; a packed op every 4.08 and a v_rsq_f32 every 8.3 SIMD cycles, and -- an assumption, not
a measurement -- every other vector operation another 4.08: DESIGN.md 5.8).  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/neighbour_bench.py`.

  python tools/neighbour_bench.py [--seconds 0.25] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from tools.ensemble_bench import timed_ms  # noqa: E402

POINTS = [16384, 65536, 262144]
ONE_SIDED = 11 * 4.08 + 2 * 8.3
MODEL_PLAIN = (6 + 7) * 4.08 / ONE_SIDED
MODEL_POT = ((8 + 7) * 4.08 + 2 * 8.3) / ONE_SIDED


def point(pkg, n, seconds):
    dtype = np.float32
    rng = np.random.default_rng(7)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3], pos[:, 3] = rng.standard_normal((n, 3)), 1.0 / n
    eps2, dt = dtype(0.01), dtype(1e-4)
    r2 = dtype((0.35 * (5000 / n) ** (1 / 3)) ** 2)
    lib = pkg.lib()
    lib.nb_set_softening_sq_f32(np.float32(eps2))
    here, other, velocities = pkg.DeviceBuffer(pos.nbytes), pkg.DeviceBuffer(pos.nbytes), pkg.DeviceBuffer(pos.nbytes)
    here.upload(pos), velocities.upload(vel)
    state = {"read": here.ptr.value, "write": other.ptr.value}

    def euler():
        pkg.check(lib.nb_integrate_f32(state["write"], state["read"], velocities.ptr, np.float32(dt), np.float32(1.0), n, 256, pkg.NB_MODE_FAST, None), "nb_integrate")
        state["read"], state["write"] = state["write"], state["read"]

    survey = pkg.NeighbourSurvey(n, dtype, softening_sq=eps2)
    survey._pos.upload(pos)
    total = survey.lists(survey._pos, radius_sq=r2)["status"]["total_neighbours"]
    t_plain, reps = timed_ms(pkg, lambda: survey.enqueue_survey(survey._pos, radius_sq=r2), seconds)
    t_pot, _ = timed_ms(pkg, lambda: survey.enqueue_survey(survey._pos, radius_sq=r2, potentials=True), seconds)
    t_lists, _ = timed_ms(pkg, lambda: survey.enqueue_lists(survey._pos, radius_sq=r2, capacity=total), seconds)
    t_euler, _ = timed_ms(pkg, euler, seconds)
    plan = pkg.neighbour_plan(n, dtype)
    for buf in (here, other, velocities):
        buf.free()
    survey.free()
    return {"precision": "fp32", "num_bodies": n,
            "plan": {"bodies_per_lane": plan.bodies_per_lane, "waves_per_group": plan.waves_per_group, "unroll": plan.unroll, "tiles": plan.tiles, "list_ranges": plan.list_ranges},
            "survey_ms": round(t_plain, 5), "survey_calls_timed": reps, "survey_with_potentials_ms": round(t_pot, 5), "lists_ms": round(t_lists, 5),
            "list_entries": total, "mean_list": round(total / n, 2), "one_sided_fast_step_ms": round(t_euler, 5),
            "survey_ratio": round(t_plain / t_euler, 3), "model": round(MODEL_PLAIN, 3), "ratio_over_model": round(t_plain / t_euler / MODEL_PLAIN, 3),
            "potentials_ratio": round(t_pot / t_euler, 3), "potentials_model": round(MODEL_POT, 3), "potentials_ratio_over_model": round(t_pot / t_euler / MODEL_POT, 3),
            "lists_ratio": round(t_lists / t_euler, 3), "pairs_per_s": float(n) * n / (t_plain * 1e-3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=0.25, help="timed device time per measurement (default 0.25)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
    for n in POINTS:
        row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **point(pkg, n, args.seconds)}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
