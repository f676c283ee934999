#!/usr/bin/env python3
"""Hermite evaluation and step (nb_hermite_eval_* / nb_hermite_step_*, include/nbody_hip_hermite.h), and the 6th-order scheme's
(nb_hermite6_eval_* / nb_hermite6_step_*, include/nbody_hip_hermite6.h), next to the one-sided FAST step of the product (nb_integrate_*
without a workspace) timed in the same process.  One JSON line per point:

  fp32 at 16 384, 65 536 and 262 144 bodies; fp64 at 65 536 and 262 144.

Times come from device events after a warm-up, over at least --seconds of timed calls.  `model` is the issue-cost ratio of the two
fp32 loops as compiled (25 packed ops + 2 v_rsq_f32 against 11 + 2 per packed pair of interactions, a packed op every 4.08 and a
v_rsq_f32 every 8.3 SIMD cycles: DESIGN.md 5.2 / 5.6); `hermite6_model` the same for the 6th-order loop against the 4th-order one (47 + 2
against 25 + 2: DESIGN.md 5.13).  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/hermite_bench.py`.

  python tools/hermite_bench.py [--seconds 0.25] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from tools.ensemble_bench import timed_ms  # noqa: E402

POINTS = [(np.float32, 16384), (np.float32, 65536), (np.float32, 262144), (np.float64, 65536), (np.float64, 262144)]
MODEL_FP32 = (25 * 4.08 + 2 * 8.3) / (11 * 4.08 + 2 * 8.3)
MODEL6_FP32 = (47 * 4.08 + 2 * 8.3) / (25 * 4.08 + 2 * 8.3)


def point(pkg, dtype, n, seconds):
    f32 = dtype == np.float32
    scalar = np.float32 if f32 else float
    rng = np.random.default_rng(1)
    pos, vel = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    pos[:, :3], pos[:, 3], vel[:, :3] = rng.standard_normal((n, 3)), 1.0, rng.standard_normal((n, 3))
    eps2, dt = dtype(0.01), dtype(1e-4)
    lib, her = pkg.lib(), pkg.hermite_lib()
    (lib.nb_set_softening_sq_f32 if f32 else lib.nb_set_softening_sq_f64)(scalar(eps2))
    system = pkg.HermiteSystem(n, dtype, softening_sq=eps2)
    system.set_state(pos, vel)
    other = pkg.DeviceBuffer(pos.nbytes)
    single = lib.nb_integrate_f32 if f32 else lib.nb_integrate_f64
    state = {"read": system._pos.ptr.value, "write": other.ptr.value}

    def euler():
        pkg.check(single(state["write"], state["read"], system._vel.ptr, scalar(dt), scalar(1.0), n, 256, pkg.NB_MODE_FAST, None), "nb_integrate")
        state["read"], state["write"] = state["write"], state["read"]

    t_eval, _ = timed_ms(pkg, system.eval, seconds)
    t_step, reps = timed_ms(pkg, lambda: system.step(dt), seconds)
    system.set_state(pos, vel)
    t_euler, _ = timed_ms(pkg, euler, seconds)
    system.free(), other.free()
    # the 6th-order scheme: nb_hermite6_eval_* with the stored accelerations as acc_in (one pack and one evaluation launch), and the step
    sixth = pkg.Hermite6System(n, dtype, softening_sq=eps2)
    sixth.set_state(pos, vel)
    sixth.eval()
    eval6 = getattr(pkg.hermite6_lib(), "nb_hermite6_eval_f32" if f32 else "nb_hermite6_eval_f64")

    def evaluate6():
        pkg.check(eval6(sixth._acc.ptr, sixth._jerk.ptr, sixth._snap.ptr, sixth._pos.ptr, sixth._vel.ptr, sixth._acc.ptr, sixth._workspace.ptr, sixth._workspace_bytes, n,
                        scalar(eps2), None), "nb_hermite6_eval")

    t_eval6, _ = timed_ms(pkg, evaluate6, seconds)
    t_step6, reps6 = timed_ms(pkg, lambda: sixth.step(dt), seconds)
    sixth.free()
    plan = pkg.hermite_plan(n, dtype)
    inter = float(n) * n
    row = {"precision": "fp32" if f32 else "fp64", "num_bodies": n,
           "plan": {"bodies_per_lane": plan.bodies_per_lane, "waves_per_group": plan.waves_per_group, "unroll": plan.unroll, "groups": plan.groups},
           "hermite_eval_ms": round(t_eval, 5), "hermite_step_ms": round(t_step, 5), "hermite_steps_timed": reps, "one_sided_fast_step_ms": round(t_euler, 5),
           "step_ratio": round(t_step / t_euler, 3), "hermite_interactions_per_s": inter / (t_step * 1e-3), "one_sided_interactions_per_s": inter / (t_euler * 1e-3)}
    row.update({"hermite6_eval_ms": round(t_eval6, 5), "hermite6_step_ms": round(t_step6, 5), "hermite6_steps_timed": reps6,
                "hermite6_over_hermite_step": round(t_step6 / t_step, 3), "hermite6_interactions_per_s": inter / (t_step6 * 1e-3)})
    if f32:
        row["model"] = round(MODEL_FP32, 3)
        row["ratio_over_model"] = round(t_step / t_euler / MODEL_FP32, 3)
        row["hermite6_model"] = round(MODEL6_FP32, 3)
        row["hermite6_ratio_over_model"] = round(t_step6 / t_step / MODEL6_FP32, 3)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=0.25, help="timed device time per measurement (default 0.25)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
    for dtype, n in POINTS:
        row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **point(pkg, dtype, n, args.seconds)}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
