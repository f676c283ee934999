#!/usr/bin/env python3
"""The K nearest neighbours (nb_knn_survey_f32, include/nbody_hip_knn.h) next to the neighbour survey without potentials
(nb_neighbour_survey_f32) timed in the same process.  One JSON line per point: fp32 on a standard normal cloud at 16 384, 65 536 and
262 144 bodies x K = 1, 6 and 16; the lists alone (one launch) and, for K >= 2, with the densities and the structure record (four).

Times come from device events after a warm-up, over at least --seconds of timed calls.  `model` is the ratio of vector operations per
body j and packed pair of bodies i of the two loops as compiled, with the rates at which a randomly ordered cloud enters the insertion
path: `groups_model` of the groups of 4 bodies j and `candidates_model` of the candidates.  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/knn_bench.py`.

  python tools/knn_bench.py [--seconds 0.25] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402
from tools.ensemble_bench import timed_ms  # noqa: E402

POINTS = [16384, 65536, 262144]
KS = [1, 6, 16]
SURVEY_OPS = 6 + 7


def entering_rate(a, t):
    return 1.0 if a >= t else a * (1 + math.log(t / a)) / t


def model(n, k, plan):
    t = n / plan.waves_per_group
    groups, candidates = entering_rate(512 * k, t), entering_rate(64 * k, t)
    ops = 6 + 3 + groups * 6 + candidates * 2 * (6 * plan.capacity + 2)
    return ops / SURVEY_OPS, groups, candidates


def point(pkg, pos, k, seconds, t_survey):
    n, dtype = pos.shape[0], np.float32
    knn = pkg.KnnSurvey(n, dtype, max_k=k)
    knn._pos.upload(pos)
    t_lists, reps = timed_ms(pkg, lambda: knn.enqueue_survey(knn._pos, k, densities=False, structure=False), seconds)
    t_all = timed_ms(pkg, lambda: knn.enqueue_survey(knn._pos, k), seconds)[0] if k >= 2 else None
    plan = pkg.knn_plan(n, k, dtype)
    ratio, groups, candidates = model(n, k, plan)
    knn.free()
    return {"precision": "fp32", "num_bodies": n, "k": k,
            "plan": {"bodies_per_lane": plan.bodies_per_lane, "waves_per_group": plan.waves_per_group, "capacity": plan.capacity, "tiles": plan.tiles, "lds_bytes": plan.lds_bytes},
            "lists_ms": round(t_lists, 5), "calls_timed": reps, "with_record_ms": None if t_all is None else round(t_all, 5), "neighbour_survey_ms": round(t_survey, 5),
            "ratio": round(t_lists / t_survey, 3), "model": round(ratio, 3), "ratio_over_model": round(t_lists / t_survey / ratio, 3),
            "groups_model": round(groups, 3), "candidates_model": round(candidates, 4), "pairs_per_s": float(n) * n / (t_lists * 1e-3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=0.25, help="timed device time per measurement (default 0.25)")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    args = ap.parse_args()
    pkg = entry.load_package()
    pkg.check(pkg.lib().nb_set_device(0), "nb_set_device")
    for n in POINTS:
        rng = np.random.default_rng(7)
        pos = np.zeros((n, 4), np.float32)
        pos[:, :3], pos[:, 3] = rng.standard_normal((n, 3)), 1.0 / n
        survey = pkg.NeighbourSurvey(n, np.float32)
        survey._pos.upload(pos)
        t_survey, _ = timed_ms(pkg, lambda: survey.enqueue_survey(survey._pos, radius_sq=np.float32(0.01)), args.seconds)
        for k in KS:
            row = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), **point(pkg, pos, k, args.seconds, t_survey)}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
        survey.free()


if __name__ == "__main__":
    main()
