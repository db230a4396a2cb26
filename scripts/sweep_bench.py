#!/usr/bin/env python3
"""What sweep registration costs, next to the registration it stands beside (profiles/sweep_bench.json).

A 100 k point skewed scan of the analytic room (tests/sweep_cases.py's motion) against a 1 M point map, maxDist 2 + TrimmedDist 0.85, at
k = 1 and knn 6.  Per round, alternating on the same handle in the same session: one sweep iteration (icpmi_register_sweep_dev with
max_iterations = 1), the whole 12-iteration call, and icpmi_register_prior_dev with 12 fixed iterations (the yardstick: the parent commit
cannot run the new path).  Medians over the rounds; the scan and its point times stay in HBM."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deskew_reference as dr  # noqa: E402
import localizability_reference as lr  # noqa: E402
import sweep_cases as sc  # noqa: E402
import sweep_reference as sr  # noqa: E402

F = np.float32
M, N, ROUNDS, WARMUP, ITERATIONS = 1_000_000, 100_000, 15, 3, 12


def scene():
    s = lr.scene("room", m=M, n=N)
    P = s["reading"][:, :3].astype(np.float64)
    az = np.arctan2(P[:, 1] - sc.SENSOR[1], P[:, 0] - sc.SENSOR[0])
    t_rel = (((az + np.pi) / (2 * np.pi)) * (sr.END_S - sr.BEGIN_S) / sr.UNIT_S).astype(F)
    alpha = sr.alpha_of(t_rel)
    Tb = lr.make_T(-0.5 * np.array(sc.MOTION_ROT), -0.5 * np.array(sc.MOTION_TRANS))
    Te = lr.make_T(0.5 * np.array(sc.MOTION_ROT), 0.5 * np.array(sc.MOTION_TRANS))
    R, p = dr.pose_at([0.0, 1.0], np.stack([sr.pose7(Tb), sr.pose7(Te)]), alpha.astype(np.float64))
    scan = np.ones((N, 4), F)
    scan[:, :3] = R.inv().apply(P - p).astype(F)
    return s["map"], s["normals"], scan, t_rel, alpha, sr.world_points(scan, alpha, Tb, Te)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    import norlab_icp_mapper_amd as amd
    mp, nm, scan, t_rel, alpha, truth = scene()
    d_scan, d_t = torch.from_numpy(scan).cuda(), torch.from_numpy(t_rel).cuda()
    T0 = sc.STARTS["off"].astype(F)
    span = dict(begin=sr.BEGIN_S, end=sr.END_S, unit=sr.UNIT_S, min_step_rot=0.0, min_step_trans=0.0)
    doc = {"what": "ms per call, medians of %d alternating rounds after %d warm-up rounds; %d x %d, maxDist 2 + TrimmedDist 0.85, from 0.3 m / 0.05 rad off; "
                   "scan and point times resident in HBM" % (ROUNDS, WARMUP, N, M), "cases": {}}
    for k in (1, 6):
        icp = amd.ICPSequence(knn=k, max_dist=sc.MAX_DIST, outliers=[(sc.OUT_TRIMMED, sc.TRIM_RATIO)], max_iterations=ITERATIONS, use_differential=0)
        assert icp.setMap(mp, nm)
        rows = {"sweep_1_iteration": [], "sweep_12_iterations": [], "register_prior_12_iterations": []}
        res = None
        for r in range(WARMUP + ROUNDS):
            a, _ = timed(lambda: icp.register_sweep_dev(d_scan.data_ptr(), N, d_t.data_ptr(), T0, T0, max_iterations=1, **span))
            b, res = timed(lambda: icp.register_sweep_dev(d_scan.data_ptr(), N, d_t.data_ptr(), T0, T0, max_iterations=ITERATIONS, **span))
            c, _ = timed(lambda: icp.registerWithPriorDev(d_scan.data_ptr(), N, T0))
            assert icp.stats.iterations == ITERATIONS
            if r >= WARMUP:
                for key, v in zip(rows, (a, b, c)):
                    rows[key].append(v)
        err, worst = sr.point_error(sr.world_points(scan, alpha, res.T_begin, res.T_end), truth)
        case = {key: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for key, v in rows.items()}
        case["mean_point_error_m"], case["max_point_error_m"], case["pairs"] = err, worst, res.pairs
        doc["cases"]["knn_%d" % k] = case
        print(k, json.dumps(case))
        icp.close()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sweep_bench.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
