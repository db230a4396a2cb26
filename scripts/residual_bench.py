"""getResidualError: cost of one evaluation at the headline shape (100 k x 1 M, point-to-plane, maxDist 2, TrimmedDist 0.85), for k = 1
and for the documented knn-6 chain, next to one iteration of the same chain's registration from the same session.

    python scripts/residual_bench.py [--reps 30] [--warmup 3] [--out FILE.json]

An evaluation is one matcher launch, one selection and two small kernels, so one iteration is what it is to be compared against: the
iteration's time is (registerDev with 21 fixed iterations - registerDev with 1) / 20, medians.  The calls alternate inside one loop:
icpmi_residual_error_dev (the scan in HBM), icpmi_residual_error_staged (the scan icpmi_register_prior_dev left there), the two
registrations.  Times are host wall times around the whole call (each waits for its result).  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_ms": float(np.median(ts) * 1e3), "p10_ms": float(np.percentile(ts, 10) * 1e3), "p90_ms": float(np.percentile(ts, 90) * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    n = sc["scan"].shape[0]
    d = torch.from_numpy(sc["scan"]).cuda()
    eye = np.eye(4, dtype=np.float32)
    doc = {"shape": "100 k x 1 M, point-to-plane, maxDist 2.0, TrimmedDist 0.85", "reps": a.reps, "device": torch.cuda.get_device_name(0), "chains": {}}
    for name, k in (("k1", 1), ("docs_knn6", 6)):
        icp = amd.ICPSequence(minimizer=2, knn=k, max_dist=2.0, outliers=[(4, 0.85)])
        assert icp.setMap(sc["map"], sc["normals"])
        T = icp.registerWithPriorDev(d.data_ptr(), n, eye)          # (stages the scan; the pose every evaluation below scores)
        calls = {"residual_dev": lambda: icp.residualDev(d.data_ptr(), n, T), "residual_staged": lambda: icp.residualStaged(T),
                 "register_1_iteration": lambda: icp.registerDev(d.data_ptr(), n, fixed_iterations=1),
                 "register_21_iterations": lambda: icp.registerDev(d.data_ptr(), n, fixed_iterations=21)}
        ts = {key: [] for key in calls}
        res = None
        for rep in range(a.warmup + a.reps):
            for key, fn in calls.items():
                dt, out = timed(fn)
                if rep >= a.warmup:
                    ts[key].append(dt)
                if key == "residual_dev":
                    res = out
        row = {key: stats(v) for key, v in ts.items()}
        row["one_iteration_ms"] = (row["register_21_iterations"]["median_ms"] - row["register_1_iteration"]["median_ms"]) / 20.0
        row["residual"] = {"sum_abs": res.sum_abs, "pairs": res.pairs, "mean_abs": res.sum_abs / res.pairs, "max_abs": float(res.max_abs),
                           "weighted_point_used_ratio": float(res.weighted_point_used_ratio)}
        doc["chains"][name] = row
        icp.close()
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
