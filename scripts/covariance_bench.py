"""PointToPlaneWithCovErrorMinimizer: cost of the covariance pass at the headline shape (100 k x 1 M point-to-plane, TrimmedDist 0.85).

    python scripts/covariance_bench.py [--reps 50] [--warmup 5] [--knn 1] [--cov 0|1] [--out FILE.json]

Times registrations (20 fixed iterations, one cached graph) with the covariance on or off; the extra device time per registration comes
from a run under `rocprofv3 --kernel-trace --stats -- python scripts/covariance_bench.py --knn K --cov 1` (cov_pairs_kernel +
cov_solve_kernel), and a --cov 0 trace shows the kernels a registration launched before the feature.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--knn", type=int, default=1)
    ap.add_argument("--cov", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    icp = amd.ICPSequence(knn=a.knn, outliers=[(4, 0.85)], covariance=a.cov)
    assert icp.setMap(sc["map"], sc["normals"])
    d = torch.from_numpy(sc["scan"]).cuda()
    n = sc["scan"].shape[0]
    for _ in range(a.warmup):
        icp.registerDev(d.data_ptr(), n, fixed_iterations=20)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        icp.registerDev(d.data_ptr(), n, fixed_iterations=20)
        if a.cov:
            icp.errorMinimizer.getCovariance()   # (waits for the two launches behind the loop)
        ts.append(time.perf_counter() - t0)
    res = dict(knn=a.knn, cov=a.cov, reps=a.reps, median_ms=float(np.median(ts) * 1e3), p10_ms=float(np.percentile(ts, 10) * 1e3),
               p90_ms=float(np.percentile(ts, 90) * 1e3), iterations=int(icp.stats.iterations))
    if a.cov:
        res["cov_diag"] = [float(v) for v in np.diag(icp.errorMinimizer.getCovariance())]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
