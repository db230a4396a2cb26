"""CovarianceSamplingDataPointsFilter on the device (icpmi_covariance_sampling): call time per (cloud size, nbSample).

    python scripts/covariance_sampling_bench.py [--reps 30] [--warmup 3] [--case NAME] [--out FILE.json]

Every call uploads the cloud and its normals, runs the pipeline (moments, L, C, Jacobi, keys, one radix sort of the six lists, the greedy
loop) and downloads the selection; it returns after a stream synchronisation, so the wall time of a call is the device-synchronised call
time.  Normals come from icp.surfaceNormals (knn 10) once per case, outside the timing.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/covariance_sampling_bench.py --case NAME --reps 20`.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def cases():
    import norlab_icp_mapper_amd as amd
    scan = amd.synth.make_scene(m=10, n=100_000)["scan"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))
    xyz = np.concatenate([z[f"scan{k}_xyz"] for k in range(3)])[:100_000]
    lidar = np.concatenate([xyz, np.ones((xyz.shape[0], 1), np.float32)], 1).astype(np.float32)
    big = amd.synth.make_scene(m=1_000_000, n=10)["map"]
    return [("synth100k_5000", scan, 5000), ("bundled100k_5000", lidar, 5000), ("map1M_5000", big, 5000),
            ("synth100k_50000", scan, 50_000), ("bundled100k_50000", lidar, 50_000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import norlab_icp_mapper_amd as amd
    icp = amd.ICPSequence()
    rows = []
    for name, cloud, nb in cases():
        if a.case and name != a.case:
            continue
        cloud = np.ascontiguousarray(cloud, np.float32)
        nrm = icp.surfaceNormals(cloud, 10)
        for _ in range(a.warmup):
            icp.covarianceSampling(cloud, nrm, nb, 1)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            order = icp.covarianceSampling(cloud, nrm, nb, 1)
            ts.append((time.perf_counter() - t0) * 1e3)
        r = dict(case=name, n=int(cloud.shape[0]), nb_sample=nb, torque_norm=1, kept=int(order.shape[0]), ms_median=float(np.median(ts)),
                 ms_min=float(np.min(ts)), ms_p90=float(np.percentile(ts, 90)), reps=a.reps)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
