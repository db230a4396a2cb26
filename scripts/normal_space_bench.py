"""NormalSpaceDataPointsFilter on the device (icpmi_normal_space_sampling): call time and kernel times per (cloud size, nbSample).

    python scripts/normal_space_bench.py [--reps 30] [--warmup 3] [--case NAME] [--out profiles/normal_space_bench.json]
    python scripts/normal_space_bench.py --kernels DIR          # DIR: where the rocprofv3 runs below wrote their output

Every call uploads the cloud and its normals, runs the pipeline (keys, one radix sort, bucket bounds, the R* search, keep flags, the flag
scan, the compaction) and downloads the selection; it returns after a stream synchronisation, so the wall time of a call is the
device-synchronised call time.  Normals are random unit vectors (the time does not depend on them beyond the bucket populations); seed 1,
epsilon 0.09817.  Kernel times come from separate runs, one per case, under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CASE -- python scripts/normal_space_bench.py --case CASE --reps 20 --warmup 3`; --kernels reads their
`*kernel_stats.csv` and merges the per-call averages into the rows.  A case that was not run is written as "not measured".  Nothing here is
gated; not part of bench.py."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [("synth100k_5000", 100_000, 5000), ("synth1M_5000", 1_000_000, 5000), ("synth1M_500000", 1_000_000, 500_000)]


def cloud_of(n):
    rng = np.random.default_rng(n)
    xyz = rng.uniform([-30, -12, -3], [30, 12, 5], (n, 3))
    nrm = rng.normal(size=(n, 3)) * [1.0, 0.6, 1.4]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([xyz, np.ones((n, 1))], 1).astype(np.float32), np.ascontiguousarray(nrm, np.float32)


def kernel_rows(directory, calls):
    """rocprofv3's kernel_stats.csv of one case -> {kernel: microseconds per call}, or None"""
    found = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return None
    out = {}
    with open(found[0]) as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
            out[name] = out.get(name, 0.0) + float(row["TotalDurationNs"]) * 1e-3 / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None, help="directory with one rocprofv3 output directory per case (see above)")
    ap.add_argument("--kernel-calls", type=int, default=23, help="calls of the traced runs (reps + warmup)")
    a = ap.parse_args()
    import norlab_icp_mapper_amd as amd
    icp = amd.ICPSequence()
    rows = []
    for name, n, nb in CASES:
        if a.case and name != a.case:
            rows.append(dict(case=name, n=n, nb_sample=nb, status="not measured", reason="the case was not run"))
            continue
        cloud, nrm = cloud_of(n)
        for _ in range(a.warmup):
            icp.normalSpaceSampling(cloud, nrm, nb)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            order = icp.normalSpaceSampling(cloud, nrm, nb)
            ts.append((time.perf_counter() - t0) * 1e3)
        r = dict(case=name, n=n, nb_sample=nb, seed=1, epsilon=0.09817, kept=int(order.shape[0]), ms_median=float(np.median(ts)),
                 ms_min=float(np.min(ts)), ms_p90=float(np.percentile(ts, 90)), reps=a.reps)
        k = kernel_rows(os.path.join(a.kernels, name), a.kernel_calls) if a.kernels else None
        if k is None:
            r["kernels_us_per_call"] = "not measured"
        else:
            r["kernels_us_per_call"] = {kn: round(v, 2) for kn, v in sorted(k.items(), key=lambda kv: -kv[1])}
            r["kernels_us_per_call_total"] = round(sum(k.values()), 2)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
