"""VoxelGridDataPointsFilter on the device (icpmi_voxel_grid): call time and the largest voxel population of each case.

    python scripts/voxel_grid_bench.py [--reps 50] [--warmup 5] [--case NAME] [--out FILE.json]

Every call uploads the cloud, runs the pipeline and downloads the result; it returns after a stream synchronisation, so the wall
time of a call is the device-synchronised call time.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/voxel_grid_bench.py --case NAME --reps 20`.  Not part of bench.py."""
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
    out = []
    for vs in (0.1, 0.3, 1.0):
        out.append((f"synth100k_{vs:g}", scan, vs))
    for vs in (0.1, 0.3, 1.0):
        out.append((f"bundled100k_{vs:g}", lidar, vs))
    out.append(("map1M_0.1", big, 0.1))
    out.append(("map1M_50", big, 50.0))   # a few voxels of ~10^5 points: the serial per-voxel sums at their longest
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import norlab_icp_mapper_amd as amd
    import voxel_grid_reference as vgr
    icp = amd.ICPSequence()
    rows = []
    for name, cloud, vs in cases():
        if a.case and name != a.case:
            continue
        cloud = np.ascontiguousarray(cloud, np.float32)
        for _ in range(a.warmup):
            icp.voxelGrid(cloud, vs)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            order, _, _ = icp.voxelGrid(cloud, vs)
            ts.append((time.perf_counter() - t0) * 1e3)
        _, _, idx = vgr.grid(cloud[:, :3], vs)
        pop = int(np.unique(idx, return_counts=True)[1].max())
        r = dict(case=name, n=int(cloud.shape[0]), vsize=vs, voxels=int(order.shape[0]), largest_voxel=pop,
                 ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_p90=float(np.percentile(ts, 90)), reps=a.reps)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
