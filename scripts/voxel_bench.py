"""VoxelMatcher: what one loop iteration costs next to plane-to-plane through the nearest-neighbour matcher at the headline shape
(100 k x 1 M), what the table of a 1 M-point map costs to build, and the table's lookup against a binary search over the sorted keys.

    python scripts/voxel_bench.py [--rounds 15] [--warmup 3] [--out profiles/voxel_bench.json]

Three handles on the same map -- VoxelMatcher at sizes 0.5 and 1.0, and plane-to-plane at knn 1 with maxDist 2 and no filter -- take turns,
round after round, so that drift of the machine lands on all alike; medians over the rounds.  Per handle: a whole registration of 20 fixed
iterations (one cached graph, host wall clock) and one loop iteration (the loop's device time / 20).  The table: icpmi_debug_voxel_build_times
(HIP events around its sort, reduce and fill stages) and icpmi_debug_voxel_lookup_times (100 k queries, the reading at the true pose).
Nothing is compared against a threshold: the record says what was measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ITERS = 20
SIZES = (0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_bench.json"))
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    d = torch.from_numpy(sc["scan"]).cuda()
    dn = torch.from_numpy(sc["scan_normals"]).cuda()
    n = sc["scan"].shape[0]
    icps = {f"voxel_{s}": amd.ICPSequence(knn=1, max_dist=2.0, outliers=[], minimizer=3, voxel_size=s) for s in SIZES}
    icps["plane_to_plane_knn1"] = amd.ICPSequence(knn=1, max_dist=2.0, outliers=[], minimizer=3)
    for icp in icps.values():
        assert icp.setMap(sc["map"], sc["normals"])
    wall = {key: [] for key in icps}
    loop = {key: [] for key in icps}
    pose, pairs = {}, {}
    for r in range(a.warmup + a.rounds):
        for key, icp in icps.items():
            t0 = time.perf_counter()
            pose[key] = icp.registerDev(d.data_ptr(), n, fixed_iterations=ITERS, d_normals_ptr=dn.data_ptr())
            t1 = time.perf_counter()
            pairs[key] = int(icp.stats.pairs)
            if r >= a.warmup:
                wall[key].append((t1 - t0) * 1e3)
                loop[key].append(float(icp.stats.loop_ms))
    med = lambda v: float(np.median(v))
    res = dict(shape="100k x 1M; plane-to-plane: knn 1, maxDist 2, no filter", iterations=ITERS, rounds=a.rounds, handles={}, ratio_iteration={},
               table={})
    for key in icps:
        dt, dr = amd.synth.pose_error(pose[key], sc["T_gt"])
        res["handles"][key] = dict(registration_ms=med(wall[key]), registration_ms_p10=float(np.percentile(wall[key], 10)),
                                   registration_ms_p90=float(np.percentile(wall[key], 90)), loop_ms=med(loop[key]),
                                   iteration_us=med(loop[key]) / ITERS * 1e3, pairs_last=pairs[key], pose_err_m=float(dt), pose_err_rad=float(dr))
    for s in SIZES:
        res["ratio_iteration"][f"voxel_{s}"] = res["handles"][f"voxel_{s}"]["iteration_us"] / res["handles"]["plane_to_plane_knn1"]["iteration_us"]
    # the table of the 1 M-point map: build stages and lookup, per size
    q = np.ascontiguousarray(sc["scan"], dtype=np.float32).copy()
    for s in SIZES:
        icp = icps[f"voxel_{s}"]
        q[:, :3] = sc["scan"][:, :3] - icp.getMapMean()[None, :]
        stages = []
        for _ in range(a.rounds):
            t = (C.c_float * 3)()
            icp._check(icp._lib.icpmi_debug_voxel_build_times(icp._h, t))
            stages.append(list(t))
        stages = np.median(np.array(stages), 0)
        ms, bad = (C.c_float * 2)(), C.c_int64(-1)
        icp._check(icp._lib.icpmi_debug_voxel_lookup_times(icp._h, q.ctypes.data, n, 50, ms, C.byref(bad)))
        nv = C.c_int64(0)
        icp._lib.icpmi_get_voxel_map(icp._h, 0, None, None, None, None, C.byref(nv))
        res["table"][f"size_{s}"] = dict(voxels=int(nv.value), build_sort_ms=float(stages[0]), build_reduce_ms=float(stages[1]), build_fill_ms=float(stages[2]),
                                         lookup_table_us=float(ms[0]) * 1e3, lookup_binary_search_us=float(ms[1]) * 1e3, lookup_queries=int(n),
                                         lookup_mismatches=int(bad.value))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
