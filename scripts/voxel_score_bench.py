"""Scoring many candidate poses by voxel-table lookup (icpmi_voxel_score_poses_dev) against what a voxel user ran before it: the
nearest-neighbour route, icpmi_residual_error_poses_dev, on the same handle in the same session -- 100 k x 1 M, voxel sizes 0.5 and 1.0,
on one MI355X.

    python scripts/voxel_score_bench.py [--reps 15] [--warmup 2] [--out profiles/voxel_score_bench.json]
    python scripts/voxel_score_bench.py --trace-poses 256      (only voxel-score calls, for a kernel trace collected in a run of its own)
    python scripts/voxel_score_bench.py --sizes 0.5 --poses 1,64,256,4096 --nn-max-poses 0     (the voxel route alone: what every build of
        profiles/voxel_score_sweep.json ran, after VS_PPT / VS_TILE in csrc/voxel.hip were set to the variant and the library rebuilt)

- 1, 16, 64, 256 and 4096 poses on the candidate generator's grid around the true pose, and on a grid far from it (half a turn of yaw, tens
  of metres: most points find no voxel, and the nearest-neighbour route walks the map out of the order its sort gave the reading);
- every figure is host wall time around the whole call (it waits for its result); the routes take turns inside one loop and the medians
  of the rounds are reported.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NPOSES = (1, 16, 64, 256, 4096)
SIZES = (0.5, 1.0)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_ms": float(np.median(ts) * 1e3), "p10_ms": float(np.percentile(ts, 10) * 1e3), "p90_ms": float(np.percentile(ts, 90) * 1e3)}


def grid(icp_mod, centre, P, half_xy, half_yaw):
    """the first P poses of a generator grid around `centre` (3 steps per side in x and y, 2 in yaw: 245 poses), repeated up to P"""
    g = icp_mod.candidate_grid(centre, half_xy, half_xy, half_yaw, 3, 3, 2)
    while g.shape[0] < P:
        g = np.concatenate([g, g[:P - g.shape[0]]])
    return np.ascontiguousarray(g[:P])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-poses", type=int, default=0)
    ap.add_argument("--poses", default=None, help="comma-separated pose counts (default 1,16,64,256,4096)")
    ap.add_argument("--sizes", default=None, help="comma-separated voxel sizes (default 0.5,1.0)")
    ap.add_argument("--nn-max-poses", type=int, default=4096, help="the nearest-neighbour route is timed up to this many poses")
    a = ap.parse_args()
    nposes = NPOSES if a.poses is None else tuple(int(v) for v in a.poses.split(","))
    sizes = SIZES if a.sizes is None else tuple(float(v) for v in a.sizes.split(","))
    from norlab_icp_mapper_amd import _capi
    import torch
    import norlab_icp_mapper_amd as amd
    from norlab_icp_mapper_amd import icp as I
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    n = sc["scan"].shape[0]
    d, dn = torch.from_numpy(sc["scan"]).cuda(), torch.from_numpy(sc["scan_normals"]).cuda()
    T_gt = np.asarray(sc["T_gt"], np.float32)
    far = amd.synth.make_T((0, 0, np.pi), (20.0, -15.0, 0.0)).astype(np.float32)
    import ctypes as C
    sl, tl = C.c_int32(0), C.c_int32(0)
    _capi.load().icpmi_voxel_score_shape(C.byref(sl), C.byref(tl))
    doc = {"shape": "100 k x 1 M, VoxelMatcher on PlaneToPlaneErrorMinimizer; the NN route: k = 1, maxDist 2.0, point-to-plane residual", "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "slice": sl.value, "tile": tl.value, "sizes": {}}
    for size in sizes:
        icp = amd.ICPSequence(minimizer=3, knn=1, max_dist=2.0, outliers=[], voxel_size=size, max_iterations=40, use_differential=1)
        assert icp.setMap(sc["map"], sc["normals"])
        voxels = int(icp.voxelMap()[0].shape[0])                                    # (builds the table: not part of any timed call)
        if a.trace_poses:
            poses = grid(I, T_gt, a.trace_poses, 1.0, 0.1)
            for _ in range(a.warmup + a.reps):
                icp.voxelScoresDev(d.data_ptr(), n, dn.data_ptr(), poses)
            icp.close()
            continue
        rows = {}
        for where, centre, hxy, hyaw in (("near", T_gt, 1.0, 0.1), ("far", far, 5.0, 0.5)):
            for P in nposes:
                poses = grid(I, centre, P, hxy, hyaw)
                calls = {"voxel_score": lambda: icp.voxelScoresDev(d.data_ptr(), n, dn.data_ptr(), poses)}
                if P <= a.nn_max_poses:
                    calls["nn_residuals"] = lambda: icp.residualsDev(d.data_ptr(), n, poses, dn.data_ptr())
                ts = {key: [] for key in calls}
                got = {}
                for rep in range(a.warmup + a.reps):
                    for key, fn in calls.items():
                        dt, out = timed(fn)
                        got[key] = out
                        if rep >= a.warmup:
                            ts[key].append(dt)
                row = {key: stats(v) for key, v in ts.items()}
                vs = got["voxel_score"]
                row.update(n_poses=P, ok_poses=int(sum(1 for s in vs.status if s == 0)), mean_pairs_ratio=float(np.mean([s.pairs_ratio for s in vs.scores])),
                           voxel_ms_per_pose=row["voxel_score"]["median_ms"] / P)
                if "nn_residuals" in row:
                    row["nn_ms_per_pose"] = row["nn_residuals"]["median_ms"] / P
                    row["nn_batched"] = got["nn_residuals"].batched
                    row["ratio_nn_over_voxel"] = row["nn_residuals"]["median_ms"] / row["voxel_score"]["median_ms"]
                rows[f"{where}_{P}"] = row
                print(size, where, P, json.dumps(row), flush=True)
        doc["sizes"][str(size)] = {"voxels": voxels, "rows": rows}
        icp.close()
    if a.trace_poses:
        return
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
