"""Global localisation (icpmi_global_localize_dev) on the bench's 1 M-point map, one MI355X: a reading of 100 k points and the
same reading decimated to about 5 k; s0 = 0.5, 360 yaw steps, the map's bounding box, levels automatic, min_score_ratio 0 and 0.5.

    python scripts/global_localize_bench.py [--reps 15] [--warmup 1] [--out profiles/global_localize_bench.json]
    python scripts/global_localize_bench.py --trace      (only search calls on the 5 k reading, for a kernel trace collected in a run of its own)

Recorded: the pyramid's build time per level and its bytes; nodes, leaves and launches; wall time of the whole call (it waits for its
result), medians of the rounds.  The baseline, in the same session: what the parent commit had for the same question -- lattice poses scored
4096 per call through icpmi_voxel_score_poses_dev on a VoxelMatcher handle of the same map; its time per pose times the window's leaf count is
stated as the exhaustive cost (the calls themselves are timed, the product is arithmetic).  --max-nodes caps a search so that a reading the
bound prunes badly cannot run away with the session; a capped row says proven = false.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S0, YAW_STEPS = 0.5, 360


def stats(ts):
    return {"median_ms": float(np.median(ts) * 1e3), "p10_ms": float(np.percentile(ts, 10) * 1e3), "p90_ms": float(np.percentile(ts, 90) * 1e3), "rounds": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--max-nodes", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=None, help="nodes expanded per round (default: the library's, 64)")
    ap.add_argument("--only", default=None, help="one reading, 100k or 5k; no baseline")
    ap.add_argument("--slow-ms", type=float, default=400.0, help="a call slower than this is timed over 3 rounds, not --reps")
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    from norlab_icp_mapper_amd import icp as I
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    rot = I.yaw_rotations(YAW_STEPS)
    # (the scene's scan is the reading moved by T_gt^-1: the pose the search should land next to is T_gt, a small rotation about all axes)
    full = np.ascontiguousarray(sc["scan"], np.float32)
    readings = {"100k": full, "5k": np.ascontiguousarray(full[::20])}
    icp = amd.ICPSequence(minimizer=1, knn=1, max_dist=2.0, max_iterations=40, use_differential=1)
    assert icp.setMap(sc["map"])
    doc = {"shape": "1 M-point map, s0 0.5, 360 yaw steps, the map's bounding box, levels automatic", "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "max_nodes": a.max_nodes, "batch": a.batch or 64, "rows": {},
           "rounds": "a call slower than --slow-ms is timed over 3 rounds, not --reps: every row says how many its median is of"}
    dev = {k: torch.from_numpy(v).cuda() for k, v in readings.items()}
    if a.trace:
        d = dev["5k"]
        for _ in range(a.warmup + a.reps):
            got = icp.globalLocalizeDev(d.data_ptr(), d.shape[0], rot, S0, max_nodes=a.max_nodes, batch=a.batch)
        print(json.dumps({"trace": "5k, ratio 0", "nodes_scored": got.nodes_scored, "launches": got.launches, "calls": a.warmup + a.reps}))
        icp.close()
        return
    t0 = time.perf_counter()
    first = icp.globalLocalizeDev(dev["5k"].data_ptr(), dev["5k"].shape[0], rot, S0, max_nodes=a.max_nodes, batch=a.batch)      # (builds the pyramid)
    doc["first_call_ms"] = (time.perf_counter() - t0) * 1e3
    info = icp.occupancyInfo()
    doc["pyramid"] = info
    lo, hi = icp.occupancyLevel(S0, 1, 0).min(0), icp.occupancyLevel(S0, 1, 0).max(0)
    leaves = int(np.prod(hi - lo + 1)) * YAW_STEPS
    doc["window_cells"] = (hi - lo + 1).tolist()
    doc["window_leaves"] = leaves
    print("pyramid", json.dumps(info), "window", doc["window_cells"], flush=True)
    if a.only:
        dev = {a.only: dev[a.only]}
    for name, d in dev.items():
        for ratio in (0.0, 0.5):
            ts, got = [], None
            reps = a.reps
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                got = icp.globalLocalizeDev(d.data_ptr(), d.shape[0], rot, S0, min_score_ratio=ratio, max_nodes=a.max_nodes, batch=a.batch)
                dt = time.perf_counter() - t0
                if rep >= a.warmup:
                    ts.append(dt)
                if dt * 1e3 > a.slow_ms:
                    reps = min(reps, 3)
                if len(ts) >= reps:
                    break
            row = stats(ts)
            row.update(n=int(d.shape[0]), min_score_ratio=ratio, found=got.found, proven=got.proven, score=got.score, points=got.points, rotation=got.rotation,
                       cell=list(got.cell), levels=got.levels, nodes_scored=got.nodes_scored, leaves_scored=got.leaves_scored, launches=got.launches,
                       wall_us_per_node=row["median_ms"] * 1e3 / max(got.nodes_scored, 1), fraction_of_leaves=got.nodes_scored / leaves)
            dt_, dr_ = amd.synth.pose_error(got.pose, sc["T_gt"]) if got.found else (None, None)
            row.update(pose_error_m=dt_, pose_error_rad=dr_)
            doc["rows"][f"{name}_ratio{ratio}"] = row
            print(name, ratio, json.dumps(row), flush=True)
    icp.close()
    if a.only:
        print(json.dumps(doc))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        return
    # the baseline: lattice poses through the voxel table's score, 4096 per call
    vox = amd.ICPSequence(minimizer=3, knn=1, max_dist=2.0, outliers=[], voxel_size=S0, max_iterations=40, use_differential=1)
    assert vox.setMap(sc["map"], sc["normals"])
    mean = vox.getMapMean().astype(np.float64)
    poses = np.tile(np.eye(4, dtype=np.float32), (4096, 1, 1))
    for i in range(4096):
        poses[i, :3, :3] = rot[i % YAW_STEPS]
        poses[i, :3, 3] = (mean + S0 * np.array([(i // 360) - 5, (i % 7) - 3, 0.0])).astype(np.float32)
    base = {}
    for name, d in dev.items():
        dn = torch.from_numpy(np.ascontiguousarray(sc["scan_normals"][::(1 if name == "100k" else 20)], np.float32)).cuda()
        ts = []
        for rep in range(1 + 5):
            t0 = time.perf_counter()
            vox.voxelScoresDev(d.data_ptr(), d.shape[0], dn.data_ptr(), poses)
            if rep >= 1:
                ts.append(time.perf_counter() - t0)
        row = stats(ts)
        row["us_per_pose"] = row["median_ms"] * 1e3 / 4096
        row["exhaustive_s_for_the_window"] = row["us_per_pose"] * 1e-6 * leaves
        base[name] = row
        print("baseline", name, json.dumps(row), flush=True)
    doc["baseline_voxel_score_poses"] = base
    vox.close()
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
