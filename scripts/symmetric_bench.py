"""SymmetricPointToPlaneErrorMinimizer: what one loop iteration costs next to plane-to-plane (the yardstick: the same four gathers per pair) and
point-to-plane at the headline shape (100 k x 1 M, maxDist 2, TrimmedDist 0.85), at knn 1 and knn 6.

    python scripts/symmetric_bench.py [--rounds 15] [--warmup 3] [--out profiles/symmetric_bench.json]

Six handles on the same map -- {point-to-plane, plane-to-plane, symmetric} x {knn 1, knn 6} -- take turns, round after round, so that drift
of the machine lands on all alike; medians over the rounds.  Per handle: a whole registration of 20 fixed iterations (one cached graph, host
wall clock around a call that ends in a device synchronise) and one loop iteration (the loop's device time / 20).  All get the reading's
normals handed over; point-to-plane does not read them.  The pair-sum kernel's own time is not in here: it comes from a kernel trace of this
script taken in a run of its own (rocprofv3 --kernel-trace --stats -- python scripts/symmetric_bench.py ...; scripts/kstats.py prints it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ITERS = 20
HANDLES = {"point_to_plane": dict(minimizer=2), "plane_to_plane": dict(minimizer=3, plane_model="gicp"), "symmetric": dict(minimizer=3, plane_model="symmetric")}
KNN = (1, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symmetric_bench.json"))
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    d = torch.from_numpy(sc["scan"]).cuda()
    dn = torch.from_numpy(sc["scan_normals"]).cuda()
    n = sc["scan"].shape[0]
    icps = {}
    for k in KNN:
        for name, kw in HANDLES.items():
            icps[(name, k)] = amd.ICPSequence(knn=k, max_dist=2.0, outliers=[(4, 0.85)], **kw)
            assert icps[(name, k)].setMap(sc["map"], sc["normals"])
    wall = {key: [] for key in icps}
    loop = {key: [] for key in icps}
    pose = {}
    for r in range(a.warmup + a.rounds):
        for key, icp in icps.items():
            t0 = time.perf_counter()
            pose[key] = icp.registerDev(d.data_ptr(), n, fixed_iterations=ITERS, d_normals_ptr=dn.data_ptr())
            t1 = time.perf_counter()
            if r >= a.warmup:
                wall[key].append((t1 - t0) * 1e3)
                loop[key].append(float(icp.stats.loop_ms))
    med = lambda v: float(np.median(v))
    res = dict(shape="100k x 1M, maxDist 2, TrimmedDist 0.85", iterations=ITERS, rounds=a.rounds, handles={}, ratio_iteration_to_plane_to_plane={},
               ratio_iteration_to_point_to_plane={})
    for (name, k) in icps:
        key = (name, k)
        dt, dr = amd.synth.pose_error(pose[key], sc["T_gt"])
        res["handles"][f"{name}_knn{k}"] = dict(registration_ms=med(wall[key]), registration_ms_p10=float(np.percentile(wall[key], 10)),
                                                registration_ms_p90=float(np.percentile(wall[key], 90)), loop_ms=med(loop[key]),
                                                iteration_us=med(loop[key]) / ITERS * 1e3, iteration_us_p10=float(np.percentile(loop[key], 10)) / ITERS * 1e3,
                                                iteration_us_p90=float(np.percentile(loop[key], 90)) / ITERS * 1e3, pose_err_m=float(dt), pose_err_rad=float(dr))
    for k in KNN:
        it = lambda name: res["handles"][f"{name}_knn{k}"]["iteration_us"]
        res["ratio_iteration_to_plane_to_plane"][f"knn{k}"] = it("symmetric") / it("plane_to_plane")
        res["ratio_iteration_to_point_to_plane"][f"knn{k}"] = it("symmetric") / it("point_to_plane")
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
