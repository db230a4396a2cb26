"""IntensityPointToPlaneErrorMinimizer: what one loop iteration costs next to point-to-plane on the same handle at the headline shape
(100 k x 1 M, maxDist 2, TrimmedDist 0.85), at knn 1 and knn 6, and what icpmi_set_map_intensity costs at 1 M points.

    python scripts/intensity_bench.py [--rounds 15] [--warmup 3] [--out profiles/intensity_bench.json]

Two handles on the same map (knn 1, knn 6), each run with the term (weight 0.032) and without it (weight 0) turn by turn, round after round,
so that drift of the machine lands on both alike; medians over the rounds.  Per turn: a whole registration of 20 fixed iterations (one cached
graph per weight, host wall clock around a call that ends in a device synchronise) and one loop iteration (the loop's device time / 20).  The
intensities are a synthetic field on the benchmark clouds (tests/intensity_reference.py: field, no noise).  icpmi_set_map_intensity: the whole
call (upload, self search with k = 11, gradients) on the host clock, the first call of each handle (which sizes the private search handle's
buffers) apart from the warm ones.  Kernel times are not in here: the pair-sum kernel's own time and the search and gradient kernels of
icpmi_set_map_intensity come from a kernel trace of this script taken in a run of its own (rocprofv3 --kernel-trace --stats -- python
scripts/intensity_bench.py ...; scripts/kstats.py prints it), kept as profiles/intensity_kernel_trace.txt."""
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
ITERS = 20
WEIGHT = 0.032
KNN = (1, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensity_bench.json"))
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    import intensity_reference as ir
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    map_i = ir.field(sc["map"][:, :3]).astype(np.float32)
    # the reading's intensities are the field where its points lie in the MAP frame
    gt = np.asarray(sc["T_gt"], np.float64)
    scan_i = ir.field(sc["scan"][:, :3].astype(np.float64) @ gt[:3, :3].T + gt[:3, 3]).astype(np.float32)
    d = torch.from_numpy(sc["scan"]).cuda()
    n = sc["scan"].shape[0]
    icps, set_first_ms, set_warm_ms = {}, [], []
    for k in KNN:
        icps[k] = amd.ICPSequence(knn=k, max_dist=2.0, outliers=[(4, 0.85)], minimizer=2)
        assert icps[k].setMap(sc["map"], sc["normals"])
        for call in range(6):                            # (a handle's first call also creates and sizes its private search handle)
            t0 = time.perf_counter()
            icps[k].setMapIntensity(map_i, knn=10)
            (set_first_ms if call == 0 else set_warm_ms).append((time.perf_counter() - t0) * 1e3)
    turns = [(k, w) for k in KNN for w in (0.0, WEIGHT)]
    wall = {t: [] for t in turns}
    loop = {t: [] for t in turns}
    pose = {}
    for r in range(a.warmup + a.rounds):
        for k, w in turns:
            icp = icps[k]
            icp.setIntensityWeight(w)
            if w > 0:
                icp.setReadingIntensity(scan_i)          # (outside the clock: a one-shot upload of 400 kB, which a host would overlap)
            t0 = time.perf_counter()
            pose[(k, w)] = icp.registerDev(d.data_ptr(), n, fixed_iterations=ITERS)
            t1 = time.perf_counter()
            if r >= a.warmup:
                wall[(k, w)].append((t1 - t0) * 1e3)
                loop[(k, w)].append(float(icp.stats.loop_ms))
    med = lambda v: float(np.median(v))
    res = dict(shape="100k x 1M, maxDist 2, TrimmedDist 0.85", iterations=ITERS, rounds=a.rounds, weight=WEIGHT, handles={}, ratio_iteration_to_point_to_plane={},
               set_map_intensity_1M=dict(first_call_ms=set_first_ms, warm_calls_ms=set_warm_ms, warm_ms=med(set_warm_ms)),
               kernel_times="not in this file: profiles/intensity_kernel_trace.txt (a kernel trace taken in a run of its own)")
    for k, w in turns:
        dt, dr = amd.synth.pose_error(pose[(k, w)], sc["T_gt"])
        name = ("intensity" if w > 0 else "point_to_plane") + f"_knn{k}"
        res["handles"][name] = dict(registration_ms=med(wall[(k, w)]), registration_ms_p10=float(np.percentile(wall[(k, w)], 10)),
                                    registration_ms_p90=float(np.percentile(wall[(k, w)], 90)), loop_ms=med(loop[(k, w)]),
                                    iteration_us=med(loop[(k, w)]) / ITERS * 1e3, iteration_us_p10=float(np.percentile(loop[(k, w)], 10)) / ITERS * 1e3,
                                    iteration_us_p90=float(np.percentile(loop[(k, w)], 90)) / ITERS * 1e3, pose_err_m=float(dt), pose_err_rad=float(dr))
    for k in KNN:
        res["ratio_iteration_to_point_to_plane"][f"knn{k}"] = res["handles"][f"intensity_knn{k}"]["iteration_us"] / res["handles"][f"point_to_plane_knn{k}"]["iteration_us"]
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
