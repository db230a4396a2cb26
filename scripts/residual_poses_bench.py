"""Scoring many candidate poses in one call, and multistart registration, at the headline shape (100 k x 1 M, point-to-plane, maxDist 2,
TrimmedDist 0.85) on one MI355X.

    python scripts/residual_poses_bench.py [--reps 15] [--warmup 2] [--out profiles/residual_poses_bench.json]

- icpmi_residual_error_poses_dev with 1, 16, 64 and 256 poses on the candidate generator's grid against that many calls of
  icpmi_residual_error_dev, for k = 1 (the batched route) and the documented knn-6 chain (the sequential route);
- the same on a grid far from identity (half a turn of yaw, tens of metres): the moved reading no longer walks the map in the tile order
  the sort gave it;
- icpmi_register_multistart_dev with 16 starts against 16 calls of icpmi_register_prior_dev.
Every figure is host wall time around the whole call or loop of calls (each waits for its result); the two sides alternate inside one
loop and the medians are reported.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NPOSES = (1, 16, 64, 256)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_ms": float(np.median(ts) * 1e3), "p10_ms": float(np.percentile(ts, 10) * 1e3), "p90_ms": float(np.percentile(ts, 90) * 1e3)}


def grid(icp_mod, centre, P, half_xy, half_yaw):
    """the first P poses of a generator grid around `centre` (3 steps per side in x and y, 2 in yaw: 245 poses and the centre again for 256)"""
    g = icp_mod.candidate_grid(centre, half_xy, half_xy, half_yaw, 3, 3, 2)
    while g.shape[0] < P:
        g = np.concatenate([g, g[:P - g.shape[0]]])
    return np.ascontiguousarray(g[:P])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    from norlab_icp_mapper_amd import icp as I
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    n = sc["scan"].shape[0]
    d = torch.from_numpy(sc["scan"]).cuda()
    T_gt = np.asarray(sc["T_gt"], np.float32)
    far = amd.synth.make_T((0, 0, np.pi), (20.0, -15.0, 0.0)).astype(np.float32)
    doc = {"shape": "100 k x 1 M, point-to-plane, maxDist 2.0, TrimmedDist 0.85", "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "chains": {}}
    for name, k in (("k1", 1), ("docs_knn6", 6)):
        icp = amd.ICPSequence(minimizer=2, knn=k, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=40, use_differential=1)
        assert icp.setMap(sc["map"], sc["normals"])
        rows = {}
        for where, centre, hxy, hyaw in (("near", T_gt, 1.0, 0.1), ("far", far, 5.0, 0.5)):
            for P in NPOSES:
                if where == "far" and P != 64:
                    continue
                poses = grid(I, centre, P, hxy, hyaw)

                def one_by_one():
                    out = []
                    for T in poses:
                        try:
                            out.append(icp.residualDev(d.data_ptr(), n, T).bits())
                        except I.ConvergenceError:
                            out.append(None)
                    return out

                calls = {"poses_call": lambda: icp.residualsDev(d.data_ptr(), n, poses), "single_calls": one_by_one}
                ts = {key: [] for key in calls}
                got = {}
                for rep in range(a.warmup + a.reps):
                    for key, fn in calls.items():
                        dt, out = timed(fn)
                        got[key] = out
                        if rep >= a.warmup:
                            ts[key].append(dt)
                sc_out = got["poses_call"]
                same = [(r.bits() if s == 0 else None) for s, r in zip(sc_out.status, sc_out.residuals)] == got["single_calls"]
                row = {key: stats(v) for key, v in ts.items()}
                row.update(n_poses=P, batched=sc_out.batched, same_bits=bool(same), ok_poses=int(sum(1 for s in sc_out.status if s == 0)),
                           ratio_single_over_poses=row["single_calls"]["median_ms"] / row["poses_call"]["median_ms"],
                           ms_per_pose=row["poses_call"]["median_ms"] / P)
                rows[f"{where}_{P}"] = row
        # multistart: 16 perturbed priors
        rng = np.random.default_rng(7)
        priors = [(amd.synth.make_T(rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.1, 0.1, 3)) @ sc["T_gt"]).astype(np.float32) for _ in range(16)]

        def alone():
            return [icp.registerWithPriorDev(d.data_ptr(), n, P) for P in priors]

        calls = {"multistart_16": lambda: icp.registerMultiStartDev(d.data_ptr(), n, priors)[0], "register_prior_x16": alone}
        ts = {key: [] for key in calls}
        got = {}
        for rep in range(a.warmup + a.reps):
            for key, fn in calls.items():
                dt, out = timed(fn)
                got[key] = out
                if rep >= a.warmup:
                    ts[key].append(dt)
        row = {key: stats(v) for key, v in ts.items()}
        row["same_bits"] = bool(all(np.array_equal(x, y) for x, y in zip(got["multistart_16"], got["register_prior_x16"])))
        row["ratio_alone_over_multistart"] = row["register_prior_x16"]["median_ms"] / row["multistart_16"]["median_ms"]
        rows["multistart"] = row
        doc["chains"][name] = rows
        icp.close()
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
