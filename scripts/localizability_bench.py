"""Degeneracy-aware point-to-plane solve: what the option costs at the headline shape (100 k x 1 M point-to-plane, maxDist 2,
TrimmedDist 0.85).

    python scripts/localizability_bench.py [--rounds 15] [--warmup 3] [--out profiles/localizability_bench.json]

Three handles on the same map -- off, report (threshold < 0) and constrain (threshold > 0) -- take turns, round after round, so that
drift of the machine lands on all three alike; medians over the rounds.  Per mode: a whole registration of 20 fixed iterations (one
cached graph, host wall clock, the report read back where there is one) and one loop iteration (the loop's device time / 20)."""
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
MODES = {"off": 0.0, "report": -5e-3, "constrain": 5e-3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localizability_bench.json"))
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    sc = amd.synth.make_scene(m=1_000_000, n=100_000)
    d = torch.from_numpy(sc["scan"]).cuda()
    n = sc["scan"].shape[0]
    icps = {}
    for mode, thr in MODES.items():
        icps[mode] = amd.ICPSequence(knn=1, max_dist=2.0, outliers=[(4, 0.85)], degeneracy_threshold=thr)
        assert icps[mode].setMap(sc["map"], sc["normals"])
    wall = {m: [] for m in MODES}
    loop = {m: [] for m in MODES}
    for r in range(a.warmup + a.rounds):
        for mode, icp in icps.items():
            t0 = time.perf_counter()
            icp.registerDev(d.data_ptr(), n, fixed_iterations=ITERS)
            if mode != "off":
                icp.localizability()
            t1 = time.perf_counter()
            if r >= a.warmup:
                wall[mode].append((t1 - t0) * 1e3)
                loop[mode].append(float(icp.stats.loop_ms))
    med = lambda v: float(np.median(v))
    res = dict(shape="100k x 1M, point-to-plane, maxDist 2, TrimmedDist 0.85, knn 1", iterations=ITERS, rounds=a.rounds, modes={})
    for mode in MODES:
        res["modes"][mode] = dict(registration_ms=med(wall[mode]), registration_ms_p10=float(np.percentile(wall[mode], 10)),
                                  registration_ms_p90=float(np.percentile(wall[mode], 90)), loop_ms=med(loop[mode]),
                                  iteration_us=med(loop[mode]) / ITERS * 1e3)
    res["n_degenerate"] = int(icps["constrain"].localizability()["n_degenerate"])
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
