"""The map update of a density-bounding `post:` chain, resident against host path.

    python scripts/max_density_bench.py [--passes 6] [--max-density 10] [--out profiles/max_density_bench.json]

The config-4 replay (tests/config4_data.py: the 14 bundled scans through the C++ Mapper::processInput, DynamicPoints + Octree 0.15 m modules,
one map update per scan) with the `post:` chain SurfaceNormal{knn: 10, keepDensities: 1}, MaxDensity, CutAtDescriptorThreshold, run by the
example harness under NIM_TIMING (scans preloaded; the clock is around the map update inside processInput, which waits for the GPU work):
once with NIM_RESIDENT_MAP_UPDATE=0 -- the host path: download the map, normals and the draw through host pointers, upload, rebuild the
index; what every commit before the resident MaxDensity step did for this chain -- and once resident.  Pass 0 pays the one-time allocations
and is left out; the figure is the median over the scans of the remaining passes, with the spread beside it.  The unchanged config-4 chain
(no densities) is timed next to them as the yardstick the README quotes.  Nothing here is gated; not part of bench.py."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NUM = r"([-+0-9.eE]+)"


def chain_yaml(max_density):
    import config4_data as c4
    shipped = "    - SurfaceNormalDataPointsFilter:\n        knn: 10\n"
    assert shipped in c4.CONFIG4_YAML
    return c4.CONFIG4_YAML.replace(shipped, "    - SurfaceNormalDataPointsFilter:\n        knn: 10\n        keepDensities: 1\n"
                                   "    - MaxDensityDataPointsFilter:\n        maxDensity: %g\n" % max_density)


def replay(exe, tmp, yaml, passes, resident):
    cfg = os.path.join(tmp, "config_%d.yaml" % resident)
    open(cfg, "w").write(yaml)
    env = dict(os.environ, NIM_TIMING=str(passes), NIM_RESIDENT_MAP_UPDATE=str(resident))
    run = subprocess.run([exe, tmp, cfg], capture_output=True, text=True, timeout=900, env=env)
    if run.returncode != 0:
        return {"status": "failed", "reason": (run.stderr + run.stdout)[-400:]}
    per = [tuple(map(float, m)) for m in re.findall(
        rf"timing: pass {NUM} scan {NUM} points {NUM} process_ms {NUM} register_ms {NUM} update_ms {NUM} iterations {NUM} map {NUM}", run.stdout)]
    res = re.findall(r"resident map updates: (\d+)", run.stdout)
    warm = [r for r in per if r[0] >= 1]
    if not warm:
        return {"status": "failed", "reason": "no timing line of a warm pass in the harness output: " + run.stdout[-300:]}
    upd = np.array([r[5] for r in warm])
    last = [r for r in warm if r[0] == warm[-1][0]]
    return {"status": "measured on the GPU", "passes_timed": passes - 1, "scans_per_pass": len(last), "update_ms_median": float(np.median(upd)),
            "update_ms_min": float(upd.min()), "update_ms_p90": float(np.percentile(upd, 90)), "update_ms_mean": float(upd.mean()),
            "update_ms_per_scan_last_pass": [round(r[5], 4) for r in last], "register_ms_median": float(np.median([r[4] for r in warm if r[1] > 1])),
            "map_points_final": int(last[-1][7]), "resident_map_updates_reported": int(res[-1]) if res else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=6, help="replays of the 14 scans per process; the first is warm-up")
    ap.add_argument("--max-density", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import config4_data as c4
    exe = os.path.join(ROOT, "norlab_icp_mapper_amd", "build_map_from_scans_and_trajectory")
    z = np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))
    out = {"workload": "config-4 replay, post: SurfaceNormal{knn 10, keepDensities 1} + MaxDensity{maxDensity %g} + CutAtDescriptorThreshold; "
                       "one map update per scan, update_ms = Mapper::lastMapUpdateMs()" % a.max_density,
           "passes": a.passes, "warmup_passes": 1}
    with tempfile.TemporaryDirectory() as tmp:
        c4.write_bundled_dataset(tmp, z)
        out["host_path"] = replay(exe, tmp, chain_yaml(a.max_density), a.passes, 0)
        out["resident"] = replay(exe, tmp, chain_yaml(a.max_density), a.passes, 1)
        out["config4_unchanged_resident"] = replay(exe, tmp, c4.CONFIG4_YAML, a.passes, 1)
    h, r = out["host_path"], out["resident"]
    if "update_ms_median" in h and "update_ms_median" in r:
        out["host_over_resident"] = h["update_ms_median"] / r["update_ms_median"]
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
