"""The sensor-model filters on the device (icpmi_sensor_model): whole-call time of a run next to the host loops it replaces.

    python scripts/sensor_model_bench.py [--n 100000] [--reps 200] [--warmup 10] [--out FILE.json]

Rows (each call ends in a stream synchronisation or is pure host work, so the wall time of a call is its whole time):
  capi_all_four        ICPSequence.sensorModel: upload, one kernel, download of normals, observationDirections, noise and keep
  chain_od_on_host     the host shell's chain [ObservationDirection, OrientNormals] WITHOUT a GPU context: the two host loops
  chain_od_on_device   the same chain with a context: one icpmi_sensor_model call
  chain_all_four       [ObservationDirection, OrientNormals, Shadow, SimpleSensorNoise] with a context: one call, one compaction
  chain_one_by_one     the same four filters as four one-filter chains: four calls
The chain rows go through the test hook, which copies the cloud and its descriptors in and out on every call, the same for every row;
the repetitions alternate between the rows.  Not part of bench.py."""
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

S = (0.5, -1.25, 2.0)
OD = "- ObservationDirectionDataPointsFilter: {x: 0.5, y: -1.25, z: 2.0}\n"
ON = "- OrientNormalsDataPointsFilter: {towardCenter: 1}\n"
SH = "- ShadowDataPointsFilter: {eps: 0.1}\n"
SN = "- SimpleSensorNoiseDataPointsFilter: {sensorType: 0}\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import norlab_icp_mapper_amd as amd
    import host_chain_bindings as hcb
    icp = amd.ICPSequence()
    h = icp._h.value
    rng = np.random.default_rng(1)
    cloud = np.concatenate([rng.uniform(-10, 10, (a.n, 3)), np.ones((a.n, 1))], 1).astype(np.float32)
    nrm = rng.normal(size=(a.n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    steps = [("observation_direction",) + S, ("orient_normals", 1), ("shadow", 0.1), ("simple_sensor_noise", 0, 1.0)]
    descs = [("normals", nrm)]

    def one_by_one():
        c, d = cloud, descs
        for y in (OD, ON, SH, SN):
            c, d = hcb.filter_chain_descs(y, c, d, handle=h)

    rows = {
        "capi_all_four": lambda: icp.sensorModel(cloud, steps, normals=nrm),
        "chain_od_on_host": lambda: hcb.filter_chain_descs(OD + ON, cloud, descs, handle=None),
        "chain_od_on_device": lambda: hcb.filter_chain_descs(OD + ON, cloud, descs, handle=h),
        "chain_all_four": lambda: hcb.filter_chain_descs(OD + ON + SH + SN, cloud, descs, handle=h),
        "chain_one_by_one": one_by_one,
    }
    ts = {k: [] for k in rows}
    for r in range(a.warmup + a.reps):
        for k, fn in rows.items():
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                ts[k].append(dt)
    out = []
    for k, v in ts.items():
        r = dict(case=k, n=a.n, ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_p90=float(np.percentile(v, 90)), reps=a.reps)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
