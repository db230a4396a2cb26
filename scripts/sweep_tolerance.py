#!/usr/bin/env python3
"""Records the figures tests/test_gpu_sweep.py allows four times, in profiles/sweep_tolerance.json:
  sums_float32  the float32 restatement's distance from float64 over the sums cases (CPU; tests/test_sweep_cpu.py writes the same figure)
  pose_margin   on the device: the largest distance (metres; a rotation counts at a 10 m arm) between icpmi_register_sweep's two poses and
                the float64 reference's on the `room` case, from "off" and from the true mid pose
Needs a GPU for the second figure; --cpu records the first alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import sweep_cases as sc  # noqa: E402


def main():
    sc.record(sums_float32=sc.measure_tolerance())
    if "--cpu" in sys.argv:
        return
    import norlab_icp_mapper_amd as amd
    import test_gpu_sweep as t
    by_start = {}
    for start in ("off", "true"):
        res, (Tb, Te, _, _), _ = t._end_to_end(amd, "room", start)
        by_start[start] = max(t.pose_distance(res.T_begin, Tb), t.pose_distance(res.T_end, Te))
    sc.record(pose_margin=max(by_start.values()), pose_margin_by_start=by_start,
              pose_what="max over T_begin, T_end of test_gpu_sweep.pose_distance(device, float64 reference) on the room case, 12 iterations, "
                        "maxDist 2 + TrimmedDist 0.85; measured on an MI355X")
    print(sc.recorded())


if __name__ == "__main__":
    main()
