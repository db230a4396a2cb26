#!/usr/bin/env python
"""Measure what float32 per-pair arithmetic costs the plane-to-plane pair sums and the step solved from them, on the analytic scenes, and
record it in profiles/plane_to_plane_tolerance.json.  tests/test_gpu_plane_to_plane.py allows the device four times these figures: the
float32 restatement (tests/plane_to_plane_reference.py: float32_sums, float32_step) and the kernels differ by the order of a double sum
and of a few float additions only.  Pure numpy: no GPU, no library -- the tolerance never comes from the device's own output.

    python scripts/plane_to_plane_tolerance.py [--check]      (--check: measure, compare with the record, write nothing)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import plane_to_plane_cases as pc  # noqa: E402
import plane_to_plane_reference as pr  # noqa: E402


def measure():
    sums = {s: 0.0 for s in pc.SCENES}
    step = 0.0
    for name, start, k, chain in pc.SUM_CASES:
        pairs = pr.scene_pairs(name, pc.STARTS[start], k=k, **pc.CHAINS[chain]["reference"])
        for eps in pc.EPSILONS:
            ref = pr.reference_sums(eps=eps, **pairs)
            f32 = pr.float32_sums(eps=eps, **pairs)
            sums[name] = max(sums[name], pr.rel_distance(f32, ref))
            if name == "room" and eps == pr.EPS_DEFAULT:
                for four in (False, True):
                    x64 = pr.solve_step(f32, four)
                    x32 = pr.float32_step(f32, four)
                    step = max(step, float(np.linalg.norm(x32 - x64) / np.linalg.norm(x64)))
    return dict(max_rel_sums=sums, max_rel_step_room=step)


def main():
    got = measure()
    if "--check" in sys.argv:
        with open(pc.TOLERANCE_FILE) as f:
            rec = json.load(f)
        print(json.dumps(dict(measured=got, recorded={k: rec[k] for k in got}), indent=1))
        return
    got["note"] = ("worst relative distance (plane_to_plane_reference.rel_distance) of the float32 restatement from the float64 reference over "
                   "the cases of tests/plane_to_plane_cases.py, per scene, and worst |x32 - x64| / |x64| of the float32 restatement of the "
                   "solve on room; the GPU tests allow the device 4 x these")
    with open(pc.TOLERANCE_FILE, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got, indent=1))


if __name__ == "__main__":
    main()
