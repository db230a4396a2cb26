#!/usr/bin/env python
"""Measure what float32 arithmetic costs the scheduled VoxelMatcher registration on the room scene, reproduce the float64
prototype's table, and record both in profiles/voxel_pyramid_tolerance.json.  tests/test_gpu_voxel_pyramid.py allows the device four
times the float32 restatement's distance from the float64 loop (tests/voxel_pyramid_reference.py: register(precision=32) fixes one valid
operation order and the device another).  Pure numpy: no GPU, no library -- the tolerance never comes from the device's own output.

    python scripts/voxel_pyramid_tolerance.py [--check]      (--check: measure, compare with the record, write nothing)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voxel_cases as vc  # noqa: E402
import voxel_pyramid_cases as pc  # noqa: E402
import voxel_pyramid_reference as vpr  # noqa: E402
import voxel_reference as vr  # noqa: E402


def measure():
    table, reg = {}, {}
    for sizes in pc.SCHEDULES:
        for k in pc.STARTS:
            _, rd, _, truth = pc.registration_inputs(k)
            r64 = pc.reference_run(k, sizes, 64)
            et, er = vr.centroid_error(r64["T"], truth, rd)
            table[pc.case_key(k, sizes)] = dict(trans_err=et, rot_err=er, report=vpr.report(r64), stops=[lv["stop"] for lv in r64["levels"]])
    for k, sizes in [(k, s) for s in pc.WORKING for k in pc.STARTS]:
        _, rd, _, _ = pc.registration_inputs(k)
        r64, r32 = pc.reference_run(k, sizes, 64), pc.reference_run(k, sizes, 32)
        ok, worst = vpr.margins(r64, r32)
        dt, dr = vc.pose_distance(r32["T"], r64["T"], rd)
        reg[pc.case_key(k, sizes)] = dict(float32_from_float64_trans=dt, float32_from_float64_rot=dr, float32_report=vpr.report(r32),
                                          margins_hold=bool(ok), worst_margin=worst)
    return dict(prototype_table=table, registration_room=reg)


def main():
    got = measure()
    if "--check" in sys.argv:
        with open(pc.TOLERANCE_FILE) as f:
            rec = json.load(f)
        print(json.dumps(dict(measured=got, recorded={k: rec[k] for k in got}), indent=1))
        return
    got["note"] = ("prototype_table: the float64 loop per (start xK, schedule) -- error to the truth at the reading's centroid and the report (iterations, "
                   "pairs of the first and of the last iteration per level); registration_room: the float32 restatement's distance from the float64 "
                   "loop's pose, its report, and whether every Differential decision of the float64 loop lies further from the thresholds than the "
                   "float32 restatement lies from float64 at that check (worst_margin: the smallest such slack in units of the threshold); the GPU "
                   "tests allow the device 4 x the float32 distances")
    with open(pc.TOLERANCE_FILE, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got["registration_room"], indent=1))


if __name__ == "__main__":
    main()
