#!/usr/bin/env python
"""Measure what float32 arithmetic costs VoxelMatcher -- the table, the pair sums, the step solved from them and the whole registration --
on the analytic scenes, reproduce the figures of the float64 prototype the feature rests on, and record all of it in
profiles/voxel_tolerance.json.  tests/test_gpu_voxel.py allows the device four times the float32 figures: the float32 restatement
(tests/voxel_reference.py: table_f32, float32_sums, register(precision=32)) fixes one valid operation order and the device another.
Pure numpy: no GPU, no library -- the tolerance never comes from the device's own output.

    python scripts/voxel_tolerance.py [--check]      (--check: measure, compare with the record, write nothing)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import localizability_reference as lr  # noqa: E402
import plane_to_plane_reference as pr  # noqa: E402
import voxel_cases as vc  # noqa: E402
import voxel_reference as vr  # noqa: E402


def measure():
    sums, step = {}, 0.0
    for name, pose, size, variant in vc.SUM_CASES:
        c = vc.sum_inputs(name, pose, size, variant)
        ref = vr.reference_sums(c["p"], c["npr"], c["vox"], c["tab"])
        f32 = vr.float32_sums(c["p"], c["npr"], c["vox"], vr.table_f32(c["tab"]))
        assert f32[28] == ref[28] and ref[28] > 0
        sums[vc.case_key(name, pose, size, variant)] = pr.rel_distance(f32, ref)
        if variant == "full":
            x64, x32 = pr.solve_step(f32), pr.float32_step(f32)
            step = max(step, float(np.linalg.norm(x32 - x64) / np.linalg.norm(x64)))
    sc, rd, rn, truth = vc.registration_inputs()
    reg = {}
    for size in (0.5, 1.0, 2.0):
        r64 = vr.register(sc["map"], sc["normals"], rd, rn, size, 64)
        r32 = vr.register(sc["map"], sc["normals"], rd, rn, size, 32)
        et, er = vr.centroid_error(r64["T"], truth, rd)
        dt, dr = vc.pose_distance(r32["T"], r64["T"], rd)
        reg[str(size)] = dict(float64_trans_err=et, float64_rot_err=er, float64_iterations=r64["iterations"], float64_pairs_first=r64["pairs"][0],
                              float32_iterations=r32["iterations"], float32_from_float64_trans=dt, float32_from_float64_rot=dr)
    # the nearest-neighbour plane-to-plane step on the same start (the prototype's last row): brute-force k = 1, maxDist 2, float64
    import symmetric_reference as sr
    T = np.eye(4)
    mean = vr.map_mean(sc["map"])
    mc, rc = vr.centred(sc["map"], mean), vr.centred(rd, mean)
    poses = []
    for _ in range(vr.MAX_ITER):
        p = rc[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        npr = rn.astype(np.float64) @ T[:3, :3].T
        idx, d2 = sr.brute_nn(p, mc, 1)
        w = (d2 <= 4.0).astype(np.float64).ravel()
        x = pr.solve_step(pr.reference_sums(p, mc[idx.ravel(), :3], sc["normals"][idx.ravel()], npr, w=w))
        T = lr.make_T(x[:3], x[3:]) @ T
        poses.append(T.copy())
        if sr.differential_stop(poses, **vr.DIFFERENTIAL) is not None:
            break
    Tw = T.copy()
    m64 = mean.astype(np.float64)
    Tw[:3, 3] = Tw[:3, 3] + m64 - Tw[:3, :3] @ m64
    nn = dict(trans_err=vr.centroid_error(Tw, truth, rd)[0], iterations=len(poses))
    return dict(rel_sums=sums, max_rel_step=step, registration_room=reg, nearest_neighbour_plane_to_plane_room=nn)


def main():
    got = measure()
    if "--check" in sys.argv:
        with open(vc.TOLERANCE_FILE) as f:
            rec = json.load(f)
        print(json.dumps(dict(measured=got, recorded={k: rec[k] for k in got}), indent=1))
        return
    got["note"] = ("rel_sums: plane_to_plane_reference.rel_distance of the float32 restatement (float32 table, float32 per-pair terms) from the float64 "
                   "reference on the same (point, voxel) pairs, per case of tests/voxel_cases.py; max_rel_step: worst |x32 - x64| / |x64| of the float32 "
                   "restatement of the solve; registration_room: the float64 loop's error to the truth at the reading's centroid (the prototype's "
                   "figures) and the float32 loop's distance from the float64 loop's pose; the GPU tests allow the device 4 x the float32 figures")
    with open(vc.TOLERANCE_FILE, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got, indent=1))


if __name__ == "__main__":
    main()
