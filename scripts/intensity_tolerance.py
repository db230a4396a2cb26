#!/usr/bin/env python
"""Measure what float32 arithmetic costs the intensity-aided point-to-plane minimiser -- the map-side gradients, the pair sums, the step
solved from them and the poses a registration converges to -- on the analytic scenes, and record it in profiles/intensity_tolerance.json.
tests/test_gpu_intensity.py allows the device four times these figures: the float32 restatements (tests/intensity_reference.py:
gradient_float32, float32_sums; plane_to_plane_reference.py: float32_step) and the kernels differ by the order of a double sum only.  Pure
numpy: no GPU, no library -- the tolerance never comes from the device's own output.

    python scripts/intensity_tolerance.py [--check]      (--check: measure, compare with the record, write nothing)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import intensity_cases as ic  # noqa: E402
import intensity_reference as ir  # noqa: E402
import plane_to_plane_reference as pp  # noqa: E402
import symmetric_reference as sr  # noqa: E402


def gradient_record():
    """worst distance of the float32 gradients from the float64 ones on the same neighbours: the patches of the operator's tests and the
    maps of the scenes"""
    worst = {}
    for label, m, K in ic.PATCH_CASES:
        cloud, normals, inten = ic.patch(m)
        nbr = ir.self_knn(cloud, K)
        floor = ic.gradient_floor(cloud, inten, nbr)
        worst["patch " + label] = ir.gradient_distance(ir.gradient_float32(cloud, normals, inten, nbr), ir.gradient_reference(cloud, normals, inten, nbr), floor)
    cloud, normals, inten, pick = ic.wrap_case()
    nbr = ir.self_knn(cloud, ic.KNN, pick)
    worst["patch wrap"] = ir.gradient_distance(ir.gradient_float32(cloud, normals, inten, nbr, pick), ir.gradient_reference(cloud, normals, inten, nbr, pick),
                                               ic.gradient_floor(cloud, inten, nbr))
    for name in ic.SCENES:
        sc = ir.scene(name)
        mc = ir.centred(name)[0]
        ir.map_gradients(name, 64)
        floor = ic.gradient_floor(mc, sc["map_intensity"], ir._nbr_cache[(name, ic.KNN)])
        worst[name] = ir.gradient_distance(ir.map_gradients(name, 32), ir.map_gradients(name, 64), floor)
    return worst


def loop_errors(poses):
    return [np.abs(ir.residual_pose(T)[:3, 3]).tolist() for T in poses]


def loop_record(name, iterations, tail_from_stop):
    """the float32 loop with the term next to the float64 one, and the float64 point-to-plane twin: errors against the truth (translation
    per axis in the map frame, m; rotation rad) and the distance between the two precisions.  tail_from_stop None: at the last iteration;
    else the worst over the poses from the Differential checker's stop through tail_from_stop iterations behind it"""
    truth = np.linalg.inv(ir.START)
    p32 = ir.register(name, ic.WEIGHT, 32, iterations)
    p64 = ir.register(name, ic.WEIGHT, 64, iterations)
    twin = ir.register(name, 0.0, 64, ic.TWIN_ITERATIONS)
    if tail_from_stop is None:
        span, stop = [iterations - 1], None
    else:
        stop = sr.differential_stop(p32, **sr.DIFFERENTIAL)
        assert stop is not None and stop + tail_from_stop < iterations
        span = list(range(stop, stop + tail_from_stop + 1))
    gap = [sr.pose_error(p32[i], p64[i]) for i in span]
    err = [sr.pose_error(p32[i], truth) for i in span]
    return dict(iterations=iterations, differential_stop=stop,
                float32_from_float64_translation=max(g[0] for g in gap), float32_from_float64_rotation=max(g[1] for g in gap),
                float32_translation_error=max(e[0] for e in err), float32_rotation_error=max(e[1] for e in err),
                float64_axis_errors=loop_errors(p64), float32_axis_errors=loop_errors(p32),
                twin_iterations=ic.TWIN_ITERATIONS, twin_differential_stop=sr.differential_stop(twin, **sr.DIFFERENTIAL),
                twin_axis_errors=loop_errors(twin)[-1])


def measure():
    sums = {s: 0.0 for s in ic.SCENES}
    step = 0.0
    for name, start, k, chain in ic.SUM_CASES:
        T = ir.centred_pose(ic.STARTS[start], ir.centred(name)[2])
        ref = ir.reference_sums(weight=ic.WEIGHT, **ir.scene_pairs(name, T, k=k, precision=64, **ic.CHAINS[chain]["reference"]))
        f32 = ir.float32_sums(weight=ic.WEIGHT, **ir.scene_pairs(name, T, k=k, precision=32, **ic.CHAINS[chain]["reference"]))
        sums[name] = max(sums[name], pp.rel_distance(f32, ref))
        if name == "room":
            for four in (False, True):
                step = max(step, sr.rel_step(pp.float32_step(f32, four), pp.solve_step(f32, four)))
    return dict(max_rel_gradient=gradient_record(), max_rel_sums=sums, max_rel_step_room=step,
                loops=dict(corridor=loop_record("corridor", ic.CORRIDOR_ITERATIONS, None), room=loop_record("room", ic.ROOM_ITERATIONS, ic.ROOM_TAIL)))


def main():
    got = measure()
    if "--check" in sys.argv:
        with open(ic.TOLERANCE_FILE) as f:
            rec = json.load(f)
        print(json.dumps(dict(measured=got, recorded={k: rec[k] for k in got}), indent=1))
        return
    got["note"] = ("worst intensity_reference.gradient_distance of the float32 gradients from the float64 ones on the same neighbours (per patch of "
                   "tests/intensity_cases.py and per scene map; the floor is intensity_cases.gradient_floor); worst relative distance "
                   "(plane_to_plane_reference.rel_distance) of the float32 pair sums WITH float32 gradients from the float64 reference over "
                   "intensity_cases.SUM_CASES, per scene; worst symmetric_reference.rel_step of the float32 restatement of the solve on room; and "
                   "the float32 registration loop from intensity_reference.START (brute-force k = 1, maxDist 2, TrimmedDist 0.85, weight 0.032, "
                   "gradients from 10 neighbours) next to the float64 one, with the per-axis translation errors of every iteration and of the "
                   "float64 point-to-plane twin after 30: corridor after 8 iterations, room as the worst pose from the Differential checker's "
                   "stop through 4 iterations behind it.  The GPU tests allow the device 4 x these")
    with open(ic.TOLERANCE_FILE, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got, indent=1))


if __name__ == "__main__":
    main()
