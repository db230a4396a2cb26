#!/usr/bin/env python
"""Measure what float32 per-pair arithmetic costs the symmetric point-to-plane pair sums, the step solved from them and the poses a
registration converges to, on the analytic scenes, and record it in profiles/symmetric_tolerance.json.  tests/test_gpu_symmetric.py allows
the device four times these figures: the float32 restatement (tests/symmetric_reference.py: float32_sums; plane_to_plane_reference.py:
float32_step) and the kernels differ by the order of a double sum only.  Pure numpy: no GPU, no library -- the tolerance never comes from
the device's own output.

    python scripts/symmetric_tolerance.py [--check]      (--check: measure, compare with the record, write nothing)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import plane_to_plane_reference as pp  # noqa: E402
import symmetric_cases as sc  # noqa: E402
import symmetric_reference as sr  # noqa: E402


def loop_record(name, iterations, tail_from_stop):
    """the float32 loop of a scene from the "off" start next to the float64 one: its error against the truth (translation m, rotation rad)
    and its distance from the float64 loop's pose.  tail_from_stop None: at the last iteration; else the worst over the poses from the
    Differential checker's stop through tail_from_stop iterations behind it (the loop's float32 noise floor)"""
    off = sc.STARTS["off"]
    truth = np.linalg.inv(off)
    p32 = sr.register(name, off, "symmetric", 32, iterations)
    p64 = sr.register(name, off, "symmetric", 64, iterations)
    if tail_from_stop is None:
        span = [iterations - 1]
        stop = None
    else:
        stop = sr.differential_stop(p32, **sr.DIFFERENTIAL)
        assert stop is not None and stop + tail_from_stop < iterations
        span = list(range(stop, stop + tail_from_stop + 1))
    err = [sr.pose_error(p32[i], truth) for i in span]
    gap = [sr.pose_error(p32[i], p64[i]) for i in span]
    e64 = sr.pose_error(p64[span[-1]], truth)
    return dict(iterations=iterations, differential_stop=stop, float32_translation_error=max(e[0] for e in err),
                float32_rotation_error=max(e[1] for e in err), float32_from_float64_translation=max(g[0] for g in gap),
                float32_from_float64_rotation=max(g[1] for g in gap), float64_translation_error=e64[0], float64_rotation_error=e64[1])


def measure():
    sums = {s: 0.0 for s in sc.SCENES}
    step = 0.0
    for name, start, k, chain in sc.SUM_CASES:
        pairs = sr.scene_pairs(name, sc.STARTS[start], k=k, **sc.CHAINS[chain]["reference"])
        ref = sr.reference_sums(**pairs)
        f32 = sr.float32_sums(**pairs)
        sums[name] = max(sums[name], pp.rel_distance(f32, ref))
        if name == "room":
            for four in (False, True):
                step = max(step, sr.rel_step(pp.float32_step(f32, four), pp.solve_step(f32, four)))
    return dict(max_rel_sums=sums, max_rel_step_room=step,
                loops=dict(ellipsoid=loop_record("ellipsoid", sc.ELLIPSOID_ITERATIONS, None), room=loop_record("room", sc.ROOM_ITERATIONS, sc.ROOM_TAIL)))


def main():
    got = measure()
    if "--check" in sys.argv:
        with open(sc.TOLERANCE_FILE) as f:
            rec = json.load(f)
        print(json.dumps(dict(measured=got, recorded={k: rec[k] for k in got}), indent=1))
        return
    got["note"] = ("worst relative distance (plane_to_plane_reference.rel_distance) of the float32 restatement from the float64 reference over "
                   "the cases of tests/symmetric_cases.py, per scene; worst symmetric_reference.rel_step of the float32 restatement of the solve on "
                   "room; and the float32 registration loop from the off start (brute-force k = 1, maxDist 2, TrimmedDist 0.85) next to the "
                   "float64 one: ellipsoid after 8 iterations, room as the worst pose from the Differential checker's stop through 5 "
                   "iterations behind it.  The GPU tests allow the device 4 x these")
    with open(sc.TOLERANCE_FILE, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got, indent=1))


if __name__ == "__main__":
    main()
