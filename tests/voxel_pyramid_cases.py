"""The cases shared by tests/test_voxel_pyramid_cpu.py, tests/test_gpu_voxel_pyramid.py and scripts/voxel_pyramid_tolerance.py (which
records the float32-against-float64 distances the GPU tests allow four times): the xK starts, the schedules, the issue's prototype table."""
import json
import os

import numpy as np

import localizability_reference as lr
import symmetric_reference as sr
import voxel_pyramid_reference as vpr
import voxel_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "voxel_pyramid_tolerance.json")
F32 = np.float32
STARTS = (1, 2, 3, 4, 6)
# the schedules of the prototype table, in its row order; the two that work from every start
SCHEDULES = ((0.5,), (1.0,), (2.0,), (1.0, 0.5), (4.0, 2.0, 1.0, 0.5), (2.0, 1.0, 0.5))
WORKING = ((1.0, 0.5), (4.0, 2.0, 1.0, 0.5))
# translation error at the reading's centroid, as the issue prints it: schedule -> start -> metres
PROTOTYPE = {
    (0.5,): {1: 4.05e-5, 2: 4.05e-5, 3: 4.2e-2, 4: 0.28, 6: 3.1},
    (1.0,): {1: 2.77e-4, 2: 2.77e-4, 3: 2.77e-4, 4: 2.77e-4, 6: 0.195},
    (2.0,): {1: 2.4e-2, 2: 1.18, 3: 1.18, 4: 1.18, 6: 1.18},
    (1.0, 0.5): {1: 4.05e-5, 2: 4.05e-5, 3: 4.05e-5, 4: 4.05e-5, 6: 4.05e-5},
    (4.0, 2.0, 1.0, 0.5): {1: 4.05e-5, 2: 4.05e-5, 3: 4.05e-5, 4: 4.05e-5, 6: 4.05e-5},
    (2.0, 1.0, 0.5): {1: 4.05e-5, 2: 1.80, 3: 1.80, 4: 1.80, 6: 1.80},
}
# ... and the iterations per level of the four-level run
PROTOTYPE_ITERATIONS = {1: (16, 13, 4, 4), 6: (22, 15, 4, 4)}
FLOOR = 4.05e-5                  # the voxel-mean bias of the 0.5 m level on this scene
# the (start, schedule) pairs the GPU tests register: both working schedules from x1, x3 and x6 (test_voxel_pyramid_cpu.py: their margins hold)
GPU_CASES = [(k, s) for s in WORKING for k in (1, 3, 6)]


def printed(value):
    """half a unit of the last digit the issue prints for `value` (two or three significant digits, read off its text)"""
    text = {4.05e-5: 3, 2.77e-4: 3, 4.2e-2: 2, 0.28: 2, 3.1: 2, 0.195: 3, 2.4e-2: 2, 1.18: 3, 1.80: 3}[value]
    return 0.5 * 10.0 ** (np.floor(np.log10(value)) - (text - 1))


def start_pose(k):
    """xK: the start of 4.20 scaled by K -- rotation vector K (0.02, -0.03, 0.05), translation K (0.3, -0.2, 0.1) m"""
    return lr.make_T(tuple(k * v for v in vr.START_ROT), tuple(k * v for v in vr.START_TRANS))


_inputs = {}


def registration_inputs(k):
    """voxel_cases.registration_inputs with the xK start: (scene, reading, its normals, the pose a registration must answer).  Computed once
    per K; callers must not write into the arrays."""
    if k not in _inputs:
        sc = lr.scene("room")
        M = np.eye(4)
        M[:3, 3] = vr.map_mean(sc["map"]).astype(np.float64)
        Tm = M @ start_pose(k) @ np.linalg.inv(M)
        rd, rn = sr.moved_reading(sc, Tm)
        _inputs[k] = (sc, rd, rn, np.linalg.inv(Tm))
    return _inputs[k]


_runs = {}


def reference_run(k, sizes, precision=64, max_iter=vr.MAX_ITER, differential=vr.DIFFERENTIAL):
    """voxel_pyramid_reference.register on the xK inputs, computed once per argument set (callers must not write into the result)"""
    key = (k, tuple(sizes), precision, max_iter, None if differential is None else tuple(sorted(differential.items())))
    if key not in _runs:
        sc, rd, rn, _ = registration_inputs(k)
        _runs[key] = vpr.register(sc["map"], sc["normals"], rd, rn, sizes, precision, max_iter, differential)
    return _runs[key]


def case_key(k, sizes):
    return f"x{k}/" + ",".join(str(s) for s in sizes)


def recorded():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)
