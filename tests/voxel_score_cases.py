"""The cases shared by tests/test_voxel_score_cpu.py, tests/test_gpu_voxel_score.py and scripts/voxel_score_tolerance.py (which records the
float32-against-float64 distances the GPU test allows four times, and the floor it derives from expf's documented error)."""
import json
import os

import numpy as np

import localizability_reference as lr
import voxel_reference as vr
import voxel_score_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "voxel_score_tolerance.json")
F32 = np.float32
SCENE = "room"
SIZES = (0.5, 1.0)
SCHEDULE = (1.0, 0.5)
SLICE, TILE = 1024, 8                   # icpmi_voxel_score_shape (the GPU test checks that the library says the same)
N_VALUES = (1, 63, 64, 65, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 2000)
# the poses of the reference cases, in the centred frame: the truth, the start of the voxel tests, a half turn of yaw with 5 m of translation
POSES = {"identity": np.eye(4), "start": vr.POSES["start"], "half_turn": lr.make_T((0.0, 0.0, np.pi), (3.0, -4.0, 0.0))}
POSE_COUNTS = (1, 2, 15, 16, 17, TILE - 1, TILE, TILE + 1, 65)
# float32 roundoff, and the documented bound of the device's expf (ROCm's HIP math API lists expf with a maximum error of 1 ULP): every
# term of the likelihood is positive, so the sum is off by at most 1 ULP = 2 u of itself -- the restatement's own exp is part of the
# recorded distance, not of this
U = 2.0 ** -24
EXPF_ULP_BOUND = 1.0
LIKELIHOOD_FLOOR_UNITS = 2.0 * EXPF_ULP_BOUND
MARGIN = 4.0
# the issue's prototype: candidates G = make_T((0, 0, a), (x, y, 0)), the scored pose G K; likelihood / n of the best and the second best
GRID_YAW = (-0.4, -0.2, 0.0, 0.2, 0.4)
GRID_XY = (-3.0, -1.5, 0.0, 1.5, 3.0)
CENTRE = 62
PROTOTYPE = {(0.5, "identity"): (0.985, 0.860), (0.5, "start"): (0.193, 0.180), (1.0, "identity"): (0.950, 0.862), (1.0, "start"): (0.384, 0.358),
             (2.0, "identity"): (0.756, 0.700), (2.0, "start"): (0.478, 0.435)}
RUNNER_UP_MAX = 0.95


def grid():
    """the 125 candidates, yaw outermost, then x, then y: (125, 4, 4) float64; index CENTRE is the identity"""
    return np.stack([lr.make_T((0.0, 0.0, a), (x, y, 0.0)) for a in GRID_YAW for x in GRID_XY for y in GRID_XY])


def case_key(size, pose, n):
    return f"{size}/{pose}/{n}"


_cache = {}


def inputs(mean=None):
    """the room scene in the handle's centred frame: dict(sc, mean, mc, rc, rn, tab: {size: float64 table})"""
    key = None if mean is None else tuple(np.asarray(mean, F32).tolist())
    if key not in _cache:
        sc = lr.scene(SCENE)
        m = vr.map_mean(sc["map"]) if mean is None else np.asarray(mean, F32)
        mc, rc = vr.centred(sc["map"], m), vr.centred(sc["reading"], m)
        _cache[key] = dict(sc=sc, mean=m, mc=mc, rc=rc, rn=sc["reading_normals"], tab={s: vr.table(mc, sc["normals"], s) for s in (0.5, 1.0, 2.0)})
    return _cache[key]


def map_frame(Tc, mean):
    """the float32 map-frame correction handed to the library for the centred-frame pose Tc, and the centred pose the library forms of it"""
    T = sr.map_frame_pose(Tc, mean).astype(F32)
    return T, sr.centred_pose(T, mean)


def references(size, pose, n, mean=None):
    """(float64 score, float32 restatement) of the first n reading points under POSES[pose], as the library sees the pose"""
    c = inputs(mean)
    _, Tc = map_frame(POSES[pose], c["mean"])
    tab = c["tab"][size]
    r32 = sr.score32(Tc, c["rc"][:n], c["rn"][:n], vr.table_f32(tab))
    r64 = sr.score64(Tc, c["rc"][:n], c["rn"][:n], tab, vox=r32["vox"])
    return r64, r32


def ranking_case(size, kname):
    """likelihood / n of the 125 candidates G K in float64: (125,)"""
    c = inputs()
    K = np.eye(4) if kname == "identity" else vr.POSES[kname]
    n = c["rc"].shape[0]
    return np.array([sr.score64((G @ K).astype(F32), c["rc"], c["rn"], c["tab"][size])["likelihood"] / n for G in grid()])


def recorded():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)
