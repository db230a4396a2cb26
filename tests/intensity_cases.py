"""The cases shared by tests/test_intensity_cpu.py, tests/test_gpu_intensity.py and scripts/intensity_tolerance.py (which records the
float32-against-float64 distances the GPU tests allow four times)."""
import json
import os

import numpy as np

import intensity_reference as ir
import plane_to_plane_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "intensity_tolerance.json")
F = np.float32
SCENES = ir.SCENES
STARTS = {"true": np.eye(4), "start": ir.START}
MAX_DIST = pc.MAX_DIST
MIN_POINT_TO_PLANE = 2
CHAINS = pc.CHAINS                      # maxdist, trimmed (the fused selection), cauchy (EXT)
SUM_CASES = [(name, start, k, chain) for name in SCENES for start in STARTS for k in (1, 3) for chain in CHAINS]
WEIGHT = ir.WEIGHT_DEFAULT
KNN = ir.KNN_DEFAULT
CORRIDOR_ITERATIONS = 8                 # the fixed-count registration on `corridor`
TWIN_ITERATIONS = 30                    # ... and its point-to-plane twin
ROOM_ITERATIONS = 12                    # the reference loops on `room` (the Differential checker stops them well before)
ROOM_TAIL = 4                           # poses behind the Differential stop whose worst error is recorded (the float32 loop's noise floor)
ALONG_AXIS_BOUND = 1e-2                 # m: ten times the error seen when the feature was proposed, a thirtieth of the start
TWIN_STAYS_ABOVE = 0.25                 # m
# Floor under the recorded float32-against-float64 ROTATION distance of a loop: a float32 pose holds the sine of its rotation angle to
# eps_f of its size, so two float32 poses that round the same rotation differ by up to eps_f times the angle -- the start's 0.03 rad here,
# which every registration has to undo.  The two CPU loops happen to differ by less.
ROTATION_FLOOR = 1.1920928955078125e-07 * 0.03      # rad

# ---- the gradient operator's cases: a patch of a tilted plane with a linear field I = a . x + c, whose gradient is the tangential part of a
PATCH_NORMAL = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
PATCH_A = np.array([0.7, -0.4, 0.2])
PATCH_C = 0.3
GRID_WRAP = 2048 * 256 + 1              # one point past the gradient kernel's grid (pointops.hip: intensity_grid)
# (label, points, K)
PATCH_CASES = [("m=K+1", 11, 10), ("m=K", 10, 10), ("K=1", 64, 1), ("K=31", 300, 31), ("257", 257, 10), ("4097", 4097, 10)]


def patch(m, seed=7, half=1.0):
    """m random points of the plane through (0.5, -0.25, 1) with normal PATCH_NORMAL, within `half` of it along both tangents: cloud (m, 4)
    float32, normals (m, 3) float32 (the exact one, every row), intensity (m,) float32 of the linear field at the ROUNDED points"""
    rng = np.random.default_rng(seed)
    t1 = np.cross(PATCH_NORMAL, [1.0, 0.0, 0.0]); t1 /= np.linalg.norm(t1)
    t2 = np.cross(PATCH_NORMAL, t1)
    uv = rng.uniform(-half, half, (m, 2))
    xyz = (np.array([0.5, -0.25, 1.0]) + uv[:, :1] * t1 + uv[:, 1:] * t2).astype(F)
    cloud = np.concatenate([xyz, np.ones((m, 1), F)], 1)
    normals = np.repeat(PATCH_NORMAL[None, :], m, 0).astype(F)
    inten = (xyz.astype(np.float64) @ PATCH_A + PATCH_C).astype(F)
    return cloud, normals, inten


def wrap_case():
    """the patch of GRID_WRAP points (80 m wide: the neighbour spacing of the scenes) and the points its test looks at: every 4099th and the last"""
    cloud, normals, inten = patch(GRID_WRAP, half=40.0)
    return cloud, normals, inten, np.concatenate([np.arange(0, GRID_WRAP - 1, 4099), [GRID_WRAP - 1]])


def patch_gradient():
    """the tangential part of PATCH_A: what every point of a patch answers, whatever its neighbours"""
    return PATCH_A - PATCH_NORMAL * (PATCH_A @ PATCH_NORMAL)


def gradient_floor(cloud, inten, nbr):
    """the absolute floor under a gradient's relative distance: the rounding of an intensity (eps_f times the field's amplitude) over the
    spacing of the neighbours (the median distance to the nearest other point)"""
    x = np.asarray(cloud, np.float64)[:, :3]
    nbr = np.asarray(nbr)
    if x.shape[0] < 2 or nbr.shape[1] < 2:
        return ir.lr.EPS_F
    own, first = nbr[:, 0], nbr[:, 1]
    ok = (first >= 0) & (own >= 0)
    h = float(np.median(np.linalg.norm(x[first[ok]] - x[own[ok]], axis=1))) if ok.any() else 1.0
    amp = float(np.nanmax(np.abs(np.asarray(inten, np.float64))))
    return ir.lr.EPS_F * amp / max(h, 1e-12)


def recorded():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)
