"""The cases shared by tests/test_voxel_cpu.py, tests/test_gpu_voxel.py and scripts/voxel_tolerance.py (which records the
float32-against-float64 distances the GPU tests allow four times)."""
import json
import os

import numpy as np

import localizability_reference as lr
import plane_to_plane_reference as pr
import symmetric_reference as sr
import voxel_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "voxel_tolerance.json")
F32 = np.float32
SCENES = ("room", "corridor")
POSES = ("true", "start")
SIZES = (0.5, 1.0)
VARIANTS = ("full", "n1", "zero_normals")       # the whole reading; its first point alone; the reading with all-zero normals
SUM_CASES = [(name, pose, size, "full") for name in SCENES for pose in POSES for size in SIZES] + \
            [("room", "start", 1.0, "n1"), ("room", "start", 1.0, "zero_normals")]
REG_SIZES = SIZES
MIN_PLANE_TO_PLANE = 3
# the issue's prototype on the room scene from the start pose (error at the reading's centroid): size -> (translation, rotation, iterations, pairs
# of the first iteration); the errors quoted to two digits, so reproduced means within half a unit of the second digit of the smallest (2.1 %); the counts exactly
PROTOTYPE = {0.5: (4.1e-5, 1.4e-5, 6, 877), 1.0: (2.8e-4, 2.1e-5, 5, 1902), 2.0: (2.4e-2, None, None, None)}
PROTOTYPE_REL = 0.021


def case_key(name, pose, size, variant="full"):
    return f"{name}/{pose}/{size}/{variant}"


def reading_of(name, variant):
    sc = lr.scene(name)
    rd, rn = sc["reading"], sc["reading_normals"]
    if variant == "n1":
        rd, rn = rd[:1], rn[:1]
    elif variant == "zero_normals":
        rn = np.zeros_like(rn)
    return rd, rn


def sum_inputs(name, pose, size, variant="full", mean=None):
    """what one sums case is evaluated on: dict(T float32, rc: the centred reading, rn, p, npr: the points and normals under T as the device
    forms them, tab: the float64 table of the centred map, vox: the voxel of every point by the float32 key)"""
    sc = lr.scene(name)
    rd, rn = reading_of(name, variant)
    mean = vr.map_mean(sc["map"]) if mean is None else mean
    T = vr.POSES[pose].astype(F32)
    mc, rc = vr.centred(sc["map"], mean), vr.centred(rd, mean)
    tab = vr.table(mc, sc["normals"], size)
    p, npr = pr.xf_points(T, rc), pr.rot_normals(T, rn)
    return dict(T=T, rc=rc, rn=rn, p=p, npr=npr, tab=tab, vox=vr.lookup(tab, p), mc=mc)


def registration_inputs():
    """the room scene's reading moved off the truth by the start pose, taken in the map's centred frame as the prototype took it (the first
    iteration's points are then START (x - mean), those of the sums cases): registering it must answer the inverse"""
    sc = lr.scene("room")
    M = np.eye(4)
    M[:3, 3] = vr.map_mean(sc["map"]).astype(np.float64)
    Tm = M @ vr.POSES["start"] @ np.linalg.inv(M)
    rd, rn = sr.moved_reading(sc, Tm)
    return sc, rd, rn, np.linalg.inv(Tm)


def pose_distance(T, T_ref, reading4):
    """(translation at the reading's centroid, rotation) between two poses"""
    return vr.centroid_error(T, T_ref, reading4)


def recorded():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)
