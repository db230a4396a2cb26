"""The device side of the localizability tests: one minimisation step on an analytic scene through icpmi_minimize_step, compared with the
float64 restatement evaluated on the sums the same call returned.  Shared by tests/test_gpu_localizability.py and
scripts/localizability_tolerance.py (which records the measured deviation the test allows four times)."""
import json
import os

import numpy as np

import localizability_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "localizability_tolerance.json")
F = np.float32
THR = float(F(lr.THRESHOLD))
STARTS = {"true": np.eye(4), "off": lr.make_T((0.02, -0.03, 0.035), (0.2, -0.2, 0.1))}   # |rot| = 0.05 rad, |t| = 0.3 m
STEP_CASES = [(name, four, start) for name in lr.SCENES for four in (0, 1) for start in ("true", "off")]


def centred(cloud, mean):
    """the reading as the registration centres it: float32 difference with the handle's float32 mean"""
    out = np.array(cloud, dtype=F)
    out[:, :3] = cloud[:, :3] - np.asarray(mean, F)[None, :]
    return out


def step_case(pkg, name, four_dof, start, threshold=THR):
    sc = lr.scene(name)
    icp = pkg.ICPSequence(knn=1, max_dist=2.0, outliers=[], force_4dof=int(four_dof), degeneracy_threshold=threshold)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        rc = centred(sc["reading"], icp.getMapMean())
        T_iter = STARTS[start].astype(F)
        T_step, sums = icp.minimizeStep(rc, T_iter)
        loc = icp.localizability()
    finally:
        icp.close()
    A, b, W, pairs = lr.unpack_sums(sums)
    c0, L = lr.reading_stats(rc)
    c = lr.pivot(T_iter, c0)
    ref = lr.localizability_reference(A, b, W, c, L, abs(threshold), bool(four_dof))
    x_dev = lr.step_from_T(T_step)
    y_dev = lr.scaled_step(x_dev, c, L)
    d, ny = np.linalg.norm(y_dev - ref["y"]), np.linalg.norm(ref["y"])
    rel = d / ny if ny > 0 else (0.0 if d == 0 else np.inf)
    return dict(ref=ref, loc=loc, x_dev=x_dev, y_dev=y_dev, rel_x=float(rel), c=c, L=L, W=W, pairs=pairs, mean=None)


def recorded_tolerance():
    with open(TOLERANCE_FILE) as f:
        return float(json.load(f)["max_rel_x"])
