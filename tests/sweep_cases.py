"""The cases shared by tests/test_sweep_cpu.py and tests/test_gpu_sweep.py: the skewed `room` scan, the chains, the sums cases, and the
recorded float32-against-float64 distances (profiles/sweep_tolerance.json) the GPU tests allow four times."""
import json
import os

import numpy as np
from scipy.spatial import cKDTree

import covariance_reference as cr
import deskew_reference as dr
import localizability_cases as lc
import localizability_reference as lr
import residual_reference as rr
import sweep_reference as sr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCE_FILE = os.path.join(ROOT, "profiles", "sweep_tolerance.json")
STARTS = lc.STARTS                               # "true": identity, "off": 0.05 rad / 0.3 m
SENSOR = np.array([0.3, 1.0, 1.5])               # where the sensor sits in the room; a point's time is its azimuth seen from there
MOTION_ROT, MOTION_TRANS = (0.0, 0.0, 0.06), (0.15, 0.05, 0.0)      # the motion over the sweep, split evenly about the mid pose (identity)
MAX_DIST, TRIM_RATIO, ITERATIONS = 2.0, 0.85, 12
NS = (1, 63, 64, 65, 257, 1000)
KS = (1, 3)
OUT_MAXDIST, OUT_MEDIAN, OUT_TRIMMED = 1, 3, 4
CHAINS = {"none": [], "maxdist+trimmed": [(OUT_MAXDIST, 1.5), (OUT_TRIMMED, TRIM_RATIO)], "median": [(OUT_MEDIAN, 3.0)]}
SUM_CASES = [(n, k, chain) for n in NS for k in KS for chain in CHAINS]
# the distinct poses of the skewed sums cases: off the truth by a few centimetres and milliradians, begin and end differently
SUMS_T_BEGIN = lr.make_T((0.004, -0.006, -0.025), (-0.05, -0.04, 0.02))
SUMS_T_END = lr.make_T((-0.005, 0.003, 0.035), (0.09, 0.01, -0.015))

_room = None


def room():
    """the `room` scene seen by a moving sensor: map, normals, scan (N, 4) float32 in the sensor's moving frame, t_rel (N,) float32 in
    UNIT_S, alpha, the true poses at sweep begin and end, and the points' true places in the map"""
    global _room
    if _room is None:
        sc = lr.scene("room")
        P = sc["reading"][:, :3].astype(np.float64)
        az = np.arctan2(P[:, 1] - SENSOR[1], P[:, 0] - SENSOR[0])
        t_rel = (((az + np.pi) / (2 * np.pi)) * (sr.END_S - sr.BEGIN_S) / sr.UNIT_S).astype(F)
        alpha = sr.alpha_of(t_rel)
        Tb = lr.make_T(-0.5 * np.array(MOTION_ROT), -0.5 * np.array(MOTION_TRANS))
        Te = lr.make_T(0.5 * np.array(MOTION_ROT), 0.5 * np.array(MOTION_TRANS))
        R, p = dr.pose_at([0.0, 1.0], np.stack([sr.pose7(Tb), sr.pose7(Te)]), alpha.astype(np.float64))
        scan = np.ones((P.shape[0], 4), F)
        scan[:, :3] = R.inv().apply(P - p).astype(F)
        truth = sr.world_points(scan, alpha, Tb, Te)          # (of the float32 scan: what a perfect estimate reproduces)
        _room = dict(map=sc["map"], normals=sc["normals"], scan=scan, t_rel=t_rel, alpha=alpha, T_begin=Tb, T_end=Te, truth=truth,
                     mean=rr.map_mean64(sc["map"]).astype(F))
        for a in _room.values():
            a.setflags(write=False)
    return _room


def static_room():
    """the same room scanned without motion: the reading as it is, the same point times"""
    c = room()
    sc = lr.scene("room")
    return dict(c, scan=sc["reading"], truth=sc["reading"][:, :3].astype(np.float64), T_begin=np.eye(4), T_end=np.eye(4))


def chain_weights(chain, d2):
    """the chain's weights over float32 d2 (+inf = no match), the filters of CHAINS in the library's float32 comparisons"""
    d2 = np.asarray(d2, F)
    w = np.isfinite(d2).astype(F)
    import match_reference as mr
    for typ, prm in CHAINS[chain]:
        if typ == OUT_MAXDIST:
            w = w * (d2 <= F(prm) * F(prm))
        elif typ == OUT_TRIMMED:
            w = w * (d2 <= F(mr.trimmed_quantile(d2, prm)))
        else:
            w = w * (d2 <= F(F(prm) * F(mr.trimmed_quantile(d2, 0.5))))
    return w


def float32_pairs(scan, t_rel, Tb, Te, mean32):
    """the reading's points as the device forms them: the float32 deskew under the table of (Tb, Te), centred, under the centred end pose"""
    poses = np.stack([sr.pose7(np.asarray(Tb, F)), sr.pose7(np.asarray(Te, F))])
    work, _, bad = dr.deskew32(scan, t_rel, sr.STAMPS, dr.table32(sr.STAMPS, poses, ref=sr.END_S), unit=sr.UNIT_S, extrapolate=True)
    assert not bad.any()
    return cr.fma_transform(rr.centred_pose(np.asarray(Te, F), mean32), rr.centre_reading(work, mean32)), work


def cpu_sums_case(n, k, chain, alpha_mode="skewed"):
    """one sums case with exact neighbours: (float32 restatement, float64 reference, the scale of g)"""
    c = room()
    scan, t_rel = c["scan"][:n], c["t_rel"][:n]
    Tb, Te = SUMS_T_BEGIN.astype(F), SUMS_T_END.astype(F)
    alpha = sr.alpha_of(t_rel)
    mean32 = c["mean"]
    p32, _ = float32_pairs(scan, t_rel, Tb, Te, mean32)
    P64 = sr.world_points(scan, alpha, Tb.astype(np.float64), Te.astype(np.float64))
    mp64 = c["map"][:, :3].astype(np.float64)
    dist, ids = cKDTree(mp64).query(P64, k=k, distance_upper_bound=MAX_DIST)
    dist, ids = dist.reshape(n, k), ids.reshape(n, k)
    qi, qj = np.nonzero(np.isfinite(dist))
    s = ids[qi, qj]
    mapc = rr.centred_map(c["map"], mean32)
    d2 = np.full((n, k), np.inf, F)
    d2[qi, qj] = rr.sqdist3_f32(p32[qi], mapc[s])
    w = chain_weights(chain, d2)[qi, qj]
    a, _ = sr.sums32(p32[qi], mapc[s], c["normals"][s], w, alpha[qi])
    mu = mean32.astype(np.float64)
    b, gs = sr.sums64(P64[qi] - mu, mp64[s] - mu, c["normals"][s], w, alpha[qi])
    return a, b, gs


def measure_tolerance():
    """the largest deviation (sweep_reference.deviation) of the float32 restatement from float64 over the sums cases"""
    worst = 0.0
    for n, k, chain in SUM_CASES:
        a, b, gs = cpu_sums_case(n, k, chain)
        if b[sr.PAIRS] > 0:
            worst = max(worst, sr.deviation(a, b, gs))
    return worst


def recorded():
    with open(TOLERANCE_FILE) as f:
        return json.load(f)


def record(**kw):
    """merge figures into profiles/sweep_tolerance.json (the CPU test writes `sums_float32`, the GPU tests `pose_margin`)"""
    data = recorded() if os.path.exists(TOLERANCE_FILE) else {}
    data.update(kw)
    with open(TOLERANCE_FILE, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
