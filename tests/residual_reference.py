"""numpy restatements of the residual include/icpmi.h (icpmi_residual_error) writes down, and the inputs of tests/test_gpu_residual.py.

An error element is a filled match with weight != 0; its residual r is sqrt(d2) (point-to-point, d2 the matcher's squared distance) or
|(p - q) . n| (point-to-plane; x and y terms only for planar / force2D chains); the answer is the sum of r, with sum r^2, max r, the pair
count and sum w next to it.  residuals_f32 forms r with the device's float32 operations in the device's order (the centred frame,
xf_point's fused multiply-adds, plain multiplies and adds in the dot); residuals_f64 does everything in float64 in the map frame, from
the same float32 inputs.  Sums are float64 on both sides."""
import json
import os

import numpy as np

import covariance_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TOLERANCE_JSON = os.path.join(ROOT, "profiles", "residual_tolerance.json")

M = 5000                               # map points
NS = (1, 63, 64, 65, 257, 1000)        # one lane, a partial wave, the wave edges, a partial workgroup, a strided tail
KS = (1, 6)
MAX_DIST = 0.8                         # the matcher's maxDist: ~1 % of the queries match nothing, most find fewer than six
PLANAR_MAX_DIST = 0.3                  # ... of the flattened scene, whose 5 000 points share one plane
POSE_RV, POSE_T = (0.012, -0.013, 0.018), (0.13, -0.05, 0.02)   # the evaluated correction: near the scene's T_gt, not on it

_scene = None


def scene():
    """fixed-seed box + pillars at a fifth of the benchmark's size: 5 000 map points with normals (~0.7 m apart), 1 000 scan points"""
    global _scene
    if _scene is None:
        from norlab_icp_mapper_amd import synth
        sc = synth.make_scene(m=M, n=max(NS), scale=0.2)
        sc["pose"] = synth.make_T(POSE_RV, POSE_T).astype(F)
        sc["max_dist"] = MAX_DIST
        _scene = sc
    return _scene


def planar_scene():
    """the same clouds flattened to z = 0, normals in the plane (a 2-D mapper's clouds) and a pose about z"""
    from norlab_icp_mapper_amd import synth
    sc = scene()
    mp, scan = sc["map"].copy(), sc["scan"].copy()
    mp[:, 2] = 0; scan[:, 2] = 0
    nm = sc["normals"].copy(); nm[:, 2] = 0
    flat = np.linalg.norm(nm, axis=1) == 0                  # floor / ceiling points: give them an in-plane normal
    nm[flat] = np.array([1, 0, 0], F)
    return {"map": mp, "normals": nm, "scan": scan, "pose": synth.make_T((0, 0, POSE_RV[2]), (POSE_T[0], POSE_T[1], 0)).astype(F),
            "max_dist": PLANAR_MAX_DIST}


# ------------------------------------------------------------------------------------------------------------------ frames
def map_mean64(mp):
    """setMap's mean: sequential float64 sum (tests/test_gpu_covariance.py)"""
    return np.cumsum(mp[:, :3].astype(np.float64), axis=0)[-1] / mp.shape[0]


def centred_map(mp, mean32=None):
    """the map as the library stores it: every point minus the float32 mean, in float32"""
    mean32 = map_mean64(mp).astype(F) if mean32 is None else np.asarray(mean32, F)
    return mp[:, :3] - mean32[None, :]


def centre_reading(reading, mean32):
    rc = reading.copy()
    rc[:, :3] = reading[:, :3] - np.asarray(mean32, F)[None, :]
    return rc


def centred_pose(T, mean32):
    """the pose the matcher moves the centred reading by: [R | t + R mu - mu], the translation in float64 in the library's order, rounded
    to float32 (T: 4 x 4 row-major float32, mu: the library's float32 map mean)"""
    T = np.asarray(T, F)
    A = T.astype(np.float64); mu = np.asarray(mean32, F).astype(np.float64)
    out = np.eye(4, dtype=F)
    out[:3, :3] = T[:3, :3]
    for r in range(3):
        out[r, 3] = F((A[r, 3] + ((A[r, 0] * mu[0] + A[r, 1] * mu[1]) + A[r, 2] * mu[2])) - mu[r])
    return out


def sqdist3_f32(p, q):
    """the matcher's d2: fma(dz, dz, fma(dy, dy, dx dx)) in float32 (products of float32 are exact in float64)"""
    d = (p.astype(F) - q.astype(F)).astype(np.float64)
    acc = (d[:, 0] * d[:, 0]).astype(F)
    acc = (d[:, 1] * d[:, 1] + acc.astype(np.float64)).astype(F)
    return (d[:, 2] * d[:, 2] + acc.astype(np.float64)).astype(F)


# ------------------------------------------------------------------------------------------------------------------ the restatements
def residuals_f32(kind, p, q, n, d2, planar=False):
    """per pair, float32: p the moved reading points (xf_point), q the matched centred map points, n their normals, d2 the matcher's"""
    if kind == 1:
        return np.sqrt(np.asarray(d2, F))
    p, q, n = (np.asarray(v, F) for v in (p, q, n))
    d = p - q
    dot = d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]
    if not planar:
        dot = dot + d[:, 2] * n[:, 2]
    return np.abs(dot).astype(F)


def residuals_f64(kind, reading, T, qmap, n, planar=False):
    """end to end in float64, map frame: reading rows (float32 data) moved by T, the matched map points and normals as given"""
    T = np.asarray(T, np.float64)
    p = reading[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d = p - qmap[:, :3].astype(np.float64)
    if kind == 1:
        return np.sqrt((d * d).sum(1))
    prod = d * np.asarray(n, np.float64)
    return np.abs(prod[:, :2].sum(1) if planar else prod.sum(1))


def summarise(r, w, filled=None):
    """the reduction over the error elements (filled and w != 0): float64 sums, float32 max; a soft weight counts as one pair"""
    r = np.asarray(r); w = np.asarray(w, F)
    el = (w != 0) if filled is None else (np.asarray(filled, bool) & (w != 0))
    re = r[el]
    return {"sum_abs": float(re.astype(np.float64).sum()), "sum_sq": float((re.astype(np.float64) ** 2).sum()),
            "max_abs": F(re.max()) if re.size else F(0), "pairs": int(el.sum()), "weight_sum": float(w[el].astype(np.float64).sum())}


# ------------------------------------------------------------------------------------------------------------------ exact neighbours
def brute_knn(q, ref, k, max_dist):
    """float64 exact neighbours of the rows of q among ref: (ids (n, k) ascending by distance, -1 where unfilled; d2 float64, inf there;
    gap: second-nearest minus nearest distance of every query)"""
    q = np.asarray(q, np.float64); ref = np.asarray(ref, np.float64)
    d2 = ((q[:, None, :] - ref[None, :, :]) ** 2).sum(2)
    kk = max(k, 2)
    ids = np.argsort(d2, axis=1, kind="stable")[:, :kk]
    dd = np.take_along_axis(d2, ids, 1)
    gap = np.sqrt(dd[:, 1]) - np.sqrt(dd[:, 0])
    ids, dd = ids[:, :k].copy(), dd[:, :k].copy()
    out = dd > float(max_dist) ** 2
    ids[out] = -1; dd[out] = np.inf
    return ids, dd, gap


def cpu_case(sc, n, k, kind, planar=False):
    """the MaxDist pair set of reading[:n] under the scene's pose from exact neighbours, both restatements over it:
    (summary f32, summary f64, pairs)"""
    mp, nm, reading, T = sc["map"], sc["normals"], sc["scan"][:n], sc["pose"]
    mean32 = map_mean64(mp).astype(F)
    moved64 = reading[:, :3].astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
    ids, _, _ = brute_knn(moved64, mp[:, :3], k, sc["max_dist"])
    qi, qj = np.nonzero(ids >= 0)
    s = ids[qi, qj]
    p = cr.fma_transform(centred_pose(T, mean32), centre_reading(reading, mean32))[qi]
    q = centred_map(mp, mean32)[s]
    d2 = sqdist3_f32(p, q)
    w = np.ones(s.shape[0], F)
    a = summarise(residuals_f32(kind, p, q, nm[s], d2, planar), w)
    b = summarise(residuals_f64(kind, reading[qi], T, mp[s], nm[s], planar), w)
    return a, b, s.shape[0]


def rel_dev(a, b):
    """(a sum that is exactly 0 in float64 -- one pair lying in its plane -- is exactly 0 in float32 too: nothing to divide by)"""
    dev = 0.0
    for key in ("sum_abs", "sum_sq"):
        if b[key] == 0:
            assert a[key] == 0
        else:
            dev = max(dev, abs(a[key] - b[key]) / b[key])
    return dev


def measure_tolerance():
    """largest relative deviation of the float32 restatement's sums from the float64 ones over the GPU tests' scenes, by kind"""
    worst = {"1": 0.0, "1_planar": 0.0, "2": 0.0, "2_force2d": 0.0, "2_planar": 0.0}
    for n in NS:
        for k in KS:
            for name, sc, kind, planar in (("1", scene(), 1, False), ("1_planar", planar_scene(), 1, False), ("2", scene(), 2, False),
                                            ("2_force2d", scene(), 2, True), ("2_planar", planar_scene(), 2, True)):
                a, b, pairs = cpu_case(sc, n, k, kind, planar)
                if pairs:
                    worst[name] = max(worst[name], rel_dev(a, b))
    return worst


def device_bound(name):
    """what the GPU tests allow against float64: four times the measured figure of that kind (profiles/residual_tolerance.json)"""
    with open(TOLERANCE_JSON) as f:
        return 4.0 * float(json.load(f)["by_kind"][name])
