"""The cases of tests/test_gpu_dynamic_points.py and tests/test_dynamic_points_cpu.py: inputs of DynamicPointsMapperModule built to reach the
corners of the device's angular bucket grid (csrc/dynpts.hip) -- both scan routes, grids smaller than the 5 x 5 block, the poles, the
azimuth seam, angles on bucket edges, dense buckets, exact ties, wave-run shapes, the decision boundaries of the update.

Clouds are built in the SENSOR frame from chosen (elevation, azimuth, range) triples and moved into the map frame by the case's pose;
where exact angle bits matter (ties, on-edge angles, the poles, the seam) the pose is the identity.  No point sits at the sensor's origin.

    case(cid) -> (to_sensor f32 4x4 row-major, beams f32 n x 4, map f32 m x 4, normals f32 m x 3, prob0 f32 m, params, flags)

flags["float64"]: the float64 bar (tests/golden/make_recalled.py::dynamic_points_update, TOL below) applies; the other entries of flags are
named index arrays of the queries a test looks at."""
import functools
import math

import numpy as np

F32 = np.float32
KEYS = ("threshold_dynamic", "alpha", "beta", "beam_half_angle", "epsilon_a", "epsilon_d", "sensor_max_range")
PARAMS = dict(threshold_dynamic=0.6, alpha=0.8, beta=0.99, beam_half_angle=0.01, epsilon_a=0.01, epsilon_d=0.01, sensor_max_range=100.0)
RATIOS = np.array([0.5, 0.8, 0.97, 0.995, 1.005, 1.03, 1.3])     # map range / beam range (make_recalled.py::dynamic_vectors)
PROBS = np.array([0.1, 0.3, 0.55, 0.7, 0.9])
RINGS = 2                          # DYN_RINGS: buckets per search radius
HALF_PI32, PI32, TWO_PI32 = F32(1.5707963267949), F32(3.14159265358979), F32(6.28318530717959)   # the kernel's literals
SIDE_SCAN_MAX_CELLS = 8192 * 2048  # device_scan_side_ok: the two-kernel scan takes tables up to here
MAX_CELLS = 1 << 28                # beyond: ICPMI_ERR_UNSUPPORTED
SURE_SHARE = 0.8                   # share of the map points the float64 reference must be sure about (tests/test_gpu_recalled.py)


# ---- the grid as the device lays it out (float32) --------------------------------------------------------------------------------
def grid(b):
    """(cell, ne, na) of a half angle: dyn_grid of csrc/dynpts.hip"""
    cell = F32(F32(2) * F32(b)) / F32(RINGS) * (F32(1) + F32(1) / F32(256))   # (a little wider than half the reach: see dyn_grid)
    return cell, int(np.floor(PI32 / cell)) + 2, int(np.floor(TWO_PI32 / cell)) + 2


def ncells_formula(b):
    """the estimate of the table size in exact arithmetic, for buckets of exactly half the reach: (pi / b + 2)(2 pi / b + 2) at RINGS = 2"""
    return (math.floor(math.pi / b) + 2) * (math.floor(2 * math.pi / b) + 2)


def angles32(p):
    """(elevation, azimuth) float32 of float32 points in the sensor frame as the kernel and the oracle compute them: the radius in float32,
    asin / atan2 in double, rounded once"""
    p = np.asarray(p, F32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    radius = np.sqrt((x * x + y * y) + z * z)
    return np.arcsin((z / radius).astype(np.float64)).astype(F32), np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F32)


def cells32(b, e, a):
    """(elevation cell, azimuth cell) of float32 angles: dyn_ecell / dyn_acell"""
    cell, ne, na = grid(b)
    ce = np.clip(np.floor((e + HALF_PI32) / cell).astype(np.int64), 0, ne - 1)
    ca = np.clip(np.floor((a + PI32) / cell).astype(np.int64), 0, na - 1)
    return ce, ca


def ulps(v, k):
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return v


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
def from_angles(e, a, r):
    """float64 sensor-frame points of (elevation, azimuth, range)"""
    e, a, r = np.broadcast_arrays(np.asarray(e, np.float64), np.asarray(a, np.float64), np.asarray(r, np.float64))
    return np.stack([r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e)], axis=-1)


def tilted_pose():
    """the sensor of make_recalled.py::dynamic_vectors, tilted: no axis of the sensor frame is one of the map's"""
    cz, sz, cx, sx = math.cos(0.3), math.sin(0.3), math.cos(0.2), math.sin(0.2)
    pose = np.eye(4)
    pose[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    pose[:3, 3] = [1.0, -0.5, 0.8]
    return pose


def to_sensor_of(pose):
    return np.linalg.inv(pose).astype(F32)


def pose_of(to_sensor):
    """the float64 pose whose inverse IS the float32 to_sensor (what the float64 reference is given)"""
    return np.linalg.inv(np.asarray(to_sensor, np.float64))


def cloud(sensor_pts, to_sensor):
    """sensor-frame points -> float32 n x 4 in the map frame (identity: the float32 rounding of the sensor-frame coordinates)"""
    s = np.asarray(sensor_pts, np.float64).reshape(-1, 3)
    out = np.ones((s.shape[0], 4), F32)
    if np.array_equal(to_sensor, np.eye(4, dtype=F32)):
        out[:, :3] = s.astype(F32)
    else:
        P = pose_of(to_sensor)
        out[:, :3] = (s @ P[:3, :3].T + P[:3, 3]).astype(F32)
    return out


def random_normals(rng, m):
    v = rng.normal(size=(m, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def pack(to_sensor, beams_s, map_s, rng, params=None, prob0=None, normals=None, float64=True, **groups):
    prm = dict(PARAMS)
    prm.update(params or {})
    beams, mp = cloud(beams_s, to_sensor), cloud(map_s, to_sensor)
    m = mp.shape[0]
    assert 1 <= beams.shape[0] <= 4096 and 1 <= m <= 8192
    assert (np.linalg.norm(np.asarray(beams_s, np.float64).reshape(-1, 3), axis=1) > 0.5).all() and (np.linalg.norm(np.asarray(map_s, np.float64).reshape(-1, 3), axis=1) > 0.5).all()
    nrm = random_normals(rng, m) if normals is None else np.asarray(normals, F32)
    p0 = rng.choice(PROBS, m).astype(F32) if prob0 is None else np.asarray(prob0, F32)
    flags = dict(float64=float64)
    flags.update({k: np.asarray(v) for k, v in groups.items()})
    return to_sensor, beams, mp, nrm, p0, prm, flags


IDENTITY = np.eye(4, dtype=F32)


# ---- generic(b): the recipe of make_recalled.py::dynamic_vectors, the angular jitter scaled to the half angle -----------------------
def generic(b, seed):
    rng = np.random.default_rng(seed)
    n, m = 3000, 2500
    dirs = rng.normal(size=(n, 3)); dirs[:, 2] *= 0.3; dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rng_in = rng.uniform(3.0, 12.0, n)
    pick = rng.integers(0, n, m)
    ratio = rng.choice(RATIOS, m)
    md = dirs[pick] + rng.normal(0, 0.4 * b, (m, 3)); md /= np.linalg.norm(md, axis=1, keepdims=True)
    map_s = md * (rng_in[pick] * ratio)[:, None]
    map_s[:100] *= 40.0                                              # (most of them) out of range
    return pack(to_sensor_of(tilted_pose()), dirs * rng_in[:, None], map_s, rng, dict(beam_half_angle=b))


# ---- poles: first and last elevation rows, straight up and down ------------------------------------------------------------------
def poles(seed=31):
    rng = np.random.default_rng(seed)
    b = PARAMS["beam_half_angle"]
    golden = math.pi * (3.0 - math.sqrt(5.0))
    be, ba, br, qe, qa, qr = [], [], [], [], [], []
    for sign in (1.0, -1.0):
        t = np.linspace(0.3 * b, 6.0 * b, 40)                         # distance of the beam from the pole
        e = sign * (math.pi / 2 - t)
        a = ((np.arange(40) * golden + (0.5 if sign < 0 else 0.0)) % (2 * math.pi)) - math.pi    # far apart in azimuth: one candidate beam per query
        r = rng.uniform(3.0, 12.0, 40)
        be.append(e); ba.append(a); br.append(r)
        for _ in range(6):                                            # queries clearly inside the radius of their beam, in (elevation, azimuth)
            de, da = rng.uniform(-0.8 * b, 0.8 * b, 40), rng.uniform(-0.8 * b, 0.8 * b, 40)
            qe.append(sign * np.minimum(sign * (e + de), math.pi / 2 - 1e-4)); qa.append(np.clip(a + da, -math.pi + 1e-4, math.pi - 1e-4)); qr.append(r * rng.choice(RATIOS, 40))
        qe.append(e); qa.append(a + 6.0 * b * np.where(a > 0, -1.0, 1.0)); qr.append(r * 0.8)   # same row, 6 b away in azimuth: no beam
    beams_s = from_angles(np.concatenate(be), np.concatenate(ba), np.concatenate(br))
    map_s = from_angles(np.concatenate(qe), np.concatenate(qa), np.concatenate(qr))
    # exactly +-z: x = y = 0, atan2(0, 0) = 0, asin(+-1) = +-pi / 2 -- beams and map points, and map points a little off the axis
    axis_beams = np.array([[0, 0, 7.0], [0, 0, -5.0]])
    axis_map = np.array([[0, 0, 3.5], [0, 0, 6.9], [0, 0, 9.0], [0, 0, -2.5], [0, 0, -4.9], [0, 0, -6.5],
                         [0.01, 0.0, 5.0], [0.012, 0.001, -4.0], [0.02, 0.0, 8.0], [0.015, 0.002, -6.0]])
    n0, m0 = beams_s.shape[0], map_s.shape[0]
    return pack(IDENTITY, np.r_[beams_s, axis_beams], np.r_[map_s, axis_map], rng, axis=m0 + np.arange(6), axis_beams=n0 + np.arange(2))


# ---- seam: the first and last azimuth columns; the reference's kd-tree does not wrap at +-pi ---------------------------------------
def seam(seed=32):
    rng = np.random.default_rng(seed)
    b = PARAMS["beam_half_angle"]
    rows = -1.2 + 0.05 * np.arange(50)                                # 5 b apart: a query sees the beams of its own row only
    beams, pts, across, same = [], [], [], []
    for k, e in enumerate(rows):
        side = 1.0 if k % 2 == 0 else -1.0
        d1 = rng.uniform(0.05 * b, 0.8 * b)
        r = rng.uniform(3.0, 12.0)
        beams.append(from_angles(e, side * (math.pi - d1), r))
        for ratio, near in ((0.8, 0.5), (0.995, 0.8), (1.3, 0.995)):
            d2 = rng.uniform(0.05 * b, 0.8 * b)                        # d1 + d2 < 1.6 b: closer than 2 b ACROSS the seam -- must stay unmatched
            across.append(len(pts)); pts.append(from_angles(e + rng.uniform(-0.2 * b, 0.2 * b), -side * (math.pi - d2), r * near))   # (in front of the beam: a match WOULD move it)
            d3 = rng.uniform(0.05 * b, 1.5 * b)                        # |d1 - d3| < 1.5 b on the same side: must match
            same.append(len(pts)); pts.append(from_angles(e + rng.uniform(-0.2 * b, 0.2 * b), side * (math.pi - d3), r * ratio))
    # azimuth exactly 0, +-pi / 2 and +pi (y = 0 or x = 0 exactly), on rows of their own, with queries on and next to them
    exact, exact_near = [], []
    for j, (ux, uy) in enumerate([(1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-1.0, 0.0)]):
        for e in (-1.3 - 0.05 * j, 1.33 + 0.05 * j):
            r = rng.uniform(4.0, 9.0)
            c, s = math.cos(e), math.sin(e)
            beams.append(np.array([ux * r * c, uy * r * c, r * s]))
            for ratio in (0.8, 1.3):
                exact.append(len(pts)); pts.append(np.array([ux * r * c, uy * r * c, r * s]) * ratio)
                a0 = math.atan2(uy, ux)
                a = a0 - 0.5 * b if ux < 0 else a0 + rng.uniform(-0.7 * b, 0.7 * b)
                exact_near.append(len(pts)); pts.append(from_angles(e + 0.1 * b, a, r * ratio))
                if ux < 0 and ratio < 1:                               # the beam AT +pi: a query just across, at -pi + 0.5 b
                    across.append(len(pts)); pts.append(from_angles(e + 0.1 * b, -math.pi + 0.5 * b, r * ratio))
    m = len(pts)
    prob0 = np.full(m, 0.3, F32)                                       # below the threshold: a match moves the probability
    return pack(IDENTITY, np.array(beams), np.array(pts), rng, prob0=prob0, across=across, same=same, exact=exact, exact_near=exact_near)


# ---- bucket edges: angles k cell - pi / 2 and k cell - pi, each +- {0, 1, 2} ulps, partners two buckets away at about 2 b ----------
def _exact_point(rng, e_t, a_t, which):
    """a float32 point whose elevation (which = 'e') or azimuth ('a') has the wanted float32 bits -- or, where no float32 z / radius gives
    that elevation (asin stretches the spacing of the ratio by 1 / cos), the nearest float32 angle that can be had"""
    t = F32(e_t if which == "e" else a_t)
    r = rng.uniform(3.0, 9.0, 512)
    jit = rng.uniform(-0.5, 0.5, 512) * float(np.spacing(np.abs(t)))
    p = from_angles(float(e_t) + (jit if which == "e" else 0.0), float(a_t) + (jit if which == "a" else 0.0), r).astype(F32)
    got = angles32(p)[0 if which == "e" else 1]
    off = np.abs(got.astype(np.float64) - float(t))
    assert off.min() <= 1.5 * float(np.spacing(np.abs(t))), ("no float32 point near this angle", which, e_t, a_t)
    return p[int(off.argmin())]


PARTNER_ULPS = (-64, -2, -1, 0, 1, 2, 64)   # the partner at 2 b from the on-edge angle: clearly / barely under, at, barely / clearly over


def bucket_edges(b, seed=33):
    """pairs (query, beam) of which ONE sits on a bucket edge +- {0, 1, 2} ulps -- the query for the first edge, the beam for the second --
    and the other about 2 b away, below or above: two buckets away, give or take what the float32 bucket assignment makes of it"""
    rng = np.random.default_rng(seed)
    cell, ne, na = grid(b)
    reach = F32(2) * F32(b)
    assert 2.4 / 69 > 2.5 * float(cell)
    beams, pts, on_e, on_a = [], [], [], []
    for which, c, edges, group in (("e", HALF_PI32, (int(0.35 * ne), int(0.7 * ne)), on_e), ("a", PI32, (int(0.2 * na), int(0.8 * na)), on_a)):
        for k, query_on_edge in zip(edges, (True, False)):
            j = 0
            for eo in (-2, -1, 0, 1, 2):
                for po in PARTNER_ULPS:
                    for side in (-1, 1):
                        # every pair in a band of its own: elevation pairs 5 buckets apart in azimuth, azimuth pairs on 70 rows over 2.4 rad
                        free = -3.0 + 5.0 * float(cell) * j + 0.37 * float(cell) if which == "e" else -1.2 + 2.4 / 69 * j
                        j += 1
                        edge = ulps(F32(k) * cell - c, eo)
                        other = ulps(edge + F32(side) * reach, po)
                        qv, bv = (edge, other) if query_on_edge else (other, edge)
                        group.append(len(pts))
                        pts.append(_exact_point(rng, qv, free, "e") if which == "e" else _exact_point(rng, free, qv, "a"))
                        beams.append(_exact_point(rng, bv, free, "e") if which == "e" else _exact_point(rng, free, bv, "a"))
    return pack(IDENTITY, np.array(beams), np.array(pts), rng, dict(beam_half_angle=b), prob0=np.full(len(pts), 0.3, F32), float64=False,
                on_e=on_e, on_a=on_a)


# ---- dense buckets: 4 q + r records in the table's first and last populated bucket, queries from all 25 bucket positions around ------
def _in_bucket(rng, b, ce, ca, count, lo=0.1, hi=0.9):
    cell = float(grid(b)[0])
    return (ce + rng.uniform(lo, hi, count)) * cell - math.pi / 2, (ca + rng.uniform(lo, hi, count)) * cell - math.pi


def dense(r, seed=34, q=60):
    rng = np.random.default_rng(seed + r)
    b = PARAMS["beam_half_angle"]
    count = 4 * q + r
    first, last = (60, 100), (250, 520)
    be, ba, qe, qa, at_last = [], [], [], [], []
    for ce, ca in (first, last):                                       # consecutive indices: whole waves of one key
        e, a = _in_bucket(rng, b, ce, ca, count)
        be.append(e); ba.append(a)
    e, a = _in_bucket(rng, b, rng.integers(100, 200, 200), rng.integers(5, 620, 200), 200)   # filler between the two, one or two per bucket
    be.append(e); ba.append(a)
    be, ba = np.concatenate(be), np.concatenate(ba)
    br, qr = rng.uniform(4.0, 10.0, be.shape[0]), []
    for blk, (ce, ca) in enumerate((first, last)):
        for de in range(-RINGS, RINGS + 1):
            for da in range(-RINGS, RINGS + 1):
                e, a = _in_bucket(rng, b, ce + de, ca + da, 8)
                qe.append(e); qa.append(a); qr.append(rng.uniform(3.0, 12.0, 8))
        top = blk * count + count - 1                                  # the record with the largest beam index of the bucket: queries right next to it
        at_last += list(sum(len(v) for v in qe) + np.arange(4))
        qe.append(be[top] + rng.uniform(-2e-5, 2e-5, 4)); qa.append(ba[top] + rng.uniform(-2e-5, 2e-5, 4)); qr.append(br[top] * np.array([0.5, 0.8, 0.97, 0.995]))
    qe, qa = np.concatenate(qe), np.concatenate(qa)
    beams_s = from_angles(be, ba, br)
    map_s = from_angles(qe, qa, np.concatenate(qr))
    prob0 = rng.choice(PROBS, qe.shape[0])
    prob0[at_last] = 0.3                                               # (below the threshold: which beam matched shows in the result)
    out = pack(IDENTITY, beams_s, map_s, rng, prob0=prob0, at_last=at_last, dense_counts=[count, count])
    ce_, ca_ = cells32(b, *angles32(out[1]))
    key = ce_ * grid(b)[2] + ca_
    assert (key[:count] == key.min()).all() and (key[count:2 * count] == key.max()).all() and (key[2 * count:] > key.min()).all() and (key[2 * count:] < key.max()).all()
    return out


# ---- ties: beams p, 2 p, p / 2 -- bit-identical angles, three ranges ---------------------------------------------------------------
def ties(seed=35):
    rng = np.random.default_rng(seed)
    b = PARAMS["beam_half_angle"]
    K = 300
    e = rng.uniform(-1.2, 1.2, K)
    a = -3.0 + 6.0 * (np.arange(K) + rng.uniform(0.2, 0.8, K)) / K       # 2 b apart and more: a query sees one direction only
    base = from_angles(e, a, rng.uniform(4.0, 8.0, K)).astype(F32)
    trio = np.concatenate([base, base * F32(2), base * F32(0.5)])       # powers of two: z / radius and atan2(y, x) keep their bits
    perm = rng.permutation(3 * K)
    beams = trio[perm]
    te, ta = angles32(trio)
    assert np.array_equal(te[:K], te[K:2 * K]) and np.array_equal(te[:K], te[2 * K:]) and np.array_equal(ta[:K], ta[K:2 * K]) and np.array_equal(ta[:K], ta[2 * K:]), \
        "the tied beams must have bit-equal float32 angles"
    pts = []
    for scale in (0.3, 0.75, 1.5, 3.0):                                # in front of p / 2, between the returns, behind 2 p
        d = from_angles(e + rng.uniform(-0.6 * b, 0.6 * b, K), a + rng.uniform(-0.6 * b, 0.6 * b, K), 1.0)
        pts.append(d * (np.linalg.norm(base.astype(np.float64), axis=1) * scale)[:, None])
    pts.append(base.astype(np.float64) * 4.0)                            # ON the ray: three beams at angular distance exactly 0
    pts.append(base.astype(np.float64) * 0.25)
    inv = np.empty(3 * K, np.int64); inv[perm] = np.arange(3 * K)        # trio j is beam inv[j]
    trio = np.stack([inv[:K], inv[K:2 * K], inv[2 * K:]], axis=1)        # the beam indices of (p, 2 p, p / 2) per direction
    # the queries the tie rule decides: between p / 2 and p the short return leaves the point untouched and the other two update it alike,
    # between p and 2 p only the long return updates it -- the smallest and the largest index of the trio give different results where that
    # odd return is one of the two
    odd_short = (trio.argmin(axis=1) == 2) | (trio.argmax(axis=1) == 2)
    odd_long = (trio.argmin(axis=1) == 1) | (trio.argmax(axis=1) == 1)
    decided = np.r_[K + np.flatnonzero(odd_short), 2 * K + np.flatnonzero(odd_long)]
    out = pack(IDENTITY, beams, np.concatenate(pts), rng, prob0=np.full(6 * K, 0.3, F32), float64=False, trio=trio, decided=decided)
    assert np.array_equal(out[1][:, :3], beams)
    return out


# ---- wave runs: beam counts around the wave and block sizes, all keys equal (runs of 64) and all distinct (runs of 1) ----------------
WAVE_N = (1, 63, 64, 65, 255, 256, 257)
WAVE_M = (1, 255, 256, 257)


def wave_runs(n, m, equal, seed=36):
    rng = np.random.default_rng(seed + 2 * n + int(equal))
    b = PARAMS["beam_half_angle"]
    if equal:
        be, ba = _in_bucket(rng, b, np.full(n, 157), np.full(n, 314), n)
    else:
        j = np.arange(n)
        be, ba = _in_bucket(rng, b, 150 + 10 * (j // 200), 10 + 3 * (j % 200), n)
    br = rng.uniform(3.0, 12.0, n)
    pick = rng.integers(0, n, m)
    off = rng.uniform(0.1 * b, 0.7 * b, m)
    th = rng.uniform(0, 2 * math.pi, m)
    if m == 1:
        pick, off = np.array([0]), np.array([0.3 * b])
    map_s = from_angles(be[pick] + off * np.cos(th), ba[pick] + off * np.sin(th), br[pick] * (rng.choice(RATIOS, m) if m > 1 else 0.8))
    out = pack(IDENTITY, from_angles(be, ba, br), map_s, rng)
    ce, ca = cells32(b, *angles32(out[1]))
    key = ce * grid(b)[2] + ca
    assert (np.unique(key).size == 1) if equal else (np.unique(key).size == n)
    return out


# ---- boundaries: the exact decision points of the update -----------------------------------------------------------------------------
def boundaries(max_range, seed=37):
    rng = np.random.default_rng(seed)
    thr = F32(PARAMS["threshold_dynamic"])
    j = np.arange(60)
    be, ba, br = 0.05 * np.sin(j), -3.0 + 0.1 * j, np.full(60, 4.0)
    beams_s = np.r_[from_angles(be, ba, br), [[3.6, 4.8, 0.0]]]          # the last beam: along (3, 4, 0), behind it
    pts, prob0, nrm = [], [], []
    specials = [thr, np.nextafter(thr, F32(0)), np.nextafter(thr, F32(1)), F32(0), F32(1), F32(0.3)]
    for i in range(60):
        for t, ratio in enumerate((0.8, 0.97, 1.03, 1.2)):
            pts.append(from_angles(be[i] + 0.2 * PARAMS["beam_half_angle"], ba[i] - 0.3 * PARAMS["beam_half_angle"], br[i] * ratio))
            prob0.append(specials[(4 * i + t) % len(specials)])
            v = rng.normal(size=3)
            nrm.append(np.zeros(3) if (i + t) % 7 == 0 else v / np.linalg.norm(v))   # a zero normal: w_v = eps
    n_ring = len(pts)
    pts += [np.array([3.0, 4.0, 0.0]), np.array([3.0, 4.0, 0.0]) * (1 - 2.0 ** -20), np.array([3.0, 4.0, 0.0]) * (1 + 2.0 ** -20)]   # (exact in float32)
    prob0 += [F32(0.3)] * 3
    nrm += [np.array([0.6, 0.8, 0.0])] * 3
    return pack(IDENTITY, beams_s, np.array(pts), rng, dict(sensor_max_range=max_range), prob0=np.array(prob0, F32), normals=np.array(nrm), float64=False,
                at_range=[n_ring], inside=[n_ring + 1], outside=[n_ring + 2], latched=[i for i, p in enumerate(prob0[:n_ring]) if p >= thr],
                zero_normal=[i for i, v in enumerate(nrm) if not np.any(v)])


# ---- the registry ----------------------------------------------------------------------------------------------------------------------
GENERIC_B = (0.001, 0.0011, 0.01, 0.5, 2.0)      # 0.001 / 0.0011: either side of the two-kernel scan's limit; 0.5 / 2.0: grids smaller than the 5 x 5 block
BUILDERS = {f"generic-b{b}": (generic, (b, 100 + i)) for i, b in enumerate(GENERIC_B)}
BUILDERS["generic-b0.03"] = (generic, (0.03, 110))                       # (one handle across grid sizes)
BUILDERS.update({"poles": (poles, ()), "seam": (seam, ()), "ties": (ties, ()),
                 "bucket_edges-b0.01": (bucket_edges, (0.01,)), "bucket_edges-b0.0137": (bucket_edges, (0.0137,)),
                 "boundaries-r5": (boundaries, (5.0,)), "boundaries-inf": (boundaries, (math.inf,))})
BUILDERS.update({f"dense-r{r}": (dense, (r,)) for r in range(4)})
BUILDERS.update({f"wave-n{n}-{'equal' if eq else 'distinct'}-m{WAVE_M[(2 * i + eq) % 4]}": (wave_runs, (n, WAVE_M[(2 * i + eq) % 4], bool(eq)))
                 for i, n in enumerate(WAVE_N) for eq in (0, 1)})
IDS = sorted(BUILDERS)

# float64 bar per flagged case: |result - float64| <= tol on the points the float64 reference is sure about.  tol = max(2e-4, twice the
# oracle's largest error there as MEASURED on the CPU -- the number beside it); 2e-4 is the bar of tests/test_gpu_recalled.py at b = 0.01.
# w_d1 divides a float32 angular distance by 2 b: the error grows as b shrinks, and near the poles asin amplifies the rounding of z / radius.
MEASURED = {
    "dense-r0": 5.240e-06,
    "dense-r1": 2.683e-06,
    "dense-r2": 6.292e-06,
    "dense-r3": 5.378e-06,
    "generic-b0.001": 1.686e-04,
    "generic-b0.0011": 6.728e-05,
    "generic-b0.01": 2.087e-05,
    "generic-b0.03": 4.435e-06,
    "generic-b0.5": 4.076e-06,
    "generic-b2.0": 4.352e-06,
    "poles": 3.128e-04,
    "seam": 1.166e-05,
    "wave-n1-distinct-m1": 1.660e-08,
    "wave-n1-equal-m255": 9.216e-08,
    "wave-n255-distinct-m1": 1.660e-08,
    "wave-n255-equal-m255": 1.546e-07,
    "wave-n256-distinct-m256": 2.105e-06,
    "wave-n256-equal-m257": 1.205e-07,
    "wave-n257-distinct-m1": 1.660e-08,
    "wave-n257-equal-m255": 1.962e-07,
    "wave-n63-distinct-m256": 6.621e-06,
    "wave-n63-equal-m257": 1.278e-07,
    "wave-n64-distinct-m1": 2.375e-06,
    "wave-n64-equal-m255": 3.114e-07,
    "wave-n65-distinct-m256": 1.002e-05,
    "wave-n65-equal-m257": 1.053e-07,
}


def tol(cid):
    return max(2e-4, 2.0 * MEASURED[cid])


@functools.lru_cache(maxsize=None)
def case(cid):
    fn, args = BUILDERS[cid]
    out = fn(*args)
    for v in out[:5]:
        v.setflags(write=False)
    return out


def kwargs(params):
    """the keyword arguments of icp.dynamicPointsUpdate / oracle_bindings.dynamic_points_update"""
    return {k: float(params[k]) for k in KEYS}


def module(params):
    """the ('dynamic_points', ...) operator of icp.mapUpdateChain"""
    return ("dynamic_points",) + tuple(float(params[k]) for k in KEYS)


# ---- the float64 yardstick: the project's own restatement of the reference, imported by path -------------------------------------------
@functools.lru_cache(maxsize=None)
def recalled():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_recalled.py")
    spec = importlib.util.spec_from_file_location("make_recalled", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def float64_reference(cid):
    """(expected float64, sure) of a case: sure = (margin > 1e-4) & ~ambiguous, as make_recalled.py::dynamic_vectors stores it"""
    to_sensor, beams, mp, nrm, prob0, prm, _ = case(cid)
    f = {k: float(F32(prm[k])) for k in KEYS}
    expected, margin, amb = recalled().dynamic_points_update(pose_of(to_sensor), beams, mp, nrm, prob0, thresholdDynamic=f["threshold_dynamic"], alpha=f["alpha"],
                                                             beta=f["beta"], beamHalfAngle=f["beam_half_angle"], epsilonA=f["epsilon_a"], epsilonD=f["epsilon_d"],
                                                             sensorMaxRange=f["sensor_max_range"])
    return expected, (margin > 1e-4) & ~amb


def float64_error(cid, result):
    """(largest |result - float64| on the sure points, the map index where, share of sure points)"""
    expected, sure = float64_reference(cid)
    err = np.where(sure, np.abs(result.astype(np.float64) - expected), 0.0)
    return float(err.max()), int(err.argmax()), float(sure.mean())


def first_diff(got, ref, limit=10):
    return np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))[:limit].tolist()
