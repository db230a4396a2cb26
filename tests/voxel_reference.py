"""Float64 reference of VoxelMatcher (include/icpmi.h: icpmi_set_voxel_matcher), a float32 restatement of the same
specification, and the helpers their tests share.  Pure numpy: nothing here touches the library.

The table of a (centred) map: per axis i = (int)floor(x / size) in FLOAT32, a point taking part iff its coordinates are finite and every
|i| < 2^20; key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20); per occupied voxel its count, the mean mu of its points and
N = (1 / count) sum u u^T over the unit normals u (unit_or_zero in float32: a zero or non-finite normal adds nothing).  Keys and unit
normals are float32 exactly as specified, everything else float64.

For a pair (reading point p = T x, the voxel it falls into): q = mu, C_v = I - (1 - eps) N, u_p = unit_or_zero(R n_x),
S = C_v + C(u_p) = 2 I - (1 - eps)(N + u_p u_p^T), M = S^-1, then plane_to_plane_reference.sums_from_M with weight 1.
"""
import numpy as np

import localizability_reference as lr
import plane_to_plane_reference as pr
import symmetric_reference as sr

F32 = np.float32
BIAS = 1 << 20
HASH_MUL = 0x9E3779B97F4A7C15
# the start of the issue's prototype: 0.3 / -0.2 / 0.1 m and the rotation vector (0.02, -0.03, 0.05) off the truth
START_TRANS, START_ROT = (0.3, -0.2, 0.1), (0.02, -0.03, 0.05)
POSES = {"true": np.eye(4), "start": lr.make_T(START_ROT, START_TRANS)}
DIFFERENTIAL = sr.DIFFERENTIAL
MAX_ITER = 40


def voxel_index(xyz, size):
    """(ok (N,), ijk (N, 3) int64): the float32 floor(x / size) of every row; ok = finite and every |i| < 2^20 (ijk is 0 where not ok)"""
    x = np.asarray(xyz, F32)[:, :3]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor(x / F32(size))
        assert f.dtype == F32
        ok = np.isfinite(x).all(1) & (np.abs(f) < F32(BIAS)).all(1)
    return ok, np.where(ok[:, None], f, 0).astype(np.int64)


def pack_keys(ijk):
    b = np.asarray(ijk, np.int64) + BIAS
    return ((b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]).astype(np.uint64)


def first_slot(keys, capacity):
    """where a key's probe sequence starts in a table of `capacity` slots (a power of two): include/icpmi.h states the hash"""
    k = np.asarray(keys, np.uint64)
    with np.errstate(over="ignore"):
        h = (k * np.uint64(HASH_MUL)) >> np.uint64(32)
    return (h & np.uint64(capacity - 1)).astype(np.int64)


def capacity_of(n_voxels):
    cap = 2
    while cap < 2 * n_voxels:
        cap <<= 1
    return cap


def table(points, normals, size):
    """the float64 table of (centred, float32) points and their normals: dict(keys uint64 ascending, ijk, count, mu (V, 3), N (V, 6):
    xx xy xz yy yz zz, max_abs (V,): the largest |coordinate| among the voxel's points, of (N,): every point's voxel).  Raises ValueError
    for a point that cannot take part (the build's ICPMI_ERR_INVALID_ARG)."""
    pts = np.asarray(points, F32)[:, :3]
    ok, ijk = voxel_index(pts, size)
    if not ok.all():
        raise ValueError("a map point is not finite or out of the key's range")
    keys, of, count = np.unique(pack_keys(ijk), return_inverse=True, return_counts=True)
    of = of.ravel()
    V = keys.size
    u = pr.unit_or_zero(np.asarray(normals, F32).copy()).astype(np.float64)
    p64 = pts.astype(np.float64)
    mu = np.zeros((V, 3))
    N = np.zeros((V, 6))
    for c in range(3):
        mu[:, c] = np.bincount(of, p64[:, c], V)
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        N[:, j] = np.bincount(of, u[:, a] * u[:, b], V)
    mu /= count[:, None]
    N /= count[:, None]
    max_abs = np.zeros(V)
    np.maximum.at(max_abs, of, np.abs(p64).max(1))
    first = np.zeros(V, np.int64)
    first[of[::-1]] = np.arange(pts.shape[0])[::-1]
    return dict(keys=keys, ijk=ijk[first], count=count.astype(np.int64), mu=mu, N=N, max_abs=max_abs, of=of, size=float(size))


def table_f32(tab):
    """the table as the device keeps it: every sum rounded ONCE to float32"""
    out = dict(tab)
    out["mu"], out["N"] = tab["mu"].astype(F32), tab["N"].astype(F32)
    return out


def lookup(tab, q):
    """index into the table's order of the voxel every row of q (float32, centred) falls into, -1 for none: a float32 floor(x / size)"""
    ok, ijk = voxel_index(q, tab["size"])
    keys = pack_keys(ijk)
    pos = np.searchsorted(tab["keys"], keys)
    pos = np.minimum(pos, tab["keys"].size - 1)
    hit = ok & (tab["keys"][pos] == keys)
    return np.where(hit, pos, -1).astype(np.int64)


def _full(N6):
    N6 = np.asarray(N6)
    M = np.empty((N6.shape[0], 3, 3), N6.dtype)
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        M[:, a, b] = M[:, b, a] = N6[:, j]
    return M


def pair_matrices(N6, npr, eps):
    """M (P, 3, 3) float64 by numpy.linalg.inv from the voxels' moments and the reading's ROTATED normals (not yet normalised)"""
    up = pr.unit_or_zero(np.asarray(npr, np.float64))
    g = 1.0 - float(eps)
    S = 2.0 * np.eye(3)[None] - g * (_full(np.asarray(N6, np.float64)) + up[:, :, None] * up[:, None, :])
    return np.linalg.inv(S)


def reference_sums(p, npr, vox, tab, eps=pr.EPS_DEFAULT):
    """the float64 sums on given (point, voxel) pairs: p (N, 3) transformed reading points, npr their rotated normals, vox (N,) the voxel
    of every point (-1: no pair), tab a table (float64, or table_f32 for the device's)"""
    sel = np.asarray(vox) >= 0
    if not sel.any():
        out = np.zeros(32)
        return out
    v = np.asarray(vox)[sel]
    mu, N6 = np.asarray(tab["mu"], np.float64)[v], np.asarray(tab["N"], np.float64)[v]
    return pr.sums_from_M(np.asarray(p, np.float64)[sel], mu, pair_matrices(N6, np.asarray(npr)[sel], eps))


def float32_sums(p, npr, vox, tab, eps=pr.EPS_DEFAULT):
    """the specification as the kernel evaluates it: the float32 table, every per-pair quantity in float32 (adjugate / determinant inverse,
    no contraction), the sums in float64.  Differs from the kernel by the order of the double sums only."""
    sel = np.asarray(vox) >= 0
    out = np.zeros(32)
    if not sel.any():
        return out
    v = np.asarray(vox)[sel]
    p, up = np.asarray(p, F32)[sel], pr.unit_or_zero(np.asarray(npr, F32)[sel].copy())
    q, N6 = np.asarray(tab["mu"]).astype(F32)[v], np.asarray(tab["N"]).astype(F32)[v]
    g, two = F32(1) - F32(eps), F32(2)
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}

    def s(i, j):
        t = g * (N6[:, idx[(i, j)]] + up[:, i] * up[:, j])
        return two - t if i == j else -t

    sxx, syy, szz, sxy, sxz, syz = s(0, 0), s(1, 1), s(2, 2), s(0, 1), s(0, 2), s(1, 2)
    c00, c01, c02 = syy * szz - syz * syz, sxz * syz - sxy * szz, sxy * syz - sxz * syy
    c11, c12, c22 = sxx * szz - sxz * sxz, sxy * sxz - sxx * syz, sxx * syy - sxy * sxy
    idet = F32(1) / (sxx * c00 + sxy * c01 + sxz * c02)
    m0 = np.stack([c00 * idet, c01 * idet, c02 * idet], 1)
    m1 = np.stack([m0[:, 1], c11 * idet, c12 * idet], 1)
    m2 = np.stack([m0[:, 2], m1[:, 2], c22 * idet], 1)
    d = p - q
    md = np.stack([m0[:, 0] * d[:, 0] + m0[:, 1] * d[:, 1] + m0[:, 2] * d[:, 2], m1[:, 0] * d[:, 0] + m1[:, 1] * d[:, 1] + m1[:, 2] * d[:, 2],
                   m2[:, 0] * d[:, 0] + m2[:, 1] * d[:, 1] + m2[:, 2] * d[:, 2]], 1)
    cross = pr._cross
    pmd = cross(p, md)
    k0, k1, k2 = cross(p, m0), cross(p, m1), cross(p, m2)
    pm = [np.stack([k0[:, i], k1[:, i], k2[:, i]], 1) for i in range(3)]
    r = [cross(p, pm[i]) for i in range(3)]
    for a in (m0, md, pmd, pm[0], r[0]):
        assert a.dtype == F32
    cols = [r[0][:, 0], r[0][:, 1], r[0][:, 2], pm[0][:, 0], pm[0][:, 1], pm[0][:, 2], r[1][:, 1], r[1][:, 2], pm[1][:, 0], pm[1][:, 1], pm[1][:, 2],
            r[2][:, 2], pm[2][:, 0], pm[2][:, 1], pm[2][:, 2], m0[:, 0], m0[:, 1], m0[:, 2], m1[:, 1], m1[:, 2], m2[:, 2],
            -pmd[:, 0], -pmd[:, 1], -pmd[:, 2], -md[:, 0], -md[:, 1], -md[:, 2]]
    for i, c in enumerate(cols):
        out[i] = float(c.astype(np.float64).sum())
    out[27] = out[28] = float(sel.sum())
    return out


def centred(cloud, mean):
    """x - mean in float32, as the handle centres a cloud (mean: icpmi_get_map_mean, or map_mean below)"""
    out = np.array(cloud, F32, copy=True)
    out[:, :3] = out[:, :3] - np.asarray(mean, F32)[None, :]
    return out


def map_mean(map4):
    return np.asarray(map4)[:, :3].astype(np.float64).mean(0).astype(F32)


def register(map4, normals, reading4, read_normals, size, precision=64, eps=pr.EPS_DEFAULT, mean=None):
    """ICP of a reading against a map from the identity with the voxel pairing, CounterTransformationChecker 40 and the Differential checker
    of the tests.  precision 64: the float64 table, sums and solve on the float32 clouds; 32: the float32 restatements (table_f32,
    float32_sums, plane_to_plane_reference.float32_step, float32 pose products).  Returns dict(T: the pose in the clouds' frame, float64
    4 x 4; iterations; pairs: the pair count of every iteration)."""
    assert precision in (32, 64)
    mean = map_mean(map4) if mean is None else np.asarray(mean, F32)
    mc, rc = centred(map4, mean), centred(reading4, mean)
    tab = table(mc, normals, size)
    if precision == 32:
        tab = table_f32(tab)
    T = np.eye(4, dtype=F32 if precision == 32 else np.float64)
    rn = np.asarray(read_normals, F32)
    poses, pairs = [], []
    for _ in range(MAX_ITER):
        if precision == 32:
            p, npr = pr.xf_points(T, rc), pr.rot_normals(T, rn)
        else:
            p = rc[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            npr = rn.astype(np.float64) @ T[:3, :3].T
        vox = lookup(tab, p.astype(F32))           # (the pairing is the float32 key of the point rounded to float32, in both loops)
        pairs.append(int((vox >= 0).sum()))
        if pairs[-1] == 0:
            raise RuntimeError("no point to minimize")
        if precision == 32:
            T = (sr._float32_step_T(float32_sums(p, npr, vox, tab, eps)) @ T).astype(F32)
        else:
            x = pr.solve_step(reference_sums(p, npr, vox, tab, eps))
            T = lr.make_T(x[:3], x[3:]) @ T
        poses.append(np.array(T, np.float64))
        if sr.differential_stop(poses, **DIFFERENTIAL) is not None:
            break
    Tw = poses[-1].copy()
    m64 = mean.astype(np.float64)
    Tw[:3, 3] = Tw[:3, 3] + m64 - Tw[:3, :3] @ m64      # centred frame -> the clouds' frame
    return dict(T=Tw, iterations=len(poses), pairs=pairs)


def centroid_error(T, T_true, reading4):
    """(translation error measured at the reading's centroid, rotation error) of T against T_true"""
    c = np.asarray(reading4, np.float64)[:, :3].mean(0)
    D = np.asarray(T, np.float64) @ np.linalg.inv(np.asarray(T_true, np.float64))
    a, b = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    dt = float(np.linalg.norm((a[:3, :3] @ c + a[:3, 3]) - (b[:3, :3] @ c + b[:3, 3])))
    return dt, float(np.linalg.norm(lr.step_from_T(D)[:3]))
