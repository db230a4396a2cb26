"""Sweep registration (include/icpmi.h: icpmi_register_sweep) in float64 numpy with exact neighbours, and the float32 restatement of its
pair expressions.  Poses are 4 x 4 float64 (row-major numpy); the sensor's pose at the time fraction alpha is the translation's lerp and
the rotation's slerp between the pose at sweep begin and the pose at sweep end, as icpmi_deskew interpolates its table.

Layout of the 80 sums: [0..20] M0 (upper triangle, row-major), [21..41] M1, [42..62] M2, [63..68] g0, [69..74] g1, [75] sum w, [76] pairs,
[77] sum w r^2, [78], [79] zero."""
import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

import deskew_reference as dr
import localizability_reference as lr

F = np.float32
BEGIN_S, END_S, UNIT_S = 0.0, 0.1, 1e-9           # the sweep's span and the unit of t_rel (nanoseconds, as the bundled scans' `t`)
STAMPS = (BEGIN_S, END_S)
M0, M1, M2, G0, G1, W, PAIRS, WR2 = 0, 21, 42, 63, 69, 75, 76, 77
IU = np.triu_indices(6)


# ------------------------------------------------------------------------------------------------------------------ time and poses
def alpha_of(t_rel, begin=BEGIN_S, end=END_S, unit=UNIT_S):
    """alpha = clamp((t_rel * unit - begin) / (end - begin), 0, 1) in float64, rounded once to float32"""
    tau = np.asarray(t_rel, F).astype(np.float64) * np.float64(unit)
    tau = np.where(tau < begin, begin, np.where(tau > end, end, tau))
    return ((tau - begin) / (np.float64(end) - np.float64(begin))).astype(F)


def pose7(T):
    """tx ty tz qx qy qz qw of a 4 x 4"""
    T = np.asarray(T, np.float64)
    return np.concatenate([T[:3, 3], Rotation.from_matrix(T[:3, :3]).as_quat()])


def T_of_pose7(p):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(np.asarray(p[3:7], np.float64)).as_matrix()
    T[:3, 3] = p[:3]
    return T


def world_points(scan, alpha, Tb, Te):
    """T(alpha_i) x_i: the raw scan's points in the map frame under the two-pose motion (float64)"""
    x = np.asarray(scan, F).astype(np.float64)[:, :3]
    R, p = dr.pose_at([0.0, 1.0], np.stack([pose7(Tb), pose7(Te)]), np.asarray(alpha, F).astype(np.float64))
    return R.apply(x) + p


def deskew_to_end(scan, alpha, Tb, Te):
    """the scan as seen from the end pose: T_e^-1 T(alpha_i) x_i (float64)"""
    Te = np.asarray(Te, np.float64)
    return (world_points(scan, alpha, Tb, Te) - Te[:3, 3]) @ Te[:3, :3]


def apply_step(T, xi, mu):
    """S(xi) T with the centred-frame step xi = (omega, t) moved to the map frame: S = [R_s | t + mu - R_s mu]"""
    S = lr.make_T(xi[:3], xi[3:])
    mu = np.asarray(mu, np.float64)
    S[:3, 3] = S[:3, 3] + mu - S[:3, :3] @ mu
    return S @ np.asarray(T, np.float64)


# ------------------------------------------------------------------------------------------------------------------ the sums
def pack(m0, m1, m2, g0, g1, w, pairs, wr2):
    s = np.zeros(80)
    s[M0:M0 + 21], s[M1:M1 + 21], s[M2:M2 + 21] = m0[IU], m1[IU], m2[IU]
    s[G0:G0 + 6], s[G1:G1 + 6], s[W], s[PAIRS], s[WR2] = g0, g1, w, pairs, wr2
    return s


def unpack(s):
    s = np.asarray(s, np.float64)
    out = {}
    for name, off in (("M0", M0), ("M1", M1), ("M2", M2)):
        m = np.zeros((6, 6))
        m[IU] = s[off:off + 21]
        out[name] = m + np.triu(m, 1).T
    out.update(g0=s[G0:G0 + 6].copy(), g1=s[G1:G1 + 6].copy(), W=s[W], pairs=s[PAIRS], wr2=s[WR2])
    return out


def _sums(Fm, r, w, a):
    """the double-precision part, shared by both restatements: Fm (P, 6), r (P,), w (P,), a (P,) as float64; pairs with w == 0 left out.
    Returns (sums (80,), the sums of |w F r| (6,) that scale the deviation of g)"""
    el = w != 0
    Fm, r, w, a = Fm[el], r[el], w[el], a[el]
    m = (w[:, None] * Fm)[:, :, None] * Fm[:, None, :]
    gr = (w[:, None] * Fm) * r[:, None]
    s = pack(m.sum(0), (a[:, None, None] * m).sum(0), ((a * a)[:, None, None] * m).sum(0), gr.sum(0), (a[:, None] * gr).sum(0), w.sum(), float(el.sum()),
             ((w * r) * r).sum())
    return s, np.abs(gr).sum(0)


def sums64(p, q, n, w, alpha):
    """float64 end to end: p the reading's points, q their matches, n the matches' normals (all relative to the same origin)"""
    p, q, n = (np.asarray(v, np.float64) for v in (p, q, n))
    Fm = np.concatenate([np.cross(p, n), n], 1)
    r = ((p - q) * n).sum(1)
    return _sums(Fm, r, np.asarray(w, np.float64), np.asarray(alpha, F).astype(np.float64))


def sums32(p, q, n, w, alpha):
    """the device's pair expressions: F and r in float32 in the order include/icpmi.h writes them, the sums in double"""
    p, q, n = (np.asarray(v, F) for v in (p, q, n))
    Fm = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
                   n[:, 0], n[:, 1], n[:, 2]], 1)
    d = p - q
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    assert Fm.dtype == F and r.dtype == F
    return _sums(Fm.astype(np.float64), r.astype(np.float64), np.asarray(w, F).astype(np.float64), np.asarray(alpha, F).astype(np.float64))


def deviation(got, want, gscale):
    """how far the sums `got` lie from `want`: per block the largest absolute difference over the block's scale (the largest entry of a
    moment block; the largest sum of |w F r| for g0 and g1; the value itself for sum w and sum w r^2).  The pair counts must be equal."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got[PAIRS] == want[PAIRS]
    dev = 0.0
    for off in (M0, M1, M2):
        sc = np.abs(want[M0:M0 + 21]).max()
        dev = max(dev, np.abs(got[off:off + 21] - want[off:off + 21]).max() / sc)
    gs = np.max(gscale)
    if gs > 0:
        dev = max(dev, np.abs(got[G0:G1 + 6] - want[G0:G1 + 6]).max() / gs)
    for i in (W, WR2):
        if want[i] != 0:
            dev = max(dev, abs(got[i] - want[i]) / abs(want[i]))
    return float(dev)


# ------------------------------------------------------------------------------------------------------------------ the solve
def system(sums, lambda_rot=0.0, lambda_trans=0.0, d=None):
    """A (12, 12) and rhs (12,) of the step x = (xi_b, xi_e), as include/icpmi.h writes them"""
    u = unpack(sums)
    A = np.block([[u["M0"] - 2 * u["M1"] + u["M2"], u["M1"] - u["M2"]], [u["M1"] - u["M2"], u["M2"]]])
    rhs = -np.concatenate([u["g0"] - u["g1"], u["g1"]])
    L = u["W"] * np.diag([lambda_rot] * 3 + [lambda_trans] * 3)
    D = np.concatenate([-np.eye(6), np.eye(6)], 1)
    d = np.zeros(6) if d is None else np.asarray(d, np.float64)
    return A + D.T @ L @ D, rhs - D.T @ L @ d


def solve(sums, lambda_rot=0.0, lambda_trans=0.0, d=None):
    A, rhs = system(sums, lambda_rot, lambda_trans, d)
    return np.linalg.solve(A, rhs)


# ------------------------------------------------------------------------------------------------------------------ the chain
def trimmed_limit(d2, ratio):
    """TrimmedDistOutlierFilter's limit (tests/match_reference.py: trimmed_quantile) on float64 distances"""
    v = d2[np.isfinite(d2) & (d2 > 0)]
    if v.size == 0:
        return -1.0
    r = min(int(F(v.size) * F(ratio)), v.size - 1)
    return float(np.partition(v, r)[r])


def match(tree, mp, nm, P, max_dist, trim):
    """exact nearest neighbours within max_dist, then the Trimmed filter: (q, n, w)"""
    dist, ids = tree.query(P, k=1, distance_upper_bound=max_dist)
    ok = np.isfinite(dist)
    ids = np.where(ok, ids, 0)
    d2 = np.where(ok, dist * dist, np.inf)
    w = ok.astype(np.float64)
    if trim is not None:
        w = w * (d2 <= trimmed_limit(d2, trim))
    return mp[ids], nm[ids], w


def register_sweep(mp, nm, scan, alpha, Tb, Te, mu, max_dist, trim, iterations=12, lambda_rot=0.0, lambda_trans=0.0, min_rot=0.0, min_trans=0.0):
    """the whole algorithm: (T_b, T_e, iterations run, the steps' norms per iteration)"""
    mp64, nm64 = np.asarray(mp, F).astype(np.float64)[:, :3], np.asarray(nm, F).astype(np.float64)
    tree = cKDTree(mp64)
    mu = np.asarray(mu, np.float64)
    Tb, Te = np.array(Tb, np.float64), np.array(Te, np.float64)
    d = np.zeros(6)
    norms = []
    it = 0
    while it < iterations:
        P = world_points(scan, alpha, Tb, Te)
        q, n, w = match(tree, mp64, nm64, P, max_dist, trim)
        s, _ = sums64(P - mu, q - mu, n, w, alpha)
        x = solve(s, lambda_rot, lambda_trans, d)
        Tb, Te = apply_step(Tb, x[:6], mu), apply_step(Te, x[6:], mu)
        d += x[6:] - x[:6]
        it += 1
        nr = [np.linalg.norm(x[0:3]), np.linalg.norm(x[3:6]), np.linalg.norm(x[6:9]), np.linalg.norm(x[9:12])]
        norms.append(nr)
        if nr[0] < min_rot and nr[2] < min_rot and nr[1] < min_trans and nr[3] < min_trans:
            break
    return Tb, Te, it, norms


def register_rigid(mp, nm, scan, T, mu, max_dist, trim, iterations=12):
    """point-to-plane ICP of the scan as a rigid body through the same chain: the step is M0^-1 (-g0)"""
    mp64, nm64 = np.asarray(mp, F).astype(np.float64)[:, :3], np.asarray(nm, F).astype(np.float64)
    tree = cKDTree(mp64)
    mu = np.asarray(mu, np.float64)
    T = np.array(T, np.float64)
    x3 = np.asarray(scan, F).astype(np.float64)[:, :3]
    zero = np.zeros(x3.shape[0], F)
    for _ in range(iterations):
        P = x3 @ T[:3, :3].T + T[:3, 3]
        q, n, w = match(tree, mp64, nm64, P, max_dist, trim)
        u = unpack(sums64(P - mu, q - mu, n, w, zero)[0])
        T = apply_step(T, np.linalg.solve(u["M0"], -u["g0"]), mu)
    return T


def point_error(P, truth):
    e = np.linalg.norm(np.asarray(P, np.float64) - np.asarray(truth, np.float64), axis=1)
    return float(e.mean()), float(e.max())
