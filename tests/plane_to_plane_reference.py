"""Float64 restatement of the plane-to-plane (generalized ICP) pair sums (include/icpmi.h: ICPMI_MIN_PLANE_TO_PLANE), a float32
restatement of the same specification, and the helpers their tests share.  Pure numpy: nothing here touches the library.

For a pair: p = T x, q its match, n_q the match's normal, n_p = R n_x the reading point's normal under T's rotation; each normalised, a zero
or non-finite normal counting as "no surface model" (that side's covariance is I):
    C(n) = I - (1 - eps) n n^T,  S = C(n_q) + C(n_p),  M = S^-1,  G = J^T = [[p]x; I] (6 x 3),  d = p - q
    A += w G M G^T (upper 21 -> slots 0..20),  b -= w G M d (slots 21..26),  slot 27 = sum w, slot 28 = pairs
With M = n n^T this is localizability_reference.pair_sums (point-to-plane): G n = [p x n; n] = F.
"""
import numpy as np

import localizability_reference as lr

F32 = np.float32
EPS_DEFAULT = 1e-3
IU = np.triu_indices(6)     # the order of slots 0..20: upper triangle, row-major


def xf_points(T, xyzw):
    """p = T x as the device forms it (common.h: xf_point): float32 fmaf chains, column by column.  A float64 product of two float32 is exact
    and its sum with a float32 is rounded once to 53 bits and once more to 24: the fmaf result but for rare double roundings."""
    T = np.asarray(T, F32).astype(np.float64)
    x = np.asarray(xyzw, F32).astype(np.float64)
    out = np.empty((x.shape[0], 3), F32)
    for r in range(3):
        a = (T[r, 0] * x[:, 0]).astype(F32).astype(np.float64)
        a = (T[r, 1] * x[:, 1] + a).astype(F32).astype(np.float64)
        a = (T[r, 2] * x[:, 2] + a).astype(F32).astype(np.float64)
        out[:, r] = (T[r, 3] * x[:, 3] + a).astype(F32)
    return out


def rot_normals(T, n):
    """R n in float32 by the same chains (no translation)"""
    return xf_points(T, np.concatenate([np.asarray(n, F32), np.zeros((len(n), 1), F32)], 1))


def unit_or_zero(n):
    """rows scaled to length 1; a zero or non-finite row -> 0 (no surface model).  Works in the dtype it is given."""
    n = np.asarray(n)
    l2 = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
    ok = (l2 > 0) & np.isfinite(l2)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ok, n.dtype.type(1) / np.sqrt(l2), n.dtype.type(0))
        u = n * inv[:, None]
    u[~ok] = 0
    return u


def pair_matrices(nq, npr, eps):
    """M (N, 3, 3) float64 by numpy.linalg.inv; nq / npr: normals as given (not yet normalised), npr already rotated"""
    uq, up = unit_or_zero(np.asarray(nq, np.float64)), unit_or_zero(np.asarray(npr, np.float64))
    g = 1.0 - float(eps)
    S = 2.0 * np.eye(3)[None] - g * (uq[:, :, None] * uq[:, None, :] + up[:, :, None] * up[:, None, :])
    return np.linalg.inv(S)


def sums_from_M(p, q, M, w=None):
    """sums[32] in float64 from per-pair 3 x 3 matrices M: A = sum w G M G^T, b = -sum w G M d"""
    p, q, M = np.asarray(p, np.float64), np.asarray(q, np.float64), np.asarray(M, np.float64)
    N = p.shape[0]
    w = np.ones(N) if w is None else np.asarray(w, np.float64)
    G = np.zeros((N, 6, 3))
    G[:, 0, 1], G[:, 0, 2] = -p[:, 2], p[:, 1]
    G[:, 1, 0], G[:, 1, 2] = p[:, 2], -p[:, 0]
    G[:, 2, 0], G[:, 2, 1] = -p[:, 1], p[:, 0]
    G[:, 3:, :] = np.eye(3)[None]
    GM = G @ M
    A = np.einsum("n,nij->ij", w, GM @ G.transpose(0, 2, 1))
    b = -np.einsum("n,ni->i", w, (GM @ (p - q)[:, :, None])[:, :, 0])
    keep = w != 0
    return lr.pack_sums(A, b, float(w.sum()), int(keep.sum()))


def reference_sums(p, q, nq, npr, eps=EPS_DEFAULT, w=None):
    """the float64 reference: p (N, 3) transformed reading points, q their matches, nq the matches' normals, npr the reading's normals
    ALREADY rotated, w the weights (pairs with w == 0 do not count)"""
    return sums_from_M(p, q, pair_matrices(nq, npr, eps), w)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def float32_sums(p, q, nq, npr, eps=EPS_DEFAULT, w=None):
    """the specification as the kernel evaluates it: every per-pair quantity in float32 (adjugate / determinant inverse, no contraction),
    the weight's product and the sums in float64.  Differs from the kernel by the order of the double sums only."""
    p, q, nq, npr = (np.asarray(a, F32) for a in (p, q, nq, npr))
    N = p.shape[0]
    w = np.ones(N, F32) if w is None else np.asarray(w, F32)
    uq, up = unit_or_zero(nq), unit_or_zero(npr)
    g = F32(1) - F32(eps)
    two = F32(2)

    def s(i, j):
        t = g * (uq[:, i] * uq[:, j] + up[:, i] * up[:, j])
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
    pmd = _cross(p, md)
    k0, k1, k2 = _cross(p, m0), _cross(p, m1), _cross(p, m2)
    pm = [np.stack([k0[:, i], k1[:, i], k2[:, i]], 1) for i in range(3)]
    r = [_cross(p, pm[i]) for i in range(3)]
    for a in (m0, md, pmd, pm[0], r[0]):
        assert a.dtype == F32
    wd = w.astype(np.float64)
    cols = [r[0][:, 0], r[0][:, 1], r[0][:, 2], pm[0][:, 0], pm[0][:, 1], pm[0][:, 2], r[1][:, 1], r[1][:, 2], pm[1][:, 0], pm[1][:, 1], pm[1][:, 2],
            r[2][:, 2], pm[2][:, 0], pm[2][:, 1], pm[2][:, 2], m0[:, 0], m0[:, 1], m0[:, 2], m1[:, 1], m1[:, 2], m2[:, 2],
            -pmd[:, 0], -pmd[:, 1], -pmd[:, 2], -md[:, 0], -md[:, 1], -md[:, 2]]
    out = np.zeros(32)
    for i, c in enumerate(cols):
        out[i] = float((wd * c.astype(np.float64)).sum())
    out[27] = float(wd.sum())
    out[28] = float((w != 0).sum())
    return out


def rel_distance(sums, ref):
    """the distance the tolerances are stated in: |A - A_ref|_F / |A_ref|_F and |b - b_ref| / max(|b_ref|, |A_ref|_F * 1e-3) -- the larger
    of the two.  (b vanishes at the true pose: its error is then measured against the size of A times a millimetre-scale step.)"""
    A, b, _, _ = lr.unpack_sums(sums)
    Ar, br, _, _ = lr.unpack_sums(ref)
    nA = np.linalg.norm(Ar)
    return float(max(np.linalg.norm(A - Ar) / nA, np.linalg.norm(b - br) / max(np.linalg.norm(br), 1e-3 * nA)))


def solve_step(sums, four_dof=False):
    """x = (omega, t) of A x = b in float64 (force4DOF: the {2..5} sub-system, roll = pitch = 0)"""
    A, b, _, _ = lr.unpack_sums(sums)
    x = np.zeros(6)
    sel = np.arange(2, 6) if four_dof else np.arange(6)
    x[sel] = np.linalg.solve(A[np.ix_(sel, sel)], b[sel])
    return x


def brute_nn(p, mp, k=1):
    """indices (N, k) and squared distances of the k nearest map points, float64, brute force (in blocks of rows)"""
    mq = mp[None, :, :3].astype(np.float64)
    idx, d2 = [], []
    for r0 in range(0, p.shape[0], 256):
        dd = ((p[r0:r0 + 256, None, :].astype(np.float64) - mq) ** 2).sum(2)
        ii = np.argsort(dd, axis=1, kind="stable")[:, :k]
        idx.append(ii)
        d2.append(np.take_along_axis(dd, ii, 1))
    return np.concatenate(idx), np.concatenate(d2)


def float32_step(sums, four_dof=False):
    """the step as the device solves it, restated: the sums rounded to float32, Cholesky and the two substitutions in float32, the rotation
    by Rodrigues' formula in float32 -- then read back as x = (omega, t) from the float32 4 x 4 (localizability_reference.step_from_T)"""
    A64, b64, _, _ = lr.unpack_sums(sums)
    sel = np.arange(2, 6) if four_dof else np.arange(6)
    A, b = A64[np.ix_(sel, sel)].astype(F32), b64[sel].astype(F32)
    n = sel.size
    L, iL = np.zeros((n, n), F32), np.zeros(n, F32)     # (solve.h: chol_solve -- one reciprocal per pivot, multiplied through)
    for j in range(n):
        d = A[j, j]
        for k in range(j):
            d = F32(d - L[j, k] * L[j, k])
        L[j, j] = np.sqrt(d)
        iL[j] = F32(1) / L[j, j]
        for i in range(j + 1, n):
            v = A[i, j]
            for k in range(j):
                v = F32(v - L[i, k] * L[j, k])
            L[i, j] = F32(v * iL[j])
    y = np.zeros(n, F32)
    for i in range(n):
        v = b[i]
        for k in range(i):
            v = F32(v - L[i, k] * y[k])
        y[i] = F32(v * iL[i])
    xs = np.zeros(n, F32)
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v = F32(v - L[k, i] * xs[k])
        xs[i] = F32(v * iL[i])
    x = np.zeros(6, F32)
    x[sel] = xs
    om = x[:3]
    th = F32(np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]))
    T = np.eye(4, dtype=F32)
    if th > 0:
        a = om / th
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], F32)
        T[:3, :3] = (np.eye(3, dtype=F32) + F32(np.sin(th)) * K + F32(F32(1) - F32(np.cos(th))) * (K @ K)).astype(F32)
    T[:3, 3] = x[3:]
    return lr.step_from_T(T)


def cauchy_weights(d2, tuning=1.0):
    """RobustOutlierFilter{robustFct: cauchy, scaleEstimator: none, distanceType: point2point}: w = 1 / (1 + d2 / tuning^2) in float32"""
    d2 = np.asarray(d2, F32)
    k2 = F32(tuning) * F32(tuning)
    return (F32(1) / (F32(1) + d2 / k2)).astype(F32)


_nn_cache = {}
K_MAX = 3


def centred_scene(name):
    """map and reading of a scene as a registration centres them: minus the map's mean, in float32 (T of the tests lives in this frame)"""
    sc = lr.scene(name)
    mean = sc["map"][:, :3].astype(np.float64).mean(0).astype(F32)
    mc, rc = sc["map"].copy(), sc["reading"].copy()
    mc[:, :3] = sc["map"][:, :3] - mean[None, :]
    rc[:, :3] = sc["reading"][:, :3] - mean[None, :]
    return mc, rc


def scene_pairs(name, T, k=1, max_dist=2.0, trimmed=None, cauchy=None):
    """the pairs of one iteration on scene `name` under pose T, by brute force in float64 on the float32 clouds: dict(p, q, nq, npr, w)
    flattened over the k matches; trimmed = ratio of TrimmedDist (None: MaxDist alone); cauchy = tuning of a Robust filter behind them"""
    sc = lr.scene(name)
    mc, rc = centred_scene(name)
    T32 = np.asarray(T, F32)
    key = (name, T32.tobytes())
    if key not in _nn_cache:     # (the search is the slow part: once per scene and pose, K_MAX neighbours)
        p = xf_points(T32, rc)
        _nn_cache[key] = (p, rot_normals(T32, sc["reading_normals"])) + brute_nn(p, mc, K_MAX)
    assert k <= K_MAX
    p, npr, idx, d2 = _nn_cache[key]
    idx, d2 = idx[:, :k], d2[:, :k]
    w = (d2 <= max_dist * max_dist).astype(np.float64)
    if trimmed is not None:
        flat = np.sort(d2.ravel())
        limit = flat[min(flat.size - 1, int(trimmed * flat.size))]
        w *= d2 <= limit
    if cauchy is not None:
        w *= np.where(np.isfinite(d2), cauchy_weights(d2, cauchy).astype(np.float64), 0.0)
    rep = lambda a: np.repeat(a, k, axis=0)
    return dict(p=rep(p), q=mc[idx.ravel(), :3], nq=sc["normals"][idx.ravel()], npr=rep(npr), w=w.ravel())
