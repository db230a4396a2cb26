"""CovarianceSamplingDataPointsFilter{nbSample, torqueNorm} restated in numpy float64 from the formulation as recalled
(include/icpmi.h, icpmi_covariance_sampling), not from the kernels.  Every elementwise step is one IEEE double
operation in the order the formulation pins (numpy contracts nothing), so keys and weights computed from the same c, L and basis
are the device's bits: `covariance_sampling(..., info=device_info)` replays the device's selection exactly.  Without `info` the
restatement computes its own c, L (numpy sums) and eigenbasis (numpy.linalg.eigh, ascending)."""
import numpy as np

F = np.float32
D = np.float64


def center_and_lnorm(xyz, torque_norm):
    """c (3,) and L of the torque normalisation: 0 -> 1, 1 -> mean |p - c|, 2 -> half the largest bounding-box extent; L == 0 -> 1"""
    p = np.asarray(xyz, F)[:, :3].astype(D)
    n = p.shape[0]
    c = p.sum(0) / n
    if torque_norm == 0:
        L = 1.0
    elif torque_norm == 1:
        a = p - c
        L = float(np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).sum() / n)
    elif torque_norm == 2:
        L = 0.5 * float((p.max(0) - p.min(0)).max())
    else:
        raise ValueError("torqueNorm must be 0, 1 or 2")
    return c, (1.0 if L == 0.0 else L)


def vectors(xyz, normals, c, L):
    """v_i = [ s ((p_i - c) x n_i) ; n_i ], s = 1.0 / L, (n, 6)"""
    p = np.asarray(xyz, F)[:, :3].astype(D)
    b = np.asarray(normals, F).reshape(-1, 3).astype(D)
    c = np.asarray(c, D)
    a = p - c
    tx = (a[:, 1] * b[:, 2]) - (a[:, 2] * b[:, 1])
    ty = (a[:, 2] * b[:, 0]) - (a[:, 0] * b[:, 2])
    tz = (a[:, 0] * b[:, 1]) - (a[:, 1] * b[:, 0])
    s = 1.0 / L
    return np.stack([s * tx, s * ty, s * tz, b[:, 0], b[:, 1], b[:, 2]], 1)


def covariance(v):
    return v.T @ v


def eigenbasis(C):
    """(eigenvalues ascending, X) with column k of X = x_k"""
    return np.linalg.eigh(C)


def projections(v, X):
    """m[i, k] = v_i . x_k, summed left to right over j = 0 .. 5"""
    m = v[:, 0:1] * X[0][None, :]
    for j in range(1, 6):
        m = m + v[:, j:j + 1] * X[j][None, :]
    return m


def sorted_lists(m):
    """list k: every index sorted by (float)|m[:, k]| descending; ties in ascending index order (stable)"""
    key = np.abs(m).astype(F)
    return [np.argsort(-key[:, k], kind="stable") for k in range(6)]


def greedy(lists, w, nb):
    """nb picks: k = first argmin of t, the front unselected point of list k, t_j += w[pick, j] in j order"""
    n = w.shape[0]
    lists = [l.tolist() for l in lists]
    wl = w.tolist()
    sel = bytearray(n)
    head = [0] * 6
    t = [0.0] * 6
    out = []
    for _ in range(nb):
        k = min(range(6), key=t.__getitem__)
        lk = lists[k]
        h = head[k]
        while sel[lk[h]]:
            h += 1
        i = lk[h]
        head[k] = h + 1
        sel[i] = 1
        out.append(i)
        wi = wl[i]
        for j in range(6):
            t[j] += wi[j]
    return np.asarray(out, np.int64)


def covariance_sampling(xyz, normals, nb, torque_norm=1, info=None):
    """-> (order, {center, lnorm, eigval, basis}) of CovarianceSamplingDataPointsFilter.  info (a dict with center, lnorm and basis,
    column k = x_k) replays from the given c, L and basis; without it the restatement computes its own."""
    n = np.asarray(xyz).shape[0]
    if nb >= n:
        return np.arange(n, dtype=np.int64), None
    if normals is None:
        raise KeyError("normals")
    if info is None:
        c, L = center_and_lnorm(xyz, torque_norm)
        v = vectors(xyz, normals, c, L)
        ev, X = eigenbasis(covariance(v))
        info = {"center": c, "lnorm": L, "eigval": ev, "basis": X}
    else:
        v = vectors(xyz, normals, info["center"], info["lnorm"])
        X = np.asarray(info["basis"], D)
    m = projections(v, X)
    return greedy(sorted_lists(m), m * m, nb), info
