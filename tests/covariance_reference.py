"""float64 numpy restatement of PointToPlaneWithCovErrorMinimizer's covariance as include/icpmi.h (icpmi_get_covariance) writes it down.

Pairs in the centred frame: p (reading point under T_prev), q (matched map point), n (its normal); x = (tx, ty, tz, alpha, beta, gamma)
of the last step T_s = T_iter T_prev^-1.  Cov = sigma^2 H^-1 S H^-1 with H = sum h h^T, S = sum (a a^T + b b^T)."""
import numpy as np

SENTINEL = np.float32(np.finfo(np.float32).max)


def step_params(T_iter, T_prev):
    """(tx, ty, tz, alpha, beta, gamma) of T_s = T_iter T_prev^-1, T_prev^-1 = [R^T | -R^T t] (4 x 4 row-major inputs)"""
    A = np.asarray(T_iter, np.float64)
    P = np.asarray(T_prev, np.float64)
    R = A[:3, :3] @ P[:3, :3].T
    t = A[:3, 3] - R @ P[:3, 3]
    beta = -np.arcsin(R[2, 0])
    cb = np.cos(beta)
    return np.array([t[0], t[1], t[2], np.arctan2(R[2, 1], R[2, 2]), beta, np.arctan2(R[1, 0] / cb, R[0, 0] / cb)])


def _L(v, x):
    """L v = v + (alpha, beta, gamma) x v, row by row"""
    return v + np.cross(np.broadcast_to(x[3:6], v.shape), v)


def terms(p, q, n, x):
    """per pair: h, a, b (each (P, 6)) and E"""
    p, q, n = (np.asarray(v, np.float64) for v in (p, q, n))
    r = np.linalg.norm(p, axis=1)[:, None]
    rho = np.linalg.norm(q, axis=1)[:, None]
    d, u = p / r, q / rho
    c = np.cross(d, n)
    E = (n * (_L(p, x) + x[:3] - q)).sum(1)[:, None]
    Nr = (n * _L(d, x)).sum(1)[:, None]
    Nq = -(n * u).sum(1)[:, None]
    h = np.concatenate([n, r * c], 1)
    a = np.concatenate([n * Nr, c * (E + r * Nr)], 1)
    b = np.concatenate([n * Nq, r * c * Nq], 1)
    return h, a, b, E[:, 0]


def sums(p, q, n, x):
    h, a, b, _ = terms(p, q, n, x)
    return h.T @ h, a.T @ a + b.T @ b


def covariance(p, q, n, x, sigma):
    """(Cov float64 or None when H is not positive definite, H, S)"""
    H, S = sums(p, q, n, x)
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None, H, S
    Hi = np.linalg.inv(H)
    cov = float(sigma) ** 2 * (Hi @ S @ Hi)
    return 0.5 * (cov + cov.T), H, S


def covariance_f32(p, q, n, x, sigma):
    """what the device returns: float32, FLT_MAX I when H is not positive definite"""
    cov, _, _ = covariance(p, q, n, x, sigma)
    if cov is None:
        return np.eye(6, dtype=np.float32) * SENTINEL
    return cov.astype(np.float32)


def gradient(x, r, rho, d, u, n):
    """half the gradient of the linearised cost sum E^2 by x, with p = r d and q = rho u"""
    p, q = r[:, None] * d, rho[:, None] * u
    E = (n * (_L(p, x) + x[:3] - q)).sum(1)
    h = np.concatenate([n, np.cross(p, n)], 1)
    return (E[:, None] * h).sum(0)


def rel_tol(H, npairs):
    """device vs restatement over the same float32 pairs and the same T_s: the float32 rounding of the result plus the double sums'
    rounding amplified by the conditioning of H (Cov = H^-1 S H^-1 moves by ~2 cond(H) times a relative change of H)"""
    return 2.0 ** -20 + 4.0 * np.linalg.cond(H) * max(npairs, 1) * 2.0 ** -52


def fma_transform(T, pts4):
    """xf_point of the library: o = fma(T[:,3], w, fma(T[:,2], z, fma(T[:,1], y, T[:,0] x))) per row, float32; float32 products are
    exact in float64, so each fma is one float64 add rounded to float32"""
    T = np.asarray(T, np.float32).astype(np.float64)
    P = np.asarray(pts4, np.float32).astype(np.float64)
    out = np.empty((P.shape[0], 3), np.float32)
    for r in range(3):
        acc = (T[r, 0] * P[:, 0]).astype(np.float32)
        for k in (1, 2, 3):
            acc = (T[r, k] * P[:, k] + acc.astype(np.float64)).astype(np.float32)
        out[:, r] = acc
    return out
