"""Float64 reference and float32 restatement of the intensity-aided point-to-plane minimiser (include/icpmi.h: icpmi_set_intensity_weight;
DESIGN.md 4.19): the map-side intensity gradients, the pair sums and a registration loop, with the scalar field and the scenes its tests run
on.  Pure numpy: nothing here touches the library.

Map side, per point i with unit normal u and its K nearest other points j (row i of `nbr`: the point itself first, -1 = unfilled):
    e1 = normalise(u x axis), axis = the coordinate axis of the smallest |u| component; e2 = u x e1
    d = (x_j - x_i) - u (u . (x_j - x_i)), a = d . e1, b = d . e2, dI = I_j - I_i;  S = sum [a b]^T [a b], r = sum [a b]^T dI
    g = (S^-1 r).x e1 + (S^-1 r).y e2;  g = 0 for a zero / non-finite normal, a non-finite I_i, fewer than 2 usable neighbours or
    det S <= 1e-4 (tr S / 2)^2
Per pair with weight w, lambda = 1 - weight:
    r_G = (p - q) . n, F_G = [p x n; n];  m = g - n (g . n), p' = p - n r_G, r_I = I_q + g . (p' - q) - I_p, F_I = [p x m; m]
    A += w (lambda F_G F_G^T + (1 - lambda) F_I F_I^T),  b -= w (lambda F_G r_G + (1 - lambda) F_I r_I)
    (a non-finite I_p or I_q: the geometric part only)
"""
import numpy as np

import localizability_reference as lr
import plane_to_plane_reference as pp
import symmetric_reference as sr

F32 = np.float32
KNN_DEFAULT = 10
WEIGHT_DEFAULT = float(F32(1.0) - F32(0.968))      # lambdaGeometric 0.968 as the handle holds its complement
NOISE_SIGMA = 0.02
SCENES = ("corridor", "room")
MAX_DIST, TRIMMED = 2.0, 0.85
DET_FLOOR = 1e-4
# the start of the registrations: 0.3 m off along the corridor's axis (y), 0.05 m / -0.04 m across it, 0.03 rad of yaw
START = lr.make_T((0.0, 0.0, 0.03), (0.05, 0.3, -0.04))
AXIS = 1


def field(xyz):
    """the scalar field the scenes' surfaces carry: periodic along the corridor's axis and across it"""
    x, y, z = (np.asarray(xyz, np.float64)[:, i] for i in range(3))
    return 0.5 + 0.25 * np.sin(2 * np.pi * y / 2.5) + 0.15 * np.sin(2 * np.pi * (x + z) / 1.7)


FIELD_GRADIENT_MAX = 2 * np.pi * (0.25 / 2.5 + 0.15 * np.sqrt(2.0) / 1.7)    # bound of |grad field|


_scene_cache = {}


def scene(name, m=8000, n=2000):
    """localizability_reference.scene(name, m, n) plus `map_intensity` (m,) and `reading_intensity` (n,): the field at the points plus Gaussian noise
    of sigma 0.02 from a fixed seed, float32.  Generated once per name; callers must not write into the arrays."""
    if (name, m, n) not in _scene_cache:
        sc = dict(lr.scene(name, m, n))
        rng = np.random.default_rng(4190 + SCENES.index(name))
        for cloud, key in (("map", "map_intensity"), ("reading", "reading_intensity")):
            v = (field(sc[cloud][:, :3]) + NOISE_SIGMA * rng.standard_normal(sc[cloud].shape[0])).astype(F32)
            v.setflags(write=False)
            sc[key] = v
        _scene_cache[(name, m, n)] = sc
    return _scene_cache[(name, m, n)]


# ------------------------------------------------------------------------------------------------------------------ neighbours
def self_knn(xyz, K, rows=None):
    """(m, K + 1) indices of every point's (rows: of those points') K + 1 nearest points of the same cloud, itself (distance 0) first, by
    brute force in float64, stable by index among equals; -1 past the cloud's size"""
    x = np.asarray(xyz, np.float64)[:, :3]
    m = x.shape[0]
    rows = np.arange(m) if rows is None else np.asarray(rows)
    out = np.full((rows.size, K + 1), -1, np.int64)
    kk = min(K + 1, m)
    step = max(1, min(512, (1 << 22) // m))
    for r0 in range(0, rows.size, step):
        dd = ((x[rows[r0:r0 + step], None, :] - x[None, :, :]) ** 2).sum(2)
        out[r0:r0 + step, :kk] = np.argsort(dd, axis=1, kind="stable")[:, :kk]
    return out


# ------------------------------------------------------------------------------------------------------------------ gradients
def _tangent_basis(u):
    """e1, e2 of unit normals u (m, 3), in u's dtype"""
    a = np.abs(u)
    ax = np.where((a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2]), 0, np.where(a[:, 1] <= a[:, 2], 1, 2))
    z = np.zeros_like(u[:, 0])
    c = np.where((ax == 0)[:, None], np.stack([z, u[:, 2], -u[:, 1]], 1),
                 np.where((ax == 1)[:, None], np.stack([-u[:, 2], z, u[:, 0]], 1), np.stack([u[:, 1], -u[:, 0], z], 1)))
    one = u.dtype.type(1)
    cinv = one / np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    e1 = c * cinv[:, None]
    e2 = np.stack([u[:, 1] * e1[:, 2] - u[:, 2] * e1[:, 1], u[:, 2] * e1[:, 0] - u[:, 0] * e1[:, 2], u[:, 0] * e1[:, 1] - u[:, 1] * e1[:, 0]], 1)
    return e1, e2


def _gradients(xyz, normals, inten, nbr, dt, rows=None):
    """the specification in dtype dt, operation for operation (every elementwise numpy operation rounds once to dt, as the kernel's float
    arithmetic does without contraction); sums in neighbour order.  rows: nbr holds the rows of these points only, and so does the answer"""
    x = np.asarray(xyz, F32)[:, :3].astype(dt)
    nbr = np.asarray(nbr)
    rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    n = np.asarray(normals, F32).astype(dt)[rows]
    Iall = np.asarray(inten, F32).astype(dt)
    I = Iall[rows]
    m = rows.size
    with np.errstate(all="ignore"):
        l2 = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        ok = (nbr[:, 0] >= 0) & (l2 > 0) & np.isfinite(l2) & np.isfinite(I)
        inv = dt(1) / np.sqrt(np.where(ok, l2, dt(1)))
        u = n * inv[:, None]
        u[~ok] = np.array([1, 0, 0], dt)          # (never used: ok gates the result)
        e1, e2 = _tangent_basis(u)
        xi = x[np.where(nbr[:, 0] < 0, 0, nbr[:, 0])]
        saa = np.zeros(m, dt); sab = np.zeros(m, dt); sbb = np.zeros(m, dt); ra = np.zeros(m, dt); rb = np.zeros(m, dt)
        used = np.zeros(m, np.int64)
        for j in range(1, nbr.shape[1]):
            s = nbr[:, j]
            safe = np.where(s < 0, 0, s)
            Ij = Iall[safe]
            use = ok & (s >= 0) & np.isfinite(Ij)
            d = x[safe] - xi
            t = d[:, 0] * u[:, 0] + d[:, 1] * u[:, 1] + d[:, 2] * u[:, 2]
            pr = d - u * t[:, None]
            a = pr[:, 0] * e1[:, 0] + pr[:, 1] * e1[:, 1] + pr[:, 2] * e1[:, 2]
            b = pr[:, 0] * e2[:, 0] + pr[:, 1] * e2[:, 1] + pr[:, 2] * e2[:, 2]
            dI = Ij - I
            saa = np.where(use, saa + a * a, saa); sab = np.where(use, sab + a * b, sab); sbb = np.where(use, sbb + b * b, sbb)
            ra = np.where(use, ra + a * dI, ra); rb = np.where(use, rb + b * dI, rb)
            used += use
        det = saa * sbb - sab * sab
        htr = (saa + sbb) * dt(0.5)
        good = ok & (used >= 2) & (det > dt(F32(DET_FLOOR)) * (htr * htr))
        sd = np.where(good, det, dt(1))
        g2x = (sbb * ra - sab * rb) / sd
        g2y = (saa * rb - sab * ra) / sd
        g = g2x[:, None] * e1 + g2y[:, None] * e2
    g[~good] = 0
    return g


def gradient_reference(xyz, normals, inten, nbr, rows=None):
    """(m, 3) float64 gradients on the float32 inputs"""
    return _gradients(xyz, normals, inten, nbr, np.float64, rows)


def gradient_float32(xyz, normals, inten, nbr, rows=None):
    """the float32 restatement of intensity_gradient_kernel"""
    return _gradients(xyz, normals, inten, nbr, F32, rows)


def gradient_distance(g, ref, floor):
    """largest over the points of |g - ref| / (|ref| + floor)"""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    return float((np.linalg.norm(g - ref, axis=1) / (np.linalg.norm(ref, axis=1) + floor)).max()) if len(ref) else 0.0


# ------------------------------------------------------------------------------------------------------------------ pair sums
def _lambda(weight):
    return 1.0 - float(F32(weight))


def reference_sums(p, q, n, g, Iq, Ip, w, weight):
    """the 32 sums of one iteration in float64 on whatever precision the inputs carry, packed like localizability_reference.unpack_sums reads
    them.  The geometric part IS localizability_reference.pair_sums with the weights w lambda; weight 0 adds nothing to it."""
    p, q, n, g, Iq, Ip, w = (np.asarray(a, np.float64) for a in (p, q, n, g, Iq, Ip, w))
    lam = _lambda(weight)
    A, b, _ = lr.pair_sums(p, q, n, w * lam)
    ok = np.isfinite(Iq) & np.isfinite(Ip)
    wi = np.where(ok, w * (1.0 - lam), 0.0)
    if (wi != 0).any():
        rg = ((p - q) * n).sum(1)
        mm = g - n * (g * n).sum(1)[:, None]
        e = (p - q) - n * rg[:, None]
        with np.errstate(invalid="ignore"):
            ri = np.where(ok, Iq + (g * e).sum(1) - Ip, 0.0)
        FI = np.concatenate([np.cross(p, mm), mm], axis=1)
        A = A + (FI * wi[:, None]).T @ FI
        b = b - (FI * (wi * ri)[:, None]).sum(0)
    return lr.pack_sums(A, b, float(w.sum()), int((w != 0).sum()))


def _cross32(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def float32_sums(p, q, n, g, Iq, Ip, w, weight):
    """the pair sums as accumulate_kernel<PAIR_INTENSITY> forms them: per-pair terms in float32, the weight's products and the sums in double
    (the order of the double sum is numpy's, the one thing that differs from the device)"""
    p, q, n, g, Iq, Ip = (np.asarray(a, F32) for a in (p, q, n, g, Iq, Ip))
    w = np.asarray(w, F32)
    wi32 = F32(weight)
    lam32 = F32(1) - wi32
    out = np.zeros(32)
    FG = np.concatenate([_cross32(p, n), n], 1)
    d = p - q
    dot = d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1] + d[:, 2] * n[:, 2]
    wg = w.astype(np.float64) * float(lam32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(Iq) & np.isfinite(Ip) & (w != 0)
        gn = g[:, 0] * n[:, 0] + g[:, 1] * n[:, 1] + g[:, 2] * n[:, 2]
        mm = g - n * gn[:, None]
        e = d - n * dot[:, None]
        ri = (Iq + (g[:, 0] * e[:, 0] + g[:, 1] * e[:, 1] + g[:, 2] * e[:, 2])) - Ip
    FI = np.concatenate([_cross32(p, mm), mm], 1)
    wp = np.where(ok, w.astype(np.float64) * float(wi32), 0.0)
    ri = np.where(ok, ri, F32(0))
    FI = np.where(ok[:, None], FI, F32(0))
    photometric = bool((wp != 0).any())          # (no pair with the term: nothing is added, not even a +0 to a -0)
    idx = 0
    for a in range(6):
        wfg = wg * FG[:, a].astype(np.float64)
        wfi = wp * FI[:, a].astype(np.float64)
        for b in range(a, 6):
            out[idx] = float((wfg * FG[:, b].astype(np.float64)).sum())
            if photometric:
                out[idx] += float((wfi * FI[:, b].astype(np.float64)).sum())
            idx += 1
        out[21 + a] = -float((wfg * dot.astype(np.float64)).sum())
        if photometric:
            out[21 + a] -= float((wfi * ri.astype(np.float64)).sum())
    out[27] = float(w.astype(np.float64).sum())
    out[28] = float((w != 0).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ pairs of one iteration
_nn_cache = {}
_grad_cache = {}
_nbr_cache = {}
K_MAX = 3


def map_gradients(name, precision=64, K=KNN_DEFAULT):
    """the gradients of the scene's map as a registration centres it (what the index holds), brute-force neighbours: once per (scene,
    precision, K)"""
    key = (name, precision, K)
    if key not in _grad_cache:
        sc = scene(name)
        mc = centred(name)[0]
        if (name, K) not in _nbr_cache:
            _nbr_cache[(name, K)] = self_knn(mc, K)
        fn = gradient_float32 if precision == 32 else gradient_reference
        _grad_cache[key] = fn(mc, sc["normals"], sc["map_intensity"], _nbr_cache[(name, K)])
    return _grad_cache[key]


def centred(name):
    """map and reading of a scene as a registration centres them (symmetric_reference.centred_scene, on this module's scenes)"""
    sc = scene(name)
    mean = sc["map"][:, :3].astype(np.float64).mean(0).astype(F32)
    mc, rc = sc["map"].copy(), sc["reading"].copy()
    mc[:, :3] = sc["map"][:, :3] - mean[None, :]
    rc[:, :3] = sc["reading"][:, :3] - mean[None, :]
    return mc, rc, mean


def centred_pose(T, mean):
    """a pose of the clouds' frame in the centred one: [R | t + R mu - mu]"""
    T = np.array(T, np.float64)
    mu = np.asarray(mean, np.float64)
    T[:3, 3] = T[:3, 3] + T[:3, :3] @ mu - mu
    return T


def scene_pairs(name, T, k=1, max_dist=MAX_DIST, trimmed=None, cauchy=None, precision=64, K=KNN_DEFAULT):
    """the pairs of one iteration on scene `name` under the centred-frame pose T, by brute force in float64 on the float32 clouds:
    dict(p, q, n, g, Iq, Ip, w) flattened over the k matches; g: the gradients of `precision`"""
    sc = scene(name)
    mc, rc, _ = centred(name)
    T32 = np.asarray(T, F32)
    key = (name, T32.tobytes())
    if key not in _nn_cache:
        p = pp.xf_points(T32, rc)
        _nn_cache[key] = (p,) + sr.brute_nn(p, mc, K_MAX)
    assert k <= K_MAX
    p, idx, d2 = _nn_cache[key]
    idx, d2 = idx[:, :k], d2[:, :k]
    w = sr.chain_weights(d2, max_dist, trimmed, cauchy)
    rep = lambda a: np.repeat(a, k, axis=0)
    ii = idx.ravel()
    g = map_gradients(name, precision, K)
    return dict(p=rep(p), q=mc[ii, :3], n=sc["normals"][ii], g=g[ii], Iq=sc["map_intensity"][ii], Ip=rep(sc["reading_intensity"]), w=w.ravel())


# ------------------------------------------------------------------------------------------------------------------ registration loops
_loop_cache = {}


def register(name, weight, precision=64, iterations=8, T_move=START, K=KNN_DEFAULT):
    """_register, computed once per argument set (callers must not write into the poses)"""
    key = (name, float(weight), precision, iterations, np.asarray(T_move, np.float64).tobytes(), K)
    if key not in _loop_cache:
        _loop_cache[key] = _register(name, weight, precision, iterations, np.asarray(T_move, np.float64), K)
    return _loop_cache[key]


def _register(name, weight, precision, iterations, T_move, K):
    """ICP of scene `name`'s reading moved by T_move against its map, from the identity: brute-force k = 1, maxDist 2, TrimmedDist 0.85,
    the photometric term with `weight` (0: point-to-plane).  precision 64: float64 gradients, sums and solve on the float32 clouds; 32: the
    float32 restatements.  Returns the poses after every iteration in the clouds' frame (float64 4 x 4): the answer is T_move^-1."""
    assert precision in (32, 64)
    sc = scene(name)
    rd, _ = sr.moved_reading(sc, T_move)
    mean = sc["map"][:, :3].astype(np.float64).mean(0).astype(F32)
    mc = sc["map"][:, :3] - mean[None, :]
    rc = rd.copy()
    rc[:, :3] = rd[:, :3] - mean[None, :]
    g = map_gradients(name, precision, K) if weight > 0 else np.zeros((mc.shape[0], 3))
    wdt = F32 if precision == 32 else np.float64
    T = np.eye(4, dtype=wdt)
    out = []
    for _ in range(iterations):
        p = pp.xf_points(T, rc) if precision == 32 else rc[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        idx, d2 = sr.brute_nn(p, mc, 1)
        w = sr.chain_weights(d2, MAX_DIST, TRIMMED).ravel()
        ii = idx.ravel()
        args = (p, mc[ii], sc["normals"][ii], g[ii], sc["map_intensity"][ii], sc["reading_intensity"], w, weight)
        if precision == 32:
            x = pp.float32_step(float32_sums(*args))
            T = (lr.make_T(x[:3], x[3:]).astype(F32) @ T).astype(F32)
        else:
            x = solve_or_min_norm(reference_sums(*args))
            T = lr.make_T(x[:3], x[3:]) @ T
        Tw = np.array(T, np.float64)
        Tw[:3, 3] = Tw[:3, 3] + mean.astype(np.float64) - Tw[:3, :3] @ mean.astype(np.float64)
        out.append(Tw)
    return out


def solve_or_min_norm(sums):
    """plane_to_plane_reference.solve_step; for a system without full rank (point-to-plane in the corridor: no normal has a component along
    the axis) the minimum-norm step over the eigenvalues above 6 eps_f lambda_max, the rule of the device's solve (solve.h: solve_min_norm)"""
    A, b, _, _ = lr.unpack_sums(sums)
    lam, V = np.linalg.eigh(A)
    keep = lam > 6 * lr.EPS_F * np.abs(lam).max()
    if keep.all():
        return pp.solve_step(sums)
    return (V[:, keep] * (V[:, keep].T @ b / lam[keep])[None, :]).sum(1)


def residual_pose(T, T_move=START):
    """T T_move: the identity for a perfect registration; its translation is the error in the map frame (x, y, z)"""
    return np.asarray(T, np.float64) @ np.asarray(T_move, np.float64)
