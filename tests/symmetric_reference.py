"""Float64 restatement of the symmetric point-to-plane pair sums (include/icpmi.h: ICPMI_PLANE_MODEL_SYMMETRIC), a float32
restatement of the same specification, registration loops over brute-force nearest neighbours in both precisions, and the closed curved
scene `ellipsoid`.  Pure numpy: nothing here touches the library.

For a pair with weight w != 0: p = T x, q its match, u_q = unit_or_zero(n_q), u_p = unit_or_zero(R n_x), c = u_q . u_p,
    n_s = ( |c| u_q + c u_p ) / 2        (u_p = 0: n_s = u_q;  u_q = 0: n_s = u_p;  both 0: the pair only counts)
and then the point-to-plane sums with n_s for the normal (localizability_reference.pair_sums):
    F = [p x n_s; n_s],  A += w F F^T (upper 21 -> slots 0..20),  b -= w F ((p - q) . n_s) (slots 21..26),  slot 27 = sum w, slot 28 = pairs
"""
import numpy as np

import localizability_reference as lr
import plane_to_plane_reference as pp

F32 = np.float32
ELLIPSOID_AXES = (4.0, 10.0, 1.5)
SCENES = ("room", "corridor", "tunnel", "ellipsoid")
MAX_DIST, TRIMMED = 2.0, 0.85           # the chain of the registration loops: brute-force k = 1, maxDist 2, TrimmedDist 0.85
DIFFERENTIAL = dict(min_rot=1e-3, min_trans=1e-3, smooth=3)

_cache = {}


def scene(name, m=8000, n=2000):
    """lr.scene, plus `ellipsoid`: unit directions v from default_rng(7).normal (map first, then reading, one generator), points
    v * (4, 10, 1.5), inward unit normals -x / a^2 normalised; float32 clouds.  Callers must not write into the arrays."""
    if name != "ellipsoid":
        return lr.scene(name, m, n)
    key = (name, m, n)
    if key not in _cache:
        rng = np.random.default_rng(7)
        a = np.asarray(ELLIPSOID_AXES)

        def sample(count):
            v = rng.normal(size=(count, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            x = v * a
            nn = -x / (a * a)
            return x, nn / np.linalg.norm(nn, axis=1, keepdims=True)

        mp, mn = sample(m)
        rd, rn = sample(n)
        f4 = lambda c: np.concatenate([c, np.ones((c.shape[0], 1))], 1).astype(F32)
        out = dict(map=f4(mp), normals=mn.astype(F32), reading=f4(rd), reading_normals=rn.astype(F32))
        for arr in out.values():
            arr.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def pair_normals(nq, npr):
    """n_s (N, 3) in the dtype of nq (float32: the operations and their order are the kernel's); npr = the reading's normals ALREADY rotated"""
    nq, npr = np.asarray(nq), np.asarray(npr, np.asarray(nq).dtype)
    t = nq.dtype.type
    uq, up = pp.unit_or_zero(nq), pp.unit_or_zero(npr)
    hq, hp = (uq != 0).any(1), (up != 0).any(1)
    c = uq[:, 0] * up[:, 0] + uq[:, 1] * up[:, 1] + uq[:, 2] * up[:, 2]
    ac = np.abs(c)
    ns = t(0.5) * (ac[:, None] * uq + c[:, None] * up)
    ns = np.where(hq[:, None], ns, up)
    ns = np.where(hp[:, None], ns, uq)
    assert ns.dtype == nq.dtype
    return ns


def reference_sums(p, q, nq, npr, w=None):
    """the float64 reference: p (N, 3) transformed reading points, q their matches, nq the matches' normals, npr the reading's normals
    ALREADY rotated, w the weights (pairs with w == 0 do not count)"""
    p = np.asarray(p, np.float64)
    w = np.ones(p.shape[0]) if w is None else np.asarray(w, np.float64)
    ns = pair_normals(np.asarray(nq, np.float64), np.asarray(npr, np.float64))
    A, b, W = lr.pair_sums(p, q, ns, w)
    return lr.pack_sums(A, b, W, int((w != 0).sum()))


def float32_sums(p, q, nq, npr, w=None):
    """the specification as the kernel evaluates it: every per-pair quantity in float32 (no contraction), the weight's product and the sums
    in float64.  Differs from the kernel by the order of the double sums only."""
    p, q, nq, npr = (np.asarray(a, F32) for a in (p, q, nq, npr))
    w = np.ones(p.shape[0], F32) if w is None else np.asarray(w, F32)
    nn = pair_normals(nq, npr)
    Fm = np.stack([p[:, 1] * nn[:, 2] - p[:, 2] * nn[:, 1], p[:, 2] * nn[:, 0] - p[:, 0] * nn[:, 2], p[:, 0] * nn[:, 1] - p[:, 1] * nn[:, 0],
                   nn[:, 0], nn[:, 1], nn[:, 2]], 1)
    d = p - q
    dot = d[:, 0] * nn[:, 0] + d[:, 1] * nn[:, 1] + d[:, 2] * nn[:, 2]
    assert Fm.dtype == F32 and dot.dtype == F32
    wd = w.astype(np.float64)
    out = np.zeros(32)
    idx = 0
    for a in range(6):
        wf = wd * Fm[:, a].astype(np.float64)
        for b in range(a, 6):
            out[idx] = float((wf * Fm[:, b].astype(np.float64)).sum())
            idx += 1
        out[21 + a] = -float((wf * dot.astype(np.float64)).sum())
    out[27] = float(wd.sum())
    out[28] = float((w != 0).sum())
    return out


def rel_step(x, ref):
    """|x - ref| / max(|ref|, 1e-3) of two steps (omega, t): the step vanishes at the true pose of a scene of planes (same-face pairs have a
    zero residual, pairs across a corner a zero pair normal), where the error is measured against a millimetre-scale step -- as
    plane_to_plane_reference.rel_distance measures b"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-3))


# ------------------------------------------------------------------------------------------------------------------ pairs of one iteration
_nn_cache = {}
K_MAX = 3


def brute_nn(p, mp, k=1):
    """indices (N, k) and squared distances of the k nearest map points in float64, brute force: candidates by |p|^2 + |m|^2 - 2 p . m (one
    matrix product; k + 4 of them per query, which absorbs its cancellation error of about 1e-13 m^2), then their distances formed exactly as
    plane_to_plane_reference.brute_nn forms them, and sorted (stable, by index among equals)"""
    p, m = np.asarray(p, np.float64)[:, :3], np.asarray(mp, np.float64)[:, :3]
    kc = min(k + 4, m.shape[0])
    dd = (p * p).sum(1)[:, None] + (m * m).sum(1)[None, :] - 2.0 * (p @ m.T)
    cand = np.sort(np.argpartition(dd, kc - 1, axis=1)[:, :kc], axis=1)
    d2 = ((p[:, None, :] - m[cand]) ** 2).sum(2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(cand, order, 1), np.take_along_axis(d2, order, 1)


def centred_scene(name):
    """map and reading of a scene as a registration centres them: minus the map's mean, in float32 (T of the tests lives in this frame)"""
    sc = scene(name)
    mean = sc["map"][:, :3].astype(np.float64).mean(0).astype(F32)
    mc, rc = sc["map"].copy(), sc["reading"].copy()
    mc[:, :3] = sc["map"][:, :3] - mean[None, :]
    rc[:, :3] = sc["reading"][:, :3] - mean[None, :]
    return mc, rc


def chain_weights(d2, max_dist=MAX_DIST, trimmed=None, cauchy=None):
    """MaxDist, then TrimmedDist{ratio} over all pairs, then a cauchy Robust filter: float64 weights in the shape of d2"""
    w = (d2 <= max_dist * max_dist).astype(np.float64)
    if trimmed is not None:
        flat = np.sort(d2.ravel())
        w *= d2 <= flat[min(flat.size - 1, int(trimmed * flat.size))]
    if cauchy is not None:
        w *= np.where(np.isfinite(d2), pp.cauchy_weights(d2, cauchy).astype(np.float64), 0.0)
    return w


def scene_pairs(name, T, k=1, max_dist=MAX_DIST, trimmed=None, cauchy=None):
    """the pairs of one iteration on scene `name` under pose T, by brute force in float64 on the float32 clouds: dict(p, q, nq, npr, w)
    flattened over the k matches (plane_to_plane_reference.scene_pairs, on this module's scenes)"""
    sc = scene(name)
    mc, rc = centred_scene(name)
    T32 = np.asarray(T, F32)
    key = (name, T32.tobytes())
    if key not in _nn_cache:     # (the search is the slow part: once per scene and pose, K_MAX neighbours)
        p = pp.xf_points(T32, rc)
        _nn_cache[key] = (p, pp.rot_normals(T32, sc["reading_normals"])) + brute_nn(p, mc, K_MAX)
    assert k <= K_MAX
    p, npr, idx, d2 = _nn_cache[key]
    idx, d2 = idx[:, :k], d2[:, :k]
    w = chain_weights(d2, max_dist, trimmed, cauchy)
    rep = lambda a: np.repeat(a, k, axis=0)
    return dict(p=rep(p), q=mc[idx.ravel(), :3], nq=sc["normals"][idx.ravel()], npr=rep(npr), w=w.ravel())


# ------------------------------------------------------------------------------------------------------------------ registration loops
def moved_reading(sc, T):
    """the reading and its normals moved by T (float64 4 x 4): registering it must answer T^-1"""
    rd = sc["reading"].copy()
    rd[:, :3] = (sc["reading"][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F32)
    rn = (sc["reading_normals"].astype(np.float64) @ T[:3, :3].T).astype(F32)
    return rd, rn


def pose_error(T, T_true):
    """(|translation|, |rotation|) of T T_true^-1"""
    D = np.asarray(T, np.float64) @ np.linalg.inv(T_true)
    return float(np.linalg.norm(D[:3, 3])), float(np.linalg.norm(lr.step_from_T(D)[:3]))


def _float32_step_T(sums):
    """the 4 x 4 of plane_to_plane_reference.float32_step's x: a float32 rotation by Rodrigues' formula from the float32 solve"""
    x = pp.float32_step(sums)
    return lr.make_T(x[:3], x[3:]).astype(F32)


_loop_cache = {}


def register(name, T_move, model="symmetric", precision=64, iterations=12):
    """_register, computed once per argument set (the loops are the slow part of the tests that share them; callers must not write into the poses)"""
    key = (name, np.asarray(T_move, np.float64).tobytes(), model, precision, iterations)
    if key not in _loop_cache:
        _loop_cache[key] = _register(name, T_move, model, precision, iterations)
    return _loop_cache[key]


def _register(name, T_move, model, precision, iterations):
    """ICP of scene `name`'s reading moved by T_move against its map, from the identity: brute-force k = 1, maxDist 2, TrimmedDist 0.85.
    model: "symmetric" | "point_to_plane" (the map's normal alone).  precision 64: float64 sums and solve on the float32 clouds; 32: the
    float32 restatements (float32_sums, plane_to_plane_reference.float32_step, float32 pose products).  Returns the poses after every
    iteration, in the frame of the clouds as given (list of float64 4 x 4): the answer is T_move^-1."""
    assert model in ("symmetric", "point_to_plane") and precision in (32, 64)
    sc = scene(name)
    rd, rn = moved_reading(sc, np.asarray(T_move, np.float64))
    mean = sc["map"][:, :3].astype(np.float64).mean(0).astype(F32)
    mc = sc["map"][:, :3] - mean[None, :]
    rc = rd.copy()
    rc[:, :3] = rd[:, :3] - mean[None, :]
    wdt = F32 if precision == 32 else np.float64
    T = np.eye(4, dtype=wdt)
    zero = np.zeros_like(rn)
    out = []
    for _ in range(iterations):
        if precision == 32:
            p, npr = pp.xf_points(T, rc), pp.rot_normals(T, rn)
        else:
            p = rc[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            npr = rn.astype(np.float64) @ T[:3, :3].T
        idx, d2 = brute_nn(p, mc, 1)
        w = chain_weights(d2, MAX_DIST, TRIMMED).ravel()
        q, nq = mc[idx.ravel()], sc["normals"][idx.ravel()]
        if model == "point_to_plane":       # (no surface model on the reading side; the map's normal as given: it has unit length)
            npr = zero
        if precision == 32:
            Ts = _float32_step_T(float32_sums(p, q, nq, npr, w))
            T = (Ts @ T).astype(F32)
        else:
            x = pp.solve_step(reference_sums(p, q, nq, npr, w))
            T = lr.make_T(x[:3], x[3:]) @ T
        # centred frame -> the clouds' frame: x_c = x - mean
        Tw = np.array(T, np.float64)
        Tw[:3, 3] = Tw[:3, 3] + mean.astype(np.float64) - Tw[:3, :3] @ mean.astype(np.float64)
        out.append(Tw)
    return out


def differential_stop(poses, min_rot=1e-3, min_trans=1e-3, smooth=3):
    """index into `poses` of the iteration at which DifferentialTransformationChecker stops (the mean of the last `smooth` steps, the first
    of them measured from the identity, under both thresholds), or None"""
    hist = [np.eye(4)] + list(poses)
    rot, tr = [], []
    for a, b in zip(hist[1:], hist[:-1]):
        rot.append(np.linalg.norm(lr.step_from_T(a @ np.linalg.inv(b))[:3]))
        tr.append(np.linalg.norm(a[:3, 3] - b[:3, 3]))
        if len(rot) >= smooth and np.mean(rot[-smooth:]) < min_rot and np.mean(tr[-smooth:]) < min_trans:
            return len(rot) - 1
    return None
