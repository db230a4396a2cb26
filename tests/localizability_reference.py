"""Float64 restatement of the degeneracy-aware point-to-plane solve (include/icpmi.h: icpmi_get_localizability; csrc/solve.h: degen_*),
with numpy.linalg.eigh, and the analytic scenes its tests run on.  Pure numpy: nothing here touches the library.

The quantity, for one iteration with pair sums A (6 x 6), b (6), W = sum w and unknown x = (omega, t):
  c = T c0 (c0 = mean of the reading, T = the pose the pairs were formed under), L = mean |p - c0| (1 when 0)
  1. pivot     K = [[I, -[c]x], [0, I]]; A_c = K A K^T, b_c = K b
  2. scale     S = diag(1/L, 1/L, 1/L, 1, 1, 1); A_s = S A_c S, b_s = S b_c
  3. decompose force_4dof: the {2, 3, 4, 5} sub-system (n = 4), else n = 6; eigenpairs ascending, mu = lambda / W
  4. classify  degenerate when mu <= threshold or lambda <= n eps_f lambda_max
  5. step      y = sum over the others of v (v . b_s) / lambda; omega = y_omega / L, t = y_t - omega x c
"""
import numpy as np

EPS_F = 1.1920928955078125e-07
THRESHOLD = 5e-3          # what the tests run with: the scenes' informative mu are >= 5x above, the degenerate ones >= 5x below
SCENES = ("room", "corridor", "floor_ceiling", "floor", "tunnel")
N_DEGENERATE = {"room": 0, "corridor": 1, "floor_ceiling": 3, "floor": 3, "tunnel": 2}          # 6-DOF
N_DEGENERATE_4DOF = {"room": 0, "corridor": 1, "floor_ceiling": 3, "floor": 3, "tunnel": 1}    # yaw + translation


def skew(c):
    return np.array([[0.0, -c[2], c[1]], [c[2], 0.0, -c[0]], [-c[1], c[0], 0.0]])


def unpack_sums(sums):
    """sums[32] of icpmi_minimize_step / icpmi_debug_last_sums -> A (6 x 6), b (6), W, pairs"""
    s = np.asarray(sums, np.float64)
    A = np.zeros((6, 6))
    idx = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = s[idx]
            idx += 1
    return A, s[21:27].copy(), float(s[27]), int(round(s[28]))


def pack_sums(A, b, W, pairs):
    s = np.zeros(32)
    idx = 0
    for a in range(6):
        for bb in range(a, 6):
            s[idx] = A[a, bb]
            idx += 1
    s[21:27] = b
    s[27] = W
    s[28] = pairs
    return s


def pair_sums(p, q, n, w=None):
    """A = sum w F F^T, b = -sum w F ((p - q) . n), F = [p x n; n] -- float64 on whatever precision the inputs carry"""
    p, q, n = (np.asarray(a, np.float64) for a in (p, q, n))
    w = np.ones(p.shape[0]) if w is None else np.asarray(w, np.float64)
    F = np.concatenate([np.cross(p, n), n], axis=1)
    e = ((p - q) * n).sum(1)
    A = (F * w[:, None]).T @ F
    b = -(F * (w * e)[:, None]).sum(0)
    return A, b, float(w.sum())


def reading_stats(xyz):
    """c0 and L of a reading (the frame the registration centres it in is the caller's business)"""
    xyz = np.asarray(xyz, np.float64)[:, :3]
    c0 = xyz.sum(0) / xyz.shape[0]
    L = float(np.linalg.norm(xyz - c0, axis=1).sum() / xyz.shape[0])
    return c0, (1.0 if L == 0.0 else L)


def pivot(T, c0):
    T = np.asarray(T, np.float64)
    return T[:3, :3] @ np.asarray(c0, np.float64) + T[:3, 3]


def localizability_reference(A, b, W, c, L, threshold, four_dof=False):
    """steps 1 - 5.  Returns n, mu (n, ascending), lam, V ((6, n): eigenvectors in the full pivoted, scaled coordinates), degenerate (n
    bools), y (6, the scaled step), x (6 = (omega, t), float64), P_kept ((6, 6) projector onto the kept span)"""
    A, b, c = np.asarray(A, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    K = np.eye(6)
    K[:3, 3:] = -skew(c)
    S = np.diag([1.0 / L] * 3 + [1.0] * 3)
    As = S @ (K @ A @ K.T) @ S
    bs = S @ (K @ b)
    sel = np.arange(2, 6) if four_dof else np.arange(6)
    n = sel.size
    lam, v = np.linalg.eigh(0.5 * (As + As.T)[np.ix_(sel, sel)])
    V = np.zeros((6, n))
    V[sel, :] = v
    mu = lam / W if W > 0 else np.zeros(n)
    deg = ~(mu > threshold) | ~(lam > n * EPS_F * lam.max())
    y = np.zeros(6)
    for e in range(n):
        if not deg[e]:
            y += V[:, e] * (V[:, e] @ bs) / lam[e]
    om = y[:3] / L
    x = np.concatenate([om, y[3:] - np.cross(om, c)])
    Vk = V[:, ~deg]
    return dict(n=n, mu=mu, lam=lam, V=V, degenerate=deg, n_degenerate=int(deg.sum()), y=y, x=x, P_kept=Vk @ Vk.T, bs=bs)


def scaled_step(x, c, L):
    """x = (omega, t) -> y = (omega L, t + omega x c): the coordinates the eigenvectors live in"""
    x = np.asarray(x, np.float64)
    return np.concatenate([x[:3] * L, x[3:] + np.cross(x[:3], c)])


def step_from_T(T):
    """x = (omega, t) of a 4 x 4 step built as angle_axis_T builds it (row-major numpy 4 x 4)"""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])   # sin(theta) axis
    s = np.linalg.norm(v)
    cth = 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, cth)
    om = v * (th / s) if s > 1e-300 else v
    return np.concatenate([om, T[:3, 3]])


def make_T(rot, trans):
    """exp of the rotation vector `rot`, translation `trans`: a float64 4 x 4"""
    rot = np.asarray(rot, np.float64)
    th = np.linalg.norm(rot)
    Kx = skew(rot / th) if th > 0 else np.zeros((3, 3))
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = trans
    return T


# ------------------------------------------------------------------------------------------------------------------ scenes
# a 4 x 20 x 3 m box: x in [-2, 2], y in [-10, 10], z in [0, 3]; faces as (origin, edge u, edge v, inward normal)
_BOX = {
    "floor":   ((-2, -10, 0), (4, 0, 0), (0, 20, 0), (0, 0, 1)),
    "ceiling": ((-2, -10, 3), (4, 0, 0), (0, 20, 0), (0, 0, -1)),
    "wall_x-": ((-2, -10, 0), (0, 20, 0), (0, 0, 3), (1, 0, 0)),
    "wall_x+": ((2, -10, 0), (0, 20, 0), (0, 0, 3), (-1, 0, 0)),
    "end_y-":  ((-2, -10, 0), (4, 0, 0), (0, 0, 3), (0, 1, 0)),
    "end_y+":  ((-2, 10, 0), (4, 0, 0), (0, 0, 3), (0, -1, 0)),
}
_FACES = {
    "room": tuple(_BOX),
    "corridor": ("floor", "ceiling", "wall_x-", "wall_x+"),
    "floor_ceiling": ("floor", "ceiling"),
    "floor": ("floor",),
}
TUNNEL_RADIUS = 2.0
TUNNEL_AXIS_POINT = np.array([0.0, 0.0, 0.0])   # the cylinder's axis: this point + s * (0, 1, 0)


def _sample_faces(rng, faces, count):
    area = np.array([np.linalg.norm(np.cross(_BOX[f][1], _BOX[f][2])) for f in faces])
    which = rng.choice(len(faces), size=count, p=area / area.sum())
    uv = rng.random((count, 2))
    pts, nrm = np.empty((count, 3)), np.empty((count, 3))
    for i, f in enumerate(faces):
        o, eu, ev, nn = (np.asarray(a, np.float64) for a in _BOX[f])
        m = which == i
        pts[m] = o + uv[m, :1] * eu + uv[m, 1:] * ev
        nrm[m] = nn
    return pts, nrm


def _sample_tunnel(rng, count, bias):
    """points on the radius-2 cylinder along y; bias > 0 thins the side away from the sensor (which sits off the axis, towards +x)"""
    th = np.empty(0)
    while th.size < count:
        t = rng.uniform(-np.pi, np.pi, 2 * count)
        th = np.concatenate([th, t[rng.random(t.size) * (1 + bias) < 1 + bias * np.cos(t)]])
    th = th[:count]
    y = rng.uniform(-10, 10, count)
    nrm = np.stack([-np.cos(th), np.zeros(count), -np.sin(th)], 1)          # inward
    pts = TUNNEL_AXIS_POINT + np.stack([TUNNEL_RADIUS * np.cos(th), y, TUNNEL_RADIUS * np.sin(th)], 1)
    return pts, nrm


_cache = {}


def scene(name, m=8000, n=2000):
    """map (m, 4) float32 with exact normals (m, 3), reading (n, 4) float32 at the true pose with ITS exact normals (n, 3): independent
    samples of the same analytic surfaces.  Generated once per name; callers must not write into the arrays."""
    key = (name, m, n)
    if key not in _cache:
        rng = np.random.default_rng(1000 + SCENES.index(name))
        if name == "tunnel":
            mp, mn = _sample_tunnel(rng, m, 0.0)
            rd, rn = _sample_tunnel(rng, n, 0.6)
        else:
            mp, mn = _sample_faces(rng, _FACES[name], m)
            rd, rn = _sample_faces(rng, _FACES[name], n)
        f4 = lambda a: np.concatenate([a, np.ones((a.shape[0], 1))], 1).astype(np.float32)
        out = dict(map=f4(mp), normals=mn.astype(np.float32), reading=f4(rd), reading_normals=rn.astype(np.float32))
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def exact_system(name, origin=(0.0, 0.0, 0.0)):
    """the scene's system with EXACT pairs at the true pose (every reading point paired with its own foot point on the surface, its exact
    normal, weight 1), all coordinates moved by -origin: A, b, W, c, L"""
    sc = scene(name)
    p = sc["reading"][:, :3].astype(np.float64) - np.asarray(origin, np.float64)
    nn = sc["reading_normals"].astype(np.float64)
    A, b, W = pair_sums(p, p, nn)
    c0, L = reading_stats(p)
    return A, b, W, c0, L
