"""One table of inputs that drive the single-lane solve (csrc/solve.h; oracle/icp_oracle.c) into each of its branches: the polar
iteration and the route through the SVD (reflecting, rank 2, rank 1, zero H), Cholesky and the minimum-norm solution at N = 6, 4, 3,
both sides of the 0.5 rad switch of the step's sin / cos, the planar closed form with r == 0.  Pure numpy: no GPU, no oracle.

Every case is built so that the nearest map point of reading point i is map point i (`spacing`, the smallest distance between two
map points, is at least four times the largest displacement; the octahedra state their own rule), and is used with max_dist = inf
and no outlier filter.  The axis-aligned scenes sit on a dyadic lattice that is symmetric about its centre: the map's mean is exact,
the centred coordinates are the lattice itself, and what is zero by construction stays exactly 0.0 through float32.

A case is a dict: name, map4 (M, 4) float32, normals (M, 3) float32 or None, reading4 (N, 4) float32, kw (ICPSequence keywords), route
('newton' | 'svd' | 'reflect' | 'planar' | 'chol' | 'minnorm' | 'zero' | 'either'), unique (the optimum is one pose), null (indices of x = (rx, ry, rz, tx,
ty, tz) that are unobservable AND axis aligned: exactly 0.0 expected; their rows of A and b are exactly 0.0), spacing, pairs."""
import numpy as np

F = np.float32
EPS_F = float(np.finfo(np.float32).eps)

# ---- bounds -----------------------------------------------------------------------------------------------------------------
# well-conditioned single steps: the suite's existing bounds (tests/test_gpu_golden.py)
DT_FLOOR, DR_FLOOR = 2e-5, 2e-6
# ill-conditioned ones: K eps_f kappa (metres for the translation, radians for the rotation), kappa the case's own condition figure (solver_reference).  K is 4 x the worst
# error / (eps_f kappa) of the ORACLE against the float64 reference over this whole table, measured on the CPU by
# tests/test_solver_branches_cpu.py::test_table_report (it prints every case's figure; the device was never used to set it).
# Measured worst ratio: 0.352 (p2p_threshold_sweep_01: a well-conditioned case, kappa 2.06, rotation error 8.7e-8 rad; the ill-conditioned
# cases -- corridor with end wall, kappa 228; floor at 100 k pairs, kappa 533 -- stay below 0.001), rounded up; factor 4.
K_MEASURED = 0.36
K_FACTOR = 4.0
K = K_FACTOR * K_MEASURED
# device against oracle on the same inputs (tests/test_gpu_ext_filters.py::test_force_4dof_single_step_matches_oracle)
DEV_ORACLE_DT, DEV_ORACLE_DR = 1e-5, 1e-5
# largest |A_jj| of test_gpu_golden.py::test_point_to_plane_step_matches_numpy, whose atol = 2e-3 the sums' check scales by
GOLDEN_AJJ = 2.956e4       # max diag of sum F F^T over that test's 643 pairs, float64
SUM_RTOL_A, SUM_RTOL_B, SUM_ATOL = 2e-5, 2e-4, 2e-3


def h4(xyz):
    out = np.ones((xyz.shape[0], 4), dtype=F)
    out[:, :3] = xyz
    return out


def rotvec_R(v):
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K_ = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K_ + (1 - np.cos(th)) * K_ @ K_


def move(xyz, rotvec, t, about=None):
    """rigid motion of float64 points: rotation about `about` (default: their centroid), then translation"""
    c = xyz.mean(0) if about is None else np.asarray(about, np.float64)
    return (xyz - c) @ rotvec_R(rotvec).T + c + np.asarray(t, np.float64)


def lattice(*axes):
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack([a.ravel() for a in g], axis=1).astype(np.float64)


def sym(n, step):
    """n lattice coordinates symmetric about 0 (dyadic for dyadic steps)"""
    return (np.arange(n) - (n - 1) / 2.0) * step


TILT = rotvec_R((0.3, -0.2, 0.1))
OFFSET = np.array([3.0, -2.0, 1.5])


def _case(name, mp, nrm, rd, kw, route, unique=True, null=(), spacing=0.0, exact_mean=False, pairing="identity"):
    base = dict(max_dist=np.inf, outliers=[])
    base.update(kw)
    return dict(name=name, map4=h4(mp), normals=None if nrm is None else np.ascontiguousarray(nrm, dtype=F), reading4=h4(rd), kw=base,
                route=route, unique=unique, null=tuple(null), spacing=float(spacing), pairs=int(rd.shape[0]), exact_mean=exact_mean,
                pairing=pairing)


# ------------------------------------------------------------------------------------------------------------- point to point
P2P = dict(minimizer=1)
SMALL_MOTION = ((0.004, -0.006, 0.008), (0.02, -0.01, 0.01))


def p2p_generic():
    rng = np.random.default_rng(101)
    mp = lattice(sym(8, 1.0), sym(8, 1.0), sym(8, 1.0)) + rng.uniform(-0.1, 0.1, size=(512, 3)) + OFFSET
    return _case("p2p_generic", mp, None, move(mp, *SMALL_MOTION), P2P, "newton", spacing=0.8)


def _plane_grid(nx, ny, step):
    return lattice(sym(nx, step), sym(ny, step), np.zeros(1))


def p2p_coplanar():
    flat = _plane_grid(20, 16, 0.5)
    rd = move(flat, (0, 0, 0.01), (0.02, -0.015, 0.0))                    # in-plane motion
    return _case("p2p_coplanar", flat @ TILT.T + OFFSET, None, rd @ TILT.T + OFFSET, P2P, "svd", spacing=0.5)


def _slab(nx, ny, step, t):
    g = lattice(sym(nx, step), sym(ny, step), np.zeros(1))
    ij = np.rint(g[:, :2] / step - 0.5).astype(np.int64)
    g[:, 2] = np.where((ij[:, 0] + ij[:, 1]) % 2 == 0, 0.5 * t, -0.5 * t)   # checkerboard +- t / 2
    return g


def p2p_reflection():
    """a slab of thickness t = 0.2 on a 1 m grid; the reading is its mirror image through the mid plane, moved in that plane:
    H ~ diag(Sxx, Syy, -Szz), d ~ -(t / L)^2 / 2.8"""
    slab = _slab(8, 6, 1.0, 0.2)
    mir = slab * np.array([1.0, 1.0, -1.0])
    rd = move(mir, (0, 0, 0.006), (0.02, -0.01, 0.0), about=(0, 0, 0))
    return _case("p2p_reflection", slab @ TILT.T + OFFSET, None, rd @ TILT.T + OFFSET, P2P, "reflect", spacing=1.0)


def p2p_collinear():
    line = lattice(sym(30, 0.5), np.zeros(1), np.zeros(1))
    rd = move(line, (0, 0.005, -0.004), (0.03, 0.02, -0.01))
    return _case("p2p_collinear", line @ TILT.T + OFFSET, None, rd @ TILT.T + OFFSET, P2P, "svd", unique=False, spacing=0.5)


def p2p_coincident():
    mp = np.tile(np.array([[1.0, 2.0, 3.0]]), (16, 1))
    rd = np.tile(np.array([[1.25, 1.5, 3.125]]), (16, 1))
    return _case("p2p_coincident", mp, None, rd, P2P, "svd", unique=False, spacing=0.0, pairing="distance")


def p2p_two_points():
    mp = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, -0.5]])
    rd = move(mp, (0.01, -0.02, 0.015), (0.03, -0.02, 0.01))
    return _case("p2p_two_points", mp, None, rd, P2P, "svd", unique=False, spacing=2.29)


SWEEP_STEPS = 14
SWEEP_D = np.logspace(-9, -3, SWEEP_STEPS)


def _sweep_thickness(d):
    """slab on the 8 x 6 grid: Sxx = 48 * 5.25, Syy = 48 * 35 / 12, Szz = 48 t^2 / 4; d = Sxx Syy Szz / |H|^3"""
    sxx, syy = 48 * 5.25, 48 * 35.0 / 12.0
    n3 = (sxx * sxx + syy * syy) ** 1.5
    return float(np.sqrt(d * n3 / (sxx * syy) * 4.0 / 48.0))


def p2p_threshold_sweep():
    """one slab scene, one rigid motion; only the thickness changes: d runs over 1e-9 .. 1e-3 across the polar iteration's 1e-6"""
    out = []
    for k, d in enumerate(SWEEP_D):
        slab = _slab(8, 6, 1.0, _sweep_thickness(d))
        mp = slab @ TILT.T + OFFSET
        rd = move(mp, (0.003, -0.004, 0.005), (0.02, -0.01, 0.015))
        route = "svd" if d < 0.9e-7 else ("newton" if d > 1.1e-5 else "either")
        c = _case(f"p2p_threshold_sweep_{k:02d}", mp, None, rd, P2P, route, spacing=1.0)
        c["sweep"] = k
        out.append(c)
    return out


def p2p_planar_zero():
    mp = np.tile(np.array([[1.0, 2.0, 0.0]]), (16, 1))
    rd = np.tile(np.array([[1.25, 1.5, 0.0]]), (16, 1))
    return _case("p2p_planar_zero", mp, None, rd, dict(minimizer=1, is_2d=1), "planar", unique=False, spacing=0.0, pairing="distance")


def p2p_planar_generic():
    rng = np.random.default_rng(102)
    mp = lattice(sym(24, 1.0), sym(20, 1.0), np.zeros(1))
    mp[:, :2] += rng.uniform(-0.1, 0.1, size=(mp.shape[0], 2)) + OFFSET[:2]
    rd = move(mp, (0, 0, 0.007), (0.03, -0.02, 0.0))
    rd[:, 2] = 0.0
    return _case("p2p_planar_generic", mp, None, rd, dict(minimizer=1, is_2d=1), "planar", spacing=0.8)


# ------------------------------------------------------------------------------------------------------------- point to plane
P2L = dict(minimizer=2)
EZ = np.array([0.0, 0.0, 1.0])


def p2l_generic():
    rng = np.random.default_rng(201)
    mp = lattice(sym(6, 1.0), sym(6, 1.0), sym(6, 1.0)) + rng.uniform(-0.1, 0.1, size=(216, 3)) + OFFSET
    nrm = rng.normal(size=(216, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return _case("p2l_generic", mp, nrm, move(mp, *SMALL_MOTION), P2L, "chol", spacing=0.8)


def _floor(n, step=0.25, z=1.5):
    g = lattice(sym(n, step), sym(n, step), np.zeros(1))
    g[:, 2] = z
    return g, np.tile(EZ, (g.shape[0], 1))


def _floor_reading(mp, scale=1.0):
    """tilt about x and y and a lift: the three things a floor shows"""
    return move(mp, (0.004 * scale, -0.003 * scale, 0.0), (0.0, 0.0, 0.02), about=(0.0, 0.0, mp[0, 2]))


def p2l_floor(kw=P2L, name="p2l_floor", null=(2, 3, 4)):
    mp, nrm = _floor(32)
    return _case(name, mp, nrm, _floor_reading(mp), kw, "minnorm", null=null, spacing=0.25, exact_mean=True)


def p2l_floor_100k():
    mp, nrm = _floor(320)
    return _case("p2l_floor_100k", mp, nrm, _floor_reading(mp, 0.05), P2L, "minnorm", null=(2, 3, 4), spacing=0.25, exact_mean=True)


def p2l_two_parallel_planes():
    lo, n_lo = _floor(24, z=-1.0)
    hi, n_hi = _floor(24, z=1.0)
    mp = np.concatenate([lo, hi]); nrm = np.concatenate([n_lo, -n_hi])
    rd = move(mp, (0.004, -0.003, 0.0), (0.0, 0.0, 0.02), about=(0, 0, 0))
    return _case("p2l_two_parallel_planes", mp, nrm, rd, P2L, "minnorm", null=(2, 3, 4), spacing=0.25, exact_mean=True)


def _corridor():
    """walls x = -+1 (normals +-x), floor / ceiling z = -+1 (normals +-z), 8 m along y, no end wall"""
    y, s = sym(32, 0.25), sym(6, 0.25)
    parts, nrms = [], []
    for sx in (-1.0, 1.0):
        w = lattice(np.array([sx]), y, s); parts.append(w); nrms.append(np.tile([-sx, 0.0, 0.0], (w.shape[0], 1)))
    for sz in (-1.0, 1.0):
        f = lattice(s, y, np.array([sz])); parts.append(f); nrms.append(np.tile([0.0, 0.0, -sz], (f.shape[0], 1)))
    return np.concatenate(parts), np.concatenate(nrms)


CORRIDOR_MOTION = ((0.003, -0.002, 0.004), (0.01, 0.0, -0.015))


def p2l_corridor(kw=P2L, name="p2l_corridor", null=(4,)):
    mp, nrm = _corridor()
    return _case(name, mp, nrm, move(mp, *CORRIDOR_MOTION, about=(0, 0, 0)), kw, "minnorm", null=null, spacing=0.25, exact_mean=True)


def p2l_corridor_with_end_wall():
    mp, nrm = _corridor()
    s = sym(3, 0.5)
    end = lattice(s, np.array([4.25]), s)
    mp = np.concatenate([mp, end]); nrm = np.concatenate([nrm, np.tile([0.0, -1.0, 0.0], (end.shape[0], 1))])
    rd = move(mp, *CORRIDOR_MOTION, about=(0, 0, 0)) + np.array([0.0, 0.012, 0.0])
    return _case("p2l_corridor_with_end_wall", mp, nrm, rd, P2L, "chol", spacing=0.25)


def p2l_floor_4dof():
    return p2l_floor(dict(minimizer=2, force_4dof=1), "p2l_floor_4dof", null=(0, 1, 2, 3, 4))


def p2l_corridor_4dof():
    return p2l_corridor(dict(minimizer=2, force_4dof=1), "p2l_corridor_4dof", null=(0, 1, 4))


def p2l_wall_2d():
    """force2D over ONE wall x = -1: F = [x ny - y nx; nx; ny] = [-y; 1; 0]: rank 2 of 3"""
    w = lattice(np.array([-1.0]), sym(32, 0.25), sym(6, 0.25))
    nrm = np.tile([1.0, 0.0, 0.0], (w.shape[0], 1))
    rd = move(w, (0.0, 0.0, 0.004), (0.01, 0.0, 0.0), about=(-1.0, 0, 0))
    return _case("p2l_wall_2d", w, nrm, rd, dict(minimizer=2, force_2d=1), "minnorm", null=(0, 1, 4, 5), spacing=0.25, exact_mean=True)


def p2l_corridor_2d():
    return p2l_corridor(dict(minimizer=2, force_2d=1), "p2l_corridor_2d", null=(0, 1, 4, 5))


def p2l_floor_2d():
    """force2D over a floor: F = [x ny - y nx; nx; ny] == 0 for every pair: A == 0 exactly, nothing is kept, x == 0"""
    c = p2l_floor(dict(minimizer=2, force_2d=1), "p2l_floor_2d", null=(0, 1, 2, 3, 4, 5))
    c["route"] = "zero"
    return c


YAW = rotvec_R((0.0, 0.0, 0.37))


def _yawed_corridor(turn=None):
    """the corridor without the y < 0 half of its +x wall (the centroid leaves the axis: yaw couples with the translations), turned
    about z by a generic angle and moved away: the free direction is no coordinate axis and the rounded normals are not exact"""
    mp, nrm = _corridor()
    keep = ~((mp[:, 0] == 1.0) & (mp[:, 1] < 0))
    mp, nrm = mp[keep], nrm[keep]
    rd = move(mp, (0.0, 0.0, 0.004), (0.01, 0.0, -0.015), about=(0, 0, 0))
    Rt = YAW if turn is None else turn
    return mp @ Rt.T + OFFSET, nrm @ Rt.T, rd @ Rt.T + OFFSET


def p2l_yawed_corridor_4dof():
    """... tilted as well, so that tz couples with yaw, tx, ty: the {rz, tx, ty, tz} block is full, rank 3 (free along the corridor)"""
    mp, nrm, rd = _yawed_corridor(TILT @ YAW)
    return _case("p2l_yawed_corridor_4dof", mp, nrm, rd, dict(minimizer=2, force_4dof=1), "either", unique=False, spacing=0.25)


def p2l_yawed_corridor_2d():
    mp, nrm, rd = _yawed_corridor()
    return _case("p2l_yawed_corridor_2d", mp, nrm, rd, dict(minimizer=2, force_2d=1), "either", unique=False, spacing=0.25)


def p2l_tilted_floor():
    mp, nrm = _floor(32, z=0.0)
    rd = _floor_reading(mp)
    return _case("p2l_tilted_floor", mp @ TILT.T + OFFSET, nrm @ TILT.T, rd @ TILT.T + OFFSET, P2L, "either", unique=False, spacing=0.25)


# six points on a regular octahedron, generic unit normals (seed found by a search over the float64 reference alone: kappa(A) < 1e4 and
# the step's angle on the wanted side of 0.5 rad), reading = map turned about (1, 1, 1) through the centroid: every point moves by
# 2 r sin(angle / 2) sqrt(2 / 3) < 0.707 r / 2 ... (half the neighbour distance), so pairing holds
OCTA_R = 2.0
BIG_STEP = dict(seed=8, angle=0.6)        # |x[0:3]| = 0.553, kappa 31
BELOW_STEP = dict(seed=8, angle=0.5)      # |x[0:3]| = 0.493, kappa 50


def _octa(name, seed, angle):
    mp = OCTA_R * np.concatenate([np.eye(3), -np.eye(3)]) + OFFSET
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(6, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rd = move(mp, angle * np.ones(3) / np.sqrt(3.0), (0, 0, 0))
    return _case(name, mp, nrm, rd, P2L, "chol", spacing=OCTA_R * np.sqrt(2.0), pairing="octahedron")


def p2l_big_step():
    return _octa("p2l_big_step", **BIG_STEP)


def p2l_below_big_step():
    return _octa("p2l_below_big_step", **BELOW_STEP)


def all_cases():
    cases = [p2p_generic(), p2p_coplanar(), p2p_reflection(), p2p_collinear(), p2p_coincident(), p2p_two_points()]
    cases += p2p_threshold_sweep()
    cases += [p2p_planar_zero(), p2p_planar_generic()]
    cases += [p2l_generic(), p2l_floor(), p2l_two_parallel_planes(), p2l_corridor(), p2l_corridor_with_end_wall(), p2l_floor_4dof(),
              p2l_corridor_4dof(), p2l_wall_2d(), p2l_corridor_2d(), p2l_floor_2d(), p2l_yawed_corridor_4dof(), p2l_yawed_corridor_2d(),
              p2l_tilted_floor(), p2l_big_step(), p2l_below_big_step(),
              p2l_floor_100k()]
    return cases


_cache = {}


def cases_by_name():
    if not _cache:
        for c in all_cases():
            _cache[c["name"]] = c
    return _cache


NAMES = list(cases_by_name())
SWEEP_NAMES = [n for n in NAMES if n.startswith("p2p_threshold_sweep_")]
