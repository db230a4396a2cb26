"""PlaneToPlaneErrorMinimizer (ICPMI_MIN_PLANE_TO_PLANE) on the device, through the C ABI.

The pair sums of icpmi_minimize_step_normals against the float64 reference (tests/plane_to_plane_reference.py) evaluated on the pairs and
weights that icpmi_knn + icpmi_outlier_weights return for the same pose; the edges of the kernel; registrations; and that nothing of the
point-to-plane path moved.  Tolerances: four times what the float32 restatement of the specification loses against float64 on the same
scenes (profiles/plane_to_plane_tolerance.json, measured on the CPU by scripts/plane_to_plane_tolerance.py) -- never the device's own output.
"""
import ctypes as C

import numpy as np
import pytest

import localizability_cases as lcs
import localizability_reference as lr
import plane_to_plane_cases as pc
import plane_to_plane_reference as pr

pytestmark = pytest.mark.gpu
F = np.float32
MARGIN = 4.0


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def tol():
    return pc.recorded()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def make_icp(amd, k=1, chain="maxdist", eps=None, **kw):
    return amd.ICPSequence(knn=k, max_dist=pc.MAX_DIST, minimizer=pc.MIN_PLANE_TO_PLANE, outliers=pc.CHAINS[chain]["outliers"] if isinstance(chain, str) else chain,
                           plane_epsilon=eps, **kw)


def reference_on_device_pairs(icp, rc, rn, T, map4, map_normals, eps, k):
    """float64 sums on the pairs icpmi_knn finds for the queries T rc and the weights icpmi_outlier_weights gives them"""
    mc = lcs.centred(map4, icp.getMapMean())
    p = pr.xf_points(T, rc)
    ids, d2 = icp.knn(np.concatenate([p, np.ones((p.shape[0], 1), F)], 1), k=k, max_dist=pc.MAX_DIST)
    w, _ = icp.outlierWeights(d2, ids)
    ids, w = ids.ravel(), w.ravel().astype(np.float64)
    w[ids < 0] = 0.0
    safe = np.where(ids < 0, 0, ids)
    rep = lambda a: np.repeat(a, k, axis=0)
    return pr.reference_sums(rep(p), mc[safe, :3], map_normals[safe], rep(pr.rot_normals(T, rn)), eps, w)


def step_sums(amd, name, start, k, chain, eps=pr.EPS_DEFAULT, n=None, map_normals=None, read_normals=None, reading=None, **kw):
    """(T_step, device sums, reference sums) of one icpmi_minimize_step_normals on a scene"""
    sc = lr.scene(name)
    rd = sc["reading"] if reading is None else reading
    rn = sc["reading_normals"] if read_normals is None else read_normals
    if n is not None:
        rd, rn = rd[:n], rn[:n]
    mn = sc["normals"] if map_normals is None else map_normals
    T = pc.STARTS[start].astype(F)
    icp = make_icp(amd, k, chain, eps, **kw)
    try:
        assert icp.getPlaneEpsilon() == F(eps)
        assert icp.setMap(sc["map"], mn)
        rc = lcs.centred(rd, icp.getMapMean())
        T_step, sums = icp.minimizeStep(rc, T, read_normals=rn)
        ref = reference_on_device_pairs(icp, rc, rn, T, sc["map"], mn, eps, k)
    finally:
        icp.close()
    return T_step, sums, ref


def check_sums(sums, ref, bound, what):
    d = pr.rel_distance(sums, ref)
    print(f"{what}: rel distance {d:.3e} (allowed {bound:.3e}), pairs {int(sums[28])}, sum w {sums[27]:.6f}")
    assert sums[28] == ref[28], what
    assert sums[27] == pytest.approx(ref[27], rel=1e-12), what
    assert d <= bound, what
    assert (sums[29:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 1. sums and step
@pytest.mark.parametrize("name, start, k, chain", pc.SUM_CASES, ids=["-".join(map(str, c)) for c in pc.SUM_CASES])
def test_sums_against_float64(amd, tol, name, start, k, chain):
    _, sums, ref = step_sums(amd, name, start, k, chain)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"][name], f"{name} {start} k{k} {chain}")


@pytest.mark.parametrize("start", ["true", "off"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("four", [0, 1])
def test_step_against_float64_solve_of_the_device_sums(amd, tol, start, k, four):
    """room, cond(A) about 2.5e2: T_step against numpy's solve of the sums the same call returned"""
    T_step, sums, _ = step_sums(amd, "room", start, k, "trimmed", force_4dof=four)
    x_dev, x_ref = lr.step_from_T(T_step), pr.solve_step(sums, bool(four))
    rel = np.linalg.norm(x_dev - x_ref) / np.linalg.norm(x_ref)
    A = lr.unpack_sums(sums)[0]
    print(f"room {start} k{k} 4dof{four}: |x_dev - x_ref| / |x_ref| = {rel:.3e} (allowed {MARGIN * tol['max_rel_step_room']:.3e}), cond(A) {np.linalg.cond(A):.3g}")
    assert rel <= MARGIN * tol["max_rel_step_room"]
    if four:
        assert x_dev[0] == 0 and x_dev[1] == 0


# ------------------------------------------------------------------------------------------------------------------ 2. edges of the kernel
ACC_WORKGROUPS = 256      # the pair sums' grid (loop.hip: acc_cap)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 * 256 * ACC_WORKGROUPS + 1])
def test_pair_counts_k1(amd, tol, n):
    """around the two prefetched pairs of a lane, and one pair past a full grid (the tail loop)"""
    big = lr.scene("room", m=8000, n=n) if n > 2000 else lr.scene("room")
    _, sums, ref = step_sums(amd, "room", "off", 1, "maxdist", n=n, reading=big["reading"], read_normals=big["reading_normals"])
    assert sums[28] > 0.9 * n
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"n = {n}")


@pytest.mark.parametrize("n", [341, 342])
def test_pair_counts_k3(amd, tol, n):
    """3 n pairs around one 1024-thread workgroup"""
    _, sums, ref = step_sums(amd, "room", "off", 3, "maxdist", n=n)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"k = 3, n = {n}")


@pytest.mark.parametrize("which", ["reading", "map", "both-eps1", "scaled"])
@pytest.mark.parametrize("k", [1, 3])
def test_normals(amd, tol, which, k):
    sc = lr.scene("room")
    zr, zm = np.zeros_like(sc["reading_normals"]), np.zeros_like(sc["normals"])
    bound = MARGIN * tol["max_rel_sums"]["room"]
    if which == "reading":
        _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", read_normals=zr)
    elif which == "map":
        _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", map_normals=zm)
    elif which == "scaled":      # the reference sees unit normals, the device three times as long ones
        _, sums, _ = step_sums(amd, "room", "off", k, "maxdist", read_normals=3 * sc["reading_normals"], map_normals=3 * sc["normals"])
        _, _, ref = step_sums(amd, "room", "off", k, "maxdist")
    else:
        _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", eps=1.0, read_normals=zr, map_normals=zm)
        # M = I / 2 exactly: the translation block is 0.5 sum w I to the rounding of the double sum, its off-diagonal is exactly zero
        assert sums[15] == pytest.approx(0.5 * sums[27], rel=1e-13) and sums[18] == pytest.approx(0.5 * sums[27], rel=1e-13)
        assert sums[20] == pytest.approx(0.5 * sums[27], rel=1e-13)
        assert sums[16] == 0 and sums[17] == 0 and sums[19] == 0
    check_sums(sums, ref, bound, f"{which} k{k}")


def test_every_pair_rejected(amd):
    sc = lr.scene("room")
    icp = make_icp(amd, 1, [(pc.OUT_MAXDIST, 1e-9)])
    icp.setMap(sc["map"], sc["normals"])
    rc = lcs.centred(sc["reading"], icp.getMapMean())
    with pytest.raises(amd.icp.ConvergenceError, match="no point to minimize|convergence error"):
        icp.minimizeStep(rc, pc.STARTS["off"].astype(F), read_normals=sc["reading_normals"])
    assert icp._lib.icpmi_minimize_step_normals(icp._h, rc.ctypes.data, rc.shape[0], sc["reading_normals"].ctypes.data, None, None, None, None) == 3
    with pytest.raises(amd.icp.ConvergenceError):
        icp(sc["reading"], sc["reading_normals"])
    icp.close()


def test_missing_normals(amd):
    from norlab_icp_mapper_amd import _capi
    sc = lr.scene("room")
    icp = make_icp(amd)
    icp.setMap(sc["map"])                                        # a map without normals
    rc = lcs.centred(sc["reading"], icp.getMapMean())
    with pytest.raises(amd.icp.InvalidField):
        icp(sc["reading"], sc["reading_normals"])
    with pytest.raises(amd.icp.InvalidField):
        icp.minimizeStep(rc, None, read_normals=sc["reading_normals"])
    icp.setMap(sc["map"], sc["normals"])                         # ... and a reading without
    with pytest.raises(amd.icp.InvalidField):
        icp(sc["reading"])
    T, sums = (C.c_float * 16)(), (C.c_double * 32)()
    assert icp._lib.icpmi_minimize_step_normals(icp._h, rc.ctypes.data, rc.shape[0], None, None, T, sums, None) == _capi.ERR_MISSING_NORMALS
    with pytest.raises(amd.icp.InvalidField):                    # icpmi_register_prior carries no normals
        icp.registerWithPrior(sc["reading"], np.eye(4))
    assert np.isfinite(icp(sc["reading"], sc["reading_normals"])).all()
    icp.close()


def test_entry_points_that_cannot_carry_normals(amd):
    from norlab_icp_mapper_amd import _capi
    sc = lr.scene("room")
    icp = make_icp(amd)
    icp.setMap(sc["map"], sc["normals"])
    rc = lcs.centred(sc["reading"], icp.getMapMean())
    with pytest.raises(NotImplementedError, match="PlaneToPlaneErrorMinimizer"):
        icp.minimizeStep(rc)
    T, stats, status = (C.c_float * 16)(), _capi.Stats(), (C.c_int * 1)()
    ptrs, ns = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    assert icp._lib.icpmi_register_batch_dev(icp._h, 1, ptrs, ns, 0, T, C.byref(stats), status) == _capi.ERR_UNSUPPORTED
    assert "PlaneToPlaneErrorMinimizer" in icp._lib.icpmi_last_error(icp._h).decode()
    prior = np.eye(4, dtype=F)
    assert icp._lib.icpmi_register_multistart(icp._h, sc["reading"].ctypes.data, sc["reading"].shape[0], prior.ctypes.data, 1, 0, T, C.byref(stats),
                                              status) == _capi.ERR_UNSUPPORTED
    icp.close()


@pytest.mark.parametrize("extra", [dict(force_2d=1), dict(is_2d=1), dict(covariance=1), dict(degeneracy_threshold=0.01)])
def test_rejected_combinations(amd, extra):
    with pytest.raises(amd.icp.InvalidParameter, match="PlaneToPlaneErrorMinimizer"):
        make_icp(amd, **extra)
    icp = make_icp(amd)
    with pytest.raises(amd.icp.InvalidParameter, match="PlaneToPlaneErrorMinimizer"):
        icp.setConfig(minimizer=pc.MIN_PLANE_TO_PLANE, **extra)
    icp.close()


def test_plane_epsilon_setter(amd):
    icp = make_icp(amd)
    assert icp.getPlaneEpsilon() == F(1e-3)
    for bad in (0.0, -1.0, 1.0001, float("nan"), float("inf")):
        with pytest.raises(amd.icp.InvalidParameter):
            icp.setPlaneEpsilon(bad)
        assert icp.getPlaneEpsilon() == F(1e-3)
    icp.setPlaneEpsilon(0.25)
    icp.setConfig(minimizer=pc.MIN_PLANE_TO_PLANE, knn=3, max_dist=1.0)     # handle state: a new chain leaves it
    assert icp.getPlaneEpsilon() == 0.25
    icp.setPlaneEpsilon(1.0)
    assert icp.getPlaneEpsilon() == 1.0
    icp.close()


@pytest.mark.parametrize("chain", ["maxdist", "trimmed"])
def test_tile_sorted_reading_picks_its_own_normal(amd, tol, chain):
    """the k = 1 loop registers the reading in tile order (qindex): every reading point carries a normal of its own, so a normal gathered by
    the sorted position instead of the caller's index cannot pass"""
    sc = lr.scene("room")
    rng = np.random.default_rng(5)
    rn = rng.normal(size=sc["reading_normals"].shape)
    rn = (rn / np.linalg.norm(rn, axis=1, keepdims=True)).astype(F)
    icp = make_icp(amd, 1, chain, max_iterations=1)
    icp.setMap(sc["map"], sc["normals"])
    icp.keepSums(1)
    icp(sc["reading"], rn)
    assert icp.stats.iterations == 1
    ids, d2, T_used = icp.lastMatches()
    sums, limits = icp.lastSums()[:2]
    mean = icp.getMapMean()
    icp.close()
    assert np.array_equal(T_used, np.eye(4, dtype=F))
    mc, rc = lcs.centred(sc["map"], mean), lcs.centred(sc["reading"], mean)
    ids = ids.ravel()
    w = ((ids >= 0) & (d2.ravel() <= (limits[0] if chain == "trimmed" else F(pc.MAX_DIST * pc.MAX_DIST)))).astype(np.float64)
    assert 0.8 * ids.size < w.sum() < (0.9 if chain == "trimmed" else 1.01) * ids.size
    safe = np.where(ids < 0, 0, ids)
    ref = pr.reference_sums(rc[:, :3], mc[safe, :3], sc["normals"][safe], rn, pr.EPS_DEFAULT, w)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], "tile-sorted")
    wrong = pr.reference_sums(rc[:, :3], mc[safe, :3], sc["normals"][safe], np.roll(rn, 1, axis=0), pr.EPS_DEFAULT, w)
    assert pr.rel_distance(wrong, ref) > 1e3 * MARGIN * tol["max_rel_sums"]["room"]      # (the test can tell)


# ------------------------------------------------------------------------------------------------------------------ 3. registration
def moved_reading(sc, T):
    """the reading and its normals moved by T (float64 4 x 4): registering it must answer T^-1"""
    rd = sc["reading"].copy()
    rd[:, :3] = (sc["reading"][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    rn = (sc["reading_normals"].astype(np.float64) @ T[:3, :3].T).astype(F)
    return rd, rn


def pose_error(T, T_true):
    D = np.asarray(T, np.float64) @ np.linalg.inv(T_true)
    return float(np.linalg.norm(D[:3, 3])), float(np.linalg.norm(lr.step_from_T(D)[:3]))


REG = dict(max_iterations=40, use_differential=1)


def test_register_converges_on_room(amd):
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])
    icp = make_icp(amd, 1, "trimmed", **REG)
    icp.setMap(sc["map"], sc["normals"])
    T = icp(rd, rn)
    dt, dr = pose_error(T, np.linalg.inv(pc.STARTS["off"]))
    print(f"room from the off start: {icp.stats.iterations} iterations, |dt| {dt:.2e} m, |dr| {dr:.2e} rad")
    assert icp.stats.stop_reason == 2 and dt <= 1e-3 and dr <= 1e-3
    T2 = icp(rd, rn)
    assert np.array_equal(_bits(T), _bits(T2))                    # two calls, the same bits
    res = icp.residual(rd, T, normals=rn)                         # ErrorMinimizer::getResidualError: the point-to-plane residual
    assert res.kind == 2 and res.pairs > 0
    icp.close()
    ref = amd.ICPSequence(knn=1, max_dist=pc.MAX_DIST, minimizer=2, outliers=pc.CHAINS["trimmed"]["outliers"], **REG)
    ref.setMap(sc["map"], sc["normals"])
    assert ref.residual(rd, T, kind=2).bits() == res.bits()
    ref.close()


@pytest.mark.parametrize("k", [1, 3])
def test_force_4dof_keeps_roll_and_pitch_zero(amd, k):
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])
    icp = make_icp(amd, k, "trimmed", force_4dof=1, **REG)
    icp.setMap(sc["map"], sc["normals"])
    T = icp(rd, rn)
    icp.close()
    assert T[2, 0] == 0 and T[2, 1] == 0 and T[0, 2] == 0 and T[1, 2] == 0 and T[2, 2] == 1
    assert abs(T[0, 1]) > 0      # (it did turn about z)


@pytest.mark.parametrize("k", [1, 3])
def test_graph_replay_is_the_eager_run(amd, k):
    import torch
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()
    out = {}
    for graph in (1, 0):
        icp = make_icp(amd, k, "trimmed", use_graph=graph, **REG)
        icp.setMap(sc["map"], sc["normals"])
        out[graph] = [icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=6, d_normals_ptr=dn.data_ptr()) for _ in range(3)]   # capture, replay, replay
        assert icp.stats.iterations == 6
        icp.close()
    for T in out[1] + out[0]:
        assert np.array_equal(_bits(T), _bits(out[0][0]))


def test_epsilon_change_reaches_a_cached_graph(amd):
    import torch
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()
    run = lambda icp: icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=2, d_normals_ptr=dn.data_ptr())
    icp = make_icp(amd, 1, "trimmed")
    icp.setMap(sc["map"], sc["normals"])
    a0, a1 = run(icp), run(icp)                                   # the second call replays the graph
    icp.setPlaneEpsilon(1.0)
    b0, b1 = run(icp), run(icp)
    icp.setPlaneEpsilon(1e-3)
    a2 = run(icp)
    icp.close()
    fresh = make_icp(amd, 1, "trimmed", eps=1.0)
    fresh.setMap(sc["map"], sc["normals"])
    bf = run(fresh)
    fresh.close()
    assert np.array_equal(_bits(a0), _bits(a1)) and np.array_equal(_bits(a0), _bits(a2))
    assert np.array_equal(_bits(b0), _bits(b1)) and np.array_equal(_bits(b0), _bits(bf))
    assert not np.array_equal(_bits(a0), _bits(b0))


YAML_CHAIN = """matcher:
  KDTreeMatcher:
    knn: 3
    maxDist: 2.0
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.85
errorMinimizer:
  PlaneToPlaneErrorMinimizer:
    epsilon: 0.01
    force4DOF: 0
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 40
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.001
      smoothLength: 3
"""


def test_yaml_chains_reach_the_same_pose(amd):
    import host_chain_bindings as hcb
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])
    direct = make_icp(amd, 3, "trimmed", eps=0.01, **REG)
    direct.setMap(sc["map"], sc["normals"])
    T = direct(rd, rn)
    its = direct.stats.iterations
    direct.close()
    dt, dr = pose_error(T, np.linalg.inv(pc.STARTS["off"]))
    assert dt <= 1e-3 and dr <= 1e-3
    chain = {"matcher": {"KDTreeMatcher": {"knn": 3, "maxDist": 2.0}}, "outlierFilters": [{"TrimmedDistOutlierFilter": {"ratio": 0.85}}],
             "errorMinimizer": {"PlaneToPlaneErrorMinimizer": {"epsilon": 0.01, "force4DOF": 0}},
             "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}},
                                        {"DifferentialTransformationChecker": {"minDiffRotErr": 0.001, "minDiffTransErr": 0.001, "smoothLength": 3}}]}
    py = amd.ICPSequence.loadFromYaml(chain)
    assert py.getPlaneEpsilon() == F(0.01)
    py.setMap(sc["map"], sc["normals"])
    T_py = py(rd, rn)
    py.close()
    T_cpp, stats = hcb.icp_register(YAML_CHAIN, sc["map"], sc["normals"], rd, rn)
    print("python yaml max |dT|", np.abs(T_py - T).max(), "c++ yaml max |dT|", np.abs(T_cpp - T).max(), "iterations", its, stats.iterations)
    assert np.array_equal(_bits(T_py), _bits(T))
    assert np.array_equal(_bits(T_cpp), _bits(T)) and stats.iterations == its
    with pytest.raises(RuntimeError, match="normals"):            # a reading without `normals`: InvalidField
        hcb.icp_register(YAML_CHAIN, sc["map"], sc["normals"], rd, None)


# ------------------------------------------------------------------------------------------------------------------ 4. nothing else moved
def test_point_to_plane_is_untouched_by_a_plane_to_plane_handle(amd):
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])

    def point_to_plane():
        icp = amd.ICPSequence(knn=1, max_dist=pc.MAX_DIST, minimizer=2, outliers=pc.CHAINS["trimmed"]["outliers"], **REG)
        icp.setMap(sc["map"], sc["normals"])
        rc = lcs.centred(rd, icp.getMapMean())
        T_step, sums = icp.minimizeStep(rc, pc.STARTS["true"].astype(F))
        T = icp(rd)
        icp.close()
        return T_step, sums, T

    before = point_to_plane()
    gicp = make_icp(amd, 1, "trimmed", **REG)
    gicp.setMap(sc["map"], sc["normals"])
    gicp.minimizeStep(lcs.centred(rd, gicp.getMapMean()), None, read_normals=rn)
    T_gicp = gicp(rd, rn)
    gicp.close()
    after = point_to_plane()
    assert np.array_equal(_bits(before[0]), _bits(after[0]))
    assert np.array_equal(before[1].view(np.uint64), after[1].view(np.uint64))
    assert np.array_equal(_bits(before[2]), _bits(after[2]))
    assert not np.array_equal(_bits(T_gicp), _bits(after[2]))     # (the two minimisers do differ)


# ------------------------------------------------------------------------------------------------------------------ 5. the rest of the chain
OUT_SURFACENORMAL = 5


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("behind", ["trimmed", "cauchy"])
def test_surface_normal_filter_in_the_chain(amd, tol, k, behind):
    """SurfaceNormalOutlierFilter reads the reading's normal the pair sums already hold (plain and EXT instantiations): pairs across the
    room's edges (normals at right angles) drop out exactly as icpmi_outlier_weights drops them"""
    sc = lr.scene("room")
    chain = [(OUT_SURFACENORMAL, 0.9)] + pc.CHAINS[behind]["outliers"]
    T = pc.STARTS["off"].astype(F)
    icp = make_icp(amd, k, chain)
    icp.setMap(sc["map"], sc["normals"])
    rc = lcs.centred(sc["reading"], icp.getMapMean())
    rn = sc["reading_normals"]
    _, sums = icp.minimizeStep(rc, T, read_normals=rn)
    mc = lcs.centred(sc["map"], icp.getMapMean())
    p = pr.xf_points(T, rc)
    rn_rot = pr.rot_normals(T, rn)
    ids, d2 = icp.knn(np.concatenate([p, np.ones((p.shape[0], 1), F)], 1), k=k, max_dist=pc.MAX_DIST)
    w, _ = icp.outlierWeights(d2, ids, read_normals=rn_rot)
    icp.close()
    ids, w = ids.ravel(), w.ravel().astype(np.float64)
    w[ids < 0] = 0.0
    safe = np.where(ids < 0, 0, ids)
    rep = lambda a: np.repeat(a, k, axis=0)
    ref = pr.reference_sums(rep(p), mc[safe, :3], sc["normals"][safe], rep(rn_rot), pr.EPS_DEFAULT, w)
    assert 0 < (w == 0).sum() < 0.5 * w.size      # (the filter did reject something)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"surface normal + {behind}, k{k}")


def test_var_dist_matcher_is_served(amd):
    """KDTreeVarDistMatcher with a constant row of radii is KDTreeMatcher{maxDist} bit for bit, under this minimiser too"""
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])
    fixed = make_icp(amd, 1, "trimmed", **REG)
    fixed.setMap(sc["map"], sc["normals"])
    T = fixed(rd, rn)
    fixed.close()
    var = amd.ICPSequence(knn=1, var_dist=1, minimizer=pc.MIN_PLANE_TO_PLANE, outliers=pc.CHAINS["trimmed"]["outliers"], **REG)
    var.setMap(sc["map"], sc["normals"])
    var.setReadingMaxDist(np.full(rd.shape[0], pc.MAX_DIST, F))
    T_var = var(rd, rn)
    var.close()
    assert np.array_equal(_bits(T), _bits(T_var))


def test_sensor_noise_overlap_follows_point_to_plane(amd):
    sc = lr.scene("room")
    rd, rn = moved_reading(sc, pc.STARTS["off"])
    icp = make_icp(amd, 1, "trimmed", **REG)
    icp.setMap(sc["map"], sc["normals"])
    icp(rd, rn)
    assert icp.stats.sensor_noise_overlap == -1.0                 # no noise row: not computed
    icp.setReadingSensorNoise(np.full(rd.shape[0], 0.01, F))
    T = icp(rd, rn)
    got = float(icp.stats.sensor_noise_overlap)
    icp.close()
    # the point-to-plane count on the last iteration's pairs: |(p - q) . n_p / |n_p|| < noise.  The planes are exact and the pose is
    # within 1e-5 m of the truth, so every pair within a face passes; only pairs across an edge can fail
    assert 0.9 < got <= 1.0, got
    dt, dr = pose_error(T, np.linalg.inv(pc.STARTS["off"]))
    assert dt <= 1e-3 and dr <= 1e-3
