"""SymmetricPointToPlaneErrorMinimizer (ICPMI_MIN_PLANE_TO_PLANE under ICPMI_PLANE_MODEL_SYMMETRIC) on the device, through the C ABI.

The pair sums of icpmi_minimize_step_normals against the float64 reference (tests/symmetric_reference.py) evaluated on the pairs and weights
that icpmi_knn + icpmi_outlier_weights return for the same pose; the edges of the kernel; the properties of the pair model (sign invariance
bit for bit, agreement with point-to-plane); registrations on a curved scene and in the room; graphs; refusals; YAML.  Tolerances: four
times what the float32 restatement of the specification loses against float64 on the same scenes (profiles/symmetric_tolerance.json,
measured on the CPU by scripts/symmetric_tolerance.py) -- never the device's own output.
"""
import ctypes as C

import numpy as np
import pytest

import localizability_cases as lcs
import localizability_reference as lr
import plane_to_plane_reference as pp
import symmetric_cases as sc
import symmetric_reference as sr

pytestmark = pytest.mark.gpu
F = np.float32
MARGIN = 4.0
OFF = sc.STARTS["off"]
TRUTH = np.linalg.inv(OFF)


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def tol():
    return sc.recorded()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_icp(amd, k=1, chain="maxdist", model="symmetric", **kw):
    return amd.ICPSequence(knn=k, max_dist=sc.MAX_DIST, minimizer=sc.MIN_PLANE_TO_PLANE, outliers=sc.CHAINS[chain]["outliers"] if isinstance(chain, str) else chain,
                           plane_model=model, **kw)


def make_point_to_plane(amd, k=1, chain="maxdist", **kw):
    return amd.ICPSequence(knn=k, max_dist=sc.MAX_DIST, minimizer=sc.MIN_POINT_TO_PLANE, outliers=sc.CHAINS[chain]["outliers"], **kw)


def reference_on_device_pairs(icp, rc, rn, T, map4, map_normals, k):
    """float64 sums on the pairs icpmi_knn finds for the queries T rc and the weights icpmi_outlier_weights gives them"""
    mc = lcs.centred(map4, icp.getMapMean())
    p = pp.xf_points(T, rc)
    ids, d2 = icp.knn(np.concatenate([p, np.ones((p.shape[0], 1), F)], 1), k=k, max_dist=sc.MAX_DIST)
    w, _ = icp.outlierWeights(d2, ids)
    ids, w = ids.ravel(), w.ravel().astype(np.float64)
    w[ids < 0] = 0.0
    safe = np.where(ids < 0, 0, ids)
    rep = lambda a: np.repeat(a, k, axis=0)
    return sr.reference_sums(rep(p), mc[safe, :3], map_normals[safe], rep(pp.rot_normals(T, rn)), w)


def step_sums(amd, name, start, k, chain, n=None, map_normals=None, read_normals=None, reading=None, ref_map_normals=None, ref_read_normals=None, **kw):
    """(T_step, device sums, reference sums) of one icpmi_minimize_step_normals on a scene; ref_*: the normals the reference sees when they
    are not the device's"""
    s = sr.scene(name)
    rd = s["reading"] if reading is None else reading
    rn = s["reading_normals"] if read_normals is None else read_normals
    rrn = rn if ref_read_normals is None else ref_read_normals
    if n is not None:
        rd, rn, rrn = rd[:n], rn[:n], rrn[:n]
    mn = s["normals"] if map_normals is None else map_normals
    T = sc.STARTS[start].astype(F) if isinstance(start, str) else np.asarray(start, F)
    icp = make_icp(amd, k, chain, **kw)
    try:
        assert icp.getPlaneModel() == "symmetric"
        assert icp.setMap(s["map"], mn)
        rc = lcs.centred(rd, icp.getMapMean())
        T_step, sums = icp.minimizeStep(rc, T, read_normals=rn)
        ref = reference_on_device_pairs(icp, rc, rrn, T, s["map"], mn if ref_map_normals is None else ref_map_normals, k)
    finally:
        icp.close()
    return T_step, sums, ref


def check_sums(sums, ref, bound, what):
    d = pp.rel_distance(sums, ref)
    print(f"{what}: rel distance {d:.3e} (allowed {bound:.3e}), pairs {int(sums[28])}, sum w {sums[27]:.6f}")
    assert sums[28] == ref[28], what
    assert sums[27] == pytest.approx(ref[27], rel=1e-12), what
    assert d <= bound, what
    assert (sums[29:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 1. sums and step
@pytest.mark.parametrize("name, start, k, chain", sc.SUM_CASES, ids=["-".join(map(str, c)) for c in sc.SUM_CASES])
def test_sums_against_float64(amd, tol, name, start, k, chain):
    _, sums, ref = step_sums(amd, name, start, k, chain)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"][name], f"{name} {start} k{k} {chain}")


@pytest.mark.parametrize("start", ["true", "off"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("chain", list(sc.CHAINS))
@pytest.mark.parametrize("four", [0, 1])
def test_step_against_float64_solve_of_the_device_sums(amd, tol, start, k, chain, four):
    """room: T_step against numpy's solve of the sums the same call returned"""
    T_step, sums, _ = step_sums(amd, "room", start, k, chain, force_4dof=four)
    x_dev, x_ref = lr.step_from_T(T_step), pp.solve_step(sums, bool(four))
    rel = sr.rel_step(x_dev, x_ref)
    A = lr.unpack_sums(sums)[0]
    print(f"room {start} k{k} {chain} 4dof{four}: rel_step = {rel:.3e} (allowed {MARGIN * tol['max_rel_step_room']:.3e}), |x_ref| {np.linalg.norm(x_ref):.3e}, cond(A) {np.linalg.cond(A):.3g}")
    assert rel <= MARGIN * tol["max_rel_step_room"]
    if four:
        assert x_dev[0] == 0 and x_dev[1] == 0


# ------------------------------------------------------------------------------------------------------------------ 2. edges of the kernel
ACC_WORKGROUPS = 256      # the pair sums' grid (loop.hip: acc_cap)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 * 256 * ACC_WORKGROUPS + 1])
def test_pair_counts_k1(amd, tol, n):
    """around the two prefetched pairs of a lane, and one pair past a full grid (the tail loop that requests a pair's four gathers together)"""
    big = sr.scene("room", m=8000, n=n) if n > 2000 else sr.scene("room")
    _, sums, ref = step_sums(amd, "room", "off", 1, "maxdist", n=n, reading=big["reading"], read_normals=big["reading_normals"])
    assert sums[28] > 0.9 * n
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"n = {n}")


@pytest.mark.parametrize("n", [341, 342])
def test_pair_counts_k3(amd, tol, n):
    """3 n pairs around one 1024-thread workgroup"""
    _, sums, ref = step_sums(amd, "room", "off", 3, "maxdist", n=n)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"k = 3, n = {n}")


# ------------------------------------------------------------------------------------------------------------------ 3. normals
@pytest.mark.parametrize("which", ["reading-zero", "reading-nan", "map-zero", "scaled"])
@pytest.mark.parametrize("k", [1, 3])
def test_normals(amd, tol, which, k):
    s = sr.scene("room")
    rn, mn = s["reading_normals"], s["normals"]
    bound = MARGIN * tol["max_rel_sums"]["room"]
    if which == "reading-zero":         # no surface model on the reading side: n_s = u_q, every pair
        _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", read_normals=np.zeros_like(rn))
    elif which == "reading-nan":        # ... on every third point, by a NaN in one component, in all, or by a zero; the reference sees zeros there
        bad, zeroed = rn.copy(), rn.copy()
        bad[0::9, 1], bad[3::9, :], bad[6::9, :] = np.nan, np.nan, 0.0
        zeroed[0::3] = 0.0
        _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", read_normals=bad, ref_read_normals=zeroed)
    elif which == "map-zero":           # n_s = u_p
        _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", map_normals=np.zeros_like(mn))
    else:                               # the reference sees unit normals, the device three times as long ones
        _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", read_normals=3 * rn, map_normals=3 * mn, ref_read_normals=rn, ref_map_normals=mn)
    check_sums(sums, ref, bound, f"{which} k{k}")


@pytest.mark.parametrize("k", [1, 3])
def test_no_normal_on_either_side_only_counts(amd, k):
    s = sr.scene("room")
    _, sums, ref = step_sums(amd, "room", "off", k, "maxdist", read_normals=np.zeros_like(s["reading_normals"]), map_normals=np.zeros_like(s["normals"]))
    assert (sums[:27] == 0).all() and (ref[:27] == 0).all()
    assert sums[28] == ref[28] > 0.9 * k * 2000 and sums[27] == pytest.approx(ref[27], rel=1e-12)


@pytest.mark.parametrize("name", ["room", "ellipsoid"])
@pytest.mark.parametrize("k, chain", [(1, "trimmed"), (3, "cauchy")])
def test_sign_of_either_normal_cancels_bit_for_bit(amd, name, k, chain):
    """negating a random half of the reading's normals, and separately of the map's: all 32 sums keep their bits"""
    s = sr.scene(name)
    rng = np.random.default_rng(3)
    flip = lambda nrm: np.where(rng.random(nrm.shape[0])[:, None] < 0.5, -nrm, nrm).astype(F)
    base = step_sums(amd, name, "off", k, chain)[1]
    flipped_r, flipped_m = flip(s["reading_normals"]), flip(s["normals"])
    assert 0.4 < (flipped_r != s["reading_normals"]).any(1).mean() < 0.6 and 0.4 < (flipped_m != s["normals"]).any(1).mean() < 0.6
    got_r = step_sums(amd, name, "off", k, chain, read_normals=flipped_r)[1]
    got_m = step_sums(amd, name, "off", k, chain, map_normals=flipped_m)[1]
    assert np.array_equal(_bits64(got_r), _bits64(base))
    assert np.array_equal(_bits64(got_m), _bits64(base))
    assert base[28] > 0 and np.abs(base[:27]).max() > 0


# ------------------------------------------------------------------------------------------------------------------ 4. agreement
@pytest.mark.parametrize("k", [1, 3])
def test_vertical_normals_under_yaw_are_point_to_plane_bit_for_bit(amd, k):
    """floor and ceiling: every normal is (0, 0, +-1), and a yaw-only pose keeps the reading's there: u_q = +-u_p, n_s = u_q exactly, and the
    sums are those of a PointToPlaneErrorMinimizer handle with the same chain"""
    s = lr.scene("floor_ceiling")
    rng = np.random.default_rng(4)
    rn = (s["reading_normals"] * np.where(rng.random(s["reading_normals"].shape[0]) < 0.5, -1, 1)[:, None]).astype(F)
    assert set(np.unique(np.abs(s["normals"][:, 2]))) == {1.0} and set(np.unique(rn[:, 2])) == {-1.0, 1.0}
    T = lr.make_T((0.0, 0.0, 0.05), (0.2, -0.2, 0.1)).astype(F)
    sym = make_icp(amd, k, "trimmed")
    sym.setMap(s["map"], s["normals"])
    rc = lcs.centred(s["reading"], sym.getMapMean())
    Ts, sums = sym.minimizeStep(rc, T, read_normals=rn)
    sym.close()
    p2p = make_point_to_plane(amd, k, "trimmed")
    p2p.setMap(s["map"], s["normals"])
    Tp, sums_p = p2p.minimizeStep(rc, T)
    p2p.close()
    assert sums[28] > 0.8 * k * rc.shape[0] and np.abs(sums[:27]).max() > 0
    assert np.array_equal(_bits64(sums), _bits64(sums_p))
    assert np.array_equal(_bits(Ts), _bits(Tp))


# ------------------------------------------------------------------------------------------------------------------ 5. the reading's own normal
@pytest.mark.parametrize("chain", ["maxdist", "trimmed"])
def test_tile_sorted_reading_picks_its_own_normal(amd, tol, chain):
    """the k = 1 loop registers the reading in tile order (qindex): every reading point carries a normal of its own, so a normal gathered by
    the sorted position instead of the caller's index cannot pass"""
    s = sr.scene("room")
    rng = np.random.default_rng(5)
    rn = rng.normal(size=s["reading_normals"].shape)
    rn = (rn / np.linalg.norm(rn, axis=1, keepdims=True)).astype(F)
    icp = make_icp(amd, 1, chain, max_iterations=1)
    icp.setMap(s["map"], s["normals"])
    icp.keepSums(1)
    icp(s["reading"], rn)
    assert icp.stats.iterations == 1
    ids, d2, T_used = icp.lastMatches()
    sums, limits = icp.lastSums()[:2]
    mean = icp.getMapMean()
    icp.close()
    assert np.array_equal(T_used, np.eye(4, dtype=F))
    mc, rc = lcs.centred(s["map"], mean), lcs.centred(s["reading"], mean)
    ids = ids.ravel()
    w = ((ids >= 0) & (d2.ravel() <= (limits[0] if chain == "trimmed" else F(sc.MAX_DIST * sc.MAX_DIST)))).astype(np.float64)
    assert 0.8 * ids.size < w.sum() < (0.9 if chain == "trimmed" else 1.01) * ids.size
    safe = np.where(ids < 0, 0, ids)
    ref = sr.reference_sums(rc[:, :3], mc[safe, :3], s["normals"][safe], rn, w)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], "tile-sorted")
    wrong = sr.reference_sums(rc[:, :3], mc[safe, :3], s["normals"][safe], np.roll(rn, 1, axis=0), w)
    assert pp.rel_distance(wrong, ref) > 1e3 * MARGIN * tol["max_rel_sums"]["room"]      # (the test can tell)


# ------------------------------------------------------------------------------------------------------------------ 6, 7. registration
REG = dict(max_iterations=40, use_differential=1)


def test_register_on_the_ellipsoid_beats_point_to_plane_tenfold(amd, tol):
    """a closed curved surface sampled at different places by reading and map, from the off start, 8 fixed iterations: point-to-plane settles
    off by the sampling error, the symmetric residual vanishes on constant curvature (tests/test_symmetric_cpu.py has the same on numpy)"""
    s = sr.scene("ellipsoid")
    rd, rn = sr.moved_reading(s, OFF)
    icp = make_icp(amd, 1, "trimmed", max_iterations=sc.ELLIPSOID_ITERATIONS)
    icp.setMap(s["map"], s["normals"])
    T = icp(rd, rn)
    assert icp.stats.iterations == sc.ELLIPSOID_ITERATIONS
    T2 = icp(rd, rn)
    icp.close()
    p2p = make_point_to_plane(amd, 1, "trimmed", max_iterations=sc.ELLIPSOID_ITERATIONS)
    p2p.setMap(s["map"], s["normals"])
    Tp = p2p(rd)
    p2p.close()
    (dt, dr), (pt, prot) = sr.pose_error(T, TRUTH), sr.pose_error(Tp, TRUTH)
    rec = tol["loops"]["ellipsoid"]
    print(f"ellipsoid: symmetric {dt:.3e} m / {dr:.3e} rad, point-to-plane {pt:.3e} m / {prot:.3e} rad, float32 loop {rec['float32_translation_error']:.3e} m / "
          f"{rec['float32_rotation_error']:.3e} rad")
    assert dt <= 0.1 * pt
    assert dt <= MARGIN * rec["float32_translation_error"]
    assert np.array_equal(_bits(T), _bits(T2))                    # two calls, the same bits


def test_register_converges_on_room(amd, tol):
    s = sr.scene("room")
    rd, rn = sr.moved_reading(s, OFF)
    icp = make_icp(amd, 1, "trimmed", **REG)
    icp.setMap(s["map"], s["normals"])
    T = icp(rd, rn)
    its, reason = icp.stats.iterations, icp.stats.stop_reason
    res = icp.residual(rd, T, normals=rn)                         # ErrorMinimizer::getResidualError: the point-to-plane residual
    icp.close()
    p2p = make_point_to_plane(amd, 1, "trimmed", **REG)
    p2p.setMap(s["map"], s["normals"])
    Tp = p2p(rd)
    res_p = p2p.residual(rd, T, kind=2)
    p2p.close()
    (dt, dr), (pt, prot) = sr.pose_error(T, TRUTH), sr.pose_error(Tp, TRUTH)
    rec = tol["loops"]["room"]
    print(f"room: {its} iterations, symmetric {dt:.3e} m / {dr:.3e} rad, point-to-plane {pt:.3e} m / {prot:.3e} rad, float32 loop "
          f"{rec['float32_translation_error']:.3e} m / {rec['float32_rotation_error']:.3e} rad")
    assert reason == 2                                             # the Differential checker
    assert dt < pt and dr < prot
    assert dt <= MARGIN * rec["float32_translation_error"] and dr <= MARGIN * rec["float32_rotation_error"]
    assert res.kind == 2 and res.pairs > 0 and res.bits() == res_p.bits()


# ------------------------------------------------------------------------------------------------------------------ 8. graphs
@pytest.mark.parametrize("k", [1, 3])
def test_graph_replay_is_the_eager_run(amd, k):
    import torch
    s = sr.scene("room")
    rd, rn = sr.moved_reading(s, OFF)
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()
    out = {}
    for graph in (1, 0):
        icp = make_icp(amd, k, "trimmed", use_graph=graph, **REG)
        icp.setMap(s["map"], s["normals"])
        out[graph] = [icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=6, d_normals_ptr=dn.data_ptr()) for _ in range(3)]   # capture, replay, replay
        assert icp.stats.iterations == 6
        icp.close()
    for T in out[1] + out[0]:
        assert np.array_equal(_bits(T), _bits(out[0][0]))


def test_model_change_reaches_a_cached_graph(amd):
    import torch
    s = sr.scene("room")
    rd, rn = sr.moved_reading(s, OFF)
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()
    run = lambda icp: icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=2, d_normals_ptr=dn.data_ptr())
    icp = make_icp(amd, 1, "trimmed", model="gicp")
    icp.setMap(s["map"], s["normals"])
    a0, a1 = run(icp), run(icp)                                   # the second call replays the graph
    icp.setPlaneModel("symmetric")
    b0, b1 = run(icp), run(icp)
    icp.setPlaneModel("gicp")
    a2 = run(icp)
    icp.close()
    fresh = make_icp(amd, 1, "trimmed")
    fresh.setMap(s["map"], s["normals"])
    bf = run(fresh)
    fresh.close()
    assert np.array_equal(_bits(a0), _bits(a1)) and np.array_equal(_bits(a0), _bits(a2))
    assert np.array_equal(_bits(b0), _bits(b1)) and np.array_equal(_bits(b0), _bits(bf))
    assert not np.array_equal(_bits(a0), _bits(b0))


# ------------------------------------------------------------------------------------------------------------------ 9. refusals and state
NAME = "SymmetricPointToPlaneErrorMinimizer"


def test_missing_normals(amd):
    from norlab_icp_mapper_amd import _capi
    s = sr.scene("room")
    icp = make_icp(amd)
    icp.setMap(s["map"])                                         # a map without normals
    rc = lcs.centred(s["reading"], icp.getMapMean())
    with pytest.raises(amd.icp.InvalidField, match=NAME):
        icp(s["reading"], s["reading_normals"])
    with pytest.raises(amd.icp.InvalidField, match=NAME):
        icp.minimizeStep(rc, None, read_normals=s["reading_normals"])
    icp.setMap(s["map"], s["normals"])                           # ... and a reading without
    with pytest.raises(amd.icp.InvalidField, match=NAME):
        icp(s["reading"])
    T, sums = (C.c_float * 16)(), (C.c_double * 32)()
    assert icp._lib.icpmi_minimize_step_normals(icp._h, rc.ctypes.data, rc.shape[0], None, None, T, sums, None) == _capi.ERR_MISSING_NORMALS
    with pytest.raises(amd.icp.InvalidField):                    # icpmi_register_prior carries no normals
        icp.registerWithPrior(s["reading"], np.eye(4))
    assert np.isfinite(icp(s["reading"], s["reading_normals"])).all()
    icp.close()


def test_entry_points_that_cannot_carry_normals(amd):
    from norlab_icp_mapper_amd import _capi
    s = sr.scene("room")
    icp = make_icp(amd)
    icp.setMap(s["map"], s["normals"])
    rc = lcs.centred(s["reading"], icp.getMapMean())
    with pytest.raises(NotImplementedError, match=NAME):
        icp.minimizeStep(rc)
    T, stats, status = (C.c_float * 16)(), _capi.Stats(), (C.c_int * 1)()
    ptrs, ns = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    assert icp._lib.icpmi_register_batch_dev(icp._h, 1, ptrs, ns, 0, T, C.byref(stats), status) == _capi.ERR_UNSUPPORTED
    assert NAME in icp._lib.icpmi_last_error(icp._h).decode()
    prior = np.eye(4, dtype=F)
    assert icp._lib.icpmi_register_multistart(icp._h, s["reading"].ctypes.data, s["reading"].shape[0], prior.ctypes.data, 1, 0, T, C.byref(stats),
                                              status) == _capi.ERR_UNSUPPORTED
    assert NAME in icp._lib.icpmi_last_error(icp._h).decode()
    icp.setPlaneModel("gicp")                                    # the message names the minimiser the user configured
    with pytest.raises(NotImplementedError, match="^(?!.*Symmetric).*PlaneToPlaneErrorMinimizer"):
        icp.minimizeStep(rc)
    icp.close()


@pytest.mark.parametrize("extra", [dict(force_2d=1), dict(is_2d=1), dict(covariance=1), dict(degeneracy_threshold=0.01)])
def test_rejected_combinations(amd, extra):
    with pytest.raises(amd.icp.InvalidParameter, match="PlaneToPlaneErrorMinimizer"):
        make_icp(amd, **extra)
    icp = make_icp(amd)
    with pytest.raises(amd.icp.InvalidParameter, match="PlaneToPlaneErrorMinimizer"):
        icp.setConfig(minimizer=sc.MIN_PLANE_TO_PLANE, **extra)
    assert icp.getPlaneModel() == "symmetric"
    icp.close()


def test_plane_model_setter_and_state(amd, tol):
    from norlab_icp_mapper_amd import _capi
    icp = amd.ICPSequence(knn=1, max_dist=sc.MAX_DIST, minimizer=sc.MIN_PLANE_TO_PLANE, outliers=sc.CHAINS["maxdist"]["outliers"])
    assert icp.getPlaneModel() == "gicp"                         # the default: nothing changes for existing users
    icp.setPlaneModel("symmetric")
    for bad in (2, -1, 16, 0x7fffffff):
        assert icp._lib.icpmi_set_plane_pair_model(icp._h, bad) == _capi.ERR_INVALID_ARG
        assert icp.getPlaneModel() == "symmetric"
    assert icp._lib.icpmi_get_plane_pair_model(icp._h, None) == _capi.ERR_INVALID_ARG
    with pytest.raises(amd.icp.InvalidParameter):
        icp.setPlaneModel("plain-sum")
    icp.setConfig(minimizer=sc.MIN_PLANE_TO_PLANE, knn=3, max_dist=1.0)     # handle state: a new chain leaves it
    assert icp.getPlaneModel() == "symmetric"
    icp.setConfig(minimizer=sc.MIN_PLANE_TO_PLANE, knn=1, max_dist=sc.MAX_DIST, outliers=sc.CHAINS["maxdist"]["outliers"])
    # plane epsilon is ignored by this model, and kept
    s = sr.scene("room")
    icp.setMap(s["map"], s["normals"])
    rc = lcs.centred(s["reading"], icp.getMapMean())
    a = icp.minimizeStep(rc, OFF.astype(F), read_normals=s["reading_normals"])[1]
    icp.setPlaneEpsilon(0.5)
    b = icp.minimizeStep(rc, OFF.astype(F), read_normals=s["reading_normals"])[1]
    assert np.array_equal(_bits64(a), _bits64(b)) and icp.getPlaneEpsilon() == 0.5
    icp.setPlaneModel("gicp")
    g = icp.minimizeStep(rc, OFF.astype(F), read_normals=s["reading_normals"])[1]
    assert pp.rel_distance(g, a) > 1e3 * MARGIN * tol["max_rel_sums"]["room"]        # (the model does select the sums)
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 10. YAML
YAML_CHAIN = """matcher:
  KDTreeMatcher:
    knn: 3
    maxDist: 2.0
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.85
errorMinimizer:
  SymmetricPointToPlaneErrorMinimizer:
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
    s = sr.scene("room")
    rd, rn = sr.moved_reading(s, OFF)
    direct = make_icp(amd, 3, "trimmed", **REG)
    direct.setMap(s["map"], s["normals"])
    T = direct(rd, rn)
    its = direct.stats.iterations
    direct.close()
    dt, dr = sr.pose_error(T, TRUTH)
    assert dt <= 1e-3 and dr <= 1e-3
    gicp = make_icp(amd, 3, "trimmed", model="gicp", **REG)
    gicp.setMap(s["map"], s["normals"])
    T_gicp = gicp(rd, rn)
    gicp.close()
    assert not np.array_equal(_bits(T_gicp), _bits(T))           # (a chain that lost its model on the way would answer this)
    chain = {"matcher": {"KDTreeMatcher": {"knn": 3, "maxDist": 2.0}}, "outlierFilters": [{"TrimmedDistOutlierFilter": {"ratio": 0.85}}],
             "errorMinimizer": {"SymmetricPointToPlaneErrorMinimizer": {"force4DOF": 0}},
             "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}},
                                        {"DifferentialTransformationChecker": {"minDiffRotErr": 0.001, "minDiffTransErr": 0.001, "smoothLength": 3}}]}
    py = amd.ICPSequence.loadFromYaml(chain)
    assert py.getPlaneModel() == "symmetric"
    py.setMap(s["map"], s["normals"])
    T_py = py(rd, rn)
    py.close()
    T_cpp, stats = hcb.icp_register(YAML_CHAIN, s["map"], s["normals"], rd, rn)
    print("python yaml max |dT|", np.abs(T_py - T).max(), "c++ yaml max |dT|", np.abs(T_cpp - T).max(), "iterations", its, stats.iterations)
    assert np.array_equal(_bits(T_py), _bits(T))
    assert np.array_equal(_bits(T_cpp), _bits(T)) and stats.iterations == its
    with pytest.raises(RuntimeError, match="normals"):            # a reading without `normals`: InvalidField
        hcb.icp_register(YAML_CHAIN, s["map"], s["normals"], rd, None)
