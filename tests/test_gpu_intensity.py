"""IntensityPointToPlaneErrorMinimizer (ICPMI_MIN_POINT_TO_PLANE with icpmi_set_intensity_weight > 0) on the device, through the C ABI.

The gradient operator against the float64 reference on the neighbours the device's own search reports; the pair sums of icpmi_minimize_step
against the float64 reference (tests/intensity_reference.py) evaluated on the pairs and weights that icpmi_knn + icpmi_outlier_weights return
for the same pose; the properties of the term; registrations in the corridor and the room; graphs; state and refusals.  Tolerances: four times
what the float32 restatement of the specification loses against float64 on the same cases (profiles/intensity_tolerance.json, measured on the
CPU by scripts/intensity_tolerance.py) -- never the device's own output.
"""
import ctypes as C

import numpy as np
import pytest

import intensity_cases as ic
import intensity_reference as ir
import localizability_cases as lcs
import localizability_reference as lr
import plane_to_plane_reference as pp
import symmetric_reference as sr

pytestmark = pytest.mark.gpu
F = np.float32
MARGIN = 4.0
TRUTH = np.linalg.inv(ir.START)
REG = dict(max_iterations=40, use_differential=1, min_diff_rot=1e-3, min_diff_trans=1e-3, smooth_length=3)


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def tol():
    return ic.recorded()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_icp(amd, k=1, chain="maxdist", weight=ic.WEIGHT, **kw):
    return amd.ICPSequence(knn=k, max_dist=ic.MAX_DIST, minimizer=ic.MIN_POINT_TO_PLANE, outliers=ic.CHAINS[chain]["outliers"] if isinstance(chain, str) else chain,
                           intensity_weight=weight, **kw)


def loaded(amd, name="room", k=1, chain="maxdist", weight=ic.WEIGHT, **kw):
    """a handle with the scene's map and its intensity channel"""
    s = ir.scene(name)
    icp = make_icp(amd, k, chain, weight, **kw)
    assert icp.setMap(s["map"], s["normals"])
    icp.setMapIntensity(s["map_intensity"])
    return icp, s


# ------------------------------------------------------------------------------------------------------------------ 1. gradients
def device_gradients(amd, cloud, normals, inten, K, with_neighbours=True):
    """the operator's answer and (with_neighbours) the rows of the search it ran on: icpmi_debug_self_knn on the same private handle"""
    icp = amd.ICPSequence(knn=1, max_dist=ic.MAX_DIST, outliers=[])
    try:
        g = icp.intensityGradient(cloud, normals, inten, knn=K)
        g2 = icp.intensityGradient(cloud, normals, inten, knn=K)
        nbr = icp.debugSelfKnn(cloud, K + 1)[0].astype(np.int64) if with_neighbours else None
    finally:
        icp.close()
    assert np.array_equal(_bits(g), _bits(g2))                   # two calls, the same bits
    return g, nbr


def check_gradients(g, cloud, normals, inten, nbr, bound, what):
    ref = ir.gradient_reference(cloud, normals, inten, nbr)
    floor = ic.gradient_floor(cloud, inten, nbr)
    d = ir.gradient_distance(g, ref, floor)
    print(f"{what}: gradient distance {d:.3e} (allowed {bound:.3e}), floor {floor:.3e}, |g| up to {np.linalg.norm(ref, axis=1).max():.3f}")
    assert d <= bound, what
    assert ((g == 0).all(1) == (ref == 0).all(1)).all(), what     # the points without a gradient are the reference's
    return ref


@pytest.mark.parametrize("label, m, K", ic.PATCH_CASES, ids=[c[0] for c in ic.PATCH_CASES])
def test_gradient_on_a_plane_with_a_linear_field(amd, tol, label, m, K):
    """m = K + 1: every point sees all the others; m = K: unfilled slots; K = 1: one neighbour is a line (g = 0); K = 31; 257 and 4097 points:
    a second workgroup and seventeen.  Wherever a gradient exists it is the tangential part of the field's"""
    cloud, normals, inten = ic.patch(m)
    g, nbr = device_gradients(amd, cloud, normals, inten, K)
    assert (nbr[:, 0] == np.arange(m)).all() and ((nbr[:, 1:] >= 0).sum(1) == min(K, m - 1)).all()
    ref = check_gradients(g, cloud, normals, inten, nbr, MARGIN * tol["max_rel_gradient"]["patch " + label], label)
    has = (ref != 0).any(1)
    assert has.all() if K > 1 else not has.any()
    if K > 1:                                                     # (the reference itself against the analytic answer: the field is linear)
        assert np.abs(ref - ic.patch_gradient()[None, :]).max() <= 1e-4


def test_gradient_past_the_grid(amd, tol):
    """one point more than the gradient kernel's grid covers in one pass: the points of the second pass (and a sample of the first) against
    the reference on the device's neighbours"""
    cloud, normals, inten, pick = ic.wrap_case()
    g, nbr = device_gradients(amd, cloud, normals, inten, ic.KNN)
    assert (nbr[pick, 0] == pick).all()
    ref = ir.gradient_reference(cloud, normals, inten, nbr[pick], pick)
    d = ir.gradient_distance(g[pick], ref, ic.gradient_floor(cloud, inten, nbr[pick]))
    print(f"{ic.GRID_WRAP} points: distance {d:.3e} over {pick.size} points (allowed {MARGIN * tol['max_rel_gradient']['patch wrap']:.3e}), last point {g[-1]}")
    assert d <= MARGIN * tol["max_rel_gradient"]["patch wrap"]
    assert (g != 0).any(1).all() and np.abs(g[pick] - ic.patch_gradient()[None, :]).max() <= 1e-3


def test_gradient_single_point_duplicates_and_a_line(amd):
    """no neighbour, neighbours on the point itself, neighbours on a line: no gradient"""
    cloud, normals, inten = ic.patch(1)
    assert (device_gradients(amd, cloud, normals, inten, ic.KNN, False)[0] == 0).all()
    cloud, normals, inten = ic.patch(12)
    dup = np.repeat(cloud[:1], 12, 0)
    assert (device_gradients(amd, dup, normals, inten, ic.KNN, False)[0] == 0).all()
    line = cloud.copy()
    t = np.cross(ic.PATCH_NORMAL, [0.0, 0.0, 1.0])
    line[:, :3] = (cloud[0, :3].astype(np.float64) + np.linspace(-1, 1, 12)[:, None] * t[None, :]).astype(F)
    li = (line[:, :3].astype(np.float64) @ ic.PATCH_A + ic.PATCH_C).astype(F)
    assert (device_gradients(amd, line, normals, li, ic.KNN, False)[0] == 0).all()


def test_gradient_nan_intensities_and_a_zero_normal(amd, tol):
    """a NaN on a neighbour is skipped (the others still give the field's gradient), on the point itself there is no gradient; a zero or
    non-finite normal has no tangent plane"""
    cloud, normals, inten = ic.patch(257)
    inten, normals = inten.copy(), normals.copy()
    inten[[5, 100]] = np.nan
    normals[17] = 0.0
    normals[33, 1] = np.inf
    g, nbr = device_gradients(amd, cloud, normals, inten, ic.KNN)
    assert (g[[5, 100, 17, 33]] == 0).all()
    near = np.unique(np.where((nbr[:, 1:] == 5) | (nbr[:, 1:] == 100))[0])
    near = near[~np.isin(near, [5, 100, 17, 33])]
    assert near.size > 0 and np.abs(g[near] - ic.patch_gradient()[None, :]).max() <= 1e-4
    check_gradients(g, cloud, normals, inten, nbr, MARGIN * tol["max_rel_gradient"]["patch 257"], "NaN / zero normal")


# ------------------------------------------------------------------------------------------------------------------ 2. sums and step
def reference_on_device_pairs(icp, rc, Ip, T, mc, s, k, weight=ic.WEIGHT, K=ic.KNN, map_normals=None, map_intensity=None):
    """float64 sums on the pairs icpmi_knn finds for the queries T rc, the weights icpmi_outlier_weights gives them and the float64 gradients
    of the centred map on the neighbours the device's search reports"""
    mn = s["normals"] if map_normals is None else map_normals
    mi = s["map_intensity"] if map_intensity is None else map_intensity
    g = ir.gradient_reference(mc, mn, mi, icp.debugSelfKnn(mc, K + 1)[0].astype(np.int64))
    p = pp.xf_points(T, rc)
    ids, d2 = icp.knn(np.concatenate([p, np.ones((p.shape[0], 1), F)], 1), k=k, max_dist=ic.MAX_DIST)
    w, _ = icp.outlierWeights(d2, ids)
    ids, w = ids.ravel(), w.ravel().astype(np.float64)
    w[ids < 0] = 0.0
    safe = np.where(ids < 0, 0, ids)
    rep = lambda a: np.repeat(a, k, axis=0)
    return ir.reference_sums(rep(p), mc[safe, :3], mn[safe], g[safe], mi[safe], rep(Ip), w, weight)


def step_sums(amd, name, start, k, chain, n=None, weight=ic.WEIGHT, reading=None, reading_intensity=None, order=None, **kw):
    """(T_step, device sums, reference sums) of one icpmi_minimize_step on a scene; order: the map handed over in that permutation"""
    s = ir.scene(name)
    rd = s["reading"] if reading is None else reading
    Ip = s["reading_intensity"] if reading_intensity is None else reading_intensity
    if n is not None:
        rd, Ip = rd[:n], Ip[:n]
    mp, mn, mi = s["map"], s["normals"], s["map_intensity"]
    if order is not None:
        mp, mn, mi = mp[order], mn[order], mi[order]
    icp = make_icp(amd, k, chain, weight, **kw)
    try:
        assert icp.setMap(mp, mn)
        icp.setMapIntensity(mi)
        mean = icp.getMapMean()
        rc, mc = lcs.centred(rd, mean), lcs.centred(mp, mean)
        T = ir.centred_pose(ic.STARTS[start], mean).astype(F) if isinstance(start, str) else np.asarray(start, F)
        icp.setReadingIntensity(Ip)
        T_step, sums = icp.minimizeStep(rc, T)
        ref = reference_on_device_pairs(icp, rc, Ip, T, mc, s, k, weight, map_normals=mn, map_intensity=mi)
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


@pytest.mark.parametrize("name, start, k, chain", ic.SUM_CASES, ids=["-".join(map(str, c)) for c in ic.SUM_CASES])
def test_sums_against_float64(amd, tol, name, start, k, chain):
    _, sums, ref = step_sums(amd, name, start, k, chain)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"][name], f"{name} {start} k{k} {chain}")


@pytest.mark.parametrize("start", list(ic.STARTS))
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("chain", list(ic.CHAINS))
@pytest.mark.parametrize("four", [0, 1])
def test_step_against_float64_solve_of_the_device_sums(amd, tol, start, k, chain, four):
    """room: T_step against numpy's solve of the sums the same call returned"""
    T_step, sums, _ = step_sums(amd, "room", start, k, chain, force_4dof=four)
    x_dev, x_ref = lr.step_from_T(T_step), pp.solve_step(sums, bool(four))
    rel = sr.rel_step(x_dev, x_ref)
    print(f"room {start} k{k} {chain} 4dof{four}: rel_step = {rel:.3e} (allowed {MARGIN * tol['max_rel_step_room']:.3e}), |x_ref| {np.linalg.norm(x_ref):.3e}")
    assert rel <= MARGIN * tol["max_rel_step_room"]
    if four:
        assert x_dev[0] == 0 and x_dev[1] == 0


ACC_WORKGROUPS = 256      # the pair sums' grid (loop.hip: acc_cap)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2 * 256 * ACC_WORKGROUPS + 1])
def test_pair_counts_k1(amd, tol, n):
    """around a wave and a workgroup, and one pair past the two prefetched pairs of every lane of a full grid (the tail loop that requests
    everything a pair reads together).  Every reading point carries its own intensity: a wrong index shows in the sums"""
    big = ir.scene("room", m=8000, n=n) if n > 2000 else ir.scene("room")
    assert np.unique(big["reading_intensity"][:n]).size > 0.99 * n
    _, sums, ref = step_sums(amd, "room", "start", 1, "trimmed", n=n, reading=big["reading"], reading_intensity=big["reading_intensity"])
    assert sums[28] >= 0.8 * n - 1
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"n = {n}")


@pytest.mark.parametrize("n", [341, 342])
def test_pair_counts_k3(amd, tol, n):
    """3 n pairs around one 1024-thread workgroup"""
    _, sums, ref = step_sums(amd, "room", "start", 3, "maxdist", n=n)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"k = 3, n = {n}")


@pytest.mark.parametrize("k", [1, 3])
def test_a_shuffled_map_gives_the_same_agreement(amd, tol, k):
    """the intensity row is handed over in the caller's order and kept in the index's: a map in another order reaches the same reference"""
    order = np.random.default_rng(11).permutation(8000)
    _, sums, ref = step_sums(amd, "corridor", "start", k, "trimmed", order=order)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["corridor"], f"shuffled k{k}")
    _, plain, _ = step_sums(amd, "corridor", "start", k, "trimmed")
    assert pp.rel_distance(sums, plain) <= 2 * MARGIN * tol["max_rel_sums"]["corridor"]


# ------------------------------------------------------------------------------------------------------------------ 3. properties
def _fixed(amd, icp, s, iterations=5):
    import torch
    rd, _ = sr.moved_reading(s, ir.START)
    d = torch.from_numpy(rd).cuda()
    return icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=iterations)


@pytest.mark.parametrize("k, chain", [(1, "trimmed"), (3, "cauchy")])
def test_weight_zero_is_point_to_plane_bit_for_bit(amd, k, chain):
    """weight 0 after weight 0.032: the sums and a whole registration are those of a handle that never saw the setters"""
    s = ir.scene("room")
    plain = amd.ICPSequence(knn=k, max_dist=ic.MAX_DIST, minimizer=ic.MIN_POINT_TO_PLANE, outliers=ic.CHAINS[chain]["outliers"])
    plain.setMap(s["map"], s["normals"])
    rc = lcs.centred(s["reading"], plain.getMapMean())
    T = ir.centred_pose(ir.START, plain.getMapMean()).astype(F)
    base, base_T = plain.minimizeStep(rc, T)[1], _fixed(amd, plain, s)
    plain.close()
    icp, _ = loaded(amd, "room", k, chain)
    icp.setReadingIntensity(s["reading_intensity"])
    with_term = icp.minimizeStep(rc, T)[1]
    icp.setIntensityWeight(0.0)
    assert icp.getIntensityWeight() == 0.0
    off, off_T = icp.minimizeStep(rc, T)[1], _fixed(amd, icp, s)
    icp.close()
    assert np.array_equal(_bits64(off), _bits64(base)) and np.array_equal(_bits(off_T), _bits(base_T))
    assert not np.array_equal(_bits64(with_term), _bits64(base))


def test_small_weights_approach_point_to_plane(amd, tol):
    """lambda -> 1: the sums approach point-to-plane's, and reach them within the tolerance.  A weight w moves the sums by about
    w (1 + |F_I|^2 / |F_G|^2) relative: the distance shrinks with the weight, the reference follows it, and at 2^-40 -- where lambda rounds
    to 1.0f and the photometric part is 1e-12 of the geometric one -- the sums lie within the tolerance of the weight-0 sums"""
    _, base, _ = step_sums(amd, "room", "start", 1, "maxdist", weight=0.0)
    prev = np.inf
    for wgt in (ic.WEIGHT, 2.0 ** -10, 2.0 ** -20, 2.0 ** -40):
        _, sums, ref = step_sums(amd, "room", "start", 1, "maxdist", weight=wgt)
        check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"weight {wgt:g}")
        d = pp.rel_distance(sums, base)
        print(f"weight {wgt:g}: distance from point-to-plane {d:.3e}")
        assert d < prev
        prev = d
    assert prev <= MARGIN * tol["max_rel_sums"]["room"]


@pytest.mark.parametrize("k", [1, 3])
def test_a_nan_reading_intensity_adds_the_geometric_part_only(amd, tol, k):
    """every third reading point without an intensity, and every fifth map point: the reference sees the same NaNs; with none finite the
    sums are lambda times point-to-plane's"""
    s = ir.scene("room")
    Ip = s["reading_intensity"].copy()
    Ip[::3] = np.nan
    _, sums, ref = step_sums(amd, "room", "start", k, "maxdist", reading_intensity=Ip)
    check_sums(sums, ref, MARGIN * tol["max_rel_sums"]["room"], f"NaN I_p k{k}")
    _, none, _ = step_sums(amd, "room", "start", k, "maxdist", reading_intensity=np.full_like(Ip, np.nan))
    _, base, _ = step_sums(amd, "room", "start", k, "maxdist", weight=0.0)
    lam = float(F(1) - F(ic.WEIGHT))
    # (w lambda) F F against lambda (w F F): two roundings of a double per term, far below 1e-12 of the largest sum
    assert np.abs(none[:27] - lam * base[:27]).max() <= 1e-12 * np.abs(base[:27]).max() and np.array_equal(none[27:], base[27:])


# ------------------------------------------------------------------------------------------------------------------ 4. registrations
def test_register_in_the_corridor_recovers_the_axis(amd, tol):
    """from 0.3 m off along the axis, 8 fixed iterations: the term finds the pose point-to-plane cannot observe.  Both halves of the
    pose distance are held to four times the record; under the rotation's lies intensity_cases.ROTATION_FLOOR (eps_f times the 0.03 rad a
    float32 pose has to represent), which is above the 1.7e-9 rad the two CPU loops happen to differ by"""
    s = ir.scene("corridor")
    rd, _ = sr.moved_reading(s, ir.START)
    icp, _ = loaded(amd, "corridor", 1, "trimmed", max_iterations=ic.CORRIDOR_ITERATIONS)
    icp.setReadingIntensity(s["reading_intensity"])
    T = icp(rd)
    assert icp.stats.iterations == ic.CORRIDOR_ITERATIONS
    with pytest.raises(amd.icp.InvalidField, match="icpmi_set_reading_intensity"):   # the row was one shot
        icp(rd)
    T2 = icp(rd, descriptors={"intensity": s["reading_intensity"]})     # (the row by the descriptor's name, as a YAML chain's host hands it over)
    icp.setIntensityWeight(0.0)                                   # point-to-plane on the same handle
    icp.setConfig(knn=1, max_dist=ic.MAX_DIST, minimizer=ic.MIN_POINT_TO_PLANE, outliers=ic.CHAINS["trimmed"]["outliers"], max_iterations=ic.TWIN_ITERATIONS)
    Tp = icp(rd)
    icp.close()
    ref = ir.register("corridor", ic.WEIGHT, 64, ic.CORRIDOR_ITERATIONS)[-1]
    rec = tol["loops"]["corridor"]
    dt, dr = sr.pose_error(T, ref)
    along, along_p = abs(ir.residual_pose(T)[ir.AXIS, 3]), abs(ir.residual_pose(Tp)[ir.AXIS, 3])
    print(f"corridor: from the float64 loop {dt:.3e} m / {dr:.3e} rad (float32 loop {rec['float32_from_float64_translation']:.3e} m / "
          f"{rec['float32_from_float64_rotation']:.3e} rad), along the axis {along:.3e} m, point-to-plane {along_p:.4f} m")
    assert along < ic.ALONG_AXIS_BOUND
    assert along_p > ic.TWIN_STAYS_ABOVE
    assert dt <= MARGIN * rec["float32_from_float64_translation"]
    assert dr <= MARGIN * max(rec["float32_from_float64_rotation"], ic.ROTATION_FLOOR)
    assert sr.pose_error(T, TRUTH)[1] <= MARGIN * rec["float32_rotation_error"]
    assert np.array_equal(_bits(T), _bits(T2))                    # two calls, the same bits


def test_register_converges_in_the_room(amd, tol):
    s = ir.scene("room")
    rd, _ = sr.moved_reading(s, ir.START)
    icp, _ = loaded(amd, "room", 1, "trimmed", **REG)
    icp.setReadingIntensity(s["reading_intensity"])
    T = icp(rd)
    its, reason = icp.stats.iterations, icp.stats.stop_reason
    icp.close()
    dt, dr = sr.pose_error(T, TRUTH)
    rec = tol["loops"]["room"]
    print(f"room: {its} iterations, {dt:.3e} m / {dr:.3e} rad, float32 loop {rec['float32_translation_error']:.3e} m / {rec['float32_rotation_error']:.3e} rad")
    assert reason == 2                                             # the Differential checker
    assert dt <= MARGIN * rec["float32_translation_error"] and dr <= MARGIN * rec["float32_rotation_error"]


@pytest.mark.parametrize("k", [1, 3])
def test_graph_replay_is_the_eager_run(amd, k):
    import torch
    s = ir.scene("room")
    rd, _ = sr.moved_reading(s, ir.START)
    d = torch.from_numpy(rd).cuda()
    out = {}
    for graph in (1, 0):
        icp, _ = loaded(amd, "room", k, "trimmed", use_graph=graph, **REG)
        out[graph] = []
        for _ in range(3):                                        # capture, replay, replay
            icp.setReadingIntensity(s["reading_intensity"])
            out[graph].append(icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=6))
        assert icp.stats.iterations == 6
        icp.close()
    for T in out[1] + out[0]:
        assert np.array_equal(_bits(T), _bits(out[0][0]))


def test_weight_change_reaches_a_cached_graph(amd):
    import torch
    s = ir.scene("room")
    rd, _ = sr.moved_reading(s, ir.START)
    d = torch.from_numpy(rd).cuda()
    icp, _ = loaded(amd, "room", 1, "trimmed")

    def run():
        icp.setReadingIntensity(s["reading_intensity"])
        return icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=2)
    a0, a1 = run(), run()                                         # the second call replays the graph
    icp.setIntensityWeight(0.25)
    b0, b1 = run(), run()
    icp.setIntensityWeight(ic.WEIGHT)
    a2 = run()
    icp.close()
    assert np.array_equal(_bits(a0), _bits(a1)) and np.array_equal(_bits(a0), _bits(a2))
    assert np.array_equal(_bits(b0), _bits(b1)) and not np.array_equal(_bits(a0), _bits(b0))


def test_register_prior_serves_the_term(amd):
    """icpmi_register_prior with the one-shot row: the scan moved by the prior on the device answers what icpmi_register answers for the
    scan moved on the host by the same float32 prior, and the row is consumed"""
    s = ir.scene("corridor")
    icp, _ = loaded(amd, "corridor", 1, "trimmed", max_iterations=ic.CORRIDOR_ITERATIONS)
    icp.setReadingIntensity(s["reading_intensity"])
    T = icp.registerWithPrior(s["reading"], ir.START.astype(F))
    along = abs((T.astype(np.float64) @ ir.START)[ir.AXIS, 3])
    print(f"register_prior: along the axis {along:.3e} m")
    assert along < ic.ALONG_AXIS_BOUND
    with pytest.raises(amd.icp.InvalidParameter, match="InvalidField.*icpmi_set_reading_intensity"):
        icp.registerWithPrior(s["reading"], ir.START.astype(F))
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 5. state and refusals
TERM = "intensity term"


def test_setter_range_and_state(amd):
    from norlab_icp_mapper_amd import _capi
    icp = amd.ICPSequence(knn=1, max_dist=ic.MAX_DIST, outliers=[])
    assert icp.getIntensityWeight() == 0.0                       # the default: nothing changes for existing users
    icp.setIntensityWeight(0.25)
    for bad in (1.0, -0.001, 1.5, np.nan, np.inf, -np.inf):
        assert icp._lib.icpmi_set_intensity_weight(icp._h, C.c_float(bad)) == _capi.ERR_INVALID_ARG
        assert icp.getIntensityWeight() == 0.25
    assert icp._lib.icpmi_get_intensity_weight(icp._h, None) == _capi.ERR_INVALID_ARG
    icp.setConfig(knn=3, max_dist=1.0, outliers=[])               # handle state: a new chain leaves it
    assert icp.getIntensityWeight() == 0.25
    with pytest.raises(amd.icp.InvalidParameter):
        amd.ICPSequence(intensity_weight=1.0)
    with pytest.raises(amd.icp.InvalidParameter):
        amd.ICPSequence(intensity_knn=32)
    icp.close()


def test_map_channel_arguments_and_lifetime(amd):
    from norlab_icp_mapper_amd import _capi
    s = ir.scene("room")
    icp = make_icp(amd)
    row = s["map_intensity"]
    assert icp._lib.icpmi_set_map_intensity(icp._h, row.ctypes.data, row.shape[0], 10) == _capi.ERR_INVALID_ARG      # no map
    icp.setMap(s["map"])
    assert icp._lib.icpmi_set_map_intensity(icp._h, row.ctypes.data, row.shape[0], 10) == _capi.ERR_MISSING_NORMALS
    icp.setMap(s["map"], s["normals"])
    assert icp._lib.icpmi_set_map_intensity(icp._h, row.ctypes.data, row.shape[0] - 1, 10) == _capi.ERR_INVALID_ARG   # m must match
    for knn in (0, 32):
        assert icp._lib.icpmi_set_map_intensity(icp._h, row.ctypes.data, row.shape[0], knn) == _capi.ERR_INVALID_ARG
    assert icp._lib.icpmi_set_map_intensity(icp._h, None, row.shape[0], 10) == _capi.ERR_INVALID_ARG
    # no channel yet: the registration names the missing setter
    icp.setReadingIntensity(s["reading_intensity"])
    with pytest.raises(amd.icp.InvalidField, match="icpmi_set_map_intensity"):
        icp(s["reading"])
    icp.setMapIntensity(row)
    icp.setReadingIntensity(s["reading_intensity"])
    assert np.isfinite(icp(s["reading"])).all()
    # a map change drops the channel
    icp.setMap(s["map"], s["normals"])
    icp.setReadingIntensity(s["reading_intensity"])
    with pytest.raises(amd.icp.InvalidField, match="icpmi_set_map_intensity"):
        icp(s["reading"])
    icp.setMapIntensity(row)
    icp.mapUpdatePointDistance(s["reading"][:50] + F([0, 0, 50, 0]), 0.05, scan_normals=s["reading_normals"][:50])      # ... an append as well
    icp.setReadingIntensity(s["reading_intensity"])
    with pytest.raises(amd.icp.InvalidField, match="icpmi_set_map_intensity"):
        icp(s["reading"])
    icp.close()


def test_reading_row_is_one_shot_and_sized(amd):
    s = ir.scene("room")
    icp, _ = loaded(amd)
    rc = lcs.centred(s["reading"], icp.getMapMean())
    with pytest.raises(amd.icp.InvalidField, match="icpmi_set_reading_intensity"):   # a missing row
        icp(s["reading"])
    with pytest.raises(amd.icp.InvalidParameter, match="icpmi_set_reading_intensity"):
        icp.minimizeStep(rc)
    icp.setReadingIntensity(s["reading_intensity"][:-1])                             # an n mismatch
    with pytest.raises(amd.icp.InvalidField, match="icpmi_set_reading_intensity"):
        icp(s["reading"])
    icp.setReadingIntensity(s["reading_intensity"])
    icp.residual(s["reading"])                                                       # consumed by the call that takes a reading, whatever it is
    with pytest.raises(amd.icp.InvalidField, match="icpmi_set_reading_intensity"):
        icp(s["reading"])
    icp.setReadingIntensity(s["reading_intensity"])
    assert np.isfinite(icp(s["reading"])).all()
    icp.close()


def test_the_reading_rows_share_one_buffer(amd, tol):
    """GenericDescriptorOutlierFilter{source: reading} next to the term: both one-shot rows armed, in either order"""
    from norlab_icp_mapper_amd import _capi
    s = ir.scene("room")
    flags = _capi.GEN_SOURCE_READING            # hard threshold, keep the points whose descriptor is SMALLER than 0.5
    out = {}
    keep = (np.arange(2000) % 2).astype(F)
    for order in ("scalar-first", "intensity-first"):
        icp, _ = loaded(amd, "room", 1, [(_capi.OUT_MAXDIST, ic.MAX_DIST), (_capi.OUT_GENERICDESCRIPTOR, 0.5, flags, 0.0)], max_iterations=3)
        if order == "scalar-first":
            icp.setReadingScalar(keep); icp.setReadingIntensity(s["reading_intensity"])
        else:
            icp.setReadingIntensity(s["reading_intensity"]); icp.setReadingScalar(keep)
        out[order] = icp(s["reading"])
        pairs = icp.stats.pairs
        icp.close()
        assert 0.4 * 2000 < pairs < 0.6 * 2000
    assert np.array_equal(_bits(out["scalar-first"]), _bits(out["intensity-first"]))
    icp, _ = loaded(amd, "room", 1, "maxdist", max_iterations=3)
    icp.setReadingIntensity(s["reading_intensity"])
    every = icp(s["reading"])
    icp.close()
    assert not np.array_equal(_bits(every), _bits(out["scalar-first"]))


@pytest.mark.parametrize("extra, status", [(dict(minimizer=1), "unsupported"), (dict(minimizer=3), "unsupported"), (dict(minimizer=0), "unsupported"),
                                           (dict(force_2d=1), "unsupported"), (dict(is_2d=1), "unsupported"), (dict(covariance=1), "unsupported"),
                                           (dict(degeneracy_threshold=0.01), "unsupported")])
def test_rejected_chains(amd, extra, status):
    """every chain the term is not defined for is refused with a message that names it -- by the registration and by the single step"""
    s = ir.scene("room")
    kw = dict(knn=1, max_dist=ic.MAX_DIST, minimizer=ic.MIN_POINT_TO_PLANE, outliers=ic.CHAINS["maxdist"]["outliers"])
    kw.update(extra)
    icp = amd.ICPSequence(intensity_weight=ic.WEIGHT, **kw)
    icp.setMap(s["map"], s["normals"])
    icp.setMapIntensity(s["map_intensity"])
    rc = lcs.centred(s["reading"], icp.getMapMean())
    icp.setReadingIntensity(s["reading_intensity"])
    with pytest.raises(NotImplementedError, match=TERM):
        icp(s["reading"], s["reading_normals"])
    icp.setReadingIntensity(s["reading_intensity"])
    with pytest.raises(NotImplementedError, match=TERM):
        icp.minimizeStep(rc, None, read_normals=s["reading_normals"])
    icp.setIntensityWeight(0.0)                                    # ... and served as ever without it
    if not extra.get("is_2d"):
        assert np.isfinite(icp(s["reading"], s["reading_normals"])).all()
    icp.close()


def test_rejected_entry_points(amd):
    from norlab_icp_mapper_amd import _capi
    s = ir.scene("room")
    icp, _ = loaded(amd)
    rd = s["reading"]
    T, stats, status = (C.c_float * 16)(), _capi.Stats(), (C.c_int * 1)()
    ptrs, ns = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0)
    assert icp._lib.icpmi_register_batch_dev(icp._h, 1, ptrs, ns, 0, T, C.byref(stats), status) == _capi.ERR_UNSUPPORTED
    assert TERM in icp._lib.icpmi_last_error(icp._h).decode()
    import torch
    prior = np.eye(4, dtype=F)
    d, dt = torch.from_numpy(np.array(rd)).cuda(), torch.zeros(rd.shape[0], dtype=torch.float32).cuda()
    for fn, scan in ((icp._lib.icpmi_register_multistart, rd.ctypes.data), (icp._lib.icpmi_register_multistart_dev, d.data_ptr())):
        assert fn(icp._h, scan, rd.shape[0], prior.ctypes.data, 1, 0, T, C.byref(stats), status) == _capi.ERR_UNSUPPORTED
        assert TERM in icp._lib.icpmi_last_error(icp._h).decode()
    with pytest.raises(NotImplementedError, match=TERM):
        icp.register_sweep(rd, np.zeros(rd.shape[0], F), np.eye(4), np.eye(4))
    with pytest.raises(NotImplementedError, match=TERM):
        icp.register_sweep_dev(d.data_ptr(), rd.shape[0], dt.data_ptr(), np.eye(4), np.eye(4))
    with pytest.raises(NotImplementedError, match=TERM):
        icp.sweep_sums(rd, np.zeros(rd.shape[0], F), np.eye(4), np.eye(4))
    # the residual is the point-to-plane residual, unchanged
    res = icp.residual(rd, kind=0)
    icp.setIntensityWeight(0.0)
    assert icp.residual(rd, kind=0).bits() == res.bits() and res.kind == 2 and res.pairs > 0
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 6. the host shell
YAML_ICP = """matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 2.0
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.85
errorMinimizer:
  IntensityPointToPlaneErrorMinimizer:
    lambdaGeometric: 0.968
    descName: intensity
    gradientKnn: 10
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 8
"""


def test_mapper_runs_the_yaml_minimiser_over_two_scans(amd, tmp_path):
    """scan 0 (the corridor's map cloud with its intensity) builds the map: normals by the post filter, the descriptor kept, the channel set
    behind the index build.  Scan 1 (the reading, prior 0.3 m off along the axis) is registered against it and merged on the host path (the
    resident chain does not carry the descriptor): its pose comes back along the axis -- below a tenth of the offset, where point-to-plane,
    which cannot move along the axis at all, stays at the whole of it -- and the map has grown with the descriptor on it"""
    import host_bindings as hb
    from test_host_cpp import P2PLANE_CONFIG, _build_host
    _build_host()
    lib = hb.load()
    s = ir.scene("corridor")
    head, tail = P2PLANE_CONFIG.split("icp:\n")
    cfg = tmp_path / "intensity.yaml"
    cfg.write_text(head + "icp:\n" + "".join("  " + ln + "\n" for ln in YAML_ICP.splitlines()) + "  inspector: NullInspector\n")
    scans = [np.ascontiguousarray(s["map"]), np.ascontiguousarray(s["reading"])]
    descs = [np.ascontiguousarray(s["map_intensity"]), np.ascontiguousarray(s["reading_intensity"])]
    col = lambda T: np.ascontiguousarray(np.asarray(T, F).T).ravel()
    poses = np.concatenate([col(np.eye(4)), col(ir.START)])
    ns = (C.c_int64 * 2)(*[a.shape[0] for a in scans])
    stamps = (C.c_int64 * 2)(1_000_000_000, 2_000_000_000)
    sp = (C.c_void_p * 2)(*[a.ctypes.data for a in scans])
    dp = (C.c_void_p * 2)(*[a.ctypes.data for a in descs])
    out, sizes, has = np.zeros(32, F), (C.c_int64 * 2)(), (C.c_int * 2)()
    err = C.create_string_buffer(512)
    fn = lib.nim_test_mapper_descriptor_scans
    fn.restype = C.c_int
    rc = fn(str(cfg).encode(), C.c_int(2), sp, ns, b"intensity", dp, C.c_void_p(poses.ctypes.data), stamps, C.c_void_p(out.ctypes.data), sizes, has, err,
            C.c_int(512))
    assert rc == 0, err.value.decode(errors="replace")
    pose = out[16:].reshape(4, 4).T.astype(np.float64)
    print("map sizes", sizes[0], sizes[1], "pose after scan 1: translation", pose[:3, 3])
    assert np.array_equal(out[:16].reshape(4, 4).T, np.eye(4, dtype=F)) and 1000 < sizes[0] <= 8000 and sizes[1] >= sizes[0]
    assert has[0] == 1 and has[1] == 1
    assert abs(pose[ir.AXIS, 3]) < 0.1 * ir.START[ir.AXIS, 3]
    # the C++ chain alone (a hook that carries no descriptor): InvalidField without the row
    import host_chain_bindings as hcb
    with pytest.raises(RuntimeError, match="no 1-row descriptor intensity"):
        hcb.icp_register(YAML_ICP, s["map"], s["normals"], s["reading"])
