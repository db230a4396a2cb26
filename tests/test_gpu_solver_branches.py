"""The fallback branches of the device's single-lane solve (csrc/solve.h) through the public C ABI, against the float64 reference
(tests/solver_reference.py) and the oracle: the route through the SVD (reflecting, rank 2, rank 1, zero H), the minimum-norm solution
with its Jacobi eigen-decomposition at N = 6, 4, 3 (the tilted floor and the yawed corridors are the cases whose rotations are not trivial), both sides of the 0.5 rad switch of the step's sin / cos, the zero-rotation early
return, the planar closed form with r == 0, and the covariance's FLT_MAX sentinel.  The cases, their margins and the bounds are those
of tests/solver_cases.py; tests/test_solver_branches_cpu.py runs the same check_step on the oracle and sets the constant K there.

Whole registrations: the steps of a composed pose do not commute -- two tilts compose to a little yaw, a yaw moves an
earlier tx into ty -- so "the unobservable components stay exactly at the prior" holds for the composed pose only where one
direction is observable (the floor under force4DOF: everything but tz); it is asserted there, and step by step everywhere
(check_step: exact zeros in x)."""
import numpy as np
import pytest

import covariance_reference as cr
import solver_cases as sc
import solver_reference as sr
from solver_oracle import oracle_step

pytestmark = pytest.mark.gpu

CASES = sc.cases_by_name()
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


_steps = {}


def device_step(amd, name):
    """(T, sums, mc, rc) of icpmi_minimize_step on the case, after the pairing was asserted with icpmi_knn; two calls, same bits"""
    if name in _steps:
        return _steps[name]
    case = CASES[name]
    icp = amd.ICPSequence(**case["kw"])
    assert icp.setMap(case["map4"], case["normals"])
    mc, rc, mean = sr.centre(case["map4"], case["reading4"])
    assert np.array_equal(icp.getMapMean(), mean.astype(F)), (name, icp.getMapMean(), mean)
    ids, d2 = icp.knn(rc, k=1)
    n = rc.shape[0]
    if case["pairing"] == "distance":       # every map point ties: the distances instead
        want = ((rc[:, :3].astype(np.float64) - mc[0, :3]) ** 2).sum(1)
        np.testing.assert_allclose(d2[:, 0], want, rtol=1e-6)
        assert ((ids[:, 0] >= 0) & (ids[:, 0] < n)).all()
    else:
        assert np.array_equal(ids[:, 0], np.arange(n)), name
    T, sums = icp.minimizeStep(rc)
    assert icp.stats.pairs == case["pairs"], (name, icp.stats.pairs)
    T2, sums2 = icp.minimizeStep(rc)
    assert np.array_equal(_bits(T), _bits(T2)) and np.array_equal(sums.view(np.uint64), sums2.view(np.uint64)), name
    icp.close()
    _steps[name] = (T, sums, mc, rc)
    return _steps[name]


_figs = {}


def figures(amd, name):
    if name not in _figs:
        T, sums, mc, rc = device_step(amd, name)
        _figs[name] = sr.check_step(CASES[name], T, sums, mc, rc, sc, "device")
    return _figs[name]


@pytest.mark.parametrize("name", sc.NAMES)
def test_device_step_against_float64(amd, name):
    """1 - 4: pairing, pairs, sums against the float64 sums of the pairs (zeros exact), branch membership from the device's own sums,
    the universal properties, the value against the float64 solve of the system the device solved"""
    fig = figures(amd, name)
    print("\n" + sr.line(fig))


@pytest.mark.parametrize("name", sc.NAMES)
def test_device_step_against_oracle(amd, oracle, name):
    """6: the oracle on the same pairs.  Where the optimum is a set (rank <= 1 H) the two may pick different members of it -- both are
    held to the optimum by check_step --; coincident points have the documented identity"""
    case = CASES[name]
    T = device_step(amd, name)[0]
    To = oracle_step(oracle, case)[0]
    dt, dr = sr.pose_error(T, To)
    print(f"\n{name}: device vs oracle dt {dt:.2e} dr {dr:.2e}")
    if case["unique"] or case["pairing"] == "distance" or case["kw"]["minimizer"] == 2:
        assert dt < sc.DEV_ORACLE_DT and dr < sc.DEV_ORACLE_DR, (name, dt, dr)


def test_threshold_sweep_is_continuous(amd):
    """5: every step met 3 and 4 against the same float64 SVD whichever route the device took; no jump at the switch"""
    figs = [figures(amd, n) for n in sc.SWEEP_NAMES]
    d = np.array([f["ref"]["d"] for f in figs])
    assert len(d) >= 12 and d[0] < 2e-9 and d[-1] > 5e-4 and (d < 1e-6).sum() >= 4 and (d > 1e-6).sum() >= 4, d
    for na, nb, fa, fb in zip(sc.SWEEP_NAMES[:-1], sc.SWEEP_NAMES[1:], figs[:-1], figs[1:]):
        dt, dr = sr.pose_error(device_step(amd, na)[0], device_step(amd, nb)[0])
        assert dt <= fa["bound"][0] + fb["bound"][0] and dr <= fa["bound"][1] + fb["bound"][1], (na, dt, dr)


# --------------------------------------------------------------------------------------------------------- whole registrations
def _registration_reading(name):
    """the case's map displaced in observable directions only"""
    case = CASES[name]
    mp = case["map4"][:, :3].astype(np.float64)
    if name == "p2l_floor_4dof":
        return sc.h4(mp + np.array([0.0, 0.0, 0.03]))
    if name == "p2l_corridor_4dof":
        return sc.h4(sc.move(mp, (0.0, 0.0, 0.004), (0.01, 0.0, -0.015), about=(0, 0, 0)))
    return case["reading4"]


REGISTRATIONS = ["p2l_floor", "p2l_corridor", "p2l_corridor_4dof", "p2l_floor_4dof", "p2p_coplanar"]


@pytest.mark.parametrize("name", REGISTRATIONS)
def test_registration_in_the_fallback(amd, oracle, name):
    """7: iterations, stop reason, pairs equal the oracle's, pose within 1e-4 m / 1e-4 rad; the fixed launch sequence (graph replay) and
    a batch with two fallback members give the single registration's bits.  (Every reading of a rank-deficient MAP is rank deficient:
    the batch that mixes fallback members with a Cholesky member is test_batch_mixes_fallback_and_generic_members.)"""
    import torch
    case = CASES[name]
    kw = dict(case["kw"], max_iterations=15, use_differential=1)
    reading = _registration_reading(name)
    icp = amd.ICPSequence(**kw)
    assert icp.setMap(case["map4"], case["normals"])
    T = icp(reading)
    its, why, pairs = icp.stats.iterations, icp.stats.stop_reason, icp.stats.pairs
    o = oracle.OracleICP(oracle.make_config(nthreads=4, **kw)); o.setMap(case["map4"], case["normals"])
    err, T_ref = o(reading)
    assert err == 0
    assert (its, why, pairs) == (o.stats.iterations, o.stats.stop_reason, o.stats.pairs), (name, its, why, pairs, o.stats.iterations)
    assert pairs == case["pairs"] and its < 15
    dt, dr = amd.synth.pose_error(T, T_ref)
    print(f"\n{name}: {its} iterations, device vs oracle dt {dt:.2e} dr {dr:.2e}")
    assert dt <= 1e-4 and dr <= 1e-4, (name, dt, dr)
    assert np.isfinite(T).all()
    if name == "p2l_floor_4dof":            # one observable direction: everything else exactly the prior
        want = np.eye(4, dtype=F); want[2, 3] = T[2, 3]
        assert np.array_equal(T, want) and abs(float(T[2, 3]) + 0.03) < 1e-5, T
    if name == "p2l_floor":                 # the two tilts and the lift are found (the in-plane shift of the true inverse motion, 1e-4 m, is unobservable)
        gt = sc.rotvec_R((0.004, -0.003, 0.0)).T
        gdr = amd.synth.pose_error(T, np.block([[gt, T[:3, 3:4].astype(np.float64)], [np.zeros((1, 3)), np.ones((1, 1))]]))[1]
        tz = float(T[2, 3]) - float(((np.eye(3) - gt) @ np.array([0, 0, 1.5]) - gt @ np.array([0, 0, 0.02]))[2])
        assert gdr < 1e-4 and abs(tz) < 1e-4, (gdr, tz)
    # the unobservable part of the COMPOSED pose, in the centred frame: every step has exact zeros there (check_step), and composing steps
    # (rotation angles th_j, translations t_k) leaves at most (sum th_j)(sum |t_k|) of translation and (sum th_j)^2 of rotation in them.
    # The first step carries nearly all of the motion and the later ones shrink, so both sums stay below twice the composed pose's own
    # angle / translation: bounds 4 th |t| and 4 th^2 -- first-order drift along a free direction would be 100 x larger
    mean = sr.centre(case["map4"], reading)[2]
    M = np.eye(4); M[:3, 3] = mean
    Mi = np.eye(4); Mi[:3, 3] = -mean
    xc = sr.x_from_T(Mi @ T.astype(np.float64) @ M)
    th, tn = np.linalg.norm(xc[:3]), np.linalg.norm(xc[3:])
    free_t = {"p2l_corridor": [4], "p2l_corridor_4dof": [4], "p2l_floor": [3, 4]}.get(name, [])
    free_r = {"p2l_floor": [2]}.get(name, [])
    print(f"{name}: composed x (centred) {np.array2string(xc, precision=3)}, bounds {4 * th * tn:.2e} m / {4 * th * th:.2e} rad")
    for i in free_t:
        assert abs(xc[i]) <= 4 * th * tn + 1e-7, (name, i, xc, 4 * th * tn)
    for i in free_r:
        assert abs(xc[i]) <= 4 * th * th + 1e-7, (name, i, xc, 4 * th * th)
    d = torch.from_numpy(np.ascontiguousarray(reading, dtype=F)).cuda()
    assert np.array_equal(_bits(icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=its)), _bits(T)), name
    other = np.ascontiguousarray(reading[::2], dtype=F)
    d2 = torch.from_numpy(other).cuda()
    T_other = icp.registerDev(d2.data_ptr(), d2.shape[0])
    st_other = (icp.stats.iterations, icp.stats.stop_reason, icp.stats.pairs)
    for rep in range(2):
        Ts, stats, status = icp.registerBatchDev([d.data_ptr(), d2.data_ptr(), d.data_ptr()], [d.shape[0], d2.shape[0], d.shape[0]])
        assert status == [0, 0, 0]
        assert np.array_equal(_bits(Ts[0]), _bits(T)) and np.array_equal(_bits(Ts[2]), _bits(T)) and np.array_equal(_bits(Ts[1]), _bits(T_other)), name
        assert (stats[0].iterations, stats[0].stop_reason, stats[0].pairs) == (its, why, pairs)
        assert (stats[1].iterations, stats[1].stop_reason, stats[1].pairs) == st_other


@pytest.mark.parametrize("extra", [{}, {"force_4dof": 1}, {"force_2d": 1}], ids=["6dof", "4dof", "2d"])
def test_batch_mixes_fallback_and_generic_members(amd, extra):
    """two rank-deficient members next to a well-conditioned one in one launch sequence (N = 6, 4, 3): over the corridor WITH its end
    wall a full reading is solved by Cholesky, the same reading without the end wall's nine points by the minimum-norm route.  The
    routes are asserted: the open reading never pairs with the end wall, its single step has the exact zero along y that only the
    minimum-norm solution has, the full reading's step moves along y"""
    import torch
    case = CASES["p2l_corridor_with_end_wall"]
    kw = dict(case["kw"], max_iterations=15, use_differential=1, **extra)
    icp = amd.ICPSequence(**kw)
    assert icp.setMap(case["map4"], case["normals"])
    full = case["reading4"]
    open_ = np.ascontiguousarray(full[:-9])
    m = case["map4"].shape[0]
    mc, rc, _ = sr.centre(case["map4"], full)
    T_open, sums_open = icp.minimizeStep(np.ascontiguousarray(rc[:-9]))
    assert icp.stats.pairs == m - 9
    A = np.zeros((6, 6)); A[sr.IU] = sums_open[:21]; A = A + A.T
    assert not A[4].any() and sums_open[25] == 0.0 and T_open[1, 3] == 0.0, (A[4], T_open)      # ny == 0 for every pair: ty is free
    T_full, sums_full = icp.minimizeStep(rc)
    assert sums_full[18] == 9.0 and abs(float(T_full[1, 3]) + 0.012) < 2e-3, (sums_full[18], T_full)   # A[4, 4] = the end wall's pairs
    dev = [torch.from_numpy(x).cuda() for x in (open_, full, open_)]
    single = []
    for d in dev:
        T = icp.registerDev(d.data_ptr(), d.shape[0])
        ids = icp.lastMatches(d.shape[0])[0]
        if d.shape[0] == m - 9:
            assert ids.max() < m - 9, ids.max()                   # never an end-wall point
        else:
            assert np.array_equal(ids[:, 0], np.arange(m))
        single.append((T, icp.stats.iterations, icp.stats.stop_reason, icp.stats.pairs))
    for rep in range(2):
        Ts, stats, status = icp.registerBatchDev([d.data_ptr() for d in dev], [d.shape[0] for d in dev])
        assert status == [0, 0, 0]
        for b, (T, it, why, pairs) in enumerate(single):
            assert np.array_equal(_bits(Ts[b]), _bits(T)) and (stats[b].iterations, stats[b].stop_reason, stats[b].pairs) == (it, why, pairs), b
    assert np.isfinite(Ts[0]).all() and not np.array_equal(Ts[0], Ts[1])
    assert abs(float(Ts[1][1, 3]) + 0.012) < 2e-3 and abs(float(Ts[0][1, 3])) < 1e-3, (Ts[0], Ts[1])   # the end wall fixes y, without it y stays


# --------------------------------------------------------------------------------------------------------------- covariance
def _cov_run(amd, name, j=3, sigma=0.01):
    import torch
    case = CASES[name]
    icp = amd.ICPSequence(**dict(case["kw"], max_iterations=15, covariance=1, sensor_std_dev=sigma))
    assert icp.setMap(case["map4"], case["normals"])
    mc, rc, _ = sr.centre(case["map4"], case["reading4"])
    n = rc.shape[0]
    d = torch.from_numpy(case["reading4"]).cuda()
    icp.registerDev(d.data_ptr(), n, fixed_iterations=j)
    cov = icp.errorMinimizer.getCovariance()
    ids, d2, T_prev = icp.lastMatches(n)
    icp.registerDev(d.data_ptr(), n, fixed_iterations=j)
    assert np.array_equal(_bits(cov), _bits(icp.errorMinimizer.getCovariance()))
    icp.registerDev(d.data_ptr(), n, fixed_iterations=j + 1)
    T_iter = icp.lastMatches(n)[2]
    icp.close()
    assert np.array_equal(ids[:, 0], np.arange(n)), name
    p = cr.fma_transform(T_prev, rc)
    x = cr.step_params(T_iter, T_prev)
    return cov, p, mc[:, :3], case["normals"], x, sigma, n


@pytest.mark.parametrize("name", ["p2l_floor", "p2l_corridor"])
def test_covariance_sentinel_when_H_is_singular(amd, name):
    """8: one plane, a corridor without end wall: H = sum h h^T is not positive definite, the covariance is exactly FLT_MAX I"""
    cov, p, q, nn, x, sigma, n = _cov_run(amd, name)
    want = cr.covariance_f32(p, q, nn, x, sigma)
    assert np.array_equal(want, np.eye(6, dtype=F) * cr.SENTINEL)          # the restatement agrees that there is none
    assert np.array_equal(_bits(cov), _bits(want)), cov


def test_covariance_of_the_corridor_with_end_wall(amd):
    cov, p, q, nn, x, sigma, n = _cov_run(amd, "p2l_corridor_with_end_wall")
    ref, H, _ = cr.covariance(p, q, nn, x, sigma)
    assert ref is not None
    err = np.linalg.norm(cov.astype(np.float64) - ref) / np.linalg.norm(ref)
    tol = cr.rel_tol(H, n)
    print(f"\ncovariance: relative error {err:.2e}, tolerance {tol:.2e}, cond(H) {np.linalg.cond(H):.2e}")
    assert err <= tol, (err, tol)
    var_t = np.diag(cov)[:3]
    assert np.argmax(var_t) == 1 and var_t[1] > 10 * max(var_t[0], var_t[2]), var_t      # the corridor's axis is the weak one
