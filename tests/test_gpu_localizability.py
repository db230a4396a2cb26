"""Degeneracy-aware point-to-plane ICP on the device (icpmi_config::degeneracy_threshold, icpmi_get_localizability; csrc/solve.h: degen_*).

- step parity: on the five analytic scenes (tests/localizability_reference.py), 6-DOF and force_4dof, at the true pose and off by
  (0.05 rad, 0.3 m), the step of icpmi_minimize_step equals the float64 restatement evaluated on the sums the same call returned, within four
  times the deviation recorded in profiles/localizability_tolerance.json (scripts/localizability_tolerance.py measured it on the device;
  the device works in double and rounds once to float, so the record itself must stay under 1e-5); the projector onto the kept span
  equals the reference's; the scaled step has no component along a degenerate eigenvector;
- report: after a full registration (k = 1 and 6, graph and eager, register / prior / fixed) eigval, pivot, lnorm, weight_sum and
  n_degenerate equal the restatement evaluated on the pairs icpmi_debug_last_matches returns under its T_used; two calls, same bits;
- constraint end to end on the corridor; off and report-only are bit-identical; batch and multistart on a constrained handle are the
  single calls bit for bit; every INVALID_ARG / UNSUPPORTED case; the host shell's YAML keys, report and map-update veto."""
import ctypes as C
import os

import numpy as np
import pytest

import covariance_reference as cr
import localizability_cases as lc
import localizability_reference as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
THR = lc.THR
TRIM = (4, 0.85)     # TrimmedDistOutlierFilter ratio 0.85
MAXD = (1, 0.6)      # MaxDistOutlierFilter maxDist 0.6


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _loc_bits(loc):
    return np.concatenate([np.asarray(loc[k], np.float64).ravel().view(np.uint64) for k in ("eigval", "basis", "pivot")] +
                          [np.array([loc["lnorm"], loc["weight_sum"]], np.float64).view(np.uint64),
                           np.array([loc["n"], loc["n_degenerate"], loc["pairs"], loc["iterations"]], np.uint64), loc["degenerate"].astype(np.uint64)])


# ------------------------------------------------------------------------------------------------------------------ step parity
def test_recorded_tolerance_is_a_rounding_error():
    assert 0.0 < lc.recorded_tolerance() <= 1e-5


@pytest.mark.parametrize("name,four,start", lc.STEP_CASES)
def test_step_parity(amd, name, four, start):
    A, b, W, c, L = lr.exact_system(name)
    exact = lr.localizability_reference(A, b, W, c, L, THR, bool(four))
    deg, inf = exact["mu"][exact["degenerate"]], exact["mu"][~exact["degenerate"]]
    assert (deg * 5 <= THR).all() and (inf >= 5 * THR).all(), exact["mu"]       # the reference's own spectrum keeps clear of the threshold
    r = lc.step_case(amd, name, four, start)
    ref, loc = r["ref"], r["loc"]
    print(name, four, start, "rel_x", r["rel_x"], "mu", loc["eigval"])
    assert loc["n"] == ref["n"] == (4 if four else 6)
    assert loc["n_degenerate"] == ref["n_degenerate"] == (lr.N_DEGENERATE_4DOF if four else lr.N_DEGENERATE)[name]
    assert np.array_equal(loc["degenerate"], ref["degenerate"])
    assert r["rel_x"] <= 4 * lc.recorded_tolerance(), (r["rel_x"], lc.recorded_tolerance())
    # same sums, both in double: the spectra agree to rounding, the kept spans to rounding over the gap (>= 25x around the threshold)
    np.testing.assert_allclose(loc["eigval"], ref["mu"], rtol=0, atol=1e-12 * ref["mu"].max())
    Vk = loc["basis"][:, ~loc["degenerate"]]
    assert np.linalg.norm(Vk @ Vk.T - ref["P_kept"]) <= 1e-8
    np.testing.assert_allclose(loc["basis"].T @ loc["basis"], np.eye(loc["n"]), atol=1e-12)
    ny = np.linalg.norm(r["y_dev"])
    for e in np.nonzero(loc["degenerate"])[0]:
        assert abs(loc["basis"][:, e] @ r["y_dev"]) <= 1e-6 * ny
    assert loc["lnorm"] == pytest.approx(r["L"], rel=1e-12) and loc["weight_sum"] == r["W"] and loc["pairs"] == r["pairs"] and loc["iterations"] == 1


# ------------------------------------------------------------------------------------------------------------------ report
OFFSET = lr.make_T((0.004, -0.006, 0.02), (0.1, 0.3, 0.05))     # recoverable x, z, yaw (and a little roll / pitch), 0.3 m along y
_moved = {}


def moved_reading(name):
    if name not in _moved:
        rd = lr.scene(name)["reading"]
        out = rd.copy()
        out[:, :3] = (rd[:, :3].astype(np.float64) @ OFFSET[:3, :3].T + OFFSET[:3, 3]).astype(F)
        out.setflags(write=False)
        _moved[name] = out
    return _moved[name]


def _centred_map(mp):
    """setMap's centred copy: the mean in double (sequential sum), the difference rounded to float"""
    mean = np.cumsum(mp[:, :3].astype(np.float64), axis=0)[-1] / mp.shape[0]
    return (mp[:, :3].astype(np.float64) - mean).astype(F)


PRIOR = lr.make_T((0.01, -0.02, 0.3), (1.5, -2.0, 0.4)).astype(F)     # a real prior: the scan arrives in the sensor frame


def _run(icp, entry, reading, d, fixed):
    if entry == "register":
        return icp(reading)
    if entry == "prior":
        return icp.registerWithPrior(reading, np.eye(4, dtype=F))
    if entry == "prior_moved":
        return icp.registerWithPrior(reading, PRIOR)
    return icp.registerDev(d.data_ptr(), reading.shape[0], fixed_iterations=fixed)


REPORT_CASES = [  # (scene, k, use_graph, entry, threshold, extra)
    ("corridor", 1, 1, "register", THR, {}),
    ("corridor", 1, 0, "register", -THR, {}),
    ("corridor", 6, 1, "fixed", THR, {}),
    ("tunnel", 6, 0, "prior", THR, {}),
    ("room", 1, 1, "prior", THR, {"force_4dof": 1}),
    ("corridor", 1, 1, "prior_moved", THR, {}),
    ("tunnel", 6, 0, "prior_moved", -THR, {}),
    ("floor", 6, 0, "fixed", -THR, {"force_4dof": 1}),
    ("floor_ceiling", 1, 1, "fixed", THR, {}),
]


@pytest.mark.parametrize("name,k,graph,entry,thr,extra", REPORT_CASES)
def test_report_matches_the_restatement_on_the_last_pairs(amd, name, k, graph, entry, thr, extra):
    import torch
    sc = lr.scene(name)
    reading = moved_reading(name)
    n = reading.shape[0]
    icp = amd.ICPSequence(knn=k, max_dist=2.0, outliers=[MAXD], use_graph=graph, use_differential=1, degeneracy_threshold=thr, **extra)
    assert icp.setMap(sc["map"], sc["normals"])
    mean = icp.getMapMean()
    if entry == "prior_moved":
        # the scan in the sensor frame; what the registration centres is the device's PRIOR * scan, restated here in float32
        Pi = np.linalg.inv(PRIOR.astype(np.float64))
        sensor = np.array(reading)
        sensor[:, :3] = (reading[:, :3].astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(F)
        in_map = np.array(sensor)
        in_map[:, :3] = cr.fma_transform(PRIOR, sensor)
        assert np.array_equal(_bits(icp.transform(PRIOR, sensor)), _bits(in_map))     # (the restatement is the library's transform)
        run_reading, reading = sensor, in_map
    else:
        run_reading = reading
    d = torch.from_numpy(np.array(run_reading)).cuda()
    out = []
    for _ in range(2):      # the second registration replays the cached graphs
        _run(icp, entry, run_reading, d, 5)
        out.append(icp.localizability())
    ids, d2, T_used = icp.lastMatches(n)
    pairs, iters = int(icp.stats.pairs), int(icp.stats.iterations)
    icp.close()
    assert np.array_equal(_loc_bits(out[0]), _loc_bits(out[1]))
    loc = out[1]
    w = np.isfinite(d2) & (d2 <= F(MAXD[1]) * F(MAXD[1]))
    assert int(w.sum()) == pairs == loc["pairs"]
    qi, qj = np.nonzero(w)
    rc = lc.centred(reading, mean)
    p = cr.fma_transform(T_used, rc)[qi]
    A, b, W = lr.pair_sums(p, _centred_map(sc["map"])[ids[qi, qj]], sc["normals"][ids[qi, qj]])
    c0, L = lr.reading_stats(rc)
    c = lr.pivot(T_used, c0)
    ref = lr.localizability_reference(A, b, W, c, L, abs(thr), bool(extra.get("force_4dof")))
    print(name, k, entry, "mu dev", loc["eigval"], "mu ref", ref["mu"])
    assert loc["n"] == ref["n"] and loc["n_degenerate"] == ref["n_degenerate"] and np.array_equal(loc["degenerate"], ref["degenerate"])
    assert loc["iterations"] == iters and loc["weight_sum"] == W
    # The device forms every pair's six features in float32 (three roundings of <= 2^-24 |p| |n| each, |p| <= 11 m from the map's centroid)
    # and sums them exactly; against the float64 features that is a relative perturbation of <= 3 * 6e-8 * 11 / L ~ 4e-7 per feature row, twice
    # that on A_s.  Eigenvalues of a symmetric matrix move by at most |dA_s| <= 1e-6 lambda_max: allowed ten times.
    np.testing.assert_allclose(loc["eigval"], ref["mu"], rtol=0, atol=1e-5 * ref["mu"].max())
    np.testing.assert_allclose(loc["pivot"], c + mean.astype(np.float64), rtol=0, atol=1e-9)     # double sums of the same float32 values, another order
    assert loc["lnorm"] == pytest.approx(L, rel=1e-12)


# ------------------------------------------------------------------------------------------------------------------ constraint end to end
def _residual_pose(T):
    """what is left of the offset after the correction T: x, z (m) and yaw (rad) of T OFFSET"""
    E = np.asarray(T, np.float64) @ OFFSET
    return np.array([E[0, 3], E[2, 3], np.arctan2(E[1, 0], E[0, 0])])


def test_corridor_is_constrained_end_to_end(amd):
    # (MaxDist, not Trimmed: a 0.85 trim drops exactly the end walls' pairs, the 8 % with the 0.3 m residual, and the room turns into a corridor)
    kw = dict(knn=1, max_dist=2.0, outliers=[(1, 1.0)], max_iterations=40, degeneracy_threshold=THR)
    res = {}
    for name in ("room", "corridor"):
        sc = lr.scene(name)
        icp = amd.ICPSequence(**kw)
        assert icp.setMap(sc["map"], sc["normals"])
        T = icp(moved_reading(name))
        res[name] = (T, icp.localizability(), icp.getMapMean())
        icp.close()
    T, loc, mean = res["corridor"]
    corr_err = np.abs(_residual_pose(T))
    E_room = np.asarray(res["room"][0], np.float64) @ OFFSET
    # the accuracy the room reaches, where every direction is observable: its largest translation error and its rotation error.  (What is
    # left there is the scene's, not the solver's: the clouds are 0.2 m apart, and a reading point next to an edge may pair with the other face.)
    room_t, room_r = np.abs(E_room[:3, 3]).max(), np.linalg.norm(lr.step_from_T(E_room)[:3])
    print("room", room_t, room_r, E_room[:3, 3], "corridor", corr_err)
    assert res["room"][1]["n_degenerate"] == 0 and room_t < 5e-3 and room_r < 1e-3      # (the room did register: the start was 0.3 m off)
    assert corr_err[0] <= room_t and corr_err[1] <= room_t and corr_err[2] <= room_r, (corr_err, room_t, room_r)
    assert loc["n_degenerate"] == 1 and loc["degenerate"][0]
    v = loc["basis"][:, 0]
    assert abs(v[4]) >= np.cos(np.radians(2.0)), v             # a translation within 2 degrees of +-y
    u = v[3:] / np.linalg.norm(v[3:])
    # the correction moves the reading's centroid (the pivot every iteration's constraint is stated about) by < 1 mm along that direction:
    # every step has t' . u = 0; what is left is second order in the rotation, (0.02 rad)^2 |c| / 2 ~ 1e-4 m
    c_read = moved_reading("corridor")[:, :3].astype(np.float64).mean(0)
    moved = np.asarray(T, np.float64)[:3, :3] @ c_read + np.asarray(T, np.float64)[:3, 3] - c_read
    assert abs(moved @ u) < 1e-3, moved


# ------------------------------------------------------------------------------------------------------------------ off and report-only
_synth = {}


def synth_scene():
    if not _synth:
        from norlab_icp_mapper_amd import synth
        sc = synth.make_scene(m=50_000, n=5_000)
        _synth.update(map=sc["map"], normals=sc["normals"], scan=sc["scan"])
    return _synth["map"], _synth["normals"], _synth["scan"]


CASES = [  # (k, use_graph, entry, outliers, extra): those of test_gpu_covariance.py::test_pose_and_pairs_untouched
    (1, 1, "register", [TRIM], {}),
    (1, 0, "register", [TRIM], {}),
    (6, 1, "register", [MAXD], {}),
    (6, 0, "prior", [TRIM], {}),
    (1, 1, "fixed", [MAXD], {}),
    (6, 1, "fixed", [TRIM], {}),
    (1, 1, "prior", [TRIM], {"force_4dof": 1}),
    (6, 0, "register", [MAXD, TRIM], {"force_4dof": 1}),
]


@pytest.mark.parametrize("k,graph,entry,outs,extra", CASES)
def test_report_only_leaves_pose_and_pairs_untouched(amd, k, graph, entry, outs, extra):
    import torch
    mp, nm, reading = synth_scene()
    d = torch.from_numpy(reading).cuda()
    res = []
    for thr in (0.0, -THR):
        icp = amd.ICPSequence(knn=k, outliers=outs, use_graph=graph, use_differential=1, degeneracy_threshold=thr, **extra)
        assert icp.setMap(mp, nm)
        out = []
        for _ in range(2):
            T = _run(icp, entry, reading, d, 5)
            s = icp.stats
            ids, d2, Tu = icp.lastMatches(reading.shape[0])
            out.append((_bits(T), s.iterations, s.stop_reason, s.pairs, ids, _bits(d2), _bits(Tu)))
            if thr:
                loc = icp.localizability()
                assert np.isfinite(loc["eigval"]).all() and loc["iterations"] == s.iterations and loc["pairs"] == s.pairs
            else:
                with pytest.raises(NotImplementedError):
                    icp.localizability()
        res.append(out)
        icp.close()
    for a, b in zip(res[0], res[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_batch_and_multistart_are_the_single_calls(amd):
    import torch
    sc = lr.scene("corridor")
    reading = moved_reading("corridor")
    n = reading.shape[0]
    other = np.array(lr.scene("corridor")["reading"])
    d0, d1 = torch.from_numpy(np.array(reading)).cuda(), torch.from_numpy(other).cuda()
    icp = amd.ICPSequence(knn=1, max_dist=2.0, outliers=[TRIM], use_differential=1, degeneracy_threshold=THR)
    assert icp.setMap(sc["map"], sc["normals"])
    for fixed in (0, 5):
        single = []
        for d in (d0, d1):
            T = icp.registerDev(d.data_ptr(), n, fixed_iterations=fixed)
            single.append((_bits(T), icp.stats.iterations, icp.stats.pairs))
        icp.localizability()
        Ts, stats, status = icp.registerBatchDev([d0.data_ptr(), d1.data_ptr()], [n, n], fixed_iterations=fixed)
        assert status == [0, 0]
        for b in range(2):
            assert np.array_equal(_bits(Ts[b]), single[b][0]) and (stats[b].iterations, stats[b].pairs) == single[b][1:]
        with pytest.raises(NotImplementedError):    # after a batch there is nothing to read
            icp.localizability()
    priors = np.stack([np.eye(4), lr.make_T((0, 0, 0.01), (0.05, 0.1, 0.0))]).astype(F)
    single = []
    for P in priors:
        T = icp.registerWithPriorDev(d1.data_ptr(), n, P)
        single.append((_bits(T), icp.stats.iterations, icp.stats.pairs))
    Ts, stats, status = icp.registerMultiStartDev(d1.data_ptr(), n, priors)
    assert list(status) == [0, 0]
    for b in range(2):
        assert np.array_equal(_bits(Ts[b]), single[b][0]) and (stats[b].iterations, stats[b].pairs) == single[b][1:]
    with pytest.raises(NotImplementedError):
        icp.localizability()
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(amd):
    from norlab_icp_mapper_amd import _capi, icp as icpmod
    for bad in (dict(degeneracy_threshold=float("nan")), dict(degeneracy_threshold=float("inf")), dict(degeneracy_threshold=-float("inf")),
                dict(degeneracy_threshold=THR, minimizer=_capi.MIN_POINT_TO_POINT), dict(degeneracy_threshold=-THR, minimizer=_capi.MIN_IDENTITY),
                dict(degeneracy_threshold=THR, force_2d=1), dict(degeneracy_threshold=-THR, is_2d=1)):
        with pytest.raises(icpmod.InvalidParameter, match="degeneracyThreshold"):
            amd.ICPSequence(**bad)
    sc = lr.scene("room")
    icp = amd.ICPSequence(knn=1, max_dist=2.0)
    assert icp.setMap(sc["map"], sc["normals"])
    icp(np.array(sc["reading"]))
    with pytest.raises(NotImplementedError, match="does not ask"):      # option off
        icp.localizability()
    for bad in (dict(degeneracy_threshold=float("nan")), dict(degeneracy_threshold=THR, force_2d=1), dict(degeneracy_threshold=THR, minimizer=_capi.MIN_POINT_TO_POINT)):
        with pytest.raises(icpmod.InvalidParameter, match="degeneracyThreshold"):
            icp.setConfig(**bad)
    icp.setConfig(knn=1, max_dist=2.0, degeneracy_threshold=THR)
    with pytest.raises(NotImplementedError, match="no report"):         # no registration yet on this chain
        icp.localizability()
    icp(np.array(sc["reading"]))
    assert icp.localizability()["n_degenerate"] == 0
    assert icp._lib.icpmi_get_localizability(icp._h, None) == _capi.ERR_INVALID_ARG
    # a new map moves the mean the pivot is stated against: the report of the registration before it is gone, as the covariance is
    shifted = np.array(sc["map"]); shifted[:, :3] += np.array([5.0, -3.0, 1.0], F)
    assert icp.setMap(shifted, sc["normals"])
    with pytest.raises(NotImplementedError, match="no report"):
        icp.localizability()
    icp(np.array(sc["reading"]) + np.array([5.0, -3.0, 1.0, 0.0], F))
    loc = icp.localizability()
    assert loc["n_degenerate"] == 0 and np.abs(loc["pivot"] - (np.array(sc["reading"])[:, :3].astype(np.float64).mean(0) + [5.0, -3.0, 1.0])).max() < 5e-3
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ host shell
def _host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb.load()


def test_host_yaml_keys():
    fn = _host().nim_test_icp_degeneracy_yaml
    fn.restype = C.c_int
    thr = C.c_float(7.0); err = C.create_string_buffer(512)
    parse = lambda text: fn(("errorMinimizer:\n" + text).encode(), C.byref(thr), err, 512)
    assert parse("  PointToPlaneErrorMinimizer:\n    force4DOF: 1\n") == 0 and thr.value == 0.0
    assert parse("  PointToPlaneErrorMinimizer:\n    degeneracyThreshold: 0.005\n") == 0 and thr.value == F(0.005)
    assert parse("  PointToPlaneErrorMinimizer:\n    degeneracyThreshold: 0.005\n    degeneracyAction: report\n") == 0 and thr.value == -F(0.005)
    assert parse("  PointToPlaneWithCovErrorMinimizer:\n    degeneracyThreshold: 0.01\n    degeneracyAction: constrain\n") == 0 and thr.value == F(0.01)
    assert parse("  PointToPlaneWithCovErrorMinimizer:\n    degeneracyTreshold: 0.01\n") == 1 and b"unknown parameter degeneracyTreshold" in err.value
    assert parse("  PointToPlaneErrorMinimizer:\n    degeneracyTreshold: 0.01\n") == 1 and b"unknown parameter degeneracyTreshold" in err.value
    assert parse("  PointToPlaneErrorMinimizer:\n    degeneracyThreshold: 0.01\n    degeneracyaction: report\n") == 1 and b"unknown parameter degeneracyaction" in err.value
    assert parse("  PointToPlaneErrorMinimizer:\n    degeneracyThreshold: 0.01\n    degeneracyAction: ignore\n") == 1 and b"degeneracyAction" in err.value
    assert parse("  PointToPlaneErrorMinimizer:\n    degeneracyThreshold: -0.01\n") == 1 and b"degeneracyThreshold" in err.value
    assert parse("  PointToPlaneErrorMinimizer:\n    degeneracyThreshold: 0.01\n    force2D: 1\n") == 1 and b"force2D" in err.value


def _replay(lib, tmp, cfg_text, paths, traj, max_degenerate=-1):
    from config4_data import quat_T
    from norlab_icp_mapper_amd import _capi
    cfg = os.path.join(tmp, "config.yaml")
    open(cfg, "w").write(cfg_text)
    n = len(paths)
    poses = np.stack([quat_T(r[2:]).T.ravel() for r in traj]).astype(F)     # column-major
    stamps = np.array([int(r[0]) * 1_000_000_000 + int(r[1]) for r in traj], np.int64)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    out = np.zeros((n, 16), F); loc = (_capi.Localizability * n)(); ok = np.zeros(n, np.int32); grew = np.zeros(n, np.int32)
    err = C.create_string_buffer(1024)
    fn = lib.nim_test_mapper_replay_localizability
    fn.restype = C.c_int
    rc = fn(cfg.encode(), C.c_int(n), arr, C.c_void_p(poses.ctypes.data), C.c_void_p(stamps.ctypes.data), C.c_int(max_degenerate),
            C.c_void_p(out.ctypes.data), loc, C.c_void_p(ok.ctypes.data), C.c_void_p(grew.ctypes.data), err, 1024)
    assert rc == 0, err.value
    return out, loc, ok, grew


def test_config4_replay_report_only_and_veto(tmp_path):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    lib = _host()
    z = np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))
    names, traj = write_bundled_dataset(str(tmp_path), z)
    paths = [os.path.join(str(tmp_path), "scans", nm) for nm in names]
    assert len(names) == 14 and "PointToPlaneErrorMinimizer:" in CONFIG4_YAML
    lines = CONFIG4_YAML.split("\n")
    at = next(i for i, ln in enumerate(lines) if "PointToPlaneErrorMinimizer:" in ln)
    pad = " " * (len(lines[at]) - len(lines[at].lstrip()) + 2)
    # a threshold of 1e6 flags every direction: the report-only replay must still be the plain one, and the veto must then stop every update
    report = "\n".join(lines[:at + 1] + [pad + "degeneracyThreshold: 1000000.0", pad + "degeneracyAction: report"] + lines[at + 1:])
    plain, _, ok0, grew0 = _replay(lib, str(tmp_path), CONFIG4_YAML, paths, traj)
    rep, loc, ok, grew = _replay(lib, str(tmp_path), report, paths, traj)
    assert np.array_equal(_bits(plain), _bits(rep)) and np.array_equal(grew0, grew)
    assert not ok0.any() and ok[1:].all() and not ok[0]        # the first scan starts the map: nothing to register
    for r in loc[1:]:
        assert r.n in (4, 6) and np.isfinite(r.eigval[:r.n]).all() and np.isfinite(r.basis[:]).all() and np.isfinite(r.pivot[:]).all()
        assert r.lnorm > 0 and r.weight_sum > 0 and r.pairs > 0 and r.iterations >= 1 and r.n_degenerate == r.n
    vetoed, _, _, grew_v = _replay(lib, str(tmp_path), report, paths, traj, max_degenerate=0)
    assert grew0[1:].any()                                     # (the plain replay does grow its map after the first scan)
    assert grew_v[0] == 1 and not grew_v[1:].any()             # every registered scan is vetoed; the poses are still published
    assert np.isfinite(vetoed).all() and np.array_equal(_bits(vetoed[:2]), _bits(plain[:2]))
