"""PointToPlaneWithCovErrorMinimizer on the device (icpmi_get_covariance, csrc/loop.hip: cov_pairs_kernel / cov_solve_kernel).

- the covariance pass changes nothing else: pose, iterations, stop reason and the last iteration's pairs are bit-identical with and
  without it, for k = 1 and 6, graph and eager loops, register / register_prior / register_fixed_dev, Trimmed and MaxDist filters,
  force4DOF;
- its value equals the float64 restatement (tests/covariance_reference.py) over the pairs icpmi_debug_last_matches returns, with
  T_prev = that call's T_used and T_iter = the T_used of the same registration run one iteration longer (so T_s is exact), within a
  tolerance derived from cond(H) (covariance_reference.rel_tol);
- two identical calls give the same bits; every UNSUPPORTED / INVALID_ARG case; the config-4 Mapper replay with the WithCov minimizer
  gives the same 14 poses as with PointToPlaneErrorMinimizer and a finite, positive semidefinite covariance for every registered scan."""
import ctypes as C
import os

import numpy as np
import pytest

import covariance_reference as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TRIM = (4, 0.85)     # TrimmedDistOutlierFilter ratio 0.85
MAXD = (1, 0.6)      # MaxDistOutlierFilter maxDist 0.6


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


_scenes = {}


def scene(name):
    if name not in _scenes:
        from norlab_icp_mapper_amd import synth
        sc = synth.make_scene(m=1_000_000, n=100_000) if name == "headline" else synth.make_scene(m=200_000, n=20_000)
        scan = sc["scan"]
        if name == "misaligned":  # ~0.15 rad / 1.5 m on top of the scene's own offset: large residuals in the first iterations
            Tx = synth.make_T((0.08, -0.05, 0.12), (1.2, -0.8, 0.5)).astype(np.float64)
            scan = scan.copy(); scan[:, :3] = (scan[:, :3].astype(np.float64) @ Tx[:3, :3].T + Tx[:3, 3]).astype(F)
        _scenes[name] = (sc["map"], sc["normals"], scan)
    return _scenes[name]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _centred_map(mp):
    """setMap's centred copy: the mean in double (sequential sum), the difference rounded to float"""
    mean = np.cumsum(mp[:, :3].astype(np.float64), axis=0)[-1] / mp.shape[0]
    return (mp[:, :3].astype(np.float64) - mean).astype(F)


def _run(icp, entry, reading, d, fixed):
    if entry == "register":
        return icp(reading)
    if entry == "prior":
        return icp.registerWithPrior(reading, np.eye(4, dtype=F))
    return icp.registerDev(d.data_ptr(), reading.shape[0], fixed_iterations=fixed)


# ------------------------------------------------------------------------------------------------------------------ pose untouched
CASES = [  # (k, use_graph, entry, outliers, extra)
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
def test_pose_and_pairs_untouched(amd, k, graph, entry, outs, extra):
    import torch
    mp, nm, reading = scene("mid")
    d = torch.from_numpy(reading).cuda()
    res = []
    for cov in (0, 1):
        icp = amd.ICPSequence(knn=k, outliers=outs, use_graph=graph, use_differential=1, covariance=cov, **extra)
        assert icp.setMap(mp, nm)
        out = []
        for _ in range(2):  # the second registration replays the cached graphs
            T = _run(icp, entry, reading, d, 5)
            s = icp.stats
            ids, d2, Tu = icp.lastMatches(reading.shape[0])
            out.append((_bits(T), s.iterations, s.stop_reason, s.pairs, ids, _bits(d2), _bits(Tu)))
            if cov:
                c = icp.errorMinimizer.getCovariance()
                assert c.shape == (6, 6) and c.dtype == F and np.isfinite(c).all()
        res.append(out)
        icp.close()
    for a, b in zip(res[0], res[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ value
def check_value(amd, name, k, outs, j, sigma=0.01, **extra):
    import torch
    mp, nm, reading = scene(name)
    n = reading.shape[0]
    icp = amd.ICPSequence(knn=k, outliers=outs, max_iterations=40, covariance=1, sensor_std_dev=sigma, **extra)
    assert icp.setMap(mp, nm)
    mean = icp.getMapMean()
    d = torch.from_numpy(reading).cuda()
    icp.registerDev(d.data_ptr(), n, fixed_iterations=j)
    cov = icp.errorMinimizer.getCovariance()
    lim = float(icp.stats.trimmed_limit)
    pairs = int(icp.stats.pairs)
    ids, d2, T_prev = icp.lastMatches(n)
    icp.registerDev(d.data_ptr(), n, fixed_iterations=j + 1)
    T_iter = icp.lastMatches(n)[2]
    icp.close()
    # the pairs with w > 0 under the chain
    w = np.isfinite(d2)
    for t, prm in outs:
        w &= (d2 <= F(lim)) if t == 4 else (d2 <= F(prm) * F(prm))
    assert int(w.sum()) == pairs
    qi, qj = np.nonzero(w)
    rc = reading.copy(); rc[:, :3] = reading[:, :3] - mean[None, :]
    p = cr.fma_transform(T_prev, rc)[qi]
    q = _centred_map(mp)[ids[qi, qj]]
    nn = nm[ids[qi, qj]]
    x = cr.step_params(T_iter, T_prev)
    ref, H, _ = cr.covariance(p, q, nn, x, sigma)
    assert ref is not None
    err = np.linalg.norm(cov.astype(np.float64) - ref) / np.linalg.norm(ref)
    tol = cr.rel_tol(H, pairs)
    assert err <= tol, (name, k, j, err, tol, np.linalg.cond(H))
    assert np.array_equal(cov, cov.T)
    return cov, ref, dict(p=p, q=q, n=nn, x=x, H=H, w=w, ids=ids, d2=d2, rc=rc, T_iter=T_iter, T_used=T_prev, mapc=_centred_map(mp), nm=nm, tol=tol)


@pytest.mark.parametrize("k,outs,j", [(1, [TRIM], 2), (1, [MAXD], 3), (6, [TRIM], 2), (6, [MAXD, TRIM], 1), (1, [TRIM], 12)])
def test_value_matches_the_restatement(amd, k, outs, j):
    check_value(amd, "mid", k, outs, j)


def test_value_force4dof_and_sigma(amd):
    c1, _, _ = check_value(amd, "mid", 1, [TRIM], 2, sigma=0.01, force_4dof=1)
    c3, _, _ = check_value(amd, "mid", 1, [TRIM], 2, sigma=0.03, force_4dof=1)
    np.testing.assert_allclose(c3, 9 * c1, rtol=1e-5)


@pytest.mark.parametrize("k", [1, 6])
def test_value_rejects_the_wrong_pair_set_step_and_residual(amd, k):
    """the device's answer is within the tolerance and what a kernel that counts w = 0 pairs, forms p under T_iter or drops E would
    return is far outside it (a misaligned start, one iteration, the trimmed filter drops 15 % of the pairs)"""
    cov, ref, c = check_value(amd, "misaligned", k, [TRIM], 1)
    got = cov.astype(np.float64)
    rel = lambda other: np.linalg.norm(got - other) / np.linalg.norm(other)
    finite = np.isfinite(c["d2"])
    assert (finite & ~c["w"]).sum() > 0.1 * finite.sum()
    ai, aj = np.nonzero(finite)                                        # every finite pair, w = 0 included
    all_pairs, _, _ = cr.covariance(cr.fma_transform(c["T_used"], c["rc"])[ai],
                                    c["mapc"][c["ids"][ai, aj]], c["nm"][c["ids"][ai, aj]], c["x"], 0.01)
    qi, qj = np.nonzero(c["w"])
    under_iter, _, _ = cr.covariance(cr.fma_transform(c["T_iter"], c["rc"])[qi], c["q"], c["n"], c["x"], 0.01)
    h, a, b, E = cr.terms(c["p"], c["q"], c["n"], c["x"])
    a_noE = a.copy()
    a_noE[:, 3:] -= np.cross(c["p"] / np.linalg.norm(c["p"], axis=1)[:, None], c["n"]) * E[:, None]
    Hi = np.linalg.inv(h.T @ h)
    drop_e = 1e-4 * Hi @ (a_noE.T @ a_noE + b.T @ b) @ Hi
    for name, other in (("w = 0 pairs", all_pairs), ("p under T_iter", under_iter), ("E dropped", drop_e)):
        assert rel(other) > 10 * c["tol"], (name, rel(other), c["tol"])


def test_value_headline_shape(amd):
    """100 k x 1 M, k = 1 and 6"""
    check_value(amd, "headline", 1, [TRIM], 2)
    check_value(amd, "headline", 6, [TRIM], 2)


def test_two_calls_give_the_same_bits(amd):
    mp, nm, reading = scene("mid")
    out = []
    for _ in range(2):
        icp = amd.ICPSequence(knn=6, outliers=[TRIM], covariance=1, use_differential=1)
        assert icp.setMap(mp, nm)
        icp(reading)
        out.append(_bits(icp.errorMinimizer.getCovariance()))
        icp(reading)
        out.append(_bits(icp.errorMinimizer.getCovariance()))
        icp.close()
    for o in out[1:]:
        assert np.array_equal(o, out[0])


# ------------------------------------------------------------------------------------------------------------------ errors
def test_unsupported_cases(amd):
    import torch
    mp, nm, reading = scene("mid")
    icp = amd.ICPSequence(outliers=[TRIM], covariance=1)
    with pytest.raises(NotImplementedError):          # nothing computed yet
        icp.errorMinimizer.getCovariance()
    assert icp.setMap(mp, nm)
    icp(reading)
    icp.errorMinimizer.getCovariance()
    d = torch.from_numpy(reading).cuda()
    icp.registerBatchDev([d.data_ptr(), d.data_ptr()], [reading.shape[0]] * 2, fixed_iterations=3)
    with pytest.raises(NotImplementedError):          # a batch came after it
        icp.errorMinimizer.getCovariance()
    icp(reading)
    icp.errorMinimizer.getCovariance()
    assert icp.setMap(mp, nm)
    with pytest.raises(NotImplementedError):          # the map changed: the pairs are gone
        icp.errorMinimizer.getCovariance()
    icp(reading)
    icp.knn(reading[:100].copy(), k=2)
    with pytest.raises(NotImplementedError):          # the matcher's buffers were reused
        icp.errorMinimizer.getCovariance()
    icp(reading)
    icp.setConfig(outliers=[TRIM], covariance=1, use_bound=1, max_trans_norm=1e-6, max_rot_norm=1e-6)
    with pytest.raises(amd.icp.ConvergenceError):
        icp(reading)
    with pytest.raises(NotImplementedError):          # the last registration failed
        icp.errorMinimizer.getCovariance()
    icp.setConfig(outliers=[TRIM], covariance=0)
    icp(reading)
    with pytest.raises(NotImplementedError):          # the chain does not ask for it
        icp.errorMinimizer.getCovariance()
    icp.close()


def test_invalid_configs(amd):
    from norlab_icp_mapper_amd.icp import InvalidParameter
    for kw in (dict(minimizer=1), dict(minimizer=0), dict(is_2d=1), dict(sensor_std_dev=float("nan")), dict(sensor_std_dev=float("inf")),
               dict(sensor_std_dev=-1e-3), dict(covariance=2)):
        with pytest.raises(InvalidParameter):
            amd.ICPSequence(**dict(dict(covariance=1), **kw))
        icp = amd.ICPSequence()
        with pytest.raises(InvalidParameter):
            icp.setConfig(**dict(dict(covariance=1), **kw))
        icp.close()
    amd.ICPSequence(covariance=1, sensor_std_dev=0.0, force_2d=1).close()   # force2D on 3-D clouds is served


def _host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb.load()


def test_host_yaml_rejects_unknown_keys_and_serves_the_name():
    lib = _host()
    fn = lib.nim_test_icp_set_map
    fn.restype = C.c_int
    c = np.ones((100, 4), F); c[:, :3] = np.random.default_rng(1).normal(size=(100, 3))
    out = np.empty_like(c); m = C.c_int64(0); err = C.create_string_buffer(512)
    good = "errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer:\n    sensorStdDev: 0.02\n    force4DOF: 1\n"
    assert fn(good.encode(), C.c_void_p(c.ctypes.data), C.c_int64(100), C.c_void_p(out.ctypes.data), C.byref(m), err, 512) == 0, err.value
    bad = "errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer:\n    sensorStdDv: 0.02\n"
    assert fn(bad.encode(), C.c_void_p(c.ctypes.data), C.c_int64(100), C.c_void_p(out.ctypes.data), C.byref(m), err, 512) == 1
    assert b"unknown parameter sensorStdDv" in err.value
    bad = "errorMinimizer:\n  PointToPointWithCovErrorMinimizer:\n"
    assert fn(bad.encode(), C.c_void_p(c.ctypes.data), C.c_int64(100), C.c_void_p(out.ctypes.data), C.byref(m), err, 512) == 1


# ------------------------------------------------------------------------------------------------------------------ Mapper replay
def _replay(lib, tmp, cfg_text, paths, traj):
    from config4_data import quat_T
    cfg = os.path.join(tmp, "config.yaml")
    open(cfg, "w").write(cfg_text)
    n = len(paths)
    poses = np.stack([quat_T(r[2:]).T.ravel() for r in traj]).astype(F)     # column-major
    stamps = np.array([int(r[0]) * 1_000_000_000 + int(r[1]) for r in traj], np.int64)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    out = np.zeros((n, 16), F); cov = np.zeros((n, 36), F); ok = np.zeros(n, np.int32); err = C.create_string_buffer(1024)
    fn = lib.nim_test_mapper_replay
    fn.restype = C.c_int
    rc = fn(cfg.encode(), C.c_int(n), arr, C.c_void_p(poses.ctypes.data), C.c_void_p(stamps.ctypes.data), C.c_void_p(out.ctypes.data),
            C.c_void_p(cov.ctypes.data), C.c_void_p(ok.ctypes.data), err, 1024)
    assert rc == 0, err.value
    return out, cov.reshape(n, 6, 6), ok


def test_config4_replay_with_cov_minimizer(tmp_path):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    lib = _host()
    z = np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))
    names, traj = write_bundled_dataset(str(tmp_path), z)
    paths = [os.path.join(str(tmp_path), "scans", nm) for nm in names]
    assert "PointToPlaneErrorMinimizer:" in CONFIG4_YAML
    plain, _, ok0 = _replay(lib, str(tmp_path), CONFIG4_YAML, paths, traj)
    withcov, cov, ok = _replay(lib, str(tmp_path), CONFIG4_YAML.replace("PointToPlaneErrorMinimizer:", "PointToPlaneWithCovErrorMinimizer:", 1),
                               paths, traj)
    assert len(names) == 14
    assert np.array_equal(_bits(plain), _bits(withcov))
    assert not ok0.any()
    assert ok[1:].all(), ok                       # the first scan starts the map: nothing to register
    for c in cov[1:]:
        assert np.isfinite(c).all() and np.array_equal(c, c.T)
        assert np.linalg.eigvalsh(c.astype(np.float64)).min() >= -1e-6 * np.abs(c).max()
