"""Sweep registration on the device (icpmi_register_sweep*, icpmi_sweep_sums; csrc/sweep.hip).

1. the pair sums: same bits twice; alpha == 0 everywhere reproduces icpmi_minimize_step's sums; alpha == 1 everywhere makes the three time
   moments one; skewed input under distinct poses lies within four times the recorded float32 distance of the float64 reference
   evaluated on the device's own pairs (icpmi_knn + icpmi_outlier_weights on the deskewed, centred scan);
2. end to end on the `room` case: a tenth of the rigid registration's point error, the poses next to the float64 reference's within the
   margin recorded in profiles/sweep_tolerance.json (allowed four times); no motion; a stiff prior;
3. behaviour: out4 == icpmi_deskew with the returned poses, host and device pointers, every refusal, a later registration's bits;
4. the host shell: Mapper::processSweep on an empty and on a filled map."""
import ctypes as C
import math

import numpy as np
import pytest

import covariance_reference as cr
import residual_reference as rr
import sweep_cases as sc
import sweep_reference as sr

pytestmark = pytest.mark.gpu
F = np.float32
LEVER = 10.0             # metres: the arm that turns a rotation error into the pose distance (the room is 20 m long)


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F else np.uint64)


E2E = "the introduction's"      # maxDist 2 with TrimmedDist 0.85: the chain of the end-to-end cases


def _make(amd, k=1, chain="maxdist+trimmed", **extra):
    c = sc.room()
    outs = [(sc.OUT_TRIMMED, sc.TRIM_RATIO)] if chain == E2E else sc.CHAINS[chain]
    icp = amd.ICPSequence(knn=k, max_dist=sc.MAX_DIST, outliers=outs, **extra)
    assert icp.setMap(c["map"], c["normals"])
    return icp


def _span():
    return dict(begin=sr.BEGIN_S, end=sr.END_S, unit=sr.UNIT_S)


def pose_distance(A, B):
    """metres: the larger of the translations' distance and the relative rotation's angle at LEVER"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    R = A[:3, :3].T @ B[:3, :3]
    ang = math.atan2(0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]), 0.5 * (np.trace(R) - 1.0))
    return max(float(np.linalg.norm(A[:3, 3] - B[:3, 3])), LEVER * ang)


def _margin():
    return 4.0 * float(sc.recorded()["pose_margin"])


def _moment_bound(u, pairs):
    """|difference| a re-ordered double sum of `pairs` terms may show: pairs 2^-52 sum |terms|, and sum |w F_i F_j| <= sqrt(M_ii M_jj)"""
    dg = np.sqrt(np.diag(u["M0"]))
    return pairs * 2.0 ** -52 * np.outer(dg, dg), pairs * 2.0 ** -52 * dg * math.sqrt(u["wr2"])


# ------------------------------------------------------------------------------------------------------------------ 1. the pair sums
@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("chain", list(sc.CHAINS))
def test_sums_same_bits_twice(amd, chain, k):
    c = sc.room()
    icp = _make(amd, k, chain)
    for n in sc.NS:
        a, ra = icp.sweep_sums(c["scan"][:n], c["t_rel"][:n], sc.SUMS_T_BEGIN, sc.SUMS_T_END, **_span())
        b, rb = icp.sweep_sums(c["scan"][:n], c["t_rel"][:n], sc.SUMS_T_BEGIN, sc.SUMS_T_END, **_span())
        assert np.array_equal(_bits(a), _bits(b)) and ra.bits() == rb.bits(), (chain, k, n)
        assert a[sr.PAIRS] == ra.pairs > 0 and a[78] == a[79] == 0
    icp.close()


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("chain", list(sc.CHAINS))
def test_alpha_zero_is_the_point_to_plane_system(amd, chain, k):
    c = sc.room()
    icp = _make(amd, k, chain)
    T = sc.STARTS["off"].astype(F)
    mean = icp.getMapMean()
    for n in sc.NS:
        scan = c["scan"][:n]
        s, res = icp.sweep_sums(scan, np.zeros(n, F), T, T, **_span())
        u = sr.unpack(s)
        assert not s[sr.M1:sr.M2 + 21].any() and not s[sr.G1:sr.G1 + 6].any()             # M1, M2, g1 exactly 0
        _, ms = icp.minimizeStep(rr.centre_reading(scan, mean), rr.centred_pose(T, mean))
        assert s[sr.PAIRS] == ms[28] == icp.stats.pairs, (chain, k, n)
        A = np.zeros((6, 6)); A[sr.IU] = ms[:21]; A = A + np.triu(A, 1).T
        bm, bg = _moment_bound(u, s[sr.PAIRS])
        # ... and icpmi_minimize_step's own error: its pair sums join the workgroups' partials as fixed-point limbs of 2^-40 absolute
        # resolution (csrc/common.h: ICPMI_ACC_*), so each of its at most 256 partials (256 slots each, 1024 with k > 1) is off by up to 2^-41
        quantum = min(256, -(-n * k // (256 if k == 1 else 1024))) * 2.0 ** -41
        bm, bg = bm + quantum, bg + quantum
        print(chain, k, n, "pairs", s[sr.PAIRS], "largest |M0 - A|", np.abs(u["M0"] - A).max(), "of", np.abs(A).max(), "largest |g0 + b|",
              np.abs(u["g0"] + ms[21:27]).max(), "of", np.abs(ms[21:27]).max())
        assert (np.abs(u["M0"] - A) <= bm).all(), (chain, k, n)
        assert (np.abs(u["g0"] + ms[21:27]) <= bg).all(), (chain, k, n)                     # (the step's sums hold b = -g0)
        assert abs(u["W"] - ms[27]) <= s[sr.PAIRS] * 2.0 ** -52 * ms[27] + quantum
        assert _bits(res.weighted_point_used_ratio) == _bits(F(icp.stats.weighted_point_used_ratio))
        assert _bits(res.trimmed_limit) == _bits(F(icp.stats.trimmed_limit))
    icp.close()


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("chain", list(sc.CHAINS))
def test_alpha_one_makes_the_moments_one(amd, chain, k):
    c = sc.room()
    icp = _make(amd, k, chain)
    T = sc.STARTS["off"].astype(F)
    for n in sc.NS:
        s, _ = icp.sweep_sums(c["scan"][:n], np.full(n, sr.END_S / sr.UNIT_S, F), T, T, **_span())
        u = sr.unpack(s)
        bm, bg = _moment_bound(u, s[sr.PAIRS])
        assert s[sr.PAIRS] > 0 and u["M0"].any()
        assert (np.abs(u["M1"] - u["M0"]) <= bm).all() and (np.abs(u["M2"] - u["M0"]) <= bm).all() and (np.abs(u["g1"] - u["g0"]) <= bg).all()
    icp.close()


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("chain", list(sc.CHAINS))
def test_skewed_sums_against_float64(amd, chain, k):
    c = sc.room()
    icp = _make(amd, k, chain)
    mean = icp.getMapMean()
    assert np.array_equal(mean, c["mean"])
    mapc = rr.centred_map(c["map"], mean)
    mp64, mu = c["map"][:, :3].astype(np.float64), mean.astype(np.float64)
    Tb, Te = sc.SUMS_T_BEGIN.astype(F), sc.SUMS_T_END.astype(F)
    tol = 4.0 * float(sc.recorded()["sums_float32"])
    for n in sc.NS:
        scan, t_rel = c["scan"][:n], c["t_rel"][:n]
        alpha = sr.alpha_of(t_rel)
        s, res = icp.sweep_sums(scan, t_rel, Tb, Te, **_span())
        # the device's own pairs: the deskew under the poses the call ran with, centred, moved as the matcher moves it
        work = icp.deskew(scan, t_rel, sr.STAMPS, res.pose7, ref=sr.END_S, unit=sr.UNIT_S, extrapolate=True)
        moved = np.ones((n, 4), F)
        moved[:, :3] = cr.fma_transform(rr.centred_pose(Te, mean), rr.centre_reading(work, mean))
        ids, d2 = icp.knn(moved, k=k, max_dist=sc.MAX_DIST)
        w, _ = icp.outlierWeights(d2, ids=ids)
        qi, qj = np.nonzero(ids >= 0)
        m = ids[qi, qj]
        a32, _ = sr.sums32(moved[qi, :3], mapc[m], c["normals"][m], w[qi, qj], alpha[qi])
        P64 = sr.world_points(scan, alpha, Tb.astype(np.float64), Te.astype(np.float64))
        f64, gs = sr.sums64(P64[qi] - mu, mp64[m] - mu, c["normals"][m], w[qi, qj], alpha[qi])
        dev, dev32 = sr.deviation(s, f64, gs), sr.deviation(s, a32, gs)
        print(chain, k, n, "device vs float64", dev, "allowed", tol, "| device vs float32 restatement", dev32)
        assert dev <= tol, (chain, k, n, dev, tol)
        assert dev32 <= 1e-12, (chain, k, n, dev32)                                        # the restatement IS the device's arithmetic
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 2. end to end
_runs = {}


def _end_to_end(amd, case, start, lam=0.0):
    """(device result, reference poses, the case) -- computed once per (case, start, prior weight)"""
    key = (case, start, lam)
    if key not in _runs:
        c = sc.room() if case == "room" else sc.static_room()
        icp = _make(amd, 1, E2E)
        T0 = sc.STARTS[start].astype(F)
        res = icp.register_sweep(c["scan"], c["t_rel"], T0, T0, max_iterations=sc.ITERATIONS, min_step_rot=0.0, min_step_trans=0.0,
                                 lambda_rot=lam, lambda_trans=lam, **_span())
        mu = icp.getMapMean().astype(np.float64)
        icp.close()
        ref = sr.register_sweep(c["map"], c["normals"], c["scan"], c["alpha"], T0.astype(np.float64), T0.astype(np.float64), mu, sc.MAX_DIST,
                                sc.TRIM_RATIO, sc.ITERATIONS, lam, lam)
        _runs[key] = (res, ref, c)
    return _runs[key]


@pytest.mark.parametrize("start", ["off", "true"])
def test_room_end_to_end(amd, start):
    res, (Tb, Te, _, _), c = _end_to_end(amd, "room", start)
    assert res.iterations == sc.ITERATIONS and res.stop_reason == 1 and res.pairs > 1000
    mean_err, max_err = sr.point_error(sr.world_points(c["scan"], c["alpha"], res.T_begin, res.T_end), c["truth"])
    # icpmi_register on the same skewed scan, same chain, same iteration count
    icp = _make(amd, 1, E2E, max_iterations=sc.ITERATIONS, use_differential=0)
    T0 = sc.STARTS[start].astype(F)
    T = icp(icp.transform(T0, c["scan"])).astype(np.float64) @ T0.astype(np.float64)
    assert icp.stats.iterations == sc.ITERATIONS
    icp.close()
    x3 = c["scan"][:, :3].astype(np.float64)
    rigid_err, _ = sr.point_error(x3 @ T[:3, :3].T + T[:3, 3], c["truth"])
    d = max(pose_distance(res.T_begin, Tb), pose_distance(res.T_end, Te))
    print(start, "sweep", mean_err, max_err, "rigid", rigid_err, "pose distance to the reference", d, "allowed", _margin())
    assert mean_err <= 0.1 * rigid_err
    assert d <= _margin()
    assert np.allclose(sr.T_of_pose7(res.pose7[1]), res.T_end, atol=1e-6)


def test_no_motion_stays_no_motion(amd):
    res, (Tb, Te, _, _), c = _end_to_end(amd, "static", "off")
    rel = np.linalg.inv(res.T_begin.astype(np.float64)) @ res.T_end.astype(np.float64)
    d = pose_distance(rel, np.linalg.inv(Tb) @ Te)
    print("relative motion against the reference's", d, "against none", pose_distance(rel, np.eye(4)), "allowed", _margin())
    assert d <= _margin()


def test_stiff_prior_keeps_the_relative_motion(amd):
    res, (Tb, Te, _, _), c = _end_to_end(amd, "room", "off", 1e6)
    rel = np.linalg.inv(res.T_begin.astype(np.float64)) @ res.T_end.astype(np.float64)
    print("T_end against the reference", pose_distance(res.T_end, Te), "relative motion", pose_distance(rel, np.eye(4)), "allowed", _margin())
    assert pose_distance(res.T_end, Te) <= _margin()
    assert pose_distance(rel, np.eye(4)) <= _margin()


# ------------------------------------------------------------------------------------------------------------------ 3. behaviour
def test_out_cloud_host_and_device_pointers(amd):
    import torch
    c = sc.room()
    n = 1000
    scan, t_rel = c["scan"][:n], c["t_rel"][:n]
    T0 = sc.STARTS["off"].astype(F)
    icp = _make(amd, 1, "maxdist+trimmed")
    res, cloud = icp.register_sweep(scan, t_rel, T0, T0, max_iterations=4, with_cloud=True, **_span())
    want = icp.deskew(scan, t_rel, sr.STAMPS, res.pose7, ref=sr.END_S, unit=sr.UNIT_S, extrapolate=True)
    assert np.array_equal(_bits(cloud), _bits(want))
    assert not np.array_equal(cloud, scan)
    d_scan, d_t, d_out = torch.from_numpy(scan).cuda(), torch.from_numpy(t_rel).cuda(), torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    dev = icp.register_sweep_dev(d_scan.data_ptr(), n, d_t.data_ptr(), T0, T0, max_iterations=4, d_out_ptr=d_out.data_ptr(), **_span())
    assert dev.bits() == res.bits()
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(cloud))
    assert icp.register_sweep(scan, t_rel, T0, T0, max_iterations=4, **_span()).bits() == res.bits()         # and the same bits twice
    # the step thresholds end the iteration early: the chain's defaults against none
    early = icp.register_sweep(scan, t_rel, T0, T0, max_iterations=30, min_step_rot=1e-3, min_step_trans=1e-2, **_span())
    assert early.stop_reason == 2 and early.iterations < 30
    icp.close()


def test_refusals(amd):
    I = amd.icp
    c = sc.room()
    scan, t_rel = c["scan"][:257], c["t_rel"][:257]
    T = np.eye(4, dtype=F)
    ok = dict(_span(), max_iterations=2)
    for extra in (dict(force_4dof=1), dict(force_2d=1), dict(is_2d=1), dict(covariance=1), dict(degeneracy_threshold=5e-3), dict(minimizer=1),
                  dict(minimizer=0)):
        icp = amd.ICPSequence(knn=1, max_dist=sc.MAX_DIST, **extra)                          # (refused before the map is looked at)
        with pytest.raises(I.InvalidParameter):
            icp.register_sweep(scan, t_rel, T, T, **ok)
        with pytest.raises(I.InvalidParameter):
            icp.sweep_sums(scan, t_rel, T, T, **_span())
        icp.close()
    icp = amd.ICPSequence(knn=1, max_dist=sc.MAX_DIST, minimizer=3)
    with pytest.raises(I.InvalidParameter):
        icp.register_sweep(scan, t_rel, T, T, **ok)                      # plane-to-plane
    icp.close()
    icp = amd.ICPSequence(knn=1, max_dist=sc.MAX_DIST)
    with pytest.raises(I.InvalidParameter, match="no map"):
        icp.register_sweep(scan, t_rel, T, T, **ok)
    empty = icp.register_sweep(scan[:0], t_rel[:0], sc.STARTS["off"], T, **ok)                 # n == 0: the priors, whatever the map
    assert np.array_equal(empty.T_begin, sc.STARTS["off"].astype(F)) and np.array_equal(empty.T_end, T) and empty.iterations == 0
    assert icp.setMap(c["map"])                                          # no normals
    with pytest.raises(I.InvalidField):
        icp.register_sweep(scan, t_rel, T, T, **ok)
    assert icp.setMap(c["map"], c["normals"])
    bad = T.copy(); bad[0, 0] = 1.01
    for Tb, Te in ((bad, T), (T, bad)):
        with pytest.raises(I.TransformationError):
            icp.register_sweep(scan, t_rel, Tb, Te, **ok)
    for kw in (dict(begin=0.1, end=0.1), dict(begin=0.2, end=0.1), dict(begin=float("nan")), dict(end=float("inf")), dict(unit=0.0), dict(unit=float("nan")),
               dict(lambda_rot=-1.0), dict(lambda_trans=float("inf")), dict(min_step_rot=float("nan")), dict(max_iterations=0)):
        with pytest.raises(I.InvalidParameter):
            icp.register_sweep(scan, t_rel, T, T, **dict(ok, **kw))
    t_nan = t_rel.copy(); t_nan[100] = np.nan
    with pytest.raises(I.InvalidParameter, match="NaN"):
        icp.register_sweep(scan, t_nan, T, T, **ok)
    with pytest.raises(I.InvalidParameter):
        icp.register_sweep(scan, t_rel[:10], T, T, **ok)
    for robust in ((7, 1.0, 0 | (2 << 4), 0.0), (7, 1.0, 0 | (1 << 4), 2.0)):              # iteration state: refused as icpmi_residual_error refuses them
        icp.setConfig(knn=1, max_dist=sc.MAX_DIST, outliers=[robust])
        with pytest.raises(NotImplementedError, match="RobustOutlierFilter"):
            icp.register_sweep(scan, t_rel, T, T, **ok)
    icp.setConfig(knn=1, max_dist=1e-6)
    with pytest.raises(I.ConvergenceError, match="no point to minimize"):
        icp.register_sweep(scan, t_rel, T, T, **ok)
    icp.setConfig(knn=1, max_dist=sc.MAX_DIST)
    assert icp.register_sweep(scan, t_rel, T, T, **ok).iterations == 2                      # the handle serves the next call
    icp.close()


@pytest.mark.parametrize("k", sc.KS)
def test_a_later_registration_is_untouched(amd, k):
    c = sc.room()
    T0 = sc.STARTS["off"].astype(F)
    runs = []
    for sweep in (False, True):
        icp = _make(amd, k, "maxdist+trimmed", max_iterations=sc.ITERATIONS)
        moved = icp.transform(T0, c["scan"])
        out = []
        for _ in range(2):
            T = icp(moved)
            s = icp.stats
            out += [_bits(T), s.iterations, s.stop_reason, s.pairs, _bits(F(s.weighted_point_used_ratio)), _bits(F(s.trimmed_limit))]
            if sweep:
                icp.register_sweep(c["scan"][:257], c["t_rel"][:257], T0, T0, max_iterations=2, **_span())
                icp.sweep_sums(c["scan"], c["t_rel"], T0, T0, **_span())
        icp.close()
        runs.append(out)
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ 4. the host shell
def test_mapper_process_sweep_on_an_empty_and_on_a_filled_map(amd, tmp_path):
    """scan 0 (the room's map cloud, no motion) meets an empty map: the priors are the motion and the map is built from it (normals by
    the post filter).  Scan 1 (the skewed room scan, both priors "off") is registered as a motion against that map: the estimated motion puts
    the points within a centimetre of where they were measured (the float64 reference with exact normals reaches 1.4 mm; the priors are
    0.3 m off), and the mapper goes on from the end pose."""
    import host_bindings as hb
    from norlab_icp_mapper_amd import _capi
    from test_host_cpp import P2PLANE_CONFIG, _build_host
    _build_host()
    lib = hb.load()
    c = sc.room()
    cfg = tmp_path / "sweep.yaml"
    cfg.write_text(P2PLANE_CONFIG)
    scans = [np.ascontiguousarray(c["map"]), np.ascontiguousarray(c["scan"])]
    times = [np.zeros(scans[0].shape[0], F), np.ascontiguousarray(c["t_rel"])]
    off = sc.STARTS["off"].astype(F)
    col = lambda T: np.ascontiguousarray(np.asarray(T, F).T).ravel()
    pb = np.concatenate([col(np.eye(4)), col(off)])
    pe = np.concatenate([col(np.eye(4)), col(off)])
    ns = (C.c_int64 * 2)(*[s.shape[0] for s in scans])
    stamps = (C.c_int64 * 2)(1_000_000_000, 2_000_000_000)
    sp = (C.c_void_p * 2)(*[s.ctypes.data for s in scans])
    tp = (C.c_void_p * 2)(*[t.ctypes.data for t in times])
    b_out, e_out, p_out = np.zeros(32, F), np.zeros(32, F), np.zeros(32, F)
    res = (_capi.SweepResult * 2)()
    sizes = (C.c_int64 * 2)()
    err = C.create_string_buffer(512)
    fn = lib.nim_test_mapper_sweep
    fn.restype = C.c_int
    rc = fn(str(cfg).encode(), C.c_int(2), sp, ns, tp, C.c_void_p(pb.ctypes.data), C.c_void_p(pe.ctypes.data), stamps, C.c_double(sr.BEGIN_S),
            C.c_double(sr.END_S), C.c_int(sc.ITERATIONS), C.c_void_p(b_out.ctypes.data), C.c_void_p(e_out.ctypes.data), res,
            C.c_void_p(p_out.ctypes.data), sizes, err, C.c_int(512))
    assert rc == 0, err.value.decode(errors="replace")
    T = lambda a, i: a[16 * i:16 * i + 16].reshape(4, 4).T
    # the empty map: the priors as they came, no iteration, the map built from the scan
    assert np.array_equal(T(b_out, 0), np.eye(4, dtype=F)) and np.array_equal(T(e_out, 0), np.eye(4, dtype=F)) and res[0].iterations == 0
    assert 1000 < sizes[0] <= scans[0].shape[0]
    # the filled map
    assert 1 <= res[1].iterations <= sc.ITERATIONS and res[1].pairs > 1000
    before, _ = sr.point_error(sr.world_points(c["scan"], c["alpha"], off, off), c["truth"])
    after, worst = sr.point_error(sr.world_points(c["scan"], c["alpha"], T(b_out, 1), T(e_out, 1)), c["truth"])
    print("mean point error under the priors", before, "under the estimated motion", after, "max", worst, "iterations", res[1].iterations)
    assert after < 0.01 < before
    assert np.array_equal(T(p_out, 1), T(e_out, 1))                                       # the mapper's pose is the end pose
    assert sizes[1] >= sizes[0]
