"""Many candidate poses in one call (icpmi_residual_error_poses*, icpmi_register_multistart*) and relocalisation from them.

Every check is bit equality against entries that existed before these calls: out[p] (as bytes) and status[p] equal
icpmi_residual_error_dev under T[p] on the same handle, whatever poses share a launch; a start of a multistart equals
icpmi_register_prior_dev alone.
1. the chains the batched route serves (tests/test_gpu_batch.py's CHAINS on mid_scene): n in (1, 63, 64, 65, 257, 1000), 1 / 2 / 16 / 17 / 33
   poses cycling through the scene's pose, identity, a quarter turn, 1000 m away (nothing to match) and a matrix that is not rigid, failing
   poses at positions 0, 15, 16 and inside a chunk; twice, reversed, from host pointers;
2. the chains it does not serve: same bytes, batched == 0, a one-shot row serves every pose and is gone afterwards;
3. the handle afterwards; 4. every whole-call error leaves out and status zeroed; 5. multistart; 6. relocalisation through icp.py and
   through the host shell, on the candidate set tests/test_residual_poses_cpu.py separates in float64 in both of a relocalisation's
   rankings: the winner's index is the true candidate's with the default options, and its pose lies within POSE_TOL_* of the ground truth."""
import ctypes as C
import os

import numpy as np
import pytest

import relocalize_bindings as rb
import relocalize_cases as rc
import residual_reference as rr
from test_gpu_batch import CHAINS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NS = (1, 63, 64, 65, 257, 1000)
NPOSES = (1, 2, 16, 17, 33)
ERR_INVALID_ARG, ERR_NO_POINT, ERR_NO_OUTLIER, ERR_MISSING_NORMALS, ERR_UNSUPPORTED = 1, 3, 4, 7, 8


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def _cm(poses):
    P = np.asarray(poses, F).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(-1)


def single(icp, d_ptr, n, T, d_normals=None, kind=0):
    """icpmi_residual_error_dev: (status, the icpmi_residual's bytes)"""
    from norlab_icp_mapper_amd import _capi
    res = _capi.Residual()
    Tc = _cm(T)
    st = icp._lib.icpmi_residual_error_dev(icp._h, d_ptr, int(n), d_normals, Tc.ctypes.data, int(kind), C.byref(res))
    return int(st), bytes(res)


def many(icp, ptr, n, poses, normals=None, kind=0, host=False, prefill=False, n_poses=None, with_status=True):
    """icpmi_residual_error_poses[_dev]: (return value, [bytes per pose], [status per pose], batched)"""
    from norlab_icp_mapper_amd import _capi
    Tc = _cm(poses)
    P = Tc.shape[0] // 16 if n_poses is None else n_poses
    cap = max(P, 1)
    res = (_capi.Residual * cap)(); status = (C.c_int * cap)(); batched = C.c_int32(-7)
    if prefill:
        C.memset(res, 0xFF, C.sizeof(res)); C.memset(status, 0xFF, C.sizeof(status))
    fn = icp._lib.icpmi_residual_error_poses if host else icp._lib.icpmi_residual_error_poses_dev
    rv = fn(icp._h, ptr, int(n), normals, Tc.ctypes.data if Tc.size else None, P, int(kind), res, status if with_status else None, C.byref(batched))
    return int(rv), [bytes(res[i]) for i in range(P)], [int(status[i]) for i in range(P)], batched.value


def pose_kinds(sc):
    from norlab_icp_mapper_amd import synth
    far = np.eye(4, dtype=F); far[0, 3] = 1000.0
    bad = np.eye(4, dtype=F); bad[0, 0] = 1.01
    return [np.asarray(sc["T_gt"], F), np.eye(4, dtype=F), synth.make_T((0, 0, np.pi / 2), (0, 0, 0)).astype(F), far, bad]


def pose_list(P):
    """indices into pose_kinds: the cycle, with the failing kinds (3: far, 4: not rigid) also at positions 0, 15, 16 and mid-chunk"""
    kinds = [i % 5 for i in range(P)]
    for pos, k in ((0, 3), (7, 4), (15, 4), (16, 3), (23, 3)):
        if pos < P:
            kinds[pos] = k
    return kinds


# ------------------------------------------------------------------------------------------------------------------ 1. served chains
@pytest.mark.parametrize("name", list(CHAINS))
def test_served_chains_equal_the_single_call(amd, mid_scene, name):
    import torch
    sc = mid_scene
    icp = amd.ICPSequence(**CHAINS[name])
    assert icp.setMap(sc["map"], sc["normals"])
    kinds = pose_kinds(sc)
    quant = any(o[0] in (3, 4) for o in CHAINS[name]["outliers"])
    for n in NS:
        reading = np.ascontiguousarray(sc["scan"][:n])
        d = torch.from_numpy(reading).cuda()
        ref = [single(icp, d.data_ptr(), n, T) for T in kinds]                 # one single call per kind of pose, shared below
        assert ref[3][0] == (ERR_NO_OUTLIER if quant else ERR_NO_POINT) and ref[4][0] == ERR_INVALID_ARG, (name, n, ref[3][0], ref[4][0])
        assert ref[0][0] == 0 and ref[1][0] == 0, (name, n)
        for P in NPOSES:
            idx = pose_list(P)
            poses = [kinds[i] for i in idx]
            rigid = sum(1 for i in idx if i != 4)
            rv, out, status, batched = many(icp, d.data_ptr(), n, poses)
            tag = (name, n, P)
            assert rv == 0, tag
            assert status == [ref[i][0] for i in idx], tag
            assert out == [ref[i][1] for i in idx], tag
            assert batched == rigid, tag
            assert many(icp, d.data_ptr(), n, poses) == (rv, out, status, batched), tag                   # twice
            rv2, out2, status2, batched2 = many(icp, d.data_ptr(), n, poses[::-1])                        # reversed
            assert (rv2, out2[::-1], status2[::-1], batched2) == (rv, out, status, batched), tag
            assert many(icp, reading.ctypes.data, n, poses, host=True) == (rv, out, status, batched), tag  # host pointers
        # status == NULL: the first per-pose error is the return value
        rv, out, _, _ = many(icp, d.data_ptr(), n, [kinds[0], kinds[4], kinds[3]], with_status=False)
        assert rv == ERR_INVALID_ARG and out == [ref[0][1], ref[4][1], ref[3][1]]
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 2. unserved chains
TRIM, MED, MAXD = (4, 0.85), (3, 1.5), (1, 0.6)
UNSERVED = {
    "knn6": dict(knn=6, outliers=[TRIM]),
    "maxdist+trimmed+median": dict(knn=1, outliers=[MAXD, TRIM, MED]),         # two quantile filters
    "surface_normal": dict(knn=1, outliers=[TRIM, (5, 0.5)]),                  # reads the reading's normals
    "generic_soft_reading": dict(knn=1, outliers=[(6, 0.1, 1 | 2, 0.0)]),      # GenericDescriptor{source: reading, soft}: a one-shot row
}


@pytest.mark.parametrize("name", list(UNSERVED))
def test_unserved_chains_run_pose_after_pose(amd, name):
    import torch
    sc = rr.scene()
    icp = amd.ICPSequence(max_dist=sc["max_dist"], minimizer=2, **UNSERVED[name])
    assert icp.setMap(sc["map"], sc["normals"])
    kinds = pose_kinds(sc)
    kinds[0] = sc["pose"]
    for n in (65, 1000):
        reading = np.ascontiguousarray(sc["scan"][:n])
        d = torch.from_numpy(reading).cuda()
        nrm = torch.from_numpy(np.ascontiguousarray(sc["scan_normals"][:n])).cuda() if name == "surface_normal" else None
        nptr = None if nrm is None else nrm.data_ptr()
        row = ((np.arange(n) % 5).astype(F) / F(4)) if name == "generic_soft_reading" else None
        arm = (lambda: icp.setReadingScalar(row)) if row is not None else (lambda: None)
        ref = []
        for T in kinds:
            arm()
            ref.append(single(icp, d.data_ptr(), n, T, nptr))
        assert ref[0][0] == 0 and ref[4][0] == ERR_INVALID_ARG
        for P in (1, 2, 17):
            idx = pose_list(P)
            arm()                                                                 # once: the row serves every pose
            rv, out, status, batched = many(icp, d.data_ptr(), n, [kinds[i] for i in idx], nptr)
            assert rv == 0 and batched == 0, (name, n, P)
            assert status == [ref[i][0] for i in idx], (name, n, P)
            assert out == [ref[i][1] for i in idx], (name, n, P)
        if row is not None:                                                       # ... and is gone afterwards
            st, _ = single(icp, d.data_ptr(), n, kinds[0], nptr)
            assert st == ERR_INVALID_ARG and "icpmi_set_reading_scalar" in icp._lib.icpmi_last_error(icp._h).decode()
            rv, out, status, _ = many(icp, d.data_ptr(), n, [kinds[0]] * 3, nptr, prefill=True)
            assert rv == ERR_INVALID_ARG and out == [bytes(len(out[0]))] * 3 and status == [0] * 3
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 3. the handle afterwards
def test_the_handle_afterwards(amd, mid_scene):
    import torch
    sc = mid_scene
    reading = np.ascontiguousarray(sc["scan"][:5000])
    d = torch.from_numpy(reading).cuda()
    poses = [pose_kinds(sc)[i] for i in pose_list(17)]
    runs = []
    for evaluate in (False, True):
        icp = amd.ICPSequence(covariance=1, max_iterations=30, use_differential=1, **CHAINS["p2plane_trimmed"])
        assert icp.setMap(sc["map"], sc["normals"])
        out = []
        for _ in range(2):
            T = icp.registerDev(d.data_ptr(), reading.shape[0])
            s = icp.stats
            out += [T.view(np.uint32), s.iterations, s.stop_reason, s.pairs, np.float32(s.trimmed_limit).view(np.uint32)]
            if evaluate:
                rv, _, status, batched = many(icp, d.data_ptr(), reading.shape[0], poses)
                assert rv == 0 and batched == sum(1 for i in pose_list(17) if i != 4) and status[1] == 0
            out.append(icp.errorMinimizer.getCovariance().view(np.uint32))        # still the registration's matrix
        if evaluate:
            with pytest.raises(NotImplementedError):
                icp.lastMatches(reading.shape[0])                                 # the matcher's buffers were reused
        icp.close()
        runs.append(out)
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ 4. errors
def test_whole_call_errors_leave_the_outputs_zeroed(amd):
    import torch
    sc = rr.scene()
    n = 257
    reading = np.ascontiguousarray(sc["scan"][:n])
    d = torch.from_numpy(reading).cuda()
    nrm = torch.from_numpy(np.ascontiguousarray(sc["scan_normals"][:n])).cuda()
    poses = [sc["pose"], np.eye(4, dtype=F), sc["pose"]]

    def refused(icp, code, text=None, **kw):
        args = dict(ptr=d.data_ptr(), n=n, poses=poses)
        args.update(kw)
        rv, out, status, batched = many(icp, args.pop("ptr"), args.pop("n"), args.pop("poses"), prefill=True, **args)
        assert rv == code, (rv, code, icp._lib.icpmi_last_error(icp._h).decode())
        assert all(o == bytes(len(o)) for o in out) and not any(status) and batched == 0
        if text:
            assert text in icp._lib.icpmi_last_error(icp._h).decode()

    icp = amd.ICPSequence(max_dist=rr.MAX_DIST, minimizer=2, outliers=[TRIM])
    refused(icp, ERR_INVALID_ARG, "no map")
    assert icp.setMap(sc["map"])                                                   # no normals on the map
    refused(icp, ERR_MISSING_NORMALS, "normals")
    refused(icp, ERR_MISSING_NORMALS, "normals", kind=2)
    assert icp.setMap(sc["map"], sc["normals"])
    refused(icp, ERR_INVALID_ARG, kind=3)
    refused(icp, ERR_INVALID_ARG, kind=-1)
    refused(icp, ERR_INVALID_ARG, ptr=None)                                        # null reading
    refused(icp, ERR_INVALID_ARG, poses=np.zeros((0, 4, 4), F), n_poses=3)         # null poses
    refused(icp, ERR_INVALID_ARG, poses=[sc["pose"]], n_poses=0)
    refused(icp, ERR_INVALID_ARG, poses=[sc["pose"]] * 4097)
    refused(icp, ERR_NO_OUTLIER, "no outlier to filter", n=0)
    from norlab_icp_mapper_amd import _capi
    st = (C.c_int * 3)(*[9, 9, 9])
    assert icp._lib.icpmi_residual_error_poses_dev(icp._h, d.data_ptr(), n, None, _cm(poses).ctypes.data, 3, 0, None, st, None) == ERR_INVALID_ARG   # null out
    icp.setConfig(max_dist=rr.MAX_DIST, minimizer=2, outliers=[])
    refused(icp, ERR_NO_POINT, "no point to minimize", n=0)
    icp.setConfig(max_dist=rr.MAX_DIST, minimizer=2, outliers=[TRIM, (5, 0.5)])
    refused(icp, ERR_MISSING_NORMALS, "SurfaceNormalOutlierFilter")                # no reading normals
    rv, _, status, batched = many(icp, d.data_ptr(), n, poses, nrm.data_ptr())
    assert rv == 0 and status == [0, 0, 0] and batched == 0
    for robust in ((7, 1.0, 0 | (2 << 4), 0.0), (7, 1.0, 0 | (1 << 4), 2.0)):      # scaleEstimator berg; mad with nbIterationForScale 2
        icp.setConfig(max_dist=rr.MAX_DIST, minimizer=2, outliers=[robust])
        refused(icp, ERR_UNSUPPORTED, "RobustOutlierFilter")
    icp.setConfig(max_dist=rr.MAX_DIST, minimizer=0)
    refused(icp, ERR_UNSUPPORTED, "IdentityErrorMinimizer")
    rv, _, status, _ = many(icp, d.data_ptr(), n, poses, kind=1)
    assert rv == 0 and status == [0, 0, 0]
    icp.setConfig(max_dist=rr.MAX_DIST, minimizer=2, outliers=[(6, 0.1, 1 | 2, 0.0)])
    refused(icp, ERR_INVALID_ARG, "icpmi_set_reading_scalar")                      # a missing one-shot row
    icp.setConfig(minimizer=2, var_dist=1)
    refused(icp, ERR_INVALID_ARG, "icpmi_set_reading_max_dist")
    icp.setReadingMaxDist(np.full(n, 0.8, F))
    rv, _, status, batched = many(icp, d.data_ptr(), n, poses)
    assert rv == 0 and status == [0, 0, 0] and batched == 0                        # var-dist: pose after pose on the one row
    with pytest.raises(Exception):
        icp.residuals(reading, np.zeros((0, 4, 4), F))
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 5. multistart
def _priors(sc, S):
    """the scene's prior perturbed by up to 0.05 rad and 0.2 m; the last of three or more is 1000 m away"""
    from norlab_icp_mapper_amd import synth
    rng = np.random.default_rng(91)
    out = []
    for s in range(S):
        rv = rng.uniform(-1, 1, 3); rv *= 0.05 * rng.uniform() / np.linalg.norm(rv)
        t = rng.uniform(-1, 1, 3); t *= 0.2 * rng.uniform() / np.linalg.norm(t)
        out.append((synth.make_T(rv, t) @ sc["T_gt"]).astype(F))
    out[0] = np.asarray(sc["T_gt"], F)
    if S >= 2:
        out[-1] = out[-1].copy(); out[-1][0, 3] += 1000.0
    return out


MS_CHAINS = {"served": dict(CHAINS["p2plane_trimmed"]), "unserved_knn3": dict(CHAINS["p2plane_trimmed"], knn=3)}


@pytest.mark.parametrize("fixed", [0, 7])
@pytest.mark.parametrize("name", list(MS_CHAINS))
def test_multistart_equals_register_prior_alone(amd, mid_scene, name, fixed):
    import torch
    sc = mid_scene
    n = 5000
    d = torch.from_numpy(np.ascontiguousarray(sc["scan"][:n])).cuda()
    icp = amd.ICPSequence(max_iterations=30, use_differential=1, **MS_CHAINS[name])
    # the chain of `fixed` iterations as a handle of its own: Counter alone, what fixed_iterations makes of the loop
    alone = icp if fixed == 0 else amd.ICPSequence(max_iterations=fixed, use_differential=0, **MS_CHAINS[name])
    for h in {id(icp): icp, id(alone): alone}.values():
        assert h.setMap(sc["map"], sc["normals"])
    all_priors = _priors(sc, 16)
    ref = {}
    for S in (1, 2, 16):
        priors = _priors(sc, S)
        Ts, stats, status = icp.registerMultiStartDev(d.data_ptr(), n, priors, fixed_iterations=fixed)
        assert status[0] == 0 and (S < 2 or status[-1] == ERR_NO_OUTLIER)
        # nothing is left staged (asked before the reference calls below stage a scan of their own on this handle)
        assert icp._lib.icpmi_map_update_staged(icp._h, _cm(np.eye(4)).ctypes.data, C.c_float(0.1), 0, None, None, None) == ERR_INVALID_ARG
        assert "no scan staged" in icp._lib.icpmi_last_error(icp._h).decode()
        for s, P in enumerate(priors):
            key = P.tobytes()
            if key not in ref:
                T = (C.c_float * 16)(); st = type(alone.stats)()
                rv = alone._lib.icpmi_register_prior_dev(alone._h, d.data_ptr(), n, _cm(P).ctypes.data, T, C.byref(st))
                ref[key] = (int(rv), np.array(T[:], F).reshape(4, 4).T.copy(), st.iterations, st.stop_reason, st.pairs, np.float32(st.trimmed_limit))
            rv, T, it, why, pairs, lim = ref[key]
            tag = (name, fixed, S, s)
            assert status[s] == rv, tag
            assert np.array_equal(Ts[s].view(np.uint32), T.view(np.uint32)), tag
            assert (stats[s].iterations, stats[s].stop_reason, stats[s].pairs) == (it, why, pairs), tag
            assert np.float32(stats[s].trimmed_limit).view(np.uint32) == lim.view(np.uint32), tag
    with pytest.raises(Exception):
        icp.registerMultiStartDev(d.data_ptr(), n, all_priors + [all_priors[0]])          # 17 starts
    # the host-pointer entry: one upload, the same bits
    priors = _priors(sc, 2)
    a = icp.registerMultiStartDev(d.data_ptr(), n, priors, fixed_iterations=fixed)
    b = icp.registerMultiStart(np.ascontiguousarray(sc["scan"][:n]), priors, fixed_iterations=fixed)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[2] == b[2]
    icp.close()
    if alone is not icp:
        alone.close()


# ------------------------------------------------------------------------------------------------------------------ 6. relocalisation
def _host():
    from test_host_cpp import _build_host
    _build_host()


# The winner against the scene's ground truth.  The clouds carry Gaussian noise of sigma = 0.01 m (synth.make_scene), so the optimum of ~850
# pairs lies within 2 sigma of the truth -- 0.02 m, and 0.02 m over the scene's 10 m half-extent = 0.002 rad -- and the
# DifferentialTransformationChecker (0.001 m / 0.001 rad, smoothed over 3 iterations) stops within three such steps of it.
POSE_TOL_M, POSE_TOL_RAD = 0.02 + 3 * 0.001, 0.002 + 3 * 0.001


def test_relocalize_python_and_host_shell(amd):
    from norlab_icp_mapper_amd import icp as I
    _host()
    sc = rr.scene()
    scan = np.ascontiguousarray(sc["scan"])
    cand = rc.candidates()
    n = scan.shape[0]
    icp = amd.ICPSequence(**rc.CHAIN)
    assert icp.setMap(sc["map"], sc["normals"])
    table = icp.residuals(scan, cand)
    assert table.status == [0] * len(cand)
    order = I.rank_candidates(table, n, 0.5)
    assert order[0] == rc.TRUE_INDEX
    for opts in ({}, dict(refine=1)):                            # the default (refine = 4) first
        got = icp.relocalize(scan, cand, **opts)
        assert got.index == rc.TRUE_INDEX, (opts, got.index)
        assert got.scores.bits() == table.bits()                                  # the score table is residuals()
        Ts, _, status = icp.registerMultiStart(scan, [cand[got.index]])           # that candidate refined alone
        assert status == [0]
        want = I.compose_pose(Ts[0], cand[got.index])
        assert np.array_equal(got.pose.view(np.uint32), want.view(np.uint32)), opts
        again = icp.residuals(scan, [got.pose])
        assert again.residuals[0].bits() == got.residual.bits()
        dt, dr = amd.synth.pose_error(got.pose, sc["T_gt"])
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (opts, dt, dr)
        # the host shell: the same call on a GpuICPSequence of its own
        host = rb.icp_relocalize(rc.CHAIN_YAML, sc["map"], sc["normals"], scan, cand, ratio=0.5, refine=opts.get("refine", 4), ms_index=got.index)
        assert host["index"] == rc.TRUE_INDEX
        assert np.array_equal(host["pose"].view(np.uint32), got.pose.view(np.uint32)), opts
        assert I.Residual(host["residual"]).bits() == got.residual.bits()
        assert [(s, I.Residual(r).bits()) for s, r in zip(host["status"], host["scores"])] == table.bits()
        assert host["batched"] == table.batched
        assert host["ms_status"] == 0 and np.array_equal(host["ms_T"].view(np.uint32), Ts[0].view(np.uint32))
    # no survivor: ConvergenceError on both sides
    far = cand.copy(); far[:, 0, 3] += 1000.0
    with pytest.raises(I.ConvergenceError):
        icp.relocalize(scan, far)
    with pytest.raises(RuntimeError, match="ConvergenceError"):
        rb.icp_relocalize(rc.CHAIN_YAML, sc["map"], sc["normals"], scan, far)
    icp.close()


def test_chains_that_read_the_reading_are_refused_up_front(amd):
    """the multistart registration carries the points alone: relocalize and registerMultiStart say so instead of failing start by start"""
    from norlab_icp_mapper_amd import icp as I
    _host()
    sc = rr.scene()
    scan = np.ascontiguousarray(sc["scan"])
    cand = rc.candidates()[:3]
    for outs, extra in (([(4, 0.85), (5, 0.5)], {}), ([(6, 0.1, 1 | 2, 0.0)], {}), ([(4, 0.85)], dict(var_dist=1))):
        icp = amd.ICPSequence(minimizer=2, max_dist=2.0, outliers=outs, **extra)
        assert icp.setMap(sc["map"], sc["normals"])
        with pytest.raises(I.InvalidParameter, match="does not carry"):
            icp.relocalize(scan, cand)
        with pytest.raises(I.InvalidParameter, match="does not carry"):
            icp.registerMultiStart(scan, cand)
        icp.close()
    yaml = rc.CHAIN_YAML.replace("outlierFilters:\n", "outlierFilters:\n  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.5\n")
    assert "SurfaceNormalOutlierFilter" in yaml
    with pytest.raises(RuntimeError, match="InvalidParameter.*does not carry"):
        rb.icp_relocalize(yaml, sc["map"], sc["normals"], scan, cand)


MAPPER_YAML = """
input:
  - BoundingBoxDataPointsFilter:
      xMin: -0.1
      xMax: 0.1
      yMin: -0.1
      yMax: 0.1
      zMin: -0.1
      zMax: 0.1
      removeInside: 1
mapper:
  updateCondition:
    type: delay
    value: 0.05
  sensorMaxRange: 200
icp:%s
""" % rc.CHAIN_YAML.replace("\n", "\n  ").rstrip()


def test_mapper_relocalize_sets_the_pose_and_leaves_the_map(amd, tmp_path):
    _host()
    sc = rr.scene()
    scan = np.ascontiguousarray(sc["scan"])
    cand = rc.candidates()
    cfg = os.path.join(str(tmp_path), "config.yaml")
    open(cfg, "w").write(MAPPER_YAML)
    got = rb.mapper_relocalize(cfg, sc["map"], sc["normals"], scan, cand)
    assert got["map_before"] == got["map_after"] == sc["map"].shape[0]            # the map is not updated
    assert np.array_equal(got["pose"].view(np.uint32), got["get_pose"].view(np.uint32))   # the next processInput starts here
    icp = amd.ICPSequence(**rc.CHAIN)
    assert icp.setMap(sc["map"], sc["normals"])
    want = icp.relocalize(scan, cand)                                             # (the input filter drops nothing of this scan)
    assert got["index"] == want.index == rc.TRUE_INDEX
    assert np.array_equal(got["pose"].view(np.uint32), want.pose.view(np.uint32))
    icp.close()
