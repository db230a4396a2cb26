"""getResidualError on the device (icpmi_residual_error*, csrc/loop.hip: loop_residual, res_pairs_kernel / res_finish_kernel).

1. against the stage entries, an independent path through the library: the reading centred and moved by hand, the pair set and d2 from
   icpmi_knn, the weights from icpmi_outlier_weights, the float32 restatement of tests/residual_reference.py over them: pairs, max_abs and
   the trimmed limit bit-equal, the double sums within pairs * 2^-52 relative (the bound of re-ordering a double sum of non-negative
   terms); kinds 1 and 2, k = 1 and 6, n in residual_reference.NS, seven chains;
2. against float64: the same pair set through the float64 restatement, within four times profiles/residual_tolerance.json; point-to-point
   with MaxDist also against exact float64 neighbours, no library call in the reference at all;
3. against a registration: pairs and weighted ratio equal icpmi_minimize_step's at the same pose; SurfaceNormalOutlierFilter's pair count
   equals icpmi_outlier_weights' with the rotated reading normals;
4. behaviour: same bits twice, from host and device pointers, staged; NULL = identity; a registration, its stats and its covariance are
   untouched by an evaluation in between;
5. every error; 6. the host shell: GpuICPSequence::residual, Mapper::setScoreRegistrations on the one-upload and the host path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import covariance_reference as cr
import residual_reference as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MAXD = (1, 0.6)          # MaxDistOutlierFilter, inside the matcher's 0.8
TRIM = (4, 0.85)         # TrimmedDistOutlierFilter
MED = (3, 1.5)           # MedianDistOutlierFilter
GEN_SOFT = (6, 0.1, 2, 0.0)   # GenericDescriptorOutlierFilter{source: reference, useSoftThreshold: 1}: the weight is the map's scalar
CHAINS = {   # name: (outlier filters, config, planar scene, the residual drops the z term)
    "maxdist": ([MAXD], {}, False, False),
    "trimmed": ([TRIM], {}, False, False),
    "median": ([MED], {}, False, False),
    "maxdist+trimmed": ([MAXD, TRIM], {}, False, False),
    "generic_soft": ([GEN_SOFT], {}, False, False),
    "force_2d": ([MAXD], {"force_2d": 1}, False, True),
    "planar": ([TRIM], {"is_2d": 1}, True, True),
}


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _scene(planar):
    return rr.planar_scene() if planar else rr.scene()


def _map_scalar():
    """the soft weights: 0 (out), 0.3, 1 and values in between, by map index"""
    s = (np.arange(rr.M) % 7).astype(F) / F(6)
    s[np.arange(rr.M) % 7 == 1] = F(0.3)
    return s


def _make(amd, k, outs, extra, sc):
    icp = amd.ICPSequence(knn=k, max_dist=sc["max_dist"], outliers=outs, **extra)
    assert icp.setMap(sc["map"], sc["normals"])
    if any(o[0] == 6 for o in outs):
        icp.setMapScalar(_map_scalar())
    return icp


def _moved(icp, sc, reading, T):
    """the queries as the matcher forms them: (reading - mean) under the centred pose, xf_point's arithmetic"""
    mean = icp.getMapMean()
    Tc = rr.centred_pose(T, mean)
    rc = rr.centre_reading(reading, mean)
    moved = np.ones((reading.shape[0], 4), F)
    moved[:, :3] = cr.fma_transform(Tc, rc)
    return moved, rc, Tc


_cases = {}


def cases(amd, chain, k):
    """per n and kind: the device's answer and both restatements over the stage entries' pair set (computed once, shared by tests 1 and 2)"""
    if (chain, k) in _cases:
        return _cases[chain, k]
    outs, extra, planar_sc, planar = CHAINS[chain]
    sc = _scene(planar_sc)
    icp = _make(amd, k, outs, extra, sc)
    mapc = rr.centred_map(sc["map"], icp.getMapMean())
    T = sc["pose"]
    out = []
    for n in rr.NS:
        reading = sc["scan"][:n].copy()
        moved, _, _ = _moved(icp, sc, reading, T)
        ids, d2 = icp.knn(moved, k=k, max_dist=sc["max_dist"])
        w, lim = icp.outlierWeights(d2, ids=ids)                  # (the stage entries serve every chain of CHAINS)
        filled = ids >= 0
        assert np.array_equal(filled, np.isfinite(d2))
        qi, qj = np.nonzero(filled)
        s = ids[qi, qj]
        for kind in (1, 2):
            res = icp.residual(reading, T, kind=kind)
            pl = planar and kind == 2
            r32 = rr.residuals_f32(kind, moved[qi, :3], mapc[s], sc["normals"][s], d2[qi, qj], pl)
            r64 = rr.residuals_f64(kind, reading[qi], T, sc["map"][s], sc["normals"][s], pl)
            out.append(dict(n=n, kind=kind, res=res, lim=lim, want=rr.summarise(r32, w[qi, qj]), want64=rr.summarise(r64, w[qi, qj]),
                            unfilled=int((~filled).sum()), empty=int((~filled).all(1).sum()), soft=int(((w > 0) & (w < 1)).sum())))
    icp.close()
    _cases[chain, k] = out
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. stage entries
@pytest.mark.parametrize("k", rr.KS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_against_the_stage_entries(amd, chain, k):
    for c in cases(amd, chain, k):
        res, want, tag = c["res"], c["want"], (chain, k, c["n"], c["kind"])
        print(tag, res, want)
        assert res.kind == c["kind"]
        assert res.pairs == want["pairs"] > 0, tag
        assert _bits(res.max_abs) == _bits(want["max_abs"]), tag
        tol = want["pairs"] * 2.0 ** -52
        assert abs(res.weight_sum - want["weight_sum"]) <= tol * want["weight_sum"], tag
        assert abs(res.sum_abs - want["sum_abs"]) <= tol * want["sum_abs"], tag
        assert abs(res.sum_sq - want["sum_sq"]) <= tol * want["sum_sq"], tag
        assert _bits(res.weighted_point_used_ratio) == _bits(F(res.weight_sum / (k * c["n"]))), tag
        if any(o[0] in (3, 4) for o in CHAINS[chain][0]):
            assert _bits(res.trimmed_limit) == _bits(F(c["lim"])), tag
        else:
            assert res.trimmed_limit == -1
    big = [c for c in cases(amd, chain, k) if c["n"] == 1000][0]
    assert big["unfilled"] > 0 and (k == 1 or big["unfilled"] > big["empty"] * k)      # maxDist leaves slots (k = 6: partial rows) empty
    assert big["empty"] > 0
    if chain == "generic_soft":
        assert big["soft"] > 100                                                       # soft weights counted as pairs


# ------------------------------------------------------------------------------------------------------------------ 2. float64
@pytest.mark.parametrize("k", rr.KS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_against_float64(amd, chain, k):
    for c in cases(amd, chain, k):
        res, want = c["res"], c["want64"]
        name = {("planar", 1): "1_planar", ("planar", 2): "2_planar", ("force_2d", 2): "2_force2d"}.get((chain, c["kind"]), str(c["kind"]))
        tol = rr.device_bound(name)
        dev = rr.rel_dev({"sum_abs": res.sum_abs, "sum_sq": res.sum_sq}, want)
        print(chain, k, c["n"], c["kind"], dev, tol)
        assert res.pairs == want["pairs"]
        assert dev <= tol, (chain, k, c["n"], c["kind"], dev, tol)


def test_point_to_point_against_exact_neighbours(amd):
    """no library call in the reference: exact float64 neighbours within the MaxDist filter's radius, float64 distances (n = 257;
    tests/test_residual_cpu.py shows the seed has no near-tie that could move the sum by the tolerance)"""
    sc = rr.scene()
    reading = sc["scan"][:257].copy()
    T = sc["pose"].astype(np.float64)
    moved = reading[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    _, d2, _ = rr.brute_knn(moved, sc["map"][:, :3], 1, MAXD[1])
    want = np.sqrt(d2[np.isfinite(d2)])
    icp = _make(amd, 1, [MAXD], {}, sc)
    res = icp.residual(reading, sc["pose"], kind=1)
    icp.close()
    assert res.pairs == want.shape[0]
    assert abs(res.sum_abs - want.sum()) <= rr.device_bound("1") * want.sum()
    assert abs(res.sum_sq - (want ** 2).sum()) <= rr.device_bound("1") * (want ** 2).sum()


# ------------------------------------------------------------------------------------------------------------------ 3. a registration
@pytest.mark.parametrize("k", rr.KS)
@pytest.mark.parametrize("chain", ["maxdist", "trimmed", "median", "maxdist+trimmed", "generic_soft"])
def test_against_a_registration(amd, chain, k):
    outs, extra, _, _ = CHAINS[chain]
    sc = rr.scene()
    reading = sc["scan"].copy()
    icp = _make(amd, k, outs, dict(extra, use_differential=1), sc)
    T = icp(reading)
    res = icp.residual(reading, T)
    assert res.kind == 2                                       # ICPMI_RES_CHAIN on the default point-to-plane chain
    assert res.sum_abs == icp.errorMinimizer.getResidualError(reading, T)
    _, rc, Tc = _moved(icp, sc, reading, T)
    icp.minimizeStep(rc, T_iter=Tc)
    assert res.pairs == icp.stats.pairs > 0
    assert _bits(res.weighted_point_used_ratio) == _bits(icp.stats.weighted_point_used_ratio)
    assert _bits(res.trimmed_limit) == _bits(icp.stats.trimmed_limit)
    # the pose the registration ended on fits better than the prior it started from
    start = icp.residual(reading, None)
    assert res.sum_abs / res.pairs < start.sum_abs / start.pairs
    icp.close()


@pytest.mark.parametrize("k", rr.KS)
def test_surface_normal_filter(amd, k):
    sc = rr.scene()
    reading, rn = sc["scan"].copy(), sc["scan_normals"].copy()
    icp = _make(amd, k, [(5, 0.5), MAXD], {}, sc)               # SurfaceNormalOutlierFilter{maxAngle: 0.5}, then MaxDist
    T = sc["pose"]
    moved, _, Tc = _moved(icp, sc, reading, T)
    rot = cr.fma_transform(Tc, np.concatenate([rn, np.zeros((rn.shape[0], 1), F)], 1))      # the loop rotates them by T
    ids, d2 = icp.knn(moved, k=k, max_dist=rr.MAX_DIST)
    w, _ = icp.outlierWeights(d2, ids=ids, read_normals=rot)
    count = int(((w != 0) & (ids >= 0)).sum())
    res = icp.residual(reading, T, normals=rn, kind=2)
    assert res.pairs == count and 0 < count < int((ids >= 0).sum())
    with pytest.raises(amd.icp.InvalidField):
        icp.residual(reading, T, kind=2)                                                    # no reading normals
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 4. behaviour
def test_same_bits_from_every_entry(amd):
    import torch
    sc = rr.scene()
    reading = sc["scan"][:257].copy()
    for k, outs in ((1, [TRIM]), (6, [MAXD, TRIM])):
        icp = _make(amd, k, outs, {}, sc)
        a = icp.residual(reading, sc["pose"], kind=2)
        b = icp.residual(reading, sc["pose"], kind=2)
        assert a.bits() == b.bits()
        d = torch.from_numpy(reading).cuda()
        assert icp.residualDev(d.data_ptr(), reading.shape[0], sc["pose"], kind=2).bits() == a.bits()
        assert icp.residual(reading, None, kind=1).bits() == icp.residual(reading, np.eye(4, dtype=F), kind=1).bits()
        # the scan registerWithPrior leaves in HBM is the scan moved by the prior
        prior = np.asarray(sc["T_gt"], F)
        T = icp.registerWithPrior(reading, prior)
        staged = icp.residualStaged(T, kind=2)
        in_map = icp.transform(prior, reading)
        dm = torch.from_numpy(in_map).cuda()
        assert staged.bits() == icp.residualDev(dm.data_ptr(), reading.shape[0], T, kind=2).bits()
        assert staged.bits() == icp.residualStaged(T, kind=2).bits()
        icp.close()


@pytest.mark.parametrize("k", rr.KS)
def test_a_registration_is_untouched(amd, k):
    sc = rr.scene()
    reading = sc["scan"].copy()
    runs = []
    for evaluate in (False, True):
        icp = _make(amd, k, [TRIM], dict(covariance=1, use_differential=1), sc)
        out = []
        for _ in range(2):
            T = icp(reading)
            s = icp.stats
            out += [_bits(T), s.iterations, s.stop_reason, s.pairs, _bits(s.weighted_point_used_ratio), _bits(s.trimmed_limit)]
            if evaluate:
                icp.residual(reading, T)
                icp.residual(reading[:65], None, kind=1)
            out.append(_bits(icp.errorMinimizer.getCovariance()))
        if evaluate:
            with pytest.raises(NotImplementedError):
                icp.lastMatches(reading.shape[0])              # the matcher's buffers were reused
            icp.knn(reading[:10].copy(), k=1)
            with pytest.raises(NotImplementedError):
                icp.errorMinimizer.getCovariance()             # ... and after any other call the covariance is gone, as before
        icp.close()
        runs.append(out)
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ 5. errors
def test_errors(amd):
    I = amd.icp
    sc = rr.scene()
    reading = sc["scan"][:257].copy()
    icp = amd.ICPSequence(max_dist=rr.MAX_DIST)
    with pytest.raises(I.InvalidParameter, match="no map"):
        icp.residual(reading)
    with pytest.raises(I.InvalidParameter, match="no scan staged"):
        icp.residualStaged()
    assert icp.setMap(sc["map"])                                # no normals
    with pytest.raises(I.InvalidField):
        icp.residual(reading, kind=2)
    with pytest.raises(I.InvalidField):
        icp.residual(reading)                                   # ICPMI_RES_CHAIN: the point-to-plane chain's kind
    assert icp.residual(reading, sc["pose"], kind=1).pairs > 0
    assert icp.setMap(sc["map"], sc["normals"])
    with pytest.raises(I.InvalidParameter, match="no scan staged"):
        icp.residualStaged()
    bad = np.eye(4, dtype=F); bad[0, 0] = 1.01
    with pytest.raises(I.TransformationError):
        icp.residual(reading, bad)
    with pytest.raises(I.ConvergenceError):
        icp.residual(reading[:0])                               # n = 0
    with pytest.raises(I.InvalidParameter):
        icp.residual(reading, kind=3)
    icp.setConfig(max_dist=1e-6)
    with pytest.raises(I.ConvergenceError, match="no point to minimize"):
        icp.residual(reading, sc["pose"])                       # P == 0
    icp.setConfig(max_dist=rr.MAX_DIST, minimizer=0)
    with pytest.raises(NotImplementedError):
        icp.residual(reading)                                   # IdentityErrorMinimizer has no residual
    assert icp.residual(reading, kind=1).kind == 1 and icp.residual(reading, kind=2).kind == 2
    for robust in ((7, 1.0, 0 | (2 << 4), 0.0), (7, 1.0, 0 | (1 << 4), 2.0)):       # scaleEstimator berg; mad with nbIterationForScale 2
        icp.setConfig(max_dist=rr.MAX_DIST, outliers=[robust])
        with pytest.raises(NotImplementedError, match="RobustOutlierFilter"):
            icp.residual(reading)
    icp.setConfig(max_dist=rr.MAX_DIST, outliers=[(7, 1.0, 0 | (1 << 4), 0.0)])     # cauchy / mad, every iteration: served
    assert icp.residual(reading, sc["pose"]).pairs > 0
    icp.close()


# ------------------------------------------------------------------------------------------------------------------ 6. host shell
def _host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb.load()


P2PLANE_YAML = ("matcher:\n  KDTreeMatcher:\n    knn: %d\n    maxDist: 0.8\n    epsilon: 0\noutlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n"
                "errorMinimizer:\n  PointToPlaneErrorMinimizer:\ntransformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 10\n")


def _hook(lib, yaml, mp, nm, scan, T=None, kind=0):
    from norlab_icp_mapper_amd import _capi
    fn = lib.nim_test_icp_residual
    fn.restype = C.c_int
    res = _capi.Residual(); T_out = np.zeros(16, F); val = C.c_float(0); err = C.create_string_buffer(512)
    Tc = None if T is None else np.ascontiguousarray(np.asarray(T, F).T).ravel()
    rc = fn(yaml.encode(), C.c_void_p(mp.ctypes.data), C.c_int64(mp.shape[0]), C.c_void_p(None if nm is None else nm.ctypes.data),
            C.c_void_p(scan.ctypes.data), C.c_int64(scan.shape[0]), None, C.c_void_p(None if Tc is None else Tc.ctypes.data), C.c_int(kind),
            C.byref(res), C.c_void_p(T_out.ctypes.data), C.byref(val), err, C.c_int(512))
    return rc, res, T_out.reshape(4, 4).T.copy(), val.value, err.value.decode(errors="replace")


@pytest.mark.parametrize("k", rr.KS)
def test_host_sequence_residual(amd, k):
    """GpuICPSequence::residual / errorMinimizer->getResidualError equal the C ABI's answer; the exception types of operator()"""
    lib = _host()
    sc = rr.scene()
    mp, nm, scan = sc["map"], sc["normals"], sc["scan"].copy()
    rc, res, T, val, err = _hook(lib, P2PLANE_YAML % k, mp, nm, scan)
    assert rc == 0, err
    icp = _make(amd, k, [TRIM], dict(max_iterations=10), sc)
    assert amd.icp.Residual(res).bits() == icp.residual(scan, T).bits()
    assert res.kind == 2 and val == F(res.sum_abs)
    icp.close()
    rc, _, _, _, err = _hook(lib, (P2PLANE_YAML % k).replace("maxDist: 0.8", "maxDist: 0.000001"), mp, nm, scan, T=np.eye(4))
    assert rc == 2 and "ConvergenceError" in err                               # (the Trimmed filter finds nothing to filter)
    rc, _, _, _, err = _hook(lib, P2PLANE_YAML % k, mp, None, scan, T=np.eye(4))
    assert rc == 3 and "normals" in err                                        # InvalidField
    bad = np.eye(4); bad[1, 1] = 1.01
    rc, _, _, _, err = _hook(lib, P2PLANE_YAML % k, mp, nm, scan, T=bad)
    assert rc == 4                                                             # InvalidParameter


N_SCANS = 4


@pytest.fixture(scope="module")
def scored_replays(tmp_path_factory):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    _host()
    tmp = str(tmp_path_factory.mktemp("residual_replay"))
    z = np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))
    sub = {"scan_names": z["scan_names"][:N_SCANS], "trajectory": z["trajectory"][:N_SCANS]}
    for k in range(N_SCANS):
        sub[f"scan{k}_xyz"] = z[f"scan{k}_xyz"]
    names, traj = write_bundled_dataset(tmp, sub)
    open(os.path.join(tmp, "names.txt"), "w").write("\n".join(names) + "\n")
    np.save(os.path.join(tmp, "trajectory.npy"), np.asarray(traj, dtype=np.float64))
    cfg = os.path.join(tmp, "config.yaml")
    assert "PointToPlaneErrorMinimizer:" in CONFIG4_YAML and "samplingMethod: 0" in CONFIG4_YAML
    open(cfg, "w").write(CONFIG4_YAML.replace("samplingMethod: 0", "samplingMethod: 1"))       # the reproducible hash on both paths
    out = {}
    for mode in ("1", "0"):
        dst = os.path.join(tmp, f"replay_{mode}.npz")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "residual_replay.py"), tmp, cfg, str(N_SCANS), dst],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, NIM_RESIDENT_MAP_UPDATE=mode))
        assert p.returncode == 0, p.stderr[-2000:] + p.stdout[-500:]
        out[mode] = dict(np.load(dst))
    return out


@pytest.mark.parametrize("mode", ["1", "0"])
def test_mapper_scores_registrations(scored_replays, mode):
    """NIM_RESIDENT_MAP_UPDATE=1: the one-upload path (icpmi_residual_error_staged); 0: the host path (GpuICPSequence::residual)"""
    r = scored_replays[mode]
    assert np.array_equal(_bits(r["on_poses"]), _bits(r["off_poses"]))         # scoring changes no pose
    assert r["on_valid"].tolist() == [0, 1, 1, 1] and r["frozen_valid"].tolist() == [0, 1, 1, 1]
    assert not r["off_valid"].any()
    assert np.array_equal(r["frozen_res"][1:], r["frozen_hand"][1:])            # lastResidual() == residual() by hand
    from norlab_icp_mapper_amd import _capi
    for raw in list(r["on_res"][1:]) + list(r["frozen_res"][1:]):
        res = _capi.Residual.from_buffer_copy(raw.tobytes())
        assert res.kind == 2 and res.pairs > 1000 and 0 < res.sum_abs < res.pairs * 2.0 and res.max_abs <= 2.0


def test_mapper_paths_give_the_same_residual(scored_replays):
    a, b = scored_replays["1"], scored_replays["0"]
    assert np.array_equal(_bits(a["frozen_poses"]), _bits(b["frozen_poses"]))
    assert np.array_equal(a["frozen_res"], b["frozen_res"])
