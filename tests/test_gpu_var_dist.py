"""KDTreeVarDistMatcher on the device: every reading point is matched within its own radius (icpmi_set_reading_max_dist /
icpmi_knn_var, icpmi_config::var_dist).  The search prunes with one bound, the largest radius of the row; only the accept test where
a matcher kernel writes its result is per query -- so the tests go through every kernel that writes one: nn1_wg_kernel (k = 1),
nnk_ml_kernel and nnk_wg_kernel (k = 6, 16), the one-lane kernel (k = 20) and, with +inf in the row, the brute passes behind them.

Inputs (tests/var_dist_reference.py; tests/test_var_dist_cpu.py checks the generator without a GPU): a 4 096-point map and a 1 024-point
reading from synth; the reference is the oracle's exact unbounded kNN masked per query in numpy; the row is built from each query's own
exact neighbour distances and keeps 1e-5 (relative) clear of them, asserted wherever a comparison relies on it, so that the tie rule
`d2 <= r^2` decides no case of tests 1 and 3; test 2 pins the tie rule (a constant row is maxDist, bit for bit)."""
import ctypes as C
import math

import numpy as np
import pytest

import var_dist_reference as vr
from loop_driver import centring

pytestmark = pytest.mark.gpu

RATIO = 0.85
INF = math.inf


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ref(amd, oracle):
    """the scene, centred as the handle centres it, the exact rows of the reading as handed in, and the mixed radii row; computed once"""
    sc = vr.scene()
    icp = amd.ICPSequence(minimizer=0)
    assert icp.setMap(sc["map"])
    mean = icp.getMapMean()
    o = oracle.OracleICP(oracle.make_config()); o.setMap(sc["map"])
    assert np.array_equal(mean, o.getMapMean())
    mapc, q = vr.centred(sc["map"], mean), vr.centred(sc["scan"], mean)
    ids, d2 = vr.exact_rows(oracle, mapc, q)
    r, kind = vr.radii_row(d2)
    assert vr.clear_of(r, d2).all()          # the condition on the inputs
    for a in (mapc, q, ids, d2, r, kind):
        a.setflags(write=False)
    return dict(sc=sc, mean=mean, mapc=mapc, q=q, ids=ids, d2=d2, r=r, kind=kind, stage=icp)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", vr.KS)
def test_knn_var_equals_the_masked_exact_knn(ref, k):
    ids, d2 = ref["stage"].knnVar(ref["q"], ref["r"], k=k)
    rids, rd2 = vr.masked(ref["ids"], ref["d2"], ref["r"], k)
    assert same_bits(d2, rd2), np.nonzero((bits(d2) != bits(rd2)).any(1))[0][:8]
    assert np.array_equal(ids, rids), np.nonzero((ids != rids).any(1))[0][:8]
    assert np.array_equal((ids >= 0).sum(1), vr.expected_filled(ref["kind"], k))


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("k", vr.KS)
@pytest.mark.parametrize("r", [0.05, 0.5, INF])
def test_constant_row_is_max_dist(ref, k, r):
    ids, d2 = ref["stage"].knnVar(ref["q"], np.full(vr.N, r, np.float32), k=k)
    uids, ud2 = ref["stage"].knn(ref["q"], k=k, max_dist=r)
    assert same_bits(d2, ud2) and np.array_equal(ids, uids)


CHAINS = {
    "k1_p2p_trimmed": dict(minimizer=1, knn=1, outliers=[(4, RATIO)], max_iterations=40, use_differential=1),
    "k6_p2plane_trimmed_surfacenormal": dict(minimizer=2, knn=6, outliers=[(4, RATIO), (5, 1.2)], max_iterations=40, use_differential=1),
}


def outcome(amd, sc, kw, row=None, n=None, with_normals=True):
    """one registration on a fresh handle: ("ok", pose bits, stats) or ("error", exception type name)"""
    n = sc["scan"].shape[0] if n is None else n
    try:
        icp = amd.ICPSequence(**kw)
        assert icp.setMap(sc["map"], sc["normals"])
        if row is not None:
            icp.setReadingMaxDist(row)
        T = icp(sc["scan"][:n], sc["scan_normals"][:n] if with_normals else None)
    except (amd.icp.InvalidParameter, amd.icp.InvalidField, amd.icp.ConvergenceError) as e:
        return ("error", type(e).__name__)
    s = icp.stats
    return ("ok", bits(T).tolist(), int(s.iterations), int(s.stop_reason), int(s.pairs), bits(np.float32(s.point_used_ratio)).item(),
            bits(np.float32(s.weighted_point_used_ratio)).item(), bits(np.float32(s.trimmed_limit)).item())


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_registration_with_a_constant_row_is_the_max_dist_registration(amd, ref, chain, use_graph):
    sc = ref["sc"]
    ran = 0
    for r in (0.05, 0.5, INF):
        kw = dict(CHAINS[chain], use_graph=use_graph)
        uni = outcome(amd, sc, dict(kw, max_dist=r))
        var = outcome(amd, sc, dict(kw, var_dist=1), row=np.full(vr.N, r, np.float32))
        assert var == uni, (chain, r, var, uni)
        ran += uni[0] == "ok"
    assert ran >= 2, "the comparison must cover registrations that run"


# ------------------------------------------------------------------------------------------------------------------ 3
def loop_row(ref):
    """the mixed row with the last quarter of the reading at 0.3 m: radii that bite while the reading moves"""
    r = ref["r"].copy()
    r[3 * vr.N // 4:] = np.float32(0.3)
    return r


def loop_registration(amd, ref, k, wg_from, through_descriptors=False):
    sc = ref["sc"]
    icp = amd.ICPSequence(minimizer=1 if k == 1 else 2, knn=k, var_dist=1, outliers=[(4, RATIO)], max_iterations=40, use_differential=1,
                          knn_wg_from=wg_from)
    assert icp.setMap(sc["map"], sc["normals"])
    r = loop_row(ref)
    if through_descriptors:
        T = icp(sc["scan"], descriptors={"maxSearchDist": r[None, :], "intensity": np.zeros(vr.N, np.float32)})
    else:
        icp.setReadingMaxDist(r)
        T = icp(sc["scan"])
    ids, d2, T_used = icp.lastMatches()
    return icp, r, T, ids, d2, T_used


@pytest.mark.parametrize("k,wg_from", [(1, 0), (6, -1), (6, 0)])
def test_loop_matches_are_the_masked_exact_knn(amd, oracle, ref, k, wg_from):
    """k = 1: nn1_wg_kernel, seeded from iteration 1 on; k = 6: nnk_ml_kernel everywhere (knn_wg_from = -1), or nnk_ml_kernel for two
    iterations and nnk_wg_kernel after (default)"""
    icp, r, T, ids, d2, T_used = loop_registration(amd, ref, k, wg_from, through_descriptors=(k == 6 and wg_from == 0))
    assert icp.stats.iterations >= 3, icp.stats.iterations   # the seeded steady launches ran
    q = oracle.transform(T_used, oracle.transform(centring(ref["mean"]), ref["sc"]["scan"]))
    eids, ed2 = vr.exact_rows(oracle, ref["mapc"], q)
    assert vr.clear_of(r, ed2).all(), np.nonzero(~vr.clear_of(r, ed2))[0][:8]   # the condition, at the pose the last iteration searched from
    rids, rd2 = vr.masked(eids, ed2, r, k)
    assert same_bits(d2, rd2), np.nonzero((bits(d2) != bits(rd2)).any(1))[0][:8]
    assert np.array_equal(ids, rids), np.nonzero((ids != rids).any(1))[0][:8]
    filled = (ids >= 0).sum(1)
    assert (filled[: 3 * vr.N // 4][ref["kind"][: 3 * vr.N // 4] == 0] == 0).all() and 0 < filled[3 * vr.N // 4:].sum() < k * (vr.N // 4)
    # pairs: the filled slots whose weight is not zero (TrimmedDist over exactly these d2)
    lim = oracle.dists_quantile(d2, RATIO)
    assert float(icp.stats.trimmed_limit) == lim
    assert int(icp.stats.pairs) == int((np.isfinite(d2) & (d2 <= np.float32(lim))).sum())


# ------------------------------------------------------------------------------------------------------------------ 4
def small_scene(ref, m, n):
    sc = ref["sc"]
    return dict(map=sc["map"][:m], normals=sc["normals"][:m], scan=sc["scan"][:n], scan_normals=sc["scan_normals"][:n])


EDGE_KW = dict(minimizer=1, knn=6, outliers=[(4, RATIO)], max_iterations=10)


@pytest.mark.parametrize("m,n", [(vr.M, 1), (vr.M, 63), (vr.M, 64), (vr.M, 65), (1, 65), (7, 65)])
def test_edge_rows(amd, oracle, ref, m, n):
    sc = small_scene(ref, m, n)
    k = EDGE_KW["knn"]
    stage = amd.ICPSequence(minimizer=0)
    assert stage.setMap(sc["map"])
    q = vr.centred(sc["scan"], stage.getMapMean())
    # all +inf: the unbounded matcher, bit for bit -- as a stage call and as a registration
    ids, d2 = stage.knnVar(q, np.full(n, INF, np.float32), k=k)
    uids, ud2 = stage.knn(q, k=k, max_dist=INF)
    assert same_bits(d2, ud2) and np.array_equal(ids, uids)
    assert ((ids >= 0).sum(1) == min(k, m)).all()
    assert outcome(amd, sc, dict(EDGE_KW, var_dist=1), row=np.full(n, INF, np.float32), with_normals=False) == \
        outcome(amd, sc, dict(EDGE_KW, max_dist=INF), with_normals=False)
    # all 0: every slot unfilled; the registration ends as KDTreeMatcher{maxDist: 0} does
    ids, d2 = stage.knnVar(q, np.zeros(n, np.float32), k=k)
    assert (ids == -1).all() and np.isposinf(d2).all()
    zero = outcome(amd, sc, dict(EDGE_KW, var_dist=1), row=np.zeros(n, np.float32), with_normals=False)
    assert zero == outcome(amd, sc, dict(EDGE_KW, max_dist=0.0), with_normals=False) and zero[0] == "error", zero
    # a mixed row at this size against the masked exact kNN
    mapc = vr.centred(sc["map"], stage.getMapMean())
    eids, ed2 = oracle.knn(mapc, q, k=k, max_dist=INF, nthreads=4)
    r = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.sqrt(ed2[:, 0].astype(np.float64)) * 1.5).astype(np.float32)
    ok = vr.clear_of(r, ed2)
    ids, d2 = stage.knnVar(q, r, k=k)
    rids, rd2 = vr.masked(eids, ed2, r, k)
    assert same_bits(d2[ok], rd2[ok]) and np.array_equal(ids[ok], rids[ok])


def test_row_contract(amd, ref):
    sc = ref["sc"]
    icp = amd.ICPSequence(**dict(CHAINS["k1_p2p_trimmed"], var_dist=1))
    assert icp.setMap(sc["map"], sc["normals"])
    good = np.full(vr.N, 0.5, np.float32)
    for poison in (np.nan, -1.0, -INF):
        bad = good.copy(); bad[vr.N // 2] = poison
        with pytest.raises(amd.icp.InvalidParameter):
            icp.setReadingMaxDist(bad)
        with pytest.raises(amd.icp.InvalidParameter):
            icp.knnVar(ref["q"], bad, k=1)
        with pytest.raises(amd.icp.InvalidField):   # ... and a rejected row arms nothing
            icp(sc["scan"])
    lib = icp._lib   # radii == NULL
    ids = np.empty(vr.N, np.int32); d2 = np.empty(vr.N, np.float32)
    assert lib.icpmi_knn_var(icp._h, ref["q"].ctypes.data, vr.N, 1, None, 1, ids.ctypes.data, d2.ctypes.data) == amd._capi.ERR_INVALID_ARG
    with pytest.raises(amd.icp.InvalidField):       # no row at all
        icp(sc["scan"])
    icp.setReadingMaxDist(good[:-1])                # a row of another size
    with pytest.raises(amd.icp.InvalidField):
        icp(sc["scan"])
    icp.setReadingMaxDist(good)                     # one shot: the second registration finds no row
    T = icp(sc["scan"])
    assert np.isfinite(T).all() and icp.stats.pairs > 0
    with pytest.raises(amd.icp.InvalidField):
        icp(sc["scan"])
    icp.setReadingMaxDist(good)                     # NULL clears an armed row
    icp.setReadingMaxDist(None)
    with pytest.raises(amd.icp.InvalidField):
        icp(sc["scan"])
    with pytest.raises(amd.icp.InvalidField):       # the Python mirror: the named descriptor is missing / has more than one row
        icp(sc["scan"], descriptors={"intensity": good})
    with pytest.raises(amd.icp.InvalidField):
        icp(sc["scan"], descriptors={"maxSearchDist": np.zeros((2, vr.N), np.float32)})
    with pytest.raises(NotImplementedError):        # the stage call that runs the handle's matcher carries no radii
        icp.minimizeStep(ref["q"])


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("k", [1, 6])
def test_loop_registration_is_reproducible(amd, ref, k):
    a = loop_registration(amd, ref, k, 0)
    b = loop_registration(amd, ref, k, 0)
    assert same_bits(a[2], b[2]) and np.array_equal(a[3], b[3]) and same_bits(a[4], b[4]) and same_bits(a[5], b[5])
    assert (a[0].stats.iterations, a[0].stats.pairs) == (b[0].stats.iterations, b[0].stats.pairs)
    # the same handle again, the row handed over again (the cached loop graphs / segments read the new row)
    icp = a[0]
    icp.setReadingMaxDist(a[1])
    T = icp(ref["sc"]["scan"])
    assert same_bits(T, a[2])


def test_var_dist_zero_is_neutral(amd, oracle, ref):
    """var_dist = 0 is the zeroed tail of a caller compiled before the field existed: the default chain, its bits, the oracle's pose"""
    sc = ref["sc"]
    old = amd.icp.default_config()
    C.memset(C.byref(old, amd._capi.Config.reserved.offset), 0, 8)   # what such a caller hands over
    new = amd.icp.default_config(var_dist=0)
    res = []
    for cfg in (old, new):
        icp = amd.ICPSequence(cfg)
        assert icp.setMap(sc["map"], sc["normals"])
        T = icp(sc["scan"])
        res.append((bits(T).tolist(), int(icp.stats.iterations), int(icp.stats.pairs)))
    assert res[0] == res[1]
    oicp = oracle.OracleICP(oracle.make_config(nthreads=4)); oicp.setMap(sc["map"], sc["normals"])
    err, T_ref = oicp(sc["scan"])
    assert err == 0 and res[1][1] == oicp.stats.iterations and res[1][2] == oicp.stats.pairs
    dt, dr = amd.synth.pose_error(T, T_ref)
    assert dt <= 1e-4 and dr <= 1e-4, (dt, dr)


# ------------------------------------------------------------------------------------------------------------------ the C++ shell
def test_cpp_shell_hands_the_filtered_readings_row_over(amd, ref):
    """GpuICPSequence: the radii are the descriptor of the FILTERED reading -- here the row SimpleSensorNoiseDataPointsFilter writes inside
    readingDataPointsFilters -- and the registration is the Python mirror's with that row"""
    import host_chain_bindings as hcb
    sc = ref["sc"]
    filt = "SimpleSensorNoiseDataPointsFilter: {sensorType: 0, gain: 5}"
    yaml = ("readingDataPointsFilters:\n  - SimpleSensorNoiseDataPointsFilter:\n      sensorType: 0\n      gain: 5\n"
            "matcher:\n  KDTreeVarDistMatcher:\n    knn: 1\n    maxDistField: simpleSensorNoise\n"
            "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\nerrorMinimizer: PointToPointErrorMinimizer\n"
            "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 8\n")
    T, st = hcb.icp_register(yaml, sc["map"], sc["normals"], sc["scan"])
    stage = amd.ICPSequence(minimizer=0)
    _, descs = hcb.filter_chain_descs("[{%s}]" % filt, sc["scan"], handle=stage._h.value)
    row = dict(descs)["simpleSensorNoise"].ravel()
    assert row.shape == (vr.N,) and 0.05 < row.min() and row.max() < 1.0
    icp = amd.ICPSequence.loadFromYaml({     # the same chain in the mirror: maxDistField names the row __call__ takes from `descriptors`
        "matcher": {"KDTreeVarDistMatcher": {"knn": 1, "maxDistField": "simpleSensorNoise"}},
        "outlierFilters": [{"TrimmedDistOutlierFilter": {"ratio": RATIO}}], "errorMinimizer": "PointToPointErrorMinimizer",
        "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 8}}]})
    assert icp.cfg.var_dist == 1 and icp.cfg.max_dist_field == "simpleSensorNoise"
    assert icp.setMap(sc["map"], sc["normals"])
    icp.setReadingSensorNoise(row)           # (the shell also hands a reading's `simpleSensorNoise` row over for getOverlap())
    T_py = icp(sc["scan"], descriptors={"simpleSensorNoise": row})
    assert same_bits(T, T_py) and st.pairs == icp.stats.pairs and 0 < st.pairs < vr.N
    with pytest.raises(RuntimeError, match="no 1-row descriptor maxSearchDist"):
        hcb.icp_register(yaml.replace("    maxDistField: simpleSensorNoise\n", ""), sc["map"], sc["normals"], sc["scan"])
