"""The voxel pose score on the device (csrc/voxel.hip: voxel_score_kernel, voxel_score_finish_kernel), through the C ABI:
against the float64 score and the float32 restatement of the header's arithmetic (tests/voxel_score_reference.py), bit for bit across the
ways the same pose can be asked for, the errors of one pose and of the whole call, and ranking / relocalisation on the room scene.
Tolerances: pairs and max_maha exactly the restatement's; likelihood and sum_maha within four times what the restatement loses against
float64 on the same case (profiles/voxel_score_tolerance.json, measured on the CPU by scripts/voxel_score_tolerance.py), the likelihood
with a floor of 2 units of float32 roundoff, the documented bound of the device's expf (1 ULP) -- never the device's own output.

The pair count is also compared with slot 27 of the sums icpmi_minimize_step_normals returns under the same pose.  (icpmi_debug_last_sums
serves the nearest-neighbour loop's registrations only: on a voxel handle it answers ICPMI_ERR_UNSUPPORTED, so the step call's own sums,
the same 32 doubles, are read instead.)"""
import ctypes as C
import os

import numpy as np
import pytest

import host_voxel_score_bindings as hv
import localizability_reference as lr
import voxel_reference as vr
import voxel_score_cases as vsc
import voxel_score_reference as sr

pytestmark = pytest.mark.gpu
F = np.float32
OK, INVALID_ARG, NO_POINT, MISSING_NORMALS, UNSUPPORTED = 0, 1, 3, 7, 8
MIN_PLANE_TO_PLANE = 3
REG = dict(max_iterations=vr.MAX_ITER, use_differential=1)


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def tol():
    return vsc.recorded()


@pytest.fixture(scope="module")
def scene():
    sc = lr.scene(vsc.SCENE)
    return dict(map=sc["map"], normals=sc["normals"], rd=np.ascontiguousarray(sc["reading"]), rn=np.ascontiguousarray(sc["reading_normals"]))


def make_icp(amd, scene, size=None, sizes=None, **kw):
    kw.setdefault("minimizer", MIN_PLANE_TO_PLANE)
    kw.setdefault("outliers", [])
    icp = amd.ICPSequence(knn=1, max_dist=2.0, voxel_size=size, voxel_sizes=None if sizes is None else list(sizes), **kw)
    assert icp.setMap(scene["map"], scene["normals"])
    return icp


@pytest.fixture(scope="module")
def handles(amd, scene):
    """one handle per size and one with the schedule, shared by the tests that only score"""
    hs = {s: make_icp(amd, scene, size=s, **REG) for s in vsc.SIZES}
    hs["sched"] = make_icp(amd, scene, sizes=vsc.SCHEDULE, **REG)
    yield hs
    for h in hs.values():
        h.close()


def map_pose(icp, Tc):
    """the float32 map-frame correction for a centred-frame pose"""
    return sr.map_frame_pose(Tc, icp.getMapMean()).astype(F)


def grid_poses(icp, K):
    return np.stack([map_pose(icp, G @ K) for G in vsc.grid()])


def raw(icp, reading, normals, poses, level=-1, beta=1.0, dev=False, with_status=True, opts=True):
    """the C call itself: (return value, bytes of out, list of status)"""
    from norlab_icp_mapper_amd import _capi
    Tc = icp._poses_to_c(poses)
    P = Tc.shape[0] // 16
    o = _capi.VoxelScoreOptions()
    icp._lib.icpmi_voxel_score_options_default(C.byref(o))
    o.level, o.beta = level, beta
    out = (_capi.VoxelScore * P)()
    status = (C.c_int * P)(*([-1] * P))
    C.memset(out, 0xAB, C.sizeof(out))
    if dev:
        import torch
        d, dn = torch.from_numpy(np.ascontiguousarray(reading, F)).cuda(), torch.from_numpy(np.ascontiguousarray(normals, F)).cuda()
        rv = icp._lib.icpmi_voxel_score_poses_dev(icp._h, d.data_ptr(), reading.shape[0], dn.data_ptr(), Tc.ctypes.data, P, C.byref(o) if opts else None, out,
                                                  status if with_status else None)
    else:
        r, nn = np.ascontiguousarray(reading, F), np.ascontiguousarray(normals, F)
        rv = icp._lib.icpmi_voxel_score_poses(icp._h, r.ctypes.data, r.shape[0], nn.ctypes.data, Tc.ctypes.data, P, C.byref(o) if opts else None, out,
                                              status if with_status else None)
    size = C.sizeof(_capi.VoxelScore)
    b = bytes(out)
    return rv, [b[i * size:(i + 1) * size] for i in range(P)], list(status)


# ------------------------------------------------------------------------------------------------------------------ 1. against the references
def test_shape_is_what_the_cases_assume(amd):
    from norlab_icp_mapper_amd import _capi
    sl, tl = C.c_int32(0), C.c_int32(0)
    _capi.load().icpmi_voxel_score_shape(C.byref(sl), C.byref(tl))
    assert (sl.value, tl.value) == (vsc.SLICE, vsc.TILE)


@pytest.mark.parametrize("n", vsc.N_VALUES)
@pytest.mark.parametrize("size", vsc.SIZES)
def test_against_float64_and_the_float32_restatement(handles, scene, tol, size, n):
    icp = handles[size]
    mean = icp.getMapMean()
    names = list(vsc.POSES)
    got = icp.voxelScores(scene["rd"][:n], scene["rn"][:n], [map_pose(icp, vsc.POSES[p]) for p in names])
    rc = vr.centred(scene["rd"][:n], mean)
    for p, st, g in zip(names, got.status, got.scores):
        r64, r32 = vsc.references(size, p, n, mean)
        rec = tol["rel"][vsc.case_key(size, p, n)]
        dl, ds = sr.rel(g.likelihood, r64["likelihood"]), sr.rel(g.sum_maha, r64["sum_maha"])
        allow_l = max(vsc.MARGIN * rec["likelihood"], tol["likelihood_floor_units"] * tol["roundoff"])
        allow_s = vsc.MARGIN * rec["sum_maha"]
        print(f"size {size} n {n} {p}: pairs {g.pairs} (restatement {r32['pairs']}), likelihood off by {dl:.3e} (allowed {allow_l:.3e}; from the "
              f"restatement {sr.rel(g.likelihood, r32['likelihood']):.3e}), sum_maha off by {ds:.3e} (allowed {allow_s:.3e}; from the restatement "
              f"{sr.rel(g.sum_maha, r32['sum_maha']):.3e}), max_maha {g.max_maha!r} (restatement {r32['max_maha']!r})")
        assert g.pairs == r32["pairs"]
        assert st == (OK if g.pairs else NO_POINT)
        assert np.float32(g.max_maha).view(np.uint32) == np.float32(r32["max_maha"]).view(np.uint32)
        assert dl <= allow_l and ds <= allow_s
        assert g.level == 0 and g.pairs_ratio == np.float32(g.pairs / n)
        # the pair count of the registration's own pair sums under the same pose
        _, Tc = vsc.map_frame(vsc.POSES[p], mean)
        if g.pairs:
            _, sums = icp.minimizeStep(rc, Tc, read_normals=scene["rn"][:n])
            assert sums[27] == g.pairs == sums[28]


# ------------------------------------------------------------------------------------------------------------------ 2. bits
def pose_pool(icp, count):
    """`count` distinct rigid poses around the truth (deterministic): small yaw / translation offsets of the start pose"""
    rng = np.random.default_rng(42)
    out = []
    for _ in range(count):
        G = lr.make_T((0.0, 0.0, rng.uniform(-0.2, 0.2)), (rng.uniform(-1, 1), rng.uniform(-1, 1), 0.0))
        out.append(map_pose(icp, G @ vr.POSES["start"]))
    return np.stack(out)


def test_every_pose_is_the_single_pose_call(handles, scene):
    icp = handles[0.5]
    n = 257
    rd, rn = scene["rd"][:n], scene["rn"][:n]
    pool = pose_pool(icp, 65)
    single = [raw(icp, rd, rn, pool[i:i + 1]) for i in range(65)]
    assert all(rv == OK for rv, _, _ in single) and len({s[1][0] for s in single}) > 50
    for P in vsc.POSE_COUNTS:
        rv, out, status = raw(icp, rd, rn, pool[:P])
        assert rv == OK and out == [single[i][1][0] for i in range(P)] and status == [single[i][2][0] for i in range(P)], P
        assert raw(icp, rd, rn, pool[:P]) == (rv, out, status), P                                   # twice
        perm = np.random.default_rng(P).permutation(P)
        rv2, out2, status2 = raw(icp, rd, rn, pool[:P][perm])
        assert rv2 == OK and out2 == [out[i] for i in perm] and status2 == [status[i] for i in perm], P
        assert raw(icp, rd, rn, pool[:P], dev=True) == (rv, out, status), P                         # the reading in HBM
    assert raw(icp, rd, rn, pool[:3], opts=False) == raw(icp, rd, rn, pool[:3])                      # opts NULL = the defaults


def test_4096_poses(handles, scene):
    icp = handles[1.0]
    n = 65
    rd, rn = scene["rd"][:n], scene["rn"][:n]
    pool = pose_pool(icp, 64)
    idx = np.random.default_rng(7).integers(0, 64, 4096)
    single = [raw(icp, rd, rn, pool[i:i + 1]) for i in range(64)]
    rv, out, status = raw(icp, rd, rn, pool[idx])
    assert rv == OK and out == [single[i][1][0] for i in idx] and status == [single[i][2][0] for i in idx]
    rv, out, status = raw(icp, rd, rn, np.concatenate([pool[idx], pool[:1]]))                       # 4097: the whole call fails, zeroed
    assert rv == INVALID_ARG and all(b == bytes(len(b)) for b in out[:4096]) and status[:4096] == [0] * 4096   # (the limit's worth is zeroed)


def test_a_level_of_the_schedule_is_the_one_size_handle(handles, scene):
    sched = handles["sched"]
    n = 1025
    rd, rn = scene["rd"][:n], scene["rn"][:n]
    pool = pose_pool(sched, 17)
    for level, size in enumerate(vsc.SCHEDULE):
        rv, out, status = raw(sched, rd, rn, pool, level=level)
        rv1, out1, status1 = raw(handles[size], rd, rn, pool)
        assert rv == rv1 == OK and status == status1
        lv = np.frombuffer(b"".join(out), np.int32).reshape(17, -1)[:, 8]                           # icpmi_voxel_score::level
        assert (lv == level).all()
        strip = lambda b: b[:32] + b[36:]                                                            # every field but the level
        assert [strip(b) for b in out] == [strip(b) for b in out1], level
    assert raw(sched, rd, rn, pool, level=-1) == raw(sched, rd, rn, pool, level=len(vsc.SCHEDULE) - 1)   # -1: the finest


def test_beta_changes_the_likelihood_alone(handles, scene):
    icp = handles[1.0]
    pool = pose_pool(icp, 5)
    a = icp.voxelScores(scene["rd"], scene["rn"], pool, beta=1.0)
    b = icp.voxelScores(scene["rd"], scene["rn"], pool, beta=0.1)
    for x, y in zip(a.scores, b.scores):
        assert x.likelihood < y.likelihood <= x.pairs                                               # a flatter kernel: every term grows, none above 1
        assert (x.sum_maha, x.pairs, x.max_maha, x.pairs_ratio, x.level) == (y.sum_maha, y.pairs, y.max_maha, y.pairs_ratio, y.level)
    assert a.status == b.status == [OK] * 5


# ------------------------------------------------------------------------------------------------------------------ 3. errors
def test_errors_of_one_pose(handles, scene):
    icp = handles[0.5]
    n = 257
    rd, rn = scene["rd"][:n], scene["rn"][:n]
    pool = pose_pool(icp, 4)
    bad = pool[0].copy()
    bad[:3, :3] *= F(1.5)                                                                            # not rigid
    far = map_pose(icp, lr.make_T((0.0, 0.0, 0.0), (1000.0, 0.0, 0.0)))
    rv0, out0, status0 = raw(icp, rd, rn, pool)
    rv, out, status = raw(icp, rd, rn, np.stack([pool[0], bad, pool[1], far, pool[2], pool[3]]))
    assert rv == OK and status == [OK, INVALID_ARG, OK, NO_POINT, OK, OK]
    assert [out[i] for i in (0, 2, 4, 5)] == out0 and out[1] == bytes(len(out[1]))                  # the others as without it; that pose zero
    s = np.frombuffer(out[3], np.float64, 2)
    assert (s == 0).all() and np.frombuffer(out[3], np.int64, 1, 16)[0] == 0
    # status == NULL: the first per-pose error is the return value
    rv, out2, _ = raw(icp, rd, rn, np.stack([pool[0], far, bad]), with_status=False)
    assert rv == NO_POINT and out2[0] == out0[0]
    assert icp.voxelScores(rd, rn, np.stack([pool[0], bad])).status == [OK, INVALID_ARG]


def test_errors_of_the_whole_call(amd, handles, scene):
    from norlab_icp_mapper_amd import _capi, icp as I
    icp = handles[0.5]
    rd, rn = scene["rd"][:100], scene["rn"][:100]
    pool = pose_pool(icp, 3)
    lib, h = icp._lib, icp._h
    Tc = icp._poses_to_c(pool)

    def call(handle=h, scan=rd.ctypes.data, n=100, nrm=rn.ctypes.data, T=Tc.ctypes.data, P=3, level=-1, beta=1.0, out_null=False):
        o = _capi.VoxelScoreOptions()
        lib.icpmi_voxel_score_options_default(C.byref(o))
        o.level, o.beta = level, beta
        cap = max(P, 3)
        out = (_capi.VoxelScore * cap)()
        C.memset(out, 0xAB, C.sizeof(out))
        status = (C.c_int * cap)(*([-1] * cap))
        rv = lib.icpmi_voxel_score_poses(handle, scan, n, nrm, T, P, C.byref(o), None if out_null else out, status)
        if rv != OK and P >= 1 and not out_null:                                                     # zeroed on every whole-call error
            Z = min(P, 4096)
            assert bytes(out)[:Z * C.sizeof(_capi.VoxelScore)] == bytes(Z * C.sizeof(_capi.VoxelScore)) and list(status)[:Z] == [0] * Z
        return rv

    assert call(scan=None) == INVALID_ARG and call(T=None) == INVALID_ARG and call(out_null=True) == INVALID_ARG
    assert call(n=-1) == INVALID_ARG and call(P=0) == INVALID_ARG and call(P=4097) == INVALID_ARG
    assert call(level=1) == INVALID_ARG and call(level=-2) == INVALID_ARG                            # a one-size handle has level 0 alone
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert call(beta=beta) == INVALID_ARG
    assert call(nrm=None) == MISSING_NORMALS
    assert call(n=0) == NO_POINT
    assert call(handles["sched"]._h, level=2) == INVALID_ARG and call(handles["sched"]._h, level=1, P=3) == OK
    # not on the voxel path: the message names the call and the setter
    nn = amd.ICPSequence(knn=1, max_dist=2.0, minimizer=MIN_PLANE_TO_PLANE, outliers=[])
    try:
        assert nn.setMap(scene["map"], scene["normals"])
        assert call(nn._h) == UNSUPPORTED
        msg = lib.icpmi_last_error(nn._h).decode()
        assert "voxel_score_poses" in msg and "icpmi_set_voxel_matcher" in msg
        with pytest.raises(NotImplementedError, match="icpmi_set_voxel_matcher"):
            nn.voxelScores(rd, rn, pool)
    finally:
        nn.close()
    # no map; a map without normals
    empty = amd.ICPSequence(knn=1, max_dist=2.0, minimizer=MIN_PLANE_TO_PLANE, outliers=[], voxel_size=0.5)
    try:
        assert call(empty._h) == INVALID_ARG and "no map" in lib.icpmi_last_error(empty._h).decode()
        assert empty.setMap(scene["map"])
        assert call(empty._h) == MISSING_NORMALS
        with pytest.raises(I.InvalidField):
            empty.voxelScores(rd, rn, pool)
    finally:
        empty.close()


def test_the_handle_afterwards(amd, scene):
    """a registration before and after the call gives the same bits (result, statistics, schedule report), and a scan staged by
    icpmi_register_prior is still the one icpmi_residual_error_staged scores"""
    icp = make_icp(amd, scene, sizes=vsc.SCHEDULE, **REG)
    try:
        K = map_pose(icp, vr.POSES["start"])
        moved, movedn = icp.transform(K, scene["rd"], scene["rn"])
        reg = lambda: (icp(moved, movedn).view(np.uint32).tolist(), icp.stats.iterations, icp.stats.stop_reason, icp.stats.pairs, icp.voxelScheduleReport())
        before = reg()
        again = reg()                                                                                # (the second runs the cached loop)
        assert again == before
        with pytest.raises(Exception):
            icp.registerWithPrior(scene["rd"], np.eye(4, dtype=F))                                   # refused (no normals travel), but the scan is staged
        staged = icp.residualStaged(K, kind=1).bits()
        rep = icp.voxelScheduleReport()
        pool = pose_pool(icp, 20)
        s0 = icp.voxelScores(scene["rd"], scene["rn"], pool, level=0)
        assert icp.voxelScheduleReport() == rep
        assert icp.residualStaged(K, kind=1).bits() == staged                                        # the staged scan survived
        assert reg() == before
        assert icp.voxelScores(scene["rd"], scene["rn"], pool, level=0).bits() == s0.bits()
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 4. ranking and relocalisation
@pytest.mark.parametrize("key", list(vsc.PROTOTYPE))
def test_the_centre_ranks_first(amd, handles, scene, key):
    size, kname = key
    own = None
    if size in handles:
        icp = handles[size]
    else:
        icp = own = make_icp(amd, scene, size=size, **REG)
    try:
        K = np.eye(4) if kname == "identity" else vr.POSES[kname]
        scores = icp.voxelScores(scene["rd"], scene["rn"], grid_poses(icp, K))
        order = amd.rank_voxel_candidates(scores, scene["rd"].shape[0])
        L = [s.likelihood / scene["rd"].shape[0] for s in scores.scores]
        print(key, order[:2], L[order[0]], L[order[1]], "prototype", vsc.PROTOTYPE[key])
        assert order[0] == vsc.CENTRE
    finally:
        if own is not None:
            own.close()


CHAIN = {"matcher": {"VoxelMatcher": {"voxelSizes": list(vsc.SCHEDULE)}}, "errorMinimizer": {"PlaneToPlaneErrorMinimizer": {"epsilon": 0.001}},
         "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}},
                                    {"DifferentialTransformationChecker": {"minDiffRotErr": 0.001, "minDiffTransErr": 0.001, "smoothLength": 3}}]}
YAML_CHAIN = """matcher:
  VoxelMatcher:
    voxelSizes: [1.0, 0.5]
errorMinimizer:
  PlaneToPlaneErrorMinimizer:
    epsilon: 0.001
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 40
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.001
      smoothLength: 3
"""
MAPPER_YAML = """
input:
  - BoundingBoxDataPointsFilter:
      xMin: 100.0
      xMax: 100.1
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
icp:
  %s
""" % YAML_CHAIN.replace("\n", "\n  ").rstrip()


def test_relocalize_voxel(amd, scene, tmp_path):
    from norlab_icp_mapper_amd import icp as I
    icp = amd.ICPSequence.loadFromYaml(CHAIN)
    try:
        assert icp.setMap(scene["map"], scene["normals"]) and icp.getVoxelSchedule() == list(vsc.SCHEDULE)
        cand = grid_poses(icp, vr.POSES["start"])
        rd, rn = scene["rd"], scene["rn"]
        found = icp.relocalizeVoxel(rd, rn, cand)
        assert found.index == vsc.CENTRE and len(found.scores) == 125 and found.scores.scores[0].level == 0
        assert isinstance(found.residual, I.VoxelScore) and found.residual.level == 1 and found.residual.pairs > 0.9 * rd.shape[0]
        # the pose: what registering the reading moved by that candidate returns alone, composed with the candidate
        moved, movedn = icp.transform(cand[vsc.CENTRE], rd, rn)
        alone = I.compose_pose(icp(moved, movedn), cand[vsc.CENTRE])
        assert np.array_equal(found.pose.view(np.uint32), alone.view(np.uint32))
        # ... and it is the truth: the reading sits at the true pose, so the correction in the centred frame is the identity
        Tc = sr.centred_pose(found.pose, icp.getMapMean()).astype(np.float64)
        assert np.abs(Tc[:3, 3]).max() < 5e-3 and np.abs(Tc[:3, :3] - np.eye(3)).max() < 2e-3
        with pytest.raises(NotImplementedError):                                                     # relocalize is refused as before
            icp.relocalize(rd, cand[:3])
        want_scores = found.scores.bits()
    finally:
        icp.close()
    # the host shell: the same bits
    got = hv.icp_relocalize_voxel(YAML_CHAIN, scene["map"], scene["normals"], rd, rn, cand)
    assert got["index"] == vsc.CENTRE and np.array_equal(got["pose"].view(np.uint32), found.pose.view(np.uint32))
    assert (got["status"], [I.VoxelScore(s).bits() for s in got["scores"]]) == ([st for st, _ in want_scores], [b for _, b in want_scores])
    assert I.VoxelScore(got["score"]).bits() == found.residual.bits()
    alone = hv.icp_relocalize_voxel(YAML_CHAIN, scene["map"], scene["normals"], rd, rn, cand[:7], refine=-1, level=1, beta=0.1)
    icp = amd.ICPSequence.loadFromYaml(CHAIN)
    try:
        assert icp.setMap(scene["map"], scene["normals"])
        ref = icp.voxelScores(rd, rn, cand[:7], level=1, beta=0.1)
        assert [I.VoxelScore(s).bits() for s in alone["scores"]] == [s.bits() for s in ref.scores] and alone["status"] == ref.status
    finally:
        icp.close()
    # the mapper: the input filters, the current map, the pose set, no map update
    cfg = os.path.join(str(tmp_path), "config.yaml")
    open(cfg, "w").write(MAPPER_YAML)
    m = hv.mapper_relocalize_voxel(cfg, scene["map"], scene["normals"], rd, rn, cand)
    assert m["map_before"] == m["map_after"] == scene["map"].shape[0]
    assert np.array_equal(m["pose"].view(np.uint32), m["get_pose"].view(np.uint32))
    assert m["index"] == vsc.CENTRE and np.array_equal(m["pose"].view(np.uint32), found.pose.view(np.uint32))


def test_relocalize_voxel_without_a_survivor(amd, handles, scene):
    icp = handles["sched"]
    far = np.stack([map_pose(icp, lr.make_T((0.0, 0.0, 0.0), (1000.0 + i, 0.0, 0.0))) for i in range(3)])
    with pytest.raises(amd.ConvergenceError, match="no candidate survived"):
        icp.relocalizeVoxel(scene["rd"], scene["rn"], far)
