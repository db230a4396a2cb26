"""Many readings, or many starts, registered in one loop on the voxel path (csrc/voxel.hip: voxel_pairs_batch_kernel; csrc/loop.hip:
voxel_advance_batch_kernel, loop_run_voxel_batch), through the C ABI and both front ends.  Equality is == on the float32
bits of T_out and on every field of icpmi_stats but the timing fields (loop_ms, nn_ms_avg, nn_launches): no tolerance anywhere.  The
reference of every batch is the single call (icpmi_register_dev / icpmi_register_fixed_dev) on the same handle."""
import ctypes as C

import numpy as np
import pytest

import localizability_reference as lr
import voxel_batch_cases as bc
import voxel_cases as vc
import voxel_reference as vr
import voxel_score_cases as vsc
import voxel_score_reference as sr

pytestmark = pytest.mark.gpu
F = np.float32
OK, INVALID_ARG, NO_POINT, MISSING_NORMALS, UNSUPPORTED = 0, 1, 3, 7, 8
REG = dict(max_iterations=vr.MAX_ITER, use_differential=1)
TIMING = ("loop_ms", "nn_ms_avg", "nn_launches")
IDENTITY_BITS = tuple(np.eye(4, dtype=F).T.ravel().view(np.uint32).tolist())


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def make_icp(amd, sizes, with_map=True, **kw):
    kw.setdefault("minimizer", vc.MIN_PLANE_TO_PLANE)
    kw.setdefault("outliers", [])
    for k, v in REG.items():
        kw.setdefault(k, v)
    icp = amd.ICPSequence(knn=1, max_dist=2.0, voxel_sizes=None if sizes is None else list(sizes), **kw)
    if with_map:
        sc = lr.scene("room")
        assert icp.setMap(sc["map"], sc["normals"])
    return icp


@pytest.fixture(scope="module")
def handles(amd):
    hs = {s: make_icp(amd, s) for s in bc.HANDLES}
    yield hs
    for h in hs.values():
        h.close()


class Dev:
    """readings and normals in HBM, kept alive while the pointers are in use"""
    def __init__(self, readings):
        import torch
        self.t = [(torch.from_numpy(np.ascontiguousarray(r, F)).cuda() if r.shape[0] else None,
                   torch.from_numpy(np.ascontiguousarray(n, F)).cuda() if n is not None and n.shape[0] else None) for r, n in readings]
        self.n = [r.shape[0] for r, _ in readings]

    def pts(self, b):
        return None if self.t[b][0] is None else self.t[b][0].data_ptr()

    def nrm(self, b):
        return None if self.t[b][1] is None else self.t[b][1].data_ptr()


def stats_key(st):
    """every field of icpmi_stats outside the timing fields, floats by their bits"""
    from norlab_icp_mapper_amd import _capi
    out = []
    for name, typ in _capi.Stats._fields_:
        if name in TIMING:
            continue
        v = getattr(st, name)
        if typ is C.c_float:
            v = int(np.array([v], F).view(np.uint32)[0])
        elif not isinstance(v, int):
            v = tuple(v)
        out.append((name, v))
    return tuple(out)


def bits16(T):
    return tuple(np.array(T[:16], F).view(np.uint32).tolist())


def report_of(icp, member=None):
    if len(icp.getVoxelSchedule()) < 2:
        return None
    return icp.voxelScheduleReport() if member is None else icp.voxel_batch_report(member)


def single(icp, d, b, fixed=0):
    """the single call on member b: (status, T bits, stats key, report)"""
    from norlab_icp_mapper_amd import _capi
    T, st = (C.c_float * 16)(), _capi.Stats()
    if fixed:
        rv = icp._lib.icpmi_register_fixed_dev(icp._h, d.pts(b), d.n[b], d.nrm(b), fixed, T, C.byref(st))
    else:
        rv = icp._lib.icpmi_register_dev(icp._h, d.pts(b), d.n[b], d.nrm(b), T, C.byref(st))
    return rv, bits16(T), stats_key(st), report_of(icp)


def batch(icp, d, order=None, fixed=0, with_status=True):
    """icpmi_voxel_register_batch_dev over the members `order` of d: (return value, [(status, T bits, stats key, report)] in that order)"""
    from norlab_icp_mapper_amd import _capi
    order = list(range(len(d.n))) if order is None else list(order)
    B = len(order)
    ptrs = (C.c_void_p * B)(*[d.pts(b) for b in order])
    nptrs = (C.c_void_p * B)(*[d.nrm(b) for b in order])
    ns = (C.c_int64 * B)(*[d.n[b] for b in order])
    T, st, status = (C.c_float * (16 * B))(), (_capi.Stats * B)(), (C.c_int * B)(*([-1] * B))
    C.memset(T, 0xAB, C.sizeof(T))
    rv = icp._lib.icpmi_voxel_register_batch_dev(icp._h, B, ptrs, ns, nptrs, fixed, T, st, status if with_status else None)
    out = [(status[i] if with_status else None, bits16(T[16 * i:16 * i + 16]), stats_key(st[i]), report_of(icp, i) if rv == OK or not with_status else None)
           for i in range(B)]
    return rv, out


def same(got, want, with_status=True):
    """a member of a batch against its single call"""
    if with_status:
        assert got[0] == want[0], (got[0], want[0])
    assert got[1] == want[1], "T_out differs"
    assert got[2] == want[2], (got[2], want[2])
    assert got[3] == want[3], (got[3], want[3])


def iterations_of(res):
    return dict(res[2])["iterations"]


# ------------------------------------------------------------------------------------------------------------------ 1. a batch is its members alone
@pytest.mark.parametrize("sizes", bc.HANDLES)
def test_a_batch_is_its_members_alone(handles, sizes):
    icp = handles[sizes]
    d = Dev(bc.members())
    before = [single(icp, d, b) for b in range(4)]
    rv, got = batch(icp, d)
    after = [single(icp, d, b) for b in range(4)]
    assert rv == OK
    for b in range(4):
        print(sizes, bc.MEMBERS[b], "status", before[b][0], "iterations", iterations_of(before[b]), "report", before[b][3])
        assert before[b] == after[b]
        same(got[b], before[b])
    # the inputs do what the test is about: the three larger members converge and stop at different iterations
    assert [r[0] for r in before[:3]] == [OK, OK, OK]
    assert len({iterations_of(r) for r in before[:3]}) == 3
    if sizes == bc.FOUR:        # ... and are at different levels at the same iteration
        reports = [got[b][3] for b in range(3)]
        shortest = min(sum(its for its, _, _ in rep) for rep in reports)
        assert any(len({bc.levels_at(rep, i) for rep in reports}) > 1 for i in range(1, shortest + 1))
        assert all(len(rep) == 4 for rep in reports)


# ------------------------------------------------------------------------------------------------------------------ 2. fixed iterations, sixteen members
@pytest.mark.parametrize("sizes", bc.HANDLES)
def test_fixed_iterations(handles, sizes):
    icp = handles[sizes]
    d = Dev(bc.members())
    want = [single(icp, d, b, fixed=3) for b in range(4)]
    rv, got = batch(icp, d, fixed=3)
    assert rv == OK
    for b in range(4):
        same(got[b], want[b])
    assert iterations_of(want[0]) == 3 * len(sizes)


def test_a_batch_of_sixteen(handles):
    icp = handles[(1.0, 0.5)]
    d = Dev(bc.members(bc.SIXTEEN))
    want = {}
    for b, spec in enumerate(bc.SIXTEEN):
        if spec not in want:
            want[spec] = single(icp, d, b)
    rv, got = batch(icp, d)
    assert rv == OK
    for b, spec in enumerate(bc.SIXTEEN):
        same(got[b], want[spec])
    assert len({iterations_of(r) for r in want.values()}) > 1


# ------------------------------------------------------------------------------------------------------------------ 3. a failed member among good ones
@pytest.mark.parametrize("sizes", [(1.0,), (4.0, 2.0, 1.0, 0.5)])
def test_a_failed_member_among_good_ones(handles, sizes):
    icp = handles[sizes]
    ms = bc.members()[:3]
    ms.insert(1, bc.far_member())
    d = Dev(ms)
    want = [single(icp, d, b) for b in range(4)]
    assert want[1][0] == NO_POINT and want[1][1] == IDENTITY_BITS
    rv, got = batch(icp, d)
    assert rv == OK and [g[0] for g in got] == [OK, NO_POINT, OK, OK]
    for b in range(4):
        same(got[b], want[b])
    # without a status array the first error is the return value, and the results are the same
    rv, got = batch(icp, d, with_status=False)
    assert rv == NO_POINT and "per-reading status" in icp._lib.icpmi_last_error(icp._h).decode()
    for b in range(4):
        same(got[b], want[b], with_status=False)


# ------------------------------------------------------------------------------------------------------------------ 4. order does not matter
@pytest.mark.parametrize("sizes", [(0.5,), (4.0, 2.0, 1.0, 0.5)])
def test_order_does_not_matter(handles, sizes):
    icp = handles[sizes]
    d = Dev(bc.members())
    rv, fwd = batch(icp, d)
    rv2, rev = batch(icp, d, order=[3, 2, 1, 0])
    assert rv == rv2 == OK
    for b in range(4):
        assert fwd[b] == rev[3 - b]
    rv3, pair = batch(icp, d, order=[2, 0])      # ... nor which readings share the launch
    assert rv3 == OK and pair[0] == fwd[2] and pair[1] == fwd[0]


# ------------------------------------------------------------------------------------------------------------------ 5. multistart
def multistart(icp, rd, rn, priors, dev, fixed=0):
    from norlab_icp_mapper_amd import _capi
    Tc = icp._poses_to_c(priors)
    S = Tc.shape[0] // 16
    T, st, status = (C.c_float * (16 * S))(), (_capi.Stats * S)(), (C.c_int * S)(*([-1] * S))
    if dev:
        d = Dev([(rd, rn)])
        rv = icp._lib.icpmi_voxel_register_multistart_dev(icp._h, d.pts(0), rd.shape[0], d.nrm(0), Tc.ctypes.data, S, fixed, T, st, status)
    else:
        rv = icp._lib.icpmi_voxel_register_multistart(icp._h, rd.ctypes.data, rd.shape[0], rn.ctypes.data, Tc.ctypes.data, S, fixed, T, st, status)
    return rv, [(status[s], bits16(T[16 * s:16 * s + 16]), stats_key(st[s]), report_of(icp, s) if rv == OK else None) for s in range(S)]


def by_hand(icp, rd, rn, prior):
    """icpmi_transform + icpmi_register, as relocalizeVoxel refined a candidate before the multistart"""
    from norlab_icp_mapper_amd import _capi
    moved, movedn = icp.transform(prior, rd, rn)
    T, st = (C.c_float * 16)(), _capi.Stats()
    rv = icp._lib.icpmi_register(icp._h, moved.ctypes.data, rd.shape[0], movedn.ctypes.data, T, C.byref(st))
    return rv, bits16(T), stats_key(st), report_of(icp)


@pytest.mark.parametrize("sizes", bc.HANDLES)
def test_multistart_is_transform_and_register(handles, sizes):
    icp = handles[sizes]
    rd, rn = bc.unmoved()
    P = bc.priors()
    want = [by_hand(icp, rd, rn, P[s]) for s in range(4)]
    rv, got = multistart(icp, rd, rn, P, dev=True)
    assert rv == OK
    for s in range(4):
        print(sizes, "start", bc.MULTISTART[s], "status", want[s][0], "iterations", iterations_of(want[s]))
        same(got[s], want[s])
    rv, host = multistart(icp, rd, rn, P, dev=False)
    assert rv == OK and host == got
    assert len({iterations_of(w) for w in want}) > 1


def test_multistart_with_a_prior_that_is_not_rigid(handles):
    icp = handles[(1.0, 0.5)]
    rd, rn = bc.unmoved()
    P = bc.priors().copy()
    rv, good = multistart(icp, rd, rn, P, dev=True)
    P[1, :3, :3] *= F(1.2)
    rv, got = multistart(icp, rd, rn, P, dev=True)
    assert rv == OK and got[1][0] == INVALID_ARG and got[1][1] == IDENTITY_BITS and got[1][3] == []
    for s in (0, 2, 3):
        assert got[s] == good[s]
    rv, fixed = multistart(icp, rd, rn, bc.priors(), dev=True, fixed=2)
    assert rv == OK and [iterations_of(f) for f in fixed] == [4, 4, 4, 4]


# ------------------------------------------------------------------------------------------------------------------ 6. special routes
@pytest.mark.parametrize("sizes", [(1.0,), (1.0, 0.5)])
def test_special_routes(amd, handles, sizes):
    icp = handles[sizes]
    ms = bc.members()
    d = Dev(ms)
    want = [single(icp, d, b) for b in range(4)]
    for b in (0, 3):                                                     # a batch of one; a reading of one point
        rv, got = batch(icp, d, order=[b])
        assert rv == OK
        same(got[0], want[b])
    empty = (np.zeros((0, 4), F), np.zeros((0, 3), F))
    d0 = Dev([ms[0], empty, ms[2]])                                      # an n = 0 member: one by one, the empty member as the single call answers
    want0 = [single(icp, d0, b) for b in range(3)]
    assert want0[1][0] != OK
    rv, got = batch(icp, d0)
    assert rv == OK
    for b in range(3):
        same(got[b], want0[b])
    bare = make_icp(amd, sizes, with_map=False)                          # an empty map: identities and OK
    try:
        rv, got = batch(bare, d)
        assert rv == OK and all(g[0] == OK and g[1] == IDENTITY_BITS for g in got)
        rd, rn = bc.unmoved()
        rv, got = multistart(bare, rd, rn, bc.priors(), dev=False)
        assert rv == OK and all(g[0] == OK and g[1] == IDENTITY_BITS for g in got)
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def refused(icp, rv, code, word):
    msg = icp._lib.icpmi_last_error(icp._h).decode()
    assert rv == code and word in msg, (rv, msg)


def test_refusals(amd, handles):
    from norlab_icp_mapper_amd import _capi
    d = Dev(bc.members())
    rd, rn = bc.unmoved()
    off = make_icp(amd, None)                                            # a plane-to-plane handle off the voxel path
    try:
        rv, got = batch(off, d)
        refused(off, rv, INVALID_ARG, "icpmi_set_voxel_matcher")
        assert all(g[1] == IDENTITY_BITS for g in got)
        rv, _ = multistart(off, rd, rn, bc.priors(), dev=False)
        refused(off, rv, INVALID_ARG, "icpmi_set_voxel_matcher")
    finally:
        off.close()
    for kw, word in ((dict(outliers=[(4, 0.85)]), "outlier filters"), (dict(plane_model="symmetric"), "symmetric pair model")):
        icp = make_icp(amd, (1.0, 0.5), **kw)
        try:
            T, st = (C.c_float * 16)(), _capi.Stats()
            rv1 = icp._lib.icpmi_register_dev(icp._h, d.pts(0), d.n[0], d.nrm(0), T, C.byref(st))
            single_msg = icp._lib.icpmi_last_error(icp._h).decode()
            rv, got = batch(icp, d)
            refused(icp, rv, INVALID_ARG, word)
            assert rv1 == rv and icp._lib.icpmi_last_error(icp._h).decode() == single_msg     # the single registration's words
            assert all(g[1] == IDENTITY_BITS for g in got)
            rv, _ = multistart(icp, rd, rn, bc.priors(), dev=True)
            refused(icp, rv, INVALID_ARG, word)
        finally:
            icp.close()
    icp = handles[(1.0, 0.5)]
    nonorm = Dev(bc.members())
    nonorm.t[2] = (nonorm.t[2][0], None)                                 # a member with points and no normals pointer
    rv, got = batch(icp, nonorm)
    refused(icp, rv, MISSING_NORMALS, "normals")
    assert all(g[1] == IDENTITY_BITS for g in got)
    dd = Dev([(rd, rn)])
    Tc = icp._poses_to_c(bc.priors())
    T, st, status = (C.c_float * 64)(), (_capi.Stats * 4)(), (C.c_int * 4)()
    refused(icp, icp._lib.icpmi_voxel_register_multistart_dev(icp._h, dd.pts(0), rd.shape[0], None, Tc.ctypes.data, 4, 0, T, st, status), MISSING_NORMALS, "normals")
    for B in (0, 17):                                                    # batch / n_starts outside 1 .. 16
        ptrs, ns = (C.c_void_p * 17)(*([d.pts(0)] * 17)), (C.c_int64 * 17)(*([d.n[0]] * 17))
        nptrs = (C.c_void_p * 17)(*([d.nrm(0)] * 17))
        T17, st17, status17 = (C.c_float * (16 * 17))(), (_capi.Stats * 17)(), (C.c_int * 17)()
        refused(icp, icp._lib.icpmi_voxel_register_batch_dev(icp._h, B, ptrs, ns, nptrs, 0, T17, st17, status17), INVALID_ARG, "1 <= batch <= 16")
        P17 = np.ascontiguousarray(np.tile(np.eye(4, dtype=F).ravel(), 17))
        refused(icp, icp._lib.icpmi_voxel_register_multistart_dev(icp._h, dd.pts(0), rd.shape[0], dd.nrm(0), P17.ctypes.data, B, 0, T17, st17, status17),
                INVALID_ARG, "1 <= n_starts <= 16")
    lv, a = C.c_int32(0), (C.c_int32 * 4)()                              # the report: a member the last call did not have, a one-size handle
    rv, _ = batch(icp, d, order=[0, 1])
    assert rv == OK and icp._lib.icpmi_get_voxel_batch_report(icp._h, 1, C.byref(lv), a, a, a) == OK
    for m in (-1, 2):
        assert icp._lib.icpmi_get_voxel_batch_report(icp._h, m, C.byref(lv), a, a, a) == INVALID_ARG
    one = handles[(1.0,)]
    rv, _ = batch(one, d, order=[0, 1])
    assert rv == OK and one._lib.icpmi_get_voxel_batch_report(one._h, 0, C.byref(lv), a, a, a) == INVALID_ARG
    # the entry points that cannot carry normals keep refusing a voxel handle
    ptrs, ns = (C.c_void_p * 1)(d.pts(0)), (C.c_int64 * 1)(d.n[0])
    prior = np.ascontiguousarray(np.eye(4, dtype=F)).ravel()
    refused(icp, icp._lib.icpmi_register_batch_dev(icp._h, 1, ptrs, ns, 0, T, st, status), UNSUPPORTED, "register_batch")
    refused(icp, icp._lib.icpmi_register_multistart_dev(icp._h, d.pts(0), d.n[0], prior.ctypes.data, 1, 0, T, st, status), UNSUPPORTED, "register_multistart")


def test_the_handle_afterwards(amd):
    """the nearest-neighbour results of a handle with the size set back to 0 are what they were before a voxel batch ran on it; after a
    batch there is no covariance, nothing for icpmi_debug_last_matches and no staged scan"""
    icp = make_icp(amd, None)
    try:
        d = Dev(bc.members())
        nn_before = single(icp, d, 0)
        assert nn_before[0] == OK
        icp.setVoxelSchedule([1.0, 0.5])
        rv, _ = batch(icp, d)
        assert rv == OK
        ids, d2, Tu = (C.c_int32 * 2000)(), (C.c_float * 2000)(), (C.c_float * 16)()
        assert icp._lib.icpmi_debug_last_matches(icp._h, 2000, 1, ids, d2, Tu) != OK
        assert icp._lib.icpmi_get_covariance(icp._h, (C.c_float * 36)()) != OK
        from norlab_icp_mapper_amd import _capi
        res = _capi.Residual()
        eye = np.ascontiguousarray(np.eye(4, dtype=F)).ravel()
        assert icp._lib.icpmi_residual_error_staged(icp._h, eye.ctypes.data, 0, C.byref(res)) == INVALID_ARG
        icp.setVoxelSchedule([])
        assert single(icp, d, 0)[:3] == nn_before[:3]
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 8. a new map between two batches
def test_a_new_map_rebuilds_the_tables(amd):
    sc = lr.scene("room")
    icp = make_icp(amd, (1.0, 0.5))
    try:
        d = Dev(bc.members())
        rv, first = batch(icp, d)
        assert rv == OK
        keep = np.ones(sc["map"].shape[0], bool)
        keep[::3] = False
        assert icp.setMap(np.ascontiguousarray(sc["map"][keep]), np.ascontiguousarray(sc["normals"][keep]))
        rv, second = batch(icp, d)
        want = [single(icp, d, b) for b in range(4)]
        assert rv == OK
        for b in range(4):
            same(second[b], want[b])
        assert any(second[b][1] != first[b][1] for b in range(3))         # (the thinned map answers differently: the tables are new)
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 9. relocalizeVoxel
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
CHAIN = {"matcher": {"VoxelMatcher": {"voxelSizes": [1.0, 0.5]}}, "errorMinimizer": {"PlaneToPlaneErrorMinimizer": {"epsilon": 0.001}},
         "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}},
                                    {"DifferentialTransformationChecker": {"minDiffRotErr": 0.001, "minDiffTransErr": 0.001, "smoothLength": 3}}]}


def calls(icp):
    out = (C.c_int64 * 3)()
    assert icp._lib.icpmi_debug_voxel_batch_calls(icp._h, out) == OK
    return tuple(out)


def relocalize_by_hand(amd, icp, rd, rn, cand, refine):
    """the refinement start after start with transform + icpmi_register: (pose, winner index, the winner's score bits, last iterations)"""
    from norlab_icp_mapper_amd import icp as I
    n = rd.shape[0]
    scores = icp.voxelScores(rd, rn, cand, level=0)
    best = amd.rank_voxel_candidates(scores, n, 0.0)[:refine]
    refined, status, last = [], [], None
    for i in best:
        rv, Tb, st, _ = by_hand(icp, rd, rn, cand[i])
        last = dict(st)["iterations"]
        if rv != OK:
            assert rv in (3, 4, 5, 6)
            refined.append(cand[i].copy())
        else:
            T = np.array(Tb, np.uint32).view(F).reshape(4, 4).T
            refined.append(I.compose_pose(T, cand[i]))
        status.append(rv)
    refined = np.stack(refined)
    again = icp.voxelScores(rd, rn, refined, level=None)
    again.status = [a if s == 0 else s for a, s in zip(again.status, status)]
    w = amd.rank_voxel_candidates(again, n, 0.0)[0]
    return refined[w], best[w], again.scores[w].bits(), scores.bits(), last


@pytest.mark.parametrize("refine,loops", [(4, 1), (20, 2)])
def test_relocalize_voxel_is_the_refinement_by_hand(amd, refine, loops):
    from norlab_icp_mapper_amd import icp as I
    sc = lr.scene("room")
    rd, rn = bc.unmoved()
    icp = amd.ICPSequence.loadFromYaml(CHAIN)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        cand = np.stack([sr.map_frame_pose(G @ vr.POSES["start"], icp.getMapMean()).astype(F) for G in vsc.grid()])
        pose, index, score, scores, last = relocalize_by_hand(amd, icp, rd, rn, cand, refine)
        c0 = calls(icp)
        found = icp.relocalizeVoxel(rd, rn, cand, refine=refine)
        c1 = calls(icp)
        # one registration loop per chunk of 16, every start in it, no single registration
        assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (loops, refine, 0)
        assert np.array_equal(found.pose.view(np.uint32), pose.view(np.uint32)) and found.index == index
        assert found.residual.bits() == score and found.scores.bits() == scores
        assert icp.stats.iterations == last
    finally:
        icp.close()
    got = bc.host_relocalize_voxel_counted(YAML_CHAIN, sc["map"], sc["normals"], rd, rn, cand, refine=refine)
    assert got["calls"] == (loops, refine, 0)
    assert np.array_equal(got["pose"].view(np.uint32), pose.view(np.uint32)) and got["index"] == index
    assert I.VoxelScore(got["score"]).bits() == score and got["stats_iterations"] == last


def test_host_shell_batch_and_multistart(amd):
    sc = lr.scene("room")
    icp = amd.ICPSequence.loadFromYaml(CHAIN)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        ms = bc.members()
        d = Dev(ms)
        want = [single(icp, d, b) for b in range(4)]
        rd, rn = bc.unmoved()
        want_ms = [by_hand(icp, rd, rn, p) for p in bc.priors()]
    finally:
        icp.close()
    got = bc.host_voxel_batch(YAML_CHAIN, sc["map"], sc["normals"], ms)
    assert got["status"] == [w[0] for w in want] and got["iterations"] == [iterations_of(w) for w in want]
    assert [bits16(np.ascontiguousarray(T.T).ravel()) for T in got["T"]] == [w[1] for w in want]
    assert got["stats_iterations"] == iterations_of(want[-1])
    got = bc.host_voxel_batch(YAML_CHAIN, sc["map"], sc["normals"], [(rd, rn)], bc.priors())
    assert got["status"] == [w[0] for w in want_ms] and [bits16(np.ascontiguousarray(T.T).ravel()) for T in got["T"]] == [w[1] for w in want_ms]
