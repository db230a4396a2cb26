"""VoxelMatcher with a schedule of voxel sizes on the device (csrc/voxel.hip: voxel_pairs_sched_kernel; csrc/loop.hip: voxel_advance_kernel;
DESIGN.md 4.21), through the C ABI: every level's table and sums bit for bit those of a one-size handle, the scheduled registration against
the float32 restatement (iterations and pair counts per level, exactly) and the float64 loop (the pose, within four times what the float32
restatement loses against it: profiles/voxel_pyramid_tolerance.json, measured on the CPU by scripts/voxel_pyramid_tolerance.py -- never the
device's own output), the smallest shapes, the state a handle keeps across calls, the refusals and the two YAML front ends."""
import ctypes as C

import numpy as np
import pytest

import localizability_reference as lr
import plane_to_plane_reference as pr
import voxel_cases as vc
import voxel_pyramid_cases as pc
import voxel_pyramid_reference as vpr
import voxel_reference as vr

pytestmark = pytest.mark.gpu
F = np.float32
MARGIN = 4.0
OK, INVALID_ARG, NO_POINT, MISSING_NORMALS, UNSUPPORTED = 0, 1, 3, 7, 8
STOP_COUNTER, STOP_DIFFERENTIAL = 1, 2
REG = dict(max_iterations=vr.MAX_ITER, use_differential=1)
THREE = (2.0, 1.0, 0.5)
FOUR = (4.0, 2.0, 1.0, 0.5)


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def tol():
    return pc.recorded()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def make_icp(amd, sizes=None, size=None, **kw):
    kw.setdefault("minimizer", vc.MIN_PLANE_TO_PLANE)
    kw.setdefault("outliers", [])
    return amd.ICPSequence(knn=1, max_dist=2.0, voxel_sizes=None if sizes is None else list(sizes), voxel_size=size, **kw)


def room_icp(amd, sizes=None, size=None, **kw):
    icp = make_icp(amd, sizes, size, **kw)
    sc = lr.scene("room")
    assert icp.setMap(sc["map"], sc["normals"])
    return icp


def f4(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


def stats_of(icp):
    return (icp.stats.iterations, icp.stats.stop_reason, icp.stats.pairs)


# ------------------------------------------------------------------------------------------------------------------ 1. level tables
def test_level_tables_are_the_one_size_tables(amd):
    sc, rd, rn, _ = pc.registration_inputs(1)
    icp = room_icp(amd, THREE)
    try:
        assert icp.getVoxelSchedule() == list(THREE) and icp.getVoxelMatcher() == 0.5
        rc = vr.centred(rd, icp.getMapMean())
        for level, size in enumerate(THREE):
            one = room_icp(amd, size=size)
            try:
                a, b = icp.voxelMap(level), one.voxelMap()
                assert a[0].shape[0] == b[0].shape[0] > 0
                for x, y in zip(a, b):
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
                la, lb = icp.voxelLookup(rc, level), one.voxelLookup(rc)
                assert np.array_equal(la, lb) and (la >= 0).sum() == pc.reference_run(1, (size,))["levels"][0]["pairs_first"]
            finally:
                one.close()
        # the signatures without a level answer for the finest
        for x, y in zip(icp.voxelMap(), icp.voxelMap(len(THREE) - 1)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert np.array_equal(icp.voxelLookup(rc), icp.voxelLookup(rc, 2))
        nv = C.c_int64(0)
        for bad in (-1, 3, 4):
            assert icp._lib.icpmi_get_voxel_map_level(icp._h, bad, 0, None, None, None, None, C.byref(nv)) == INVALID_ARG
            assert icp._lib.icpmi_voxel_lookup_level(icp._h, bad, rc.ctypes.data, 1, np.zeros(1, np.int32).ctypes.data) == INVALID_ARG
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 2. a schedule of one
def test_a_schedule_of_one_is_set_voxel_matcher(amd):
    sc, rd, rn, _ = pc.registration_inputs(1)
    out = []
    for how in ("matcher", "schedule"):
        icp = room_icp(amd, **REG)
        try:
            if how == "matcher":
                icp.setVoxelMatcher(1.0)
            else:
                icp.setVoxelSchedule([1.0])
            assert icp.getVoxelSchedule() == [1.0] and icp.getVoxelMatcher() == 1.0
            T = icp(rd, rn)
            st = stats_of(icp)
            rc = vr.centred(rd, icp.getMapMean())
            T_step, sums = icp.minimizeStep(rc, np.eye(4, dtype=F), read_normals=rn)
            out.append((_bits(T), st, _bits(T_step), np.asarray(sums).view(np.uint64)))
            lv = C.c_int32(0)
            a = (C.c_int32 * 4)()
            assert icp._lib.icpmi_get_voxel_schedule_report(icp._h, C.byref(lv), a, a, a) == INVALID_ARG     # (no schedule of two or more)
        finally:
            icp.close()
    assert out[0][1] == out[1][1] and out[0][1][0] == pc.reference_run(1, (1.0,))["iterations"]
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ 3. per-level sums
@pytest.mark.parametrize("pose", ["true", 1, 3])
def test_sums_at_every_level_are_the_one_size_sums(amd, pose):
    sc = lr.scene("room")
    T = (np.eye(4) if pose == "true" else pc.start_pose(pose)).astype(F)
    icp = room_icp(amd, THREE)
    try:
        rc = vr.centred(sc["reading"], icp.getMapMean())
        for level, size in enumerate(THREE):
            assert icp._lib.icpmi_debug_voxel_step_level(icp._h, level) == OK
            T_step, sums = icp.minimizeStep(rc, T, read_normals=sc["reading_normals"])
            pairs = icp.stats.pairs
            one = room_icp(amd, size=size)
            try:
                T_one, sums_one = one.minimizeStep(rc, T, read_normals=sc["reading_normals"])
                assert one.stats.pairs == pairs == sums[28] > 0
            finally:
                one.close()
            print(f"pose {pose} level {level} (size {size}): {pairs} pairs")
            assert np.array_equal(np.asarray(sums).view(np.uint64), np.asarray(sums_one).view(np.uint64))
            assert np.array_equal(_bits(T_step), _bits(T_one))
        assert icp._lib.icpmi_debug_voxel_step_level(icp._h, -1) == OK    # the finest again
        T_fin, sums_fin = icp.minimizeStep(rc, T, read_normals=sc["reading_normals"])
        assert np.array_equal(np.asarray(sums_fin).view(np.uint64), np.asarray(sums).view(np.uint64))
        assert icp._lib.icpmi_debug_voxel_step_level(icp._h, 3) == INVALID_ARG
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 4. the registration
@pytest.mark.parametrize("k,sizes", pc.GPU_CASES, ids=[pc.case_key(k, s) for k, s in pc.GPU_CASES])
def test_scheduled_registration(amd, tol, k, sizes):
    sc, rd, rn, truth = pc.registration_inputs(k)
    r64, r32 = pc.reference_run(k, sizes, 64), pc.reference_run(k, sizes, 32)
    icp = room_icp(amd, sizes, **REG)
    try:
        T = icp(rd, rn)
        st, rep = stats_of(icp), icp.voxelScheduleReport()
        T2 = icp(rd, rn)
        st2, rep2 = stats_of(icp), icp.voxelScheduleReport()
    finally:
        icp.close()
    rec = tol["registration_room"][pc.case_key(k, sizes)]
    dt, dr = vc.pose_distance(T, r64["T"], rd)
    et, er = vr.centroid_error(T, truth, rd)
    print(f"x{k} {sizes}: report {rep} (float32 restatement {vpr.report(r32)}); from the float64 loop {dt:.3e} m / {dr:.3e} rad (allowed "
          f"{MARGIN * rec['float32_from_float64_trans']:.3e} / {MARGIN * rec['float32_from_float64_rot']:.3e}); to the truth {et:.3e} m / {er:.3e} rad")
    assert np.array_equal(_bits(T), _bits(T2)) and st == st2 and rep == rep2      # a second registration: level 0 again, the same bits and report
    assert rep == vpr.report(r32)
    assert st[0] == r32["iterations"] == sum(r[0] for r in rep) and st[1] == STOP_DIFFERENTIAL and st[2] == rep[-1][2]
    assert dt <= MARGIN * rec["float32_from_float64_trans"] and dr <= MARGIN * rec["float32_from_float64_rot"]
    assert abs(et - pc.FLOOR) <= pc.printed(pc.FLOOR) + MARGIN * rec["float32_from_float64_trans"]


def test_the_basin_is_wider_than_the_finest_size_alone(amd):
    """from x6 (1.8 m, 0.3 rad) both schedules end at the 0.5 m floor; a one-size 0.5 m handle from the same start does not"""
    sc, rd, rn, truth = pc.registration_inputs(6)
    for sizes in pc.WORKING:
        icp = room_icp(amd, sizes, **REG)
        try:
            et, _ = vr.centroid_error(icp(rd, rn), truth, rd)
        finally:
            icp.close()
        print(f"x6 {sizes}: {et:.3e} m to the truth")
        assert et < 1.1 * pc.FLOOR
    one = room_icp(amd, size=0.5, **REG)
    try:
        try:
            et, _ = vr.centroid_error(one(rd, rn), truth, rd)
        except amd.icp.ConvergenceError:
            et = np.inf
    finally:
        one.close()
    print(f"x6 0.5 m alone: {et:.3e} m to the truth (float64 loop: {pc.PROTOTYPE[(0.5,)][6]})")
    assert et > 1.0


# ------------------------------------------------------------------------------------------------------------------ 5. the smallest shapes
def test_reading_of_one_point(amd):
    sc, rd, rn, _ = pc.registration_inputs(1)
    icp = room_icp(amd, (1.0, 0.5), max_iterations=5, use_differential=1)
    try:
        res = []
        for _ in range(2):
            T = icp(rd[:1], rn[:1])
            res.append((_bits(T).tobytes(), stats_of(icp), tuple(icp.voxelScheduleReport())))
    finally:
        icp.close()
    (_, st, rep), _ = res
    print(f"one point: stats {st}, report {rep}")
    assert res[0] == res[1]
    assert len(rep) == 2 and all(r[1] == 1 and r[2] == 1 and 1 <= r[0] <= 5 for r in rep) and st[0] == rep[0][0] + rep[1][0] and st[2] == 1


def test_no_pair_at_the_second_level(amd):
    """every point finds a voxel at 4 m and none at 0.5 m: two clusters of the map share a coarse voxel whose mean lies in an empty fine one, and
    the reading sits around that mean (zero normals: every pair pulls towards the mean alike, the step is zero to rounding)"""
    rng = np.random.default_rng(5)
    a = rng.uniform(0.05, 0.45, (200, 3))
    pos = np.concatenate([a, a + 2.0]).astype(F)
    mp = np.concatenate([pos, -pos])                                   # (centroid exactly 0: the centred frame is the frame of the test)
    mu = pos.astype(np.float64).mean(0)
    off = rng.uniform(-0.05, 0.05, (100, 3))
    rd = f4(np.concatenate([mu + off, mu - off]))
    zeros = lambda n: np.zeros((n, 3), F)
    icp = make_icp(amd, (4.0, 0.5), **REG)
    try:
        assert icp.setMap(f4(mp), zeros(mp.shape[0]))
        assert (icp.voxelLookup(rd, 0) >= 0).all() and (icp.voxelLookup(rd, 1) == -1).all()
        with pytest.raises(amd.icp.ConvergenceError, match="no point to minimize"):
            icp(rd, zeros(rd.shape[0]))
        rep = icp.voxelScheduleReport()
        rn = zeros(rd.shape[0])
        assert icp._lib.icpmi_register(icp._h, rd.ctypes.data, rd.shape[0], rn.ctypes.data, (C.c_float * 16)(), None) == NO_POINT
    finally:
        icp.close()
    print(f"report {rep}")
    assert rep == [(3, 200, 200), (0, 0, 0)]                         # level 0 finished (three steps under the thresholds), level 1 entered and empty


def test_a_first_level_of_very_few_voxels(amd):
    """1000 m: the centred room falls into the eight voxels that meet at the origin (the fewest a cloud centred on its own mean can have); a
    map of one point has a table of one voxel at every level"""
    sc, rd, rn, _ = pc.registration_inputs(1)
    sizes = (1000.0, 0.5)
    r64, r32 = pc.reference_run(1, sizes, 64), pc.reference_run(1, sizes, 32)
    assert vpr.margins(r64, r32)[0]
    icp = room_icp(amd, sizes, **REG)
    try:
        assert icp.voxelMap(0)[0].shape[0] == 8
        T = icp(rd, rn)
        rep, its = icp.voxelScheduleReport(), icp.stats.iterations
    finally:
        icp.close()
    dt, dr = vc.pose_distance(T, r64["T"], rd)
    d32 = vc.pose_distance(r32["T"], r64["T"], rd)
    print(f"1000 m first: report {rep}; from the float64 loop {dt:.3e} m / {dr:.3e} rad (allowed {MARGIN * d32[0]:.3e} / {MARGIN * d32[1]:.3e})")
    assert rep == vpr.report(r32) and its == r32["iterations"]
    assert dt <= MARGIN * d32[0] and dr <= MARGIN * d32[1]
    one = make_icp(amd, (8.0, 0.5))
    try:
        assert one.setMap(f4([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 1.0]], F))
        assert one.voxelMap(0)[3].tolist() == [1] and one.voxelMap(1)[3].tolist() == [1]
        # three points of the one voxel's positive corner and one outside it: the same record at both levels, hence the same sums
        q = f4([[0.1, 0.1, 0.05], [0.2, 0.05, 0.3], [0.4, 0.3, 0.1], [-0.1, 0.2, 0.1]])
        qn = np.tile(np.array([[0.0, 0.0, 1.0]], F), (4, 1))
        got = []
        for level in (0, 1):
            assert one._lib.icpmi_debug_voxel_step_level(one._h, level) == OK
            assert one.voxelLookup(q, level).tolist() == [0, 0, 0, -1]
            _, sums = one.minimizeStep(q, np.eye(4, dtype=F), read_normals=qn)
            assert one.stats.pairs == 3
            got.append(np.asarray(sums).view(np.uint64))
        assert np.array_equal(got[0], got[1])
    finally:
        one.close()


def test_the_counter_advances_every_level(amd):
    sc, rd, rn, _ = pc.registration_inputs(1)
    r64 = pc.reference_run(1, FOUR, 64, max_iter=3)
    r32 = pc.reference_run(1, FOUR, 32, max_iter=3)
    icp = room_icp(amd, FOUR, max_iterations=3, use_differential=1)
    try:
        T = icp(rd, rn)
        st, rep = stats_of(icp), icp.voxelScheduleReport()
    finally:
        icp.close()
    dt, dr = vc.pose_distance(T, r64["T"], rd)
    d32 = vc.pose_distance(r32["T"], r64["T"], rd)
    print(f"maxIterationCount 3: report {rep}, stats {st}; from the float64 loop {dt:.3e} m / {dr:.3e} rad (allowed {MARGIN * d32[0]:.3e} / {MARGIN * d32[1]:.3e})")
    assert [r[0] for r in rep] == [3, 3, 3, 3] and st[0] == 12 and st[1] == STOP_COUNTER
    assert rep == vpr.report(r32)
    assert dt <= MARGIN * d32[0] and dr <= MARGIN * d32[1]


def test_fixed_iterations_run_at_every_level(amd):
    import torch
    sc, rd, rn, _ = pc.registration_inputs(1)
    r64 = pc.reference_run(1, FOUR, 64, max_iter=2, differential=None)
    r32 = pc.reference_run(1, FOUR, 32, max_iter=2, differential=None)
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()
    out = {}
    for graph in (1, 0):
        icp = room_icp(amd, FOUR, use_graph=graph)
        try:
            out[graph] = []
            for _ in range(3):                                        # capture, replay, replay
                T = icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=2, d_normals_ptr=dn.data_ptr())
                out[graph].append((_bits(T).tobytes(), stats_of(icp), tuple(icp.voxelScheduleReport())))
        finally:
            icp.close()
    first = out[0][0]
    assert all(r == first for r in out[0] + out[1])
    assert first[1][0] == 8 and [r[0] for r in first[2]] == [2, 2, 2, 2] and list(first[2]) == vpr.report(r32)
    dt, dr = vc.pose_distance(T, r64["T"], rd)
    d32 = vc.pose_distance(r32["T"], r64["T"], rd)
    print(f"2 iterations at each of 4 levels: from the float64 loop {dt:.3e} m / {dr:.3e} rad (allowed {MARGIN * d32[0]:.3e} / {MARGIN * d32[1]:.3e})")
    assert dt <= MARGIN * d32[0] and dr <= MARGIN * d32[1]


def test_four_levels_at_most(amd):
    icp = make_icp(amd, FOUR)
    try:
        set_ = lambda v: icp._lib.icpmi_set_voxel_schedule(icp._h, (C.c_float * max(1, len(v)))(*v), len(v))
        for bad in ([8.0, 4.0, 2.0, 1.0, 0.5], [0.5, 1.0], [1.0, 1.0], [1.0, float("nan")], [float("inf"), 1.0], [1.0, 0.0], [1.0, -0.5]):
            assert set_(bad) == INVALID_ARG
            assert "InvalidParameter" in icp._lib.icpmi_last_error(icp._h).decode() and "VoxelMatcher" in icp._lib.icpmi_last_error(icp._h).decode()
            assert icp.getVoxelSchedule() == list(FOUR)                # the schedule stays
        assert icp._lib.icpmi_set_voxel_schedule(icp._h, None, 2) == INVALID_ARG and icp._lib.icpmi_set_voxel_schedule(icp._h, None, -1) == INVALID_ARG
        assert set_([4.0, 2.0, 1.0]) == OK and icp.getVoxelSchedule() == [4.0, 2.0, 1.0] and icp.getVoxelMatcher() == 1.0
        icp.setVoxelMatcher(0.25)
        assert icp.getVoxelSchedule() == [0.25]
        assert icp._lib.icpmi_set_voxel_schedule(icp._h, None, 0) == OK and icp.getVoxelSchedule() == [] and icp.getVoxelMatcher() == 0.0
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 6. state across calls
def test_schedule_change_reaches_a_cached_graph(amd):
    import torch
    sc, rd, rn, _ = pc.registration_inputs(1)
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()

    def run(icp):
        T = icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=2, d_normals_ptr=dn.data_ptr())
        return _bits(T).tobytes(), tuple(icp.voxelScheduleReport())

    def fresh(sizes):
        f = room_icp(amd, sizes)
        try:
            return run(f)
        finally:
            f.close()

    icp = room_icp(amd, (1.0, 0.5))
    try:
        a0, a1 = run(icp), run(icp)                                   # the second call replays the graph
        icp.setVoxelSchedule([2.0, 0.5])                              # the same count with another size
        b0, b1 = run(icp), run(icp)
        icp.setVoxelSchedule([2.0, 1.0, 0.5])                         # another count
        c0, c1 = run(icp), run(icp)
        icp.setVoxelSchedule([1.0, 0.5])
        a2 = run(icp)
    finally:
        icp.close()
    assert a0 == a1 == a2 == fresh((1.0, 0.5))
    assert b0 == b1 == fresh((2.0, 0.5))
    assert c0 == c1 == fresh((2.0, 1.0, 0.5))
    assert len({a0[0], b0[0], c0[0]}) == 3 and len(c0[1]) == 3


def test_a_shorter_schedule_gives_levels_back_and_a_longer_one_builds_them_again(amd):
    sc, rd, rn, _ = pc.registration_inputs(3)
    icp = room_icp(amd, FOUR, **REG)
    try:
        first = (_bits(icp(rd, rn)).tobytes(), tuple(icp.voxelScheduleReport()))
        icp.setVoxelSchedule([0.5])                                   # levels 1 to 3 are dropped, level 0 gets another size
        assert icp._lib.icpmi_get_voxel_map_level(icp._h, 1, 0, None, None, None, None, C.byref(C.c_int64(0))) == INVALID_ARG
        icp.setVoxelSchedule([1.0, 0.5])
        two = (_bits(icp(rd, rn)).tobytes(), tuple(icp.voxelScheduleReport()))
        icp.setVoxelSchedule(list(FOUR))
        again = (_bits(icp(rd, rn)).tobytes(), tuple(icp.voxelScheduleReport()))
    finally:
        icp.close()
    f = room_icp(amd, (1.0, 0.5), **REG)
    try:
        want_two = (_bits(f(rd, rn)).tobytes(), tuple(f.voxelScheduleReport()))
    finally:
        f.close()
    assert first == again and list(first[1]) == vpr.report(pc.reference_run(3, FOUR, 32))
    assert two == want_two and list(two[1]) == vpr.report(pc.reference_run(3, (1.0, 0.5), 32))


def test_a_new_map_rebuilds_every_level(amd):
    room, corridor = lr.scene("room"), lr.scene("corridor")
    icp = room_icp(amd, THREE)
    try:
        before = [icp.voxelMap(l) for l in range(3)]
        assert icp.setMap(corridor["map"], corridor["normals"])
        after = [icp.voxelMap(l) for l in range(3)]
        T = icp(corridor["reading"], corridor["reading_normals"])
        rep = icp.voxelScheduleReport()
    finally:
        icp.close()
    for level, size in enumerate(THREE):
        one = make_icp(amd, size=size)
        try:
            assert one.setMap(corridor["map"], corridor["normals"])
            want = one.voxelMap()
        finally:
            one.close()
        assert before[level][0].shape != after[level][0].shape or not np.array_equal(before[level][1], after[level][1])
        for x, y in zip(after[level], want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    f = make_icp(amd, THREE)
    try:
        assert f.setMap(corridor["map"], corridor["normals"])
        T_f = f(corridor["reading"], corridor["reading_normals"])
        assert f.voxelScheduleReport() == rep
    finally:
        f.close()
    assert np.array_equal(_bits(T), _bits(T_f))


def test_an_empty_schedule_is_the_nearest_neighbour_path(amd):
    sc, rd, rn, _ = pc.registration_inputs(1)
    out = []
    for touch in (False, True):
        icp = amd.ICPSequence(knn=1, max_dist=2.0, minimizer=vc.MIN_PLANE_TO_PLANE, outliers=[], **REG)
        try:
            assert icp.setMap(sc["map"], sc["normals"])
            if touch:
                icp.setVoxelSchedule(list(FOUR))
                icp(rd, rn)
                assert icp._lib.icpmi_set_voxel_schedule(icp._h, None, 0) == OK
            T = icp(rd, rn)
            rc = vr.centred(rd, icp.getMapMean())
            T_step, sums = icp.minimizeStep(rc, np.eye(4, dtype=F), read_normals=rn)
            out.append((_bits(T), stats_of(icp), _bits(T_step), np.asarray(sums).view(np.uint64)))
        finally:
            icp.close()
    assert out[0][1] == out[1][1]
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def _refused(icp, st, code, *words):
    msg = icp._lib.icpmi_last_error(icp._h).decode()
    assert st == code, (st, msg)
    for w in ("voxel matcher",) + words:
        assert w in msg, msg


def _capi_stats():
    from norlab_icp_mapper_amd import _capi
    return _capi.Stats()


@pytest.mark.parametrize("what,kw,word", [
    ("point-to-plane", dict(minimizer=2), "PlaneToPlaneErrorMinimizer only"),
    ("point-to-point", dict(minimizer=1), "PlaneToPlaneErrorMinimizer only"),
    ("identity", dict(minimizer=0), "PlaneToPlaneErrorMinimizer only"),
    ("symmetric", dict(plane_model="symmetric"), "symmetric pair model"),
    ("maxdist filter", dict(outliers=[(1, 2.0)]), "outlier filters"),
    ("trimmed filter", dict(outliers=[(4, 0.85)]), "outlier filters"),
    ("var_dist", dict(var_dist=1), "KDTreeVarDistMatcher"),
    ("covariance", dict(minimizer=2, covariance=1), "PlaneToPlaneErrorMinimizer only"),
    ("degeneracy_threshold", dict(minimizer=2, degeneracy_threshold=0.005), "PlaneToPlaneErrorMinimizer only"),
    ("force_2d", dict(minimizer=2, force_2d=1), "PlaneToPlaneErrorMinimizer only"),
])
def test_refused_combinations(amd, what, kw, word):
    sc, rd, rn, _ = pc.registration_inputs(1)
    icp = room_icp(amd, (1.0, 0.5), **kw)
    try:
        T, st = (C.c_float * 16)(), _capi_stats()
        _refused(icp, icp._lib.icpmi_register(icp._h, rd.ctypes.data, rd.shape[0], rn.ctypes.data, T, C.byref(st)), INVALID_ARG, word)
        rc = vr.centred(rd, icp.getMapMean())
        sums = (C.c_double * 32)()
        _refused(icp, icp._lib.icpmi_minimize_step_normals(icp._h, rc.ctypes.data, rc.shape[0], rn.ctypes.data, None, T, sums, C.byref(st)), INVALID_ARG, word)
    finally:
        icp.close()


def test_intensity_weight_is_refused(amd):
    sc, rd, rn, _ = pc.registration_inputs(1)
    icp = room_icp(amd, (1.0, 0.5))
    try:
        assert icp._lib.icpmi_set_intensity_weight(icp._h, C.c_float(0.1)) == OK
        _refused(icp, icp._lib.icpmi_register(icp._h, rd.ctypes.data, rd.shape[0], rn.ctypes.data, (C.c_float * 16)(), None), INVALID_ARG, "intensity")
    finally:
        icp.close()


def test_entry_points_that_do_not_serve_it(amd):
    import torch
    sc, rd, rn, _ = pc.registration_inputs(1)
    icp = room_icp(amd, (1.0, 0.5))
    try:
        lib, h = icp._lib, icp._h
        d = torch.from_numpy(rd).cuda()
        T, st, status = (C.c_float * 32)(), (_capi_stats().__class__ * 2)(), (C.c_int * 2)()
        ptrs, ns = (C.c_void_p * 1)(d.data_ptr()), (C.c_int64 * 1)(rd.shape[0])
        _refused(icp, lib.icpmi_register_batch_dev(h, 1, ptrs, ns, 2, T, st, status), UNSUPPORTED, "register_batch")
        prior = np.ascontiguousarray(np.eye(4, dtype=F).T).ravel()
        _refused(icp, lib.icpmi_register_multistart(h, rd.ctypes.data, rd.shape[0], prior.ctypes.data, 1, 2, T, st, status), UNSUPPORTED, "register_multistart")
        _refused(icp, lib.icpmi_register_multistart_dev(h, d.data_ptr(), rd.shape[0], prior.ctypes.data, 1, 2, T, st, status), UNSUPPORTED, "register_multistart")
        rc = vr.centred(rd, icp.getMapMean())
        _refused(icp, lib.icpmi_minimize_step(h, rc.ctypes.data, rc.shape[0], None, T, (C.c_double * 32)(), None), UNSUPPORTED, "minimize_step")
        t = np.zeros(rd.shape[0], F)
        for call in (lambda: icp.register_sweep(rd, t, np.eye(4), np.eye(4)), lambda: icp.sweep_sums(rd, t, np.eye(4), np.eye(4)),
                     lambda: icp.register_sweep_dev(d.data_ptr(), rd.shape[0], torch.from_numpy(t).cuda().data_ptr(), np.eye(4), np.eye(4))):
            with pytest.raises(NotImplementedError, match="voxel matcher"):
                call()
        assert lib.icpmi_register(h, rd.ctypes.data, rd.shape[0], None, T, None) == MISSING_NORMALS
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 8. host shell and Python
YAML_CHAIN = """matcher:
  VoxelMatcher:
    voxelSizes: [4.0, 2.0, 1.0, 0.5]
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


def cpp_register(yaml_icp, map4, map_normals, scan4, scan_normals):
    """nim_test_icp_register_voxel_schedule (host/TestHooksVoxelSchedule.cpp): (T (4, 4), Stats, report) through GpuICPSequence"""
    import host_bindings as hb
    from norlab_icp_mapper_amd import _capi
    fn = hb.load().nim_test_icp_register_voxel_schedule
    fn.restype = C.c_int
    arr = lambda a: np.ascontiguousarray(a, dtype=F)
    mp, mn, sc, sn = arr(map4), arr(map_normals), arr(scan4), arr(scan_normals)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    T, stats, err = np.zeros(16, F), _capi.Stats(), C.create_string_buffer(512)
    lv, it, pf, pl = C.c_int(0), (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
    if fn(yaml_icp.encode(), ptr(mp), C.c_int64(mp.shape[0]), ptr(mn), ptr(sc), C.c_int64(sc.shape[0]), ptr(sn), ptr(T), C.byref(stats), C.byref(lv), it, pf, pl,
          err, C.c_int(512)):
        raise RuntimeError(err.value.decode(errors="replace"))
    return T.reshape(4, 4).T.copy(), stats, [(it[i], pf[i], pl[i]) for i in range(lv.value)]


def test_yaml_front_ends_give_the_c_calls_bits(amd):
    sc, rd, rn, _ = pc.registration_inputs(3)
    direct = room_icp(amd, **REG)
    try:
        sizes = (C.c_float * 4)(*FOUR)
        assert direct._lib.icpmi_set_voxel_schedule(direct._h, sizes, 4) == OK
        T = direct(rd, rn)
        its, rep = direct.stats.iterations, direct.voxelScheduleReport()
    finally:
        direct.close()
    assert rep == vpr.report(pc.reference_run(3, FOUR, 32))
    chain = {"matcher": {"VoxelMatcher": {"voxelSizes": list(FOUR)}}, "errorMinimizer": {"PlaneToPlaneErrorMinimizer": {"epsilon": 0.001}},
             "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}},
                                        {"DifferentialTransformationChecker": {"minDiffRotErr": 0.001, "minDiffTransErr": 0.001, "smoothLength": 3}}]}
    py = amd.ICPSequence.loadFromYaml(chain)
    try:
        assert py.getVoxelSchedule() == list(FOUR) and py.getVoxelMatcher() == 0.5
        py.setMap(sc["map"], sc["normals"])
        T_py = py(rd, rn)
        assert py.voxelScheduleReport() == rep and py.stats.iterations == its
    finally:
        py.close()
    T_cpp, stats, rep_cpp = cpp_register(YAML_CHAIN, sc["map"], sc["normals"], rd, rn)
    assert np.array_equal(_bits(T_py), _bits(T))
    assert np.array_equal(_bits(T_cpp), _bits(T)) and stats.iterations == its and rep_cpp == rep
    for bad, word in (("voxelSizes: [0.5, 1.0]", "strictly descending"), ("voxelSizes: [1.0, 1.0]", "strictly descending"), ("voxelSizes: []", "1 to 4"),
                      ("voxelSizes: [8.0, 4.0, 2.0, 1.0, 0.5]", "1 to 4"), ("voxelSizes: [.inf, 1.0]", "finite and > 0"),
                      ("voxelSizes: [1.0, 0.5]\n    voxelSize: 0.5", "voxelSize and voxelSizes")):
        with pytest.raises(RuntimeError, match=word):
            cpp_register(YAML_CHAIN.replace("voxelSizes: [4.0, 2.0, 1.0, 0.5]", bad), sc["map"], sc["normals"], rd, rn)
    with pytest.raises(RuntimeError, match="voxel matcher.*outlier filters"):
        cpp_register(YAML_CHAIN + "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n", sc["map"], sc["normals"], rd, rn)
    for bad, word in (([0.5, 1.0], "strictly descending"), ([], "1 to 4"), ([8.0, 4.0, 2.0, 1.0, 0.5], "1 to 4"), ([float("inf"), 1.0], "finite and > 0")):
        with pytest.raises(amd.icp.InvalidParameter, match=word):
            amd.ICPSequence.loadFromYaml({**chain, "matcher": {"VoxelMatcher": {"voxelSizes": bad}}})
