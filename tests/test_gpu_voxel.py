"""VoxelMatcher on the device (csrc/voxel.hip), through the C ABI: the table of the resident map voxel by voxel against the float64 reference
(tests/voxel_reference.py), icpmi_voxel_lookup bit for bit against a numpy float32 floor, the pair sums and the step of
icpmi_minimize_step_normals against the reference evaluated on the pairs the lookup returns, registrations against the float64 loop, and
the behaviour around the path.  Tolerances: one float rounding for the table; for sums, step and pose four times what the float32
restatement loses against float64 on the same inputs (profiles/voxel_tolerance.json, measured on the CPU by scripts/voxel_tolerance.py) --
never the device's own output."""
import ctypes as C

import numpy as np
import pytest

import localizability_reference as lr
import plane_to_plane_cases as pc
import plane_to_plane_reference as pr
import voxel_cases as vc
import voxel_reference as vr

pytestmark = pytest.mark.gpu
F = np.float32
MARGIN = 4.0
U = 2.0 ** -23
SORT_TILE = 2048            # elements per workgroup of radix_sort_pairs (octree.hip: ICPMI_RS_EPB)
OK, INVALID_ARG, NO_POINT, MISSING_NORMALS, UNSUPPORTED = 0, 1, 3, 7, 8


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def tol():
    return vc.recorded()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def make_icp(amd, size, **kw):
    kw.setdefault("minimizer", vc.MIN_PLANE_TO_PLANE)
    kw.setdefault("outliers", [])
    return amd.ICPSequence(knn=1, max_dist=2.0, voxel_size=size, **kw)


def f4(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


def mirrored(xyz):
    """the points and their mirror images: the centroid is exactly 0, so the handle's centred frame is the frame of the test"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, -xyz])


def check_table(icp, map4, normals, size):
    """the device's table against the float64 reference of the map as the handle centres it; returns (reference, device arrays)"""
    mc = vr.centred(map4, icp.getMapMean())
    ref = vr.table(mc, normals, size)
    ijk, mean, mom, cnt = icp.voxelMap()
    assert np.array_equal(vr.pack_keys(ijk), ref["keys"]) and np.array_equal(ijk, ref["ijk"])
    assert np.array_equal(cnt, ref["count"])
    dmu = np.abs(mean.astype(np.float64) - ref["mu"]).max(1)
    dN = np.abs(mom.astype(np.float64) - ref["N"]).max()
    print(f"{ref['keys'].size} voxels of {mc.shape[0]} points: max |mu| error / bound {np.max(dmu / (U * np.maximum(ref['max_abs'], 1e-30))):.3f}, max |N| error {dN:.3e} (allowed {U:.3e})")
    assert (dmu <= U * ref["max_abs"]).all()
    assert dN <= U
    return ref, (ijk, mean, mom, cnt)


def random_cloud(rng, m, extent=4.0):
    pts = rng.uniform(-extent, extent, (m, 3)).astype(F)
    nrm = rng.normal(size=(m, 3)).astype(F)
    return f4(pts), nrm


# ------------------------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 5000])
def test_table_against_float64(amd, m):
    rng = np.random.default_rng(100 + m)
    map4, nrm = random_cloud(rng, m)
    icp = make_icp(amd, 1.0)
    try:
        assert icp.getVoxelMatcher() == 1.0
        assert icp.setMap(map4, nrm)
        check_table(icp, map4, nrm, 1.0)
    finally:
        icp.close()


def test_table_occupancies(amd):
    rng = np.random.default_rng(5)
    size = 0.5
    cases = {
        # (the handle centres the map on its centroid: two DIFFERENT points straddle it on some axis, so two points share a voxel only at
        # one position -- their normals differ; and a cluster stays inside one voxel with its mirror image as a counterweight)
        "two points, one voxel": np.array([[0.1, 0.1, 0.1], [0.1, 0.1, 0.1]], F),
        "two points, two voxels": np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1]], F),
        "5000 points, one voxel": mirrored(rng.uniform(0.01, 0.49, (5000, 3))),
        "every point in a voxel of its own": ((np.stack(np.meshgrid(*[np.arange(-6, 6)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) * size).astype(F),
    }
    for what, pts in cases.items():
        map4, nrm = f4(pts), rng.normal(size=pts.shape).astype(F)
        icp = make_icp(amd, size)
        try:
            assert icp.setMap(map4, nrm)
            ref, _ = check_table(icp, map4, nrm, size)
            print(what, "->", ref["keys"].size, "voxels")
            if what.startswith("two points"):
                assert ref["keys"].size == (1 if what.endswith("one voxel") else 2)
            if what == "5000 points, one voxel":
                assert ref["keys"].size == 2 and ref["count"].tolist() == [5000, 5000]   # runs longer than any workgroup
            if what == "every point in a voxel of its own":
                assert ref["keys"].size == pts.shape[0]
        finally:
            icp.close()


def test_key_edges(amd):
    size = 0.5
    # negative coordinates and points exactly on voxel faces (size 0.5: the faces are representable); mirrored: the centroid is exactly 0
    pts = mirrored([[-0.125, 0.25, 0.375], [0.5, 0.5, 0.5], [1.0, -0.5, 0.0], [0.0, 0.0, 1.5], [0.49999997, 0.0, 0.0], [2.0, 2.0, -2.0]])
    nrm = np.tile(np.array([[0, 0, 1]], F), (pts.shape[0], 1))
    icp = make_icp(amd, size)
    try:
        assert icp.setMap(f4(pts), nrm)
        assert np.array_equal(icp.getMapMean(), np.zeros(3, F))
        ref, (ijk, _, _, _) = check_table(icp, f4(pts), nrm, size)
        have = {tuple(r) for r in ijk.tolist()}
        assert (-1, 0, 0) in have            # x = -0.25 size gives index -1, not 0
        assert (1, 1, 1) in have and (-1, -1, -1) in have and (2, -1, 0) in have and (-2, 1, 0) in have and (0, 0, 3) in have and (0, 0, -3) in have
        # the lookup agrees on the faces: a query on a face belongs to the voxel above it
        q = np.array([[0.5, 0.5, 0.5], [-0.5, -0.5, -0.5], [0.49999997, 0.0, 0.0], [-0.125, 0.25, 0.375]], F)
        got = icp.voxelLookup(q)
        assert np.array_equal(got, vr.lookup(ref, q)) and (got >= 0).all()
        assert ijk[got[0]].tolist() == [1, 1, 1] and ijk[got[1]].tolist() == [-1, -1, -1] and ijk[got[2]].tolist() == [0, 0, 0]
    finally:
        icp.close()


def test_key_range(amd):
    size = 0.5
    edge = (2 ** 20 - 1) * size                                    # index 2^20 - 1 and its mirror image -(2^20 - 1): accepted
    ok = mirrored([[edge, 0.25, 0.25], [0.25, edge, 0.25], [0.25, 0.25, edge]])
    nrm = np.tile(np.array([[1, 0, 0]], F), (ok.shape[0], 1))
    icp = make_icp(amd, size)
    try:
        assert icp.setMap(f4(ok), nrm)
        assert np.array_equal(icp.getMapMean(), np.zeros(3, F))
        ref, (ijk, _, _, _) = check_table(icp, f4(ok), nrm, size)
        assert ijk.max() == 2 ** 20 - 1 and ijk.min() == -(2 ** 20 - 1)
        q = np.array([[edge, 0.25, 0.25], [edge + 0.5, 0.25, 0.25], [-edge - 0.5, 0.25, 0.25], [np.nan, 0, 0], [0, np.inf, 0], [3e38, 0, 0]], F)
        assert icp.voxelLookup(q).tolist() == [int(vr.lookup(ref, q[:1])[0]), -1, -1, -1, -1, -1]
        bad = mirrored([[2 ** 20 * size, 0.25, 0.25]])             # index 2^20: refused
        assert icp.setMap(f4(bad), nrm[:2])
        with pytest.raises(amd.icp.InvalidParameter, match="voxel matcher: a map point"):
            icp.voxelMap()
        st = icp._lib.icpmi_voxel_lookup(icp._h, f4(q).ctypes.data, 1, np.zeros(1, np.int32).ctypes.data)
        assert st == INVALID_ARG
    finally:
        icp.close()


def test_zero_and_non_finite_normals(amd):
    rng = np.random.default_rng(11)
    map4, nrm = random_cloud(rng, 600, extent=2.0)
    nrm[::3] = 0
    nrm[1::7] = np.nan
    nrm[2::11, 0] = np.inf
    nrm[5::13] *= F(1e-25)                                           # (a squared length that underflows to 0 in float32: no surface model)
    icp = make_icp(amd, 1.0)
    try:
        assert icp.setMap(map4, nrm)
        ref, (_, _, mom, _) = check_table(icp, map4, nrm, 1.0)
        assert np.isfinite(mom).all() and (ref["N"][:, [0, 3, 5]].sum(1) < 1 - 1e-3).any()   # the bad normals pull towards "no surface model"
    finally:
        icp.close()


def colliding_points(nv, cap):
    """centres of nv distinct unit voxels whose keys all start in the last two slots of a table of `cap` slots, and which sum to exactly 0
    (so that the handle's centred frame is this one): nv - 1 drawn from the voxels that hash there, the last one fixed by the sum"""
    cand = np.stack(np.meshgrid(*[np.arange(-40, 40)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pool = cand[vr.first_slot(vr.pack_keys(cand), cap) >= cap - 2]
    rng = np.random.default_rng(3)
    for _ in range(10000):
        v = pool[rng.choice(pool.shape[0], nv - 1, replace=False)]
        last = -(nv // 2) - v.sum(0)                                 # sum over all nv of (v + 0.5) = 0
        if np.abs(last).max() < 1000 and vr.first_slot(vr.pack_keys(last[None]), cap)[0] >= cap - 2 and not (v == last).all(1).any():
            return (np.concatenate([v, last[None]]) + 0.5).astype(F)
    raise AssertionError("no colliding key set found")


def test_colliding_keys_that_wrap_the_table(amd):
    """voxels whose probe sequences all start in the last two slots of the table: every one but the first two is pushed on, around the
    table's end.  The key set is built in the centred frame itself (the points sum to 0: centroid exactly 0)"""
    size, nv = 1.0, 16
    cap = vr.capacity_of(nv)
    pts = colliding_points(nv, cap)
    nrm = np.tile(np.array([[0, 1, 0]], F), (pts.shape[0], 1))
    icp = make_icp(amd, size)
    try:
        assert icp.setMap(f4(pts), nrm)
        assert np.array_equal(icp.getMapMean(), np.zeros(3, F))
        ref, _ = check_table(icp, f4(pts), nrm, size)
        assert ref["keys"].size == nv and (vr.first_slot(ref["keys"], cap) >= cap - 2).all()
        assert np.array_equal(icp.voxelLookup(pts), ref["of"])          # every voxel is found, wherever it landed
        assert (icp.voxelLookup((pts + F(200.0)).astype(F)) == -1).all()
    finally:
        icp.close()


def test_two_builds_are_bit_equal_and_the_table_follows_map_and_size(amd):
    rng = np.random.default_rng(21)
    map4, nrm = random_cloud(rng, 3000)
    other4, other_n = random_cloud(rng, 1700)
    out = []
    for _ in range(2):
        icp = make_icp(amd, 1.0)
        assert icp.setMap(map4, nrm)
        out.append(icp.voxelMap())
        if len(out) == 2:
            assert icp.setMap(other4, other_n)                     # rebuilt after icpmi_set_map ...
            check_table(icp, other4, other_n, 1.0)
            icp.setVoxelMatcher(0.5)                               # ... and after a change of size
            ref, _ = check_table(icp, other4, other_n, 0.5)
            assert np.array_equal(icp.voxelLookup(vr.centred(other4, icp.getMapMean())), ref["of"])
            assert icp.setMap(map4, nrm)
            icp.setVoxelMatcher(1.0)
            out.append(icp.voxelMap())
        icp.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)
    for a, b in zip(out[0], out[2]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)


def test_table_follows_a_map_update(amd):
    """an append through the resident-map update (the incremental insert) and a second one invalidate the table: the next call that needs
    it sees the grown map"""
    sc = lr.scene("room")
    base, nb = sc["map"][:5000].copy(), sc["normals"][:5000].copy()
    icp = make_icp(amd, 1.0)
    try:
        assert icp.setMap(base, nb)
        ref0, _ = check_table(icp, base, nb, 1.0)
        cur, curn, lo = base, nb, 5000
        for hi in (6500, 8000):
            delta, dn = sc["map"][lo:hi].copy(), sc["normals"][lo:hi].copy()
            app, new_m = icp.mapUpdatePointDistance(delta, 0.0, normals_knn=0, scan_normals=dn)
            cur, curn, lo = np.concatenate([cur, delta]), np.concatenate([curn, dn]), hi
            assert app == delta.shape[0] and new_m == cur.shape[0]
            ref, _ = check_table(icp, cur, curn, 1.0)
            assert ref["count"].sum() == cur.shape[0] > ref0["count"].sum()
            assert np.array_equal(icp.voxelLookup(vr.centred(cur, icp.getMapMean())), ref["of"])
        assert icp.debugCounters()[18] & 0xffffffff >= 1            # (builds served by map_insert: at least one of the two appends)
    finally:
        icp.close()


def test_build_and_lookup_diagnostics(amd):
    """icpmi_debug_voxel_build_times / icpmi_debug_voxel_lookup_times (scripts/voxel_bench.py): the rebuilt table is the table, and the binary
    search over the sorted keys answers every query as the table does"""
    rng = np.random.default_rng(8)
    map4, nrm = random_cloud(rng, 3000)
    icp = make_icp(amd, 0.5)
    try:
        assert icp.setMap(map4, nrm)
        before = icp.voxelMap()
        t = (C.c_float * 3)()
        assert icp._lib.icpmi_debug_voxel_build_times(icp._h, t) == OK and all(v > 0 for v in t)
        for a, b in zip(before, icp.voxelMap()):
            assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)
        q = f4(rng.uniform(-4.5, 4.5, (1000, 3)))
        q[5, 0], q[6, 1] = np.nan, 3e38
        ms, bad = (C.c_float * 2)(), C.c_int64(-1)
        assert icp._lib.icpmi_debug_voxel_lookup_times(icp._h, q.ctypes.data, q.shape[0], 2, ms, C.byref(bad)) == OK
        assert bad.value == 0 and ms[0] > 0 and ms[1] > 0
        assert icp._lib.icpmi_debug_voxel_lookup_times(icp._h, None, 10, 2, ms, None) == INVALID_ARG
    finally:
        icp.close()


def test_table_needs_a_size_and_normals(amd):
    rng = np.random.default_rng(2)
    map4, nrm = random_cloud(rng, 300)
    icp = make_icp(amd, 0.0)
    try:
        assert icp.setMap(map4, nrm)
        with pytest.raises(amd.icp.InvalidParameter, match="no voxel size set"):
            icp.voxelMap()
        with pytest.raises(amd.icp.InvalidParameter, match="finite and >= 0"):
            icp.setVoxelMatcher(-1.0)
        assert icp.getVoxelMatcher() == 0.0
        icp.setVoxelMatcher(1.0)
        icp.setConfig(minimizer=2, knn=1, max_dist=2.0)           # the size is state of the handle: icpmi_set_config leaves it
        assert icp.getVoxelMatcher() == 1.0
        assert icp.setMap(map4, None)
        with pytest.raises(amd.icp.InvalidField, match="VoxelMatcher needs the descriptor 'normals' on the map"):
            icp.voxelMap()
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 2. icpmi_voxel_lookup
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_lookup_is_the_float32_floor(amd, n):
    rng = np.random.default_rng(40 + n)
    map4, nrm = random_cloud(rng, 4000)
    icp = make_icp(amd, 0.5)
    try:
        assert icp.setMap(map4, nrm)
        mc = vr.centred(map4, icp.getMapMean())
        ref = vr.table(mc, nrm, 0.5)
        q = rng.uniform(-4.5, 4.5, (n, 3)).astype(F)                # in occupied and in empty voxels
        q[::5] = (np.round(q[::5] * 2) / 2).astype(F)                # on faces
        if n >= 63:
            q[3], q[7, 1], q[11, 2], q[13, 0] = np.nan, np.inf, -3e38, 2 ** 20 * 0.5
        got, want = icp.voxelLookup(q), vr.lookup(ref, q)
        assert np.array_equal(got, want)
        if n >= 63:
            assert (got[[3, 7, 11, 13]] == -1).all() and (got >= 0).any() and (got == -1).sum() > 4
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 3. sums and step
def device_case(amd, name, pose, size, variant):
    """(T_step, device sums, float64 reference sums on the pairs the device's lookup returns, stats.pairs)"""
    sc = lr.scene(name)
    icp = make_icp(amd, size)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        c = vc.sum_inputs(name, pose, size, variant, mean=icp.getMapMean())
        check_table(icp, sc["map"], sc["normals"], size)
        vox = icp.voxelLookup(c["p"])
        assert np.array_equal(vox, c["vox"])                         # (the float32 key of the float32 point: bit for bit numpy's)
        T_step, sums = icp.minimizeStep(c["rc"], c["T"], read_normals=c["rn"])
        pairs = icp.stats.pairs
    finally:
        icp.close()
    return T_step, sums, vr.reference_sums(c["p"], c["npr"], vox, c["tab"]), pairs


@pytest.mark.parametrize("name,pose,size,variant", vc.SUM_CASES)
def test_sums_and_step_against_float64(amd, tol, name, pose, size, variant):
    T_step, sums, ref, pairs = device_case(amd, name, pose, size, variant)
    bound = MARGIN * tol["rel_sums"][vc.case_key(name, pose, size, variant)]
    d = pr.rel_distance(sums, ref)
    print(f"{name} {pose} {size} {variant}: rel distance {d:.3e} (allowed {bound:.3e}), pairs {int(sums[28])}")
    assert sums[28] == ref[28] == pairs and sums[27] == ref[27] and ref[28] > 0
    assert (sums[29:] == 0).all()
    assert d <= bound
    if variant == "full":                                            # the step is the float64 solve of the device's own sums
        x64, x = pr.solve_step(sums), lr.step_from_T(T_step)
        rel = float(np.linalg.norm(x - x64) / np.linalg.norm(x64))
        print(f"   step: |x - x64| / |x64| = {rel:.3e} (allowed {MARGIN * tol['max_rel_step']:.3e})")
        assert rel <= MARGIN * tol["max_rel_step"]


def test_reading_with_no_pair(amd):
    sc = lr.scene("room")
    icp = make_icp(amd, 0.5)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        rc = vr.centred(sc["reading"], icp.getMapMean())
        rc[:, :3] += F(500.0)
        rc[0, 0], rc[1, 1] = np.nan, 3e38
        assert (icp.voxelLookup(rc) == -1).all()
        with pytest.raises(amd.icp.ConvergenceError):
            icp.minimizeStep(rc, np.eye(4, dtype=F), read_normals=sc["reading_normals"])
        far = sc["reading"].copy()
        far[:, :3] += F(500.0)
        with pytest.raises(amd.icp.ConvergenceError, match="no point to minimize"):     # as the loop reports it
            icp(far, sc["reading_normals"])
        assert icp._lib.icpmi_register(icp._h, far.ctypes.data, far.shape[0], sc["reading_normals"].ctypes.data, (C.c_float * 16)(), None) == NO_POINT
        # an empty reading, with and without a normals array, on the host and on the device entry points: the same answer, nothing launched on it
        import torch
        T, dn = (C.c_float * 16)(), torch.zeros((1, 3), dtype=torch.float32, device="cuda")
        for nptr in (None, sc["reading_normals"].ctypes.data):
            assert icp._lib.icpmi_register(icp._h, far.ctypes.data, 0, nptr, T, None) == NO_POINT
        for nptr in (None, dn.data_ptr()):
            assert icp._lib.icpmi_register_dev(icp._h, None, 0, nptr, T, None) == NO_POINT
            assert icp._lib.icpmi_register_fixed_dev(icp._h, None, 0, nptr, 3, T, None) == NO_POINT
        with pytest.raises(amd.icp.ConvergenceError, match="no point to minimize"):
            icp(np.zeros((0, 4), F))
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 4. registration
REG = dict(max_iterations=vr.MAX_ITER, use_differential=1)


@pytest.mark.parametrize("size", vc.REG_SIZES)
def test_registration_against_the_float64_loop(amd, tol, size):
    sc, rd, rn, truth = vc.registration_inputs()
    icp = make_icp(amd, size, **REG)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        T = icp(rd, rn)
        its, pairs = icp.stats.iterations, icp.stats.pairs
        T2 = icp(rd, rn)
        ref = vr.register(sc["map"], sc["normals"], rd, rn, size, 64, mean=icp.getMapMean())
    finally:
        icp.close()
    rec = tol["registration_room"][str(size)]
    dt, dr = vc.pose_distance(T, ref["T"], rd)
    et, er = vr.centroid_error(T, truth, rd)
    print(f"size {size}: {its} iterations (float64 loop {ref['iterations']}), {pairs} pairs; from the float64 loop {dt:.3e} m / {dr:.3e} rad "
          f"(allowed {MARGIN * rec['float32_from_float64_trans']:.3e} / {MARGIN * rec['float32_from_float64_rot']:.3e}); to the truth {et:.3e} m / {er:.3e} rad")
    assert np.array_equal(_bits(T), _bits(T2))                       # two registrations give the same bits
    assert icp.stats.stop_reason == 2 and its == ref["iterations"]
    assert dt <= MARGIN * rec["float32_from_float64_trans"] and dr <= MARGIN * rec["float32_from_float64_rot"]


# ------------------------------------------------------------------------------------------------------------------ 5. around the path
def test_graph_replay_is_the_eager_run(amd):
    import torch
    sc, rd, rn, _ = vc.registration_inputs()
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()
    out = {}
    for graph in (1, 0):
        icp = make_icp(amd, 1.0, use_graph=graph)
        icp.setMap(sc["map"], sc["normals"])
        out[graph] = [icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=5, d_normals_ptr=dn.data_ptr()) for _ in range(3)]   # capture, replay, replay
        assert icp.stats.iterations == 5 and icp.stats.pairs > 1500
        icp.close()
    for T in out[1] + out[0]:
        assert np.array_equal(_bits(T), _bits(out[0][0]))


def test_size_change_reaches_a_cached_graph(amd):
    import torch
    sc, rd, rn, _ = vc.registration_inputs()
    d, dn = torch.from_numpy(rd).cuda(), torch.from_numpy(rn).cuda()
    run = lambda icp: icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=2, d_normals_ptr=dn.data_ptr())
    icp = make_icp(amd, 1.0)
    icp.setMap(sc["map"], sc["normals"])
    a0, a1 = run(icp), run(icp)                                      # the second call replays the graph
    icp.setVoxelMatcher(0.5)
    b0, b1 = run(icp), run(icp)
    icp.setVoxelMatcher(1.0)
    a2 = run(icp)
    icp.close()
    fresh = make_icp(amd, 0.5)
    fresh.setMap(sc["map"], sc["normals"])
    bf = run(fresh)
    fresh.close()
    assert np.array_equal(_bits(a0), _bits(a1)) and np.array_equal(_bits(a0), _bits(a2))
    assert np.array_equal(_bits(b0), _bits(b1)) and np.array_equal(_bits(b0), _bits(bf))
    assert not np.array_equal(_bits(a0), _bits(b0))


YAML_CHAIN = """matcher:
  VoxelMatcher:
    voxelSize: 1.0
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


def test_yaml_front_ends_give_the_c_calls_bits(amd):
    import host_chain_bindings as hcb
    sc, rd, rn, _ = vc.registration_inputs()
    direct = make_icp(amd, 1.0, **REG)
    direct.setMap(sc["map"], sc["normals"])
    T = direct(rd, rn)
    its = direct.stats.iterations
    direct.close()
    chain = {"matcher": {"VoxelMatcher": {"voxelSize": 1.0}}, "errorMinimizer": {"PlaneToPlaneErrorMinimizer": {"epsilon": 0.001}},
             "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}},
                                        {"DifferentialTransformationChecker": {"minDiffRotErr": 0.001, "minDiffTransErr": 0.001, "smoothLength": 3}}]}
    py = amd.ICPSequence.loadFromYaml(chain)
    assert py.getVoxelMatcher() == 1.0
    py.setMap(sc["map"], sc["normals"])
    T_py = py(rd, rn)
    py.close()
    T_cpp, stats = hcb.icp_register(YAML_CHAIN, sc["map"], sc["normals"], rd, rn)
    assert np.array_equal(_bits(T_py), _bits(T))
    assert np.array_equal(_bits(T_cpp), _bits(T)) and stats.iterations == its
    with pytest.raises(RuntimeError, match="normals"):               # a reading without `normals`: InvalidField
        hcb.icp_register(YAML_CHAIN, sc["map"], sc["normals"], rd, None)
    with pytest.raises(RuntimeError, match="voxel matcher.*outlier filters"):
        hcb.icp_register(YAML_CHAIN + "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n", sc["map"], sc["normals"], rd, rn)


def _refused(icp, st, code, *words):
    msg = icp._lib.icpmi_last_error(icp._h).decode()
    assert st == code, (st, msg)
    for w in ("voxel matcher",) + words:
        assert w in msg, msg


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
    sc, rd, rn, _ = vc.registration_inputs()
    icp = make_icp(amd, 1.0, **kw)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        T, st = (C.c_float * 16)(), _capi_stats(amd)
        _refused(icp, icp._lib.icpmi_register(icp._h, rd.ctypes.data, rd.shape[0], rn.ctypes.data, T, C.byref(st)), INVALID_ARG, word)
        rc = vr.centred(sc["reading"], icp.getMapMean())
        sums = (C.c_double * 32)()
        _refused(icp, icp._lib.icpmi_minimize_step_normals(icp._h, rc.ctypes.data, rc.shape[0], rn.ctypes.data, None, T, sums, C.byref(st)), INVALID_ARG, word)
        icp.setVoxelMatcher(0.0)                                     # off: the chain runs as it always did
        if what not in ("var_dist",):
            assert icp._lib.icpmi_register(icp._h, rd.ctypes.data, rd.shape[0], rn.ctypes.data, T, C.byref(st)) == OK
    finally:
        icp.close()


def _capi_stats(amd):
    from norlab_icp_mapper_amd import _capi
    return _capi.Stats()


def test_intensity_weight_is_refused(amd):
    sc, rd, rn, _ = vc.registration_inputs()
    icp = make_icp(amd, 1.0)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        assert icp._lib.icpmi_set_intensity_weight(icp._h, C.c_float(0.1)) == OK
        _refused(icp, icp._lib.icpmi_register(icp._h, rd.ctypes.data, rd.shape[0], rn.ctypes.data, (C.c_float * 16)(), None), INVALID_ARG, "intensity")
    finally:
        icp.close()


def test_entry_points_that_do_not_serve_it(amd):
    import torch
    sc, rd, rn, _ = vc.registration_inputs()
    icp = make_icp(amd, 1.0)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        lib, h = icp._lib, icp._h
        d = torch.from_numpy(rd).cuda()
        T, st, status = (C.c_float * 32)(), (_capi_stats(amd).__class__ * 2)(), (C.c_int * 2)()
        ptrs, ns = (C.c_void_p * 1)(d.data_ptr()), (C.c_int64 * 1)(rd.shape[0])
        _refused(icp, lib.icpmi_register_batch_dev(h, 1, ptrs, ns, 2, T, st, status), UNSUPPORTED, "register_batch")
        prior = np.ascontiguousarray(np.eye(4, dtype=F).T).ravel()
        _refused(icp, lib.icpmi_register_multistart(h, rd.ctypes.data, rd.shape[0], prior.ctypes.data, 1, 2, T, st, status), UNSUPPORTED, "register_multistart")
        _refused(icp, lib.icpmi_register_multistart_dev(h, d.data_ptr(), rd.shape[0], prior.ctypes.data, 1, 2, T, st, status), UNSUPPORTED, "register_multistart")
        rc = vr.centred(sc["reading"], icp.getMapMean())
        _refused(icp, lib.icpmi_minimize_step(h, rc.ctypes.data, rc.shape[0], None, T, (C.c_double * 32)(), None), UNSUPPORTED, "minimize_step")
        t = np.zeros(rd.shape[0], F)
        for call in (lambda: icp.register_sweep(rd, t, np.eye(4), np.eye(4)), lambda: icp.sweep_sums(rd, t, np.eye(4), np.eye(4)),
                     lambda: icp.register_sweep_dev(d.data_ptr(), rd.shape[0], torch.from_numpy(t).cuda().data_ptr(), np.eye(4), np.eye(4))):
            with pytest.raises(NotImplementedError, match="voxel matcher"):
                call()
        # a reading without normals: as on the plane-to-plane path
        assert lib.icpmi_register(h, rd.ctypes.data, rd.shape[0], None, T, None) == MISSING_NORMALS
        # icpmi_residual_error* are unchanged: the pose is scored through the nearest-neighbour matcher, as on any plane-to-plane handle
        res = icp.residual(rd, np.eye(4), normals=rn)
    finally:
        icp.close()
    plain = amd.ICPSequence(knn=1, max_dist=2.0, minimizer=vc.MIN_PLANE_TO_PLANE, outliers=[])
    plain.setMap(sc["map"], sc["normals"])
    assert plain.residual(rd, np.eye(4), normals=rn).bits() == res.bits() and res.pairs > 0
    plain.close()


def plane_to_plane_results(amd, touch):
    """sums and step of every k = 1 case of tests/plane_to_plane_cases.py and a registration, on a handle that saw (touch) or never saw
    the voxel setter"""
    out = []
    for name, start, k, chain in pc.SUM_CASES:
        if k != 1 or name == "tunnel":
            continue
        sc = lr.scene(name)
        icp = amd.ICPSequence(knn=k, max_dist=pc.MAX_DIST, minimizer=pc.MIN_PLANE_TO_PLANE, outliers=pc.CHAINS[chain]["outliers"])
        if touch:
            icp.setVoxelMatcher(1.0)
            icp.setVoxelMatcher(0.0)
        icp.setMap(sc["map"], sc["normals"])
        rc = vr.centred(sc["reading"], icp.getMapMean())
        T_step, sums = icp.minimizeStep(rc, pc.STARTS[start].astype(F), read_normals=sc["reading_normals"])
        out += [_bits(T_step).ravel(), np.asarray(sums).view(np.uint64)]
        if chain == "trimmed" and start == "off":
            out.append(_bits(icp(sc["reading"], sc["reading_normals"])).ravel())
        icp.close()
    return out


def test_size_zero_changes_no_bit_of_plane_to_plane(amd):
    a, b = plane_to_plane_results(amd, False), plane_to_plane_results(amd, True)
    assert len(a) == len(b) > 8
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
