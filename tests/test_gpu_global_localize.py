"""Global localisation on the device (csrc/occupancy.hip), through the C ABI and the two front ends, against the integer
restatement in tests/global_localize_reference.py.  Every comparison is == on integers: the pyramid's key sets, the node scores, the leaf the
search returns and the number of nodes it scored; the poses are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import global_localize_reference as glr
import localizability_reference as lr
import voxel_reference as vr

pytestmark = pytest.mark.gpu
F = np.float32
OK, INVALID_ARG, NO_POINT, UNSUPPORTED = 0, 1, 3, 8
MIN_POINT_TO_POINT, MIN_PLANE_TO_PLANE = 1, 3
S0 = glr.S0


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def f4(xyz):
    xyz = np.asarray(xyz, np.float64)
    return np.concatenate([xyz[:, :3], np.ones((xyz.shape[0], 1))], 1).astype(F)


def make_icp(amd, map4, normals=None, **kw):
    kw.setdefault("minimizer", MIN_POINT_TO_POINT)
    icp = amd.ICPSequence(knn=1, max_dist=2.0, max_iterations=40, use_differential=1, **kw)
    assert icp.setMap(map4, normals)
    return icp


@pytest.fixture(scope="module")
def scene():
    return glr.scene()


@pytest.fixture(scope="module")
def handle(amd, scene):
    icp = make_icp(amd, scene["map"])
    yield icp
    icp.close()


@pytest.fixture(scope="module")
def ref(handle, scene):
    """the reference in the handle's own centred frame, six levels (what the automatic choice takes for the scene's window)"""
    pyr, rd, mean = glr.scene_inputs(handle.getMapMean(), levels=6)
    return dict(pyr=pyr, rd=rd, mean=mean)


def window_box(mean, a_min=glr.WINDOW[0], a_max=glr.WINDOW[1]):
    """a box in the map frame whose window is exactly [a_min, a_max]: the cells' centres"""
    mu = np.asarray(mean, np.float64)
    return (mu + S0 * (np.asarray(a_min) + 0.5), mu + S0 * (np.asarray(a_max) + 0.5))


def test_shape_is_what_the_reference_assumes(amd):
    from norlab_icp_mapper_amd import _capi
    sl, tl, ln = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _capi.load().icpmi_global_localize_shape(C.byref(sl), C.byref(tl), C.byref(ln))
    assert (sl.value, tl.value, ln.value) == (1024, 16, glr.TOP_CHUNK)


# ------------------------------------------------------------------------------------------------------------------ 1. the pyramid
@pytest.mark.parametrize("level", range(4))
def test_pyramid_levels_of_the_scene(handle, ref, level):
    got = handle.occupancyLevel(S0, 4, level)
    want = glr.unpack(ref["pyr"].keys[level])
    print(level, got.shape[0], want.shape[0])
    assert got.shape[0] == glr.KEYS[level]
    assert np.array_equal(got.astype(np.int64), want)


def check_pyramid(icp, map4, s0, levels):
    pyr = glr.Pyramid(vr.centred(map4, icp.getMapMean()), s0, levels)
    for l in range(levels):
        assert np.array_equal(icp.occupancyLevel(s0, levels, l).astype(np.int64), glr.unpack(pyr.keys[l])), l
    info = icp.occupancyInfo()
    assert info["levels"] >= levels and info["keys"][:levels] == [k.size for k in pyr.keys]
    assert info["bytes"][:levels] == [8 * (k.size + glr.capacity_of(k.size)) for k in pyr.keys]
    return pyr


def test_pyramid_of_one_point(amd):
    map4 = f4([[3.0, -2.0, 1.0]])
    icp = make_icp(amd, map4)
    try:
        pyr = check_pyramid(icp, map4, 0.5, 8)
        assert [k.size for k in pyr.keys] == [1] + [8] * 7
    finally:
        icp.close()


def test_pyramid_of_negative_cells_floors_the_shift(amd):
    """a cluster in cells -9 .. -1 on every axis and one counterweight far away (a centred frame cannot hold negative cells alone): a shift
    that truncated would send the cells -1, -3, ... to other blocks"""
    rng = np.random.default_rng(11)
    cluster = rng.uniform(-4.4, -0.1, (200, 3))
    map4 = f4(np.concatenate([cluster, [[900.0, 900.0, 900.0]]]))
    icp = make_icp(amd, map4)
    try:
        pyr = check_pyramid(icp, map4, 0.5, 5)
        c0 = pyr.cells[0]
        assert ((c0 < 0).all(1).sum() == c0.shape[0] - 1) and (c0 % 2 != 0).any()
    finally:
        icp.close()


def colliding_points(nk, cap):
    """centres of nk distinct unit cells whose keys all start in the last two slots of a table of `cap` slots and which sum to exactly 0, so
    that the handle's centred frame is this one"""
    cand = np.stack(np.meshgrid(*[np.arange(-40, 40)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pool = cand[glr.first_slot(glr.pack(cand), cap) >= cap - 2]
    rng = np.random.default_rng(3)
    for _ in range(10000):
        v = pool[rng.choice(pool.shape[0], nk - 1, replace=False)]
        last = -(nk // 2) - v.sum(0)
        if np.abs(last).max() < 1000 and glr.first_slot(glr.pack(last[None]), cap)[0] >= cap - 2 and not (v == last).all(1).any():
            return (np.concatenate([v, last[None]]) + 0.5).astype(F)
    raise AssertionError("no colliding key set found")


def test_colliding_keys_that_wrap_the_table(amd):
    nk = 16
    cap = glr.capacity_of(nk)
    pts = colliding_points(nk, cap)
    icp = make_icp(amd, f4(pts))
    try:
        assert np.array_equal(icp.getMapMean(), np.zeros(3, F))
        pyr = check_pyramid(icp, f4(pts), 1.0, 1)
        assert pyr.keys[0].size == nk and (glr.first_slot(pyr.keys[0], cap) >= cap - 2).all()
        # every cell is found wherever it landed: one point per cell under the identity, the leaf a = 0 scores all of them, a = (200, 0, 0) none
        got = icp.occupancyScoreNodes(f4(pts), np.eye(3, dtype=F)[None], 1.0, 1, [[0, 0, 0, 0, 0], [0, 0, 200, 0, 0]])
        assert got.tolist() == [nk, 0]
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the node scores
def random_nodes(rng, count, n_rot, levels):
    """nodes over all levels and rotations whose cubes lie around the scene's window"""
    l = rng.integers(0, levels, count)
    k = rng.integers(0, n_rot, count)
    a = np.stack([rng.integers(-12, 12, count), rng.integers(-26, 26, count), rng.integers(-6, 6, count)], 1) >> l[:, None]
    return np.concatenate([k[:, None], l[:, None], a], 1).astype(np.int32)


@pytest.mark.parametrize("n", (1428, 257, 1))
def test_scores_of_random_nodes(handle, scene, ref, n):
    rng = np.random.default_rng(100 + n)
    nodes = random_nodes(rng, 2000, glr.YAW_STEPS, 4)
    reading = np.ascontiguousarray(scene["reading"][:n])
    rd = ref["rd"] if n == 1428 else glr.Reading(reading, scene["rotations"], S0)
    want = glr.score_nodes(ref["pyr"], rd, nodes)
    got = handle.occupancyScoreNodes(reading, scene["rotations"], S0, 4, nodes)
    print(n, int(want.sum()), int((want > 0).sum()))
    assert want.sum() > 0
    assert np.array_equal(got, want)


def test_scores_skip_a_nan_point_and_a_point_beyond_the_cell_range(handle, scene, ref):
    reading = np.array(scene["reading"][:300])
    reading[7, 1] = np.nan
    reading[130, :3] = (1.0, 3.0e5, 0.5)           # 6e5 cells away: no cell
    reading[131, 0] = np.inf
    rd = glr.Reading(reading, scene["rotations"], S0)
    assert rd.points[0] == 297
    nodes = random_nodes(np.random.default_rng(7), 500, glr.YAW_STEPS, 4)
    assert np.array_equal(handle.occupancyScoreNodes(reading, scene["rotations"], S0, 4, nodes), glr.score_nodes(ref["pyr"], rd, nodes))


def test_a_node_wholly_off_the_map_scores_zero(handle, scene):
    nodes = [[k, l, 5000 >> l, 0, 0] for k in (0, 7, 63) for l in range(4)]
    assert handle.occupancyScoreNodes(scene["reading"], scene["rotations"], S0, 4, nodes).tolist() == [0] * len(nodes)


def test_more_nodes_than_one_launch_carries(handle, scene, ref):
    """every leaf of the window for 19 rotations, 70 224 nodes, against the exhaustive correlation"""
    a_min, a_max = (np.asarray(a) for a in glr.WINDOW)
    ex = glr.exhaustive(ref["pyr"], ref["rd"], a_min, a_max)
    ks = np.arange(19)
    grid = np.stack(np.meshgrid(ks, *[np.arange(a_min[j], a_max[j] + 1) for j in range(3)], indexing="ij"), -1).reshape(-1, 4)
    nodes = np.concatenate([grid[:, :1], np.zeros((grid.shape[0], 1), np.int64), grid[:, 1:]], 1)
    assert nodes.shape[0] > glr.TOP_CHUNK
    got = handle.occupancyScoreNodes(scene["reading"], scene["rotations"], S0, 1, nodes)
    assert np.array_equal(got, ex[:19].reshape(-1))


# ------------------------------------------------------------------------------------------------------------------ 3. the search
_ref_runs = {}


def reference_run(ref, levels, batch, **kw):
    key = (levels, batch, tuple(sorted(kw.items())))
    if key not in _ref_runs:
        _ref_runs[key] = glr.search(ref["pyr"], ref["rd"], glr.WINDOW[0], glr.WINDOW[1], levels, batch, **kw)
    return _ref_runs[key]


def as_dict(g):
    return dict(found=int(g.found), proven=int(g.proven), rotation=g.rotation, cell=g.cell, score=g.score, points=g.points, levels=g.levels,
                nodes_scored=g.nodes_scored, leaves_scored=g.leaves_scored, launches=g.launches)


@pytest.mark.parametrize("batch", (1, 64, 1024))
@pytest.mark.parametrize("levels", (1, 3, 4, 0))
def test_search_returns_the_maximiser_and_scores_the_reference_drivers_nodes(handle, scene, ref, levels, batch):
    got = handle.globalLocalize(scene["reading"], scene["rotations"], S0, box=window_box(ref["mean"]), levels=levels, batch=batch)
    print(levels, batch, got)
    assert (got.found, got.proven, got.score, got.rotation, got.cell, got.points) == (True, True, 1424, 7, (1, 1, 0), 1428)
    if levels == 1:                                # the exhaustive run: every leaf of the window, four launches
        assert (got.nodes_scored, got.leaves_scored, got.launches, got.levels) == (glr.LEAVES, glr.LEAVES, 4, 1)
    else:
        assert as_dict(got) == reference_run(ref, levels, batch)
    assert (got.nodes_scored, got.launches) == glr.COUNTS[(levels, batch)]
    assert np.array_equal(got.pose.view(np.uint32), glr.pose_of(scene["rotations"][7], (1, 1, 0), ref["mean"], S0).view(np.uint32))


def test_two_calls_give_the_same_bits(handle, scene, ref):
    a, b = (handle.globalLocalize(scene["reading"], scene["rotations"], S0, box=window_box(ref["mean"]), levels=4) for _ in range(2))
    assert a.bits() == b.bits()


def test_the_device_variant_gives_the_same_bits(handle, scene, ref):
    import torch
    d = torch.from_numpy(np.array(scene["reading"])).cuda()
    a = handle.globalLocalize(scene["reading"], scene["rotations"], S0, box=window_box(ref["mean"]), levels=4)
    b = handle.globalLocalizeDev(d.data_ptr(), d.shape[0], scene["rotations"], S0, box=window_box(ref["mean"]), levels=4)
    assert a.bits() == b.bits()


def test_the_pyramid_follows_the_map(amd, scene):
    """the same handle, then the map turned by a quarter turn about z: the old answer (rotation 7) is wrong for it, the new one is the
    reference's for the new map"""
    icp = make_icp(amd, scene["map"])
    try:
        first = icp.globalLocalize(scene["reading"], scene["rotations"], S0, levels=4)
        assert (first.rotation, first.score) == (7, 1424) and icp.occupancyInfo()["builds"] == 1
        turned = np.array(scene["map"])
        turned[:, 0], turned[:, 1] = -scene["map"][:, 1], scene["map"][:, 0]
        assert icp.setMap(turned)
        got = icp.globalLocalize(scene["reading"], scene["rotations"], S0, levels=4)
        mean = icp.getMapMean()
        pyr = glr.Pyramid(vr.centred(turned, mean), S0, 4)
        rd = glr.Reading(scene["reading"], scene["rotations"], S0)
        want = glr.search(pyr, rd, pyr.cells[0].min(0), pyr.cells[0].max(0), 4, 64)
        print(got, want)
        assert icp.occupancyInfo()["builds"] == 2
        assert as_dict(got) == want and got.rotation == 23 and got.score >= 1400
        assert glr.bound(pyr, rd, first.rotation, 0, first.cell) < got.score
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 4. ties
def test_ties_on_the_plain_room(amd):
    """the room without the box is symmetric under half a turn: more than one leaf may hold the maximum; whichever is returned holds it"""
    sc = lr.scene("room")
    rot = glr.yaw_rotations(glr.YAW_STEPS)
    icp = make_icp(amd, sc["map"])
    try:
        full = icp.globalLocalize(sc["reading"], rot, S0, levels=1)
        got = icp.globalLocalize(sc["reading"], rot, S0)
        pyr = glr.Pyramid(vr.centred(sc["map"], icp.getMapMean()), S0, 1)
        rd = glr.Reading(sc["reading"], rot, S0)
        ex = glr.exhaustive(pyr, rd, pyr.cells[0].min(0), pyr.cells[0].max(0))
        print(full, got, int(ex.max()), int((ex == ex.max()).sum()))
        assert full.leaves_scored == ex.size and full.score == ex.max()
        assert got.found and got.proven and got.score == full.score
        assert glr.bound(pyr, rd, got.rotation, 0, got.cell) == full.score
        assert glr.bound(pyr, rd, full.rotation, 0, full.cell) == full.score
    finally:
        icp.close()


# ------------------------------------------------------------------------------------------------------------------ 5. min_score_ratio, max_nodes
def test_min_score_ratio(handle, scene, ref):
    box = window_box(ref["mean"])
    none = handle.globalLocalize(scene["reading"], scene["rotations"], S0, box=box, levels=4, min_score_ratio=1.0)        # need = 1428
    assert as_dict(none) == reference_run(ref, 4, 64, min_score_ratio=1.0)
    assert (none.found, none.proven, none.rotation, none.nodes_scored) == (False, True, -1, 3648)
    assert np.array_equal(none.pose, np.eye(4, dtype=F))
    assert glr.need_of(0.7, 1428) == 1000
    some = handle.globalLocalize(scene["reading"], scene["rotations"], S0, box=box, levels=4, min_score_ratio=0.7)        # need = 1000
    assert as_dict(some) == reference_run(ref, 4, 64, min_score_ratio=0.7)
    assert (some.found, some.score, some.rotation, some.cell, some.nodes_scored) == (True, 1424, 7, (1, 1, 0), 3656)


@pytest.mark.parametrize("cap", (100, 2500, 3655, 3656))
def test_max_nodes(handle, scene, ref, cap):
    got = handle.globalLocalize(scene["reading"], scene["rotations"], S0, box=window_box(ref["mean"]), levels=4, batch=1, max_nodes=cap)
    want = reference_run(ref, 4, 1, max_nodes=cap)
    print(cap, got)
    assert as_dict(got) == want
    assert got.proven == (cap >= 3656) and got.nodes_scored > min(cap, 3655)
    if cap == 100:                                 # stopped behind the first launch: the top level holds no leaf
        assert not got.found and got.leaves_scored == 0 and got.launches == 1


# ------------------------------------------------------------------------------------------------------------------ 6. the front ends
def test_relocalize_global_is_the_search_then_relocalize(amd, scene, ref):
    icp = make_icp(amd, scene["map"])
    try:
        box = window_box(icp.getMapMean())
        out = icp.relocalizeGlobal(scene["reading"], scene["rotations"], S0, box=box, refine=1)
        found = icp.globalLocalize(scene["reading"], scene["rotations"], S0, box=box)
        by_hand = icp.relocalize(scene["reading"], [found.pose], refine=1)
        assert out.search.bits() == found.bits() and found.rotation == 7
        assert np.array_equal(out.pose.view(np.uint32), by_hand.pose.view(np.uint32)) and out.residual.bits() == by_hand.residual.bits()
        # the refined pose is the true one to a few centimetres: the search's cell is 0.5 m wide, ICP does the rest
        T_true = lr.make_T((0, 0, glr.YAW), glr.SENSOR)
        assert np.abs(out.pose[:3, 3] - T_true[:3, 3]).max() < 0.05 and np.abs(out.pose[:3, :3] - T_true[:3, :3]).max() < 0.02
    finally:
        icp.close()


def test_relocalize_global_on_a_voxel_handle_is_the_search_then_relocalize_voxel(amd):
    sc = lr.scene("room")
    rot = glr.yaw_rotations(glr.YAW_STEPS)
    icp = amd.ICPSequence(knn=1, max_dist=2.0, max_iterations=40, use_differential=1, minimizer=MIN_PLANE_TO_PLANE, outliers=[], voxel_size=1.0)
    try:
        assert icp.setMap(sc["map"], sc["normals"])
        out = icp.relocalizeGlobal(sc["reading"], rot, S0, normals=sc["reading_normals"], refine=1)
        found = icp.globalLocalize(sc["reading"], rot, S0)
        by_hand = icp.relocalizeVoxel(sc["reading"], sc["reading_normals"], [found.pose], refine=1)
        assert out.search.bits() == found.bits()
        assert np.array_equal(out.pose.view(np.uint32), by_hand.pose.view(np.uint32)) and out.residual.bits() == by_hand.residual.bits()
        with pytest.raises(amd.InvalidField, match="relocalizeGlobal"):
            icp.relocalizeGlobal(sc["reading"], rot, S0)
    finally:
        icp.close()


KD_CHAIN = {"matcher": {"KDTreeMatcher": {"knn": 1, "maxDist": 2.0}}, "errorMinimizer": "PointToPointErrorMinimizer",
            "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}},
                                       {"DifferentialTransformationChecker": {"minDiffRotErr": 0.001, "minDiffTransErr": 0.001, "smoothLength": 3}}]}
KD_YAML = """matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 2.0
errorMinimizer: PointToPointErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 40
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.001
      smoothLength: 3
"""
VOXEL_YAML = KD_YAML.replace("  KDTreeMatcher:\n    knn: 1\n    maxDist: 2.0\n", "  VoxelMatcher:\n    voxelSizes: [1.0, 0.5]\n").replace(
    "errorMinimizer: PointToPointErrorMinimizer\n", "errorMinimizer:\n  PlaneToPlaneErrorMinimizer:\n    epsilon: 0.001\n")
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
"""


def test_cpp_global_localize_and_relocalize_global(amd, scene):
    """the host shell's calls: the search's result struct is the Python call's bit for bit, and relocalizeGlobal is the search followed by
    relocalize(reading, [found pose]) as the Python mirror runs it by hand on the same chain"""
    import host_global_localize_bindings as hg
    from norlab_icp_mapper_amd import icp as I
    icp = amd.ICPSequence.loadFromYaml(KD_CHAIN)
    try:
        assert icp.setMap(scene["map"])
        box = window_box(icp.getMapMean())
        found = icp.globalLocalize(scene["reading"], scene["rotations"], S0, box=box, levels=4)
        by_hand = icp.relocalize(scene["reading"], [found.pose], refine=1)
        alone = hg.icp_global_localize(KD_YAML, scene["map"], None, scene["reading"], None, scene["rotations"], S0, levels=4, box=box)
        assert bytes(alone["result"]) == found.bits()
        got = hg.icp_global_localize(KD_YAML, scene["map"], None, scene["reading"], None, scene["rotations"], S0, levels=4, box=box, refine=True)
        assert bytes(got["result"]) == found.bits() and not got["voxel"]
        assert np.array_equal(got["pose"].view(np.uint32), by_hand.pose.view(np.uint32))
        assert I.Residual(got["residual"]).bits() == by_hand.residual.bits()
        with pytest.raises(RuntimeError, match="ConvergenceError: relocalizeGlobal"):
            hg.icp_global_localize(KD_YAML, scene["map"], None, scene["reading"], None, scene["rotations"], S0, levels=4, box=box, ratio=1.0, refine=True)
    finally:
        icp.close()


def test_cpp_relocalize_global_on_a_voxel_chain_and_the_mapper(amd, tmp_path):
    import os
    import host_global_localize_bindings as hg
    import host_voxel_score_bindings as hv
    sc = lr.scene("room")
    rot = glr.yaw_rotations(glr.YAW_STEPS)
    rd, rn = np.ascontiguousarray(sc["reading"]), np.ascontiguousarray(sc["reading_normals"])
    got = hg.icp_global_localize(VOXEL_YAML, sc["map"], sc["normals"], rd, rn, rot, S0, refine=True)
    res = got["result"]
    assert got["voxel"] and res.found and res.proven
    start = np.array(res.T[:], F).reshape(4, 4).T
    by_hand = hv.icp_relocalize_voxel(VOXEL_YAML, sc["map"], sc["normals"], rd, rn, [start], refine=1)
    assert np.array_equal(got["pose"].view(np.uint32), by_hand["pose"].view(np.uint32)) and bytes(got["score"]) == bytes(by_hand["score"])
    cfg = os.path.join(str(tmp_path), "config.yaml")
    open(cfg, "w").write(MAPPER_YAML % VOXEL_YAML.replace("\n", "\n  ").rstrip())
    m = hg.mapper_relocalize_global(cfg, sc["map"], sc["normals"], rd, rn, rot, S0)
    assert m["map_before"] == m["map_after"] == sc["map"].shape[0]                     # the map is not touched ...
    assert np.array_equal(m["pose"].view(np.uint32), m["get_pose"].view(np.uint32))    # ... the pose is set
    assert bytes(m["result"]) == bytes(res) and np.array_equal(m["pose"].view(np.uint32), got["pose"].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(amd, scene):
    rd, rot = scene["reading"], scene["rotations"]
    bare = amd.ICPSequence(knn=1, max_dist=2.0, minimizer=MIN_POINT_TO_POINT)
    try:
        with pytest.raises(amd.InvalidParameter, match="global_localize: no map"):
            bare.globalLocalize(rd, rot, S0)
    finally:
        bare.close()
    planar = make_icp(amd, scene["map"], force_2d=1)
    try:
        with pytest.raises(RuntimeError, match="global_localize: is not served in planar mode"):
            planar.globalLocalize(rd, rot, S0)
    finally:
        planar.close()
    icp = make_icp(amd, scene["map"])
    try:
        skew = np.array(rot[:3])
        skew[1] = skew[1] * F(1.01)
        mean = icp.getMapMean().astype(np.float64)
        for kw, args, text in (
                (dict(), (rd, skew, S0), "global_localize: rotation 1: TransformationError"),
                (dict(), (rd, np.zeros((0, 3, 3), F), S0), "n_rot must be in 1 .. 4096"),
                (dict(), (rd, np.tile(rot[:1], (4097, 1, 1)), S0), "n_rot must be in 1 .. 4096"),
                (dict(box=(mean + 1.0, mean - 1.0)), (rd, rot, S0), "bad box"),
                (dict(box=(mean, mean + np.array([np.inf, 0, 0]))), (rd, rot, S0), "bad box"),
                (dict(box=(mean, mean + 3.0e5)), (rd, rot, S0), "bad box"),
                (dict(), (rd, rot, 0.0), "cell size must be finite and > 0"),
                (dict(), (rd, rot, np.nan), "cell size must be finite and > 0"),
                (dict(levels=9), (rd, rot, S0), "levels must be in 0 .. 8"),
                (dict(batch=0), (rd, rot, S0), "batch must be in 1 .. 8192"),
                (dict(min_score_ratio=1.5), (rd, rot, S0), "min_score_ratio must be in 0 .. 1")):
            with pytest.raises(ValueError, match=text):
                icp.globalLocalize(*args, **kw)
        with pytest.raises(amd.ConvergenceError, match="the reading is empty"):
            icp.globalLocalize(np.zeros((0, 4), F), rot, S0)
        assert icp.occupancyInfo()["builds"] == 0       # every refusal came before anything was built or enqueued
    finally:
        icp.close()
