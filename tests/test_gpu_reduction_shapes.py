"""The shared device building blocks (csrc/common.h: bbox_partials_kernel / bbox_fold; csrc/ops.hip: compact_points_kernel /
compact_records_kernel) at the sizes where a reduction or a compaction can go wrong: one point, one wave short of / exactly / one past a
workgroup, and one point past the first grid-stride wrap of every caller (64 workgroups for SamplingSurfaceNormal, 256 for the self
search, 1024 for the octree and the voxel grid).  Only through the existing entry points, against the references the other tests use
(the oracle; tests/voxel_grid_reference.py), index for index and bit for bit."""
import numpy as np
import pytest

import voxel_grid_reference as vgr
from test_gpu_map_chain import host_chain

pytestmark = pytest.mark.gpu

F = np.float32
SMALL = [1, 2, 255, 256, 257]
WRAP_SSN, WRAP_SELF, WRAP_TREE = 64 * 256 + 1, 256 * 256 + 1, 1024 * 256 + 1
NONFINITE = "non-finite"          # both entry points answered ICPMI_ERR_INVALID_ARG (InvalidParameter) with this in the message before the
                                  # reductions were unified: "voxel_grid: non-finite ..." / "set_map: non-finite coordinates in the map cloud"


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def icp(amd):
    return amd.ICPSequence(minimizer=2)


def _cloud(n, seed=3):
    """n points of a gently curved sheet, 20 m x 12 m: every coordinate differs, the extrema lie at arbitrary indices"""
    rng = np.random.default_rng(seed + n)
    c = np.ones((n, 4), F)
    xy = rng.uniform(-1, 1, (n, 2)) * [10.0, 6.0]
    c[:, 0], c[:, 1] = xy[:, 0], xy[:, 1]
    c[:, 2] = 0.05 * xy[:, 0] * xy[:, 1] + 0.02 * rng.standard_normal(n)
    return c


def _extremes_last(c):
    """the same cloud with every extreme of the box in its LAST point and its first: the lanes a short last workgroup leaves idle, and lane 0"""
    c = c.copy()
    c[-1, :3] = c[:, :3].max(0) + F(0.5)
    c[0, :3] = c[:, :3].min(0) - F(0.5)
    return c


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("n", SMALL + [WRAP_TREE])
def test_octree_box_at_workgroup_and_grid_stride_edges(icp, oracle, n):
    for cloud in (_cloud(n), _extremes_last(_cloud(n))):
        for max_size, max_pts, method in ((0.5, 1, 0), (0.0, 5, 1)):
            got = icp.octreeSample(cloud, max_size, max_pts, method)
            want = oracle.octree_sample(cloud, max_size, max_pts, method)
            assert got.shape == want.shape and np.array_equal(got, want), (n, max_size, max_pts, method)


@pytest.mark.parametrize("n", SMALL + [WRAP_TREE])
def test_voxel_grid_box_at_workgroup_and_grid_stride_edges(icp, n):
    for cloud in (_cloud(n), _extremes_last(_cloud(n))):
        order, out4, _ = icp.voxelGrid(cloud, [0.3, 0.2, 0.1])
        o2, out2, _ = vgr.voxel_grid(cloud, [0.3, 0.2, 0.1], True, None)
        assert np.array_equal(order, o2), n
        assert np.array_equal(_bits(out4), _bits(out2)), n


@pytest.mark.parametrize("n", SMALL + [WRAP_SSN])
def test_sampling_surface_normal_box_at_workgroup_and_grid_stride_edges(icp, oracle, n):
    for cloud in (_cloud(n), _extremes_last(_cloud(n))):
        order, nrm = icp.samplingSurfaceNormal(cloud, ratio=0.5, knn=7, seed=1)
        o_order, o_nrm = oracle.sampling_surface_normal(cloud, 0.5, 7, seed=1, max_box_dim=np.inf)
        assert np.array_equal(order, o_order), (n, order.shape, o_order.shape)
        if order.shape[0]:
            assert (np.abs(np.einsum("ij,ij->i", nrm, o_nrm)) > 1 - 1e-5).all()


@pytest.mark.parametrize("n", [255, 256, 257, WRAP_SELF, WRAP_TREE])
def test_self_search_box_at_workgroup_and_grid_stride_edges(icp, oracle, n):
    """SurfaceNormalDataPointsFilter: neighbour ids and mean distances are the oracle's kd-tree's, bit for bit (the oracle takes about a
    second on the largest cloud: every query is compared)"""
    cloud = _extremes_last(_cloud(n))
    _, ids, md = icp.surfaceNormals(cloud, knn=10, with_matched_ids=True, with_mean_dist=True)
    _, ids_o, md_o = oracle.surface_normals_extras(cloud, knn=10, nthreads=8)
    assert np.array_equal(ids, ids_o)
    assert np.array_equal(md.view(np.uint32), md_o.view(np.uint32))


@pytest.mark.parametrize("n", [1, 2])
def test_self_search_of_fewer_points_than_neighbours(icp, oracle, n):
    cloud = _cloud(n)
    nrm = icp.surfaceNormals(cloud, knn=10)
    assert np.array_equal(_bits(nrm), _bits(oracle.surface_normals(cloud, knn=10, nthreads=1)))


@pytest.mark.parametrize("n", [257, WRAP_SELF + 300])
@pytest.mark.parametrize("where", ["last point", "last workgroup"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinate_seen_by_the_last_workgroup(amd, icp, n, where, value):
    """the only non-finite coordinate sits in the last point / in a point the last workgroup of the reduction handles: the count it
    leaves next to its partials must reach the host (self search) and the one-workgroup fold (voxel grid)"""
    cloud = _cloud(n)
    i = n - 1 if where == "last point" else n - 40     # (n - 40: inside the last 256 points in both sizes)
    cloud[i, 1] = value
    with pytest.raises(amd.InvalidParameter, match=NONFINITE):
        icp.voxelGrid(cloud, 0.1)
    with pytest.raises(amd.InvalidParameter, match=NONFINITE):
        icp.surfaceNormals(cloud, knn=10)
    good = _cloud(n)                                   # both handles' paths go on afterwards
    o2, out2, _ = vgr.voxel_grid(good, 0.25, True, None)
    order, out4, _ = icp.voxelGrid(good, 0.25)
    assert np.array_equal(order, o2) and np.array_equal(_bits(out4), _bits(out2))
    assert np.isfinite(icp.surfaceNormals(good, knn=10)).all()


def test_each_caller_keeps_its_own_finiteness_limit(amd, icp):
    """3.2e38 is a finite float: above the self search's limit (3.0e38: its grid arithmetic must not overflow), below the voxel grid's
    (FLT_MAX).  The limit is an argument of the shared kernel: the voxel grid accepts the cloud, the self search rejects it."""
    cloud = _cloud(300)
    cloud[299, 0] = F(3.2e38)
    vs = [1e37, 1.0, 1.0]                              # 33 divisions along x: within the grid's limits
    order, out4, _ = icp.voxelGrid(cloud, vs)
    o2, out2, _ = vgr.voxel_grid(cloud, vs, True, None)
    assert np.array_equal(order, o2) and np.array_equal(_bits(out4), _bits(out2))
    assert out4[:, 0].max() == F(3.2e38)
    with pytest.raises(amd.InvalidParameter, match=NONFINITE):
        icp.surfaceNormals(cloud, knn=10)


# ---- compaction: nothing kept, everything kept, only the last point kept, only point 0 dropped ------------------------------------------
def _map_and_scans(amd):
    base = _cloud(5000, seed=11)
    rng = np.random.default_rng(12)
    near = base[rng.permutation(5000)[:1500]].copy()           # on top of map points: nothing is kept at minDist 0.3
    near[:, :3] += rng.normal(0, 0.001, (1500, 3)).astype(F)
    far = _cloud(1500, seed=13); far[:, 0] += F(100.0)         # 100 m from the map: everything is kept
    last = near.copy(); last[-1] = far[0]                      # only the last point is kept
    return base, {"none": near, "all": far, "last": last}


@pytest.mark.parametrize("case", ["none", "all", "last"])
def test_append_only_update_compaction_edges(amd, oracle, case):
    base, scans = _map_and_scans(amd)
    scan = scans[case]
    keep_ref = oracle.point_distance_keep(base, scan, 0.3, nthreads=8).astype(bool)
    want = {"none": 0, "all": scan.shape[0], "last": 1}[case]
    assert int(keep_ref.sum()) == want and (case != "last" or keep_ref[-1])          # the scans are what their names say
    icp = amd.ICPSequence(minimizer=1, max_dist=2.0)
    icp.setMap(base)
    app, m, keep = icp.mapUpdatePointDistance(scan, 0.3, return_keep=True)
    assert np.array_equal(keep, keep_ref)
    assert app == want and m == base.shape[0] + want
    assert np.array_equal(_bits(icp.getMap()), _bits(np.concatenate([base, scan[keep_ref]])))


@pytest.mark.parametrize("case", ["none", "all", "last", "drop point 0"])
def test_chain_compaction_edges(amd, oracle, case):
    base, scans = _map_and_scans(amd)
    if case == "drop point 0":
        # the cut drops exactly map point 0 (scalar above the threshold), keeps the rest and the whole scan
        modules, post, scan = [("point_distance", 0.0)], [("cut_scalar", 0.65, 1)], scans["all"]
        base_s = np.full(base.shape[0], 0.5, F); base_s[0] = F(0.9)
    else:
        modules, post, scan = [("point_distance", 0.3)], [], scans[case]
        base_s = np.full(base.shape[0], 0.5, F)
    scan_s = np.full(scan.shape[0], 0.6, F)
    base_n = np.zeros((base.shape[0], 3), F); base_n[:, 2] = 1
    eye = np.eye(4, dtype=F)
    icp = amd.ICPSequence(minimizer=1, max_dist=2.0)
    icp.setMap(base, base_n)
    icp.setMapScalar(base_s)
    src, m, head = icp.mapUpdateChain(scan, modules, post, scan_scalar=scan_s, to_sensor=eye, with_prefix=True)
    pts, nrm, sc, ref_src = host_chain(oracle, base, base_n, base_s, scan, scan_s, eye, modules, post)
    if case == "none":
        assert pts.shape[0] == base.shape[0]
    if case == "last":
        assert pts.shape[0] == base.shape[0] + 1
    if case == "drop point 0":
        assert ref_src[0] == 1 and pts.shape[0] == base.shape[0] - 1 + scan.shape[0]
    moved = np.nonzero(ref_src != np.arange(ref_src.shape[0]))[0]
    assert head == (moved[0] if moved.size else ref_src.shape[0])
    assert m == pts.shape[0]
    assert np.array_equal(src, ref_src)
    got, got_n = icp.getMap(with_normals=True)
    assert np.array_equal(_bits(got), _bits(pts))
    assert np.array_equal(_bits(got_n), _bits(nrm))
    assert np.array_equal(_bits(icp.getMapScalar()), _bits(sc))
