"""VoxelGridDataPointsFilter without a GPU: the numpy restatement (tests/voxel_grid_reference.py) on hand-worked clouds, and the
host shell's parameter handling through the filter-chain test hook (no GPU context)."""
import os

import numpy as np
import pytest

import voxel_grid_reference as vgr

F = np.float32


def _c4(xyz):
    xyz = np.asarray(xyz, F)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


def test_two_voxels_known_centroids():
    c = _c4([[0.1, 0.1, 0.1], [0.3, 0.3, 0.3], [1.5, 0.2, 0.2], [1.7, 0.4, 0.4]])
    minB, nd, idx = vgr.grid(c[:, :3], 1.0)
    assert nd.tolist() == [2, 1, 1] and idx.tolist() == [0, 0, 1, 1]
    order, out, _ = vgr.voxel_grid(c, 1.0)
    assert order.tolist() == [0, 2]
    want = np.array([[(F(0.1) + F(0.3)) / F(2)] * 3, [(F(1.5) + F(1.7)) / F(2), (F(0.2) + F(0.4)) / F(2), (F(0.2) + F(0.4)) / F(2)]], F)
    assert np.array_equal(out[:, :3], want) and np.array_equal(out[:, 3], [1, 1])
    assert np.allclose(out[:, :3], [[0.2, 0.2, 0.2], [1.6, 0.3, 0.3]], atol=1e-6)


def test_output_order_is_first_point_order_not_voxel_order():
    c = _c4([[1.5, 0, 0], [0.2, 0, 0], [1.7, 0, 0], [0.0, 0, 0]])
    _, _, idx = vgr.grid(c[:, :3], 1.0)
    assert idx.tolist() == [1, 0, 1, 0]                     # voxel 1 holds point 0: it comes out first
    order, out, _ = vgr.voxel_grid(c, 1.0)
    assert order.tolist() == [0, 1]
    assert out[0, 0] == (F(1.5) + F(1.7)) / F(2) and out[1, 0] == (F(0.2) + F(0.0)) / F(2)


def test_numdiv_truncation_and_left_to_right_evaluation():
    # (1 + maxB) - minB exactly 3 and 2: a lattice without the + 1 would put (2, 0) and (0, 1) in one voxel
    c = _c4([[0, 0, 0], [2, 0, 0], [0, 1, 0]])
    _, nd, idx = vgr.grid(c[:, :3], 1.0)
    assert nd.tolist() == [3, 2, 1] and idx.tolist() == [0, 2, 3]
    assert vgr.voxel_grid(c, 1.0)[0].tolist() == [0, 1, 2]
    # 2.5 truncates to 2
    assert vgr.grid(_c4([[0, 0, 0], [1.5, 0, 0]])[:, :3], 1.0)[1].tolist() == [2, 1, 1]
    # at 1e8 the float spacing is 8: 1 + maxB == maxB, so numDivX = 8 (1 + (maxB - minB) would say 9) and the last cell, i = 8,
    # aliases (0, 1): upstream's own index, kept as it is
    c = _c4([[1e8, 0, 0], [1e8 + 8, 0, 0], [1e8, 1, 0]])
    _, nd, idx = vgr.grid(c[:, :3], 1.0)
    assert nd.tolist() == [8, 2, 1] and idx.tolist() == [0, 8, 8]
    order, out, _ = vgr.voxel_grid(c, 1.0)
    assert order.tolist() == [0, 1] and out[1, 1] == F(0.5)


def test_negative_zero_member_keeps_its_sign():
    c = _c4([[-0.0, 5, 5], [-0.0, 5.2, 5.2], [3, 3, 3]])
    order, out, _ = vgr.voxel_grid(c, 1.0)
    # the sum starts from the first member (-0.0), not from 0: -0 + -0 = -0, and -0 / 2 = -0
    assert order.tolist() == [0, 2] and out[0, 0] == 0 and np.signbit(out[0, 0])
    c1 = _c4([[-0.0, 0, 0], [3, 3, 3]])
    _, out1, _ = vgr.voxel_grid(c1, 1.0)
    assert np.signbit(out1[0, 0]) and not np.signbit(out1[0, 1])


def test_planar_cloud_is_the_2d_formula():
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-7, 9, (3000, 3)).astype(F)
    xyz[:, 2] = 0
    c = _c4(xyz)
    _, nd, _ = vgr.grid(xyz, [0.5, 0.7, 0.3])
    assert nd[2] == 1
    order, out, _ = vgr.voxel_grid(c, [0.5, 0.7, 0.3])
    o2, out2 = vgr.planar_voxel_grid_2d(c, 0.5, 0.7)
    assert np.array_equal(order, o2) and np.array_equal(out.view(np.uint32), out2.view(np.uint32))


def test_descriptors_averaged_or_first_and_limits():
    c = _c4([[0.1, 0, 0], [0.2, 0, 0], [0.4, 0, 0], [5, 0, 0]])
    d = np.array([[1, 10], [2, 20], [4, 40], [7, 70]], F)
    _, _, da = vgr.voxel_grid(c, 1.0, True, d)
    _, _, df = vgr.voxel_grid(c, 1.0, False, d)
    assert np.array_equal(da, [[((F(1) + F(2)) + F(4)) / F(3), ((F(10) + F(20)) + F(40)) / F(3)], [7, 70]])
    assert np.array_equal(df, [[1, 10], [7, 70]])
    for bad in ([0, 1, 1], [1, -1, 1], [1, 1, np.inf], [np.nan, 1, 1]):
        with pytest.raises(vgr.VoxelGridLimit):
            vgr.voxel_grid(c, bad)
    with pytest.raises(vgr.VoxelGridLimit, match="2\\^24"):
        vgr.voxel_grid(_c4([[0, 0, 0], [2e7, 0, 0]]), 1.0)
    with pytest.raises(vgr.VoxelGridLimit, match="2\\^32"):
        vgr.voxel_grid(_c4([[0, 0, 0], [1e5, 1e5, 1e5]]), 1.0)
    with pytest.raises(vgr.VoxelGridLimit, match="non-finite"):
        vgr.voxel_grid(_c4([[0, 0, 0], [np.nan, 0, 0]]), 1.0)


# ---- the host shell (norlab_icp_mapper_amd/host): parameters, without a GPU context ----
@pytest.fixture(scope="module")
def host():
    import host_bindings as hb
    if not os.path.exists(hb.LIB):
        import __graft_entry__
        __graft_entry__.build()
    return hb


def test_host_accepts_the_filter_and_its_parameters(host):
    empty = np.zeros((0, 4), F)
    for y in ("[VoxelGridDataPointsFilter]",
              "[{VoxelGridDataPointsFilter: {vSizeX: 0.1, vSizeY: 0.3, vSizeZ: 2, useCentroid: 1, averageExistingDescriptors: 0}}]"):
        out, _, _ = host.filter_chain(y, empty)
        assert out.shape == (0, 4)


@pytest.mark.parametrize("params,msg", [
    ("{vSize: 0.2}", "unknown parameter vSize"),
    ("{minPointsPerVoxel: 2}", "unknown parameter minPointsPerVoxel"),
    ("{useCentroid: 0}", "useCentroid: 0"),
    ("{vSizeX: 0}", "finite and > 0"),
    ("{vSizeY: -0.5}", "finite and > 0"),
])
def test_host_rejects_bad_parameters(host, params, msg):
    with pytest.raises(RuntimeError, match=msg):
        host.filter_chain("[{VoxelGridDataPointsFilter: %s}]" % params, np.zeros((0, 4), F))


def test_host_needs_a_gpu_context(host):
    with pytest.raises(RuntimeError, match="needs a GPU context"):
        host.filter_chain("[{VoxelGridDataPointsFilter: {vSizeX: 0.5}}]", _c4([[0, 0, 0], [1, 1, 1]]))
