"""VoxelGridDataPointsFilter on the device (icpmi_voxel_grid, csrc/voxelgrid.hip) and in the host shell, compared BIT FOR BIT with the
numpy restatement of the recalled formulation (tests/voxel_grid_reference.py): the kept first points, their order, the centroids and
the descriptor rows.  End to end: the config-4 replay with the filter in `input:` equals the replay of scans voxelised beforehand, and
a VoxelGrid among the ICP's referenceDataPointsFilters leaves the centred centroids plus the mean in the index."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import voxel_grid_reference as vgr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "norlab_icp_mapper_amd")
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def icp(amd):
    return amd.ICPSequence()


@pytest.fixture(scope="module")
def scans():
    return np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))


def _c4(xyz):
    xyz = np.asarray(xyz, F)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, F).view(np.uint32)


def _same(icp, cloud, vsize, average=True, desc=None):
    order, out4, dout = icp.voxelGrid(cloud, vsize, average_descriptors=average, descriptors=desc)
    o2, out2, d2 = vgr.voxel_grid(cloud, vsize, average, desc)
    assert np.array_equal(order, o2), (order[:10], o2[:10])
    assert np.array_equal(_bits(out4), _bits(out2))
    if desc is None:
        assert dout is None
    else:
        assert np.array_equal(_bits(dout), _bits(d2.reshape(dout.shape)))
    return order, out4, dout


def _uniform(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return _c4(rng.uniform(lo, hi, (n, 3)))


@pytest.mark.parametrize("vs", [0.1, 0.3, 1.0, [0.1, 0.3, 0.7], [0.3, 0.1, 0.05]])
def test_uniform_and_anisotropic(icp, vs):
    _same(icp, _uniform(100_000, [-10, -6, -2], [10, 6, 2], 1), vs)


@pytest.mark.parametrize("k", [0, 5, 13])
@pytest.mark.parametrize("vs", [0.1, 0.3, 1.0])
def test_bundled_lidar_scans(icp, scans, k, vs):
    _same(icp, _c4(scans[f"scan{k}_xyz"]), vs)


def test_negative_coordinates_and_negative_zero(icp):
    _same(icp, _uniform(50_000, [-80, -60, -9], [-20, -30, -1], 2), [0.3, 0.2, 0.1])
    c = _c4([[-0.0, 5, 5], [-0.0, 5.2, 5.2], [3, 3, 3], [-0.0, -0.0, -0.0]])
    order, out, _ = _same(icp, c, 1.0)
    assert np.signbit(out[0, 0])


def test_one_voxel_and_every_point_its_own_voxel(icp):
    order, out, _ = _same(icp, _uniform(20_000, 0, 0.5, 3), 10.0)
    assert order.tolist() == [0]
    g = np.stack(np.meshgrid(*[np.arange(20, dtype=F)] * 3, indexing="ij"), -1).reshape(-1, 3) + F(0.5)
    g = g[np.random.default_rng(4).permutation(g.shape[0])]
    order, out, _ = _same(icp, _c4(g), 1.0)
    assert order.tolist() == list(range(g.shape[0]))


def test_duplicates_one_point_no_point_and_the_float_boundaries(icp):
    rng = np.random.default_rng(5)
    dup = _c4(rng.integers(0, 4, (5_000, 3)).astype(F) * F(0.5))
    _same(icp, dup, 0.5)
    _same(icp, dup, 0.7)
    _same(icp, _c4([[1.0, 2.0, 3.0]]), 0.1)
    order, out, dout = icp.voxelGrid(np.zeros((0, 4), F), 0.1)
    assert order.shape == (0,) and out.shape == (0, 4) and dout is None
    _same(icp, _c4([[0, 0, 0], [2, 0, 0], [0, 1, 0]]), 1.0)              # (1 + maxB) - minB exactly 3
    _same(icp, _c4([[1e8, 0, 0], [1e8 + 8, 0, 0], [1e8, 1, 0]]), 1.0)    # 1 + maxB == maxB: upstream's aliasing index, kept


def test_planar_cloud(icp):
    c = _uniform(30_000, -15, 15, 6)
    c[:, 2] = 0
    order, out, _ = _same(icp, c, [0.4, 0.25, 0.1])
    o2, out2 = vgr.planar_voxel_grid_2d(c, 0.4, 0.25)
    assert np.array_equal(order, o2) and np.array_equal(_bits(out), _bits(out2))


@pytest.mark.parametrize("vs", [0.05, 50.0])
def test_one_million_points(icp, vs):
    c = _uniform(1_000_000, [-40, -40, -3], [40, 40, 3], 7)
    order, out, _ = _same(icp, c, vs)
    if vs == 50.0:
        assert order.shape[0] <= 8                                          # a few voxels of ~10^5 points: the long serial sums


@pytest.mark.parametrize("rows", [1, 3, 4])
@pytest.mark.parametrize("average", [True, False])
def test_descriptors(icp, rows, average):
    c = _uniform(60_000, [-5, -5, -1], [5, 5, 1], 8)
    d = np.random.default_rng(9).normal(size=(60_000, rows)).astype(F)
    _same(icp, c, 0.25, average, d[:, 0] if rows == 1 else d)


def test_limits_are_rejected(amd, icp):
    c = _uniform(1000, 0, 1, 10)
    for vs in ([0, 1, 1], [1, -0.5, 1], [1, 1, np.inf], [np.nan, 1, 1]):
        with pytest.raises(amd.InvalidParameter, match="finite and > 0"):
            icp.voxelGrid(c, vs)
    bad = c.copy(); bad[17, 1] = np.nan
    with pytest.raises(amd.InvalidParameter, match="non-finite"):
        icp.voxelGrid(bad, 0.1)
    bad[17, 1] = np.inf
    with pytest.raises(amd.InvalidParameter, match="non-finite"):
        icp.voxelGrid(bad, 0.1)
    with pytest.raises(amd.InvalidParameter, match="2\\^24"):
        icp.voxelGrid(_c4([[0, 0, 0], [2e7, 0, 0]]), 1.0)
    with pytest.raises(amd.InvalidParameter, match="2\\^32"):
        icp.voxelGrid(_c4([[0, 0, 0], [1e5, 1e5, 1e5]]), 1.0)
    _same(icp, c, 0.05)                                                     # the handle is fine afterwards


def test_two_calls_give_identical_bits(icp, scans):
    c = _c4(np.concatenate([scans[f"scan{k}_xyz"] for k in range(6)]))
    d = np.random.default_rng(12).normal(size=(c.shape[0], 3)).astype(F)
    a = icp.voxelGrid(c, 0.3, descriptors=d)
    b = icp.voxelGrid(c, 0.3, descriptors=d)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)


# ---- the host shell ----
def _host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb


def test_host_filter_with_a_live_handle(icp, scans):
    hb = _host()
    c = _c4(scans["scan3_xyz"])
    h = icp._h.value if hasattr(icp._h, "value") else icp._h
    nrm = np.random.default_rng(13).normal(size=(c.shape[0], 3)).astype(F)
    for avg in (1, 0):
        y = "[{VoxelGridDataPointsFilter: {vSizeX: 0.3, vSizeY: 0.2, vSizeZ: 0.1, averageExistingDescriptors: %d}}]" % avg
        out, got_n, _ = hb.filter_chain(y, c, handle=h, desc_name="normals", desc=nrm)
        o2, out2, d2 = vgr.voxel_grid(c, [0.3, 0.2, 0.1], bool(avg), nrm)
        assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(_bits(got_n), _bits(d2))
    # the filter is legal in readingStepDataPointsFilters (repeatable) and leaves `post:`-style chains to the host path
    out, _, _ = hb.filter_chain("[{VoxelGridDataPointsFilter: {vSizeX: 0.5, vSizeY: 0.5, vSizeZ: 0.5}}, {MaxDistDataPointsFilter: {maxDist: 30}}]",
                                c, handle=h)
    _, v, _ = vgr.voxel_grid(c, 0.5)
    r = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    assert np.array_equal(_bits(out), _bits(v[r < 30]))


def test_host_filter_keeps_the_first_points_times_and_packs_several_descriptors(icp):
    hb = _host()
    lib = hb.load()
    fn = lib.nim_test_filter_chain_times
    fn.restype = C.c_int
    c = _uniform(40_000, [-8, -8, -1], [8, 8, 1], 14)
    n = c.shape[0]
    d = np.random.default_rng(15).normal(size=(n, 4)).astype(F)
    t = (np.int64(1_700_000_000) * 10**9 + np.arange(2 * n, dtype=np.int64) * 997).reshape(n, 2)
    h = icp._h.value if hasattr(icp._h, "value") else icp._h
    for avg in (1, 0):
        out = np.empty_like(c); dout = np.empty_like(d); tout = np.empty_like(t); m = C.c_int64(0); err = C.create_string_buffer(512)
        y = "[{VoxelGridDataPointsFilter: {vSizeX: 0.4, vSizeY: 0.4, vSizeZ: 0.4, averageExistingDescriptors: %d}}]" % avg
        rc = fn(C.c_void_p(h), y.encode(), C.c_void_p(c.ctypes.data), C.c_int64(n), b"stuff", C.c_int(4), C.c_void_p(d.ctypes.data), b"stamps",
                C.c_int(2), C.c_void_p(t.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(dout.ctypes.data), C.c_void_p(tout.ctypes.data),
                C.byref(m), err, 512)
        assert rc == 0, err.value
        k = m.value
        o2, out2, d2 = vgr.voxel_grid(c, 0.4, bool(avg), d)
        assert k == o2.shape[0]
        assert np.array_equal(_bits(out[:k]), _bits(out2)) and np.array_equal(_bits(dout[:k]), _bits(d2))
        assert np.array_equal(tout[:k], t[o2])


# ---- end to end ----
VG_INPUT = "  - VoxelGridDataPointsFilter:\n      vSizeX: 0.2\n      vSizeY: 0.2\n      vSizeZ: 0.2\n"


def _write_binary_vtk(path, xyz):
    xyz = np.ascontiguousarray(xyz, F)
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nFile created by libpointmatcher\nBINARY\nDATASET POLYDATA\n")
        f.write(f"POINTS {xyz.shape[0]} float\n".encode())
        f.write(xyz.astype(">f4").tobytes())
        f.write(b"\n")


def _replay(tmp, cfg_text):
    from test_host_cpp import _read_vtk
    cfg = os.path.join(tmp, "config.yaml")
    open(cfg, "w").write(cfg_text)
    traj_out = os.path.join(tmp, "traj.vtk")
    out = subprocess.run([os.path.join(PKG, "build_map_from_scans_and_trajectory"), tmp, cfg, traj_out], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr + out.stdout
    pos, desc = _read_vtk(traj_out)
    assert pos.shape[0] == 14
    return np.concatenate([pos, desc["orientationX"], desc["orientationY"], desc["orientationZ"]], 1)


def test_config4_with_voxel_grid_input_equals_prevoxelised_scans(tmp_path, scans):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    _host()
    assert "input:\n" in CONFIG4_YAML
    a = str(tmp_path / "filter"); b = str(tmp_path / "prevoxelised")
    os.makedirs(a); os.makedirs(b)
    names, _ = write_bundled_dataset(a, scans)
    poses_a = _replay(a, CONFIG4_YAML.replace("input:\n", "input:\n" + VG_INPUT, 1))
    # the same scans, voxelised by the restatement after the mapper's sensor-range cut (sensorMaxRange 200, Mapper.cpp:174) and written
    # in binary, so that every float32 comes back as it left
    write_bundled_dataset(b, scans)
    for k, name in enumerate(names):
        xyz = scans[f"scan{k}_xyz"].astype(F)
        r = np.sqrt(xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1] + xyz[:, 2] * xyz[:, 2])
        _, v, _ = vgr.voxel_grid(_c4(xyz[r < F(200)]), 0.2)
        rv = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        assert (rv < F(200)).all()                                           # the second replay's range cut keeps every centroid
        _write_binary_vtk(os.path.join(b, "scans", name), v[:, :3])
    poses_b = _replay(b, CONFIG4_YAML)
    assert np.array_equal(poses_a, poses_b), np.abs(poses_a - poses_b).max()


def test_voxel_grid_among_the_reference_filters_indexes_centred_centroids_plus_mean(scans):
    hb = _host()
    lib = hb.load()
    fn = lib.nim_test_icp_set_map
    fn.restype = C.c_int
    c = _c4(np.concatenate([scans[f"scan{k}_xyz"] for k in range(3)]))
    n = c.shape[0]
    y = ("referenceDataPointsFilters:\n  - VoxelGridDataPointsFilter:\n      vSizeX: 0.3\n      vSizeY: 0.3\n      vSizeZ: 0.3\n"
         "      averageExistingDescriptors: 0\n")
    out = np.empty_like(c); m = C.c_int64(0); err = C.create_string_buffer(512)
    rc = fn(y.encode(), C.c_void_p(c.ctypes.data), C.c_int64(n), C.c_void_p(out.ctypes.data), C.byref(m), err, 512)
    assert rc == 0, err.value
    # setMap: the mean in double (sequential), the centred copy in float, the filter, then the mean added back
    mean = np.cumsum(c[:, :3].astype(np.float64), axis=0)[-1] / n
    centred = c.copy()
    centred[:, :3] = (c[:, :3].astype(np.float64) - mean).astype(F)
    order, v, _ = vgr.voxel_grid(centred, 0.3)
    want = (v[:, :3].astype(np.float64) + mean).astype(F)
    got = out[:m.value]
    assert got.shape[0] == want.shape[0]
    assert np.array_equal(_bits(got[:, :3]), _bits(want))
    # what carrying the original coordinates along would have given (the first members): not what the index holds
    assert not np.array_equal(got[:, :3], c[order, :3])
