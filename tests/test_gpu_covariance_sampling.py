"""CovarianceSamplingDataPointsFilter on the device (icpmi_covariance_sampling, csrc/covsampling.hip) and in the host shell, against the
numpy restatement of the recalled formulation (tests/covariance_sampling_reference.py): the selection replayed from the device's own
centre, L and eigenbasis is the device's selection index for index; the basis itself agrees with numpy; the device's selection equals
the restatement's from scratch on non-degenerate scenes and on the bundled scans.  End to end: the config-4 replay with the filter in
`input:` equals the replay of scans sampled beforehand, and the filter runs among a registration's readingDataPointsFilters."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import covariance_sampling_reference as csr

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


_SCENES = {}


def _scene(n, seed=1):
    """points in an anisotropic box with random unit normals: every direction constrained, distinct eigenvalues"""
    if (n, seed) not in _SCENES:
        rng = np.random.default_rng(seed)
        xyz = rng.uniform([-30, -12, -3], [30, 12, 5], (n, 3))
        nrm = rng.normal(size=(n, 3)) * [1.0, 0.6, 1.4]
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        _SCENES[(n, seed)] = (_c4(xyz), nrm.astype(F))
    return _SCENES[(n, seed)]


def _replay_equal(icp, cloud, nrm, nb, tn):
    order, info = icp.covarianceSampling(cloud, nrm, nb, tn, with_info=True)
    assert order.dtype == np.int32 and order.shape == (nb,)
    ref, _ = csr.covariance_sampling(cloud, nrm, nb, tn, info=info)
    assert np.array_equal(order, ref), (np.nonzero(order != ref)[0][:5], order[:10], ref[:10])
    return order, info


@pytest.mark.parametrize("tn", [0, 1, 2])
@pytest.mark.parametrize("n", [1_000, 100_000])
def test_replay_from_the_device_basis_is_bit_exact(icp, n, tn):
    cloud, nrm = _scene(n)
    for nb in (1, 500, 5000, n - 1):
        if nb < n:
            _replay_equal(icp, cloud, nrm, nb, tn)


@pytest.mark.parametrize("nb,tn", [(1, 0), (500, 1), (5000, 2), (5000, 1), (999_999, 1)])
def test_replay_one_million_points(icp, nb, tn):
    cloud, nrm = _scene(1_000_000)
    _replay_equal(icp, cloud, nrm, nb, tn)


def test_replay_above_the_lds_bitmap(icp):
    # 2^20 + 50 000 points: the selected flags go to the global bitmap
    cloud, nrm = _scene((1 << 20) + 50_000, seed=2)
    for nb in (5000, 60_000):
        _replay_equal(icp, cloud, nrm, nb, 1)


@pytest.mark.parametrize("tn", [0, 1, 2])
def test_the_basis_is_right(icp, tn):
    cloud, nrm = _scene(100_000, seed=3)
    _, info = icp.covarianceSampling(cloud, nrm, 100, tn, with_info=True)
    c, L = csr.center_and_lnorm(cloud, tn)
    assert np.abs(info["center"] - c).max() <= 1e-12 * np.abs(c).max()
    assert abs(info["lnorm"] - L) <= 1e-12 * L
    Cn = csr.covariance(csr.vectors(cloud, nrm, info["center"], info["lnorm"]))
    X, ev = info["basis"], info["eigval"]
    Cd = (X * ev[None, :]) @ X.T                                            # C rebuilt from the device's eigenpairs
    assert np.abs(Cd - Cn).max() <= 1e-12 * np.abs(Cn).max()
    w, Y = np.linalg.eigh(Cn)
    assert (np.diff(ev) >= 0).all()
    assert np.abs(ev - w).max() <= 1e-9 * np.abs(w).max()
    assert np.abs(X.T @ X - np.eye(6)).max() < 1e-12
    gap = np.minimum(np.diff(np.r_[-np.inf, w]), np.diff(np.r_[w, np.inf])) / w.max()
    for k in range(6):
        if gap[k] > 1e-6:
            assert abs(X[:, k] @ Y[:, k]) >= 1 - 1e-9


@pytest.mark.parametrize("n,nb,tn", [(1_000, 500, 1), (100_000, 5000, 1), (100_000, 5000, 0), (100_000, 2000, 2), (1_000_000, 5000, 1)])
def test_end_to_end_synthetic(icp, n, nb, tn):
    cloud, nrm = _scene(n, seed=4)
    order = icp.covarianceSampling(cloud, nrm, nb, tn)
    ref, _ = csr.covariance_sampling(cloud, nrm, nb, tn)
    assert np.array_equal(order, ref)


@pytest.mark.parametrize("k", [0, 5, 13])
def test_end_to_end_bundled_scans(icp, scans, k):
    cloud = _c4(scans[f"scan{k}_xyz"])
    nrm = icp.surfaceNormals(cloud, 10)
    assert np.isfinite(nrm).all()
    for nb, tn in ((4000, 1), (1000, 2), (20_000, 0)):
        order = icp.covarianceSampling(cloud, nrm, nb, tn)
        ref, _ = csr.covariance_sampling(cloud, nrm, nb, tn)
        assert np.array_equal(order, ref), (k, nb, tn)


def test_two_calls_give_identical_output(icp, scans):
    cloud = _c4(np.concatenate([scans[f"scan{k}_xyz"] for k in range(6)]))
    nrm = icp.surfaceNormals(cloud, 10)
    a, ia = icp.covarianceSampling(cloud, nrm, 5000, 1, with_info=True)
    b, ib = icp.covarianceSampling(cloud, nrm, 5000, 1, with_info=True)
    assert np.array_equal(a, b)
    for key in ("center", "eigval", "basis"):
        assert np.array_equal(np.asarray(ia[key]).view(np.uint64), np.asarray(ib[key]).view(np.uint64))
    assert ia["lnorm"] == ib["lnorm"]


def test_small_and_degenerate_clouds(icp):
    cloud = _c4([[1, 2, 3]] * 10)
    nrm = np.tile(np.asarray([[0, 0, 1]], F), (10, 1))
    order, info = icp.covarianceSampling(cloud, nrm, 4, 1, with_info=True)   # every point equal: L = 1, not NaN
    assert info["lnorm"] == 1.0 and order.shape == (4,) and len(set(order.tolist())) == 4
    ref, _ = csr.covariance_sampling(cloud, nrm, 4, 1, info=info)
    assert np.array_equal(order, ref)
    from test_covariance_sampling_cpu import HAND_NRM, HAND_PICKS, HAND_XYZ
    assert icp.covarianceSampling(_c4(HAND_XYZ), np.asarray(HAND_NRM, F), 7, 0).tolist() == HAND_PICKS


def test_limits_and_errors(amd, icp):
    cloud, nrm = _scene(1_000, seed=5)
    # nbSample >= N: the cloud unchanged, normals or not
    for nb in (1000, 1001):
        assert icp.covarianceSampling(cloud, None, nb).tolist() == list(range(1000))
    assert icp.covarianceSampling(np.zeros((0, 4), F), None, 0).shape == (0,)
    assert icp.covarianceSampling(cloud, nrm, 0).shape == (0,)
    with pytest.raises(amd.InvalidField):
        icp.covarianceSampling(cloud, None, 999)
    with pytest.raises(amd.InvalidField):
        icp.covarianceSampling(cloud, None, 0)
    with pytest.raises(amd.InvalidParameter, match="nbSample"):
        icp.covarianceSampling(cloud, nrm, -1)
    for tn in (-1, 3):
        with pytest.raises(amd.InvalidParameter, match="torqueNorm"):
            icp.covarianceSampling(cloud, nrm, 10, tn)
    for arr, r, col in ((cloud, 17, 1), (nrm, 40, 2)):
        for bad in (np.nan, np.inf):
            a = arr.copy(); a[r, col] = bad
            with pytest.raises(amd.InvalidParameter, match="non-finite"):
                icp.covarianceSampling(a if arr is cloud else cloud, nrm if arr is cloud else a, 10)
    # more than 2^31 - 1 points: refused before anything is read
    lib = icp._lib
    order = np.empty(4, np.int32); m = C.c_int64(-1)
    st = lib.icpmi_covariance_sampling(icp._h, cloud.ctypes.data, 1 << 31, nrm.ctypes.data, 4, 1, order.ctypes.data, C.byref(m), None)
    assert st == amd._capi.ERR_UNSUPPORTED and m.value == 0
    planar = amd.ICPSequence(is_2d=1)
    with pytest.raises(amd.InvalidParameter, match="planar"):
        planar.covarianceSampling(cloud, nrm, 10)
    _replay_equal(icp, cloud, nrm, 100, 1)                                   # the handle is fine afterwards


# ---- the host shell ----
def _host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb


def _h(icp):
    return icp._h.value if hasattr(icp._h, "value") else icp._h


def test_host_filter_defaults_and_rejections(icp, scans):
    hb = _host()
    cloud = _c4(scans["scan2_xyz"])
    nrm = icp.surfaceNormals(cloud, 10)
    out, got_n, _ = hb.filter_chain("[CovarianceSamplingDataPointsFilter]", cloud, handle=_h(icp), desc_name="normals", desc=nrm)
    order = icp.covarianceSampling(cloud, nrm, 5000, 1)                      # nbSample 5000, torqueNorm 1
    assert out.shape[0] == 5000
    assert np.array_equal(out, cloud[order]) and np.array_equal(got_n, nrm[order])
    out, _, _ = hb.filter_chain("[{CovarianceSamplingDataPointsFilter: {nbSample: 700, torqueNorm: 2}}]", cloud, handle=_h(icp),
                                desc_name="normals", desc=nrm)
    assert np.array_equal(out, cloud[icp.covarianceSampling(cloud, nrm, 700, 2)])
    with pytest.raises(RuntimeError, match="unknown parameter"):
        hb.filter_chain("[{CovarianceSamplingDataPointsFilter: {nbSample: 10, seed: 1}}]", cloud, handle=_h(icp), desc_name="normals", desc=nrm)
    for bad in ("torqueNorm: 3", "nbSample: -2"):
        with pytest.raises(RuntimeError, match="torqueNorm|nbSample"):
            hb.filter_chain("[{CovarianceSamplingDataPointsFilter: {%s}}]" % bad, cloud, handle=_h(icp), desc_name="normals", desc=nrm)
    with pytest.raises(RuntimeError, match="normals"):
        hb.filter_chain("[{CovarianceSamplingDataPointsFilter: {nbSample: 10}}]", cloud, handle=_h(icp))
    out, _, _ = hb.filter_chain("[{CovarianceSamplingDataPointsFilter: {nbSample: %d}}]" % cloud.shape[0], cloud, handle=_h(icp))
    assert np.array_equal(out, cloud)                                        # nbSample >= N: unchanged, no normals needed


def test_host_filter_carries_descriptors_and_times(icp):
    hb = _host()
    lib = hb.load()
    fn = lib.nim_test_filter_chain_times
    fn.restype = C.c_int
    cloud, _ = _scene(40_000, seed=6)
    n = cloud.shape[0]
    d = np.random.default_rng(7).normal(size=(n, 4)).astype(F)
    t = (np.int64(1_700_000_000) * 10**9 + np.arange(2 * n, dtype=np.int64) * 997).reshape(n, 2)
    out = np.empty_like(cloud); dout = np.empty_like(d); tout = np.empty_like(t); m = C.c_int64(0); err = C.create_string_buffer(512)
    y = "[{SurfaceNormalDataPointsFilter: {knn: 10}}, {CovarianceSamplingDataPointsFilter: {nbSample: 3000, torqueNorm: 1}}]"
    rc = fn(C.c_void_p(_h(icp)), y.encode(), C.c_void_p(cloud.ctypes.data), C.c_int64(n), b"stuff", C.c_int(4), C.c_void_p(d.ctypes.data),
            b"stamps", C.c_int(2), C.c_void_p(t.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(dout.ctypes.data),
            C.c_void_p(tout.ctypes.data), C.byref(m), err, 512)
    assert rc == 0, err.value
    order = icp.covarianceSampling(cloud, icp.surfaceNormals(cloud, 10), 3000, 1)
    assert m.value == 3000
    assert np.array_equal(out[:3000], cloud[order]) and np.array_equal(dout[:3000], d[order]) and np.array_equal(tout[:3000], t[order])


# ---- end to end ----
CS_CHAIN = ("  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
            "  - CovarianceSamplingDataPointsFilter:\n      nbSample: 4000\n")


def _write_binary_vtk(path, xyz, nrm):
    xyz = np.ascontiguousarray(xyz, F)
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\nFile created by libpointmatcher\nBINARY\nDATASET POLYDATA\n")
        f.write(f"POINTS {xyz.shape[0]} float\n".encode())
        f.write(xyz.astype(">f4").tobytes())
        f.write(f"\nPOINT_DATA {xyz.shape[0]}\nNORMALS normals float\n".encode())
        f.write(np.ascontiguousarray(nrm, F).astype(">f4").tobytes())
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


def test_config4_with_covariance_sampling_input_equals_presampled_scans(tmp_path, icp, scans):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    _host()
    assert "input:\n" in CONFIG4_YAML
    a = str(tmp_path / "filter"); b = str(tmp_path / "presampled")
    os.makedirs(a); os.makedirs(b)
    names, _ = write_bundled_dataset(a, scans)
    poses_a = _replay(a, CONFIG4_YAML.replace("input:\n", "input:\n" + CS_CHAIN, 1))
    # the same scans after the mapper's sensor-range cut (sensorMaxRange 200, ahead of input:), normals (knn 10) and sampling through
    # the Python API, written in binary with their normals, so that every float32 comes back as it left
    write_bundled_dataset(b, scans)
    for k, name in enumerate(names):
        xyz = scans[f"scan{k}_xyz"].astype(F)
        r = np.sqrt(xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1] + xyz[:, 2] * xyz[:, 2])
        c = _c4(xyz[r < F(200)])
        nrm = icp.surfaceNormals(c, 10)
        order = icp.covarianceSampling(c, nrm, 4000, 1)
        _write_binary_vtk(os.path.join(b, "scans", name), c[order, :3], nrm[order])
    poses_b = _replay(b, CONFIG4_YAML)
    assert np.array_equal(poses_a, poses_b), np.abs(poses_a - poses_b).max()


def test_config4_with_covariance_sampling_among_the_reading_filters(tmp_path, scans):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    _host()
    a = str(tmp_path / "plain"); b = str(tmp_path / "sampled")
    os.makedirs(a); os.makedirs(b)
    write_bundled_dataset(a, scans)
    write_bundled_dataset(b, scans)
    assert "icp:\n" in CONFIG4_YAML and "readingDataPointsFilters" not in CONFIG4_YAML
    chain = "  readingDataPointsFilters:\n" + CS_CHAIN.replace("  - ", "    - ").replace("      ", "        ")
    poses_a = _replay(a, CONFIG4_YAML)
    poses_b = _replay(b, CONFIG4_YAML.replace("icp:\n", "icp:\n" + chain, 1))
    assert np.isfinite(poses_b).all()
    assert not np.array_equal(poses_a, poses_b)                              # the readings were sampled
    assert np.abs(poses_a[:, :3] - poses_b[:, :3]).max() < 0.25              # and the trajectory is the same one
