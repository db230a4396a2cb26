"""NormalSpaceDataPointsFilter on the device (icpmi_normal_space_sampling, csrc/normalspace.hip) and in the host shell, against the
numpy restatement of the recalled formulation (tests/normal_space_reference.py).  The test normals come from nsr.safe_normals, which
rejects while generating every normal closer than 1e-3 buckets to a bucket edge (tests/test_normal_space_cpu.py holds it to that): on
them the device's buckets and its order equal the restatement's from scratch, index for index, with no point left out; and for every
case the restatement replayed from the device's buckets is the device's order.  The hand-picked normals (poles, zero, ny = -0.0) have
angles that are exactly 0, pi / 2 or pi on both sides, so they are compared in full as well.  On a bundled scan with the device's own
normals the buckets may differ only at points within 1e-4 buckets of an edge, at no more than 0.2 % of the points.  End to end: the
config-4 replay (three scans) with the filter in `input:` equals the replay of scans sampled beforehand, and the filter runs, repeatably,
among a registration's readingDataPointsFilters."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import normal_space_reference as nsr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "norlab_icp_mapper_amd")
F = np.float32
SIZES = [2, 63, 64, 65, 255, 256, 257, 1025, 4097]


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


_CLOUDS = {}


def _cloud(n):
    """n points in a box with safe random normals (clear of every bucket edge for the three epsilons), generated once per size"""
    if n not in _CLOUDS:
        rng = np.random.default_rng(1000 + n)
        _CLOUDS[n] = (_c4(rng.uniform([-30, -12, -3], [30, 12, 5], (n, 3))), nsr.safe_normals(rng, n))
    return _CLOUDS[n]


def _xyz(n, seed=3):
    return _c4(np.random.default_rng(seed).uniform(-10, 10, (n, 3)))


def _check(icp, cloud, nrm, nb, eps, seed=1, scratch=True):
    """the device's order equals the restatement replayed from the device's buckets, and -- scratch -- its buckets and order equal the
    restatement's own"""
    n = cloud.shape[0]
    order, dev_b = icp.normalSpaceSampling(cloud, nrm, nb, seed, eps, with_buckets=True)
    assert order.dtype == np.int32 and order.shape == (min(nb, n),)
    if nb == 0 or nb >= n:
        assert dev_b is None and order.tolist() == list(range(min(nb, n)) if nb >= n else [])
        return order
    assert dev_b.dtype == np.int32 and dev_b.shape == (n,) and dev_b.min() >= 0 and dev_b.max() < nsr.table_size(eps)
    replay, _ = nsr.normal_space_sampling(cloud, nrm, nb, seed, eps, buckets=dev_b)
    assert np.array_equal(order, replay), (n, nb, eps, np.nonzero(order != replay)[0][:5])
    if scratch:
        ref, ref_b = nsr.normal_space_sampling(cloud, nrm, nb, seed, eps)
        assert np.array_equal(dev_b, ref_b), (n, nb, eps, np.nonzero(dev_b != ref_b)[0][:5])
        assert np.array_equal(order, ref)
    return order


@pytest.mark.parametrize("eps", nsr.EPSILONS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_from_scratch_and_replayed(icp, n, eps):
    cloud, nrm = _cloud(n)
    for nb in (1, n // 3, n - 1):
        _check(icp, cloud, nrm, nb, eps)


@pytest.mark.parametrize("eps", nsr.EPSILONS)
def test_one_hundred_thousand_points(icp, eps):
    cloud, nrm = _cloud(100_000)
    nb = {0.04908: 1, 0.09817: 100_000 // 3, 3.14159: 99_999}[eps]
    _check(icp, cloud, nrm, nb, eps)
    if eps == 0.09817:
        for nb in (1, 5000, 99_999):
            _check(icp, cloud, nrm, nb, eps, seed=77)


@pytest.mark.parametrize("eps", nsr.EPSILONS)
def test_all_normals_equal_is_a_random_subset(icp, eps):
    n = 1000
    nrm = np.tile(nsr.safe_normals(np.random.default_rng(11), 1), (n, 1))
    for nb in (1, 333, n - 1):
        order = _check(icp, _xyz(n), nrm, nb, eps, seed=5)
        assert order.tolist() == sorted(np.argsort(nsr.minstd(5, n))[:nb].tolist())   # one bucket: the nb smallest r_i


def test_one_point_per_bucket_keeps_the_first_buckets(icp):
    eps = 0.09817
    cand = nsr.safe_normals(np.random.default_rng(12), 3000)
    _, first = np.unique(nsr.buckets_of(cand, eps), return_index=True)
    nrm = np.ascontiguousarray(cand[np.random.default_rng(13).permutation(first)[:300]])      # 300 points, 300 buckets, shuffled
    b = nsr.buckets_of(nrm, eps)
    assert np.unique(b).size == 300
    for nb in (1, 100, 299):
        order = _check(icp, _xyz(300), nrm, nb, eps)
        assert order.tolist() == sorted(np.argsort(b)[:nb].tolist())         # R* = 0: the nb lowest buckets


@pytest.mark.parametrize("eps", nsr.EPSILONS)
def test_populations_one_and_n_minus_one(icp, eps):
    two = nsr.safe_normals(np.random.default_rng(14), 64)
    b = nsr.buckets_of(two, eps)
    other = int(np.nonzero(b != b[0])[0][0])
    for n in (2, 257, 1025):
        for single_at in (0, n // 2, n - 1):
            nrm = np.tile(two[0:1], (n, 1))
            nrm[single_at] = two[other]
            for nb in sorted({1, 2, n // 3, n - 1} - {0, n}):
                order = _check(icp, _xyz(n), nrm, nb, eps)
                assert nb < 2 or single_at in order.tolist()                 # the single point goes in round one


def test_rounds_that_end_exactly(icp):
    eps = 0.09817
    four = nsr.safe_normals(np.random.default_rng(15), 400)
    _, first = np.unique(nsr.buckets_of(four, eps), return_index=True)
    nrm = np.ascontiguousarray(np.repeat(four[first[:4]], 50, axis=0)[np.random.default_rng(16).permutation(200)])
    b = nsr.buckets_of(nrm, eps)
    for nb in (4, 120, 196, 122, 199):                                       # S(1), S(30), S(49) exactly; rem 2; rem 3
        order = _check(icp, _xyz(200), nrm, nb, eps)
        per = np.bincount(b[order], minlength=b.max() + 1)[np.unique(b)]
        assert per.max() - per.min() == (0 if nb % 4 == 0 else 1) and (np.diff(per) <= 0).all()   # the extra point goes to the lowest buckets


@pytest.mark.parametrize("eps", nsr.EPSILONS)
def test_poles_zero_normals_and_negative_zero(icp, eps):
    cloud, nrm = _cloud(1025)
    nrm = nrm.copy()
    nrm[0:40] = [0, 0, 1]; nrm[40:70] = [0, 0, -1]; nrm[70:100] = [0, 0, 0]
    nrm[100:120] = [-1, -0.0, 0]; nrm[120:130] = [-1, 0.0, 0]; nrm[130:140] = [0, 0, 3.5]; nrm[140:150] = [0, -0.0, -2]
    assert np.signbit(nrm[100, 1]) and not np.signbit(nrm[120, 1])
    _, dev_b = icp.normalSpaceSampling(cloud, nrm, 10, 1, eps, with_buckets=True)
    assert len(set(dev_b[0:40].tolist()) | set(dev_b[130:140].tolist())) == 1 and dev_b[0] == 0   # nz clamped to 1: theta 0, phi 0
    assert dev_b[40] == dev_b[140] and dev_b[100] == dev_b[120]             # atan2(-0, -1) + 2 pi and atan2(+0, -1) are both pi
    for nb in (1, 341, 1024):
        _check(icp, cloud, nrm, nb, eps)


def test_bundled_scan_with_the_devices_own_normals(icp, scans):
    cloud = _c4(scans["scan0_xyz"])
    n = cloud.shape[0]
    nrm = icp.surfaceNormals(cloud, 10)
    assert np.isfinite(nrm).all()
    for eps in nsr.EPSILONS:
        for nb in (1, 5000, n // 3, n - 1):
            _check(icp, cloud, nrm, nb, eps, scratch=False)                  # replay from the device's buckets: exact
        _, dev_b = icp.normalSpaceSampling(cloud, nrm, 5000, 1, eps, with_buckets=True)
        differ = dev_b != nsr.buckets_of(nrm, eps)
        margin = nsr.edge_margin(nrm, eps)
        print(f"scan0, epsilon {eps}: {int(differ.sum())} of {n} buckets differ; {int((margin < 1e-4).sum())} points within 1e-4 of an edge")
        assert (margin[differ] < 1e-4).all(), (eps, margin[differ].max())
        assert differ.sum() <= 0.002 * n, (eps, int(differ.sum()), n)


def test_two_calls_give_identical_output(icp, scans):
    cloud = _c4(np.concatenate([scans[f"scan{k}_xyz"] for k in range(3)]))
    nrm = icp.surfaceNormals(cloud, 10)
    a, ba = icp.normalSpaceSampling(cloud, nrm, 5000, 1, 0.09817, with_buckets=True)
    other = icp.normalSpaceSampling(cloud[:7777], nrm[:7777], 100)           # another size in between: the scratch is reused
    assert other.shape == (100,)
    b, bb = icp.normalSpaceSampling(cloud, nrm, 5000, 1, 0.09817, with_buckets=True)
    assert np.array_equal(a, b) and np.array_equal(ba, bb)
    for seed in (0, 2147483647):
        assert np.array_equal(icp.normalSpaceSampling(cloud, nrm, 5000, seed), a)     # the same minstd state as seed 1
    assert not np.array_equal(icp.normalSpaceSampling(cloud, nrm, 5000, 2), a)


def test_statuses_and_their_texts(amd, icp):
    cloud, nrm = _cloud(1025)
    n = cloud.shape[0]
    lib, cap = icp._lib, amd._capi

    def raw(n_arg, nptr, nb, seed, eps, handle=None):
        order = np.full(n, -7, np.int32); m = C.c_int64(-1)
        h = icp._h if handle is None else handle
        st = lib.icpmi_normal_space_sampling(h, cloud.ctypes.data, n_arg, nptr, nb, seed, C.c_float(eps), order.ctypes.data, C.byref(m), None)
        return st, m.value, order, lib.icpmi_last_error(h).decode()

    # nbSample >= N: the identity order, normals or not
    for nb in (n, n + 1, 1 << 40):
        st, m, order, _ = raw(n, None, nb, 1, 0.09817)
        assert st == cap.ICPMI_OK and m == n and order.tolist() == list(range(n))
        assert icp.normalSpaceSampling(cloud, None, nb).tolist() == list(range(n))
    assert icp.normalSpaceSampling(np.zeros((0, 4), F), None, 0).shape == (0,)
    st, m, order, _ = raw(n, nrm.ctypes.data, 0, 1, 0.09817)                 # nbSample == 0: empty
    assert st == cap.ICPMI_OK and m == 0 and (order == -7).all()
    st, m, _, msg = raw(n, nrm.ctypes.data, -1, 1, 0.09817)
    assert st == cap.ERR_INVALID_ARG and m == 0 and msg == "normal_space_sampling: nbSample must be >= 0"
    st, m, _, msg = raw(n, nrm.ctypes.data, 10, -1, 0.09817)
    assert st == cap.ERR_INVALID_ARG and msg == "normal_space_sampling: seed must be in [0, 2147483647]"
    for eps in (0.04907, 3.1416, float("nan"), 0.0, -1.0, float("inf")):
        st, m, _, msg = raw(n, nrm.ctypes.data, 10, 1, eps)
        assert st == cap.ERR_INVALID_ARG and m == 0 and msg == "normal_space_sampling: epsilon must be in [0.04908, 3.14159]", eps
    st, m, _, msg = raw(n, None, n - 1, 1, 0.09817)
    assert st == cap.ERR_MISSING_NORMALS and m == 0 and msg == "normal_space_sampling: the cloud has no normals (InvalidField normals)"
    st, m, _, msg = raw(1 << 31, nrm.ctypes.data, 4, 1, 0.09817)             # refused before anything is read
    assert st == cap.ERR_UNSUPPORTED and m == 0 and msg == "normal_space_sampling: more than 2^31 - 1 points"
    planar = amd.ICPSequence(is_2d=1)
    st, m, _, msg = raw(n, nrm.ctypes.data, 10, 1, 0.09817, handle=planar._h)
    assert st == cap.ERR_INVALID_ARG and msg.startswith("normal_space_sampling: planar (2-D) clouds are not supported")
    for arr, r, col in ((cloud, 17, 1), (nrm, 40, 2), (nrm, 1024, 0)):
        for bad in (np.nan, np.inf, -np.inf):
            a = arr.copy(); a[r, col] = bad
            with pytest.raises(amd.InvalidParameter, match="normal_space_sampling: the cloud has non-finite coordinates or normals"):
                icp.normalSpaceSampling(a if arr is cloud else cloud, nrm if arr is cloud else a, 10)
    with pytest.raises(amd.InvalidField):
        icp.normalSpaceSampling(cloud, None, 10)
    with pytest.raises(amd.InvalidParameter, match="nbSample"):
        icp.normalSpaceSampling(cloud, nrm, -1)
    with pytest.raises(amd.InvalidParameter, match="planar"):
        planar.normalSpaceSampling(cloud, nrm, 10)
    _check(icp, cloud, nrm, 100, 0.09817)                                    # the handle is fine afterwards


# ---- the host shell ----
def _host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb


def _h(icp):
    return icp._h.value if hasattr(icp._h, "value") else icp._h


def test_host_filter_defaults_and_parameters(icp, scans):
    hb = _host()
    cloud = _c4(scans["scan2_xyz"])
    nrm = icp.surfaceNormals(cloud, 10)
    out, got_n, _ = hb.filter_chain("[NormalSpaceDataPointsFilter]", cloud, handle=_h(icp), desc_name="normals", desc=nrm)
    order = icp.normalSpaceSampling(cloud, nrm, 5000, 1, 0.09817)            # nbSample 5000, seed 1, epsilon 0.09817
    assert out.shape[0] == 5000 and (np.diff(order) > 0).all()
    assert np.array_equal(out, cloud[order]) and np.array_equal(got_n, nrm[order])
    out, _, _ = hb.filter_chain("[{NormalSpaceDataPointsFilter: {nbSample: 700, seed: 9, epsilon: 0.2}}]", cloud, handle=_h(icp),
                                desc_name="normals", desc=nrm)
    assert np.array_equal(out, cloud[icp.normalSpaceSampling(cloud, nrm, 700, 9, 0.2)])
    with pytest.raises(RuntimeError, match="normals"):
        hb.filter_chain("[{NormalSpaceDataPointsFilter: {nbSample: 10}}]", cloud, handle=_h(icp))
    out, _, _ = hb.filter_chain("[{NormalSpaceDataPointsFilter: {nbSample: %d}}]" % cloud.shape[0], cloud, handle=_h(icp))
    assert np.array_equal(out, cloud)                                        # nbSample >= N: unchanged, no normals needed


def test_host_chain_carries_descriptors_and_times(icp):
    hb = _host()
    lib = hb.load()
    fn = lib.nim_test_filter_chain_times
    fn.restype = C.c_int
    cloud, _ = _cloud(100_000)
    cloud = cloud[:40_000]
    n = cloud.shape[0]
    d = np.random.default_rng(7).normal(size=(n, 4)).astype(F)
    t = (np.int64(1_700_000_000) * 10**9 + np.arange(2 * n, dtype=np.int64) * 997).reshape(n, 2)
    out = np.empty_like(cloud); dout = np.empty_like(d); tout = np.empty_like(t); m = C.c_int64(0); err = C.create_string_buffer(512)
    y = "[{SurfaceNormalDataPointsFilter: {knn: 10}}, {NormalSpaceDataPointsFilter: {nbSample: 3000, seed: 4}}]"
    rc = fn(C.c_void_p(_h(icp)), y.encode(), C.c_void_p(cloud.ctypes.data), C.c_int64(n), b"stuff", C.c_int(4), C.c_void_p(d.ctypes.data),
            b"stamps", C.c_int(2), C.c_void_p(t.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(dout.ctypes.data),
            C.c_void_p(tout.ctypes.data), C.byref(m), err, 512)
    assert rc == 0, err.value
    order = icp.normalSpaceSampling(cloud, icp.surfaceNormals(cloud, 10), 3000, 4)
    assert m.value == 3000
    assert np.array_equal(out[:3000], cloud[order]) and np.array_equal(dout[:3000], d[order]) and np.array_equal(tout[:3000], t[order])


# ---- end to end: three scans of the config-4 replay ----
NS_CHAIN = ("  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
            "  - NormalSpaceDataPointsFilter:\n      nbSample: 4000\n")
N_SCANS = 3


def _three(scans):
    z = {f"scan{k}_xyz": scans[f"scan{k}_xyz"] for k in range(N_SCANS)}
    z["scan_names"] = scans["scan_names"][:N_SCANS]
    z["trajectory"] = scans["trajectory"][:N_SCANS]
    return z


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
                         timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    pos, desc = _read_vtk(traj_out)
    assert pos.shape[0] == N_SCANS
    return np.concatenate([pos, desc["orientationX"], desc["orientationY"], desc["orientationZ"]], 1)


def test_config4_with_normal_space_input_equals_presampled_scans(tmp_path, icp, scans):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    _host()
    assert "input:\n" in CONFIG4_YAML
    z = _three(scans)
    a = str(tmp_path / "filter"); b = str(tmp_path / "presampled")
    os.makedirs(a); os.makedirs(b)
    names, _ = write_bundled_dataset(a, z)
    poses_a = _replay(a, CONFIG4_YAML.replace("input:\n", "input:\n" + NS_CHAIN, 1))
    # the same scans after the mapper's sensor-range cut (sensorMaxRange 200, ahead of input:) and normals (knn 10), sampled beforehand
    # by the restatement from the buckets the device gives these normals, written in binary with their normals so that every float32
    # comes back as it left
    write_bundled_dataset(b, z)
    for k, name in enumerate(names):
        xyz = z[f"scan{k}_xyz"].astype(F)
        r = np.sqrt(xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1] + xyz[:, 2] * xyz[:, 2])
        c = _c4(xyz[r < F(200)])
        nrm = icp.surfaceNormals(c, 10)
        _, dev_b = icp.normalSpaceSampling(c, nrm, 4000, with_buckets=True)
        order, _ = nsr.normal_space_sampling(c, nrm, 4000, buckets=dev_b)
        _write_binary_vtk(os.path.join(b, "scans", name), c[order, :3], nrm[order])
    poses_b = _replay(b, CONFIG4_YAML)
    assert np.array_equal(poses_a, poses_b), np.abs(poses_a - poses_b).max()


def test_config4_with_normal_space_among_the_reading_filters_is_repeatable(tmp_path, scans):
    from config4_data import CONFIG4_YAML, write_bundled_dataset
    _host()
    z = _three(scans)
    dirs = [str(tmp_path / d) for d in ("plain", "sampled", "again")]
    for d in dirs:
        os.makedirs(d)
        write_bundled_dataset(d, z)
    assert "icp:\n" in CONFIG4_YAML and "readingDataPointsFilters" not in CONFIG4_YAML
    chain = "  readingDataPointsFilters:\n" + NS_CHAIN.replace("  - ", "    - ").replace("      ", "        ")
    cfg = CONFIG4_YAML.replace("icp:\n", "icp:\n" + chain, 1)
    poses_a = _replay(dirs[0], CONFIG4_YAML)
    poses_b = _replay(dirs[1], cfg)
    poses_c = _replay(dirs[2], cfg)
    assert np.isfinite(poses_b).all()
    assert np.array_equal(poses_b, poses_c)                                  # repeatable
    assert not np.array_equal(poses_a, poses_b)                              # the readings were sampled
    assert np.abs(poses_a[:, :3] - poses_b[:, :3]).max() < 0.25              # and the trajectory is the same one
