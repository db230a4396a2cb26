"""MaxDensityDataPointsFilter on the device and on the resident map.
(a) icpmi_max_density_keep against the numpy restatement (tests/max_density_reference.py, itself held to the host filter by
    tests/test_max_density_cpu.py): keep masks equal byte for byte.
(b) the resident program [POINT_DISTANCE; SURFACE_NORMALS knn 10 keepDensities; MAX_DENSITY] against a composition of entries that
    existed before it: icpmi_map_update_chain with POINT_DISTANCE alone on a second handle, icpmi_surface_normals_ex on the downloaded
    cloud, the numpy draw, icpmi_set_map of the kept points.  Points, normals, densities: bit for bit.
(c) the C++ host shell: the first 4 bundled scans through the Mapper with post: SurfaceNormal{keepDensities} / MaxDensity /
    CutAtDescriptorThreshold, resident path against host path, one child process each.  The two paths do not part: poses, points and
    the three descriptors are bit-identical after the first update and after all four (both are asserted)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import max_density_reference as mdr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 8


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def icp(amd):
    h = amd.ICPSequence(minimizer=1, max_dist=2.0, max_iterations=5)
    yield h
    h.close()


def _keep(icp, dens, max_density, seed, n=None, fill=0xAB):
    """the raw C entry: (status, keep bytes).  The output goes in filled, so a point the kernel skipped shows."""
    d = np.ascontiguousarray(dens, dtype=F)
    n = d.shape[0] if n is None else n
    keep = np.full(max(d.shape[0], 1), fill, dtype=np.uint8)
    st = icp._lib.icpmi_max_density_keep(icp._h, d.ctypes.data, C.c_int64(n), C.c_float(max_density), C.c_int32(seed), keep.ctypes.data)
    return st, keep[:d.shape[0]]


def _same(icp, dens, max_density, seed):
    st, got = _keep(icp, dens, max_density, seed)
    assert st == OK
    want = mdr.max_density_keep(dens, max_density, seed).astype(np.uint8)
    assert got.tobytes() == want.tobytes(), (int((got != want).sum()), np.nonzero(got != want)[0][:8])
    return got


# ------------------------------------------------------------------------------------------------------------------ (a) the entry
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 65_537, 100_003])
def test_keep_equals_the_reference(icp, n):
    dens = mdr.log_uniform_densities(np.random.default_rng(n), n)
    got = _same(icp, dens, 10.0, 1)
    if n > 1000:
        assert 0.2 < 1.0 - got.mean() < 0.6                                    # half the points are dense, most of those go
    st, again = _keep(icp, dens, 10.0, 1, fill=0x5C)
    assert st == OK and again.tobytes() == got.tobytes()                       # two calls, equal bytes


def test_special_densities(icp):
    n = 65_537
    rng = np.random.default_rng(4)
    assert _same(icp, np.full(n, 40.0, F), 10.0, 1).mean() == pytest.approx(0.25, abs=0.02)     # all dense
    assert _same(icp, rng.uniform(0.1, 9.9, n).astype(F), 10.0, 1).all()                        # none dense
    assert _same(icp, np.full(n, 10.0, F), 10.0, 1).all()                                       # equal to maxDensity: not dense
    dens = mdr.log_uniform_densities(rng, n)
    nan_at, inf_at = np.array([0, 63, 64, 2047, 2048, 40_000, n - 1]), np.array([1, 65, 255, 256, 4096, 50_001, n - 2])
    dens[nan_at] = np.nan
    dens[inf_at] = np.inf
    got = _same(icp, dens, 10.0, 1)
    assert got[nan_at].all() and not got[inf_at].any()                                          # NaN kept, +inf dropped (u < 0 is false)
    assert not _same(icp, np.full(300, np.inf, F), 10.0, 1).any()


def test_seeds(icp):
    dens = mdr.log_uniform_densities(np.random.default_rng(5), 100_003)
    one = _same(icp, dens, 10.0, 1)
    # the engine's constructor: seed mod (2^31 - 1), 0 taken as 1 -- and a negative seed wraps through uint32 first: -1 is 2^32 - 1 =
    # 2 (2^31 - 1) + 1, -2 is 2 (2^31 - 1) + 0 and -2^31 is 2^31 = (2^31 - 1) + 1, all three the state 1 again
    for seed in (0, 2147483647, -1, -2, -2147483648):
        assert _same(icp, dens, 10.0, seed).tobytes() == one.tobytes()
    for seed in (2, -3, -5):
        assert _same(icp, dens, 10.0, seed).tobytes() != one.tobytes()
    assert _same(icp, dens, 250.0, 12345).mean() > 0.9 and _same(icp, dens, 0.5, 12345).mean() < 0.3


def test_arguments(icp):
    dens = np.full(8, 20.0, F)
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        st, keep = _keep(icp, dens, bad, 1)
        assert st == INVALID_ARG and (keep == 0xAB).all(), bad
    st, keep = _keep(icp, np.zeros(0, F), 10.0, 1)
    assert st == OK
    st, keep = _keep(icp, dens, 10.0, 1, n=1 << 31)                             # refused before anything is read
    assert st == UNSUPPORTED and (keep == 0xAB).all()
    st, _ = _keep(icp, dens, 10.0, 1, n=-1)
    assert st == INVALID_ARG
    assert icp.maxDensityKeep(dens, 10.0, 1).dtype == bool                      # the wrapper


# ------------------------------------------------------------------------------------------------------------------ (b) the chain
KNN, MAX_DENSITY, SEED, MIN_DIST = 10, 60.0, 7, 0.05


def _box(rng, n):
    """uniform in a 4 x 4 x 2 m box: ~94 points / m^3 at 3000 points, so the kNN density estimate straddles MAX_DENSITY"""
    p = np.ones((n, 4), F)
    p[:, :3] = (rng.uniform(0, 1, (n, 3)) * [4, 4, 2]).astype(F)
    return p


@pytest.fixture(scope="module")
def chain_clouds():
    rng = np.random.default_rng(21)
    return _box(rng, 3000), [_box(rng, 1500) for _ in range(3)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _new(amd, base):
    h = amd.ICPSequence(minimizer=1, max_dist=2.0, max_iterations=5)
    h.setMap(base)
    return h


def test_chain_equals_the_composition(amd, chain_clouds):
    base, scans = chain_clouds
    a, b = _new(amd, base), _new(amd, base)
    assert a.getMapDensities() is None                                          # a map handed in has no row
    modules = [("point_distance", MIN_DIST)]
    post = [("surface_normals", KNN, 1), ("max_density", MAX_DENSITY, SEED)]
    for scan in scans:
        src, m = a.mapUpdateChain(scan, modules, post)
        # the composition: the module alone, the normals + densities of what it left, the draw, the kept points as the next map
        src_b, m_b = b.mapUpdateChain(scan, modules, [])
        pts_b = b.getMap()
        assert m_b == pts_b.shape[0] and m_b > base.shape[0]
        nrm_b, dens_b = b.surfaceNormals(pts_b, knn=KNN, with_densities=True)
        keep = mdr.max_density_keep(dens_b, MAX_DENSITY, SEED)
        removed = 1.0 - keep.mean()
        print(f"update: {m_b} points, {int((dens_b > MAX_DENSITY).sum())} dense, {removed:.3f} removed")
        assert 0.10 <= removed <= 0.90                                          # a step that removes nothing or everything would hide a wrong draw
        got, got_n = a.getMap(with_normals=True)
        assert m == int(keep.sum()) == got.shape[0]
        assert np.array_equal(_bits(got), _bits(pts_b[keep]))
        assert np.array_equal(_bits(got_n), _bits(nrm_b[keep]))
        assert np.array_equal(_bits(a.getMapDensities()), _bits(dens_b[keep]))
        assert np.array_equal(src, src_b[keep])                                 # provenance in [old map ; scan] of the kept points
        b.setMap(pts_b[keep], nrm_b[keep])
    a.close(); b.close()


def test_chain_with_nothing_dense_equals_the_run_without_the_step(amd, chain_clouds):
    base, scans = chain_clouds
    a, b = _new(amd, base), _new(amd, base)
    modules = [("point_distance", MIN_DIST)]
    for scan in scans[:2]:
        src_a, m_a = a.mapUpdateChain(scan, modules, [("surface_normals", KNN, 1), ("max_density", 1e30, SEED)])
        src_b, m_b = b.mapUpdateChain(scan, modules, [("surface_normals", KNN, 1)])
        assert m_a == m_b and np.array_equal(src_a, src_b)
        (pa, na), (pb, nb) = a.getMap(with_normals=True), b.getMap(with_normals=True)
        assert np.array_equal(_bits(pa), _bits(pb)) and np.array_equal(_bits(na), _bits(nb))
        assert np.array_equal(_bits(a.getMapDensities()), _bits(b.getMapDensities()))
        assert np.isfinite(a.getMapDensities()).all() and a.getMapDensities().shape == (m_a,)
    # the row does not outlive a program that does not write it, nor a map handed in
    b.mapUpdateChain(scans[2], modules, [("surface_normals", KNN)])
    assert b.getMapDensities() is None
    a.setMap(base)
    assert a.getMapDensities() is None
    a.close(); b.close()


def test_max_density_without_a_density_step_is_refused(amd, chain_clouds):
    base, scans = chain_clouds
    a = _new(amd, base)
    a.mapUpdateChain(scans[0], [("point_distance", MIN_DIST)], [("surface_normals", KNN, 1)])
    before, before_n = a.getMap(with_normals=True)
    before_d = a.getMapDensities()
    ops_bad = {
        "no density step": ([("point_distance", MIN_DIST)], [("surface_normals", KNN, 0), ("max_density", MAX_DENSITY, SEED)]),
        "the density step comes after": ([("point_distance", MIN_DIST)], [("max_density", MAX_DENSITY, SEED), ("surface_normals", KNN, 1)]),
        "alone": ([("point_distance", MIN_DIST)], [("max_density", MAX_DENSITY, SEED)]),
        "among the modules": ([("point_distance", MIN_DIST), ("max_density", MAX_DENSITY, SEED)], [("surface_normals", KNN, 1)]),
        "maxDensity 0": ([("point_distance", MIN_DIST)], [("surface_normals", KNN, 1), ("max_density", 0.0, SEED)]),
    }
    for what, (modules, post) in ops_bad.items():
        ops = a._mapOps(modules, post)
        src = np.empty(before.shape[0] + len(modules) * scans[1].shape[0] + 1, np.int32)
        new_m = C.c_int64(-1)
        st = a._lib.icpmi_map_update_chain(a._h, scans[1].ctypes.data, scans[1].shape[0], None, None, None, None, ops, len(ops), len(modules),
                                           src.ctypes.data, src.shape[0], None, C.byref(new_m))
        assert st == INVALID_ARG, what
        msg = a._lib.icpmi_last_error(a._h).decode()
        if what in ("no density step", "the density step comes after", "alone"):
            assert "MaxDensityDataPointsFilter: Error, no densities found in descriptors." in msg and msg.startswith("InvalidField"), msg
        after, after_n = a.getMap(with_normals=True)                            # the resident map is untouched
        assert np.array_equal(_bits(after), _bits(before)) and np.array_equal(_bits(after_n), _bits(before_n))
        assert np.array_equal(_bits(a.getMapDensities()), _bits(before_d))
    a.close()


# ------------------------------------------------------------------------------------------------------------------ (c) the host shell
N_SCANS = 4


def _config():
    from config4_data import CONFIG4_YAML
    shipped_post = "    - SurfaceNormalDataPointsFilter:\n        knn: 10\n"
    assert shipped_post in CONFIG4_YAML and "samplingMethod: 0" in CONFIG4_YAML
    cfg = CONFIG4_YAML.replace(shipped_post, "    - SurfaceNormalDataPointsFilter:\n        knn: 10\n        keepDensities: 1\n"
                               "    - MaxDensityDataPointsFilter:\n        maxDensity: %s\n        seed: 3\n" % HOST_MAX_DENSITY)
    return cfg.replace("samplingMethod: 0", "samplingMethod: 1")               # the reproducible hash on both paths


HOST_MAX_DENSITY = "10"     # the filter's default.  The bundled scans are outdoor scans: one point per 0.15 m octree leaf gives kNN-10
                            # densities with a median near 9 points / m^3 on the first scan, so about half of the map draws


def _sorted_map(r):
    pts = r["points"]
    order = np.lexsort((_bits(pts[:, 2]), _bits(pts[:, 1]), _bits(pts[:, 0])))
    return order, pts[order]


@pytest.fixture(scope="module")
def host_replays(tmp_path_factory):
    from config4_data import write_bundled_dataset
    from test_host_cpp import _build_host
    _build_host()
    tmp = str(tmp_path_factory.mktemp("max_density_replay"))
    z = np.load(os.path.join(ROOT, "tests", "golden", "bundled_scans_all.npz"))
    sub = {"scan_names": z["scan_names"][:N_SCANS], "trajectory": z["trajectory"][:N_SCANS]}
    for k in range(N_SCANS):
        sub[f"scan{k}_xyz"] = z[f"scan{k}_xyz"]
    names, traj = write_bundled_dataset(tmp, sub)
    open(os.path.join(tmp, "names.txt"), "w").write("\n".join(names) + "\n")
    np.save(os.path.join(tmp, "trajectory.npy"), np.asarray(traj, dtype=np.float64))
    cfg = os.path.join(tmp, "config.yaml")
    open(cfg, "w").write(_config())
    out = {}
    for mode in ("1", "0"):
        for n_scans in (N_SCANS, 1):
            dst = os.path.join(tmp, f"replay_{mode}_{n_scans}.npz")
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "max_density_replay.py"), tmp, cfg, str(n_scans), dst],
                               capture_output=True, text=True, timeout=300, env=dict(os.environ, NIM_RESIDENT_MAP_UPDATE=mode))
            assert p.returncode == 0, p.stderr[-2000:] + p.stdout[-500:]
            out[mode, n_scans] = dict(np.load(dst))
    return out


def _compare(res, host):
    assert np.array_equal(_bits(res["poses"]), _bits(host["poses"]))
    assert res["points"].shape == host["points"].shape
    (ro, rp), (ho, hp) = _sorted_map(res), _sorted_map(host)
    assert np.array_equal(_bits(rp), _bits(hp))                                # equal as point sets
    for name in ("normals", "densities", "probabilityDynamic"):
        assert np.array_equal(_bits(res["desc_" + name][ro]), _bits(host["desc_" + name][ho])), name
    assert sorted(k for k in res if k.startswith("desc_")) == sorted(k for k in host if k.startswith("desc_"))


def test_host_shell_resident_counts(host_replays):
    for n_scans in (N_SCANS, 1):
        res, host = host_replays["1", n_scans], host_replays["0", n_scans]
        assert int(res["map_updates"]) == int(host["map_updates"]) >= 1
        assert int(res["resident_updates"]) == int(res["map_updates"])         # every update ran on the resident map
        assert int(host["resident_updates"]) == 0
        for r in (res, host):
            assert {"desc_normals", "desc_densities", "desc_probabilityDynamic"} <= set(r)
            assert r["desc_densities"].shape == (r["points"].shape[0], 1)
    assert int(host_replays["1", N_SCANS]["map_updates"]) == N_SCANS


def test_host_shell_max_density_bites(host_replays):
    """what is left is at most maxDensity dense where it was drawn, and the step did remove points: the map is smaller than the same
    replay's map without it would be (every surviving density row says how dense the map was BEFORE the draw)"""
    d = host_replays["0", N_SCANS]["desc_densities"][:, 0]
    dense = float((d > float(HOST_MAX_DENSITY)).mean())
    print(f"final map: {d.shape[0]} points, median density {np.median(d):.0f}, {dense:.3f} of the survivors were dense")
    assert 0.02 < dense < 0.98


def test_host_shell_first_update_resident_equals_host(host_replays):
    _compare(host_replays["1", 1], host_replays["0", 1])


def test_host_shell_resident_equals_host(host_replays):
    _compare(host_replays["1", N_SCANS], host_replays["0", N_SCANS])
