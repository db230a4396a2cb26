"""What a chain asks of a call before anything is launched, entry point by entry point.

icpmi_register_dev, icpmi_residual_error_dev and icpmi_residual_error_poses_dev run the same chain, so they must agree about what it needs: every
row of ROWS is (chain, missing precondition) -> (status, a piece of icpmi_last_error), asserted on all three, with k = 1 and k = 6.  Two rows
pin the order of the checks, the rest the per-item status of the calls that take many items (batch, multistart, poses) where
tests/test_gpu_batch.py and tests/test_gpu_residual_poses.py do not: one bad item among good ones, with and without the status array,
the return value and the text of icpmi_last_error on either route.

Scene: 4 000 map points with normals, a reading of 256 points."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
M, N = 4000, 256
KS = (1, 6)
OK, ERR_INVALID_ARG, ERR_NO_POINT, ERR_NO_OUTLIER, ERR_MISSING_NORMALS, ERR_UNSUPPORTED = 0, 1, 3, 4, 7, 8
TRIM, SURFACE = (4, 0.85), (5, 0.5)
GEN_READING, GEN_MAP = (6, 0.1, 1 | 2, 0.0), (6, 0.5, 4, 0.0)        # GenericDescriptor{source: reading, soft}; on the map, largerThan
ROBUST_PLANE = (7, 0.5, 4 | (1 << 8), 0.0, 0.0)                      # Robust{tukey, distanceType: point2plane}
ROBUST_BERG = (7, 0.05, 0 | (2 << 4), 0.0, 0.0)                      # Robust{cauchy, scaleEstimator: berg}
BASE = dict(max_dist=1.0, max_iterations=5)


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def scene(amd):
    import torch
    sc = amd.synth.make_scene(m=M, n=N, scale=0.2)
    sc["d_scan"] = torch.from_numpy(np.ascontiguousarray(sc["scan"])).cuda()
    sc["d_normals"] = torch.from_numpy(np.ascontiguousarray(sc["scan_normals"])).cuda()
    far = sc["scan"].copy(); far[:, 0] += 1000.0
    sc["d_far"] = torch.from_numpy(far).cuda()
    return sc


def _cm(poses):
    P = np.asarray(poses, F).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(-1)


def last_error(icp):
    return icp._lib.icpmi_last_error(icp._h).decode()


# ---- the three entry points: (status, last error) of one call; a poses call that fails as a whole leaves out and status zeroed
def call_register(icp, d_scan, n, d_normals):
    T = (C.c_float * 16)()
    st = icp._lib.icpmi_register_dev(icp._h, d_scan, int(n), d_normals, T, C.byref(icp.stats))
    return int(st), last_error(icp)


def call_residual(icp, d_scan, n, d_normals):
    from norlab_icp_mapper_amd import _capi
    res = _capi.Residual()
    st = icp._lib.icpmi_residual_error_dev(icp._h, d_scan, int(n), d_normals, None, 0, C.byref(res))
    return int(st), last_error(icp)


def call_poses(icp, d_scan, n, d_normals):
    from norlab_icp_mapper_amd import _capi
    Tc = _cm([np.eye(4), np.eye(4)])
    res = (_capi.Residual * 2)(); status = (C.c_int * 2)()
    C.memset(res, 0xFF, C.sizeof(res)); C.memset(status, 0xFF, C.sizeof(status))
    st = icp._lib.icpmi_residual_error_poses_dev(icp._h, d_scan, int(n), d_normals, Tc.ctypes.data, 2, 0, res, status, None)
    if st != OK:
        assert bytes(res) == bytes(C.sizeof(res)) and list(status) == [0, 0]
    else:
        assert list(status) == [0, 0]
    return int(st), last_error(icp)


ENTRIES = {"register": call_register, "residual": call_residual, "poses": call_poses}


# ---- the rows: name -> (chain, map normals?, reading normals?, n, arm(icp), status, text)
def _nothing(icp):
    pass


ROWS = {
    "surface_normal_without_reading_normals":
        (dict(minimizer=2, outliers=[TRIM, SURFACE]), True, False, N, _nothing, ERR_MISSING_NORMALS, "SurfaceNormalOutlierFilter needs 'normals'"),
    "generic_reading_without_the_row":
        (dict(minimizer=2, outliers=[GEN_READING]), True, False, N, _nothing, ERR_INVALID_ARG, "icpmi_set_reading_scalar"),
    "generic_reading_row_of_the_wrong_length":
        (dict(minimizer=2, outliers=[GEN_READING]), True, False, N, lambda icp: icp.setReadingScalar(np.zeros(N - 1, F)), ERR_INVALID_ARG,
         "icpmi_set_reading_scalar"),
    "generic_map_without_the_map_scalar":
        (dict(minimizer=2, outliers=[GEN_MAP]), True, False, N, _nothing, ERR_INVALID_ARG, "icpmi_set_map_scalar"),
    "robust_point2plane_on_a_map_without_normals":
        (dict(minimizer=1, outliers=[ROBUST_PLANE]), False, False, N, _nothing, ERR_MISSING_NORMALS, "RobustOutlierFilter{distanceType: point2plane}"),
    "var_dist_without_the_row":
        (dict(minimizer=2, var_dist=1, outliers=[TRIM]), True, False, N, _nothing, ERR_INVALID_ARG, "icpmi_set_reading_max_dist"),
    "var_dist_row_of_zeros":
        (dict(minimizer=2, var_dist=1, outliers=[TRIM]), True, False, N, lambda icp: icp.setReadingMaxDist(np.zeros(N, F)), ERR_INVALID_ARG,
         "the largest radius of the row must be > 0"),
    "empty_reading_with_a_trimmed_chain":
        (dict(minimizer=2, outliers=[TRIM]), True, False, 0, _nothing, ERR_NO_OUTLIER, "no outlier to filter"),
    "empty_reading_without_a_trimmed_chain":
        (dict(minimizer=2, outliers=[(1, 0.9)]), True, False, 0, _nothing, ERR_NO_POINT, "no point to minimize"),
}


def handle(amd, sc, k, map_normals=True, **chain):
    icp = amd.ICPSequence(knn=k, **dict(BASE, **chain))
    assert icp.setMap(sc["map"], sc["normals"] if map_normals else None)
    return icp


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(ROWS))
def test_every_entry_point_reports_the_same_missing_precondition(amd, scene, name, k):
    chain, map_normals, reading_normals, n, arm, status, text = ROWS[name]
    icp = handle(amd, scene, k, map_normals, **chain)
    got = {}
    for entry, call in ENTRIES.items():
        arm(icp)                                                                   # (a one-shot row serves one call)
        st, msg = call(icp, scene["d_scan"].data_ptr() if n else None, n, scene["d_normals"].data_ptr() if reading_normals else None)
        assert st == status and text in msg, (name, k, entry, st, msg)
        got[entry] = (st, msg)
    assert got["register"] == got["residual"] == got["poses"], (name, k, got)      # the same words, not only the same piece of them
    icp.close()


# ---- the order of the checks
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_call_that_fails_early_still_consumes_its_one_shot_rows(amd, scene, entry, k):
    icp = handle(amd, scene, k, minimizer=2, var_dist=1, outliers=[SURFACE, GEN_READING])
    call, d, nrm = ENTRIES[entry], scene["d_scan"].data_ptr(), scene["d_normals"].data_ptr()
    scalar, radii = (np.arange(N) % 5).astype(F) / F(4), np.full(N, 0.8, F)
    icp.setReadingScalar(scalar); icp.setReadingMaxDist(radii)
    st, msg = call(icp, d, N, None)                                                # fails the SurfaceNormal check, the first of the chain's
    assert st == ERR_MISSING_NORMALS and "SurfaceNormalOutlierFilter" in msg, (entry, k, st, msg)
    st, msg = call(icp, d, N, nrm)                                                 # both rows went with that call: the scalar row is asked for first
    assert st == ERR_INVALID_ARG and "icpmi_set_reading_scalar" in msg, (entry, k, st, msg)
    icp.setReadingScalar(scalar)
    st, msg = call(icp, d, N, nrm)                                                 # ... then the row of radii
    assert st == ERR_INVALID_ARG and "icpmi_set_reading_max_dist" in msg, (entry, k, st, msg)
    icp.setReadingScalar(scalar); icp.setReadingMaxDist(radii)
    st, msg = call(icp, d, N, nrm)
    assert st == OK, (entry, k, st, msg)
    icp.close()


@pytest.mark.parametrize("k", KS)
def test_the_residual_refuses_robust_berg_before_it_asks_for_reading_normals(amd, scene, k):
    icp = handle(amd, scene, k, minimizer=2, outliers=[SURFACE, ROBUST_BERG])
    d = scene["d_scan"].data_ptr()
    for entry in ("residual", "poses"):
        st, msg = ENTRIES[entry](icp, d, N, None)
        assert st == ERR_UNSUPPORTED and "RobustOutlierFilter with scaleEstimator berg" in msg, (entry, k, st, msg)
    st, msg = call_register(icp, d, N, None)                                       # a registration runs such a chain: it asks for the normals
    assert st == ERR_MISSING_NORMALS and "SurfaceNormalOutlierFilter" in msg, (k, st, msg)
    icp.close()


# ---- the per-item status: one bad item among good ones.  k = 1: the route that launches the items together (pinned through `batched`),
# k = 6: one item after the other
def _served(icp, sc):
    from norlab_icp_mapper_amd import _capi
    res = (_capi.Residual * 2)(); status = (C.c_int * 2)(); batched = C.c_int32(-1)
    assert icp._lib.icpmi_residual_error_poses_dev(icp._h, sc["d_scan"].data_ptr(), N, None, _cm([np.eye(4)] * 2).ctypes.data, 2, 0, res, status,
                                                   C.byref(batched)) == OK
    return batched.value == 2


@pytest.mark.parametrize("k", KS)
def test_batch_status_fold(amd, scene, k):
    from norlab_icp_mapper_amd import _capi
    icp = handle(amd, scene, k, minimizer=2, outliers=[TRIM])
    assert _served(icp, scene) == (k == 1)
    ptrs = (C.c_void_p * 3)(scene["d_scan"].data_ptr(), scene["d_far"].data_ptr(), scene["d_scan"].data_ptr())
    nn = (C.c_int64 * 3)(N, N, N)
    out = []
    for with_status in (True, False):
        T = (C.c_float * 48)(); stats = (_capi.Stats * 3)(); status = (C.c_int * 3)(9, 9, 9)
        rv = icp._lib.icpmi_register_batch_dev(icp._h, 3, ptrs, nn, 0, T, stats, status if with_status else None)
        msg = last_error(icp)
        assert rv == (OK if with_status else ERR_NO_OUTLIER), (k, with_status, rv, msg)
        assert list(status) == ([OK, ERR_NO_OUTLIER, OK] if with_status else [9, 9, 9]), (k, with_status)
        # together: the batch's own words; one by one: the words of the reading that failed
        assert ("register_batch: a reading ended with a convergence error (see the per-reading status)" if k == 1 else "no outlier to filter") in msg
        assert np.array_equal(np.array(T[16:32], F).reshape(4, 4), np.eye(4, dtype=F))
        out.append(bytes(T))
    assert out[0] == out[1]
    icp.close()


@pytest.mark.parametrize("k", KS)
def test_multistart_status_fold(amd, scene, k):
    from norlab_icp_mapper_amd import _capi
    icp = handle(amd, scene, k, minimizer=2, outliers=[TRIM])
    assert _served(icp, scene) == (k == 1)
    far = np.eye(4, dtype=F); far[0, 3] = 1000.0
    priors = _cm([np.eye(4), far, np.eye(4)])
    out = []
    for with_status in (True, False):
        T = (C.c_float * 48)(); stats = (_capi.Stats * 3)(); status = (C.c_int * 3)(9, 9, 9)
        rv = icp._lib.icpmi_register_multistart_dev(icp._h, scene["d_scan"].data_ptr(), N, priors.ctypes.data, 3, 0, T, stats,
                                                    status if with_status else None)
        msg = last_error(icp)
        assert rv == (OK if with_status else ERR_NO_OUTLIER), (k, with_status, rv, msg)
        assert list(status) == ([OK, ERR_NO_OUTLIER, OK] if with_status else [9, 9, 9]), (k, with_status)
        assert "register_multistart: a start ended with an error (see the per-start status)" in msg
        out.append(bytes(T))
    assert out[0] == out[1]
    icp.close()


@pytest.mark.parametrize("k", KS)
def test_poses_status_fold(amd, scene, k):
    from norlab_icp_mapper_amd import _capi
    icp = handle(amd, scene, k, minimizer=2, outliers=[TRIM])
    assert _served(icp, scene) == (k == 1)
    far = np.eye(4, dtype=F); far[0, 3] = 1000.0
    bad = np.eye(4, dtype=F); bad[0, 0] = 1.01
    poses = _cm([np.eye(4), far, np.eye(4), bad])
    out = []
    for with_status in (True, False):
        res = (_capi.Residual * 4)(); status = (C.c_int * 4)(9, 9, 9, 9)
        rv = icp._lib.icpmi_residual_error_poses_dev(icp._h, scene["d_scan"].data_ptr(), N, None, poses.ctypes.data, 4, 0, res,
                                                     status if with_status else None, None)
        msg = last_error(icp)
        assert rv == (OK if with_status else ERR_NO_OUTLIER), (k, with_status, rv, msg)     # the FIRST error, not the last
        assert list(status) == ([OK, ERR_NO_OUTLIER, OK, ERR_INVALID_ARG] if with_status else [9, 9, 9, 9]), (k, with_status)
        assert "residual_error_poses_dev: a pose ended with an error (see the per-pose status)" in msg
        assert res[0].pairs > 0 and bytes(res[0]) == bytes(res[2])
        out.append(bytes(res))
    assert out[0] == out[1]
    icp.close()
