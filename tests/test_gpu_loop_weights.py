"""The ICP loop's own weights and pair sums, filter by filter (icpmi_debug_keep_sums / icpmi_debug_last_sums): the registration loop selects
its quantiles with the fused kernels (sel2_hist0_kernel / sel2_scan_hist_kernel, the last level and the median factor inside
accumulate_kernel) and evaluates every weight inside accumulate_kernel<MIN, FUSED, EXT, BT> -- qindex for the reading's descriptors of
tile-sorted queries, the matched point's .w for the map scalar, plane2 from match_pt / pnm / map, the robust scale kept in the loop state
-- none of which the stage call icpmi_outlier_weights runs, and a wrong weight on a handful of pairs moves the final pose far less than
the 1e-4 the registration tests allow.

Driver of test_gpu_loop_matches.py: fixed-iteration registrations of j = 1, 2, 3 iterations and the checked chain to its own stop, the
sums kept.  After each run, against tests/weights_reference.py over lastMatches() (float64; the binary float32 decisions restated exactly):
  - the limits of Trimmed / Median / VarTrimmed filters bitwise, the robust scale within 4 float32 ulp of the float64 replay;
  - sums[28] == stats.pairs == the reference's count of non-zero weights (undecidable pairs either way);
  - stats.weighted_point_used_ratio == float32(sums[27] / (k n));
  - every entry of the sums within SUMS_REL * sum |w term| of the reference, plus the undecidable pairs' own |w term|;
  - the pose after the iteration within SOLVE_TOL_* of the float64 solve over the reference's sums, composed with T_used."""
import numpy as np
import pytest

import loop_weights_cases as lwc
import weights_reference as wr
from loop_driver import centring, f32T, pose_out
from test_gpu_loop_matches import SOLVE_TOL_M, SOLVE_TOL_RAD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def check_iteration(ob, tag, c, inp, map_c, mean, T_prev_pose, T_now, stats, matches, last, j, d2_by_iter):
    ids, d2, T_used = matches
    sums, limits, scale, _ = last
    k, n = c["knn"], inp["reading"].shape[0]
    if T_prev_pose is None:
        assert np.array_equal(T_used, np.eye(4, dtype=np.float32)), (tag, T_used)
    else:
        assert np.array_equal(pose_out(ob, T_used, mean), f32T(T_prev_pose)), (tag, "T_used is not the previous iteration's pose")
    p = ob.transform(T_used, ob.transform(centring(mean), inp["reading"]))
    d2_by_iter[j] = d2
    # the robust scale first: it is state of the loop, and the weights are evaluated with the float32 the state holds
    s64 = lwc.scale_of(c, j, d2_by_iter)
    if s64 is not None:
        assert abs(float(scale) - s64) <= 4 * np.spacing(np.float32(s64)), (tag, "robust scale", float(scale), s64)
    res, terms, rsums, rabs = lwc.reference_iteration(c, inp, map_c, p, ids, d2, T_used, j, d2_by_iter, scale_state=scale if s64 is not None else None)
    u = int(res["und"].sum())
    lo, hi = wr.count_bounds(res)
    print(f"{tag}: {lo} pairs, {u} undecidable")
    assert u <= wr.max_undecidable(lo), (tag, "undecidable pairs", u)
    for f, lim in res["limits"].items():
        assert np.float32(limits[f]) == np.float32(lim), (tag, "limit of filter", f, float(limits[f]), lim)
    assert sums[28] == stats.pairs and lo <= stats.pairs <= hi, (tag, "pairs", sums[28], stats.pairs, lo, hi)
    assert np.float32(stats.weighted_point_used_ratio) == np.float32(sums[27] / (k * n)), (tag, stats.weighted_point_used_ratio, sums[27] / (k * n))
    tol = wr.SUMS_REL * rabs + wr.undecidable_slack(res, terms)
    tol[28] = hi - lo
    err = np.abs(sums - rsums)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(rabs > 0, err / rabs, 0.0)
    print(f"{tag}: largest |device - reference| / sum |w term| = {rel[:28].max():.3e} (entry {int(rel[:28].argmax())})")
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, (tag, "pair sums", bad.tolist(), sums[bad].tolist(), rsums[bad].tolist(), (err[bad] / np.maximum(rabs[bad], 1e-300)).tolist())
    # the pose after the iteration: float64 solve over the reference's sums, composed with T_used (compared in the centred frame)
    T_ref = wr.step_from_sums(c["minimizer"], rsums, bool(c["force_2d"])) @ T_used.astype(np.float64)
    M = np.eye(4); M[:3, 3] = mean
    Mi = np.eye(4); Mi[:3, 3] = -mean.astype(np.float64)
    T_dev = Mi @ np.asarray(T_now, dtype=np.float64) @ M
    from norlab_icp_mapper_amd import synth
    dt, dr = synth.pose_error(T_dev, T_ref)
    assert dt < SOLVE_TOL_M and dr < SOLVE_TOL_RAD, (tag, "pose after the iteration vs float64 solve over the reference's weights", dt, dr)


@pytest.mark.parametrize("cid", lwc.IDS)
def test_loop_weights_and_pair_sums(amd, oracle, cid):
    import torch
    c = lwc.CASES[lwc.IDS.index(cid)]
    inp = lwc.inputs(c)
    n = inp["reading"].shape[0]
    cfg = dict(minimizer=c["minimizer"], knn=c["knn"], max_dist=c["max_dist"], outliers=c["outliers"], force_2d=c["force_2d"])
    fixed = amd.ICPSequence(**cfg, max_iterations=40, use_differential=0)
    checked = amd.ICPSequence(**cfg, max_iterations=40, use_differential=1)
    with pytest.raises(Exception):      # off by default
        fixed.lastSums()
    for icp in (fixed, checked):
        assert icp.setMap(inp["map"], inp["normals"])
        if lwc.needs(c, "map_scalar"): icp.setMapScalar(inp["map_scalar"])
        icp.keepSums(1)
    mean = fixed.getMapMean()
    map_c = inp["map"].copy(); map_c[:, :3] = inp["map"][:, :3] - mean[None, :]
    d = torch.from_numpy(inp["reading"]).cuda()
    dn = torch.from_numpy(inp["read_normals"]).cuda() if lwc.needs(c, "read_normals") else None

    def run(icp, j):
        if lwc.needs(c, "read_scalar"): icp.setReadingScalar(inp["read_scalar"])    # one shot
        T = icp.registerDev(d.data_ptr(), n, fixed_iterations=j, d_normals_ptr=dn.data_ptr() if dn is not None else None)
        return T, icp.stats, icp.lastMatches(), icp.lastSums()

    poses, d2_by_iter = {}, {}
    for j in (1, 2, 3):
        T, st, mt, ls = run(fixed, j)
        assert st.iterations == j
        poses[j] = T
        check_iteration(oracle, f"{cid}: iteration {j} of a {j}-iteration registration", c, inp, map_c, mean, poses.get(j - 1), T, st, mt, ls, j, d2_by_iter)
    T_chk, st, mt, ls = run(checked, 0)
    F = int(st.iterations)
    assert F >= 2, (cid, F)
    if F - 1 not in poses: poses[F - 1] = run(fixed, F - 1)[0]
    # (the robust scale of iteration F is carried over from iterations <= 3, kept above, or -- berg -- follows from the first)
    check_iteration(oracle, f"{cid}: last counted iteration ({F}) of the checked chain", c, inp, map_c, mean, poses[F - 1], T_chk, st, mt, ls, F, d2_by_iter)
    fixed.keepSums(0)       # ... and off again: the registration runs as before, nothing to read
    if lwc.needs(c, "read_scalar"): fixed.setReadingScalar(inp["read_scalar"])
    T = fixed.registerDev(d.data_ptr(), n, fixed_iterations=1, d_normals_ptr=dn.data_ptr() if dn is not None else None)
    assert np.array_equal(T, poses[1]), (cid, "the first iteration's pose with and without the sums kept")
    with pytest.raises(Exception):
        fixed.lastSums()
