"""The ICP loop's own matches, query by query (icpmi_debug_last_matches): the seeded launches of iterations >= 1 -- nn1_wg_kernel with
seed_pre and the own-row pass, nnk_ml_kernel with wide seeds, nnk_wg_kernel with its CAPQ list, overflow repeats and wide-seed pass,
tile-sorted queries with results in query order, the fused level-0 histogram and its speculative window, the brute pass on slots --
are reached by no stage call (icpmi_knn runs the unseeded kernels on caller-ordered queries), and the final pose alone cannot tell a
handful of wrong neighbours from right ones.

For every case the registration runs j = 1, 2, 3 iterations (fixed-iteration registrations: unseeded, wide seeds, steady seeds) and
once to its own stop (Counter + Differential: the matches left behind must be the LAST COUNTED iteration's, not a dead one's behind the
stop).  After each run:
  - the queries are rebuilt bit for bit, q = T_used * ([I | -mean] * scan) through the same fmaf chain, and every row of matches is
    checked against the oracle's kd-tree (bitwise) and an exact float64 kNN (tests/match_reference.py);
  - T_used is the pose the (j - 1)-iteration registration returned (bitwise, through the same centring conversion);
  - the trimmed limit is the oracle's / numpy's quantile of exactly those d2 (+inf and exact zeros dropped), `pairs` their count
    below it, and the pose after the iteration is a float64 solve over exactly those pairs composed with T_used."""
import math

import numpy as np
import pytest

import match_reference as mr
from loop_driver import ROOT, centring, f32T, mat4_mul_f32, pose_out, scene  # noqa: F401

pytestmark = pytest.mark.gpu

RATIO = 0.85
# one float64 solve against the device's (test_gpu_golden.py: its step tests use the same bars)
SOLVE_TOL_M, SOLVE_TOL_RAD = 2e-5, 2e-6


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


# ------------------------------------------------------------------------------------------------------------------ references
def rodrigues(x):
    th = np.linalg.norm(x[:3])
    T = np.eye(4)
    if th > 0:
        kx = x[:3] / th
        K = np.array([[0, -kx[2], kx[1]], [kx[2], 0, -kx[0]], [-kx[1], kx[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = x[3:]
    return T


def solve_step(minimizer, p, q, nrm):
    """float64 step over the pairs (p reading point, q map point, nrm map normal): Kabsch (point-to-point) or the 6 x 6 normal equations
    of point-to-plane with the rotation through the angle-axis of x[:3] (test_gpu_golden.py)"""
    if minimizer == 1:
        mp, mq = p.mean(0), q.mean(0)
        U, S, Vt = np.linalg.svd((q - mq).T @ (p - mp))
        R = U @ Vt
        if np.linalg.det(R) < 0:
            Vt[-1] *= -1; R = U @ Vt
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = mq - R @ mp
        return T
    F = np.concatenate([np.cross(p, nrm), nrm], axis=1)
    A = F.T @ F
    b = -F.T @ ((p - q) * nrm).sum(1)
    return rodrigues(np.linalg.solve(A, b))


# ------------------------------------------------------------------------------------------------------------------ one case
def check_iteration(ob, tag, cfg, mapc, nrm, mean, reading, T_prev_pose, T_now, st, matches, minimizer):
    ids, d2, T_used = matches
    k, max_dist = cfg["knn"], cfg["max_dist"]
    # prefix: the pose the matcher moved the reading by is the pose after the previous iteration
    if T_prev_pose is None:
        assert np.array_equal(T_used, np.eye(4, dtype=np.float32)), (tag, T_used)
    else:
        assert np.array_equal(pose_out(ob, T_used, mean), f32T(T_prev_pose)), (tag, "T_used is not the previous iteration's pose", T_used)
    q = ob.transform(T_used, ob.transform(centring(mean), reading))
    mr.check_matches(mapc, q, ids, d2, k, max_dist, eps=cfg.get("epsilon", 0.0) if cfg.get("epsilon_approx") else 0.0, where=tag)
    # trimmed limit and pairs over exactly those d2
    trimmed = any(o[0] == 4 for o in cfg["outliers"])
    finite = np.isfinite(d2)
    if trimmed:
        lim = ob.dists_quantile(d2, RATIO)
        assert lim == mr.trimmed_quantile(d2, RATIO), (tag, lim, mr.trimmed_quantile(d2, RATIO))
        assert st["trimmed_limit"] == lim, (tag, "trimmed limit", st["trimmed_limit"], lim)
        w = finite & (d2 <= np.float32(lim))
    else:
        w = finite
    assert st["pairs"] == int(w.sum()), (tag, "pairs", st["pairs"], int(w.sum()))
    # the pose after the iteration: one float64 solve over exactly these pairs, composed with T_used (compared in the centred frame)
    qi, qj = np.nonzero(w)
    p = q[qi, :3].astype(np.float64)
    mq = mapc[ids[qi, qj], :3].astype(np.float64)
    mn = nrm[ids[qi, qj]].astype(np.float64) if minimizer == 2 else None
    T_ref = solve_step(minimizer, p, mq, mn) @ T_used.astype(np.float64)
    M = np.eye(4); M[:3, 3] = mean
    Mi = np.eye(4); Mi[:3, 3] = -mean.astype(np.float64)
    T_dev = Mi @ np.asarray(T_now, dtype=np.float64) @ M
    from norlab_icp_mapper_amd import synth
    dt, dr = synth.pose_error(T_dev, T_ref)
    assert dt < SOLVE_TOL_M and dr < SOLVE_TOL_RAD, (tag, "pose after the iteration vs float64 solve over its pairs", dt, dr)


def stats_of(icp):
    s = icp.stats
    return dict(iterations=int(s.iterations), pairs=int(s.pairs), trimmed_limit=float(s.trimmed_limit), hard_queries=int(s.hard_queries))


def run_case(amd, ob, name, cfg, js=(1, 2, 3), expect=None, checked_graph=1):
    import torch
    mp, nm, reading = scene(name)
    minimizer = cfg["minimizer"]
    # fixed-iteration registrations (one graph per count) and the checked chain (segment graphs or eager run-ahead)
    fixed = amd.ICPSequence(**cfg, max_iterations=40, use_differential=0)
    checked = amd.ICPSequence(**dict(cfg, use_graph=checked_graph), max_iterations=40, use_differential=1)
    for icp in (fixed, checked):
        assert icp.setMap(mp, nm if minimizer == 2 else None)
    mean = fixed.getMapMean()
    mapc = mp.copy(); mapc[:, :3] = mp[:, :3] - mean[None, :]
    d = torch.from_numpy(reading).cuda()

    T_chk = checked(reading)
    st_chk = stats_of(checked)
    F = st_chk["iterations"]
    assert F >= 2, (name, F)
    m_chk = checked.lastMatches()

    poses = {}
    def fixed_run(j):
        T = fixed.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=j)
        poses[j] = T
        return T
    last = 0
    for j in js:
        for jj in range(last + 1, j):
            if jj not in poses: fixed_run(jj)
        T = fixed_run(j)
        st = stats_of(fixed)
        dbg = fixed.debugCounters()
        mt = fixed.lastMatches()
        tag = f"{name} {cfg_tag(cfg)}: iteration {j} of a {j}-iteration registration"
        check_iteration(ob, tag, cfg, mapc, nm, mean, reading, poses.get(j - 1), T, st, mt, minimizer)
        if expect: expect(j, st, dbg)
        last = j
    # the checked chain stopped after F counted iterations: its matches are those of iteration F (prefix: the fixed (F - 1)-pose)
    T_prev = poses[F - 1] if F - 1 in poses else fixed_run(F - 1)
    tag = f"{name} {cfg_tag(cfg)}: last counted iteration ({F}) of the checked chain, use_graph={checked_graph}"
    check_iteration(ob, tag, cfg, mapc, nm, mean, reading, T_prev, T_chk, st_chk, m_chk, minimizer)
    return F


def cfg_tag(cfg):
    return " ".join(f"{k}={v}" for k, v in cfg.items() if k != "outliers")


def base(**kw):
    c = dict(minimizer=2, knn=1, max_dist=2.0, outliers=[(4, RATIO)])
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("minimizer", [1, 2])
def test_k1_seeded_sorted(amd, oracle, minimizer):
    """nn1_wg_kernel seeded (own-row pass at iteration 1, steady seeds after), tile-sorted queries, match_pt, fused hist0"""
    run_case(amd, oracle, "mid", base(minimizer=minimizer))


def test_k1_unbounded_brute_pass_on_slots(amd, oracle):
    def expect(j, st, dbg):
        assert st["hard_queries"] > 0, ("the brute pass (hard_sorted) must serve the far returns", j, st)
    run_case(amd, oracle, "far", base(max_dist=math.inf), expect=expect)


@pytest.mark.parametrize("k", [3, 6, 8])
@pytest.mark.parametrize("wg_from", [-1, 0, 1, 2])
def test_knn_ml_and_wg(amd, oracle, k, wg_from):
    """nnk_ml_kernel seeded (seeded = 3), nnk_wg_kernel from the unseeded (1) / wide-seed (2) / steady (0: iteration 2) launch on"""
    first = {-1: None, 0: 2, 1: 0, 2: 1}[wg_from]   # the 0-based iteration from which nnk_wg_kernel serves
    def expect(j, st, dbg):
        if first is not None and j - 1 >= first:
            assert dbg[12] + dbg[13] > 0, ("nnk_wg_kernel's selection window must have served", j, dbg[12], dbg[13])
    run_case(amd, oracle, "mid", base(knn=k, knn_wg_from=wg_from), expect=expect)


@pytest.mark.parametrize("k", [10, 16])
def test_knn_kmax16_unsorted(amd, oracle, k):
    """k > 8: the loop does not sort its queries (loop.hip: knn <= 8); the KMAX 16 kernels in the caller's order"""
    run_case(amd, oracle, "mid", base(knn=k))


def test_knn20_ring_kernel(amd, oracle):
    run_case(amd, oracle, "mid", base(knn=20))


def test_knn6_unbounded_hard_kernel(amd, oracle):
    def expect(j, st, dbg):
        assert st["hard_queries"] > 0, ("nnk_hard_kernel must serve the far returns", j, st)
    run_case(amd, oracle, "far", base(knn=6, max_dist=math.inf), expect=expect)


@pytest.mark.parametrize("k", [6, 8])
def test_identical_point_clusters(amd, oracle, k):
    """>= 25 identical map points under the reading: nnk_wg_kernel's CAPQ = 24 list overflows and repeats; ties by index"""
    run_case(amd, oracle, "clusters", base(knn=k, knn_wg_from=1))


@pytest.mark.parametrize("k", [1, 6])
def test_piece_list_overflow(amd, oracle, k):
    """The second round of the workgroup matchers' piece count (wg_rows_to_pieces: more pieces than the list holds, so every lane counts
    again with longer pieces).  Scene `dense_spot`: 2 000 distinct map points in a 2 cm ball around the place of one reading point, and 256
    more reading points in a 2 cm ball around that point.  The tile sort puts the 256 next to each other, so whole workgroups of 64 hold
    nothing else; once the registration has converged each of them has the 2 000 among its candidates (split over several rows they make
    more pieces, not fewer), and a workgroup needs only 9 such queries to overflow:  k = 1 (nn1_wg_kernel, pieces of 16, list of 1 024): 9 x ceil(2000 / 16) = 1 125
    > 1 024;  k = 6 (nnk_wg_kernel from iteration 1 on, pieces of 8, list of 896): 9 x ceil(2000 / 8) = 2 250 > 896.  The test cannot see
    the branch: these sizes are what guarantees it, and the matches of iterations 1 - 3 and of the checked chain's last counted iteration are
    held row by row to the oracle and the exact float64 search like every other scene's."""
    run_case(amd, oracle, "dense_spot", base(knn=k, knn_wg_from=1) if k == 6 else base(knn=k))


@pytest.mark.parametrize("k", [1, 6])
def test_large_initial_misalignment(amd, oracle, k):
    run_case(amd, oracle, "misaligned", base(knn=k))


@pytest.mark.parametrize("k", [1, 6])
def test_reading_contains_map_points(amd, oracle, k):
    """exact-zero d2 in the first iteration's fused selection: not distances to the quantile"""
    run_case(amd, oracle, "exact_hits", base(knn=k), js=(1, 2))


@pytest.mark.parametrize("k", [1, 6])
def test_bundled_lidar_scans(amd, oracle, k):
    run_case(amd, oracle, "bundled", base(minimizer=1, knn=k))


def test_shipped_epsilon_config(amd, oracle):
    """knn 6, epsilon 1 with libnabo's pruning (examples/config.yaml): the per-query (1 + eps) guarantee inside the loop"""
    run_case(amd, oracle, "mid", base(knn=6, epsilon=1.0, epsilon_approx=1, outliers=[]))


@pytest.mark.parametrize("k", [1, 6])
def test_checked_loop_eager_run_ahead(amd, oracle, k):
    """the checked chain without graphs: eager iterations enqueued ahead of the progress word, dead ones behind the stop"""
    run_case(amd, oracle, "mid", base(knn=k, use_graph=0), js=(1,), checked_graph=0)


def test_headline_shape(amd, oracle):
    """100 k x 1 M, k = 1, point-to-plane: nn1_wg_kernel with every workgroup resident"""
    run_case(amd, oracle, "headline", base(), js=())
