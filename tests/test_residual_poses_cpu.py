"""Scoring many poses and relocalising from them, without a GPU: the ranking rule (icp.rank_candidates and the host shell's
rankCandidates) against hand-written tables, the candidate generator's order and count on both sides, the new symbols of the C ABI, and
the relocalisation case of tests/test_gpu_residual_poses.py: a float64 reference with exact neighbours ranks the true candidate first
with a mean residual at most half the runner-up's, so the GPU test's winner is not a matter of luck."""
import os
import re
import subprocess

import numpy as np
import pytest

import relocalize_bindings as rb
import relocalize_cases as rc
from test_host_cpp import _build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# (status, pairs, sum_abs) rows and, for n = 100 and ratio 0.5, the expected order
TABLES = {
    "plain": ([(0, 80, 8.0), (0, 90, 4.5), (0, 100, 20.0)], [1, 0, 2]),                      # means 0.1, 0.05, 0.2
    "tie_goes_to_the_lower_index": ([(0, 60, 6.0), (0, 80, 4.0), (0, 50, 2.5), (0, 100, 5.0)], [1, 2, 3, 0]),   # 0.1, 0.05, 0.05, 0.05
    "failed_status": ([(4, 100, 0.1), (0, 70, 7.0), (3, 0, 0.0), (2, 90, 0.9)], [1]),
    "too_few_pairs": ([(0, 49, 0.001), (0, 50, 5.0), (0, 51, 10.2)], [1, 2]),                # 49 < 0.5 * 100 is out, 50 stays
    "nobody_survives": ([(4, 0, 0.0), (0, 10, 0.1), (2, 0, 0.0)], []),
    "empty": ([], []),
}


@pytest.mark.parametrize("name", list(TABLES))
def test_rank_candidates_by_hand(name):
    from norlab_icp_mapper_amd.icp import rank_candidates
    table, want = TABLES[name]
    _build_host()
    assert rank_candidates(table, 100, 0.5) == want
    assert rb.rank_candidates(table, 100, 0.5) == want


def test_rank_candidates_ratio_is_a_float32():
    """0.1f is a little above 0.1: 10 pairs of 100 points are too few on both sides of the C ABI"""
    from norlab_icp_mapper_amd.icp import rank_candidates
    table = [(0, 10, 1.0), (0, 11, 1.0)]
    _build_host()
    assert rank_candidates(table, 100, 0.1) == [1]
    assert rb.rank_candidates(table, 100, 0.1) == [1]


def test_rank_candidates_reads_pose_scores():
    from norlab_icp_mapper_amd import _capi, icp
    rows = []
    for pairs, s in ((80, 8.0), (90, 4.5)):
        r = _capi.Residual(); r.pairs = pairs; r.sum_abs = s
        rows.append(icp.Residual(r))
    assert icp.rank_candidates(icp.PoseScores(rows, [0, 0], 2), 100, 0.5) == [1, 0]
    assert icp.rank_candidates(icp.PoseScores(rows, [0, 4], 2), 100, 0.5) == [0]


def test_candidate_grid_order_and_count():
    from norlab_icp_mapper_amd import synth
    from norlab_icp_mapper_amd.icp import candidate_grid
    centre = synth.make_T((0.01, -0.02, 0.3), (1.0, -2.0, 0.5)).astype(F)
    g = candidate_grid(centre, 0.6, 0.4, 0.2, 2, 1, 1)
    assert g.shape == (5 * 3 * 3, 4, 4) and g.dtype == F
    assert np.array_equal(g[0], centre)                                   # the centre first, bit for bit
    want = [(0, 0, 0)] + [(ix, iy, ia) for ia in (-1, 0, 1) for iy in (-1, 0, 1) for ix in (-2, -1, 0, 1, 2) if (ix, iy, ia) != (0, 0, 0)]
    for row, (ix, iy, ia) in zip(g, want):
        a = 0.2 * ia
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        assert np.allclose(row[:3, :3], Rz @ centre[:3, :3].astype(np.float64), atol=1e-6)
        assert np.allclose(row[:3, 3], centre[:3, 3] + np.array([0.6 * ix / 2, 0.4 * iy, 0.0]), atol=1e-6)
        assert np.array_equal(row[3], np.array([0, 0, 0, 1], F))
    assert len({row.tobytes() for row in g}) == g.shape[0]
    assert np.array_equal(candidate_grid(centre, 0.6, 0.4, 0.2, 2, 1, 1), g)              # deterministic
    assert candidate_grid(centre, 0.6, 0.4, 0.2, 0, 0, 0).shape == (1, 4, 4)
    assert candidate_grid(centre, 0.6, 0.4, 0.2, 0, 3, 0).shape == (7, 4, 4)


def test_candidate_grid_of_the_host_shell_is_the_same_grid():
    from norlab_icp_mapper_amd.icp import candidate_grid
    _build_host()
    for steps in ((1, 1, 1), (2, 0, 1), (0, 0, 0)):
        a = candidate_grid(rc.guess_pose(), rc.HALF_X, rc.HALF_Y, rc.HALF_YAW, *steps)
        b = rb.candidate_grid(rc.guess_pose(), rc.HALF_X, rc.HALF_Y, rc.HALF_YAW, *steps)
        assert a.shape == b.shape
        assert np.array_equal(a[0], b[0])
        assert np.abs(a.astype(np.float64) - b).max() <= 2e-7             # (cos and sin come from two libraries: an ulp of float32 at most)


def test_compose_pose_is_the_float32_product_in_order():
    from norlab_icp_mapper_amd.icp import compose_pose
    rng = np.random.default_rng(5)
    A = rng.standard_normal((4, 4)).astype(F); B = rng.standard_normal((4, 4)).astype(F)
    want = np.empty((4, 4), F)
    for i in range(4):
        for j in range(4):
            s = F(0)
            for k in range(4):
                s = F(s + F(A[i, k] * B[k, j]))
            want[i, j] = s
    assert np.array_equal(compose_pose(A, B), want)


def test_reference_separates_the_true_candidate(oracle):
    """the candidate set of the GPU relocalisation test, in float64 with exact neighbours: the true candidate comes first with a mean
    residual at most half the runner-up's in the ranking of the candidates AND -- the best four refined by the CPU oracle's loop -- in
    the ranking of the refined poses, none of which lands on the true candidate's"""
    from norlab_icp_mapper_amd import synth
    from norlab_icp_mapper_amd.icp import rank_candidates
    cand = rc.candidates()
    assert cand.shape == (27, 4, 4)
    assert np.abs(cand[rc.TRUE_INDEX].astype(np.float64) - rc.near_pose()).max() <= 1e-6   # the grid holds the pose near the truth
    table = rc.reference_table(cand=cand)
    n = rc.rr.scene()["scan"].shape[0]
    order = rank_candidates(table, n, 0.5)
    mean = lambda t, i: t[i][2] / t[i][1]
    assert len(order) >= 4
    assert order[0] == rc.TRUE_INDEX
    assert mean(table, order[0]) <= 0.5 * mean(table, order[1]), [(i, table[i][1], mean(table, i)) for i in order[:4]]
    poses, again = rc.refined_reference(oracle, order, refine=4, cand=cand)
    final = rank_candidates(again, n, 0.5)
    assert final and final[0] == 0, again                                                  # position 0 of the four = the true candidate
    if len(final) > 1:
        assert mean(again, final[0]) <= 0.5 * mean(again, final[1]), again
    for other in poses[1:]:                                                                # no runner-up refined onto the winner's pose
        dt, dr = synth.pose_error(other, poses[0])
        assert dt > 0.5 * rc.HALF_X or dr > 0.5 * rc.HALF_YAW, (dt, dr)


NEW_SYMBOLS = ("icpmi_residual_error_poses", "icpmi_residual_error_poses_dev", "icpmi_register_multistart_dev", "icpmi_register_multistart")


def test_new_exports_are_declared_exported_and_bound():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported, sym
        assert sym in bound, sym
    from norlab_icp_mapper_amd import icp
    for name in ("residuals", "residualsDev", "registerMultiStartDev", "relocalize"):
        assert callable(getattr(icp.ICPSequence, name))
