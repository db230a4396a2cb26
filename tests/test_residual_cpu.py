"""getResidualError without a GPU: the restatements of tests/residual_reference.py on a hand-made case, the float32-against-float64
figure the GPU tests' tolerance is made of (profiles/residual_tolerance.json), the inputs of tests/test_gpu_residual.py (every reading
has a pair to score; the brute-force comparison does not hinge on a near-tie), and the three new symbols and icpmi_residual's layout in
header, library and ctypes table."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import residual_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------------------------------------------------------ hand-made case
def _hand():
    """seven slots: five error elements with r = 1, 2, 0.5, 3, 0.25 (point-to-point) -- one of them with the soft weight 0.3 --, a
    zero-weight pair and an unfilled slot"""
    p = np.zeros((7, 3), F)
    q = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 0.5], [3, 0, 0], [0, 0.25, 0], [9, 9, 9], [0, 0, 0]], F)
    n = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1], [1, 0, 0], [1, 0, 0]], F)
    w = np.array([1, 1, 0.3, 1, 1, 0, 1], F)
    filled = np.array([1, 1, 1, 1, 1, 1, 0], bool)
    d2 = np.where(filled, rr.sqdist3_f32(p, q), np.inf).astype(F)
    return p, q, n, w, filled, d2


def test_hand_made_point_to_point():
    p, q, n, w, filled, d2 = _hand()
    s = rr.summarise(rr.residuals_f32(1, p, q, n, d2), w, filled)
    assert s["pairs"] == 5
    assert s["sum_abs"] == 1 + 2 + 0.5 + 3 + 0.25             # the soft pair with its full r, the zero-weight and unfilled ones left out
    assert s["sum_sq"] == 1 + 4 + 0.25 + 9 + 0.0625
    assert s["max_abs"] == F(3)
    assert s["weight_sum"] == pytest.approx(4 + float(F(0.3)), abs=0)


def test_hand_made_point_to_plane_and_planar():
    p, q, n, w, filled, d2 = _hand()
    s = rr.summarise(rr.residuals_f32(2, p, q, n, d2), w, filled)
    assert s["pairs"] == 5 and s["sum_abs"] == 1 + 2 + 0.5 + 0 + 0 and s["max_abs"] == F(2)    # pairs 3 and 4 lie in their planes
    s2 = rr.summarise(rr.residuals_f32(2, p, q, n, d2, planar=True), w, filled)
    assert s2["pairs"] == 5 and s2["sum_abs"] == 1 + 2 + 0 + 0 + 0                             # ... and the z term of pair 2 is dropped
    T = np.eye(4, dtype=F)
    reading = np.concatenate([p, np.ones((7, 1), F)], 1)
    for kind, planar, want in ((1, False, 6.75), (2, False, 3.5), (2, True, 3.0)):
        got = rr.summarise(rr.residuals_f64(kind, reading, T, q, n, planar), w, filled)
        assert got["pairs"] == 5 and got["sum_abs"] == pytest.approx(want, rel=1e-15)


def test_centred_pose_is_the_pose_in_the_centred_frame():
    sc = rr.scene()
    mean = rr.map_mean64(sc["map"]).astype(F)
    Tc = rr.centred_pose(sc["pose"], mean).astype(np.float64)
    x = sc["scan"][:50, :3].astype(np.float64)
    a = (x - mean) @ Tc[:3, :3].T + Tc[:3, 3]
    b = x @ sc["pose"][:3, :3].astype(np.float64).T + sc["pose"][:3, 3] - mean
    assert np.abs(a - b).max() < 1e-6
    assert np.array_equal(rr.centred_pose(np.eye(4, dtype=F), mean), np.eye(4, dtype=F))


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_every_reading_has_a_pair_and_maxdist_bites():
    for sc in (rr.scene(), rr.planar_scene()):
        assert sc["map"].shape == (rr.M, 4) and sc["scan"].shape == (max(rr.NS), 4)
        T = sc["pose"].astype(np.float64)
        moved = sc["scan"][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        ids, _, _ = rr.brute_knn(moved, sc["map"][:, :3], 6, sc["max_dist"])
        filled = (ids >= 0).sum(1)
        assert filled[0] >= 1                                   # n = 1 has something to score
        assert (filled == 0).sum() >= 3                         # some queries match nothing
        assert ((filled > 0) & (filled < 6)).sum() >= 100       # ... and some fewer than six


def moved3d():
    sc = rr.scene()
    T = sc["pose"].astype(np.float64)
    return sc["scan"][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def test_float32_formulation_tolerance():
    """the float32 restatement against float64 over the GPU tests' scenes, written to profiles/residual_tolerance.json; the GPU tests
    allow four times the figure of the kind they check.  Point-to-point is a few float32 epsilons; a point-to-plane residual is the
    small difference of coordinates of a few metres, so its sums carry the coordinates' rounding (least when one pair is all there is)."""
    worst = rr.measure_tolerance()
    doc = {"what": "max over sum_abs, sum_sq of |float32 restatement - float64| / float64 over tests/residual_reference.py's scenes "
                   "(3-D and flattened; map %d, n in %s, k in %s, MaxDist pair sets from exact neighbours, the scene's pose)" % (rr.M, list(rr.NS), list(rr.KS)),
           "measured": max(worst.values()), "by_kind": worst, "float32_eps": float(np.finfo(F).eps),
           "device_bound": "4 x by_kind (tests/residual_reference.py: device_bound)",
           "measured_on": "CPU (numpy float32 / float64)"}
    with open(rr.TOLERANCE_JSON, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("residual float32 vs float64:", worst)
    assert 0 < worst["1"] < 16 * np.finfo(F).eps
    assert 0 < worst["1_planar"] < 1e-3
    assert all(0 < worst[name] < 1e-2 for name in ("2", "2_force2d", "2_planar"))


def test_brute_force_comparison_does_not_hinge_on_a_near_tie():
    """test_gpu_residual's comparison against exact float64 neighbours (kind 1, MaxDist, n = 257): a flipped nearest / second-nearest
    pair changes the sum by at most the gap between the two; the gaps that float32 rounding could flip (below 1e-5 m) add up to less
    than the tolerance times the sum"""
    sc = rr.scene()
    _, d2, gap = rr.brute_knn(moved3d()[:257], sc["map"][:, :3], 1, rr.MAX_DIST)
    total = np.sqrt(d2[np.isfinite(d2)]).sum()
    flippable = gap[gap < 1e-5].sum()
    assert flippable <= rr.device_bound("1") * total, (flippable, total)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_residual_error", "icpmi_residual_error_dev", "icpmi_residual_error_staged")
FIELDS = ("sum_abs", "sum_sq", "max_abs", "weighted_point_used_ratio", "weight_sum", "pairs", "trimmed_limit", "kind", "reserved")


def test_header_library_and_ctypes_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name: args for name, _, args in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported, sym
        assert sym in bound, sym
    assert len(bound["icpmi_residual_error"]) == len(bound["icpmi_residual_error_dev"]) == 7 and len(bound["icpmi_residual_error_staged"]) == 4
    assert (_capi.RES_CHAIN, _capi.RES_POINT_TO_POINT, _capi.RES_POINT_TO_PLANE) == (0, 1, 2)
    from norlab_icp_mapper_amd import icp
    for name in ("residual", "residualDev", "residualStaged"):
        assert callable(getattr(icp.ICPSequence, name))
    assert callable(icp._ErrorMinimizerView.getResidualError)


def test_residual_struct_layout_and_unchanged_sizes(tmp_path):
    from norlab_icp_mapper_amd import _capi
    src = tmp_path / "res.c"
    offs = ", ".join("offsetof(icpmi_residual, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icpmi.h"\nint main(void) { printf("%%zu %%zu %%zu %%d %%d %%d' % ()
                   + " %zu" * len(FIELDS) + '\\n", sizeof(icpmi_residual), sizeof(icpmi_config), sizeof(icpmi_stats), (int)ICPMI_RES_CHAIN, '
                   '(int)ICPMI_RES_POINT_TO_POINT, (int)ICPMI_RES_POINT_TO_PLANE, ' + offs + "); return 0; }\n")
    exe = tmp_path / "res"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_capi.Residual) == 64
    assert got[1] == C.sizeof(_capi.Config) == 5 * 4 + 8 * 20 + 15 * 4 + 8 * 4          # as before the feature
    assert got[2] == C.sizeof(_capi.Stats) == 72
    assert got[3:6] == [0, 1, 2]
    assert got[6:] == [getattr(_capi.Residual, f).offset for f in FIELDS]
    assert _capi.load().icpmi_version() == 4
