"""The voxel pose score without a GPU: the float64 reference (tests/voxel_score_reference.py) against the figures of the prototype the
feature rests on, the ranking condition the GPU test relies on, rank_voxel_candidates on both sides of the C ABI against hand-written
tables, the record the GPU test takes its allowances from, and the C ABI's new symbols and struct layouts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_score_cases as vsc
import voxel_score_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rankings():
    return {key: vsc.ranking_case(*key) for key in vsc.PROTOTYPE}


# ------------------------------------------------------------------------------------------------------------------ the prototype
@pytest.mark.parametrize("key", list(vsc.PROTOTYPE))
def test_prototype_table_is_reproduced(rankings, key):
    """the six cells of the issue's table, to the three digits quoted: the best candidate is the grid's centre, and likelihood / n of the
    best and of the second best round to the figures"""
    L = rankings[key]
    order = sorted(range(L.size), key=lambda i: (-L[i], i))
    best, second = vsc.PROTOTYPE[key]
    print(key, order[0], L[order[0]], L[order[1]])
    assert order[0] == vsc.CENTRE
    assert abs(L[order[0]] - best) <= 0.5e-3 and abs(L[order[1]] - second) <= 0.5e-3


@pytest.mark.parametrize("key", list(vsc.PROTOTYPE))
def test_runner_up_is_five_percent_behind_in_float64(rankings, key):
    """what the device's ranking test rests on: the float32 error of a likelihood is orders of magnitude below the gap"""
    L = np.sort(rankings[key])[::-1]
    print(key, L[1] / L[0])
    assert L[1] <= vsc.RUNNER_UP_MAX * L[0]


def test_mean_objective_does_not_rank():
    """why the score is a bounded likelihood: at size 1.0 the mean of d^T M d prefers a candidate 1.5 m or more from the truth"""
    c = vsc.inputs()
    means = []
    for G in vsc.grid():
        r = sr.score64(G.astype(np.float32), c["rc"], c["rn"], c["tab"][1.0])
        means.append(r["sum_maha"] / max(r["pairs"], 1) if r["pairs"] else np.inf)
    assert int(np.argmin(means)) != vsc.CENTRE


# ------------------------------------------------------------------------------------------------------------------ ranking
OK, INVALID_ARG, NO_POINT = 0, 1, 3
TABLES = [
    # (rows of (status, pairs, likelihood), n, min_pairs_ratio, expected order)
    ([(OK, 90, 50.0), (OK, 80, 70.0), (OK, 100, 60.0)], 100, 0.0, [1, 2, 0]),
    ([(OK, 90, 50.0), (INVALID_ARG, 0, 0.0), (NO_POINT, 0, 0.0), (OK, 10, 55.0)], 100, 0.0, [3, 0]),             # dropped statuses
    ([(OK, 49, 99.0), (OK, 50, 10.0), (OK, 51, 5.0)], 100, 0.5, [1, 2]),                                          # the ratio guard: 49 < 50
    ([(OK, 10, 7.0), (OK, 20, 7.0), (OK, 30, 8.0), (OK, 40, 7.0)], 40, 0.0, [2, 0, 1, 3]),                        # ties by the lower index
    ([(OK, 0, 0.0), (NO_POINT, 0, 0.0)], 10, 0.0, []),                                                            # nothing survives
    ([(OK, 3, 1e-300), (OK, 3, 2e-300)], 3, 1.0, [1, 0]),
]


@pytest.mark.parametrize("case", range(len(TABLES)))
def test_rank_voxel_candidates_python(case):
    from norlab_icp_mapper_amd import icp
    rows, n, ratio, want = TABLES[case]
    assert icp.rank_voxel_candidates(rows, n, ratio) == want
    assert sr.rank(rows, n, ratio) == want


@pytest.mark.parametrize("case", range(len(TABLES)))
def test_rank_voxel_candidates_cpp(case):
    import host_voxel_score_bindings as hv
    rows, n, ratio, want = TABLES[case]
    assert hv.rank(rows, n, ratio) == want


def test_rank_takes_a_voxel_pose_scores():
    from norlab_icp_mapper_amd import _capi, icp
    cs = []
    for lik, pairs in ((3.0, 5), (4.0, 5), (0.0, 0)):
        c = _capi.VoxelScore()
        c.likelihood, c.pairs = lik, pairs
        cs.append(icp.VoxelScore(c))
    scores = icp.VoxelPoseScores(cs, [0, 0, 3])
    assert scores.table() == [(0, 5, 3.0), (0, 5, 4.0), (3, 0, 0.0)] and len(scores) == 3
    assert icp.rank_voxel_candidates(scores, 5) == [1, 0]
    assert scores.bits()[0][1] == cs[0].bits() and scores.bits()[0] != scores.bits()[1]


# ------------------------------------------------------------------------------------------------------------------ the record
def test_recorded_tolerances_are_what_the_script_measures():
    import importlib.util
    spec = importlib.util.spec_from_file_location("voxel_score_tolerance", os.path.join(ROOT, "scripts", "voxel_score_tolerance.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    rec, got = vsc.recorded(), script.measure()
    assert set(rec["rel"]) == set(got["rel"]) == {vsc.case_key(s, p, n) for s in vsc.SIZES for p in vsc.POSES for n in vsc.N_VALUES}
    for key, want in got["rel"].items():                                                             # every one of the 66 cases
        have = rec["rel"][key]
        assert have["pairs"] == want["pairs"], key
        assert have["likelihood"] == pytest.approx(want["likelihood"], rel=1e-6, abs=1e-18), key
        assert have["sum_maha"] == pytest.approx(want["sum_maha"], rel=1e-6, abs=1e-18), key
    for k in ("expf_ulp_bound", "likelihood_floor_units", "roundoff", "margin"):
        assert rec[k] == got[k]
    for key, want in got["ranking"].items():
        assert rec["ranking"][key]["best"] == want["best"]
        assert rec["ranking"][key]["best_likelihood_per_point"] == pytest.approx(want["best_likelihood_per_point"], rel=1e-9)
    worst = max(max(v["likelihood"], v["sum_maha"]) for v in rec["rel"].values())
    assert 0 < worst < 1e-3
    # the floor is the documented bound of expf in units of float32 roundoff, not a measured figure
    assert rec["expf_ulp_bound"] == 1.0 and rec["likelihood_floor_units"] == 2.0 * rec["expf_ulp_bound"] and rec["roundoff"] == 2.0 ** -24
    assert rec["margin"] == 4.0
    for key, (best, second) in vsc.PROTOTYPE.items():
        got = rec["ranking"][f"{key[0]}/{key[1]}"]
        assert got["best"] == vsc.CENTRE and round(got["best_likelihood_per_point"], 3) == best and round(got["second_likelihood_per_point"], 3) == second


def test_centred_pose_is_the_host_expression():
    """the reference forms the centred pose as api.hip does: the text of the expression is there, and a pose built for a centred-frame target
    comes back within a float32 rounding of it"""
    api = open(os.path.join(ROOT, "norlab_icp_mapper_amd", "csrc", "api.hip")).read()
    assert "(double)T[12 + r] + (((double)T[r] * (double)h->mean[0] + (double)T[4 + r] * (double)h->mean[1]) + (double)T[8 + r] * (double)h->mean[2])" in api
    c = vsc.inputs()
    for name, Tc in vsc.POSES.items():
        T, back = vsc.map_frame(Tc, c["mean"])
        assert np.abs(back.astype(np.float64) - Tc).max() <= 8 * 2.0 ** -24 * (1 + np.abs(c["mean"]).max() + np.abs(Tc[:3, 3]).max()), name


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_voxel_score_poses", "icpmi_voxel_score_poses_dev")
NEW_VOID = ("icpmi_voxel_score_options_default", "icpmi_voxel_score_shape")


def test_header_library_and_bindings_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
    for sym in NEW_VOID:
        assert re.search(r"void\s+%s\s*\(" % sym, header), sym
    for sym in NEW_SYMBOLS + NEW_VOID:
        assert sym in exported and sym in bound, sym


def test_struct_layouts(tmp_path):
    from norlab_icp_mapper_amd import _capi
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icpmi.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(icpmi_voxel_score_options), offsetof(icpmi_voxel_score_options, beta), sizeof(icpmi_voxel_score), '
                   'offsetof(icpmi_voxel_score, likelihood), offsetof(icpmi_voxel_score, sum_maha), offsetof(icpmi_voxel_score, pairs), '
                   'offsetof(icpmi_voxel_score, max_maha), offsetof(icpmi_voxel_score, pairs_ratio), offsetof(icpmi_voxel_score, level), '
                   'offsetof(icpmi_voxel_score, reserved)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    O, S = _capi.VoxelScoreOptions, _capi.VoxelScore
    assert got == [C.sizeof(O), O.beta.offset, C.sizeof(S), S.likelihood.offset, S.sum_maha.offset, S.pairs.offset, S.max_maha.offset,
                   S.pairs_ratio.offset, S.level.offset, S.reserved.offset]
    assert got[0] == 32 and got[2] == 48


def test_options_default_and_shape_need_no_device():
    from norlab_icp_mapper_amd import _capi
    lib = _capi.load()
    o = _capi.VoxelScoreOptions()
    o.level, o.beta, o.reserved[0] = 7, 9.0, 5
    lib.icpmi_voxel_score_options_default(C.byref(o))
    assert (o.level, o.beta, list(o.reserved)) == (-1, 1.0, [0] * 6)
    sl, tl = C.c_int32(0), C.c_int32(0)
    lib.icpmi_voxel_score_shape(C.byref(sl), C.byref(tl))
    assert (sl.value, tl.value) == (vsc.SLICE, vsc.TILE) and sl.value % 256 == 0
