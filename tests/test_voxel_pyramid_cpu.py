"""The scheduled VoxelMatcher registration without a GPU: the float64 reference reproduces the issue's prototype table, the
margins under which iteration counts may be compared exactly hold for the cases the GPU tests use, the recorded tolerances are what the
script measures, both YAML front ends read `voxelSizes` by the ABI's rules, and header, library and bindings agree on the new symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_cases as vc
import voxel_pyramid_cases as pc
import voxel_pyramid_reference as vpr
import voxel_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the prototype table
@pytest.mark.parametrize("sizes", pc.SCHEDULES, ids=lambda s: ",".join(map(str, s)))
def test_prototype_table_row(sizes):
    for k in pc.STARTS:
        _, rd, _, truth = pc.registration_inputs(k)
        res = pc.reference_run(k, sizes)
        et, er = vr.centroid_error(res["T"], truth, rd)
        want = pc.PROTOTYPE[sizes][k]
        print(f"{sizes} x{k}: {et:.4e} m / {er:.2e} rad (the issue prints {want:g}), report {vpr.report(res)}")
        assert res["status"] == "ok"
        assert abs(et - want) <= pc.printed(want), (sizes, k, et, want)


def test_what_the_table_says():
    err = lambda k, s: vr.centroid_error(pc.reference_run(k, s)["T"], pc.registration_inputs(k)[3], pc.registration_inputs(k)[1])[0]
    # 0.5 m alone is lost from x3 on, 1.0 m alone from x6
    assert err(2, (0.5,)) < 1.1 * pc.FLOOR and all(err(k, (0.5,)) > 1e-2 for k in (3, 4, 6))
    assert err(4, (1.0,)) < 3e-4 and err(6, (1.0,)) > 0.1
    # both working schedules are at the 0.5 m floor from every start, x6 included
    for s in pc.WORKING:
        for k in pc.STARTS:
            assert abs(err(k, s) - pc.FLOOR) <= pc.printed(pc.FLOOR), (s, k)
    # the false minimum: a schedule that starts at 2 m in this 4 m wide room settles more than 1 m off from x2 on, and stays there
    assert err(1, (2.0, 1.0, 0.5)) < 1.1 * pc.FLOOR
    for k in (2, 3, 4, 6):
        assert err(k, (2.0,)) > 1.0 and err(k, (2.0, 1.0, 0.5)) > 1.0


def test_prototype_counts():
    for k, want in pc.PROTOTYPE_ITERATIONS.items():
        res = pc.reference_run(k, (4.0, 2.0, 1.0, 0.5))
        assert tuple(lv["iterations"] for lv in res["levels"]) == want
        assert res["iterations"] == sum(want)
    # 4.20's figures, which a schedule of one reproduces: 877 of 2000 points find a voxel at 0.5 m from the x1 start, 1902 at 1 m
    for size, (_, _, its, pairs) in vc.PROTOTYPE.items():
        if its is not None:
            res = pc.reference_run(1, (size,))
            assert vpr.report(res)[0][:2] == (its, pairs)


def test_a_schedule_of_one_is_the_one_size_loop():
    sc, rd, rn, _ = pc.registration_inputs(1)
    for precision in (64, 32):
        a = vr.register(sc["map"], sc["normals"], rd, rn, 1.0, precision)
        b = pc.reference_run(1, (1.0,), precision)
        assert np.array_equal(a["T"], b["T"]) and a["iterations"] == b["iterations"] and a["pairs"] == b["levels"][0]["pairs"]


def test_a_later_level_starts_with_an_empty_history():
    """the pose carried over is not an entry: a level after the first runs at least smoothLength + 1 iterations (the prototype's 4 and 4)"""
    res = pc.reference_run(1, (1.0, 0.5))
    assert [lv["iterations"] for lv in res["levels"]] == [5, 4]
    assert res["levels"][1]["checks"][:3] == [None, None, None] and res["levels"][0]["checks"][:2] == [None, None]
    assert res["levels"][0]["checks"][2] is not None


# ------------------------------------------------------------------------------------------------------------------ margins
@pytest.mark.parametrize("sizes", pc.WORKING, ids=lambda s: ",".join(map(str, s)))
@pytest.mark.parametrize("k", pc.STARTS)
def test_margins(k, sizes):
    """every Differential decision of the float64 loop lies further from the thresholds than the float32 restatement lies from float64 at
    that check: the condition under which the GPU tests compare iteration counts exactly.  No start had to be moved."""
    r64, r32 = pc.reference_run(k, sizes, 64), pc.reference_run(k, sizes, 32)
    ok, worst = vpr.margins(r64, r32)
    print(f"x{k} {sizes}: worst slack {worst:.3f} of a threshold; float32 report {vpr.report(r32)}")
    assert ok
    assert vpr.report(r32) == vpr.report(r64)
    assert all(lv["stop"] == "differential" for lv in r64["levels"])


def test_gpu_cases_are_among_those_whose_margins_hold():
    rec = pc.recorded()["registration_room"]
    for k, sizes in pc.GPU_CASES:
        assert rec[pc.case_key(k, sizes)]["margins_hold"]
    assert {(k, s) for k, s in pc.GPU_CASES} >= {(k, s) for s in pc.WORKING for k in (1, 3, 6)}


def test_recorded_tolerances_are_what_the_script_measures():
    rec = pc.recorded()
    for k, sizes in pc.GPU_CASES:
        _, rd, _, truth = pc.registration_inputs(k)
        r64, r32 = pc.reference_run(k, sizes, 64), pc.reference_run(k, sizes, 32)
        dt, dr = vc.pose_distance(r32["T"], r64["T"], rd)
        r = rec["registration_room"][pc.case_key(k, sizes)]
        assert r["float32_from_float64_trans"] == pytest.approx(dt, rel=1e-6) and r["float32_from_float64_rot"] == pytest.approx(dr, rel=1e-6)
        assert [tuple(x) for x in r["float32_report"]] == vpr.report(r32)
        t = rec["prototype_table"][pc.case_key(k, sizes)]
        assert t["trans_err"] == pytest.approx(vr.centroid_error(r64["T"], truth, rd)[0], rel=1e-6)
        assert [tuple(x) for x in t["report"]] == vpr.report(r64)


def test_counter_and_fixed_counts_per_level():
    """maxIterationCount 3: the Counter, not the Differential checker, moves every level on; a fixed count runs at every level"""
    res = pc.reference_run(1, (4.0, 2.0, 1.0, 0.5), 64, max_iter=3)
    assert [lv["iterations"] for lv in res["levels"]] == [3, 3, 3, 3] and all(lv["stop"] == "counter" for lv in res["levels"])
    res = pc.reference_run(1, (4.0, 2.0, 1.0, 0.5), 64, max_iter=2, differential=None)
    assert [lv["iterations"] for lv in res["levels"]] == [2, 2, 2, 2] and res["iterations"] == 8


# ------------------------------------------------------------------------------------------------------------------ config parsing
CHAIN = {"matcher": {"VoxelMatcher": {"voxelSizes": [4.0, 2.0, 1.0, 0.5]}}, "errorMinimizer": {"PlaneToPlaneErrorMinimizer": {"epsilon": 0.01}}}
BAD_LISTS = [("ascending", [0.5, 1.0], "strictly descending"), ("a repeat", [1.0, 1.0, 0.5], "strictly descending"), ("empty", [], "1 to 4"),
             ("five entries", [5.0, 4.0, 2.0, 1.0, 0.5], "1 to 4"), ("a non-finite entry", [float("inf"), 1.0], "finite and > 0"),
             ("a NaN entry", [2.0, float("nan")], "finite and > 0"), ("a zero entry", [1.0, 0.0], "finite and > 0")]


def _cfg(params):
    from norlab_icp_mapper_amd import icp
    return icp.config_from_yaml_chain({**CHAIN, "matcher": {"VoxelMatcher": params}})


def test_python_yaml():
    from norlab_icp_mapper_amd import icp
    c = _cfg({"voxelSizes": [4.0, 2.0, 1.0, 0.5]})
    assert c.voxel_sizes == [4.0, 2.0, 1.0, 0.5] and c.voxel_size == 0.5 and c.minimizer == 3
    assert _cfg({"voxelSizes": [1.0]}).voxel_sizes == [1.0]
    assert not hasattr(_cfg({"voxelSize": 0.5}), "voxel_sizes")
    with pytest.raises(icp.InvalidParameter, match="voxelSize and voxelSizes"):
        _cfg({"voxelSize": 0.5, "voxelSizes": [1.0, 0.5]})
    for what, bad, word in BAD_LISTS:
        with pytest.raises(icp.InvalidParameter, match="VoxelMatcher.*" + word):
            _cfg({"voxelSizes": bad})
    with pytest.raises(icp.InvalidParameter, match="voxelSizes"):
        _cfg({"voxelSizes": 0.5})
    with pytest.raises(icp.InvalidParameter, match="voxel matcher.*outlier filters"):
        icp.config_from_yaml_chain({**CHAIN, "outlierFilters": [{"TrimmedDistOutlierFilter": {"ratio": 0.85}}]})
    with pytest.raises(icp.InvalidParameter, match="voxel_size and voxel_sizes"):
        icp.ICPSequence(minimizer=3, voxel_size=0.5, voxel_sizes=[1.0, 0.5])   # (checked before the handle is created)
    with pytest.raises(icp.InvalidParameter, match="strictly descending"):
        icp.ICPSequence(minimizer=3, voxel_sizes=[0.5, 1.0])


def parse_voxel_schedule(yaml_matcher):
    """nim_test_parse_voxel_schedule (host/TestHooksVoxelSchedule.cpp): what parseMatcher reads of the entry, or RuntimeError"""
    import host_bindings as hb
    fn = hb.load().nim_test_parse_voxel_schedule
    fn.restype = C.c_int
    size, sizes, n = C.c_float(-1), (C.c_float * 4)(), C.c_int(-1)
    err = C.create_string_buffer(512)
    if fn(yaml_matcher.encode(), C.byref(size), sizes, C.byref(n), err, C.c_int(512)):
        raise RuntimeError(err.value.decode(errors="replace"))
    return size.value, [sizes[i] for i in range(n.value)]


def _yaml_list(values):
    word = lambda v: ".inf" if v == float("inf") else "nan" if v != v else repr(v)   # (the shell's scalars: ".inf" by name, the rest by strtof)
    return "[" + ", ".join(word(v) for v in values) + "]"


def test_cpp_yaml():
    assert parse_voxel_schedule("VoxelMatcher:\n  voxelSizes: [4.0, 2.0, 1.0, 0.5]\n") == (0.5, [4.0, 2.0, 1.0, 0.5])
    assert parse_voxel_schedule("VoxelMatcher:\n  voxelSizes:\n    - 1.0\n    - 0.5\n") == (0.5, [1.0, 0.5])
    assert parse_voxel_schedule("VoxelMatcher:\n  voxelSize: 0.5\n") == (0.5, [])
    assert parse_voxel_schedule("KDTreeMatcher:\n  knn: 1\n") == (0.0, [])
    with pytest.raises(RuntimeError, match="voxelSize and voxelSizes"):
        parse_voxel_schedule("VoxelMatcher:\n  voxelSize: 0.5\n  voxelSizes: [1.0, 0.5]\n")
    for what, bad, word in BAD_LISTS:
        with pytest.raises(RuntimeError, match="VoxelMatcher.*" + word):
            parse_voxel_schedule("VoxelMatcher:\n  voxelSizes: %s\n" % _yaml_list(bad))
    with pytest.raises(RuntimeError, match="VoxelMatcher: unknown parameter"):
        parse_voxel_schedule("VoxelMatcher:\n  voxelsizes: [1.0]\n")


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_set_voxel_schedule", "icpmi_get_voxel_schedule", "icpmi_get_voxel_map_level", "icpmi_voxel_lookup_level",
               "icpmi_get_voxel_schedule_report", "icpmi_debug_voxel_step_level")


def test_header_and_library_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported, sym
        assert sym in bound, sym
