"""Global localisation without a GPU: the integer reference's own properties (tests/global_localize_reference.py), its search against its
exhaustive maximum, the figures of the prototype the feature rests on, yaw_rotations on both sides of the C ABI, the refusals that need
no device, and the C ABI's new symbols and struct layouts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import global_localize_reference as glr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_MIN, A_MAX = (np.asarray(a, np.int64) for a in glr.WINDOW)


@pytest.fixture(scope="module")
def inputs():
    pyr, rd, mean = glr.scene_inputs(levels=6)
    return dict(pyr=pyr, rd=rd, mean=mean)


@pytest.fixture(scope="module")
def exhaustive(inputs):
    return glr.exhaustive(inputs["pyr"], inputs["rd"], A_MIN, A_MAX)


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def test_fmaf_rounds_once():
    """cases where rounding the product, or the double sum, first gives another float32"""
    f = np.float32
    a, b, c = f(1 + 2.0 ** -12), f(1 + 2.0 ** -12), f(-1.0)
    assert glr.fmaf(a, b, c) == f(2.0 ** -11 + 2.0 ** -24) and f(a * b) + c != glr.fmaf(a, b, c)
    # a tie of the double sum that the dropped bits break: 1 + 2^-24 (the float32 midpoint) + 2^-60
    assert glr.fmaf(f(2.0 ** -30), f(2.0 ** -30), f(1.0)) == f(1.0)
    x = glr.fmaf(f(1 + 2.0 ** -23), f(2.0 ** -1), f(0.5 - 2.0 ** -25))
    assert x == f(np.float64(1 + 2.0 ** -23) * 0.5 + np.float64(f(0.5 - 2.0 ** -25)))


def test_the_scene_is_the_prototypes(inputs):
    sc = glr.scene()
    assert sc["map"].shape == (8600, 4) and sc["reading"].shape == (1428, 4) and sc["rotations"].shape == (64, 3, 3)
    assert tuple(k.size for k in inputs["pyr"].keys[:4]) == glr.KEYS
    assert inputs["rd"].points == [1428] * 64


def test_bound_at_level_0_is_the_score(inputs, exhaustive):
    rng = np.random.default_rng(1)
    for _ in range(300):
        k = int(rng.integers(0, 64))
        a = np.array([rng.integers(A_MIN[j], A_MAX[j] + 1) for j in range(3)])
        assert glr.bound(inputs["pyr"], inputs["rd"], k, 0, a) == exhaustive[(k, *(a - A_MIN))]


@pytest.mark.parametrize("level", (1, 2, 3, 4, 5))
def test_bound_dominates_children_and_leaves(inputs, level):
    pyr, rd = inputs["pyr"], inputs["rd"]
    rng = np.random.default_rng(10 + level)
    w = 1 << level
    strict = 0
    for _ in range(60):
        k = int(rng.integers(0, 64))
        A = np.array([rng.integers(-14 >> level, (14 >> level) + 1), rng.integers(-24 >> level, (24 >> level) + 1), rng.integers(-4 >> level, (4 >> level) + 1)])
        b = glr.bound(pyr, rd, k, level, A)
        kids = max(glr.bound(pyr, rd, k, level - 1, 2 * A + e) for e in glr.E8)
        cube = glr.exhaustive(pyr, rd, A * w, A * w + w - 1, ks=[k])[k]
        assert b >= kids >= cube.max()
        strict += b > cube.max()
    assert strict > 0              # (the bound is not always tight: the search has something to prune with, and something to pay)


def test_search_equals_the_exhaustive_maximum_on_a_reduced_window(inputs):
    """16 rotations, 8 x 16 x 4 cells around the truth, four level counts and three batch sizes"""
    pyr = inputs["pyr"]
    sc = glr.scene()
    rot = sc["rotations"][::4]
    rd = glr.Reading(sc["reading"], rot, glr.S0)
    a_min, a_max = np.array([-3, -7, -2]), np.array([4, 8, 1])
    ex = glr.exhaustive(pyr, rd, a_min, a_max)
    assert ex.shape == (16, 8, 16, 4)
    top = int(ex.max())
    where = np.argwhere(ex == top)
    assert where.shape[0] == 1
    for levels in (1, 2, 4, 0):
        for batch in (1, 7, 4096):
            got = glr.search(pyr, rd, a_min, a_max, levels, batch)
            assert (got["found"], got["proven"], got["score"]) == (1, 1, top)
            assert (got["rotation"], *got["cell"]) == (where[0][0], *(where[0][1:] + a_min))
    assert glr.search(pyr, rd, a_min, a_max, 0, 64)["levels"] == 5      # 2^4 <= 16 cells < 2^5


# ------------------------------------------------------------------------------------------------------------------ the prototype's integers
def test_the_exhaustive_maximum_is_unique(exhaustive):
    assert exhaustive.size == glr.LEAVES
    flat = np.sort(exhaustive.ravel())
    assert (flat[-1], flat[-2]) == (glr.BEST["score"], glr.RUNNER_UP)
    k, x, y, z = np.argwhere(exhaustive == flat[-1])[0]
    assert (k, (x + A_MIN[0], y + A_MIN[1], z + A_MIN[2])) == (glr.BEST["rotation"], glr.BEST["cell"])


def test_the_maximiser_is_within_a_cell_and_a_yaw_step_of_the_truth(inputs):
    T = glr.pose_of(glr.scene()["rotations"][glr.BEST["rotation"]], glr.BEST["cell"], inputs["mean"], glr.S0)
    print(T[:3, 3], 2 * np.pi * glr.BEST["rotation"] / glr.YAW_STEPS)
    assert np.abs(T[:3, 3] - glr.SENSOR).max() < glr.S0
    assert abs(2 * np.pi * glr.BEST["rotation"] / glr.YAW_STEPS - glr.YAW) < 2 * np.pi / glr.YAW_STEPS
    assert np.allclose(T[:3, 3], (0.417, 0.751, 1.467), atol=5e-4)


@pytest.mark.parametrize("key", [k for k in glr.COUNTS if k[0] != 1])
def test_nodes_scored_and_launches(inputs, key):
    levels, batch = key
    got = glr.search(inputs["pyr"], inputs["rd"], A_MIN, A_MAX, levels, batch)
    print(key, got)
    assert (got["score"], got["rotation"], got["cell"], got["points"]) == (glr.BEST["score"], glr.BEST["rotation"], glr.BEST["cell"], glr.BEST["points"])
    assert (got["nodes_scored"], got["launches"]) == glr.COUNTS[key]
    assert got["levels"] == (levels or 6)


def test_min_score_ratio_and_max_nodes(inputs):
    pyr, rd = inputs["pyr"], inputs["rd"]
    none = glr.search(pyr, rd, A_MIN, A_MAX, 4, 64, min_score_ratio=1.0)
    assert glr.need_of(1.0, 1428) == 1428 and (none["found"], none["proven"], none["nodes_scored"]) == (0, 1, 3648)
    some = glr.search(pyr, rd, A_MIN, A_MAX, 4, 64, min_score_ratio=0.7)
    assert glr.need_of(0.7, 1428) == 1000 and (some["found"], some["score"], some["cell"], some["nodes_scored"]) == (1, 1424, (1, 1, 0), 3656)
    cut = glr.search(pyr, rd, A_MIN, A_MAX, 4, 1, max_nodes=100)
    assert (cut["found"], cut["proven"], cut["launches"], cut["nodes_scored"]) == (0, 0, 1, 64 * 2 * 6 * 2)


# ------------------------------------------------------------------------------------------------------------------ yaw_rotations
@pytest.mark.parametrize("args", [(64, 0.0, 0.0), (360, 0.0, 0.0), (7, 0.05, -0.1), (1, 0.3, 0.2)])
def test_yaw_rotations_python_cpp_and_reference(args):
    import host_global_localize_bindings as hg
    from norlab_icp_mapper_amd import icp
    a, b, c = icp.yaw_rotations(*args), hg.yaw_rotations(*args), glr.yaw_rotations(*args)
    assert a.dtype == np.float32 and a.shape == (args[0], 3, 3)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    for R in a.astype(np.float64):
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
    yaw = np.arctan2(a[:, 1, 0].astype(np.float64), a[:, 0, 0].astype(np.float64)) % (2 * np.pi)
    if args[1] == 0.0 and args[2] == 0.0:
        assert np.allclose(yaw, 2 * np.pi * np.arange(args[0]) / args[0], atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ refusals without a device
def test_refusals_that_need_no_device():
    import host_global_localize_bindings as hg
    from norlab_icp_mapper_amd import _capi, icp
    with pytest.raises(icp.InvalidParameter, match="yaw_rotations: steps must be >= 1"):
        icp.yaw_rotations(0)
    with pytest.raises(RuntimeError, match="yawRotations: steps must be >= 1"):
        hg.yaw_rotations(0)
    lib = _capi.load()
    lib.icpmi_global_localize_options_default(None)                                   # (a null pointer is ignored)
    lib.icpmi_global_localize_shape(None, None, None)
    res, o = _capi.GlobalLocalizeResult(), _capi.GlobalLocalizeOptions()
    R = np.eye(3, dtype=np.float32).reshape(-1)
    x = np.zeros(4, np.float32)
    assert lib.icpmi_global_localize(None, x.ctypes.data, 1, R.ctypes.data, 1, C.byref(o), C.byref(res)) == _capi.ERR_INVALID_ARG
    assert lib.icpmi_global_localize_dev(None, None, 1, R.ctypes.data, 1, C.byref(o), C.byref(res)) == _capi.ERR_INVALID_ARG
    assert lib.icpmi_occupancy_score_nodes(None, x.ctypes.data, 1, R.ctypes.data, 1, 0.5, 1, None, 0, None) == _capi.ERR_INVALID_ARG
    assert lib.icpmi_get_occupancy_level(None, 0.5, 1, 0, 0, None, None) == _capi.ERR_INVALID_ARG
    assert lib.icpmi_get_occupancy_info(None, None, None, None, None, None) == _capi.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_global_localize", "icpmi_global_localize_dev", "icpmi_occupancy_score_nodes", "icpmi_get_occupancy_level", "icpmi_get_occupancy_info")
NEW_VOID = ("icpmi_global_localize_options_default", "icpmi_global_localize_shape")


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
    O, R = _capi.GlobalLocalizeOptions, _capi.GlobalLocalizeResult
    of = ["cell_size", "levels", "min_score_ratio", "batch", "max_nodes", "has_box", "box_lo", "box_hi", "reserved"]
    rf = ["found", "proven", "rotation", "cell", "score", "points", "T", "levels", "launches", "nodes_scored", "leaves_scored", "reserved"]
    exprs = ["sizeof(icpmi_global_localize_options)"] + ["offsetof(icpmi_global_localize_options, %s)" % f for f in of]
    exprs += ["sizeof(icpmi_global_localize_result)"] + ["offsetof(icpmi_global_localize_result, %s)" % f for f in rf]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icpmi.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n'
                   % (" ".join(["%zu"] * len(exprs)), ", ".join(exprs)))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(O)] + [getattr(O, f).offset for f in of] + [C.sizeof(R)] + [getattr(R, f).offset for f in rf]
    assert got == want
    assert got[0] == 112 and got[len(of) + 1] == 160


def test_options_default_and_shape_need_no_device():
    from norlab_icp_mapper_amd import _capi
    lib = _capi.load()
    o = _capi.GlobalLocalizeOptions()
    o.cell_size, o.levels, o.batch, o.has_box, o.max_nodes, o.reserved[3] = 9.0, 5, 1, 1, 77, 4
    lib.icpmi_global_localize_options_default(C.byref(o))
    assert (o.cell_size, o.levels, o.min_score_ratio, o.batch, o.max_nodes, o.has_box, list(o.reserved)) == (0.5, 0, 0.0, 64, 0, 0, [0] * 8)
    sl, tl, ln = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    lib.icpmi_global_localize_shape(C.byref(sl), C.byref(tl), C.byref(ln))
    assert (sl.value, tl.value, ln.value) == (1024, 16, glr.TOP_CHUNK) and sl.value % 256 == 0
