"""IntensityPointToPlaneErrorMinimizer without a GPU: the reference gradient on a plane with a linear field, what the registration tests on the
device lean on -- checked on the numpy loops alone --, the float32 restatement against the recorded tolerance, weight 0 as point-to-plane bit
for bit, the Python YAML front end, the header's new symbols and the pinned ABI."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import intensity_cases as ic
import intensity_reference as ir
import localizability_reference as lr
import plane_to_plane_reference as pp
import symmetric_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_scenes_carry_the_specified_field():
    for name in ic.SCENES:
        s = ir.scene(name)
        assert s["map"].shape == (8000, 4) and s["reading"].shape == (2000, 4) and s["map_intensity"].dtype == np.float32
        assert np.array_equal(s["map"], lr.scene(name)["map"]) and np.array_equal(s["reading"], lr.scene(name)["reading"])
        for cloud, key in (("map", "map_intensity"), ("reading", "reading_intensity")):
            noise = s[key].astype(np.float64) - ir.field(s[cloud][:, :3])
            assert abs(noise.std() - ir.NOISE_SIGMA) < 0.002 and abs(noise.mean()) < 0.002
    x = np.array([[0.3, 1.1, 2.0]])
    assert ir.field(x)[0] == pytest.approx(0.5 + 0.25 * np.sin(2 * np.pi * 1.1 / 2.5) + 0.15 * np.sin(2 * np.pi * 2.3 / 1.7))
    assert np.allclose(ir.START[:3, 3], (0.05, 0.3, -0.04)) and np.allclose(lr.step_from_T(ir.START)[:3], (0, 0, 0.03))


@pytest.mark.parametrize("label, m, K", [c for c in ic.PATCH_CASES if c[2] > 1], ids=[c[0] for c in ic.PATCH_CASES if c[2] > 1])
def test_gradient_of_a_linear_field_on_a_plane_is_its_tangential_part(label, m, K):
    cloud, normals, inten = ic.patch(m)
    nbr = ir.self_knn(cloud, K)
    assert (nbr[:, 0] == np.arange(m)).all()
    want = ic.PATCH_A - ic.PATCH_NORMAL * (ic.PATCH_A @ ic.PATCH_NORMAL)
    for fn in (ir.gradient_reference, ir.gradient_float32):
        g = fn(cloud, normals, inten, nbr)
        # (the float32 intensities carry the field to 6e-8 of its size over neighbour spacings of a few centimetres and more)
        assert np.abs(g - want[None, :]).max() <= 1e-4, fn.__name__
        assert np.abs(g @ ic.PATCH_NORMAL).max() <= 1e-6


def test_gradient_is_withheld_where_the_specification_says():
    cloud, normals, inten = ic.patch(40)
    nbr = ir.self_knn(cloud, 10)
    for fn in (ir.gradient_reference, ir.gradient_float32):
        assert (fn(cloud, normals, inten, ir.self_knn(cloud, 1)) == 0).all()               # one neighbour: a line
        assert (fn(np.repeat(cloud[:1], 40, 0), normals, inten, nbr) == 0).all()            # neighbours on the point itself
        n2, i2 = normals.copy(), inten.copy()
        n2[3], n2[4, 0], i2[5] = 0.0, np.nan, np.nan
        g = fn(cloud, n2, i2, nbr)
        assert (g[[3, 4, 5]] == 0).all() and (g[6:] != 0).any(1).all()
        few = nbr.copy()
        few[:, 2:] = -1                                                                     # fewer than two usable neighbours
        assert (fn(cloud, normals, inten, few) == 0).all()


@pytest.mark.parametrize("name", ic.SCENES)
def test_weight_zero_is_point_to_plane_bit_for_bit(name):
    """the reference's sums at weight 0 ARE localizability_reference.pair_sums' point-to-plane sums"""
    T = ir.centred_pose(ir.START, ir.centred(name)[2])
    pairs = ir.scene_pairs(name, T, k=3, max_dist=ic.MAX_DIST, cauchy=1.0)
    got = ir.reference_sums(weight=0.0, **pairs)
    A, b, W = lr.pair_sums(pairs["p"], pairs["q"], pairs["n"], pairs["w"])
    want = lr.pack_sums(A, b, W, int((pairs["w"] != 0).sum()))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(ir.reference_sums(weight=ic.WEIGHT, **pairs).view(np.uint64), want.view(np.uint64))
    # ... and the float32 restatement's ARE those of the float32 point-to-plane restatement the project has: symmetric_reference.float32_sums
    # without a surface model on the reading side, which is point-to-plane with the unit map normal -- the scenes' map normals are exact
    # axis-aligned unit vectors, so scaling them to length 1 returns them
    assert np.array_equal(pp.unit_or_zero(pairs["n"]), pairs["n"])
    want32 = sr.float32_sums(pairs["p"], pairs["q"], pairs["n"], np.zeros_like(pairs["n"]), pairs["w"])
    assert np.array_equal(ir.float32_sums(weight=0.0, **pairs).view(np.uint64), want32.view(np.uint64))
    nan = dict(pairs, Ip=np.full_like(pairs["Ip"], np.nan))
    assert np.array_equal(ir.float32_sums(weight=0.0, **nan).view(np.uint64), want32.view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ the loops
def test_the_term_recovers_the_corridor_axis_and_point_to_plane_cannot():
    """corridor, float64, from 0.3 m off along the axis: below 1e-2 m within 8 iterations; the point-to-plane twin (the minimum-norm step of
    its rank-5 system) stays above 0.25 m after 30"""
    poses = ir.register("corridor", ic.WEIGHT, 64, ic.CORRIDOR_ITERATIONS)
    along = [abs(ir.residual_pose(T)[ir.AXIS, 3]) for T in poses]
    twin = ir.register("corridor", 0.0, 64, ic.TWIN_ITERATIONS)
    along_twin = abs(ir.residual_pose(twin[-1])[ir.AXIS, 3])
    print("along the axis per iteration:", ["%.2e" % a for a in along], "twin after 30: %.4f" % along_twin)
    assert along[-1] < ic.ALONG_AXIS_BOUND and min(along) == pytest.approx(along[-1], abs=1e-3)
    assert along_twin > ic.TWIN_STAYS_ABOVE
    A = lr.unpack_sums(ir.reference_sums(weight=ic.WEIGHT, **ir.scene_pairs("corridor", ir.centred_pose(np.eye(4), ir.centred("corridor")[2]), k=1, trimmed=ir.TRIMMED)))[0]
    A0 = lr.unpack_sums(ir.reference_sums(weight=0.0, **ir.scene_pairs("corridor", ir.centred_pose(np.eye(4), ir.centred("corridor")[2]), k=1, trimmed=ir.TRIMMED)))[0]
    lam, lam0 = np.linalg.eigvalsh(A), np.linalg.eigvalsh(A0)
    print("smallest eigenvalue of A at the true pose: %.3f with the term, %.3e without" % (lam[0], lam0[0]))
    assert lam[0] > 1.0 and abs(lam0[0]) < 1e-9 * lam0[-1]


def test_both_loops_settle_in_the_room():
    """room: both loops converge (the Differential checker stops them) and the term's pose is no worse than the record.  Point-to-plane
    settles 0.28 m off along y from this start: TrimmedDist 0.85 drops the end walls, whose pairs are the farthest"""
    rec = ic.recorded()["loops"]["room"]
    p64 = ir.register("room", ic.WEIGHT, 64, ic.ROOM_ITERATIONS)
    twin = ir.register("room", 0.0, 64, ic.TWIN_ITERATIONS)
    stop, stop_twin = sr.differential_stop(p64, **sr.DIFFERENTIAL), sr.differential_stop(twin, **sr.DIFFERENTIAL)
    assert stop is not None and stop_twin is not None
    dt, dr = sr.pose_error(p64[-1], np.linalg.inv(ir.START))
    print(f"room: stop at {stop} (twin {stop_twin}), {dt:.3e} m / {dr:.3e} rad; twin {sr.pose_error(twin[-1], np.linalg.inv(ir.START))}")
    assert dt <= rec["float32_translation_error"] * (1 + 1e-6) and dr <= rec["float32_rotation_error"] * (1 + 1e-6)
    assert dt < 2e-3


def test_float32_restatement_stays_within_the_recorded_distance():
    """where the tolerance of the GPU tests is measured (scripts/intensity_tolerance.py wrote the record from the same function)"""
    spec = importlib.util.spec_from_file_location("intensity_tolerance", os.path.join(ROOT, "scripts", "intensity_tolerance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got, rec = mod.measure(), ic.recorded()
    print({k: v for k, v in got.items() if k != "loops"})
    for key, val in got["max_rel_gradient"].items():
        assert val <= rec["max_rel_gradient"][key] * (1 + 1e-9), key
        assert rec["max_rel_gradient"][key] < 1e-5      # (a 2 x 2 inverse whose determinant is kept away from zero)
    for name in ic.SCENES:
        assert got["max_rel_sums"][name] <= rec["max_rel_sums"][name] * (1 + 1e-9), name
        assert rec["max_rel_sums"][name] < 1e-6
    assert got["max_rel_step_room"] <= rec["max_rel_step_room"] * (1 + 1e-9)
    for name in ("corridor", "room"):
        for key in ("float32_from_float64_translation", "float32_translation_error", "float32_rotation_error"):
            assert got["loops"][name][key] <= rec["loops"][name][key] * (1 + 1e-9), (name, key)
        assert got["loops"][name]["twin_axis_errors"][ir.AXIS] > ic.TWIN_STAYS_ABOVE


# ------------------------------------------------------------------------------------------------------------------ YAML (Python front end)
NAME = "IntensityPointToPlaneErrorMinimizer"


def _cfg(minimizer, **chain):
    from norlab_icp_mapper_amd import icp
    return icp.config_from_yaml_chain(dict(errorMinimizer=minimizer, **chain))


def test_python_yaml():
    from norlab_icp_mapper_amd import _capi, icp
    c = _cfg(NAME)
    assert c.minimizer == _capi.MIN_POINT_TO_PLANE == 2 and c.force_4dof == 0 and c.force_2d == 0 and c.covariance == 0 and c.degeneracy_threshold == 0.0
    assert c.intensity_weight == pytest.approx(0.032) and c.intensity_knn == 10 and c.intensity_desc_name == "intensity"
    c = _cfg({NAME: {"lambdaGeometric": 0.9, "descName": "reflectivity", "gradientKnn": 6, "force4DOF": 1}})
    assert c.minimizer == 2 and c.force_4dof == 1 and c.intensity_weight == pytest.approx(0.1) and c.intensity_knn == 6 and c.intensity_desc_name == "reflectivity"
    assert _cfg({NAME: {"lambdaGeometric": 1.0}}).intensity_weight == 0.0
    for bad in ({"force2D": 1}, {"degeneracyThreshold": 0.01}, {"sensorStdDev": 0.01}, {"epsilon": 0.1}, {"lambdaGeometrics": 0.9}):
        with pytest.raises(icp.InvalidParameter, match=NAME + ": unknown parameter"):
            _cfg({NAME: bad})
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(icp.InvalidParameter, match="lambdaGeometric"):
            _cfg({NAME: {"lambdaGeometric": bad}})
    for bad in (0, 32, 2.5):
        with pytest.raises(icp.InvalidParameter, match="gradientKnn"):
            _cfg({NAME: {"gradientKnn": bad}})
    assert not hasattr(_cfg("PointToPlaneErrorMinimizer"), "intensity_weight")
    with pytest.raises(icp.InvalidParameter, match="intensity weight"):
        icp.ICPSequence(minimizer=2, intensity_weight=1.0)        # (checked before the handle is created)


# ------------------------------------------------------------------------------------------------------------------ the C++ shell
def parse_error_minimizer_intensity(entry):
    """nim_test_parse_error_minimizer_intensity (host/TestHooks.cpp) on the chain `errorMinimizer: <entry>`: dict of what parseErrorMinimizer
    set, or RuntimeError with the exception's text"""
    lines = entry.rstrip("\n").split("\n")
    yaml_icp = ("errorMinimizer: " + lines[0] + "\n") if len(lines) == 1 and not lines[0].endswith(":") else \
        "errorMinimizer:\n" + "".join("  " + ln + "\n" for ln in lines)
    import host_bindings as hb
    fn = hb.load().nim_test_parse_error_minimizer_intensity
    fn.restype = C.c_int
    mini, f4, knn = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    weight = C.c_float(-1)
    name, err = C.create_string_buffer(64), C.create_string_buffer(512)
    if fn(yaml_icp.encode(), C.byref(mini), C.byref(f4), C.byref(weight), C.byref(knn), name, C.c_int(64), err, C.c_int(512)):
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(minimizer=mini.value, force_4dof=f4.value, weight=weight.value, knn=knn.value, desc_name=name.value.decode())


def test_cpp_yaml():
    F = np.float32
    assert parse_error_minimizer_intensity(NAME) == dict(minimizer=2, force_4dof=0, weight=F(1) - F(0.968), knn=10, desc_name="intensity")
    got = parse_error_minimizer_intensity(NAME + ":\n  lambdaGeometric: 0.9\n  descName: reflectivity\n  gradientKnn: 6\n  force4DOF: 1\n")
    assert got == dict(minimizer=2, force_4dof=1, weight=F(1) - F(0.9), knn=6, desc_name="reflectivity")
    for bad in ("force2D: 1", "degeneracyThreshold: 0.01", "sensorStdDev: 0.01", "epsilon: 0.1", "lambdaGeometrics: 0.9"):
        with pytest.raises(RuntimeError, match=NAME + ": unknown parameter"):
            parse_error_minimizer_intensity(NAME + ":\n  %s\n" % bad)
    for bad in ("lambdaGeometric: 0", "lambdaGeometric: 1.5", "lambdaGeometric: -0.1"):
        with pytest.raises(RuntimeError, match="lambdaGeometric"):
            parse_error_minimizer_intensity(NAME + ":\n  %s\n" % bad)
    for bad in ("gradientKnn: 0", "gradientKnn: 32"):
        with pytest.raises(RuntimeError, match="gradientKnn"):
            parse_error_minimizer_intensity(NAME + ":\n  %s\n" % bad)
    # the others leave the term off
    assert parse_error_minimizer_intensity("PointToPlaneErrorMinimizer") == dict(minimizer=2, force_4dof=0, weight=0.0, knn=10, desc_name="")
    assert parse_error_minimizer_intensity("PlaneToPlaneErrorMinimizer")["weight"] == 0.0


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_set_intensity_weight", "icpmi_get_intensity_weight", "icpmi_set_map_intensity", "icpmi_set_reading_intensity",
               "icpmi_intensity_gradient")


def test_header_and_library_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported, sym
        assert sym in bound, sym
    assert "Park, Zhou, Koltun" in header and "Not libpointmatcher's" in header


def test_config_size_and_version_are_unchanged(tmp_path):
    from norlab_icp_mapper_amd import _capi
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include "icpmi.h"\nint main(void) { printf("%zu %d\\n", sizeof(icpmi_config), (int)ICPMI_VERSION); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.Config), 4]
    assert got[0] == 5 * 4 + 8 * 20 + 15 * 4 + 8 * 4
