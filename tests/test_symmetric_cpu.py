"""SymmetricPointToPlaneErrorMinimizer without a GPU: the float32 restatement against the recorded tolerance, the properties of the pair model
(sign invariance bit for bit, agreement with point-to-plane), what the registration tests on the device lean on -- checked on the numpy loops
alone --, the YAML front ends, the header's new symbols and the pinned ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import localizability_reference as lr
import plane_to_plane_reference as pp
import symmetric_cases as sc
import symmetric_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = sc.STARTS["off"]
TRUTH = np.linalg.inv(OFF)


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_ellipsoid_scene_is_the_specified_one():
    s = sr.scene("ellipsoid")
    assert s["map"].shape == (8000, 4) and s["reading"].shape == (2000, 4) and s["map"].dtype == np.float32
    rng = np.random.default_rng(7)
    v = rng.normal(size=(8000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    assert np.array_equal(s["map"][:, :3], (v * (4, 10, 1.5)).astype(np.float32))
    for pts, nrm in ((s["map"], s["normals"]), (s["reading"], s["reading_normals"])):
        x = pts[:, :3].astype(np.float64)
        np.testing.assert_allclose(((x / sr.ELLIPSOID_AXES) ** 2).sum(1), 1.0, atol=1e-6)
        np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
        assert ((x * nrm).sum(1) < 0).all()      # inward
        g = -x / np.square(sr.ELLIPSOID_AXES)
        np.testing.assert_allclose(nrm, g / np.linalg.norm(g, axis=1, keepdims=True), atol=1e-6)


def test_float32_restatement_stays_within_the_recorded_distance():
    """where the tolerance of the GPU tests is measured (scripts/symmetric_tolerance.py wrote the record from the same function)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("symmetric_tolerance", os.path.join(ROOT, "scripts", "symmetric_tolerance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got, rec = mod.measure(), sc.recorded()
    print(got)
    for name in sc.SCENES:
        assert got["max_rel_sums"][name] <= rec["max_rel_sums"][name] * (1 + 1e-9), name
        assert rec["max_rel_sums"][name] < 1e-6     # (a few float32 roundings per pair, no ill-conditioned inverse)
    assert got["max_rel_step_room"] <= rec["max_rel_step_room"] * (1 + 1e-9)
    for name in ("ellipsoid", "room"):
        for key in ("float32_translation_error", "float32_rotation_error"):
            assert got["loops"][name][key] <= rec["loops"][name][key] * (1 + 1e-9), (name, key)


def _pairs_with_random_signs(name, seed):
    pairs = sr.scene_pairs(name, OFF, k=3, max_dist=sc.MAX_DIST, cauchy=1.0)
    rng = np.random.default_rng(seed)
    flip = lambda n: np.where(rng.random(n.shape[0])[:, None] < 0.5, -n, n)
    return pairs, flip


@pytest.mark.parametrize("name", sc.SCENES)
def test_sign_invariance_of_the_restatement_is_bit_exact(name):
    """negating n_x negates c and u_p together; negating n_q negates n_s, F and the residual together: the same bits in all 32 sums"""
    pairs, flip = _pairs_with_random_signs(name, 11)
    base = sr.float32_sums(**pairs)
    for side in ("nq", "npr"):
        other = dict(pairs)
        other[side] = flip(pairs[side])
        assert (other[side] != pairs[side]).any()
        assert np.array_equal(sr.float32_sums(**other).view(np.uint64), base.view(np.uint64)), side
    ref = sr.reference_sums(**pairs)
    both = dict(pairs, nq=flip(pairs["nq"]), npr=flip(pairs["npr"]))
    np.testing.assert_allclose(sr.reference_sums(**both), ref, rtol=0, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("name", sc.SCENES)
def test_equal_normals_are_point_to_plane(name):
    """u_q = u_p (either sign), and no surface model on the reading side: localizability_reference.pair_sums with the unit map normal"""
    pairs = sr.scene_pairs(name, OFF, k=1, max_dist=sc.MAX_DIST, trimmed=0.85)
    A, b, W = lr.pair_sums(pairs["p"], pairs["q"], pp.unit_or_zero(pairs["nq"].astype(np.float64)), pairs["w"])
    ref = lr.pack_sums(A, b, W, int((pairs["w"] != 0).sum()))
    scale = np.abs(ref[:27]).max()
    for npr in (pairs["nq"], -pairs["nq"], 3.0 * pairs["nq"].astype(np.float64), np.zeros_like(pairs["nq"]), np.full_like(pairs["nq"], np.nan)):
        got = sr.reference_sums(pairs["p"], pairs["q"], pairs["nq"], npr, pairs["w"])
        np.testing.assert_allclose(got[:27], ref[:27], rtol=0, atol=1e-12 * scale)
        assert got[27] == ref[27] and got[28] == ref[28]
    # the float32 restatement in the limit: the kernel's point-to-plane arithmetic on the unit normal, bit for bit
    f32 = sr.float32_sums(pairs["p"], pairs["q"], pairs["nq"], np.zeros_like(pairs["nq"]), pairs["w"])
    same = sr.float32_sums(pairs["p"], pairs["q"], pairs["nq"], pp.unit_or_zero(pairs["nq"]), pairs["w"])
    assert pp.rel_distance(f32, ref) < 1e-6 and pp.rel_distance(same, f32) < 1e-6


def test_zero_normals_and_the_quarter_weight():
    nq = np.array([[0, 0, 2], [0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1]], np.float64)
    npr = np.array([[0, 0, 0], [0, 3, 0], [0, 0, 0], [1, 0, 0], [0.6, 0, 0.8]], np.float64)
    ns = sr.pair_normals(nq, npr)
    np.testing.assert_allclose(ns[0], [0, 0, 1])          # no model on the reading side: u_q
    np.testing.assert_allclose(ns[1], [0, 1, 0])          # ... on the map side: u_p
    assert (ns[2] == 0).all()                             # on neither: the pair only counts
    assert (ns[3] == 0).all()                             # perpendicular: c = 0
    np.testing.assert_allclose(ns[4], 0.5 * 0.8 * (np.array([0, 0, 1]) + [0.6, 0, 0.8]))      # continuous: |n_s| = c cos(theta / 2)
    p = np.array([[1.0, 2.0, 3.0]] * 5)
    sums = sr.reference_sums(p, p + 0.1, nq, npr)
    assert sums[27] == 5 and sums[28] == 5
    only_both_zero = sr.reference_sums(p[2:3], p[2:3] + 0.1, nq[2:3], npr[2:3])
    assert (only_both_zero[:27] == 0).all() and only_both_zero[27] == 1 and only_both_zero[28] == 1
    # normals at 45 degrees to each other: n_s = cos(45) (u_q + u_p) / 2, |n_s|^2 = cos^2(45) cos^2(22.5)
    d = np.array([[np.sin(np.pi / 4), 0, np.cos(np.pi / 4)]])
    assert np.linalg.norm(sr.pair_normals(nq[3:4], d)) ** 2 == pytest.approx(np.cos(np.pi / 4) ** 2 * np.cos(np.pi / 8) ** 2)


# ------------------------------------------------------------------------------------------------------------------ the loops
def test_ellipsoid_symmetric_ends_twenty_times_closer_than_point_to_plane():
    """the condition tests/test_gpu_symmetric.py leans on, on the float64 reference alone"""
    sym = sr.register("ellipsoid", OFF, "symmetric", 64, sc.ELLIPSOID_ITERATIONS)
    p2p = sr.register("ellipsoid", OFF, "point_to_plane", 64, sc.ELLIPSOID_ITERATIONS)
    es, ep = sr.pose_error(sym[-1], TRUTH), sr.pose_error(p2p[-1], TRUTH)
    print(f"ellipsoid after {sc.ELLIPSOID_ITERATIONS} iterations: symmetric {es[0]:.2e} m / {es[1]:.2e} rad, point-to-plane {ep[0]:.2e} m / {ep[1]:.2e} rad")
    assert 20 * es[0] <= ep[0]
    assert sr.pose_error(sym[2], TRUTH)[0] <= 1.5 * es[0]          # reached in three iterations


def test_room_symmetric_does_not_cycle():
    poses = sr.register("room", OFF, "symmetric", 64, sc.ROOM_ITERATIONS)
    assert np.abs(poses[9] - poses[11]).max() <= 1e-9             # iteration 10 against iteration 12
    assert np.abs(poses[10] - poses[11]).max() <= 1e-9
    dt, dr = sr.pose_error(poses[-1], TRUTH)
    print(f"room: {dt:.2e} m / {dr:.2e} rad")
    assert dt < 1e-6 and dr < 1e-6


# ------------------------------------------------------------------------------------------------------------------ YAML (Python front end)
def _cfg(minimizer, **chain):
    from norlab_icp_mapper_amd import icp
    return icp.config_from_yaml_chain(dict(errorMinimizer=minimizer, **chain))


def test_python_yaml():
    from norlab_icp_mapper_amd import _capi, icp
    c = _cfg("SymmetricPointToPlaneErrorMinimizer")
    assert c.minimizer == _capi.MIN_PLANE_TO_PLANE == 3 and c.force_4dof == 0 and c.plane_model == "symmetric"
    assert c.force_2d == 0 and c.covariance == 0 and c.degeneracy_threshold == 0.0 and not hasattr(c, "plane_epsilon")
    c = _cfg({"SymmetricPointToPlaneErrorMinimizer": {"force4DOF": 1}})
    assert c.minimizer == 3 and c.force_4dof == 1 and c.plane_model == "symmetric"
    for bad in ({"epsilon": 0.01}, {"force2D": 1}, {"degeneracyThreshold": 0.01}, {"sensorStdDev": 0.01}, {"force4DOFF": 1}):
        with pytest.raises(icp.InvalidParameter, match="SymmetricPointToPlaneErrorMinimizer: unknown parameter"):
            _cfg({"SymmetricPointToPlaneErrorMinimizer": bad})
    assert not hasattr(_cfg("PlaneToPlaneErrorMinimizer"), "plane_model")
    assert not hasattr(_cfg("PointToPlaneErrorMinimizer"), "plane_model")
    assert (_capi.PLANE_MODEL_GICP, _capi.PLANE_MODEL_SYMMETRIC) == (0, 1)
    with pytest.raises(icp.InvalidParameter, match="plane_model"):
        icp.ICPSequence(minimizer=3, plane_model="symetric")      # (checked before the handle is created)


# ------------------------------------------------------------------------------------------------------------------ the C++ shell
def parse_error_minimizer_model(entry):
    """nim_test_parse_error_minimizer_model (host/TestHooks.cpp) on the chain `errorMinimizer: <entry>`: dict of what parseErrorMinimizer set,
    or RuntimeError with the exception's text"""
    lines = entry.rstrip("\n").split("\n")
    yaml_icp = ("errorMinimizer: " + lines[0] + "\n") if len(lines) == 1 and not lines[0].endswith(":") else \
        "errorMinimizer:\n" + "".join("  " + ln + "\n" for ln in lines)
    import host_bindings as hb
    fn = hb.load().nim_test_parse_error_minimizer_model
    fn.restype = C.c_int
    mini, f4, model = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    eps = C.c_float(-1)
    err = C.create_string_buffer(512)
    if fn(yaml_icp.encode(), C.byref(mini), C.byref(f4), C.byref(eps), C.byref(model), err, C.c_int(512)):
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(minimizer=mini.value, force_4dof=f4.value, epsilon=eps.value, model=model.value)


def test_cpp_yaml():
    assert parse_error_minimizer_model("SymmetricPointToPlaneErrorMinimizer") == dict(minimizer=3, force_4dof=0, epsilon=np.float32(1e-3), model=1)
    assert parse_error_minimizer_model("SymmetricPointToPlaneErrorMinimizer:\n  force4DOF: 1\n") == dict(minimizer=3, force_4dof=1, epsilon=np.float32(1e-3), model=1)
    for bad in ("epsilon: 0.01", "force2D: 1", "degeneracyThreshold: 0.01", "sensorStdDev: 0.01"):
        with pytest.raises(RuntimeError, match="SymmetricPointToPlaneErrorMinimizer: unknown parameter"):
            parse_error_minimizer_model("SymmetricPointToPlaneErrorMinimizer:\n  %s\n" % bad)
    # the others leave the model alone
    assert parse_error_minimizer_model("PlaneToPlaneErrorMinimizer:\n  epsilon: 0.01\n") == dict(minimizer=3, force_4dof=0, epsilon=np.float32(0.01), model=0)
    assert parse_error_minimizer_model("PointToPlaneErrorMinimizer")["model"] == 0
    with pytest.raises(RuntimeError, match="unknown error minimizer"):
        parse_error_minimizer_model("SymmetricErrorMinimizer")


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_set_plane_pair_model", "icpmi_get_plane_pair_model")


def test_header_and_library_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported, sym
        assert sym in bound, sym
    assert re.search(r"ICPMI_PLANE_MODEL_GICP\s*=\s*0\b", header) and re.search(r"ICPMI_PLANE_MODEL_SYMMETRIC\s*=\s*1\b", header)
    assert "Rusinkiewicz" in header


def test_config_size_and_version_are_unchanged(tmp_path):
    from norlab_icp_mapper_amd import _capi
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include "icpmi.h"\nint main(void) { printf("%zu %d %d %d\\n", sizeof(icpmi_config), (int)ICPMI_VERSION, '
                   '(int)ICPMI_PLANE_MODEL_GICP, (int)ICPMI_PLANE_MODEL_SYMMETRIC); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.Config), 4, 0, 1]
    assert got[0] == 5 * 4 + 8 * 20 + 15 * 4 + 8 * 4
