"""The float64 restatement of the degeneracy-aware point-to-plane solve (tests/localizability_reference.py) against hand-derived answers
on the five analytic scenes, the C ABI's layout, and the YAML keys of the Python front end.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import localizability_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, Z = np.eye(3)


def solve(name, four_dof=False, origin=(0.0, 0.0, 0.0), threshold=lr.THRESHOLD):
    A, b, W, c, L = lr.exact_system(name, origin)
    return lr.localizability_reference(A, b, W, c, L, threshold, four_dof), (A, b, W, c, L)


@pytest.mark.parametrize("four_dof", [False, True])
@pytest.mark.parametrize("name", lr.SCENES)
def test_threshold_has_a_factor_five_on_each_side(name, four_dof):
    r, _ = solve(name, four_dof)
    deg, inf = r["mu"][r["degenerate"]], r["mu"][~r["degenerate"]]
    assert (deg < 1e-13).all(), deg
    assert (deg * 5 <= lr.THRESHOLD).all() and (inf >= 5 * lr.THRESHOLD).all(), r["mu"]


@pytest.mark.parametrize("name", lr.SCENES)
def test_counts(name):
    assert solve(name)[0]["n_degenerate"] == lr.N_DEGENERATE[name]
    r4 = solve(name, True)[0]
    assert r4["n"] == 4 and r4["n_degenerate"] == lr.N_DEGENERATE_4DOF[name]
    assert not r4["V"][:2].any()          # roll and pitch are not in the 4-DOF system


def in_span(v, V, tol=1e-9):
    v = v / np.linalg.norm(v)
    return np.linalg.norm(v - V @ (V.T @ v)) <= tol


def null_vectors(name, c, L):
    """the hand-derived degenerate twists in the pivoted, scaled coordinates (omega L, t + omega x c)"""
    tw = lambda om, t: np.concatenate([np.asarray(om, float) * L, np.asarray(t, float) + np.cross(om, c)])
    if name == "room":
        return []
    if name == "corridor":
        return [tw(0 * X, Y)]                                  # translation along the corridor
    if name in ("floor_ceiling", "floor"):
        return [tw(0 * X, X), tw(0 * X, Y), tw(Z, 0 * X)]       # x, y and yaw (about any vertical axis: the span holds them all)
    a = lr.TUNNEL_AXIS_POINT                                   # rotation about the cylinder's axis: omega = y, t = -omega x a
    return [tw(0 * X, Y), tw(Y, -np.cross(Y, a))]


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (40.0, -30.0, 5.0)])
@pytest.mark.parametrize("name", lr.SCENES)
def test_null_vectors(name, origin):
    r, (A, b, W, c, L) = solve(name, origin=origin)
    Vd = r["V"][:, r["degenerate"]]
    if name == "tunnel":   # (the axis moves with the origin)
        a = lr.TUNNEL_AXIS_POINT - np.asarray(origin)
        want = [np.concatenate([0 * X, Y]), np.concatenate([Y * L, -np.cross(Y, a) + np.cross(Y, c)])]
    else:
        want = null_vectors(name, c, L)
    assert Vd.shape[1] == len(want)
    for v in want:
        assert in_span(v, Vd, 1e-7), (name, v)


@pytest.mark.parametrize("four_dof", [False, True])
@pytest.mark.parametrize("name", lr.SCENES)
def test_origin_independence(name, four_dof):
    r0, _ = solve(name, four_dof)
    r1, _ = solve(name, four_dof, origin=(40.0, -30.0, 5.0))
    np.testing.assert_allclose(r1["mu"], r0["mu"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(r1["P_kept"], r0["P_kept"], rtol=0, atol=1e-8)   # same directions: the coordinates are pivoted


@pytest.mark.parametrize("name", lr.SCENES)
def test_four_dof_is_the_sub_system(name):
    """the {2, 3, 4, 5} sub-system of the pivoted, scaled matrix is the pivoted, scaled {2, 3, 4, 5} sub-system (K mixes rows 2..5 only
    among themselves when omega = (0, 0, wz)): the 4-DOF spectrum equals that of the system built from yaw + translation features alone"""
    sc = lr.scene(name)
    p, nn = sc["reading"][:, :3].astype(np.float64), sc["reading_normals"].astype(np.float64)
    c, L = lr.reading_stats(p)
    F4 = np.concatenate([np.cross(p - c, nn)[:, 2:3] / L, nn], 1)
    lam = np.linalg.eigvalsh(F4.T @ F4)
    r = solve(name, True)[0]
    np.testing.assert_allclose(r["lam"], lam, rtol=0, atol=1e-9 * lam.max())


@pytest.mark.parametrize("four_dof", [False, True])
def test_below_every_mu_it_is_the_plain_solve(four_dof):
    """room, a misaligned reading (b != 0): with a threshold under every mu the constrained step is numpy.linalg.solve(A, b)"""
    sc = lr.scene("room")
    q, nn = sc["reading"][:, :3].astype(np.float64), sc["reading_normals"].astype(np.float64)
    T = lr.make_T((0.01, -0.02, 0.03), (0.05, -0.1, 0.02))
    p = q @ T[:3, :3].T + T[:3, 3]
    A, b, W = lr.pair_sums(p, q, nn)
    c0, L = lr.reading_stats(q)
    r = lr.localizability_reference(A, b, W, lr.pivot(T, c0), L, 1e-6, four_dof)
    assert r["n_degenerate"] == 0
    sel = np.arange(2, 6) if four_dof else np.arange(6)
    x = np.zeros(6)
    x[sel] = np.linalg.solve(A[np.ix_(sel, sel)], b[sel])
    np.testing.assert_allclose(r["x"], x, rtol=0, atol=1e-10 * np.abs(x).max())
    # ... and with the working threshold on the corridor the step has no component along the corridor
    sc = lr.scene("corridor")
    q, nn = sc["reading"][:, :3].astype(np.float64), sc["reading_normals"].astype(np.float64)
    p = q @ T[:3, :3].T + T[:3, 3]
    A, b, W = lr.pair_sums(p, q, nn)
    c0, L = lr.reading_stats(q)
    c = lr.pivot(T, c0)
    r = lr.localizability_reference(A, b, W, c, L, lr.THRESHOLD, four_dof)
    assert r["n_degenerate"] == 1
    v = r["V"][:, r["degenerate"]][:, 0]
    assert abs(v @ lr.scaled_step(r["x"], c, L)) <= 1e-12 * np.linalg.norm(r["y"])


def test_step_round_trip():
    x = np.array([0.01, -0.02, 0.03, 0.3, -0.1, 0.2])
    np.testing.assert_allclose(lr.step_from_T(lr.make_T(x[:3], x[3:])), x, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_library_and_binding_agree():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    assert re.search(r"icpmi_status\s+icpmi_get_localizability\s*\(", header)
    assert "icpmi_get_localizability" in exported
    assert "icpmi_get_localizability" in {name for name, _, _ in _capi.SYMBOLS}


def test_config_keeps_its_size_and_the_field_is_the_last_reserved_word(tmp_path):
    from norlab_icp_mapper_amd import _capi
    assert _capi.Config.degeneracy_threshold.offset == _capi.Config.reserved.offset + 4 == C.sizeof(_capi.Config) - 4
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icpmi.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(icpmi_config), '
                   'offsetof(icpmi_config, degeneracy_threshold), offsetof(icpmi_config, reserved), sizeof(icpmi_localizability), '
                   'offsetof(icpmi_localizability, pivot)); return 0; }\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.Config), _capi.Config.degeneracy_threshold.offset, _capi.Config.reserved.offset,
                   C.sizeof(_capi.Localizability), _capi.Localizability.pivot.offset]
    assert got[0] == 5 * 4 + 8 * 20 + 15 * 4 + 8 * 4      # as before the field existed
    cfg = _capi.Config()
    _capi.load().icpmi_config_default(C.byref(cfg))
    assert cfg.degeneracy_threshold == 0.0 and list(cfg.reserved) == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ YAML (Python front end)
def _cfg(minimizer):
    from norlab_icp_mapper_amd import icp
    return icp.config_from_yaml_chain({"errorMinimizer": minimizer})


def test_yaml_keys():
    from norlab_icp_mapper_amd import icp
    assert _cfg({"PointToPlaneErrorMinimizer": {}}).degeneracy_threshold == 0.0
    assert _cfg({"PointToPlaneErrorMinimizer": {"degeneracyThreshold": 0.005}}).degeneracy_threshold == np.float32(0.005)
    assert _cfg({"PointToPlaneErrorMinimizer": {"degeneracyThreshold": 0.005, "degeneracyAction": "report"}}).degeneracy_threshold == -np.float32(0.005)
    c = _cfg({"PointToPlaneWithCovErrorMinimizer": {"degeneracyThreshold": 0.01, "force4DOF": 1}})
    assert c.degeneracy_threshold == np.float32(0.01) and c.covariance == 1 and c.force_4dof == 1
    for name in ("PointToPlaneErrorMinimizer", "PointToPlaneWithCovErrorMinimizer"):   # a misspelt key is an error, not an option left off
        for typo in ({"degeneracyTreshold": 0.01}, {"degeneracyThreshold": 0.01, "degeneracyaction": "report"}):
            with pytest.raises(icp.InvalidParameter, match="unknown parameter"):
                _cfg({name: typo})
    assert _cfg({"PointToPlaneErrorMinimizer": {"force4DOF": 1}}).force_4dof == 1
    for bad in ({"degeneracyThreshold": -1.0}, {"degeneracyThreshold": 0.01, "degeneracyAction": "ignore"}, {"degeneracyThreshold": 0.01, "force2D": 1}):
        with pytest.raises(icp.InvalidParameter):
            _cfg({"PointToPlaneErrorMinimizer": bad})
