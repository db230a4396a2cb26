"""Sweep registration without a device: the float64 reference (tests/sweep_reference.py) on the `room` case, icpmi_sweep_solve (host only)
against numpy, the float32 restatement's distance from float64 (recorded in profiles/sweep_tolerance.json), and the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import localizability_reference as lr
import sweep_cases as sc
import sweep_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def icp_mod():
    from norlab_icp_mapper_amd import icp
    return icp


@pytest.fixture(scope="module")
def room_systems():
    """the reference's systems on the `room` case: the sums of the first iterations from "off" (exact neighbours, the case's chain)"""
    c = sc.room()
    out = []
    mu = c["mean"].astype(np.float64)
    Tb = Te = sc.STARTS["off"]
    from scipy.spatial import cKDTree
    mp64, nm64 = c["map"][:, :3].astype(np.float64), c["normals"].astype(np.float64)
    tree = cKDTree(mp64)
    for _ in range(3):
        P = sr.world_points(c["scan"], c["alpha"], Tb, Te)
        q, n, w = sr.match(tree, mp64, nm64, P, sc.MAX_DIST, sc.TRIM_RATIO)
        s, _ = sr.sums64(P - mu, q - mu, n, w, c["alpha"])
        out.append(s)
        x = sr.solve(s)
        Tb, Te = sr.apply_step(Tb, x[:6], mu), sr.apply_step(Te, x[6:], mu)
    return out


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_sums_by_hand():
    """one pair: p = (1, 2, 3), q = (1, 2, 2.5), n = (0, 0, 1), w = 2, alpha = 0.25"""
    s, gs = sr.sums64([[1, 2, 3]], [[1, 2, 2.5]], [[0, 0, 1]], [2.0], [0.25])
    u = sr.unpack(s)
    Fv = np.array([2.0, -1.0, 0.0, 0.0, 0.0, 1.0])          # [p x n ; n]
    assert np.allclose(u["M0"], 2 * np.outer(Fv, Fv)) and np.allclose(u["M1"], 0.25 * u["M0"]) and np.allclose(u["M2"], 0.0625 * u["M0"])
    assert np.allclose(u["g0"], 2 * Fv * 0.5) and np.allclose(u["g1"], 0.25 * u["g0"])
    assert (u["W"], u["pairs"], u["wr2"]) == (2.0, 1.0, 0.5)
    assert s[78] == s[79] == 0 and np.allclose(gs, np.abs(Fv))


def test_reference_normal_equations_minimise_the_cost():
    """the 12 x 12 system is the gradient of sum w (r + F . ((1 - a) xi_b + a xi_e))^2: checked by finite differences on random pairs"""
    rng = np.random.default_rng(5)
    p, q, n = rng.normal(size=(40, 3)), rng.normal(size=(40, 3)), rng.normal(size=(40, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    w, a = rng.random(40), rng.random(40).astype(F)
    s, _ = sr.sums64(p, q, n, w, a)
    Fm = np.concatenate([np.cross(p, n), n], 1)
    r = ((p - q) * n).sum(1)

    def cost(x):
        return (w * (r + (Fm * ((1 - a)[:, None] * x[:6] + a[:, None] * x[6:])).sum(1)) ** 2).sum()
    x = sr.solve(s)
    for i in range(12):
        e = np.zeros(12); e[i] = 1e-6
        assert abs(cost(x + e) - cost(x - e)) / 2e-6 < 1e-6 * cost(np.zeros(12))
    assert cost(x) < cost(np.zeros(12))


def test_room_convergence():
    """the case of the introduction: two poses estimated from "off" bring the mean point error to at most a tenth of rigid point-to-plane's"""
    c = sc.room()
    mu = c["mean"].astype(np.float64)
    start = sc.STARTS["off"]
    Tb, Te, its, norms = sr.register_sweep(c["map"], c["normals"], c["scan"], c["alpha"], start, start, mu, sc.MAX_DIST, sc.TRIM_RATIO, sc.ITERATIONS)
    sweep_mean, sweep_max = sr.point_error(sr.world_points(c["scan"], c["alpha"], Tb, Te), c["truth"])
    T = sr.register_rigid(c["map"], c["normals"], c["scan"], start, mu, sc.MAX_DIST, sc.TRIM_RATIO, sc.ITERATIONS)
    x3 = c["scan"][:, :3].astype(np.float64)
    rigid_mean, rigid_max = sr.point_error(x3 @ T[:3, :3].T + T[:3, 3], c["truth"])
    A, _ = sr.system(sr.sums64(c["truth"] - mu, c["truth"] - mu, lr.scene("room")["reading_normals"], np.ones(x3.shape[0]), c["alpha"])[0])
    print("sweep", sweep_mean, sweep_max, "rigid", rigid_mean, rigid_max, "last step", norms[-1], "cond", np.linalg.cond(A))
    assert its == sc.ITERATIONS
    assert sweep_mean <= 0.1 * rigid_mean
    assert max(norms[-1]) < 1e-9                              # converged well inside the iteration count
    assert np.linalg.cond(A) < 1e4                            # observable without a prior


# ------------------------------------------------------------------------------------------------------------------ icpmi_sweep_solve
def test_solve_against_numpy(icp_mod, room_systems):
    for s in room_systems:
        for lam_r, lam_t, d in ((0.0, 0.0, None), (0.5, 2.0, None), (10.0, 10.0, np.array([1e-3, -2e-3, 5e-4, 0.01, -0.02, 0.005]))):
            want = sr.solve(s, lam_r, lam_t, d)
            got = icp_mod.sweep_solve(s, lam_r, lam_t, d)
            assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (lam_r, lam_t)


def test_stiff_prior_gives_the_rigid_step(icp_mod, room_systems):
    for s in room_systems:
        u = sr.unpack(s)
        rigid = np.linalg.solve(u["M0"], -u["g0"])
        x = icp_mod.sweep_solve(s, 1e9, 1e9)
        assert np.abs(x[:6] - rigid).max() <= 1e-6 * np.abs(rigid).max()
        assert np.abs(x[6:] - rigid).max() <= 1e-6 * np.abs(rigid).max()


def test_solve_rejections(icp_mod):
    cor = lr.scene("corridor")
    p = cor["reading"][:, :3].astype(np.float64)
    alpha = np.linspace(0, 1, p.shape[0]).astype(F)
    s, _ = sr.sums64(p, p + 0.01 * cor["reading_normals"], cor["reading_normals"], np.ones(p.shape[0]), alpha)
    with pytest.raises(icp_mod.ConvergenceError, match="not observable"):
        icp_mod.sweep_solve(s)                                 # nothing constrains the translation along the corridor
    with pytest.raises(icp_mod.ConvergenceError, match="not observable"):
        icp_mod.sweep_solve(s, 1.0, 1.0)                       # a prior on the RELATIVE motion does not fix the common one
    with pytest.raises(icp_mod.ConvergenceError, match="no point to minimize"):
        icp_mod.sweep_solve(np.zeros(80))
    good, _ = sr.sums64(*(lambda c: (c["truth"], c["truth"] + 0.01, lr.scene("room")["reading_normals"], np.ones(c["truth"].shape[0]), c["alpha"]))(sc.room()))
    assert np.isfinite(icp_mod.sweep_solve(good)).all()
    for lam in ((-1.0, 0.0), (0.0, -1.0), (np.inf, 0.0), (0.0, np.nan)):
        with pytest.raises(icp_mod.InvalidParameter):
            icp_mod.sweep_solve(good, *lam)
    with pytest.raises(icp_mod.InvalidParameter):
        icp_mod.sweep_solve(np.zeros(79))
    with pytest.raises(icp_mod.InvalidParameter):
        icp_mod.sweep_solve(good, d=np.zeros(5))


# ------------------------------------------------------------------------------------------------------------------ the tolerance
def test_float32_formulation_tolerance():
    """the float32 restatement (deskew, centring, xf_point, F and r in float32) against float64 on every sums case, exact neighbours;
    written to profiles/sweep_tolerance.json.  The GPU tests allow four times the figure."""
    worst = sc.measure_tolerance()
    sc.record(sums_float32=worst, sums_what="max over the sums cases (tests/sweep_cases.py: SUM_CASES) of sweep_reference.deviation(float32 "
              "restatement, float64) with exact neighbours; measured on CPU (numpy float32 / float64)", float32_eps=float(np.finfo(F).eps))
    print("sweep sums float32 vs float64:", worst)
    assert 0 < worst < 1e-3


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_register_sweep", "icpmi_register_sweep_dev", "icpmi_sweep_sums", "icpmi_sweep_solve")
OPT_FIELDS = ("begin_s", "end_s", "time_unit_s", "max_iterations", "min_step_rot", "min_step_trans", "lambda_rot", "lambda_trans", "reserved")
RES_FIELDS = ("T_begin", "T_end", "pose7", "iterations", "stop_reason", "pairs", "weight_sum", "sum_sq", "weighted_point_used_ratio", "trimmed_limit",
              "reserved")


def test_header_library_and_ctypes_agree_on_the_new_symbols(icp_mod):
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name: args for name, _, args in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported and sym in bound, sym
    assert "icpmi_sweep_options_default" in exported and "icpmi_sweep_options_default" in bound
    assert len(bound["icpmi_register_sweep"]) == len(bound["icpmi_register_sweep_dev"]) == len(bound["icpmi_sweep_sums"]) == 9
    assert len(bound["icpmi_sweep_solve"]) == 5
    for name in ("register_sweep", "register_sweep_dev", "sweep_sums", "sweep_solve"):
        assert callable(getattr(icp_mod.ICPSequence, name))


def test_struct_layouts_and_defaults(tmp_path):
    from norlab_icp_mapper_amd import _capi
    src = tmp_path / "sw.c"
    offs = ", ".join(["offsetof(icpmi_sweep_options, %s)" % f for f in OPT_FIELDS] + ["offsetof(icpmi_sweep_result, %s)" % f for f in RES_FIELDS])
    nf = len(OPT_FIELDS) + len(RES_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icpmi.h"\nint main(void) { printf("%zu %zu %zu %zu' + " %zu" * nf +
                   '\\n", sizeof(icpmi_sweep_options), sizeof(icpmi_sweep_result), sizeof(icpmi_config), sizeof(icpmi_stats), ' + offs + "); return 0; }\n")
    exe = tmp_path / "sw"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_capi.SweepOptions) == 88
    assert got[1] == C.sizeof(_capi.SweepResult) == 312
    assert got[2] == C.sizeof(_capi.Config) and got[3] == C.sizeof(_capi.Stats) == 72        # as before the feature
    assert got[4:4 + len(OPT_FIELDS)] == [getattr(_capi.SweepOptions, f).offset for f in OPT_FIELDS]
    assert got[4 + len(OPT_FIELDS):] == [getattr(_capi.SweepResult, f).offset for f in RES_FIELDS]
    o = _capi.SweepOptions()
    _capi.load().icpmi_sweep_options_default(C.byref(o))
    assert (o.begin_s, o.end_s, o.time_unit_s, o.max_iterations, o.min_step_rot, o.min_step_trans, o.lambda_rot, o.lambda_trans) == \
        (0.0, 0.1, 1e-9, 12, -1.0, -1.0, 0.0, 0.0)
    assert list(o.reserved) == [0] * 8
