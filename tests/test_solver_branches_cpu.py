"""The case table of tests/solver_cases.py on the CPU: every case reaches the branch it is meant for (margins established from the
data), the ORACLE's single step meets the universal properties and the float64 reference (tests/solver_reference.py) inside the
bounds the device is held to (tests/test_gpu_solver_branches.py runs the same check_step on the device's output), and the route
the oracle took is confirmed through its own entry points.  test_table_report prints one line per case -- branch margin, kappa,
error / (eps_f kappa) -- and pins the constant K of solver_cases to 4 x the worst of them (run with -s to read the table)."""
import numpy as np
import pytest

import solver_cases as sc
import solver_reference as sr
from solver_oracle import oracle_step

CASES = sc.cases_by_name()


_figs = {}


def figures(oracle, name):
    if name not in _figs:
        T, sums, mc, rc, x = oracle_step(oracle, CASES[name])
        _figs[name] = (sr.check_step(CASES[name], T, sums, mc, rc, sc, "oracle"), T, sums, x)
    return _figs[name]


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_step_against_float64(oracle, name):
    case = CASES[name]
    fig, T, sums, x = figures(oracle, name)
    ref = fig["ref"]
    print("\n" + sr.line(fig))
    if case["kw"]["minimizer"] == 1 and not case["kw"].get("is_2d"):
        # the route, through the oracle itself: the SVD route's own entry point returns the same bits where rotation_from_H took it
        H32 = ref["H32"]
        same = np.array_equal(oracle.rotation_from_H(H32), oracle.rotation_from_H(H32, svd=True))
        if case["route"] in ("svd", "reflect"):
            assert same, name
        if case["route"] == "newton":
            assert not same, name
    if case["kw"]["minimizer"] == 2:
        # ... and the solver's: solve_n on the reference's float32 system returns the step's x; the minimum-norm route leaves exact zeros
        # where Cholesky would have divided by a zero pivot
        xs = oracle.solve_n(ref["A32"].astype(np.float32), ref["b32"].astype(np.float32))
        assert np.array_equal(xs, x[ref["idx"]]), (name, xs, x)
        if case["route"] == "minnorm":
            assert all(x[i] == 0.0 for i in case["null"]), (name, x)
    if name == "p2l_big_step":
        assert np.linalg.norm(ref["x"][:3]) >= 0.5 and np.linalg.norm(x[:3]) >= 0.5 and ref["kappa"] < 1e4, (name, ref["x"])
    if name == "p2l_below_big_step":
        assert 0.45 <= np.linalg.norm(ref["x"][:3]) < 0.5 and np.linalg.norm(x[:3]) < 0.5 and ref["kappa"] < 1e4, (name, ref["x"])


def test_threshold_sweep_is_continuous(oracle):
    """every step of the sweep against the same float64 SVD (check_step above), d from 1e-9 to 1e-3 in >= 12 steps across the switch,
    and neighbouring steps within the sum of their bounds of each other: no jump where the route changes"""
    figs = [figures(oracle, n) for n in sc.SWEEP_NAMES]
    d = np.array([f[0]["ref"]["d"] for f in figs])
    assert len(d) >= 12 and d[0] < 2e-9 and d[-1] > 5e-4 and np.all(np.diff(d[2:]) > 0), d   # (the first two sit on float32's floor of d)
    assert (d < 1e-6).sum() >= 4 and (d > 1e-6).sum() >= 4
    for (fa, Ta, _, _), (fb, Tb, _, _) in zip(figs[:-1], figs[1:]):
        dt, dr = sr.pose_error(Ta, Tb)
        assert dt <= fa["bound"][0] + fb["bound"][0] and dr <= fa["bound"][1] + fb["bound"][1], (fa["name"], dt, dr)


def test_table_report(oracle):
    """the table: per case the branch margin, kappa and the oracle's error / (eps_f kappa); K = 4 x the worst"""
    worst, who = 0.0, None
    print()
    for name in sc.NAMES:
        fig = figures(oracle, name)[0]
        print(sr.line(fig))
        if "ratio" in fig and fig["ratio"] > worst:
            worst, who = fig["ratio"], name
    print(f"worst error / (eps_f kappa) = {worst:.3f} ({who}); K_MEASURED = {sc.K_MEASURED}, K = {sc.K}")
    assert worst <= sc.K_MEASURED <= 1.1 * worst + 0.05, (worst, who, sc.K_MEASURED)
    routes = {CASES[n]["route"] for n in sc.NAMES}
    assert {"newton", "svd", "reflect", "planar", "chol", "minnorm", "zero", "either"} <= routes
