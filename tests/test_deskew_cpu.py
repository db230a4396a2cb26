"""Sweep deskewing without a GPU: the float64 reference against a known answer, icpmi_deskew_table (host code of libicpmi.so, no device
call) against the float64 preparation, and the float32 formulation's own distance from float64 -- the figure the GPU test's bound is
made of (profiles/deskew_tolerance.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import deskew_reference as dr
from norlab_icp_mapper_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float64_reference_known_answer():
    """constant rotation rate about a fixed axis and constant velocity: slerp and lerp are exact between the samples, so static world
    points W seen at times tau come back as R(ref)^T (W - p(ref))"""
    rng = np.random.default_rng(7)
    axis = np.array([0.3, -0.5, 0.8]); axis /= np.linalg.norm(axis)
    rate, v, p0 = 2.5, np.array([11.0, -4.0, 0.5]), np.array([100.0, 50.0, 2.0])
    R0 = Rotation.from_rotvec([0.2, 0.1, -0.4])
    pose = lambda s: (R0 * Rotation.from_rotvec(np.outer(np.atleast_1d(s) * rate, axis)), p0 + np.outer(np.atleast_1d(s), v))
    stamps = np.array([-0.01, 0.013, 0.05, 0.081, 0.11])
    Rk, pk = pose(stamps)
    poses = np.concatenate([pk, Rk.as_quat()], axis=1)
    n, ref = 500, 0.0625
    W = rng.uniform(-60, 60, (n, 3))
    tau = np.sort(rng.uniform(0.0, 0.1, n))
    Rt, pt = pose(tau)
    x = Rt.inv().apply(W - pt)                      # what the moving sensor measures
    pts = np.ones((n, 4)); pts[:, :3] = x
    # (deskew64 takes float32 clouds and float32 times like the library: feed it values that are float32 already)
    pts = pts.astype(np.float32); t = (tau * 1e9).astype(np.float32)
    tau32 = t.astype(np.float64) * 1e-9
    Rt, pt = pose(tau32)
    W32 = Rt.apply(pts[:, :3].astype(np.float64)) + pt
    Rr, pr = pose(ref)
    want = Rr.inv().apply(W32 - pr)
    got, _, _ = dr.deskew64(pts, t, stamps, poses, ref=ref)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def _lib_table(stamps, poses, ref, n_poses=None):
    lib = _capi.load()
    s = np.ascontiguousarray(stamps, np.float64); p = np.ascontiguousarray(poses, np.float64)
    K = len(s) if n_poses is None else n_poses
    m = _capi.SweepMotion(n_poses=K, extrapolate=0, stamp_s=s.ctypes.data_as(C.POINTER(C.c_double)),
                          pose7=p.ctypes.data_as(C.POINTER(C.c_double)), ref_s=ref, time_unit_s=1e-9, round_s=0.0)
    q, t = np.full((len(s), 4), np.nan, np.float32), np.full((len(s), 3), np.nan, np.float32)
    om, isn = np.full(len(s) - 1, np.nan, np.float32), np.full(len(s) - 1, np.nan, np.float32)
    st = lib.icpmi_deskew_table(C.byref(m), q.ctypes.data, t.ctypes.data, om.ctypes.data, isn.ctypes.data)
    return st, (q, t, om, isn)


def _assert_table(stamps, poses, ref):
    """every entry within one float32 rounding of the float64 preparation.  Two float64 computations of the same quantity differ by a
    few 1e-16 of the magnitudes they are made of (1 for a quaternion, the metres moved for a translation), which may push the
    float32 rounding to the neighbouring value: one spacing, plus that float64 noise for the entries that are (near) zero.  The
    reference's T(ref) comes from scipy, so the table as a whole may come with the opposite sign: q and -q are the same rotations."""
    st, (q, p, om, isn) = _lib_table(stamps, poses, ref)
    assert st == _capi.ICPMI_OK, _capi.load().icpmi_last_error(None).decode()
    q64, p64, om64, isn64 = dr.prepare64(stamps, poses, ref)
    if np.dot(q64[0], q[0].astype(np.float64)) < 0:
        q64 = -q64
    scale_p = max(1.0, np.abs(np.asarray(poses)[:, :3] - np.asarray(poses)[0, :3]).max())

    def close(got, want, noise):
        want32 = want.astype(np.float32)
        tol = np.spacing(np.abs(want32)).astype(np.float64) + noise
        assert (np.abs(got.astype(np.float64) - want) <= tol).all(), (np.abs(got - want).max(), tol.min())
    close(q, q64, 1e-14)
    close(p, p64, 1e-14 * scale_p)
    # Omega comes from |q_{k+1} - q_k|, a difference of numbers of size 1: absolute float64 noise of a few 1e-16, carried into 1 / sin
    close(om, om64, 1e-14)
    assert ((isn == 0) == (isn64 == 0)).all()
    close(isn, isn64, 1e-14 * np.maximum(1.0, isn64 ** 2))
    return q, p, om, isn


def test_table_k2():
    stamps, poses = dr.make_motion(2, 11)
    _assert_table(stamps, poses, 0.03)
    _assert_table(stamps, poses, stamps[0])


@pytest.mark.parametrize("where", ["on_a_stamp", "between", "last"])
def test_table_k3(where):
    stamps, poses = dr.make_motion(3, 12)
    ref = {"on_a_stamp": stamps[1], "between": 0.5 * (stamps[1] + stamps[2]) + 0.003, "last": stamps[2]}[where]
    q, p, om, isn = _assert_table(stamps, poses, float(ref))
    if where != "between":  # the pose at ref is the identity of the relative table
        k = 1 if where == "on_a_stamp" else 2
        assert np.abs(np.abs(q[k]) - [0, 0, 0, 1]).max() <= 1e-7 and np.abs(p[k]).max() <= 1e-6


def test_table_alternating_signs():
    """a caller's table that alternates q and -q describes the same motion: the same table, the quaternions sign-continued"""
    stamps, poses = dr.make_motion(11, 13, flip_signs=False)
    flipped = poses.copy()
    flipped[1::2, 3:] *= -1.0
    a = _assert_table(stamps, poses, 0.04)
    b = _assert_table(stamps, flipped, 0.04)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) or np.array_equal(x, -y)
    q = a[0].astype(np.float64)
    assert ((q[1:] * q[:-1]).sum(axis=1) > 0).all()


def test_table_identical_consecutive_poses():
    stamps, poses = dr.make_motion(5, 14)
    poses[2] = poses[1]
    poses[3, 3:] = -poses[1, 3:]           # the same rotation with the other sign
    q, p, om, isn = _assert_table(stamps, poses, 0.02)
    assert isn[1] == 0 and om[1] == 0 and isn[2] == 0 and isn[0] != 0 and isn[3] != 0
    assert np.array_equal(q[1], q[2]) and np.array_equal(q[2], q[3])


def test_table_k1024():
    stamps, poses = dr.make_motion(1024, 15)
    q, p, om, isn = _assert_table(stamps, poses, 0.07)
    assert (isn != 0).all()


def test_table_rejections():
    lib = _capi.load()
    stamps, poses = dr.make_motion(4, 16)

    def status(s=stamps, p=poses, ref=0.02, unit=1e-9, rnd=0.0, n_poses=None, null=None):
        s = np.ascontiguousarray(s, np.float64); p = np.ascontiguousarray(p, np.float64)
        m = _capi.SweepMotion(n_poses=len(s) if n_poses is None else n_poses, extrapolate=0,
                              stamp_s=None if null == "stamps" else s.ctypes.data_as(C.POINTER(C.c_double)),
                              pose7=None if null == "poses" else p.ctypes.data_as(C.POINTER(C.c_double)), ref_s=ref, time_unit_s=unit, round_s=rnd)
        out = [np.zeros(4 * 1025, np.float32) for _ in range(4)]
        ptr = [None if null == "out%d" % i else o.ctypes.data for i, o in enumerate(out)]
        st = lib.icpmi_deskew_table(None if null == "motion" else C.byref(m), *ptr)
        if st != _capi.ICPMI_OK:
            assert len(lib.icpmi_last_error(None).decode()) > 10     # ... and a message
        return st
    assert status() == _capi.ICPMI_OK
    bad = _capi.ERR_INVALID_ARG
    for null in ("motion", "stamps", "poses", "out0", "out1", "out2", "out3"):
        assert status(null=null) == bad, null
    assert status(n_poses=1) == bad and status(n_poses=0) == bad and status(n_poses=-3) == bad
    big_s, big_p = dr.make_motion(1025, 17)
    assert status(s=big_s, p=big_p) == bad                          # n_poses = 1025
    assert status(s=big_s[:1024], p=big_p[:1024]) == _capi.ICPMI_OK
    s2 = stamps.copy(); s2[2] = s2[1]
    assert status(s=s2) == bad                                      # not strictly increasing
    s2 = stamps.copy(); s2[1], s2[2] = stamps[2], stamps[1]
    assert status(s=s2) == bad
    for v in (np.nan, np.inf):
        s2 = stamps.copy(); s2[3] = v
        assert status(s=s2) == bad
        for col in (0, 5):
            p2 = poses.copy(); p2[1, col] = v
            assert status(p=p2) == bad
    p2 = poses.copy(); p2[2, 3:] *= 1.002
    assert status(p=p2) == bad                                      # | |q| - 1 | > 1e-3
    p2 = poses.copy(); p2[2, 3:] *= 1.0005
    assert status(p=p2) == _capi.ICPMI_OK
    p2 = poses.copy(); p2[0, 3:] = 0
    assert status(p=p2) == bad
    assert status(ref=stamps[0] - 1e-6) == bad and status(ref=stamps[-1] + 1e-6) == bad and status(ref=np.nan) == bad
    assert status(ref=stamps[0]) == _capi.ICPMI_OK and status(ref=stamps[-1]) == _capi.ICPMI_OK
    for unit in (0.0, -1e-9, np.nan, np.inf):
        assert status(unit=unit) == bad
    for rnd in (-1e-6, np.nan, np.inf):
        assert status(rnd=rnd) == bad
    assert status(rnd=1e-6) == _capi.ICPMI_OK


def test_float32_formulation_tolerance():
    """the float32 restatement against float64 over the GPU test's inputs: written to profiles/deskew_tolerance.json; above 16 float32
    epsilons the formulation would be at fault, not the rounding.  The device's bound is 4 x this figure."""
    worst = dr.measured_tolerance()
    path = os.path.join(ROOT, "profiles", "deskew_tolerance.json")
    doc = {"what": "max |float32 restatement - float64| / (|x| + |p|) over tests/deskew_reference.py's sweep "
                   "(n in %s, K in %s; ranges 0.5 - 120 m, up to 3 rad/s and 30 m/s)" % (list(dr.SWEEP_N), list(dr.SWEEP_K)),
           "measured": worst, "float32_eps": dr.EPS32, "measured_in_eps": worst / dr.EPS32, "device_bound": dr.device_bound(),
           "measured_on": "CPU (numpy float32); the device figure is in profiles/deskew_bench.json when it has been run"}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("deskew float32 vs float64:", worst, "=", worst / dr.EPS32, "eps")
    assert 0 < worst < 16 * dr.EPS32


def test_float32_restatement_edges():
    """the restatement at the places the kernel branches: times on the first, an inner and the last stamp, a lerp segment, clamping"""
    stamps, poses = dr.make_motion(5, 18)
    stamps = stamps.astype(np.float32).astype(np.float64)            # a float32 time can then sit exactly on a stamp
    poses[3] = poses[2]
    pts, nrm, _ = dr.make_points(6, 19)
    t = np.array([stamps[0], stamps[2], stamps[4], 0.5 * (stamps[2] + stamps[3]), -1.0, 1.0], np.float64)
    tab = dr.table32(stamps, poses, 0.01)
    out32, n32, bad = dr.deskew32(pts, t, stamps, tab, unit=1.0, extrapolate=True, normals=nrm)
    out64, n64, pn = dr.deskew64(pts, t, stamps, poses, ref=0.01, unit=1.0, extrapolate=True, normals=nrm)
    assert not bad.any()
    rel = np.linalg.norm(out32[:, :3] - out64, axis=1) / (np.linalg.norm(pts[:, :3], axis=1) + pn)
    assert rel.max() < 16 * dr.EPS32 and np.abs(n32 - n64).max() < 16 * dr.EPS32
    _, _, bad = dr.deskew32(pts, t, stamps, tab, unit=1.0, extrapolate=False)
    assert bad.tolist() == [False, False, False, False, True, True]
