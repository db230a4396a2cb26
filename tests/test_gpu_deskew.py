"""Sweep deskewing on the device (icpmi_deskew / icpmi_deskew_dev, csrc/deskew.hip) and in the host shell (Mapper::deskew through
nim_test_deskew), against the float64 reference of tests/deskew_reference.py.

The bound: 4 x the largest |float32 restatement - float64| / (|x| + |p|) that tests/test_deskew_cpu.py measures over this file's sweep
(profiles/deskew_tolerance.json: 2.2e-7 = 1.9 float32 epsilons, so 8.9e-7).  The device runs the restatement's arithmetic; its sinf and
numpy's may differ by a few ulp on the same inputs and nothing else differs.  Measured on an MI355X: at most 1.8e-7 over the sweep, 2.1e-7 on
the bundled slice.  Everything that has an exact answer is compared bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import deskew_reference as dr

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# float32-exact stamps in seconds, for the tests that put a float32 point time exactly on a stamp
EDGE_STAMPS = np.array([0.0, 1.0 / 32, 1.0 / 16, 1.0 / 8])


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def icp(amd):
    return amd.ICPSequence()


@pytest.fixture(scope="module")
def hook():
    import deskew_bindings as db
    from test_host_cpp import _build_host
    _build_host()
    db.load()
    return db


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _rel(out, pts, out64, pnorm):
    err = np.linalg.norm(np.asarray(out, np.float64)[:, :3] - out64, axis=1)
    return float((err / (np.linalg.norm(pts[:, :3].astype(np.float64), axis=1) + pnorm)).max())


@pytest.mark.parametrize("K", dr.SWEEP_K)
@pytest.mark.parametrize("n", dr.SWEEP_N)
def test_sweep_against_float64(icp, n, K):
    c = dr.sweep_case(n, K)
    out, nout = icp.deskew(c["pts"], c["t"], c["stamps"], c["poses"], ref=c["ref"], normals=c["nrm"])
    rel = dr.rel_error(out, c)
    nerr = float(np.abs(nout.astype(np.float64) - c["n64"]).max())
    norm_drift = float(np.abs(np.linalg.norm(nout.astype(np.float64), axis=1) - np.linalg.norm(c["nrm"].astype(np.float64), axis=1)).max())
    print(f"n={n} K={K}: points {rel:.3e} normals {nerr:.3e} norm drift {norm_drift:.3e} (bound {dr.device_bound():.3e})")
    assert np.array_equal(out[:, 3], c["pts"][:, 3])
    assert rel <= dr.device_bound()
    assert nerr <= dr.device_bound() and norm_drift <= dr.device_bound()     # unit vectors: the bound is relative to 1


def test_identity_table_returns_the_input(icp):
    pts, nrm, t = dr.make_points(4099, 31)
    for K in (2, 7):
        stamps = np.linspace(dr.SPAN[0], dr.SPAN[1], K)
        poses = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (K, 1))
        out, nout = icp.deskew(pts, t, stamps, poses, ref=0.05, normals=nrm)
        assert np.array_equal(out, pts) and np.array_equal(nout, nrm)


def test_same_bits_twice_in_place_and_through_device_pointers(icp):
    import torch
    c = dr.sweep_case(4099, 11)
    kw = dict(ref=c["ref"])
    a, an = icp.deskew(c["pts"], c["t"], c["stamps"], c["poses"], normals=c["nrm"], **kw)
    b, bn = icp.deskew(c["pts"], c["t"], c["stamps"], c["poses"], normals=c["nrm"], **kw)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(an), _bits(bn))
    no_normals = icp.deskew(c["pts"], c["t"], c["stamps"], c["poses"], **kw)
    assert np.array_equal(_bits(a), _bits(no_normals))
    d_in, d_t, d_n = (torch.from_numpy(np.array(c[k])).cuda() for k in ("pts", "t", "nrm"))
    d_out, d_nout = torch.zeros_like(d_in), torch.zeros_like(d_n)
    torch.cuda.synchronize()
    icp.deskewDev(d_in.data_ptr(), c["n"], d_t.data_ptr(), c["stamps"], c["poses"], d_out_ptr=d_out.data_ptr(), d_normals_ptr=d_n.data_ptr(),
                  d_normals_out_ptr=d_nout.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), c["pts"]) and np.array_equal(d_n.cpu().numpy(), c["nrm"])          # out of place: inputs untouched
    assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(a)) and np.array_equal(_bits(d_nout.cpu().numpy()), _bits(an))
    icp.deskewDev(d_in.data_ptr(), c["n"], d_t.data_ptr(), c["stamps"], c["poses"], d_normals_ptr=d_n.data_ptr(), **kw)   # in place
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_in.cpu().numpy()), _bits(a)) and np.array_equal(_bits(d_n.cpu().numpy()), _bits(an))


def _edge_motion(seed=41):
    return dr.make_motion(len(EDGE_STAMPS), seed, stamps=EDGE_STAMPS)


def test_times_exactly_on_stamps(icp):
    stamps, poses = _edge_motion()
    pts, nrm, _ = dr.make_points(5, 42)
    t = np.array([stamps[0], stamps[1], stamps[2], stamps[3], 0.5 * (stamps[2] + stamps[3])], F)
    assert np.array_equal(t.astype(np.float64)[:4], stamps)
    out = icp.deskew(pts, t, stamps, poses, ref=float(stamps[1]), unit=1.0)      # extrapolate off: the first and the last stamp are inside
    out64, _, pn = dr.deskew64(pts, t, stamps, poses, ref=float(stamps[1]), unit=1.0)
    assert _rel(out, pts, out64, pn) <= dr.device_bound()
    # at ref the relative pose is the identity up to the table's float32 rounding: the point stays where it was
    assert np.abs(out[1, :3] - pts[1, :3]).max() <= 4 * dr.EPS32 * np.linalg.norm(pts[1, :3])


def test_rounding_of_point_times(icp):
    stamps, poses = _edge_motion()
    pts, _, _ = dr.make_points(6, 43)
    r = 1.0 / 64
    t = np.array([2.5 * r, 3.5 * r, 2.4 * r, 2.6 * r, 0.49 * r, 7.9 * r], F)     # two exact ties: to 2 r and to 4 r (even), not 3 r
    rounded = np.array([2 * r, 4 * r, 2 * r, 3 * r, 0.0, 8 * r], F)
    on = icp.deskew(pts, t, stamps, poses, ref=0.01, unit=1.0, round=r)
    by_hand = icp.deskew(pts, rounded, stamps, poses, ref=0.01, unit=1.0)
    off = icp.deskew(pts, t, stamps, poses, ref=0.01, unit=1.0)
    assert np.array_equal(_bits(on), _bits(by_hand))
    assert not np.array_equal(_bits(on), _bits(off))
    for out, rs in ((on, r), (off, 0.0)):
        out64, _, pn = dr.deskew64(pts, t, stamps, poses, ref=0.01, unit=1.0, round_s=rs)
        assert _rel(out, pts, out64, pn) <= dr.device_bound()


def test_extrapolation_nan_and_sizes(icp, amd):
    stamps, poses = _edge_motion()
    pts, nrm, _ = dr.make_points(300, 44)
    t = np.linspace(0.001, 0.124, 300).astype(F)
    late, early = t.copy(), t.copy()
    late[299] = 0.1251
    early[17] = -1e-4
    for bad in (late, early):
        with pytest.raises(amd.InvalidParameter):
            icp.deskew(pts, bad, stamps, poses, ref=0.01, unit=1.0)
        out = icp.deskew(pts, bad, stamps, poses, ref=0.01, unit=1.0, extrapolate=True)
        clamped = np.clip(bad, F(stamps[0]), F(stamps[-1]))
        assert np.array_equal(_bits(out), _bits(icp.deskew(pts, clamped, stamps, poses, ref=0.01, unit=1.0)))
        out64, _, pn = dr.deskew64(pts, bad, stamps, poses, ref=0.01, unit=1.0, extrapolate=True)
        assert _rel(out, pts, out64, pn) <= dr.device_bound()
    inf = t.copy(); inf[5] = np.inf                                # +inf is a time after the last stamp
    at_end = icp.deskew(pts[5:6], np.array([stamps[-1]], F), stamps, poses, ref=0.01, unit=1.0)
    assert np.array_equal(_bits(icp.deskew(pts, inf, stamps, poses, ref=0.01, unit=1.0, extrapolate=True)[5]), _bits(at_end[0]))
    with pytest.raises(amd.InvalidParameter):
        icp.deskew(pts, inf, stamps, poses, ref=0.01, unit=1.0)
    nan = t.copy(); nan[123] = np.nan
    for ex in (False, True):
        with pytest.raises(amd.InvalidParameter):
            icp.deskew(pts, nan, stamps, poses, ref=0.01, unit=1.0, extrapolate=ex)
    assert icp.deskew(pts, t, stamps, poses, ref=0.01, unit=1.0).shape == (300, 4)      # the handle is fine after a failed call
    # n == 0, and a size past 2^31 - 1 (refused before any pointer is touched)
    assert icp.deskew(np.zeros((0, 4), F), np.zeros(0, F), stamps, poses, ref=0.01, unit=1.0).shape == (0, 4)
    m, keep = icp._sweepMotion(stamps, poses, 0.01, 1.0, 0.0, False)
    buf = np.zeros(8, F)
    from norlab_icp_mapper_amd import _capi
    st = icp._lib.icpmi_deskew(icp._h, buf.ctypes.data, 2 ** 31, buf.ctypes.data, C.byref(m), buf.ctypes.data, None, None)
    assert st == _capi.ERR_UNSUPPORTED
    # argument errors of the handle variants: the motion's, a missing pointer, normals on one side only
    with pytest.raises(amd.InvalidParameter):
        icp.deskew(pts, t, stamps[::-1].copy(), poses, ref=0.01, unit=1.0)
    with pytest.raises(amd.InvalidParameter):
        icp.deskew(pts, t, stamps, poses, ref=0.2, unit=1.0)
    assert icp._lib.icpmi_deskew(icp._h, pts.ctypes.data, 300, t.ctypes.data, C.byref(m), None, None, None) == _capi.ERR_INVALID_ARG
    out = np.empty_like(pts)
    assert icp._lib.icpmi_deskew(icp._h, pts.ctypes.data, 300, t.ctypes.data, C.byref(m), out.ctypes.data, nrm.ctypes.data, None) == _capi.ERR_INVALID_ARG
    assert icp._lib.icpmi_deskew(icp._h, pts.ctypes.data, 300, t.ctypes.data, None, out.ctypes.data, None, None) == _capi.ERR_INVALID_ARG


def test_planar_handle(amd):
    planar = amd.ICPSequence(minimizer=1, is_2d=1)
    stamps, poses = dr.make_motion(11, 45, planar=True)
    assert (poses[:, 2] == 0).all() and (poses[:, 3] == 0).all() and (poses[:, 4] == 0).all()
    pts, nrm, t = dr.make_points(257, 46, planar=True)
    assert (pts[:, 2] == 0).all()
    nrm2 = nrm.copy(); nrm2[:, 2] = 0
    out, nout = planar.deskew(pts, t, stamps, poses, ref=0.03, normals=nrm2)
    assert (out[:, 2] == 0).all() and (nout[:, 2] == 0).all()
    out64, _, pn = dr.deskew64(pts, t, stamps, poses, ref=0.03)
    assert _rel(out, pts, out64, pn) <= dr.device_bound()
    for col, v in ((2, 1e-9), (3, 1e-9), (4, -1e-9)):
        tilted = poses.copy(); tilted[5, col] = v
        with pytest.raises(amd.InvalidParameter):
            planar.deskew(pts, t, stamps, tilted, ref=0.03)
    s3, p3 = dr.make_motion(11, 47)
    with pytest.raises(amd.InvalidParameter):
        planar.deskew(pts, t, s3, p3, ref=0.03)


def test_host_shell_deskew(icp, hook):
    c = dr.sweep_case(4099, 11)
    n = c["n"]
    rng = np.random.default_rng(48)
    od = rng.normal(size=(n, 3)).astype(F)
    inten = rng.uniform(0, 255, n).astype(F)
    stamp_ns = 1_690_309_709_000_000_000                       # the scan's stamp, on the clock of the motion's stamps
    # the motion relative to the stamp is the sweep case's relative to its ref: the output is expressed at the stamp
    pose_ns = stamp_ns + np.rint((c["stamps"] - c["ref"]) * 1e9).astype(np.int64)
    s_rel = (pose_ns - stamp_ns).astype(np.float64) * 1e-9
    t_ns = np.rint(c["t"].astype(np.float64) - c["ref"] * 1e9).astype(F)                                   # offsets from the stamp, float32
    want, wn = icp.deskew(c["pts"], t_ns, s_rel, c["poses"], ref=0.0, normals=c["nrm"])
    _, wod = icp.deskew(c["pts"], t_ns, s_rel, c["poses"], ref=0.0, normals=od)
    out64, _, pn = dr.deskew64(c["pts"], t_ns, s_rel, c["poses"], ref=0.0)
    assert _rel(want, c["pts"], out64, pn) <= dr.device_bound()
    desc = {"intensity": inten, "normals": c["nrm"], "t": t_ns, "observationDirections": od}
    out, got, _ = hook.deskew(icp._h.value, c["pts"], desc, pose_ns, c["poses"], stamp_ns=stamp_ns)
    assert np.array_equal(_bits(out), _bits(want))
    assert list(got) == list(desc)                                                  # nothing added, dropped or reordered
    assert np.array_equal(_bits(got["normals"]), _bits(wn)) and np.array_equal(_bits(got["observationDirections"]), _bits(wod))
    assert not np.array_equal(wod, od)
    assert np.array_equal(got["intensity"][:, 0], inten) and np.array_equal(got["t"][:, 0], t_ns)
    # the int64 `times` path: absolute nanoseconds minus the stamp
    times = stamp_ns + t_ns.astype(np.int64)
    desc2 = {"intensity": inten, "normals": c["nrm"]}
    out2, got2, times_out = hook.deskew(icp._h.value, c["pts"], desc2, pose_ns, c["poses"], stamp_ns=stamp_ns, times=times)
    assert np.array_equal(_bits(out2), _bits(want)) and np.array_equal(_bits(got2["normals"]), _bits(wn))
    assert np.array_equal(times_out, times) and np.array_equal(got2["intensity"][:, 0], inten)
    # a cloud without normals, the float descriptor under another name and in seconds
    out3, got3, _ = hook.deskew(icp._h.value, c["pts"], {"stamps": (t_ns.astype(np.float64) * 1e-9).astype(F)}, pose_ns, c["poses"], stamp_ns=stamp_ns,
                                time_field="stamps", time_unit=1.0)
    out64s, _, pns = dr.deskew64(c["pts"], (t_ns.astype(np.float64) * 1e-9).astype(F), s_rel, c["poses"], ref=0.0, unit=1.0)
    assert _rel(out3, c["pts"], out64s, pns) <= dr.device_bound() and list(got3) == ["stamps"]
    # missing field; a time outside the motion
    with pytest.raises(hook.InvalidField):
        hook.deskew(icp._h.value, c["pts"], desc2, pose_ns, c["poses"], stamp_ns=stamp_ns)
    with pytest.raises(hook.InvalidField):
        hook.deskew(icp._h.value, c["pts"], desc, pose_ns, c["poses"], stamp_ns=stamp_ns, time_field="time")
    with pytest.raises(RuntimeError, match="outside"):
        hook.deskew(icp._h.value, c["pts"], desc, pose_ns, c["poses"], stamp_ns=stamp_ns + 200_000_000)
    j = int(np.searchsorted(s_rel, 0.0, side="right")) - 1      # the two poses around the stamp alone: most points lie outside them
    with pytest.raises(RuntimeError, match="outside"):
        hook.deskew(icp._h.value, c["pts"], desc, pose_ns[j:j + 2], c["poses"][j:j + 2], stamp_ns=stamp_ns)
    clamped = hook.deskew(icp._h.value, c["pts"], desc, pose_ns[j:j + 2], c["poses"][j:j + 2], stamp_ns=stamp_ns, extrapolate=True)[0]
    assert np.isfinite(clamped).all()


def test_bundled_scan_slice(icp):
    """every 8th point of the first bundled scan with its real `t` row (nanoseconds, not time-ordered: the sensor interleaves its rings)
    under a synthetic motion"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "deskew_scan0_slice.npz"))
    xyz, t = g["xyz"], g["t"]
    assert xyz.shape == (5175, 3) and t.dtype == F and t.min() == 0 and 9.9e7 < t.max() < 1e8
    pts = np.ones((len(xyz), 4), F); pts[:, :3] = xyz
    stamps, poses = dr.make_motion(21, 49, max_rate=1.0, max_speed=2.0)      # the issue's robot: 2 m/s, 1 rad/s
    out = icp.deskew(pts, t, stamps, poses, ref=0.0)
    out64, _, pn = dr.deskew64(pts, t, stamps, poses, ref=0.0)
    rel = _rel(out, pts, out64, pn)
    moved = np.linalg.norm(out64 - xyz.astype(np.float64), axis=1)
    print(f"bundled slice: {rel:.3e} (bound {dr.device_bound():.3e}); points move by up to {moved.max():.2f} m")
    assert rel <= dr.device_bound()
    assert moved.max() > 0.5                                                 # the smear deskewing takes out is not small
    rounded = icp.deskew(pts, t, stamps, poses, ref=0.0, round=1e-6)
    out64r, _, pnr = dr.deskew64(pts, t, stamps, poses, ref=0.0, round_s=1e-6)
    assert _rel(rounded, pts, out64r, pnr) <= dr.device_bound()
