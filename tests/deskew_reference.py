"""Two independent restatements of sweep deskewing (include/icpmi.h: icpmi_deskew_table / icpmi_deskew), and the inputs the tests share.

* float64: scipy's Slerp for the rotation and np.interp for the translation give T(tau); a point x measured at tau goes to
  T(ref)^-1 T(tau) x.  Nothing of the library's formulation is in it (no relative table, no sign continuation, no Omega).
* float32: the header's arithmetic line by line on numpy float32 arrays, reading a table that `prepare64` built in float64 (scipy for
  T(ref) and the composition) and rounded to float32.  numpy does not contract a product into a sum, so it differs from the device
  by the two sinf calls alone.
"""
import functools

import numpy as np
from scipy.spatial.transform import Rotation, Slerp

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
LERP_BELOW = 2.0 ** -20


# ---- time: the same fp64 operations as the kernel -----------------------------------------------------------------------------
def point_times(t_rel, stamps, unit, round_s=0.0, extrapolate=False):
    """tau (float64) of every point, and a mask of the points the call fails on (NaN, or out of span without extrapolate)"""
    s = np.asarray(stamps, np.float64)
    tau = np.asarray(t_rel, np.float32).astype(np.float64) * np.float64(unit)
    bad = np.isnan(tau)
    if round_s > 0:
        with np.errstate(invalid="ignore"):
            tau = np.rint(tau / np.float64(round_s)) * np.float64(round_s)
    out = (tau < s[0]) | (tau > s[-1])
    if extrapolate:
        tau = np.where(tau < s[0], s[0], np.where(tau > s[-1], s[-1], tau))
    else:
        bad = bad | out
    return tau, bad


# ---- float64 -----------------------------------------------------------------------------------------------------------------
def _unit_quats(poses):
    q = np.asarray(poses, np.float64)[:, 3:7]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def pose_at(stamps, poses, tau):
    """(Rotation, translation (M, 3)) of the sensor at the times tau: slerp along the shorter arc, linear translation"""
    s = np.asarray(stamps, np.float64)
    P = np.asarray(poses, np.float64)
    tau = np.atleast_1d(np.asarray(tau, np.float64))
    R = Slerp(s, Rotation.from_quat(_unit_quats(P)))(tau)
    p = np.stack([np.interp(tau, s, P[:, c]) for c in range(3)], axis=1)
    return R, p


def deskew64(points, t_rel, stamps, poses, ref=0.0, unit=1e-9, round_s=0.0, extrapolate=False, normals=None):
    """the float64 reference: (out (N, 3), normals_out (N, 3) or None, |relative translation| (N,)); rows of failing points are NaN"""
    x = np.asarray(points, np.float32).astype(np.float64)[:, :3]
    tau, bad = point_times(t_rel, stamps, unit, round_s, extrapolate)
    tau_ok = np.where(bad, np.asarray(stamps, np.float64)[0], tau)
    R, p = pose_at(stamps, poses, tau_ok)
    Rr, pr = pose_at(stamps, poses, [ref])
    Rrel = Rr.inv() * R
    prel = Rr.inv().apply(p - pr)
    out = Rrel.apply(x) + prel
    out[bad] = np.nan
    nout = None
    if normals is not None:
        nout = Rrel.apply(np.asarray(normals, np.float32).astype(np.float64))
        nout[bad] = np.nan
    return out, nout, np.linalg.norm(prel, axis=1)


def _qmul(a, b):
    """Hamilton product of (x, y, z, w) quaternions: the rotation of b, then of a"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def prepare64(stamps, poses, ref=0.0):
    """the table of icpmi_deskew_table in float64: q (K, 4) sign-continued, p (K, 3), omega (K - 1,), inv_sin (K - 1,)"""
    P = np.asarray(poses, np.float64)
    K = P.shape[0]
    Rr, pr = pose_at(stamps, poses, [ref])
    qr = Rr.as_quat()[0]
    qri = qr * np.array([-1.0, -1.0, -1.0, 1.0])
    uq = _unit_quats(P)
    q = np.empty((K, 4))
    for k in range(K):
        qk = _qmul(qri, uq[k])
        qk /= np.linalg.norm(qk)
        if k > 0 and np.dot(q[k - 1], qk) < 0:
            qk = -qk
        q[k] = qk
    p = Rr.inv().apply(P[:, :3] - pr)
    omega = 2.0 * np.arctan2(np.linalg.norm(q[1:] - q[:-1], axis=1), np.linalg.norm(q[1:] + q[:-1], axis=1))
    with np.errstate(divide="ignore"):
        inv_sin = np.where(omega < LERP_BELOW, 0.0, 1.0 / np.sin(omega))
    return q, p, omega, inv_sin


# ---- float32: include/icpmi.h line by line --------------------------------------------------------------------------------------
def deskew32(points, t_rel, stamps, table, unit=1e-9, round_s=0.0, extrapolate=False, normals=None):
    """table = (q, p, omega, inv_sin) as float32 arrays.  Returns (out (N, 4) float32, normals_out or None, failing mask)"""
    q, p, omega, inv_sin = (np.asarray(a, F32) for a in table)
    x = np.asarray(points, F32)
    s = np.asarray(stamps, np.float64)
    K = s.shape[0]
    tau, bad = point_times(t_rel, stamps, unit, round_s, extrapolate)
    tau = np.where(bad, s[0], tau)
    k = np.clip(np.searchsorted(s, tau, side="right") - 1, 0, K - 2)      # the largest k in [0, K - 2] with s_k <= tau
    u = ((tau - s[k]) / (s[k + 1] - s[k])).astype(F32)
    one, two = F32(1), F32(2)
    um = one - u
    om, isn = omega[k], inv_sin[k]
    lerp = isn == 0
    w0 = np.where(lerp, um, np.sin(um * om, dtype=F32) * isn).astype(F32)
    w1 = np.where(lerp, u, np.sin(u * om, dtype=F32) * isn).astype(F32)
    qa, qb, pa, pb = q[k], q[k + 1], p[k], p[k + 1]
    qx, qy, qz, qw = (w0 * qa[:, c] + w1 * qb[:, c] for c in range(4))
    px, py, pz = (um * pa[:, c] + u * pb[:, c] for c in range(3))
    xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
    R = [[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)],
         [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
         [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]]
    out = np.empty_like(x)
    for r, pr in enumerate((px, py, pz)):
        out[:, r] = ((R[r][0] * x[:, 0] + R[r][1] * x[:, 1]) + R[r][2] * x[:, 2]) + pr
    out[:, 3] = x[:, 3]
    assert out.dtype == F32 and u.dtype == F32 and R[0][0].dtype == F32
    nout = None
    if normals is not None:
        nn = np.asarray(normals, F32)
        nout = np.stack([(R[r][0] * nn[:, 0] + R[r][1] * nn[:, 1]) + R[r][2] * nn[:, 2] for r in range(3)], axis=1)
    return out, nout, bad


def table32(stamps, poses, ref=0.0):
    return tuple(a.astype(F32) for a in prepare64(stamps, poses, ref))


# ---- shared inputs --------------------------------------------------------------------------------------------------------------
SWEEP_S = 0.1                     # one revolution of the lidar
SPAN = (-0.005, 0.105)            # the pose table covers the sweep with a margin


def make_motion(K, seed, max_rate=3.0, max_speed=30.0, flip_signs=True, planar=False, stamps=None):
    """K timed poses of a sensor that turns at up to max_rate rad/s and moves at up to max_speed m/s, somewhere in a map (coordinates
    of hundreds of metres), at jittered stamps over SPAN (or at `stamps`).  Returns (stamps (K,), poses (K, 7))."""
    rng = np.random.default_rng(seed)
    s = np.linspace(SPAN[0], SPAN[1], K)
    if K > 2:
        s[1:-1] += rng.uniform(-0.3, 0.3, K - 2) * (s[1] - s[0])
    if stamps is not None:
        s = np.asarray(stamps, np.float64)
    axis = rng.normal(size=3)
    if planar:
        axis = np.array([0.0, 0.0, 1.0])
    axis /= np.linalg.norm(axis)
    wobble = rng.normal(size=3) * (0.0 if planar else 1.0)
    rate = rng.uniform(0.5, 1.0) * max_rate
    # the angular rate is |rate - 0.2 rate sin| <= rate: rotvec(s) = axis * rate * (s + 0.2 * 0.02 cos(s / 0.02)) + a small wobble
    ang = rate * (s + 0.004 * np.cos(s / 0.02))
    R0 = Rotation.from_rotvec(np.array([0.0, 0.0, 0.7]) if planar else rng.normal(size=3))
    R = R0 * Rotation.from_rotvec(ang[:, None] * axis[None, :] + 1e-3 * np.sin(40.0 * s)[:, None] * wobble[None, :])
    v = rng.normal(size=3)
    v *= rng.uniform(0.5, 1.0) * max_speed / np.linalg.norm(v)
    base = np.array([812.5, -364.25, 12.125])
    p = base + s[:, None] * v[None, :] + 0.5 * (s ** 2)[:, None] * rng.normal(size=3)[None, :] * 20.0
    q = R.as_quat()
    if planar:
        p[:, 2] = 0.0
        q[:, 0] = 0.0
        q[:, 1] = 0.0
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    if flip_signs:
        q[rng.random(K) < 0.5] *= -1.0
    return s, np.concatenate([p, q], axis=1)


def make_points(n, seed, planar=False):
    """n points at ranges 0.5 - 120 m with unit normals, and nearly time-ordered times in nanoseconds over one sweep (float32)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    if planar:
        d[:, 2] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rng_m = np.exp(rng.uniform(np.log(0.5), np.log(120.0), n))
    pts = np.ones((n, 4), F32)
    pts[:, :3] = (d * rng_m[:, None]).astype(F32)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    t = (np.arange(n) + rng.uniform(0.0, 1.0, n)) / n * SWEEP_S * 1e9 if n > 1 else np.array([0.37 * SWEEP_S * 1e9])
    return pts, nrm.astype(F32), np.sort(t).astype(F32)


SWEEP_N = (1, 63, 64, 65, 255, 256, 257, 4099)   # around the wave and the workgroup, and more than one workgroup with a ragged tail
SWEEP_K = (2, 3, 11, 1024)


@functools.lru_cache(maxsize=None)
def sweep_case(n, K):
    """one case of the GPU test's size and shape sweep, with its float64 reference (computed once, shared, never modified)"""
    seed = 1000 * K + n
    stamps, poses = make_motion(K, seed)
    pts, nrm, t = make_points(n, seed + 1)
    ref = float(np.random.default_rng(seed + 2).uniform(0.0, SWEEP_S))
    out64, n64, pnorm = deskew64(pts, t, stamps, poses, ref=ref, normals=nrm)
    case = dict(n=n, K=K, stamps=stamps, poses=poses, pts=pts, nrm=nrm, t=t, ref=ref, out64=out64, n64=n64, pnorm=pnorm)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def rel_error(out, case):
    """max over the points of |out - float64| / (|x| + |p|)"""
    x = case["pts"].astype(np.float64)[:, :3]
    err = np.linalg.norm(np.asarray(out, np.float64)[:, :3] - case["out64"], axis=1)
    return float((err / (np.linalg.norm(x, axis=1) + case["pnorm"])).max())


@functools.lru_cache(maxsize=None)
def measured_tolerance():
    """the largest |float32 restatement - float64| / (|x| + |p|) over the GPU test's sweep"""
    worst = 0.0
    for n in SWEEP_N:
        for K in SWEEP_K:
            c = sweep_case(n, K)
            out32, _, bad = deskew32(c["pts"], c["t"], c["stamps"], table32(c["stamps"], c["poses"], c["ref"]))
            assert not bad.any()
            worst = max(worst, rel_error(out32, c))
    return worst


def device_bound():
    """4 x the measured float32-against-float64 figure: the device's sinf and numpy's may differ by a few ulp on the same inputs, and
    nothing else differs"""
    return 4.0 * measured_tolerance()
