"""numpy float32 restatement of the four sensor-model DataPointsFilters (include/icpmi.h: icpmi_sensor_model; libpointmatcher 1.4.x as
recalled): ObservationDirection, OrientNormals, Shadow, SimpleSensorNoise.  Every product, sum, division and square root is ONE float32
operation, rounded before the next one starts, in the order the header writes them: the device, compiled without contraction, must give the
same bits.  (numpy evaluates an expression on float32 arrays operation by operation in float32; `_r` states the rounding and refuses a
silent promotion.)"""
import numpy as np

F = np.float32

# sensorType -> (minRadius, beamAngle, beamConst): Sick LMS-1xx, Hokuyo URG-04LX, Hokuyo UTM-30LX
SENSORS = {0: (0.012, 0.0068, 0.0008), 1: (0.028, 0.0013, 0.0001), 2: (0.018, 0.0006, 0.0015)}


def _r(a):
    """the float32 result of one operation"""
    a = np.asarray(a)
    assert a.dtype == F, a.dtype
    return a


def _xyz(a):
    a = np.ascontiguousarray(a, dtype=F)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def sqnorm(x, y, z):
    """x x + y y + z z, left to right"""
    return _r(_r(_r(x * x) + _r(y * y)) + _r(z * z))


def norm(x, y, z):
    return _r(np.sqrt(sqnorm(x, y, z)))


def observation_direction(cloud, s):
    """od = s - p"""
    px, py, pz = _xyz(cloud)
    s = np.asarray(s, dtype=F)
    return np.stack([_r(s[0] - px), _r(s[1] - py), _r(s[2] - pz)], 1)


def orient_normals(normals, od, toward_center=True):
    """d = n . od summed left to right; the normal is negated when towardCenter ? d < 0 : d > 0"""
    nx, ny, nz = _xyz(normals)
    ox, oy, oz = _xyz(od)
    d = _r(_r(_r(nx * ox) + _r(ny * oy)) + _r(nz * oz))
    flip = (d < 0) if toward_center else (d > 0)
    out = np.stack([nx, ny, nz], 1)
    out[flip] = -out[flip]
    return out


def shadow_value(cloud, normals):
    """v = | (n / |n|) . (p / |p|) |: NaN where |n| == 0, |p| == 0 or an input is NaN"""
    px, py, pz = _xyz(cloud)
    nx, ny, nz = _xyz(normals)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln, lp = norm(nx, ny, nz), norm(px, py, pz)
        t = _r(_r(_r(_r(nx / ln) * _r(px / lp)) + _r(_r(ny / ln) * _r(py / lp))) + _r(_r(nz / ln) * _r(pz / lp)))
        return _r(np.abs(t))


def shadow_keep(cloud, normals, eps=0.1):
    """kept iff v > eps (a NaN compares false: dropped)"""
    with np.errstate(invalid="ignore"):
        return shadow_value(cloud, normals) > F(eps)


def simple_sensor_noise(cloud, sensor_type=0, gain=1.0):
    px, py, pz = _xyz(cloud)
    dist = norm(px, py, pz)
    g = F(gain)
    if sensor_type in SENSORS:
        min_radius, beam_angle, beam_const = (F(v) for v in SENSORS[sensor_type])
        t = _r(_r(beam_angle * dist) + beam_const)
        with np.errstate(invalid="ignore"):
            return _r(g * np.where(t > min_radius, t, min_radius).astype(F))
    if sensor_type in (3, 4):  # Kinect, Xtion
        return _r(_r(_r(g * F(0.5)) * F(0.00285)) * _r(dist * dist))
    raise ValueError("sensorType must be 0 .. 4")


def run(cloud, steps, normals=None, obs_dirs=None):
    """the program of ICPSequence.sensorModel, step by step: the same dict (rows NOT compacted)"""
    n = None if normals is None else np.ascontiguousarray(normals, dtype=F).copy()
    od = None if obs_dirs is None else np.ascontiguousarray(obs_dirs, dtype=F).copy()
    keep = np.ones(np.shape(cloud)[0], bool)
    out = {}
    for st in steps:
        if st[0] == "observation_direction":
            od = observation_direction(cloud, st[1:4])
            out["observationDirections"] = od
        elif st[0] == "orient_normals":
            n = orient_normals(n, od, bool(st[1]) if len(st) > 1 else True)
            out["normals"] = n
        elif st[0] == "shadow":
            keep &= shadow_keep(cloud, n, st[1] if len(st) > 1 else 0.1)
            out["keep"] = keep
        elif st[0] == "simple_sensor_noise":
            out["simpleSensorNoise"] = simple_sensor_noise(cloud, st[1] if len(st) > 1 else 0, st[2] if len(st) > 2 else 1.0)
        else:
            raise ValueError(st[0])
    return out
