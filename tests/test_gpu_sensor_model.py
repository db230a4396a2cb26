"""The four sensor-model DataPointsFilters as one device pass (icpmi_sensor_model, csrc/ops.hip: sensor_model_kernel) and in the host
shell, against the float32 restatement (tests/sensor_model_reference.py): every row bit for bit at the wave and workgroup edges, the Shadow
mask, a fused run against the same filters one by one, SimpleSensorNoise feeding errorMinimizer->getOverlap() end to end, reproducibility
and the errors."""
import numpy as np
import pytest

import sensor_model_reference as smr

pytestmark = pytest.mark.gpu

F = np.float32
S = (0.5, -1.25, 2.0)   # a sensor position off the origin


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def icp(amd):
    return amd.ICPSequence()


@pytest.fixture(scope="module")
def host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    hb.load()
    import host_chain_bindings as hcb
    return hb, hcb


def _c4(xyz):
    xyz = np.asarray(xyz, F)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


_CLOUDS = {}


def _cloud(n, seed=7):
    """random points in a 20 m box, random unit normals, random observation directions"""
    if (n, seed) not in _CLOUDS:
        rng = np.random.default_rng(seed)
        p = _c4(rng.uniform(-10, 10, (n, 3)))
        nrm = rng.normal(size=(n, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
        od = rng.uniform(-10, 10, (n, 3)).astype(F)
        _CLOUDS[(n, seed)] = (p, nrm, od)
    return _CLOUDS[(n, seed)]


def _same(got, ref):
    assert sorted(got) == sorted(ref)
    for key in ref:
        if key == "keep":
            assert got[key].dtype == bool and np.array_equal(got[key], ref[key]), key
        else:
            assert got[key].shape == ref[key].shape and np.array_equal(_bits(got[key]), _bits(ref[key])), key


ALL_FOUR = [("observation_direction",) + S, ("orient_normals", 1), ("shadow", 0.1), ("simple_sensor_noise", 0, 1.0)]


# ------------------------------------------------------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_every_step_alone_and_all_four_bit_equal(icp, n):
    p, nrm, od = _cloud(n)
    programs = [[("observation_direction",) + S],
                [("orient_normals", 1)], [("orient_normals", 0)],
                [("shadow", 0.1)],
                [("simple_sensor_noise", 0, 1.0)], [("simple_sensor_noise", 1, 1.0)], [("simple_sensor_noise", 2, 2.5)],
                [("simple_sensor_noise", 3, 1.0)], [("simple_sensor_noise", 4, 0.75)],
                ALL_FOUR,
                # the order matters: a second ObservationDirection after OrientNormals changes od, not the normals; the last noise step wins
                [("observation_direction", 0, 0, 0), ("orient_normals", 0), ("observation_direction",) + S, ("simple_sensor_noise", 3, 1.0),
                 ("simple_sensor_noise", 1, 2.0), ("shadow", 0.3), ("shadow", 0.1), ("orient_normals", 1)]]
    for steps in programs:
        got = icp.sensorModel(p, steps, normals=nrm, obs_dirs=od)
        ref = smr.run(p, steps, normals=nrm, obs_dirs=od)
        if n:  # (the reference's own band around eps must be empty for the masks to be comparable: see the Shadow test)
            v = smr.shadow_value(p, ref.get("normals", nrm)).astype(np.float64)
            for st in steps:
                if st[0] == "shadow":
                    assert np.count_nonzero(np.abs(v - float(F(st[1]))) <= 4 * 2.0 ** -24) == 0
        _same(got, ref)
        for key in got:
            assert got[key].shape[0] == n


# ------------------------------------------------------------------------------------------------------------------ 2. Shadow
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.9, 1.0])
def test_shadow_mask(icp, eps):
    p, nrm, _ = _cloud(4099, seed=21)
    p, nrm = p.copy(), nrm.copy()
    p[17, :3] = 0                      # a point at the origin
    nrm[300] = 0                       # a zero normal
    p[4000, 1] = np.nan                # a NaN coordinate
    special = [17, 300, 4000]
    v = smr.shadow_value(p, nrm)
    assert np.isnan(v[special]).all() and np.isfinite(np.delete(v, special)).all()
    # the mask may differ from the reference's only where v is within 4 * 2^-24 of eps; the inputs put no point there, so it may not differ
    band = np.abs(np.delete(v, special).astype(np.float64) - float(F(eps))) <= 4 * 2.0 ** -24
    assert np.count_nonzero(band) == 0
    ref = smr.shadow_keep(p, nrm, eps)
    got = icp.sensorModel(p, [("shadow", eps)], normals=nrm)
    assert sorted(got) == ["keep"]
    assert np.array_equal(got["keep"], ref)
    assert not got["keep"][special].any()
    if 0.0 < eps < 1.0:
        assert 0 < np.count_nonzero(got["keep"]) < p.shape[0] - 3


# ------------------------------------------------------------------------------------------------------------------ 3. fusion
def _two_planes(n=5000, seed=5):
    """a floor half a metre under the origin (most of it seen at a grazing angle) and a wall, a few millimetres rough"""
    rng = np.random.default_rng(seed)
    k = n // 2
    floor = np.stack([rng.uniform(-8, 8, k), rng.uniform(-8, 8, k), -0.5 + 0.004 * rng.normal(size=k)], 1)
    wall = np.stack([6.0 + 0.004 * rng.normal(size=n - k), rng.uniform(-8, 8, n - k), rng.uniform(-1.5, 4, n - k)], 1)
    return _c4(np.concatenate([floor, wall]))


CHAIN = ["SurfaceNormalDataPointsFilter: {knn: 5}",
         "ObservationDirectionDataPointsFilter: {x: 0.5, y: -1.25, z: 2.0}",
         "OrientNormalsDataPointsFilter: {towardCenter: 1}",
         "ShadowDataPointsFilter: {eps: 0.1}",
         "SimpleSensorNoiseDataPointsFilter: {sensorType: 0}"]


def test_fused_run_equals_one_by_one(icp, host):
    hb, hcb = host
    h = icp._h.value
    p = _two_planes()
    fused, fdescs = hcb.filter_chain_descs("".join("- " + e + "\n" for e in CHAIN), p, handle=h)
    cloud, descs = p, []
    for e in CHAIN:
        cloud, descs = hcb.filter_chain_descs("- " + e + "\n", cloud, descs, handle=h)
    assert 0 < fused.shape[0] < p.shape[0]                       # the Shadow step dropped something, not everything
    assert np.array_equal(_bits(fused), _bits(cloud))
    assert [nm for nm, _ in fdescs] == [nm for nm, _ in descs] == ["observationDirections", "normals", "simpleSensorNoise"]
    for (nm, a), (_, b) in zip(fdescs, descs):
        assert a.shape == b.shape and a.shape[0] == fused.shape[0] and np.array_equal(_bits(a), _bits(b)), nm
    # ... and the rows are the reference's on the kept points
    d = dict(fdescs)
    assert np.array_equal(_bits(d["observationDirections"]), _bits(smr.observation_direction(fused, S)))
    assert np.array_equal(_bits(d["simpleSensorNoise"][:, 0]), _bits(smr.simple_sensor_noise(fused, 0, 1.0)))
    assert smr.shadow_keep(fused, d["normals"], 0.1).all()
    # the established entry gives the same cloud and normals
    out, nrm, _ = hb.filter_chain("".join("- " + e + "\n" for e in CHAIN), p, handle=h)
    assert np.array_equal(_bits(out), _bits(fused)) and np.array_equal(_bits(nrm), _bits(d["normals"]))


@pytest.mark.parametrize("toward", [1, 0])
def test_observation_direction_and_orient_normals_equal_the_host_classes(icp, host, toward):
    _, hcb = host
    p, nrm, _ = _cloud(5000, seed=9)
    yaml = ("- ObservationDirectionDataPointsFilter: {x: 0.5, y: -1.25, z: 2.0}\n"
            "- OrientNormalsDataPointsFilter: {towardCenter: %d}\n" % toward)
    # an `observationDirections` row that is already there is replaced, and both rows move to the end, on either path
    descs = [("observationDirections", np.zeros((5000, 3), F)), ("normals", nrm), ("intensity", np.arange(5000, dtype=F))]
    dev_cloud, dev = hcb.filter_chain_descs(yaml, p, descs, handle=icp._h.value)
    cpu_cloud, cpu = hcb.filter_chain_descs(yaml, p, descs, handle=None)
    assert np.array_equal(_bits(dev_cloud), _bits(cpu_cloud)) and np.array_equal(_bits(dev_cloud), _bits(p))
    assert [nm for nm, _ in dev] == [nm for nm, _ in cpu] == ["intensity", "observationDirections", "normals"]
    for (nm, a), (_, b) in zip(dev, cpu):
        assert np.array_equal(_bits(a), _bits(b)), nm
    flipped = np.count_nonzero((_bits(dict(dev)["normals"]) != _bits(nrm)).any(1))
    assert 0 < flipped < 5000
    # OrientNormals alone reads the row the cloud carries
    od = smr.observation_direction(p, S)
    alone = "- OrientNormalsDataPointsFilter: {towardCenter: %d}\n" % toward
    _, dev1 = hcb.filter_chain_descs(alone, p, [("normals", nrm), ("observationDirections", od)], handle=icp._h.value)
    _, cpu1 = hcb.filter_chain_descs(alone, p, [("normals", nrm), ("observationDirections", od)], handle=None)
    assert [nm for nm, _ in dev1] == [nm for nm, _ in cpu1] == ["observationDirections", "normals"]
    assert np.array_equal(_bits(dict(dev1)["normals"]), _bits(dict(cpu1)["normals"]))
    assert np.array_equal(_bits(dict(dev1)["normals"]), _bits(dict(dev)["normals"]))


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
ICP_YAML = """matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 2.0
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.85
errorMinimizer:
  PointToPlaneErrorMinimizer:
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 12
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.001
      smoothLength: 3
"""
READING_NOISE = """readingDataPointsFilters:
  - SimpleSensorNoiseDataPointsFilter:
      sensorType: 0
"""


def test_simple_sensor_noise_in_the_reading_chain_feeds_get_overlap(host, mid_scene):
    """the reason for the filter: a chain that lists it among its readingDataPointsFilters gets upstream's sensor-noise overlap, the very
    value a caller got by handing the same row over by hand"""
    _, hcb = host
    sc = mid_scene
    n = sc["scan"].shape[0]
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    T_plain, st_plain = hcb.icp_register(ICP_YAML, sc["map"], sc["normals"], sc["scan"], nrm)
    assert st_plain.sensor_noise_overlap == -1.0
    T_f, st_f = hcb.icp_register(ICP_YAML + READING_NOISE, sc["map"], sc["normals"], sc["scan"], nrm)
    assert st_f.sensor_noise_overlap != -1.0
    assert 0.0 <= st_f.sensor_noise_overlap <= 1.0
    T_h, st_h = hcb.icp_register(ICP_YAML, sc["map"], sc["normals"], sc["scan"], nrm, noise=smr.simple_sensor_noise(sc["scan"], 0, 1.0))
    assert F(st_f.sensor_noise_overlap).view(np.uint32) == F(st_h.sensor_noise_overlap).view(np.uint32)
    assert st_f.iterations == st_h.iterations == st_plain.iterations and st_f.pairs == st_h.pairs
    assert np.array_equal(_bits(T_f), _bits(T_h)) and np.array_equal(_bits(T_f), _bits(T_plain))


# ------------------------------------------------------------------------------------------------------------------ 5. the rest
def test_two_calls_give_the_same_bytes(icp):
    p, nrm, od = _cloud(1000)
    a = icp.sensorModel(p, ALL_FOUR, normals=nrm)
    b = icp.sensorModel(p, ALL_FOUR, normals=nrm)
    assert sorted(a) == ["keep", "normals", "observationDirections", "simpleSensorNoise"]
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_errors(amd, icp):
    from norlab_icp_mapper_amd.icp import InvalidField, InvalidParameter
    p, nrm, od = _cloud(257)
    with pytest.raises(InvalidField, match="ShadowDataPointsFilter: Error, cannot find normals"):
        icp.sensorModel(p, [("shadow", 0.1)])
    with pytest.raises(InvalidField, match="OrientNormalsDataPointsFilter: Error, cannot find normals"):
        icp.sensorModel(p, ALL_FOUR)
    # OrientNormals before any ObservationDirection step, and no row to read
    with pytest.raises(InvalidField, match="cannot find observation directions"):
        icp.sensorModel(p, [("orient_normals", 1), ("observation_direction",) + S], normals=nrm)
    icp.sensorModel(p, [("orient_normals", 1)], normals=nrm, obs_dirs=od)
    for steps in ([("shadow", -0.1)], [("shadow", 1.01)], [("shadow", float("nan"))], [("simple_sensor_noise", 5, 1.0)],
                  [("simple_sensor_noise", -1, 1.0)], [("simple_sensor_noise", 0, 0.0)], [("simple_sensor_noise", 0, float("inf"))],
                  [("simple_sensor_noise", 0, float("nan"))], [("simple_sensor_noise", 0, 1.0)] * 9):
        with pytest.raises(InvalidParameter):
            icp.sensorModel(p, steps, normals=nrm)


def test_required_outputs_and_planar_handle(amd, icp):
    """the C entry itself: a NULL output the program produces is refused, one it does not produce may be NULL; a planar handle is served"""
    import ctypes as C
    from norlab_icp_mapper_amd import _capi
    lib = _capi.load()
    p, nrm, _ = _cloud(65)
    st = (_capi.SensorStep * 1)()
    st[0].type = _capi.SM_SIMPLE_SENSOR_NOISE; st[0].f[0] = 1.0
    assert lib.icpmi_sensor_model(icp._h, p.ctypes.data, 65, None, None, st, 1, None, None, None, None) == _capi.ERR_INVALID_ARG
    noise = np.empty(65, F)
    assert lib.icpmi_sensor_model(icp._h, p.ctypes.data, 65, None, None, st, 1, None, None, noise.ctypes.data, None) == 0
    assert np.array_equal(_bits(noise), _bits(smr.simple_sensor_noise(p, 0, 1.0)))
    assert lib.icpmi_sensor_model(icp._h, p.ctypes.data, 0, None, None, st, 1, None, None, None, None) == 0       # the empty call
    assert lib.icpmi_sensor_model(icp._h, p.ctypes.data, C.c_int64(2 ** 31), None, None, st, 1, None, None, noise.ctypes.data, None) == _capi.ERR_UNSUPPORTED
    st[0].type = _capi.SM_SHADOW; st[0].f[0] = 0.1
    assert lib.icpmi_sensor_model(icp._h, p.ctypes.data, 65, nrm.ctypes.data, None, st, 1, None, None, None, None) == _capi.ERR_INVALID_ARG
    st[0].type = 7
    assert lib.icpmi_sensor_model(icp._h, p.ctypes.data, 65, nrm.ctypes.data, None, st, 1, None, None, None, None) == _capi.ERR_INVALID_ARG
    flat = amd.ICPSequence(is_2d=1, minimizer=1)
    q = p.copy(); q[:, 2] = 0
    m = nrm.copy(); m[:, 2] = 0
    _same(flat.sensorModel(q, ALL_FOUR, normals=m), smr.run(q, ALL_FOUR, normals=m))
    flat.close()
