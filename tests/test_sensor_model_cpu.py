"""CPU checks of the sensor-model filters: the numpy restatement (tests/sensor_model_reference.py) against values worked out by hand, the
host classes that run without a GPU context against it bit for bit, and what the host shell's factory accepts and refuses."""
import numpy as np
import pytest

import sensor_model_reference as smr

F = np.float32


def _c4(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


def _host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    hb.load()
    import host_chain_bindings as hcb
    return hb, hcb


def test_lms_noise_by_hand():
    # 1 m: beamAngle * 1 + beamConst = 0.0076 is below minRadius; 10 m: 0.068 + 0.0008
    z = smr.simple_sensor_noise(_c4([[1, 0, 0], [0, 10, 0]]), 0, 1.0)
    assert z.dtype == F
    assert z[0] == F(0.012)
    # three float32 roundings (the constant, the product, the sum), each within 2^-24 relative
    assert z[1] == pytest.approx(0.0688, rel=4 * 2.0 ** -24)
    assert smr.simple_sensor_noise(_c4([[1, 0, 0]]), 0, 2.0)[0] == F(2.0) * F(0.012)


def test_hokuyo_and_kinect_noise_by_hand():
    p = _c4([[0, 0, 2]])
    # Kinect at 2 m: 0.5 * 0.00285 * 4: the factors 0.5 and 4 are powers of two, so the result is float32(0.0057) exactly
    assert smr.simple_sensor_noise(p, 3, 1.0)[0] == F(0.0057)
    assert smr.simple_sensor_noise(p, 4, 1.0)[0] == F(0.0057)
    assert smr.simple_sensor_noise(p, 1, 1.0)[0] == F(0.028)       # 0.0013 * 2 + 0.0001 < minRadius
    assert smr.simple_sensor_noise(_c4([[0, 0, 30]]), 2, 1.0)[0] == pytest.approx(0.0006 * 30 + 0.0015, rel=4 * 2.0 ** -24)
    with pytest.raises(ValueError):
        smr.simple_sensor_noise(p, 5, 1.0)


def test_shadow_on_a_plane_by_hand():
    # a plane with normal +z seen under 85 and 30 degrees from its normal: v = cos(angle) = 0.087 and 0.866
    a = np.deg2rad([85.0, 30.0])
    p = _c4(np.stack([7.0 * np.sin(a), np.zeros(2), 7.0 * np.cos(a)], 1))
    n = np.tile(np.array([0, 0, 1], F), (2, 1))
    v = smr.shadow_value(p, n)
    assert v == pytest.approx(np.cos(a), abs=1e-6)
    assert smr.shadow_keep(p, n, 0.1).tolist() == [False, True]
    assert smr.shadow_keep(p, -n, 0.1).tolist() == [False, True]        # the sign of the normal does not matter
    # zero position, zero normal, NaN: v is NaN and the point goes
    bad_p = _c4([[0, 0, 0], [1, 2, 3], [np.nan, 1, 1]])
    bad_n = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1]], F)
    assert np.isnan(smr.shadow_value(bad_p, bad_n)).all()
    assert not smr.shadow_keep(bad_p, bad_n, 0.0).any()


def test_observation_direction_and_orient_by_hand():
    p = _c4([[1, 2, 3], [-4, 0, 1]])
    od = smr.observation_direction(p, (0.5, 0, 1))
    assert np.array_equal(od, np.array([[-0.5, -2, -2], [4.5, 0, 0]], F))
    n = np.array([[0, 0, 1], [1, 0, 0]], F)                              # n . od = -2 and 4.5
    assert np.array_equal(smr.orient_normals(n, od, True), np.array([[0, 0, -1], [1, 0, 0]], F))
    assert np.array_equal(smr.orient_normals(n, od, False), np.array([[0, 0, 1], [-1, 0, 0]], F))


def test_host_classes_without_context_equal_the_reference():
    """ObservationDirection + OrientNormals on the path a chain without a GPU context takes: the bits of the restatement"""
    _, hcb = _host()
    rng = np.random.default_rng(3)
    p = _c4(rng.uniform(-10, 10, (1000, 3)))
    n = rng.normal(size=(1000, 3)); n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    yaml = "- ObservationDirectionDataPointsFilter: {x: 0.5, y: -1.25, z: 2.0}\n- OrientNormalsDataPointsFilter: {towardCenter: %d}\n"
    for toward in (1, 0):
        out, descs = hcb.filter_chain_descs(yaml % toward, p, [("normals", n)])
        assert np.array_equal(out, p)
        assert [nm for nm, _ in descs] == ["observationDirections", "normals"]
        od = smr.observation_direction(p, (0.5, -1.25, 2.0))
        assert np.array_equal(descs[0][1].view(np.uint32), od.view(np.uint32))
        assert np.array_equal(descs[1][1].view(np.uint32), smr.orient_normals(n, od, bool(toward)).view(np.uint32))


@pytest.mark.parametrize("entry, text", [
    ("ShadowDataPointsFilter: {eps: -0.01}", "eps"),
    ("ShadowDataPointsFilter: {eps: 1.5}", "eps"),
    ("ShadowDataPointsFilter: {eps: nan}", "eps"),
    ("ShadowDataPointsFilter: {eps: inf}", "eps"),
    ("ShadowDataPointsFilter: {epsilon: 0.1}", "epsilon"),
    ("SimpleSensorNoiseDataPointsFilter: {sensorType: 5}", "sensorType"),
    ("SimpleSensorNoiseDataPointsFilter: {sensorType: -1}", "sensorType"),
    ("SimpleSensorNoiseDataPointsFilter: {gain: 0}", "gain"),
    ("SimpleSensorNoiseDataPointsFilter: {gain: -2}", "gain"),
    ("SimpleSensorNoiseDataPointsFilter: {gain: inf}", "gain"),
    ("SimpleSensorNoiseDataPointsFilter: {gain: nan}", "gain"),
    ("SimpleSensorNoiseDataPointsFilter: {sensor: 0}", "sensor"),
])
def test_factory_rejects(entry, text):
    hb, _ = _host()
    with pytest.raises(RuntimeError) as e:
        hb.filter_chain("- " + entry + "\n", _c4([[1, 2, 3]]))
    assert text in str(e.value)


@pytest.mark.parametrize("entry", ["ShadowDataPointsFilter", "ShadowDataPointsFilter: {eps: 0}", "ShadowDataPointsFilter: {eps: 1}",
                                   "SimpleSensorNoiseDataPointsFilter", "SimpleSensorNoiseDataPointsFilter: {sensorType: 4, gain: 0.5}"])
def test_without_a_context_the_device_filters_say_so(entry):
    """the factory accepts the entry (defaults and the ends of the ranges included); running it needs the GPU"""
    hb, _ = _host()
    n = np.tile(np.array([0, 0, 1], F), (2, 1))
    with pytest.raises(RuntimeError) as e:
        hb.filter_chain("- " + entry + "\n", _c4([[1, 2, 3], [4, 5, 6]]), desc_name="normals", desc=n)
    assert "needs a GPU context" in str(e.value)
