"""One handle walked through the pair models of the pair-sum kernel: nothing a model sets may leak into the next one.

The handle goes point-to-plane -> intensity term (w = 0.3) -> plane-to-plane (eps = 1e-3) -> symmetric -> point-to-plane with a
degeneracy_threshold -> plain point-to-plane again.  At every stop the sums and the step of icpmi_minimize_step, and the sums (keepSums /
lastSums) and the pose of a three-iteration registration, are bit-equal to those of a fresh handle configured directly for that stop.
Behaviour, not layout: epsilon, the photometric weight, the (g, I) array, the reading's intensity row and the side block of the
degeneracy-aware solve each reach the device for the model that owns them and for no other.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N = 4096, 512
MIN_POINT_TO_PLANE, MIN_PLANE_TO_PLANE = 2, 3
TRIM = (4, 0.85)          # TrimmedDistOutlierFilter ratio 0.85
DEGEN_THR = 0.05
# (name, minimizer, handle state: intensity weight / plane model / epsilon, config extras, the reading's normals travel)
STOPS = [
    ("point-to-plane", MIN_POINT_TO_PLANE, dict(intensity_weight=0.0), {}, False),
    ("intensity", MIN_POINT_TO_PLANE, dict(intensity_weight=0.3), {}, False),
    ("plane-to-plane", MIN_PLANE_TO_PLANE, dict(intensity_weight=0.0, plane_model="gicp", plane_epsilon=1e-3), {}, True),
    ("symmetric", MIN_PLANE_TO_PLANE, dict(intensity_weight=0.0, plane_model="symmetric"), {}, True),
    ("degeneracy-aware", MIN_POINT_TO_PLANE, dict(intensity_weight=0.0), dict(degeneracy_threshold=DEGEN_THR), False),
    ("point-to-plane again", MIN_POINT_TO_PLANE, dict(intensity_weight=0.0), {}, False),
]
CHAINS = {"k1": dict(knn=1, outliers=[]), "k3": dict(knn=3, outliers=[]), "trimmed": dict(knn=1, outliers=[TRIM])}


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def scene(amd):
    sc = amd.synth.make_scene(m=M, n=N)

    def intensity(p):  # a smooth field of the position: the map and the reading sample the same one
        return (0.5 + 0.3 * np.sin(0.7 * p[:, 0]) + 0.2 * np.cos(0.9 * p[:, 1]) + 0.1 * np.sin(1.3 * p[:, 2])).astype(np.float32)
    T = sc["T_gt"]
    sc["map_intensity"] = intensity(sc["map"].astype(np.float64))
    sc["scan_intensity"] = intensity(sc["scan"][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3])
    return sc


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _config(chain, minimizer, extra):
    return dict(max_dist=2.0, minimizer=minimizer, max_iterations=3, use_differential=0, **CHAINS[chain], **extra)


def _apply_state(icp, state):
    if "plane_model" in state: icp.setPlaneModel(state["plane_model"])
    if "plane_epsilon" in state: icp.setPlaneEpsilon(state["plane_epsilon"])
    icp.setIntensityWeight(state["intensity_weight"])


def _measure(icp, sc, state, with_normals):
    """(sums and step of one minimize step at the identity, sums and pose of a three-iteration registration)"""
    centred = sc["scan"].copy()
    centred[:, :3] -= icp.getMapMean()[None, :]
    rn = sc["scan_normals"] if with_normals else None
    if state["intensity_weight"] > 0: icp.setReadingIntensity(sc["scan_intensity"])      # (one shot: armed before either call)
    T_step, step_sums = icp.minimizeStep(centred, None, rn)
    icp.keepSums(1)
    if state["intensity_weight"] > 0: icp.setReadingIntensity(sc["scan_intensity"])
    T = icp(sc["scan"], rn)
    reg_sums = icp.lastSums()[0]
    assert icp.stats.iterations == 3
    return _bits64(step_sums), _bits(T_step), _bits64(reg_sums), _bits(T)


@pytest.mark.parametrize("chain", list(CHAINS))
def test_no_field_of_one_pair_model_leaks_into_another(amd, scene, chain):
    walked = amd.ICPSequence(**_config(chain, MIN_POINT_TO_PLANE, {}))
    assert walked.setMap(scene["map"], scene["normals"])
    walked.setMapIntensity(scene["map_intensity"])
    walked.setPlaneEpsilon(0.05)  # (not the default, which is the plane-to-plane stop's 1e-3: that stop's own epsilon has to arrive)
    seen = []
    for name, minimizer, state, extra, with_normals in STOPS:
        # the walked handle: leave the previous model's state before the chain that would refuse it, then enter this one's
        walked.setIntensityWeight(0.0)
        walked.setConfig(**_config(chain, minimizer, extra))
        _apply_state(walked, state)
        got = _measure(walked, scene, state, with_normals)
        fresh = amd.ICPSequence(**_config(chain, minimizer, extra))
        assert fresh.setMap(scene["map"], scene["normals"])
        fresh.setMapIntensity(scene["map_intensity"])
        _apply_state(fresh, state)
        want = _measure(fresh, scene, state, with_normals)
        fresh.close()
        for what, g, w in zip(("minimizeStep sums", "minimizeStep step", "lastSums", "pose"), got, want):
            assert np.array_equal(g, w), (chain, name, what)
        assert np.isfinite(got[2].view(np.float64)).all() and got[2].view(np.float64)[28] > 0, (chain, name)  # (pairs were summed at all)
        seen.append(got)
    walked.close()
    # the stops are different models: their sums differ (a walk that never left point-to-plane would pass the comparison above)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(seen[a][2], seen[b][2]), (chain, STOPS[a][0], STOPS[b][0])
    assert np.array_equal(seen[0][2], seen[5][2]) and np.array_equal(seen[0][3], seen[5][3]), chain  # ... and the way back is the way there
