"""PointToPlaneWithCovErrorMinimizer on the CPU: the numpy restatement (tests/covariance_reference.py) against finite differences of the
linearised cost's gradient, its symmetry and sigma^2 scaling, a corridor scene, the singular sentinel, and the ctypes Config layout."""
import ctypes as C

import numpy as np
import pytest

import covariance_reference as cr


def _random_pairs(seed, m=40):
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 8, (m, 3))
    q = p + rng.normal(0, 0.05, (m, 3))
    n = rng.normal(0, 1, (m, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    x = np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.02, 3)]
    return p, q, n, x


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_terms_are_derivatives_of_the_gradient(seed):
    p, q, n, x = _random_pairs(seed)
    r, rho = np.linalg.norm(p, axis=1), np.linalg.norm(q, axis=1)
    d, u = p / r[:, None], q / rho[:, None]
    h, a, b, _ = cr.terms(p, q, n, x)
    eps = 1e-6
    # H = d(gradient) / dx
    J = np.stack([(cr.gradient(x + eps * e, r, rho, d, u, n) - cr.gradient(x - eps * e, r, rho, d, u, n)) / (2 * eps) for e in np.eye(6)], 1)
    np.testing.assert_allclose(J, h.T @ h, rtol=1e-6, atol=1e-6 * np.abs(h.T @ h).max())
    # column i of a: d(gradient) / d r_i; of b: d(gradient) / d rho_i
    for i in range(p.shape[0]):
        dr = np.zeros_like(r); dr[i] = eps
        ga = (cr.gradient(x, r + dr, rho, d, u, n) - cr.gradient(x, r - dr, rho, d, u, n)) / (2 * eps)
        gb = (cr.gradient(x, r, rho + dr, d, u, n) - cr.gradient(x, r, rho - dr, d, u, n)) / (2 * eps)
        np.testing.assert_allclose(ga, a[i], rtol=1e-6, atol=1e-7 * (1 + np.abs(a[i]).max()))
        np.testing.assert_allclose(gb, b[i], rtol=1e-6, atol=1e-7 * (1 + np.abs(b[i]).max()))


def test_reference_range_in_b_would_fail_the_derivative():
    """the recalled variant that scales b's rotational part by rho instead of r is not the derivative"""
    p, q, n, x = _random_pairs(7)
    p *= 1.5  # ranges that differ clearly
    r, rho = np.linalg.norm(p, axis=1), np.linalg.norm(q, axis=1)
    d, u = p / r[:, None], q / rho[:, None]
    _, _, b, _ = cr.terms(p, q, n, x)
    wrong = b.copy(); wrong[:, 3:] *= (rho / r)[:, None]
    eps = 1e-6
    dr = np.zeros_like(rho); dr[0] = eps
    gb = (cr.gradient(x, r, rho + dr, d, u, n) - cr.gradient(x, r, rho - dr, d, u, n)) / (2 * eps)
    np.testing.assert_allclose(gb, b[0], rtol=1e-6, atol=1e-9)
    assert not np.allclose(gb, wrong[0], rtol=1e-3)


def test_symmetric_and_scales_as_sigma_squared():
    p, q, n, x = _random_pairs(11, 200)
    c1, _, _ = cr.covariance(p, q, n, x, 0.01)
    c2, _, _ = cr.covariance(p, q, n, x, 0.03)
    assert np.array_equal(c1, c1.T)
    np.testing.assert_allclose(c2, 9.0 * c1, rtol=1e-12)
    assert np.all(np.linalg.eigvalsh(c1) > 0)
    f = cr.covariance_f32(p, q, n, x, 0.01)
    assert f.dtype == np.float32 and np.array_equal(f, f.T)


def test_corridor_puts_the_largest_translational_variance_on_y():
    """walls at x = +-2 and floor / ceiling at z = -1 / 2 along a corridor in y: y is held only by a few points on a far end wall"""
    rng = np.random.default_rng(5)
    y = rng.uniform(-20, 20, 3000)
    pts, nrm = [], []
    for wall, axis, normal in ((-2.0, 0, (1, 0, 0)), (2.0, 0, (-1, 0, 0)), (-1.0, 2, (0, 0, 1)), (2.0, 2, (0, 0, -1))):
        P = np.c_[rng.uniform(-2, 2, y.size), y, rng.uniform(-1, 2, y.size)]
        P[:, axis] = wall
        pts.append(P); nrm.append(np.broadcast_to(np.array(normal, float), P.shape))
    end = np.c_[rng.uniform(-2, 2, 30), np.full(30, 20.0), rng.uniform(-1, 2, 30)]
    pts.append(end); nrm.append(np.broadcast_to(np.array([0.0, -1.0, 0.0]), end.shape))
    q = np.concatenate(pts); n = np.concatenate(nrm)
    p = q + rng.normal(0, 0.01, q.shape)
    cov, _, _ = cr.covariance(p, q, n, np.zeros(6), 0.01)
    var_t = np.diag(cov)[:3]
    assert np.argmax(var_t) == 1, var_t
    assert var_t[1] > 10 * max(var_t[0], var_t[2]), var_t


def test_singular_scene_returns_the_sentinel():
    """one plane: translation along it and rotation about its normal are free, H is singular"""
    rng = np.random.default_rng(3)
    q = np.c_[rng.uniform(-5, 5, 500), rng.uniform(-5, 5, 500), np.full(500, -1.5)]
    n = np.broadcast_to(np.array([0.0, 0.0, 1.0]), q.shape)
    cov, H, _ = cr.covariance(q, q, n, np.zeros(6), 0.01)
    assert cov is None
    f = cr.covariance_f32(q, q, n, np.zeros(6), 0.01)
    assert np.array_equal(f, np.eye(6, dtype=np.float32) * np.finfo(np.float32).max)


def test_zero_range_gives_nan():
    p, q, n, x = _random_pairs(4)
    p[0] = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        h, a, b, _ = cr.terms(p, q, n, x)
    assert np.isnan(h[0, 3:]).all() and np.isnan(a[0]).any()


def test_config_layout_keeps_size_and_offsets():
    from norlab_icp_mapper_amd import _capi
    assert C.sizeof(_capi.Config) == 5 * 4 + 8 * 20 + 15 * 4 + 8 * 4
    assert _capi.Config.epsilon_approx.offset == 252  # unchanged; the two new fields take the first half of the old reserved[4] at 256
    assert _capi.Config.covariance.offset == _capi.Config.epsilon_approx.offset + 4
    assert _capi.Config.sensor_std_dev.offset == _capi.Config.covariance.offset + 4
    assert _capi.Config.reserved.offset + 2 * 4 == C.sizeof(_capi.Config)
    lib = _capi.load()
    cfg = _capi.Config()
    lib.icpmi_config_default(C.byref(cfg))
    assert cfg.covariance == 0 and cfg.sensor_std_dev == pytest.approx(0.01)


def test_yaml_name_translates_and_rejects_unknown_keys():
    from norlab_icp_mapper_amd import icp
    cfg = icp.config_from_yaml_chain({"errorMinimizer": {"PointToPlaneWithCovErrorMinimizer": {"sensorStdDev": 0.02, "force4DOF": 1}}})
    assert cfg.minimizer == 2 and cfg.covariance == 1 and cfg.force_4dof == 1 and cfg.sensor_std_dev == pytest.approx(0.02)
    cfg = icp.config_from_yaml_chain({"errorMinimizer": "PointToPlaneWithCovErrorMinimizer"})
    assert cfg.covariance == 1 and cfg.sensor_std_dev == pytest.approx(0.01)
    assert icp.config_from_yaml_chain({"errorMinimizer": "PointToPlaneErrorMinimizer"}).covariance == 0
    with pytest.raises(icp.InvalidParameter):
        icp.config_from_yaml_chain({"errorMinimizer": {"PointToPlaneWithCovErrorMinimizer": {"sensorStdDv": 0.02}}})
    with pytest.raises(icp.InvalidParameter):
        icp.config_from_yaml_chain({"errorMinimizer": "PointToPointWithCovErrorMinimizer"})
