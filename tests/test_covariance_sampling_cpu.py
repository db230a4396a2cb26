"""CovarianceSamplingDataPointsFilter: the numpy restatement (tests/covariance_sampling_reference.py) on cases worked out by hand,
its tie order, and what the sampler is for -- on a corridor, the few points that pin the corridor axis are taken early, and the
sample constrains the weakest direction better than a random subset of the same size.  No GPU."""
import numpy as np
import pytest

import covariance_sampling_reference as csr

F = np.float32


def _c4(xyz):
    xyz = np.asarray(xyz, F)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


# Eight points with mean 0 and axis-aligned normals; torqueNorm 0 (L = 1).  v = [p x n ; n]:
#   0 (0, 0, 0)    n x  v = (0,    0,    0,   1, 0, 0)
#   1 (1.5, 0, 0)  n y  v = (0,    0,    1.5, 0, 1, 0)
#   2 (-1.5, 0, 0) n y  v = (0,    0,   -1.5, 0, 1, 0)
#   3 (0, 2.5, 0)  n z  v = (2.5,  0,    0,   0, 0, 1)
#   4 (0, -2.5, 0) n z  v = (-2.5, 0,    0,   0, 0, 1)
#   5 (0, 0, 0)    n z  v = (0,    0,    0,   0, 0, 1)
#   6 (2, 0, 0)    n z  v = (0,   -2,    0,   0, 0, 1)
#   7 (-2, 0, 0)   n z  v = (0,    2,    0,   0, 0, 1)
# C = diag(12.5, 8, 4.5, 1, 2, 5): ascending x_0 .. x_5 = e3, e4, e2, e5, e1, e0.  Weights (v . x_k)^2 per point:
#   0: (1,0,0,0,0,0)  1, 2: (0,1,2.25,0,0,0)  3, 4: (0,0,0,1,0,6.25)  5: (0,0,0,1,0,0)  6, 7: (0,0,0,1,4,0)
# Lists: L0 = 0 | 1..7, L1 = 1 2 | 0 3 4 5 6 7, L2 = 1 2 | ..., L3 = 3 4 5 6 7 | 0 1 2, L4 = 6 7 | 0..5, L5 = 3 4 | 0 1 2 5 6 7.
# Picks: t = 0 -> L0: 0; t = (1,0,0,0,0,0) -> L1: 1; t3 = 0 first -> L3: 3; t4 = 0 -> L4: 6; t = (1,1,2.25,2,4,6.25) -> L0 skips 0, 1:
# 2; t0 = 1 still smallest -> L0 skips 3: 4; -> L0: 5.
HAND_XYZ = [[0, 0, 0], [1.5, 0, 0], [-1.5, 0, 0], [0, 2.5, 0], [0, -2.5, 0], [0, 0, 0], [2, 0, 0], [-2, 0, 0]]
HAND_NRM = [[1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]]
HAND_PICKS = [0, 1, 3, 6, 2, 4, 5]


def test_hand_computed_case():
    xyz = _c4(HAND_XYZ)
    order, info = csr.covariance_sampling(xyz, np.asarray(HAND_NRM, F), 7, torque_norm=0)
    assert order.tolist() == HAND_PICKS
    assert np.allclose(info["eigval"], [1, 2, 4.5, 5, 8, 12.5])
    assert info["lnorm"] == 1.0 and np.array_equal(info["center"], [0, 0, 0])
    for nb in range(8):
        assert csr.covariance_sampling(xyz, np.asarray(HAND_NRM, F), nb, torque_norm=0)[0].tolist() == HAND_PICKS[:nb]


def test_identity_when_nb_sample_covers_the_cloud_even_without_normals():
    xyz = _c4(np.random.default_rng(1).normal(size=(50, 3)))
    for nb in (50, 51, 10_000):
        order, info = csr.covariance_sampling(xyz, None, nb)
        assert order.tolist() == list(range(50)) and info is None
    with pytest.raises(KeyError):
        csr.covariance_sampling(xyz, None, 49)


def test_torque_norms():
    xyz = _c4([[0, 0, 0], [4, 0, 0], [0, 2, 0], [0, 0, 1]])
    c, L = csr.center_and_lnorm(xyz, 0)
    assert np.array_equal(c, [1.0, 0.5, 0.25]) and L == 1.0
    _, L = csr.center_and_lnorm(xyz, 2)
    assert L == 2.0                                                          # half of the x extent 4
    _, L = csr.center_and_lnorm(xyz, 1)
    a = np.asarray(xyz[:, :3], np.float64) - c
    assert L == pytest.approx(np.linalg.norm(a, axis=1).mean(), rel=1e-15)
    same = _c4(np.ones((5, 3)))
    for tn in (0, 1, 2):
        assert csr.center_and_lnorm(same, tn)[1] == 1.0                      # L == 0 -> 1


def test_ties_keep_ascending_index_order():
    rng = np.random.default_rng(2)
    xyz = rng.normal(size=(40, 3)).astype(F)
    nrm = rng.normal(size=(40, 3)).astype(F)
    xyz2, nrm2 = np.concatenate([xyz, xyz]), np.concatenate([nrm, nrm])     # point i and i + 40 give equal keys
    c, L = csr.center_and_lnorm(_c4(xyz2), 1)
    v = csr.vectors(xyz2, nrm2, c, L)
    _, X = csr.eigenbasis(csr.covariance(v))
    m = csr.projections(v, X)
    for lk in csr.sorted_lists(m):
        pos = np.empty(80, int)
        pos[lk] = np.arange(80)
        assert (pos[:40] + 1 == pos[40:]).all()                              # the twin follows right behind
    key = np.abs(m).astype(F)
    key[:] = 1.0                                                             # every key equal: the lists are the index order
    assert all(lk.tolist() == list(range(80)) for lk in csr.sorted_lists(key))
    order = csr.greedy(csr.sorted_lists(m), m * m, 79)
    first = {}
    for r, i in enumerate(order.tolist()):
        first.setdefault(i % 40, (r, i))
    assert all(i < 40 for _, i in first.values())                           # of two twins, the lower index is picked first


def corridor(n_wall=6000, n_floor=4000, seed=3):
    """two walls (y = +-1.5, normals facing in) and a floor (z = 0) along x in [-20, 20]; four small bumps on the walls whose faces
    (normals +-x) are the only constraint along the corridor.  -> (xyz, normals, bump mask)"""
    rng = np.random.default_rng(seed)
    pts, nrm, bump = [], [], []
    for side in (-1.0, 1.0):
        x = rng.uniform(-20, 20, n_wall); z = rng.uniform(0, 3, n_wall)
        pts.append(np.stack([x, np.full(n_wall, side * 1.5), z], 1)); nrm.append(np.tile([0, -side, 0], (n_wall, 1)))
    x = rng.uniform(-20, 20, n_floor); y = rng.uniform(-1.5, 1.5, n_floor)
    pts.append(np.stack([x, y, np.zeros(n_floor)], 1)); nrm.append(np.tile([0, 0, 1], (n_floor, 1)))
    bump.append(np.zeros(2 * n_wall + n_floor, bool))
    for bx, side in ((-12.0, -1.0), (-3.0, 1.0), (5.0, -1.0), (14.0, 1.0)):
        for face in (-1.0, 1.0):
            k = 5
            y = side * rng.uniform(1.3, 1.5, k); z = rng.uniform(0.5, 1.0, k)
            pts.append(np.stack([np.full(k, bx + face * 0.1), y, z], 1)); nrm.append(np.tile([face, 0, 0], (k, 1)))
            bump.append(np.ones(k, bool))
    return np.concatenate(pts).astype(F), np.concatenate(nrm).astype(F), np.concatenate(bump)


def _lambda_min(xyz, nrm, c, L):
    return np.linalg.eigvalsh(csr.covariance(csr.vectors(xyz, nrm, c, L)))[0]


def test_corridor_keeps_the_points_that_pin_the_corridor_axis():
    xyz, nrm, bump = corridor()
    nb = 300
    order, info = csr.covariance_sampling(_c4(xyz), nrm, nb, torque_norm=1)
    assert len(set(order.tolist())) == nb
    # x_0, the least constrained direction, is the translation along the corridor: the first pick is a bump point, and the sample
    # holds several of the 40 bump points among 16 040 (a random subset of 300: 0.75 on average)
    assert abs(info["basis"][3, 0]) > 0.99
    assert bump[order[0]]
    assert bump[order].sum() >= 5
    c, L = info["center"], info["lnorm"]
    ours = _lambda_min(xyz[order], nrm[order], c, L)
    rng = np.random.default_rng(4)
    rand = [_lambda_min(xyz[r], nrm[r], c, L) for r in (rng.choice(xyz.shape[0], nb, replace=False) for _ in range(10))]
    assert ours > 1.5 * max(rand), (ours, rand)
