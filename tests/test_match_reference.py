"""tests/match_reference.py (the per-query checker of the loop's matches) catches what it is meant to catch: it accepts the oracle's
answer on a small scene with duplicate points and a radius, and rejects each single-slot mutation of it -- with the oracle
comparison and on the float64 references alone.  CPU only."""
import math

import numpy as np
import pytest

import match_reference as mr

K = 4
RADIUS = 0.35


@pytest.fixture(scope="module")
def scene(oracle):
    rng = np.random.default_rng(11)
    base = rng.uniform(-2.0, 2.0, (3000, 3))
    pts = np.r_[base, base[:300], base[:100]]             # points present two and three times: ties broken by index
    m = np.ones((pts.shape[0], 4), np.float32); m[:, :3] = pts
    q = np.ones((600, 4), np.float32)
    q[:500, :3] = pts[rng.integers(0, pts.shape[0], 500)] + rng.normal(0, 0.08, (500, 3))
    q[500:550, :3] = pts[:50]                              # exact hits (d2 = 0) on duplicated points
    q[550:, :3] = rng.uniform(-3.0, 3.0, (50, 3))          # sparse surroundings: unfilled slots inside the radius
    ids, d2 = oracle.knn(m, q, k=K, max_dist=RADIUS)
    ids1, d21 = oracle.knn(m, q, k=K + 1, max_dist=RADIUS)
    return m, q, ids, d2, ids1, d21


def test_accepts_the_oracle_answer(scene):
    m, q, ids, d2, _, _ = scene
    assert (ids == -1).any() and (ids >= 0).all(1).any(), "the scene must have full and partly unfilled rows"
    mr.check_matches(m, q, ids, d2, K, RADIUS)
    mr.check_matches(m, q, ids, d2, K, RADIUS, use_oracle=False)


def test_accepts_exact_answers_without_radius(oracle, scene):
    m, q, _, _, _, _ = scene
    ids, d2 = oracle.knn(m, q, k=K, max_dist=math.inf)
    mr.check_matches(m, q, ids, d2, K, math.inf)


def test_accepts_the_epsilon_answer(oracle, scene):
    m, q, _, _, _, _ = scene
    ids, d2 = oracle.knn(m, q, k=K, max_dist=math.inf, epsilon=1.0)
    mr.check_matches(m, q, ids, d2, K, math.inf, eps=1.0)


def _mutant(scene, kind):
    m, q, ids, d2, ids1, d21 = scene
    ids, d2 = ids.copy(), d2.copy()
    full = (ids1 >= 0).all(1)
    if kind == "swap_kplus1":
        # a neighbour swapped for the (k+1)-th, where that one is clearly farther
        r = int(np.nonzero(full & (d21[:, K] > d21[:, K - 1] * 1.01))[0][0])
        ids[r, K - 1], d2[r, K - 1] = ids1[r, K], d21[r, K]
    elif kind == "drop_last":
        r = int(np.nonzero((ids >= 0).all(1))[0][0])
        ids[r, K - 1], d2[r, K - 1] = -1, np.float32(np.inf)
    elif kind == "swap_tied":
        # two equal distances (duplicate points) in the wrong index order
        tie = (d2[:, :-1] == d2[:, 1:]) & (ids[:, :-1] >= 0) & (ids[:, :-1] != ids[:, 1:])
        r, j = (int(v[0]) for v in np.nonzero(tie))
        ids[r, j], ids[r, j + 1] = ids[r, j + 1], ids[r, j]
    elif kind == "nudge_8ulp":
        r = int(np.nonzero((d2[:, 0] > 0) & np.isfinite(d2[:, 0]) & (d2[:, 1] > d2[:, 0] * 1.01))[0][0])
        v = d2[r, 0]
        for _ in range(8):
            v = np.nextafter(v, np.float32(np.inf))
        d2[r, 0] = v
    else:
        raise ValueError(kind)
    return m, q, ids, d2


# the rule of the float64 references that must catch each mutation when the oracle comparison is off
FLOAT64_RULE = {"swap_kplus1": "nearer point was missed", "drop_last": "unfilled although", "swap_tied": "ascending by",
                "nudge_8ulp": "not the float32 distance"}


@pytest.mark.parametrize("use_oracle", [True, False])
@pytest.mark.parametrize("kind", sorted(FLOAT64_RULE))
def test_rejects_each_mutation(scene, kind, use_oracle):
    m, q, ids, d2 = _mutant(scene, kind)
    with pytest.raises(AssertionError, match=None if use_oracle else FLOAT64_RULE[kind]):
        mr.check_matches(m, q, ids, d2, K, RADIUS, use_oracle=use_oracle)


def test_trimmed_quantile_matches_the_oracle(oracle):
    rng = np.random.default_rng(3)
    d2 = rng.exponential(1.0, 10007).astype(np.float32)
    d2[::17] = np.inf
    d2[::29] = 0.0                                         # exact zeros are not distances to the quantile
    for ratio in (0.85, 0.5, 0.1, 1.0):
        assert mr.trimmed_quantile(d2, ratio) == oracle.dists_quantile(d2, ratio), ratio
