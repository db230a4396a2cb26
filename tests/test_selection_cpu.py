"""CPU half of the selection-edge tests: every distance set of tests/selection_cases.py has the property it claims, and the integer-exact
numpy reference (tests/selection_reference.py) equals the oracle's OutlierFilters::compute on it -- limit bitwise, weights exactly -- for
TrimmedDist at the case's ratio and at 1.0, MedianDist{3}, the two-quantile chain and MaxDist + TrimmedDist of the GPU test, and, where the
GPU test runs it, VarTrimmedDist.  The float_rank cases prove that the float32 product decides the rank in the oracle too, and that
match_reference.trimmed_quantile -- the reference of the older loop tests -- follows the same rule.

The geometry of the loop cases is checked here as well: the oracle's kd-tree over the lattice map returns distances with the case's
property, so the GPU test starts from a reading that is known to carry its edge."""
import numpy as np
import pytest

import match_reference as mr
import selection_cases as sc
import selection_reference as sr

VT_CHAINS = [[(sr.VARTRIMMED, 0.05, 0, 0.99, 0.95)], [(sr.VARTRIMMED, 0.6, 0, 0.6, 0.95)]]


def chains_of(c, d2):
    """the chains the GPU test runs on an array case (x of the MaxDist filter: the square root of the median, so that it cuts)"""
    x = float(np.sqrt(np.float64(sr.quantile(d2, 0.5)))) if not c.invalid else 1.0
    return [[(sr.TRIMMED, c.ratio)], [(sr.TRIMMED, 1.0)], [(sr.MEDIAN, 3.0)], [(sr.TRIMMED, 0.9), (sr.MEDIAN, 2.5)], [(sr.MAXDIST, x), (sr.TRIMMED, c.ratio)]]


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def test_case_lists_cover_what_they_name():
    ids = set(sc.ARRAY_IDS)
    for size in sc.SIZES: assert f"size-{size}" in ids
    assert {"all_equal", "wide-shuffled", "wide-ascending", "tiny", "mostly_invalid", "all_inf", "all_zero", "float_rank-0.7-10"} <= ids
    picks = sc.float_rank_picks()
    assert len(picks) >= 6 and all(sc.rank32(t, q) == sc.rank_exact(t, q) + 1 for q, t in picks)
    assert sc.rank32(10, 0.7) == 7 and sc.rank_exact(10, 0.7) == 6
    assert len(set(sc.LOOP_IDS)) == len(sc.LOOP_IDS) and len(ids) == len(sc.ARRAY_IDS)


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("cid", sc.ARRAY_IDS)
def test_reference_equals_oracle(oracle, cid, k):
    c = sc.array_case(cid)
    d2 = c.make(k)
    assert d2.shape[1] == k and d2.dtype == np.float32
    c.check(d2)
    ids = np.zeros(d2.shape, np.int32)
    for chain in chains_of(c, d2) + (VT_CHAINS if c.vt else []):
        err, w, lim = oracle.outlier_weights(oracle.make_config(outliers=chain), d2, ids)
        if c.invalid:
            assert err == sr.ORACLE_NO_OUTLIER_TO_FILTER, (cid, chain, err)
            with pytest.raises(sr.NoValidDistance):
                sr.chain(chain, d2)
            continue
        assert err == 0, (cid, chain, err)
        rw, rlim = sr.chain(chain, d2)
        assert same_bits(lim, rlim), (cid, k, chain, float(lim), float(rlim))
        assert np.array_equal(w, rw), (cid, k, chain)
    if not c.invalid:
        for q in (c.ratio, 1.0, 0.5):
            assert same_bits(mr.trimmed_quantile(d2, q), sr.quantile(d2, q)), (cid, q)
            assert same_bits(oracle.dists_quantile(d2, q), sr.quantile(d2, q)), (cid, q)


@pytest.mark.parametrize("cid", [c.id for c in sc.ARRAYS if c.id.startswith("float_rank")])
def test_float_rank_cases_tell_the_two_ranks_apart(oracle, cid):
    """the element at the exact-arithmetic rank has other bits: an implementation with a double product would be caught"""
    c = sc.array_case(cid)
    d2 = c.make(1)
    s = sr.sorted_bits(d2)
    r32, rex = sc.rank32(s.size, c.ratio), sc.rank_exact(s.size, c.ratio)
    assert r32 == rex + 1 and s[r32] != s[rex]
    assert np.float32(oracle.dists_quantile(d2, c.ratio)).view(np.uint32) == s[r32]


def test_lattice_map_is_symmetric():
    for k in (1, 6, 16):
        mp, nm = sc.lattice_map(k)
        assert mp.shape == (75 * k, 4) and nm.shape == (75 * k, 3)
        assert (mp[:, :3].astype(np.float64).sum(0) == 0).all()
        pts = {tuple(p) for p in mp[:, :3].tolist()}
        assert all(tuple(-np.array(p)) in pts for p in pts) and len(pts) == 75
        d = np.array(sorted(pts))
        gap = np.sqrt(((d[:, None, :] - d[None, :, :]) ** 2).sum(-1))
        assert gap[gap > 0].min() >= 8.0
        assert (np.abs(nm).sum(1) == 1).all() and len({tuple(r) for r in nm.tolist()}) == 3


@pytest.mark.parametrize("cid", sc.LOOP_IDS)
def test_loop_geometry_carries_the_property(oracle, cid):
    c = sc.loop_case(cid)
    for k in c.ks:
        mp, _ = sc.lattice_map(k)
        rd = c.reading(k)        # (as built: the misaligned cases state nothing about their first distances beyond having matches)
        _, d2 = oracle.knn(mp, rd, k=k, max_dist=sc.MAX_DIST, nthreads=8)
        c.check(d2, c.ratio(k), True)
        assert (d2 == d2[:, :1])[np.isfinite(d2[:, 0])].all()      # k coincident map points: one value per query


def test_count_edge_readings():
    for n, count in ((65_537, 1 << 20), (131_073, 1 << 21)):
        rd = sc.count_edge_reading(n)
        assert rd.shape[0] * 16 > count >= (rd.shape[0] - 1) * 16
        d2 = (rd[:, :3].astype(np.float64) ** 2).sum(1)
        near = d2 < 1e-6          # the low end sits at the central anchor, in index order
        assert near[: near.sum()].all() and near.sum() > n // 2 and (np.diff(d2[near]) >= 0).all()
