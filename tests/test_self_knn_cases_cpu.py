"""The clouds of tests/self_knn_cases.py and their references, checked without a GPU: the oracle's kd-tree and its brute force agree bit for
bit on every case, the answer passes the independent float64 check (tests/match_reference.py, its bands unchanged), and every cloud still has
the property it is named for -- an edit of a generator cannot quietly take a GPU test (tests/test_gpu_self_knn.py) off its branch."""
import numpy as np
import pytest

import match_reference as mr
import self_knn_cases as sc


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("name", sc.CASES)
def test_reference_is_exact(oracle, name, k):
    c = sc.make(name)
    ids, d2 = sc.reference(name, k)
    other = sc.reference_of(c, k, brute=(name != "identical"))       # the other of the two searches
    assert np.array_equal(ids, other[0]) and np.array_equal(d2.view(np.uint32), other[1].view(np.uint32))
    mr.check_matches(c, c, ids, d2, k, np.inf, use_oracle=False, where=f"{name} k={k}")
    # row 0: the point itself, or a point of the same coordinates and a smaller index
    first = ids[:, 0]
    assert (d2[:, 0] == 0).all() and (first <= np.arange(c.shape[0])).all()
    assert np.array_equal(c[first, :3], c[:, :3])


@pytest.mark.parametrize("k", [1, 2, 10, 17, 32])
def test_tiny_references(oracle, k):
    for m in sc.tiny_sizes(k):
        c = sc.tiny(m)
        ids, d2 = sc.reference_of(c, k)
        b = sc.reference_of(c, k, brute=True)
        assert np.array_equal(ids, b[0]) and np.array_equal(d2.view(np.uint32), b[1].view(np.uint32))
        mr.check_matches(c, c, ids, d2, k, np.inf, use_oracle=False, where=f"tiny m={m} k={k}")
        assert ((ids >= 0).sum(1) == min(k, m)).all()                # unfilled slots exactly where the cloud runs out


def test_tiny_sizes_cover_the_edges():
    assert sc.tiny_sizes(1) == [1, 2] and sc.tiny_sizes(2) == [1, 2, 3] and sc.tiny_sizes(3) == [2, 3, 4]
    assert sc.tiny_sizes(32) == [31, 32, 33]


def test_every_cloud_is_float32_w1_and_finite():
    for name in sc.CASES:
        c = sc.make(name)
        assert c.dtype == np.float32 and c.shape[1] == 4 and (c[:, 3] == 1).all() and np.isfinite(c).all(), name
        assert np.array_equal(c, sc.make(name)), name            # seeded


def test_identical_has_no_extent():
    c = sc.make("identical")
    assert c.shape[0] == 3000 and (c == c[0]).all()


def test_piles_hold_the_big_pile_and_the_small_ones():
    c = sc.make("piles")
    _, inverse, counts = np.unique(c[:, :3], axis=0, return_inverse=True, return_counts=True)
    assert sorted(set(counts.tolist())) == [sc.PILE_COPIES, sc.BIG_PILE] and (counts == sc.BIG_PILE).sum() == 1
    assert sc.BIG_PILE > 256                                         # more than the cell kernel's candidate registers (64 x SG_R)
    assert counts.size == sc.PILE_SITES + 1
    # the copies of a site are scattered through the cloud: the index, not the position, orders them
    big = np.nonzero(counts[np.asarray(inverse).ravel()] == sc.BIG_PILE)[0]
    assert big.max() - big.min() > sc.BIG_PILE


def test_line_and_plane_have_exact_zero_axes():
    c = sc.make("line")
    assert c.shape[0] == 4000 and (c[:, 1] == 0).all() and (c[:, 2] == 0).all() and np.ptp(c[:, 0]) > 90
    p = sc.make("plane_z0")
    assert (p[:, 2] == 0).all() and np.ptp(p[:, 0]) > 19 and np.ptp(p[:, 1]) > 19


def test_lattice_is_exact_in_float32():
    c = sc.make("lattice")
    assert c.shape[0] == 16 ** 3
    q = c[:, :3].astype(np.float64) / 0.25
    assert np.array_equal(q, np.round(q)) and q.min() == 0 and q.max() == 15
    assert np.unique(q, axis=0).shape[0] == 16 ** 3
    _, d2 = sc.reference("lattice", 10)
    assert (d2[:, 1] == np.float32(0.0625)).all()                    # massive ties: every nearest neighbour at the spacing, exactly
    assert ((d2[:, 1:] == d2[:, :1] + np.float32(0.0625)).sum(1) >= 3).all()   # a corner has 3 of them, an interior point 6


def test_clump_far_has_both_scales():
    c = sc.make("clump_far")
    r = np.linalg.norm(c[:, :3].astype(np.float64), axis=1)
    far = r > 1.0
    assert far.sum() == 40 and (~far).sum() == 6000
    assert r[far].min() > 2000 and r[far].max() < 10001 and r[~far].max() < 0.5
    # the box is kilometres wide, the clump's neighbours millimetres apart: no cell edge serves both within 2^24 blocks
    _, d2 = sc.reference("clump_far", 10)
    assert np.median(np.sqrt(d2[~far, 9])) < 0.05 and np.ptp(c[:, 0]) > 2000


def test_heavy_has_a_heavy_tail():
    c = sc.make("heavy")
    _, d2 = sc.reference("heavy", 10)
    kth = np.sqrt(d2[:, 9].astype(np.float64))
    assert c.shape[0] == 12000 and np.quantile(kth, 0.999) > 100 * np.median(kth)


def test_offset_sits_far_from_the_origin():
    c = sc.make("offset")
    lo, hi = c[:, :3].min(0), c[:, :3].max(0)
    centre = np.array(sc.OFFSET_CENTRE)
    assert c.shape[0] == 8000 and (np.abs((lo + hi) / 2 - centre) < 0.1).all()
    assert (hi - lo <= np.array([16.01, 16.01, 1.61])).all() and (hi - lo >= np.array([15.9, 15.9, 1.55])).all()
    # the coordinates round at 2^-8 m (x) while neighbours are decimetres apart: the grid's slack maxabs * 2e-6 = 0.08 m matters
    assert np.spacing(np.float32(40000.0)) == np.float32(2.0 ** -8)


def test_two_clusters_are_apart():
    c = sc.make("two_clusters")
    left = c[:, 0] < 250
    assert left.sum() == 2000 and (~left).sum() == 2000
    assert c[left, 0].max() < 1 and c[~left, 0].min() > 499
    ids, _ = sc.reference("two_clusters", 32)
    assert (left[ids] == left[:, None]).all()                        # no neighbourhood crosses the gap


@pytest.mark.parametrize("cell", [0.0625, 0.1, 0.25, 0.3137])
def test_margin_gadgets_sit_on_the_margin(oracle, cell):
    """whatever edge the handle's tuner settles on: a good share of the gadgets defeat a margin without slack, and in each of those the exact
    second neighbour of q is p (outside the block), not L (inside it)"""
    c, fired, edge = sc.margin_gadgets(cell)
    assert c.shape[0] == sc.MARGIN_M == sc.margin_warmup().shape[0] and edge == np.float32(cell)
    assert fired >= 20 and (c[:, 1:3] == 0).all()
    ids, d2 = sc.reference_of(c, 2)
    b = sc.reference_of(c, 2, brute=True)
    assert np.array_equal(ids, b[0]) and np.array_equal(d2.view(np.uint32), b[1].view(np.uint32))
    mr.check_matches(c, c, ids, d2, 2, np.inf, use_oracle=False, where=f"margin gadgets, edge {cell}")
    q = 1 + 3 * np.arange((c.shape[0] - 2) // 3)
    assert (ids[q, 1] == q + 1).all()
    left = c[q, 0] - c[q + 2, 0]; right = c[q + 1, 0] - c[q, 0]
    q9 = 2.0 ** -9                                                   # p about one to two cells to the right, L no nearer than p
    assert (left >= right).all() and (right > cell - 4 * q9).all() and (left < 2.0 * cell + 8 * q9).all()
