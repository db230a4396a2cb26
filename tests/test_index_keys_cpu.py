"""tests/index_key_cases.py on the CPU: the generator finds points whose level-0 cell depends on the centroid at every cell size, a flip is
never more than one cell (what a search of the neighbouring cells rests on), equal centroids flip nothing, and points that overhang the box
clamp to the same border cell under both centroids (map_insert's overhang rule)."""
import numpy as np
import pytest

import index_key_cases as K

F = np.float32
CELLS = (0.1933, 0.25, 0.2871, 0.37, 0.61, 1.07)
LO = np.array([-7.3127, 2.4411, -0.8312], dtype=F)     # a box of about 20 x 12 x 3 m, nowhere near round numbers
HI = LO + np.array([20.137, 12.049, 3.017], dtype=F)
MEAN = (LO.astype(np.float64) + HI.astype(np.float64)) / 2 + np.array([0.713, -0.291, 0.118])
SHIFTS = (1e-3, 1e-1)


def case(cell, shift, seed=0, **kw):
    mean_a = MEAN.astype(F)
    mean_b = (MEAN + shift * np.array([1.0, -0.6, 0.35]) / np.linalg.norm([1.0, -0.6, 0.35])).astype(F)
    dims = K.grid_dims(LO, HI, cell, mean_a)
    pts, flips, comp = K.wall_points(LO, HI, F(cell), dims, mean_a, mean_b, np.random.default_rng(seed), **kw)
    return mean_a, mean_b, dims, pts, flips, comp


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("cell", CELLS)
def test_generator_finds_flips_and_they_are_one_cell(cell, shift):
    mean_a, mean_b, dims, pts, flips, comp = case(cell, shift)
    assert dims == K.grid_dims(LO, HI, cell, mean_b)          # the insert's own condition: same grid under both centroids
    print(f"cell {cell}: {int(flips.sum())} predicted flips of {pts.shape[0]} points, dims {dims}")
    assert flips.sum() >= 32
    assert flips.all()                                         # the generator keeps nothing else
    ca, cb = K.cells(pts, mean_a, LO, F(cell), dims), K.cells(pts, mean_b, LO, F(cell), dims)
    assert np.abs(ca - cb).max() == 1
    assert (pts[:, :3] >= LO).all() and (pts[:, :3] <= HI).all()
    # the companions: three per point, 1 to 3 cm away, not collinear with it
    d = comp[:, :3].reshape(-1, 3, 3).astype(np.float64) - pts[:, None, :3].astype(np.float64)
    r = np.linalg.norm(d, axis=2)
    assert comp.shape[0] == 3 * pts.shape[0] and (r > 0.0099).all() and (r < 0.0301).all()
    assert (np.abs(np.linalg.det(d)) > 0).all()


@pytest.mark.parametrize("cell", CELLS)
def test_no_point_of_a_dense_cloud_moves_by_more_than_one_cell(cell):
    """not only the constructed points: a million uniform ones, and every float32 neighbour of every wall"""
    rng = np.random.default_rng(3)
    pts = rng.uniform(LO, HI, size=(1_000_000, 3)).astype(F)
    for shift in SHIFTS + (1e-2, 1.0):
        mean_a = MEAN.astype(F)
        mean_b = (MEAN - shift).astype(F)
        dims = K.grid_dims(LO, HI, cell, mean_a)
        d = np.abs(K.cells(pts, mean_a, LO, F(cell), dims) - K.cells(pts, mean_b, LO, F(cell), dims))
        assert d.max() <= 1


@pytest.mark.parametrize("cell", CELLS)
def test_equal_centroids_flip_nothing(cell):
    mean_a, _, dims, pts, flips, _ = case(cell, 1e-3)
    assert not K.flip_mask(pts, LO, F(cell), dims, mean_a, mean_a.copy()).any()
    _, flips0, _ = K.wall_points(LO, HI, F(cell), dims, mean_a, mean_a.copy(), np.random.default_rng(0))
    assert flips0.size == 0


@pytest.mark.parametrize("cell", CELLS)
def test_overhanging_points_clamp_to_the_same_border_cell(cell):
    """map_insert takes a delta that overhangs the box by up to two cells: cell_of clamps it into the border cells, under any centroid"""
    rng = np.random.default_rng(5)
    n = 20000
    for shift in SHIFTS:
        mean_a, mean_b, dims, *_ = case(cell, shift)
        for a in range(3):
            over = rng.uniform(1e-6, 2.0 * cell, n)
            below = (LO[a].astype(np.float64) - over).astype(F)
            above = (HI[a].astype(np.float64) + over).astype(F)
            below, above = below[below < LO[a]], above[above > HI[a]]
            for m in (mean_a, mean_b):
                assert (K.cell_1d(below, m[a], LO[a], F(cell), dims[a]) == 0).all()
                assert (K.cell_1d(above, m[a], LO[a], F(cell), dims[a]) == dims[a] - 1).all()


def test_planar_box_has_walls_on_x_and_y_only():
    lo, hi = LO.copy(), HI.copy()
    lo[2] = hi[2] = 0
    mean_a = np.array([MEAN[0], MEAN[1], 0.0]).astype(F)
    mean_b = (mean_a.astype(np.float64) + np.array([1e-3, -7e-4, 0.0])).astype(F)
    dims = K.grid_dims(lo, hi, 0.25, mean_a)
    assert dims[2] == 1
    pts, flips, comp = K.wall_points(lo, hi, F(0.25), dims, mean_a, mean_b, np.random.default_rng(1))
    assert flips.sum() >= 32 and flips.all()
    assert (pts[:, 2] == 0).all() and (comp[:, 2] == 0).all()


def test_ballast_sets_the_centroid_to_the_bit():
    rng = np.random.default_rng(2)
    base = np.ones((20000, 4), dtype=F)
    base[:, :3] = rng.uniform(LO, HI, size=(20000, 3))
    other = np.ones((700, 4), dtype=F)
    other[:, :3] = rng.uniform(LO, HI, size=(700, 3))
    for shift in (0.0, 1e-3, -2e-3):
        target = (K.predicted_mean([base]).astype(np.float64) + shift).astype(F)
        b = K.ballast(300, LO + 1, HI - 1, [base], [other], target, rng)
        assert np.array_equal(K.predicted_mean([base, other, b]).view(np.uint32), target.view(np.uint32))
        assert (b[:, :3] > LO).all() and (b[:, :3] < HI).all()
