"""Clouds built to reach the branches of the self k-NN grid (csrc/selfgrid.hip) that well-behaved scenes never take, and their exact
references (CPU only: seeded numpy generators and the oracle's searches; nothing here imports the GPU package).

Every cloud is float32 (m, 4) with w = 1 and as small as its branch allows:
  identical     3,000 copies of one point: extent 0, a 1 x 1 x 1 grid, a neighbourhood of 3,000 candidates
  piles         400 sites 5 times each + one site 300 times: more than 256 candidates around one cell (`big` mode, the per-query
                refetch behind the candidate registers), every rank decided by the index
  line          4,000 points on the x axis: two axes of the Morton table without bits
  plane_z0      a z = 0 sheet searched by a 3-D handle: one axis without bits
  lattice       16^3 points, spacing 0.25: equal d2 everywhere, queries on the border of the box
  clump_far     6,000 points within centimetres + 40 points 2 - 10 km out: the cap of the block table, huge cells, levels above 2
  heavy         12,000 points with Pareto(1.5) radii: the level kernel's phase A climbing several levels
  offset        8,000 points in a 16 x 16 x 1.6 m slab 47 km from the origin: the rounding slack of far coordinates
  two_clusters  2 x 2,000 points 500 m apart: empty blocks in between
  tiny(m)       m points: the 3 x 3 x 3 block is the whole grid, rows with unfilled slots
"""
import functools

import numpy as np

CASES = ("identical", "piles", "line", "plane_z0", "lattice", "clump_far", "heavy", "offset", "two_clusters")
KS = (1, 2, 10, 11, 16, 17, 32)          # 10 | 11 and 16 | 17: the register variants of the normals kernel; 32 = ICPMI_MAX_K
PILE_SITES, PILE_COPIES, BIG_PILE = 400, 5, 300
OFFSET_CENTRE = (40000.0, -25000.0, 300.0)


def cloud(xyz):
    c = np.ones((xyz.shape[0], 4), dtype=np.float32)
    c[:, :3] = np.asarray(xyz).astype(np.float32)
    return c


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def heavy_xyz(rng, n, scale):
    """the heavy-tailed cloud of test_gpu_incremental_normals: Pareto(1.5) radii, flattened in z"""
    return _unit(rng, n) * (scale * rng.pareto(1.5, size=(n, 1))) * np.array([1.0, 1.0, 0.15])


@functools.lru_cache(maxsize=None)
def _make(name):
    rng = np.random.default_rng({n: 100 + i for i, n in enumerate(CASES)}[name])
    if name == "identical":
        return cloud(np.tile(np.array([[1.5, -2.25, 0.75]]), (3000, 1)))
    if name == "piles":
        sites = rng.uniform(-5.0, 5.0, (PILE_SITES + 1, 3)).astype(np.float32)
        xyz = np.concatenate([np.repeat(sites[:PILE_SITES], PILE_COPIES, axis=0), np.repeat(sites[PILE_SITES:], BIG_PILE, axis=0)])
        return cloud(xyz[rng.permutation(xyz.shape[0])])
    if name == "line":
        return cloud(np.c_[rng.uniform(0.0, 100.0, 4000), np.zeros(4000), np.zeros(4000)])
    if name == "plane_z0":
        return cloud(np.c_[rng.uniform(0.0, 20.0, (5000, 2)), np.zeros(5000)])
    if name == "lattice":
        g = np.arange(16) * 0.25
        xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return cloud(xyz[rng.permutation(xyz.shape[0])])
    if name == "clump_far":
        far = _unit(rng, 40) * rng.uniform(2000.0, 10000.0, (40, 1))
        xyz = np.concatenate([rng.normal(0.0, 0.05, (6000, 3)), far])
        return cloud(xyz[rng.permutation(xyz.shape[0])])
    if name == "heavy":
        return cloud(heavy_xyz(rng, 12000, 2.0))
    if name == "offset":
        return cloud(np.array(OFFSET_CENTRE) + rng.uniform(-0.5, 0.5, (8000, 3)) * np.array([16.0, 16.0, 1.6]))
    if name == "two_clusters":
        xyz = np.concatenate([rng.normal(0.0, 0.1, (2000, 3)), rng.normal(0.0, 0.1, (2000, 3)) + np.array([500.0, 0.0, 0.0])])
        return cloud(xyz[rng.permutation(xyz.shape[0])])
    raise KeyError(name)


def make(name):
    """the cloud of a case (a fresh copy: callers may not disturb the cached one)"""
    return _make(name).copy()


def tiny(m, seed=7):
    return cloud(np.random.default_rng(seed + m).uniform(-1.0, 1.0, (m, 3)))


def tiny_sizes(k):
    """m = 1, 2, k - 1, k, k + 1, limited to 1 <= m and k <= m + 1"""
    return sorted({m for m in (1, 2, k - 1, k, k + 1) if m >= 1 and k <= m + 1})


def scaled(c, s):
    """the cloud scaled about the origin, rounded to float32 once"""
    out = c.copy()
    out[:, :3] = (c[:, :3].astype(np.float64) * s).astype(np.float32)
    return out


MARGIN_M = 1202      # points of margin_gadgets() with its default count; margin_warmup() has as many, so that the tuner takes the previous edge


def margin_warmup():
    """a dense line whose tuned cell edge is decimetres: searched (repeatedly) before margin_gadgets() on the same handle, it pins the edge"""
    x = np.random.default_rng(31).uniform(0.0, 200.0, MARGIN_M)
    return cloud(np.c_[x, np.zeros(MARGIN_M), np.zeros(MARGIN_M)])


def margin_gadgets(cell, gadgets=400, seed=11):
    """Points ON the margin of the cell kernel's decision, for a grid whose A-cell edge is `cell` (float32, as the handle's previous build left
    it): the rounding slack of sg_margin2 is what keeps these queries exact.

    A line (y = z = 0: those axes never bound the margin) from -20000.5 to 20001, so that (x - origin) near x = 16400 is rounded to 2^-8 m while
    the coordinates themselves step by 2^-9 m: a point's cell follows the ROUNDED difference.  Every gadget is three points 16 cells from the
    next: a query q; p, the nearest point to its right that the grid puts two cells over (outside q's 3 x 3 x 3 block); L to its left inside the
    block, at the largest distance D the margin computed WITHOUT slack -- min(1 + fr, 2 - fr) x cell, in the kernel's float32 steps -- still
    accepts.  Where D >= |p - q| (`fired`) a search that trusts that margin answers L, the exact answer is p (nearer, or as near with the
    smaller index).  Returns (cloud, number of fired gadgets, the edge the grid will have)."""
    f = np.float32
    q9 = 2.0 ** -9
    lo, hi = f(-20000.5), f(20001.0)
    cell_b = f(max(float(f(cell)), (float(hi) - float(lo)) * 1e-6, 1e-6))          # (the grid's lower bound on the edge: extent x 1e-6)
    assert 0.05 < cell_b < 1.0, cell_b
    inv = f(1.0) / cell_b
    na = int(np.floor((hi - lo) * inv)) + 1
    coord = lambda v: (v - lo) * inv                                                # float32 steps, as sg_cell_of takes them
    cell_of = lambda v: np.clip(np.floor(coord(v)).astype(np.int64), 0, na - 1)
    rng = np.random.default_rng(seed)
    step = np.ceil(16.0 * float(cell_b) / q9) * q9
    jmax = int(4.0 * float(cell_b) / q9) + 2
    q = (16400.0 + np.arange(gadgets) * step + rng.integers(0, jmax // 2, gadgets) * q9).astype(f)
    assert float(q.max()) + step < 32000.0 and np.array_equal(q.astype(np.float64) / q9, np.round(q.astype(np.float64) / q9))
    t = coord(q)
    a = np.floor(t)
    fr = np.clip(t - a, f(0), f(1))
    assert a.min() >= 2 and a.max() + 2 <= na - 1                                  # cells on both sides: both margins count
    mn = np.minimum((f(1.0) + fr) * cell_b, (f(2.0) - fr) * cell_b)
    m2 = mn * mn
    dist = (np.arange(1, jmax + 1) * q9).astype(f)                                 # candidate distances, exact in float32
    outside = cell_of(q[:, None] + dist[None, :]) >= a.astype(np.int64)[:, None] + 2
    accepted = (dist * dist)[None, :] <= m2[:, None]
    assert outside.any(1).all() and accepted.any(1).all()
    j = outside.argmax(1)                                                           # p = q + dist[j]
    i = accepted.shape[1] - 1 - accepted[:, ::-1].argmax(1)                         # D = dist[i]
    left_ok = cell_of(q - dist[i]) >= a.astype(np.int64) - 1
    fired = (i >= j) & left_ok
    d_left = np.where(fired, dist[i], dist[np.minimum(j + 3, jmax - 1)])
    x = np.stack([q, q + dist[j], q - d_left], axis=1).ravel()                      # q, p, L: p before L (a tie goes to p)
    x = np.concatenate([[lo], x, [hi]])
    c = cloud(np.c_[x.astype(np.float64), np.zeros(x.size), np.zeros(x.size)])
    assert c.shape[0] == 3 * gadgets + 2 and np.array_equal(c[:, 0], x.astype(f))
    return c, int(fired.sum()), float(cell_b)


_refs = {}


def reference_of(c, k, brute=False):
    """the oracle's exact self k-NN of a cloud: (ids (m, k) int32, d2 (m, k) float32), the point itself included, ascending by (d2, index),
    unfilled slots -1 / +inf"""
    import oracle_bindings as ob
    return ob.knn(c, c, k=k, allow_self=True, nthreads=16, brute=brute)


def reference(name, k):
    """reference_of(make(name), k), computed once and shared (read-only).  `identical`: brute force (the kd-tree cannot split 3,000 equal
    points and walks one bucket of them per query)"""
    key = (name, k)
    if key not in _refs:
        ids, d2 = reference_of(_make(name), k, brute=(name == "identical"))
        ids.setflags(write=False); d2.setflags(write=False)
        _refs[key] = (ids, d2)
    return _refs[key]
