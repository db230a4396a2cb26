"""The normals INSIDE the registration index after append-only updates (csrc/map_build.hip: map_insert, map_patch_normals): the incremental
SurfaceNormal pass recomputes a few normals per update and patch_normals_kernel rewrites their copies in the index -- d_normals_sorted, which
the k = 1 pair sums, the covariance and the voxel tables read, and the interleaved d_map_pn of the k > 1 pair sums.  It finds a point's copy
through the point's level-0 cell, recomputed under the CURRENT centroid, while the index keeps the cell the point got under the centroid of
its own insert: for a point on a cell wall the two differ (tests/index_key_cases.py restates the arithmetic and builds such points).

Flow on one handle (minimizer 2, normals_knn 10, min_dist 0: every point is appended):
  setMap(room) -> A: a plain delta (the first normals pass covers the whole map) -> B: the wall points, inserted under mean_B
  -> C: companions 1 - 3 cm from every wall point, which change its normal, under mean_C: the patch must find the wall points again.
The centroids are CHOSEN (index_key_cases.ballast trims every delta onto the sum it must have), predicted in numpy and compared with
getMapMean() to the bit, so the flips are known beforehand; they are then recomputed from the device's own centroids and grid.

After every update: icpmi_debug_index_normals equals getMap's normals bit for bit, in both copies, and icpmi_debug_counters[23] (normals
the patch could not place) is 0.  After C a point-to-plane registration and getResidualError of a reading cut from the wall points equal
those of a fresh handle built from the downloaded map, bit for bit.

Not covered: a handle that indexes raw coordinates (centroid 0) -- only the private handles of the map-side operators do, they carry no
normals and no front end creates one."""
import numpy as np
import pytest

import index_key_cases as K

pytestmark = pytest.mark.gpu

F = np.float32
KNN = 10
CFG = dict(minimizer=2, max_dist=1.0, outliers=[(4, 0.85)], max_iterations=10)
INSERTS, REBUILDS, SUBSET, WHOLE, UNPLACED = 18, 19, 20, 21, 23   # icpmi_debug_counters
T_B = np.array([4e-4, -3e-4, 2e-4])       # centroid of update B = centroid after A + this
T_STEP = np.array([1e-3, -8e-4, 5e-4])    # every later update moves it on by this


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def cloud(xyz):
    c = np.ones((xyz.shape[0], 4), dtype=F)
    c[:, :3] = xyz
    return c


def room(rng, n=20000, planar=False):
    """a slab-like room of about 20 x 12 x 3 m (floor, ceiling, four walls, 5 mm of noise) with its analytic normals; planar: its outline in
    z = 0 and two partitions"""
    org = np.array([-7.3127, 2.4411, -0.8312])
    ext = np.array([20.137, 12.049, 3.017])
    if planar:
        t = rng.uniform(0, 1, n)
        seg = rng.integers(0, 6, n)
        xy = np.empty((n, 2)); nr = np.zeros((n, 3))
        for s, (a, b) in enumerate([((0, 0), (1, 0)), ((1, 0), (1, 1)), ((1, 1), (0, 1)), ((0, 1), (0, 0)), ((0.3, 0), (0.3, 0.7)), ((0.7, 1), (0.7, 0.4))]):
            k = seg == s
            a, b = np.array(a) * ext[:2], np.array(b) * ext[:2]
            xy[k] = a + t[k, None] * (b - a)
            d = (b - a) / np.linalg.norm(b - a)
            nr[k, :2] = [-d[1], d[0]]
        xy += rng.normal(0, 0.005, (n, 2)) + org[:2]
        return cloud(np.c_[xy, np.zeros(n)]), nr.astype(F)
    area = np.array([ext[0] * ext[1]] * 2 + [ext[0] * ext[2]] * 2 + [ext[1] * ext[2]] * 2)
    face = rng.choice(6, n, p=area / area.sum())
    u = rng.uniform(0, 1, (n, 3))
    nr = np.zeros((n, 3))
    for f in range(6):
        ax = (2, 2, 1, 1, 0, 0)[f]
        k = face == f
        u[k, ax] = f % 2
        nr[k, ax] = 1.0
    xyz = org + u * ext + rng.normal(0, 0.005, (n, 3))
    return cloud(xyz), nr.astype(F)


class Grown:
    """one handle, the clouds it holds (in append order) and the checks every update ends with"""

    def __init__(self, amd, seed=0, planar=False):
        self.amd, self.planar, self.rng = amd, planar, np.random.default_rng(seed)
        self.kw = dict(CFG, is_2d=1) if planar else dict(CFG)
        self.icp = amd.ICPSequence(**self.kw)
        base, nrm = room(self.rng, planar=planar)
        assert self.icp.setMap(base, nrm)
        self.clouds = [base]
        g = self.icp.gridInfo()
        self.cell, self.dims = F(g["cell"]), list(g["dims"])
        self.lo, self.hi = base[:, :3].min(axis=0), base[:, :3].max(axis=0)
        self.mean = self.icp.getMapMean()
        assert np.array_equal(bits(self.mean), bits(K.predicted_mean(self.clouds)))
        assert self.dims == K.grid_dims(self.lo, self.hi, self.cell, self.mean)
        inner = np.array([1.0, 1.0, 0.0 if planar else 0.75])
        self.in_lo, self.in_hi = self.lo + inner, self.hi - inner
        self.check_index("setMap")

    @property
    def m(self):
        return sum(c.shape[0] for c in self.clouds)

    def expand(self, c):
        return [c]

    def append(self, delta):
        app, m = self.icp.mapUpdatePointDistance(delta, 0.0, normals_knn=KNN)
        assert app == delta.shape[0]
        return m

    def update(self, delta, name, rebuild=False, first=False):
        """append `delta`; the centroid is the predicted one, the counters name the path: the index insert (or, rebuild, a build from
        scratch) and the subset normals pass (or, first, the pass over the whole map)"""
        c0 = self.icp.debugCounters()
        m = self.append(delta)
        self.clouds += self.expand(delta)
        assert m == self.m
        c1 = self.icp.debugCounters()
        step = [int(c1[i] & 0xffffffff) - int(c0[i] & 0xffffffff) for i in (INSERTS, REBUILDS, SUBSET, WHOLE)]
        assert step == [0 if rebuild else 1, 1 if rebuild else 0, 0 if first else 1, 1 if first else 0], (name, step)
        self.mean = self.icp.getMapMean()
        want = K.predicted_mean(self.clouds)
        assert np.array_equal(bits(self.mean), bits(want)), (name, self.mean, want)

    def moved_to(self, others, mean_target, n=1500):
        """ballast that puts the centroid of [resident ; others ; ballast] on mean_target"""
        ex = [e for o in others for e in self.expand(o)]
        return K.ballast(n, self.in_lo, self.in_hi, self.clouds, ex, mean_target, self.rng, expand=self.expand)

    def check_index(self, name, note=""):
        pts, nrm = self.icp.getMap(with_normals=True)
        assert np.array_equal(bits(pts), bits(np.concatenate(self.clouds))), name
        srt, pn = self.icp.debugIndexNormals()
        unplaced = int(self.icp.debugCounters()[UNPLACED])
        stale = (bits(srt) != bits(nrm)).any(axis=1)
        stale_pn = (bits(pn) != bits(nrm)).any(axis=1) if pn is not None else np.zeros_like(stale)
        print(f"{name}: {int(stale.sum())} stale normals in the sorted copy, {int(stale_pn.sum())} in the interleaved one, "
              f"{unplaced} unplaced by the patch, of {pts.shape[0]} points{note}")
        assert pn is not None                      # an owner handle with normals keeps the interleaved copy
        assert not stale.any() and not stale_pn.any() and unplaced == 0, \
            f"{name}: {int(stale.sum())} / {int(stale_pn.sum())} stale normals, {unplaced} unplaced{note}; first {np.flatnonzero(stale | stale_pn)[:8]}"
        return nrm


def walls_then_companions(g, extra_b=(), extra_c=(), steps=1, axes=(0, 1, 2)):
    """updates A, B and C (and steps - 1 more like C) on g; returns (first index of the wall points, the wall points)"""
    rng = g.rng
    a = room(rng, 400, planar=g.planar)[0]
    a[:, :3] = np.clip(a[:, :3], g.lo, g.hi)
    g.update(a, "A", first=True)
    g.check_index("A")
    mean_b = (g.mean.astype(np.float64) + T_B).astype(F)
    mean_c = (mean_b.astype(np.float64) + T_STEP).astype(F)
    if g.planar:
        mean_b[2] = mean_c[2] = 0
    # ---- B: the wall points, keyed under mean_b
    w, flips, _ = K.wall_points(g.lo, g.hi, g.cell, g.dims, mean_b, mean_c, rng, axes=axes)
    w = w[np.sort(rng.permutation(w.shape[0])[:400])]       # (a fine grid has thousands of walls: a few hundred points are plenty)
    assert K.flip_mask(w, g.lo, g.cell, g.dims, mean_b, mean_c).sum() >= 32

    def next_mean(prev):
        """the centroid of the next update: about T_STEP further, and -- which float32 neighbour of that exactly is the test's to choose -- one
        under which at least half of the wall points still change cell against mean_b (whether a point does depends on the last bits of the
        centroid, not on how far it moved)"""
        cand = (prev.astype(np.float64) + T_STEP).astype(F)
        for _ in range(256):
            if K.flip_mask(w, g.lo, g.cell, g.dims, mean_b, cand).sum() >= w.shape[0] // 2:
                return cand
            cand = np.nextafter(cand, F(np.inf) * np.sign(T_STEP).astype(F))
            if g.planar:
                cand[2] = 0
        raise AssertionError("no centroid near the next step under which the wall points change cell")

    first = g.m
    others = [w] + list(extra_b)
    g.update(np.concatenate(others + [g.moved_to(others, mean_b)]), "B")
    assert np.array_equal(bits(g.mean), bits(mean_b))
    g.check_index("B")
    # ---- C (and on): companions of every wall point and of whatever else the caller watches; the wall points' keys are 1, 2, ... centroids old
    watched = np.concatenate([w] + list(extra_b))
    for s in range(steps):
        name = "CDEFGH"[s]
        mean_c = mean_c if s == 0 else next_mean(mean_c)
        others = [K.companions_of(e, rng, planar=g.planar) for e in [w] + list(extra_b)] + (list(extra_c) if s == 0 else [])
        before = g.icp.getMap(with_normals=True)[1]
        g.update(np.concatenate(others + [g.moved_to(others, mean_c)]), name)
        assert np.array_equal(bits(g.mean), bits(mean_c))
        after = g.icp.getMap(with_normals=True)[1]
        # the precondition, from the device's own centroids and grid: enough wall points BOTH change cell AND got a new normal
        flipped = K.flip_mask(w, g.lo, g.cell, g.dims, mean_b, g.mean)
        changed = (bits(before[first:first + w.shape[0]]) != bits(after[first:first + w.shape[0]])).any(axis=1)
        both = int((flipped & changed).sum())
        note = f" ({int(flipped.sum())} wall points predicted to change cell, {int(changed.sum())} with a new normal, {both} both, of {w.shape[0]})"
        assert both >= 32, name + note
        ch_all = (bits(before[first:first + watched.shape[0]]) != bits(after[first:first + watched.shape[0]])).any(axis=1)
        assert ch_all[w.shape[0]:].all() or not len(extra_b), "the watched extra points did not all get a new normal"
        g.check_index(name, note)
    return first, w


def registration_equals_a_fresh_handle(g, w):
    """a reading cut from the wall points: the flipped points are the ones matched"""
    pts, nrm = g.icp.getMap(with_normals=True)
    reading = w.copy()
    reading[:, :3] += np.array([0.01, -0.008, 0.0 if g.planar else 0.005], dtype=F)
    for knn in (1, 3):        # k = 1 reads the sorted normals, k > 1 the interleaved copy
        kw = dict(g.kw, knn=knn)
        # (the fresh handle on the grown one's grid -- every delta lay inside the first map's box, so the cell edge decides it: the loop sums its
        #  pairs in the order of the reading sorted by grid tile, and two grids give sums that differ in the last bits whatever the normals are)
        fresh = g.amd.ICPSequence(**dict(kw, grid_cell=float(g.cell)))
        assert fresh.setMap(pts, nrm)
        gi, gf = g.icp.gridInfo(), fresh.gridInfo()
        assert (gi["cell"], gi["dims"]) == (gf["cell"], gf["dims"])
        g.icp.setConfig(**kw)
        T, Tf = g.icp(reading), fresh(reading)
        assert np.array_equal(bits(T), bits(Tf)), (knn, T, Tf)
        r, rf = g.icp.residual(reading, T), fresh.residual(reading, T)
        assert r.pairs == rf.pairs and r.pairs > w.shape[0] // 2
        assert r.sum_abs == rf.sum_abs and r.sum_sq == rf.sum_sq and r.sum_abs > 0, (knn, r.sum_abs, rf.sum_abs)      # float64: equal values are equal bits
        assert g.icp.errorMinimizer.getResidualError(reading, T) == fresh.errorMinimizer.getResidualError(reading, T)
    g.icp.setConfig(**g.kw)


def test_patched_normals_reach_points_on_cell_walls(amd):
    g = Grown(amd, seed=0)
    first, w = walls_then_companions(g)
    registration_equals_a_fresh_handle(g, w)


def test_keys_two_and_three_centroids_stale(amd):
    g = Grown(amd, seed=1)
    first, w = walls_then_companions(g, steps=4)
    registration_equals_a_fresh_handle(g, w)


def test_planar_handle(amd):
    """is_2d: z = 0 everywhere, one layer of cells, walls on x and y only"""
    g = Grown(amd, seed=2, planar=True)
    assert g.dims[2] == 1
    first, w = walls_then_companions(g, axes=(0, 1))
    assert (np.concatenate(g.clouds)[:, 2] == 0).all()
    registration_equals_a_fresh_handle(g, w)


def test_delta_that_overhangs_the_box_by_one_cell(amd):
    """map_insert takes points up to two cells outside the box and clamps them into the border cells: the patch must clamp the same way"""
    g = Grown(amd, seed=3)
    rng = np.random.default_rng(30)
    n = 120
    xyz = rng.uniform(g.in_lo, g.in_hi, (n, 3))
    ax, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    over = rng.uniform(0.05, 0.95, n) * float(g.cell)
    xyz[np.arange(n), ax] = np.where(side == 0, g.lo[ax] - over, g.hi[ax] + over)
    out = cloud(xyz)
    assert ((out[:, :3] < g.lo) | (out[:, :3] > g.hi)).any(axis=1).all()
    walls_then_companions(g, extra_b=[out])      # (no registration against a fresh handle here: its box, hence its grid, would be another)


def test_full_rebuild_control(amd):
    """a delta far outside the box: the insert declines, the index is built from scratch under the new centroid -- every key is fresh, no
    flip is predicted, and the patch behind the build still has to leave the index equal to the map"""
    g = Grown(amd, seed=4)
    first, w = walls_then_companions(g)
    far = cloud(np.array([g.hi + 5.0 * float(g.cell) + [0.5, 0.2, 0.1], g.hi + 5.0 * float(g.cell)]))
    comp = K.companions_of(w, g.rng)
    others = [comp, far]
    mean_d = (g.mean.astype(np.float64) + T_STEP).astype(F)
    g.update(np.concatenate(others + [g.moved_to(others, mean_d)]), "rebuild", rebuild=True)
    assert not K.flip_mask(w, g.lo, g.cell, g.dims, g.mean, g.mean).any()
    g.check_index("rebuild")


class GrownByEpochs(Grown):
    """the same handle fed through the map-growth epoch (icpmi_staged_merge_allgather with normals_knn) under the loopback communicator: three
    simulated ranks, rank r's block = the scan moved r * 2^-5 m along x (an exact float32 step: p.x + r * shift rounds once, fused or not)"""
    SHIFT = F(0.03125)

    def __init__(self, amd, seed):
        super().__init__(amd, seed=seed)
        self.icp.commInit(self.icp.commUniqueId(), 1, 0)
        assert self.icp.commInfo()[0] == 3

    def expand(self, c):
        out = []
        for r in range(3):
            e = c.copy()
            if r:
                e[:, 0] = e[:, 0] + F(r) * self.SHIFT
            out.append(e)
        return out

    def append(self, delta):
        eye = np.eye(4, dtype=F)
        self.icp.registerWithPrior(delta, eye)
        mine, app, m, merged = self.icp.stagedMergeAllGather(eye, 0.0, normals_knn=KNN, return_merged=True)
        assert mine == delta.shape[0] and app == 3 * mine
        assert np.array_equal(bits(merged), bits(np.concatenate(self.expand(delta))))
        return m

    def update(self, delta, name, **kw):
        if kw.get("first"):           # update A goes in directly: the epoch route starts at B
            m = Grown.append(self, delta)
            self.clouds.append(delta)
            assert m == self.m
            self.mean = self.icp.getMapMean()
            return
        super().update(delta, name, **kw)


def test_epoch_route_under_the_loopback_communicator(amd, monkeypatch):
    monkeypatch.setenv("ICPMI_COMM_LOOPBACK", "3")
    monkeypatch.setenv("ICPMI_COMM_LOOPBACK_SHIFT", "0.03125")
    g = GrownByEpochs(amd, seed=5)
    walls_then_companions(g)                     # (the shifted copies may leave the first map's box: no fresh handle on the same grid)
