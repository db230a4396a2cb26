"""Level-0 cell keys of the registration index (csrc/map_build.hip: cell_of, key_kernel, ins_key_kernel, patch_normals_kernel), restated in
float32 numpy, and clouds built so that a point's STORED key and the key RECOMPUTED under a later centroid differ.

A point keeps the key it got under the centroid of its own build or insert (ins_move0_kernel copies it); every later insert re-centres the
point on a new centroid `mean` and moves the grid origin to float32(lo_raw - mean).  The cell of a coordinate p on one axis is

    floor(f32(f32(f32(p - mean) - o) * inv))   clamped to [0, n - 1],     o = f32(lo_raw - mean), inv = f32(1 / cell)

Every operation rounds to float32 on its own: two subtractions and then one multiply, and no multiply feeds an add or a subtract, so there
is nothing the compiler could contract into an fma -- numpy's float32 arithmetic gives the device's bits.  For a coordinate within a few
ulps of a cell wall the result depends on `mean`: such a point changes cell when the centroid moves, by one cell at the most (the three
roundings are each below an ulp of the box's extent, a cell is thousands of ulps wide).

No GPU needed: tests/test_index_keys_cpu.py checks the generator, tests/test_gpu_index_normals.py feeds its clouds to the device."""
import numpy as np

F = np.float32


def cell_1d(p, mean, lo_raw, cell, n):
    """cell_of on one axis: p any array of float32 coordinates, mean / lo_raw / cell float32 scalars, n the cells on that axis"""
    p = np.asarray(p, dtype=F)
    mean, lo_raw = F(mean), F(lo_raw)
    inv = F(1.0) / F(cell)            # make_grid: 1.0f / cell
    o = lo_raw - mean                 # float32 - float32 -> float32 (map_insert: clo, make_grid: ox)
    v = p - mean                      # the centred coordinate, as scatter_kernel / ins_move0_kernel store it
    v = v - o
    v = v * inv
    assert v.dtype == F and isinstance(o, F) and isinstance(inv, F)
    c = np.floor(v).astype(np.int64)
    return np.clip(c, 0, int(n) - 1)


def cells(pts, mean, lo_raw, cell, dims):
    """(N, 3) int64 level-0 cell of every point of pts (N, >= 3) under the centroid `mean`"""
    pts = np.asarray(pts, dtype=F)
    return np.stack([cell_1d(pts[:, a], mean[a], lo_raw[a], cell, dims[a]) for a in range(3)], axis=1)


def flip_mask(pts, lo_raw, cell, dims, mean_a, mean_b):
    """True where a point's cell under mean_a differs from its cell under mean_b, on any axis"""
    return (cells(pts, mean_a, lo_raw, cell, dims) != cells(pts, mean_b, lo_raw, cell, dims)).any(axis=1)


def grid_dims(lo_raw, hi_raw, cell, mean):
    """make_grid's cells per axis for the box [lo_raw, hi_raw] centred on `mean`"""
    lo, hi, mean = np.asarray(lo_raw, F), np.asarray(hi_raw, F), np.asarray(mean, F)
    inv = F(1.0) / F(cell)
    return [int(np.floor(((hi[a] - mean[a]) - (lo[a] - mean[a])) * inv)) + 1 for a in range(3)]


def wall_points(lo_raw, hi_raw, cell, dims, mean_a, mean_b, rng, ulps=64, per_wall=4, copies=3, axes=(0, 1, 2), companions=3):
    """Points that sit on the interior cell walls and change cell between the centroids mean_a and mean_b.

    For every interior wall w = 1 .. dims[a] - 1 of every axis a in `axes` the float32 values within `ulps` ulps of lo_raw[a] + w * cell are
    scanned; those whose cell under mean_a differs from their cell under mean_b are kept, at most per_wall per wall (chosen at random;
    the band of such values is a few ulps wide), and each becomes `copies` points.  The other two coordinates are spread uniformly over the
    inner box (one cell away from its faces; an axis with lo == hi stays there: a planar cloud).  Returns
      pts (N, 4) float32, w = 1
      flips (N,) bool: flip_mask of the finished points (all True by construction; recomputed over the three axes)
      comp (N * companions, 4) float32: the companion delta -- per point `companions` points 1 to 3 cm away in directions of its own, so they
        do not lie in one plane with whatever surrounds the point: appended later, they enter its k = 10 neighbourhood and change its normal
        (planar cloud: the offsets stay in z = const)."""
    lo, hi = np.asarray(lo_raw, F), np.asarray(hi_raw, F)
    mean_a, mean_b = np.asarray(mean_a, F), np.asarray(mean_b, F)
    steps = np.arange(-ulps, ulps + 1, dtype=np.float64)
    out = []
    for a in axes:
        n = int(dims[a])
        if n < 2:
            continue
        walls = lo[a].astype(np.float64) + np.arange(1, n, dtype=np.float64) * float(F(cell))
        walls = walls[walls < float(hi[a])].astype(F)
        cand = (walls[:, None].astype(np.float64) + steps[None, :] * np.spacing(np.abs(walls))[:, None].astype(np.float64)).astype(F)
        diff = cell_1d(cand, mean_a[a], lo[a], cell, n) != cell_1d(cand, mean_b[a], lo[a], cell, n)
        for w in range(cand.shape[0]):
            vals = np.unique(cand[w][diff[w]])
            if vals.size == 0:
                continue
            vals = np.repeat(rng.permutation(vals)[:per_wall], copies)
            p = np.empty((vals.size, 3), dtype=F)
            for b in range(3):
                if b == a:
                    p[:, b] = vals
                elif hi[b] - lo[b] > 2.5 * cell:
                    p[:, b] = rng.uniform(float(lo[b]) + cell, float(hi[b]) - cell, vals.size).astype(F)
                else:
                    p[:, b] = rng.uniform(float(lo[b]), float(hi[b]), vals.size).astype(F)
            out.append(p)
    xyz = np.concatenate(out) if out else np.zeros((0, 3), dtype=F)
    pts = np.ones((xyz.shape[0], 4), dtype=F)
    pts[:, :3] = xyz
    flips = flip_mask(pts, lo, cell, dims, mean_a, mean_b)
    return pts, flips, companions_of(pts, rng, companions, planar=bool(hi[2] == lo[2]))


def companions_of(pts, rng, companions=3, planar=False):
    """(N * companions, 4): per point of pts `companions` points 1 to 3 cm away in random directions (planar: inside z = const)"""
    xyz = np.asarray(pts, dtype=F)[:, :3]
    d = rng.normal(size=(xyz.shape[0], companions, 3))
    if planar:
        d[:, :, 2] = 0.0
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    d *= rng.uniform(0.01, 0.03, size=(xyz.shape[0], companions, 1))
    comp = np.ones((xyz.shape[0] * companions, 4), dtype=F)
    comp[:, :3] = (xyz[:, None, :].astype(np.float64) + d).reshape(-1, 3).astype(F)
    return comp


def predicted_mean(clouds):
    """the centroid the index takes for the concatenation of `clouds`: the sum in float64, divided by the count, rounded to float32 once"""
    s = np.zeros(3, dtype=np.float64)
    m = 0
    for c in clouds:
        s += np.asarray(c, dtype=F)[:, :3].astype(np.float64).sum(axis=0)
        m += c.shape[0]
    return (s / float(m)).astype(F)


def ballast(n, lo, hi, resident, others, mean_target, rng, expand=lambda c: [c]):
    """n points (n, 4) inside the inner box [lo, hi] such that the cloud [resident ; others ; expand(these)] has exactly the centroid
    mean_target (float32, as predicted_mean rounds it): uniform points around the centroid they must have -- as wide a block as the inner box
    leaves room for --, moved onto the sum they must have, the last one taking the rounding residue.  This is how a test CHOOSES the centroid of an update instead of solving for it: the wall points depend on the centroid,
    and the centroid on the wall points.  expand: what the update appends for a delta c, as a list of clouds (the loopback communicator's
    epoch appends shifted copies); `others` is handed in expanded."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)

    def total(c):
        return sum(np.asarray(e, dtype=F)[:, :3].astype(np.float64).sum(axis=0) for e in c)

    def as_cloud(xyz):
        out = np.ones((n, 4), dtype=F)
        out[:, :3] = xyz
        return out

    reps = len(expand(as_cloud(np.zeros((n, 3)))))
    m = sum(c.shape[0] for c in resident) + sum(c.shape[0] for c in others) + n * reps
    need = np.asarray(mean_target, F).astype(np.float64) * float(m) - total(list(resident) + list(others))
    centre = need / (n * reps) - (total(expand(as_cloud(np.zeros((n, 3))))) / (n * reps))   # where the ballast's own centroid has to lie
    half = np.minimum(centre - lo, hi - centre)
    assert (half >= 0).all(), f"the ballast's centroid {centre} lies outside [{lo}, {hi}]: more ballast points are needed"
    xyz = centre + rng.uniform(-1.0, 1.0, size=(n, 3)) * half * 0.98
    xyz += (need - total(expand(as_cloud(xyz)))) / (n * reps)
    xyz = xyz.astype(F)
    for _ in range(3):  # the residue of the roundings goes to the last point (its own rounding is ~1e-7 of a sum whose slack is ~1e-2)
        xyz[-1] = (xyz[-1].astype(np.float64) + (need - total(expand(as_cloud(xyz)))) / reps).astype(F)
    out = as_cloud(xyz)
    got = predicted_mean(list(resident) + list(others) + expand(out))
    assert np.array_equal(got.view(np.uint32), np.asarray(mean_target, F).view(np.uint32)), (got, mean_target)
    return out
