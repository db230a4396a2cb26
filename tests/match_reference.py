"""Per-query references for k-nearest matches (CPU only): the oracle's kd-tree bit for bit, and an independent float64 exact kNN
(scipy.spatial.cKDTree) with the guarantees a float32 matcher must meet whatever its search order.

check_matches() takes the centred float32 map and the float32 queries exactly as the matcher saw them, and raises AssertionError
naming the first query that breaks a rule.  Tolerances, for float32 coordinates whose squared distance is formed in float32
(fmaf(dz, dz, fmaf(dy, dy, dx * dx)), dx = q.x - p.x):
  - d2 against the float64 distance of the same pair: dx carries one rounding (2u on dx^2, u = 2^-24), the product and the two fmas
    one each -- at most 5u of relative error; D2_REL = 6u.  (An error of 8 ulp is at least 8u.)
  - ranks: two float64 distances further apart than RANK_REL relative cannot swap in float32; below that either order is accepted
    and only the distance bound applies.
  - maxDist: a point within MAXD_REL of maxDist^2 may fall on either side.
"""
import math

import numpy as np

U = 2.0 ** -24
D2_REL = 6 * U
RANK_REL = 2e-6
MAXD_REL = 2e-6

_trees = {}


def _tree(map_c):
    """cKDTree of the float64 copy, cached per map array (the loop tests query the same map many times)"""
    from scipy.spatial import cKDTree
    key = (map_c.__array_interface__["data"][0], map_c.shape)
    t = _trees.get(key)
    if t is None or t[0] is not map_c:
        _trees.clear()
        t = (map_c, cKDTree(map_c[:, :3].astype(np.float64)))
        _trees[key] = t
    return t[1]


def _fail(where, what, rows):
    rows = np.asarray(rows).ravel()
    raise AssertionError(f"{where}: {what} at {rows.size} queries, first query {int(rows[0])} (queries {rows[:8].tolist()})")


def exact_knn64(map_c, q, k):
    """float64 distances (n, k + 1) sorted ascending and their ids (cKDTree, eps = 0); missing ranks (k + 1 > map size): +inf / -1"""
    m = map_c.shape[0]
    kk = min(k + 1, m)
    _, ii = _tree(map_c).query(q[:, :3].astype(np.float64), k=kk, workers=16)
    ii = ii.reshape(q.shape[0], kk)
    d64 = sq_dist64(map_c, q, ii)
    # cKDTree orders by its own float64 distance: re-sort on the recomputed squared distance, ties by index
    o = np.lexsort((ii, d64), axis=1)
    ii = np.take_along_axis(ii, o, 1); d64 = np.take_along_axis(d64, o, 1)
    if kk < k + 1:
        pad = k + 1 - kk
        ii = np.concatenate([ii, np.full((q.shape[0], pad), -1, np.int64)], 1)
        d64 = np.concatenate([d64, np.full((q.shape[0], pad), np.inf)], 1)
    return ii, d64


def sq_dist64(map_c, q, ids):
    """exact squared distance in float64 of query i and map point ids[i, j] (+inf where ids < 0)"""
    p = map_c[np.maximum(ids, 0), :3].astype(np.float64)
    d = ((p - q[:, None, :3].astype(np.float64)) ** 2).sum(-1)
    return np.where(ids >= 0, d, np.inf)


def check_structure(ids, d2, where="matches"):
    """rows ascending by (d2, id), unfilled slots (-1 / +inf) only at the end of a row, no id twice in a row"""
    filled = ids >= 0
    bad = np.nonzero((filled != np.isfinite(d2)).any(1))[0]
    if bad.size: _fail(where, "id -1 and d2 +inf do not go together", bad)
    bad = np.nonzero((~filled[:, :-1] & filled[:, 1:]).any(1))[0]
    if bad.size: _fail(where, "a filled slot behind an unfilled one", bad)
    a, b = d2[:, :-1], d2[:, 1:]
    ia, ib = ids[:, :-1], ids[:, 1:]
    both = filled[:, :-1] & filled[:, 1:]
    bad = np.nonzero((both & ((b < a) | ((b == a) & (ib <= ia)))).any(1))[0]
    if bad.size: _fail(where, "row not strictly ascending by (d2, id) (equal d2 resolve to the smaller index)", bad)
    s = np.sort(np.where(filled, ids, -1 - np.arange(ids.shape[1])[None, :]), axis=1)
    bad = np.nonzero((s[:, 1:] == s[:, :-1]).any(1))[0]
    if bad.size: _fail(where, "an id repeats within a row", bad)


def check_matches(map_c, q, ids, d2, k, max_dist, eps=0.0, use_oracle=True, where="matches"):
    """Assert that (ids, d2) -- (n, k) int32 / float32, original map indices -- are the k nearest neighbours of the float32 queries q
    (n, 4) in the centred float32 map map_c (m, 4) within max_dist: bitwise the oracle's (eps == 0 and use_oracle), and against the
    float64 exact kNN within the tolerances above; eps > 0 checks libnabo's guarantee d_j <= (1 + eps) exact_j instead of exactness."""
    map_c = np.ascontiguousarray(map_c, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    ids = np.asarray(ids); d2 = np.asarray(d2)
    n = q.shape[0]
    assert ids.shape == (n, k) and d2.shape == (n, k), (where, ids.shape, d2.shape, (n, k))
    assert ids.dtype == np.int32 and d2.dtype == np.float32, (where, ids.dtype, d2.dtype)
    check_structure(ids, d2, where)
    bad = np.nonzero(((ids < -1) | (ids >= map_c.shape[0])).any(1))[0]
    if bad.size: _fail(where, "id out of range", bad)

    if eps == 0 and use_oracle:
        import oracle_bindings as ob
        rids, rd2 = ob.knn(map_c, q, k=k, max_dist=max_dist, nthreads=16)
        bad = np.nonzero((rd2.view(np.uint32) != d2.view(np.uint32)).any(1))[0]
        if bad.size: _fail(where, f"d2 differs from the oracle's (first: {d2[bad[0]].tolist()} vs {rd2[bad[0]].tolist()})", bad)
        bad = np.nonzero((rids != ids).any(1))[0]
        if bad.size: _fail(where, f"ids differ from the oracle's (first: {ids[bad[0]].tolist()} vs {rids[bad[0]].tolist()})", bad)

    filled = ids >= 0
    own = sq_dist64(map_c, q, ids)                       # float64 distance of every returned pair
    with np.errstate(invalid="ignore"):
        err = np.abs(d2.astype(np.float64) - own)
    bad = np.nonzero((filled & ~(err <= D2_REL * own)).any(1))[0]
    if bad.size: _fail(where, f"d2 is not the float32 distance of its pair (relative error above {D2_REL:.2e})", bad)

    tid, t = exact_knn64(map_c, q, k)                    # true ranks 1 .. k + 1
    tk = t[:, :k]
    r2 = math.inf if math.isinf(max_dist) else float(max_dist) ** 2
    if eps > 0:
        f2 = (1.0 + eps) ** 2
        bad = np.nonzero((filled & ~(own <= f2 * tk * (1 + RANK_REL))).any(1))[0]
        if bad.size: _fail(where, f"a returned distance breaks d_j <= (1 + {eps}) exact_j", bad)
        # an approximate search may leave a slot empty only where the j-th true neighbour lies beyond maxDist / (1 + eps)
        bad = np.nonzero((~filled & (tk * f2 <= r2 * (1 - MAXD_REL))).any(1))[0]
        if bad.size: _fail(where, "a slot is unfilled although its true neighbour is well within maxDist / (1 + eps)", bad)
        return

    # no nearer point missed: the j-th returned distance is the j-th true one (up to float32 rounding)
    bad = np.nonzero((filled & ~(own <= tk * (1 + RANK_REL))).any(1))[0]
    if bad.size: _fail(where, "the j-th returned neighbour is farther than the true j-th (a nearer point was missed)", bad)
    # filled exactly where at least j points lie within maxDist (either answer inside the band around maxDist^2)
    inside = np.isfinite(tk) & (tk <= r2 * (1 - MAXD_REL))   # (a rank the map has no point for is +inf: never inside, whatever maxDist)
    outside = tk > r2 * (1 + MAXD_REL)
    bad = np.nonzero((inside & ~filled).any(1))[0]
    if bad.size: _fail(where, "a slot is unfilled although j points lie within maxDist", bad)
    bad = np.nonzero((outside & filled).any(1))[0]
    if bad.size: _fail(where, "a slot is filled although fewer than j points lie within maxDist", bad)
    # ids wherever the rank is unambiguous in float64
    lo = np.concatenate([np.full((n, 1), -np.inf), t[:, :k - 1]], 1) if k > 1 else np.full((n, 1), -np.inf)
    hi = t[:, 1:k + 1]
    with np.errstate(invalid="ignore"):
        clear = (tk - lo > RANK_REL * tk) & (hi - tk > RANK_REL * hi)
    bad = np.nonzero((filled & clear & (ids != tid[:, :k])).any(1))[0]
    if bad.size: _fail(where, f"id differs from the exact float64 kNN where the rank is unambiguous (first: {ids[bad[0]].tolist()} vs "
                               f"{tid[bad[0], :k].tolist()})", bad)


def trimmed_quantile(d2, ratio):
    """TrimmedDistOutlierFilter's limit by plain numpy: +inf and exact zeros dropped, the element at rank (int64)((float)n * ratio)"""
    v = np.asarray(d2, dtype=np.float32).ravel()
    v = v[np.isfinite(v) & (v > 0)]
    if v.size == 0:
        return -1.0
    if ratio == 1.0:
        return float(v.max())
    r = min(int(np.float32(v.size) * np.float32(ratio)), v.size - 1)
    return float(np.partition(v, r)[r])
