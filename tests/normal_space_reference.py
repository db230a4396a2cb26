"""NormalSpaceDataPointsFilter{nbSample, seed, epsilon} restated in numpy from the formulation as recalled (include/icpmi.h,
icpmi_normal_space_sampling), not from the kernels.  float32 where the text says float32: the two angles are computed
in double and rounded once, the two quotients and floors are float32.  `normal_space_sampling(..., buckets=device_buckets)` replays the
device's selection from its own buckets; without `buckets` everything is computed here.  `round_robin` is the literal loop the closed
form stands for (Python lists, one point per non-empty bucket per round)."""
import functools

import numpy as np

F = np.float32
MINSTD_A, MINSTD_M = 48271, 2147483647
TWO_PI = 6.283185307179586                                                   # 2 pi in double
TWO_PI_F = F(6.2831855)                                                      # (float)(2 pi): the stride's numerator
EPSILONS = (0.04908, 0.09817, 3.14159)                                       # the bounds and the default


@functools.lru_cache(maxsize=8)
def _minstd(x, n):
    out = np.empty(n, np.int64)
    for i in range(n):
        x = (x * MINSTD_A) % MINSTD_M
        out[i] = x
    out.setflags(write=False)
    return out


def minstd(seed, n):
    """r_0 .. r_{n-1}: r_i = the (i + 1)-th value of std::minstd_rand seeded with `seed` (seed % (2^31 - 1), 0 -> 1)"""
    return _minstd(int(seed) % MINSTD_M or 1, int(n))


def angles64(normals):
    """theta = acos(clamp(nz, -1, 1)) and phi = atan2(ny, nx) in [0, 2 pi], in double from the float32 normals"""
    nrm = np.asarray(normals, F).astype(np.float64)
    theta = np.arccos(np.clip(nrm[:, 2], -1.0, 1.0))
    phi = np.arctan2(nrm[:, 1], nrm[:, 0])
    phi = np.where(phi < 0.0, phi + TWO_PI, phi)
    return theta, phi


def stride_of(epsilon):
    return int(np.floor(TWO_PI_F / F(epsilon)))


def table_size(epsilon):
    """the number of buckets the two floors can reach: theta <= (float)pi, phi <= (float)(2 pi)"""
    return int(np.floor(F(3.14159274) / F(epsilon))) * stride_of(epsilon) + stride_of(epsilon) + 1


def buckets_of(normals, epsilon):
    theta, phi = angles64(normals)
    eps = F(epsilon)
    bt = np.floor(theta.astype(F) / eps).astype(np.int64)                    # float32 quotient, float32 floor
    bp = np.floor(phi.astype(F) / eps).astype(np.int64)
    return (bt * stride_of(epsilon) + bp).astype(np.int32)


def edge_margin(normals, epsilon):
    """per point: the distance of theta / epsilon and of phi / epsilon, evaluated in float64, from the nearest integer (the smaller)"""
    theta, phi = angles64(normals)
    eps = np.float64(F(epsilon))
    qt, qp = theta / eps, phi / eps
    return np.minimum(np.abs(qt - np.rint(qt)), np.abs(qp - np.rint(qp)))


def safe_normals(rng, n, epsilons=EPSILONS, margin=1e-3, scale=(1.0, 0.6, 1.4)):
    """n random unit normals (float32) none of which lies within `margin` buckets of a bucket edge for any of `epsilons`: candidates
    closer than that are rejected, in float64, while generating, and drawn again"""
    out = np.empty((0, 3), F)
    while out.shape[0] < n:
        v = rng.normal(size=(2 * (n - out.shape[0]) + 16, 3)) * np.asarray(scale)
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
        ok = np.ones(v.shape[0], bool)
        for e in epsilons:
            ok &= edge_margin(v, e) >= margin
        out = np.concatenate([out, v[ok]])
    return np.ascontiguousarray(out[:n])


def closed_form(buckets, r, nb):
    """the kept indices, ascending: rank < R* in the bucket (ascending r, then index), plus rank R* in the first rem buckets that
    have one; R* = the largest R with S(R) = sum_b min(c_b, R) <= nb"""
    buckets = np.asarray(buckets, np.int64)
    n = buckets.shape[0]
    assert 0 <= nb < n
    counts = np.bincount(buckets)
    S = lambda R: int(np.minimum(counts, R).sum())
    rstar, hi = 0, n                                                         # S is non-decreasing; S(0) = 0 <= nb < n = S(n)
    while hi - rstar > 1:
        mid = (rstar + hi) // 2
        rstar, hi = (mid, hi) if S(mid) <= nb else (rstar, mid)
    rem = nb - S(rstar)
    srt = np.lexsort((np.arange(n), r, buckets))                             # by bucket, then r, then index
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.arange(n) - start[buckets[srt]]
    has = counts > rstar
    extra = has & (np.cumsum(has) - has < rem)                               # the first rem buckets, ascending, among those with c_b > R*
    take = rstar + extra.astype(np.int64)
    keep = np.zeros(n, bool)
    keep[srt] = rank < take[buckets[srt]]
    assert int(keep.sum()) == nb
    return np.nonzero(keep)[0].astype(np.int32)


def round_robin(buckets, r, nb):
    """upstream's loop, literally: every bucket a list in drawing order (ascending r); rounds over the non-empty buckets in ascending
    bucket index, one point each, until nb points are taken; the kept indices sorted"""
    lists = {}
    for i in sorted(range(len(buckets)), key=lambda i: (int(r[i]), i)):
        lists.setdefault(int(buckets[i]), []).append(i)
    kept = []
    while len(kept) < nb:
        for b in sorted(lists):
            if lists[b]:
                kept.append(lists[b].pop(0))
                if len(kept) == nb:
                    break
    return np.asarray(sorted(kept), np.int32)


def normal_space_sampling(xyz, normals, nb, seed=1, epsilon=0.09817, buckets=None):
    """-> (order, buckets): the kept indices in ascending order and every point's bucket (None when nothing is sampled)"""
    n = np.shape(xyz)[0]
    if nb >= n:
        return np.arange(n, dtype=np.int32), None
    if normals is None and buckets is None:
        raise KeyError("normals")
    if nb == 0:
        return np.empty(0, np.int32), None
    if buckets is None:
        buckets = buckets_of(normals, epsilon)
    return closed_form(buckets, minstd(seed, n), nb), np.asarray(buckets, np.int32)
