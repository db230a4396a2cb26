"""What the KDTreeVarDistMatcher tests share (test_gpu_var_dist.py, test_var_dist_cpu.py): the scene, the per-query radii row built from
each query's own exact neighbour distances, the condition that keeps the tie rule out of a comparison, and the masked reference.

Reference: the oracle's exact kNN (tests/oracle_bindings.py) with an unbounded search, masked per query in numpy -- slot j of query i
stays filled iff d2[i, j] <= r2[i], with r2 = float32(r) * float32(r) (+inf for +inf) against the oracle's float32 d2."""
import numpy as np

M, N = 4096, 1024
KS = (1, 6, 16, 20)          # nn1_wg_kernel, nnk_ml_kernel<6> / nnk_wg_kernel<6>, the KMAX 16 kernels, the one-lane kernel
KROWS = 20                   # neighbours per query the row and the condition look at
REL = 1e-5                   # no r^2 within this (relative) of one of the query's d2
KINDS = ("zero", "half_nearest", "mid_1_2", "mid_3_4", "inf")

_scene = {}


def scene():
    """dict(map, normals, scan, scan_normals) from synth: 4 096 map points and a 1 024-point reading in a 20 m room (neighbours ~0.5 m
    apart, so that a 0.3 m radius keeps some matches and drops others); built once per process"""
    if not _scene:
        from norlab_icp_mapper_amd import synth
        _scene.update(synth.make_scene(m=M, n=N, scale=0.2))
    return _scene


def centred(cloud, mean):
    out = cloud.copy()
    out[:, :3] = cloud[:, :3] - mean[None, :]
    return out


def squared(r):
    """the matcher's squaring: the float32 product, +inf for +inf"""
    r = np.asarray(r, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isinf(r), np.float32(np.inf), r * r).astype(np.float32)


def exact_rows(ob, mapc, q, k=KROWS):
    """the oracle's exact kNN, unbounded: (ids (n, k) int32, d2 (n, k) float32)"""
    return ob.knn(mapc, q, k=k, max_dist=np.inf, nthreads=16)


def clear_of(r, d2):
    """per query: r^2 is farther than REL (relative to the larger of the two) from every finite d2 of the query"""
    r2 = squared(r).astype(np.float64)[:, None]
    d = d2.astype(np.float64)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(d) & np.isfinite(r2) & (np.abs(r2 - d) <= REL * np.maximum(r2, d))
    return ~near.any(1)


def radii_row(d2_exact):
    """(radii (n,) float32, kind (n,) index into KINDS): query i takes kind i % 5 -- 0; half its nearest distance (no match); the
    midpoint between its 1st and 2nd neighbour (one match); between its 3rd and 4th (three); +inf (all).  A query whose radius would
    come within REL of one of its own d2 (coincident neighbours) takes +inf instead."""
    d = np.sqrt(d2_exact.astype(np.float64))
    n = d.shape[0]
    kind = np.arange(n) % 5
    r = np.zeros(n, np.float64)
    r[kind == 1] = 0.5 * d[kind == 1, 0]
    r[kind == 2] = 0.5 * (d[kind == 2, 0] + d[kind == 2, 1])
    r[kind == 3] = 0.5 * (d[kind == 3, 2] + d[kind == 3, 3])
    r[kind == 4] = np.inf
    r = r.astype(np.float32)
    bad = ~clear_of(r, d2_exact)
    r[bad] = np.inf
    kind[bad] = 4
    return r, kind


def expected_filled(kind, k):
    """slots the row prescribes per query, by construction"""
    return np.choose(kind, [0, 0, min(1, k), min(3, k), k])


def masked(ids, d2, r, k):
    """the reference: the first k exact neighbours, slot j unfilled (-1 / +inf) where d2 > r^2"""
    keep = d2[:, :k] <= squared(r)[:, None]
    return np.where(keep, ids[:, :k], -1).astype(np.int32), np.where(keep, d2[:, :k], np.float32(np.inf)).astype(np.float32)
