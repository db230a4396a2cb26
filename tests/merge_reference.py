"""The rank-ordered merge of the map-growth epoch (csrc/ops.hip: merge_greedy), stated as plainly as it can be stated, and -- apart from
it -- restatements of the kernel's cell index, cell key, hash and table size that the case builder uses to CONSTRUCT and CERTIFY cases.

The rule: block by block in rank order, point p of block r is dropped iff some KEPT point q of a block < r has
FLT_EPSILON < d2(p, q) and (double)d2 < (double)minDist * (double)minDist, d2 the float32 chain fma(dz, dz, fma(dy, dy, dx * dx)).

merge() is brute force over all kept points: no grid, no hash, nothing of the kernel's structure.  The restatements below it never decide
a verdict."""
import numpy as np

F = np.float32
FLT_EPSILON = F(1.1920929e-07)


def d2_rows(p, q):
    """(a, b) float32: sqdist3 of every p (a, 3) against every q (b, 3) -- the chain of residual_reference.sqdist3_f32 (differences in
    float32; a product of two float32 is exact in float64, so each fma is one float64 add rounded to float32)"""
    acc = None
    for ax in range(3):
        d = (p[:, None, ax] - q[None, :, ax]).astype(np.float64)
        acc = (d * d).astype(F) if acc is None else (d * d + acc.astype(np.float64)).astype(F)
    return acc


def near(d2, lim):
    return (d2 > FLT_EPSILON) & (d2.astype(np.float64) < lim)


def merge(blocks, min_dist, chunk=512):
    """blocks: (n_r, >= 3) float32 arrays in rank order.  Returns (kept masks per block, merged set: rank order then input order inside a
    block, undecidable pairs).  An undecidable pair ((r, i), (r_q, i_q)) is a point and a KEPT lower-block point whose verdict changes
    when d2 moves one float32 ulp either way: the numpy restatement of the fma chain can round twice, so such a pair proves nothing."""
    blocks = [np.ascontiguousarray(b, dtype=F) for b in blocks]
    lim = float(F(min_dist)) * float(F(min_dist))
    kept_xyz = np.zeros((0, 3), F)
    kept_src = np.zeros((0, 2), np.int64)
    masks, undecidable = [], []
    for r, b in enumerate(blocks):
        n = b.shape[0]
        drop = np.zeros(n, bool)
        if n and kept_xyz.shape[0] and min_dist > 0:
            for s in range(0, n, chunk):
                d2 = d2_rows(b[s:s + chunk, :3], kept_xyz)
                verdict = near(d2, lim)
                drop[s:s + chunk] = verdict.any(1)
                moved = (near(np.nextafter(d2, F(-np.inf)), lim) != verdict) | (near(np.nextafter(d2, F(np.inf)), lim) != verdict)
                for i, j in zip(*np.nonzero(moved)):
                    undecidable.append(((r, s + int(i)), (int(kept_src[j, 0]), int(kept_src[j, 1]))))
        keep = ~drop
        masks.append(keep)
        kept_xyz = np.concatenate([kept_xyz, b[keep, :3]])
        kept_src = np.concatenate([kept_src, np.stack([np.full(int(keep.sum()), r), np.nonzero(keep)[0]], 1).astype(np.int64)])
    cols = max([b.shape[1] for b in blocks] + [4])
    merged = np.concatenate([b[m] for b, m in zip(blocks, masks)] + [np.zeros((0, cols), F)])
    return masks, merged, undecidable


# ------------------------------------------------------------------------------------------------ restatements (construct and certify only)
MASK21 = 0x1fffff
SINGLE_LAUNCH_SPAN = 1 << 22          # merge_greedy: a larger padded span takes the per-block launches


def cell_edge(min_dist):
    """(h, inv_h) as merge_greedy computes them in float32 (the library is built with -ffp-contract=off)"""
    h = F(F(F(min_dist) * F(1.001)) + F(1e-6))
    return h, F(F(1.0) / h)


def cell_of(v, inv_h):
    """merge_cell_of: floorf(v * inv_h), the product rounded to float32"""
    return np.floor(np.asarray(v, F) * F(inv_h)).astype(np.int64)


def cell_key(cells):
    """merge_cell_key: 21 bits per axis, two's complement under the mask"""
    c = np.asarray(cells, np.int64) & MASK21
    return (c[..., 0] | (c[..., 1] << 21) | (c[..., 2] << 42)).astype(np.uint64)


def mix64(x):
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33); x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33); x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def table_capacity(total):
    cap = 1024
    while cap < 2 * total:
        cap <<= 1
    return cap


def home_slot(keys, cap):
    return (mix64(keys) & np.uint64(cap - 1)).astype(np.int64)


def filter_bit(keys):
    """the 24 bits of the hash that index the occupied-cell filter"""
    return (mix64(keys) >> np.uint64(40)).astype(np.int64)


def point_cells(blocks, min_dist):
    _, inv_h = cell_edge(min_dist)
    pts = np.concatenate([np.asarray(b, F)[:, :3] for b in blocks] + [np.zeros((0, 3), F)])
    return cell_of(pts, inv_h)


NEIGHBOURS = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)


def occupied_slots(keys, cap):
    """the slots a linear-probing table holds once `keys` (distinct) are in: the set does not depend on the insertion order"""
    occ = np.zeros(cap, bool)
    for s in np.sort(home_slot(keys, cap)):
        while occ[s]:
            s = (s + 1) % cap
        occ[s] = True
    return occ


def hash_facts(blocks, min_dist):
    """what the hash table and the filter of this case look like: dict of
    cells (distinct occupied keys), cap, wrapped (occupied slots at both ends of the table while some key's home is in the last two),
    max_home (most keys on one home slot), false_positives (probes, over the 27 cells of every point behind the first non-empty block, of
    an EMPTY cell whose filter bit is set), longest_miss (slots such a probe walks before it meets a free one)"""
    cells = point_cells(blocks, min_dist)
    total = cells.shape[0]
    cap = table_capacity(total)
    keys = np.unique(cell_key(cells))
    homes = home_slot(keys, cap)
    occ = occupied_slots(keys, cap)
    counts = [len(b) for b in blocks]
    first = next((r for r, n in enumerate(counts) if n), len(counts))
    behind = cells[sum(counts[:first + 1]):]
    bits = np.zeros(1 << 24, bool)
    bits[filter_bit(keys)] = True
    fp, longest = 0, 0
    if behind.shape[0]:
        probe = np.unique(cell_key((behind[:, None, :] + NEIGHBOURS[None, :, :]).reshape(-1, 3)), return_counts=True)
        empty = ~np.isin(probe[0], keys)
        hit = empty & bits[filter_bit(probe[0])]
        fp = int(probe[1][hit].sum())
        for s in home_slot(probe[0][hit], cap):
            steps = 0
            while occ[s]:
                s = (s + 1) % cap; steps += 1
            longest = max(longest, steps)
    return {"cells": int(keys.size), "cap": cap, "wrapped": bool(keys.size and (homes >= cap - 2).any() and occ[0] and occ[cap - 1]),
            "max_home": int(np.bincount(homes).max()) if keys.size else 0, "false_positives": fp, "longest_miss": longest}
