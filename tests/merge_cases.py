"""Named cases for the rank-ordered merge (tests/merge_reference.py states the rule): each a list of blocks of DIFFERENT points plus min_dist
and the stride of the padded layout.  case(name) builds one (cached) as a dict:
  blocks, min_dist, stride, group,
  exempt   -- pairs the undecidable count may name (the threshold pairs: exact by construction, see thresholds()),
  certify  -- properties of merge_reference.hash_facts / of the layout this case was built to have,
  expect   -- kept masks known in advance (the chains), or None.
Random cases scale their slab with min_dist: the ragged slab is 6 x 6 x 1.2 m at min_dist 0.15, i.e. 40 x 40 x 8 min_dist, so that every
larger block behind the first keeps a share of its points that is neither ~0 nor ~1 whatever min_dist is."""
import functools

import numpy as np

import merge_reference as mr

F = np.float32
RAGGED = (1500, 0, 2047, 65, 1, 900, 2049, 300)


def f4(xyz, w0=0):
    """x y z w: w carries a serial number, so a merged set that holds the right coordinates of the wrong point is seen"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, (w0 + np.arange(xyz.shape[0], dtype=F))[:, None]], 1).astype(F)


def split(pts, counts):
    out, s = [], 0
    for n in counts:
        out.append(f4(pts[s:s + n], s)); s += n
    return out


def slab(seed, counts, min_dist, centre=(0.0, 0.0, 0.0), dims=(40.0, 40.0, 8.0)):
    """sum(counts) uniform points in a slab of dims * min_dist around centre, dealt to the blocks in order.  dims are scaled so that the
    slab holds 1.44 min_dist^3 per point -- the density of the 8 862 ragged points in 40 x 40 x 8"""
    rng = np.random.default_rng(seed)
    total = int(sum(counts))
    d = np.asarray(dims, np.float64)
    d = d * (1.44 * max(total, 1) / d.prod()) ** (1.0 / 3.0) * min_dist
    pts = (rng.uniform(-0.5, 0.5, (total, 3)) * d + np.asarray(centre, np.float64)).astype(F)
    return split(pts, counts)


def _case(group, blocks, min_dist, stride=None, **kw):
    counts = [b.shape[0] for b in blocks]
    c = {"group": group, "blocks": blocks, "min_dist": float(min_dist), "stride": int(max(counts + [0]) if stride is None else stride),
         "exempt": set(), "certify": {}, "expect": None}
    c.update(kw)
    return c


# ---------------------------------------------------------------------------------------------------------------------------- the groups
def ragged(stride_kind, first_empty=False, min_dist=0.15, centre=(0, 0, 0), seed=11):
    counts = list(RAGGED)
    if first_empty:
        counts = [0] + counts[:-1]                   # the first non-empty block is block 1, with different data behind it
    blocks = slab(seed, counts, min_dist, centre)
    stride = {"max": max(counts), "max+1": max(counts) + 1, "4096": 4096}[stride_kind]
    return _case("ragged", blocks, min_dist, stride)


def tpb_edge(maxc, ranks):
    """tpb = (maxc + 63) & ~63 at its edges: the largest block has maxc points, the others fewer"""
    counts = [maxc, max(1, maxc // 2), maxc, max(1, maxc - 1)][:ranks]
    return _case("tpb", slab(100 + maxc + ranks, counts, 0.2), 0.2)


def signs(octant):
    """the slab centred on the origin (None) or wholly inside one all-negative / mixed octant: negative cell indices on the chosen axes"""
    counts = (700, 0, 900, 65, 400)
    md = 0.25
    d = np.array((40.0, 40.0, 8.0)) * (1.44 * sum(counts) / 12800.0) ** (1.0 / 3.0) * md
    centre = (0, 0, 0) if octant is None else tuple(np.asarray(octant, np.float64) * (d / 2 + 3 * md))
    return _case("signs", slab(31, counts, md, centre), md)


def axis_pairs(axis):
    """near pairs that differ along ONE axis only and straddle cell 0 / -1 on it: q (block 0) just below 0, p (block 1) just above, and
    the other way round; every second pair 1.2 min_dist apart (kept).  Pairs sit 10 min_dist apart along the next axis"""
    md, n = 0.2, 40
    q, p = np.zeros((n, 3)), np.zeros((n, 3))
    rng = np.random.default_rng(7 + axis)
    for j in range(n):
        gap = (0.5 + 0.45 * rng.uniform()) * md if j % 2 == 0 else 1.2 * md
        below = -rng.uniform(0.02, 0.4) * gap
        lo, hi = below, below + gap
        q[j, axis], p[j, axis] = (lo, hi) if j % 4 < 2 else (hi, lo)
        q[j, (axis + 1) % 3] = p[j, (axis + 1) % 3] = 10 * md * (j - n // 2)
    expect = [np.ones(n, bool), np.arange(n) % 2 == 1]
    return _case("signs", [f4(q), f4(p, n)], md, expect=expect)


def neighbour_cells():
    """one near pair for each of the 26 cells around a cell: q (block 0) 0.1 of the edge inside its cell towards offset o, p (block 1)
    0.1 of the edge inside the cell at o, so they are 0.2 |o| edges apart and p is dropped -- through that one cell of the 27 and no
    other.  The pairs sit 5 cells apart along x, around cell 0 (both signs of the index)"""
    md = 0.25
    h, inv_h = mr.cell_edge(md)
    offs = mr.NEIGHBOURS[np.abs(mr.NEIGHBOURS).sum(1) > 0]
    base = np.zeros((26, 3))
    base[:, 0] = 5 * (np.arange(26) - 13)
    q = ((base + 0.5 + 0.4 * offs) * float(h)).astype(F)
    p = ((base + 0.5 + 0.6 * offs) * float(h)).astype(F)
    assert np.array_equal(mr.cell_of(p, inv_h) - mr.cell_of(q, inv_h), offs)
    return _case("signs", [f4(q), f4(p, 26)], md, expect=[np.ones(26, bool), np.zeros(26, bool)])


def chain(ranks, lines=1):
    """points on a line 0.6 min_dist apart, point j in block j: 0 is kept, 1 is dropped by 0, 2 is near 1 only and 1 is gone, so 2 is
    kept, ... -- the verdicts alternate along a dependency chain as long as the job.  lines > 1: every block holds that many such lines
    (5 min_dist apart in y), more than one wave's worth, so the wait crosses waves"""
    md = 0.25
    blocks = []
    for j in range(ranks):
        xyz = np.zeros((lines, 3))
        xyz[:, 0] = 0.6 * md * j - 3.0
        xyz[:, 1] = 5 * md * (np.arange(lines) - lines // 2)
        blocks.append(f4(xyz, j * lines))
    expect = [np.full(lines, j % 2 == 0) for j in range(ranks)]
    return _case("chain", blocks, md, expect=expect)


def square_root_to(target, above):
    """a float32 dx whose ROUNDED square is the float32 closest to `target` on the asked side (>= target if above, else <= target), and that
    square: fl(dx * dx) does not reach every float32, so the caller checks what it got"""
    r = F(np.sqrt(np.float64(target)))
    cand = [r]
    for _ in range(6):
        cand = [np.nextafter(cand[0], F(0))] + cand + [np.nextafter(cand[-1], F(np.inf))]
    cand = np.array(cand, F)
    sq = (cand.astype(np.float64) ** 2).astype(F)
    ok = sq >= target if above else sq <= target
    i = np.nonzero(ok)[0][0 if above else -1]
    return cand[i], sq[i]


def thresholds(min_dist):
    """AXIS-ALIGNED pairs (dy = dz = 0, q.x = 0): dx = p.x - 0 is exact and d2 = fl(dx * dx) is ONE rounding, the same in numpy and on
    the device -- so these pairs are EXEMPT from the undecidable count although they sit on the thresholds: their arithmetic is exact by
    construction.  d2: 0 (a duplicate across blocks: kept), the largest reachable square <= FLT_EPSILON (kept), the smallest above it
    (dropped), the largest below lim (dropped), lim itself where it is a float32 (0.5^2: kept, the comparison is strict), the smallest
    reachable square >= lim (kept).  Pair j sits at y = 10 min_dist j; q in block 0, p in block 1"""
    lim = float(F(min_dist)) ** 2
    eps = mr.FLT_EPSILON
    want = [("zero", F(0), F(0), True)]
    dx, sq = square_root_to(eps, False); want.append(("at_eps", dx, sq, True))
    dx, sq = square_root_to(np.nextafter(eps, F(1)), True); want.append(("above_eps", dx, sq, False))
    below = F(lim) if float(F(lim)) < lim else np.nextafter(F(lim), F(0))
    dx, sq = square_root_to(below, False); want.append(("below_lim", dx, sq, False))
    if float(F(lim)) == lim:
        dx, sq = square_root_to(F(lim), True); want.append(("at_lim", dx, sq, True))
    above = np.nextafter(below, F(1)) if float(F(lim)) != lim else np.nextafter(F(lim), F(1))
    dx, sq = square_root_to(above, True); want.append(("above_lim", dx, sq, True))
    n = len(want)
    q, p = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for j, (_, dx, _, _) in enumerate(want):
        q[j, 1] = p[j, 1] = F(10 * min_dist * j)
        p[j, 0] = dx
    c = _case("thresholds", [f4(q), f4(p, n)], min_dist, expect=[np.ones(n, bool), np.array([w[3] for w in want])])
    c["exempt"] = {((1, j), (0, j)) for j in range(n)}
    c["pairs"] = [(w[0], float(w[2])) for w in want]
    return c


FACE_CELLS = (8000, 17000, 100000, 8191, 16383, 32767, 65535, 131071, 262143, 524287, 1048575)
FACE_DRAWS = 200000


@functools.lru_cache(None)
def face_search(min_dist):
    """Pairs just under min_dist apart along x across the face between cells c and c + 1 (and mirrored at -c), FACE_DRAWS draws per index
    and sign; of those the reference calls near, how far apart the float32 cell restatement puts them.  Returns (searched, widest gap,
    kept pairs (q.x, p.x): per index and sign the 4 near pairs with the widest gap, the longest among equals)"""
    rng = np.random.default_rng(5)
    h, inv_h = mr.cell_edge(min_dist)
    lim = float(F(min_dist)) ** 2
    searched, widest, pairs = 0, 0, []
    for c in FACE_CELLS:
        for sign in (1.0, -1.0):
            q = (sign * (c + rng.uniform(0.99, 1.0, FACE_DRAWS)) * float(h)).astype(F)
            p = (q.astype(np.float64) + sign * rng.uniform(0.98, 1.0, FACE_DRAWS) * min_dist).astype(F)
            d = (p - q).astype(np.float64)
            d2 = (d * d).astype(F)
            ok = np.nonzero(mr.near(d2, lim))[0]
            if not ok.size:                          # (min_dist is below the spacing of the coordinates there: no near pair exists)
                continue
            gap = np.abs(mr.cell_of(p[ok], inv_h) - mr.cell_of(q[ok], inv_h))
            searched += int(ok.size)
            widest = max(widest, int(gap.max()))
            best = ok[np.lexsort((d2[ok], gap))[-4:]]
            pairs += [(q[i], p[i]) for i in best]
    return searched, widest, pairs


def face_pairs(min_dist):
    _, _, pairs = face_search(min_dist)
    n = len(pairs)
    q, p = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for j, (qx, px) in enumerate(pairs):
        q[j, 0], p[j, 0] = qx, px
        q[j, 1] = p[j, 1] = F(10 * min_dist * j)
    return _case("far", [f4(q), f4(p, n)], min_dist, expect=[np.ones(n, bool), np.zeros(n, bool)])


def _cells_where(pred, cap, reach, count, seed, spread=2):
    """`count` cells of [-reach, reach)^3, no two of them neighbours, whose keys satisfy pred(home slot)"""
    cand = np.stack(np.meshgrid(*[np.arange(-reach, reach)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pool = cand[pred(mr.home_slot(mr.cell_key(cand), cap))]
    rng = np.random.default_rng(seed)
    picked = []
    for c in pool[rng.permutation(pool.shape[0])]:
        if all(np.abs(c - o).max() >= spread for o in picked):
            picked.append(c)
            if len(picked) == count:
                return np.array(picked)
    raise AssertionError("no such set of cells")


def cells_case(cells, min_dist=0.25):
    """one point of block 0 in every given cell (at 0.1 of the edge from its low corner); block 1 puts a point 0.3 of the edge further
    along x into every even cell (near: dropped) and one at 0.9 of the edge on every axis into every odd cell (1.39 edges away: kept);
    block 2 repeats block 1's dropped points a little higher in z: near block 0's point (dropped) whatever became of block 1's"""
    h, inv_h = mr.cell_edge(min_dist)
    cells = np.asarray(cells, np.float64)
    n = cells.shape[0]
    even = np.arange(n) % 2 == 0
    b0 = (cells + 0.1) * float(h)
    b1 = np.where(even[:, None], (cells + (0.4, 0.1, 0.1)) * float(h), (cells + 0.9) * float(h))
    b2 = ((cells + (0.4, 0.1, 0.25)) * float(h))[even]
    blocks = [f4(b0), f4(b1, n), f4(b2, 2 * n)]
    got = mr.point_cells(blocks, min_dist)             # the float32 points are in the cells they were meant for
    want = np.concatenate([cells, cells, cells[even]]).astype(np.int64)
    assert np.array_equal(got, want), "a point left its cell"
    return _case("hash", blocks, min_dist, expect=[np.ones(n, bool), ~even, np.zeros(int(even.sum()), bool)])


def hash_wrap():
    cap = 1024
    c = cells_case(_cells_where(lambda s: s >= cap - 2, cap, 40, 16, 3))
    c["certify"] = {"cap": cap, "wrapped": True, "max_home_at_least": 2}
    return c


def hash_one_home():
    cap = 1024
    c = cells_case(_cells_where(lambda s: s == 500, cap, 60, 24, 4))
    c["certify"] = {"cap": cap, "max_home_at_least": 24}
    return c


def hash_alias():
    """A (block 0) and B (block 1) sit in cells whose x indices differ by exactly 2^21: one key, one bucket, 2^21 cells apart -- B is
    kept.  D (block 1) is near A and dropped; C (block 2) is near B and dropped: both buckets' candidates are looked at, distances decide"""
    md = 1.0
    h, inv_h = mr.cell_edge(md)
    a = np.array([0.3, 0.3, 0.3], F)
    bx = F((2 ** 21 + 0.3) * float(h))
    for _ in range(64):
        if mr.cell_of(bx, inv_h) - mr.cell_of(a[0], inv_h) == 2 ** 21:
            break
        bx = np.nextafter(bx, F(0) if mr.cell_of(bx, inv_h) > 2 ** 21 else F(np.inf))
    b = np.array([bx, 0.3, 0.3], F)
    d = a + np.array([0.5, 0, 0], F)
    cpt = b + np.array([0, 0.5, 0], F)
    blocks = [f4([a]), f4([b, d], 1), f4([cpt], 3)]
    c = _case("hash", blocks, md, expect=[np.array([True]), np.array([True, False]), np.array([False])])
    c["certify"] = {"alias": True}
    return c


def hash_filter():
    """about 20 k points over about 14 k occupied cells: among the ~10^5 empty cells the points probe, chance alone sets the filter bit of
    hundreds (the `continue` behind the probe), and some of those probes go on past an occupied home slot"""
    counts = (6000, 0, 7000, 500, 6500)
    c = _case("hash", slab(17, counts, 0.2), 0.2)
    c["certify"] = {"false_positives_at_least": 100, "longest_miss_at_least": 1}
    return c


def span_above():
    """256 ranks, one block of 16 385 points, 40 blocks of a few dozen, the rest empty: stride 16 385, span 4 194 560 > 2^22 -- the
    epoch itself takes the per-block launches"""
    rng = np.random.default_rng(23)
    counts = [0] * 256
    counts[3] = 16385
    for r in rng.choice(np.arange(4, 256), 40, replace=False):
        counts[int(r)] = int(rng.integers(20, 60))
    # the small blocks are dense among themselves AND against the large one: every one of them has something to decide
    md = 0.2
    big = slab(29, [16385], md)[0]
    small_total = sum(counts) - 16385
    d = np.abs(big[:, :3]).max(0)
    pts = (rng.uniform(-1, 1, (small_total, 3)) * d * 0.5).astype(F)
    blocks, s = [], 0
    for r, n in enumerate(counts):
        if r == 3:
            blocks.append(big)
        else:
            blocks.append(f4(pts[s:s + n], 16385 + s)); s += n
    c = _case("span", blocks, md, 16385)
    c["certify"] = {"span_above": True}
    return c


def no_rule(kind):
    some = slab(41, (300, 200, 150, 0, 100), 0.2)
    if kind == "min_dist_zero":
        return _case("no_rule", some, 0.0)
    if kind == "one_block_of_five":
        return _case("no_rule", [np.zeros((0, 4), F)] * 2 + [some[0]] + [np.zeros((0, 4), F)] * 2, 0.2)
    if kind == "all_empty":
        return _case("no_rule", [np.zeros((0, 4), F)] * 4, 0.2, stride=8)
    if kind == "one_rank":
        return _case("no_rule", [some[0]], 0.2)
    raise KeyError(kind)


def _far(where, md):
    c = ragged("max+1", min_dist=md, centre=where, seed=13)
    c["group"] = "far"
    return c


BUILDERS = {
    "ragged_stride_max": lambda: ragged("max"),
    "ragged_stride_max_plus_1": lambda: ragged("max+1"),
    "ragged_stride_4096": lambda: ragged("4096"),
    "ragged_first_block_empty": lambda: ragged("max+1", first_empty=True),
    **{f"tpb_maxc_{m}_ranks_{r}": (lambda m=m, r=r: tpb_edge(m, r)) for m, r in
       ((1, 2), (63, 3), (64, 4), (65, 2), (255, 3), (256, 4), (257, 3))},
    "signs_origin": lambda: signs(None),
    **{"signs_octant_" + "".join("n" if s < 0 else "p" for s in o): (lambda o=o: signs(o)) for o in
       ((-1, -1, -1), (-1, 1, 1), (1, -1, 1), (1, 1, -1))},
    "axis_pairs_y": lambda: axis_pairs(1),
    "axis_pairs_z": lambda: axis_pairs(2),
    "neighbour_cells_26": neighbour_cells,
    "chain_4": lambda: chain(4),
    "chain_16": lambda: chain(16),
    "chain_64": lambda: chain(64),
    "chain_64_lines_70": lambda: chain(64, 70),
    "thresholds_0.5": lambda: thresholds(0.5),
    "thresholds_0.3": lambda: thresholds(0.3),
    "far_3km_0.3": lambda: _far((-3000.0, 2500.0, 40.0), 0.3),
    "far_3km_0.05": lambda: _far((-3000.0, 2500.0, 40.0), 0.05),
    "far_60km_0.3": lambda: _far((60000.0, -60000.0, 0.0), 0.3),
    "far_60km_0.05": lambda: _far((60000.0, -60000.0, 0.0), 0.05),
    "face_pairs_0.3": lambda: face_pairs(0.3),
    "face_pairs_0.05": lambda: face_pairs(0.05),
    "hash_wrap": hash_wrap,
    "hash_one_home": hash_one_home,
    "hash_alias": hash_alias,
    "hash_filter": hash_filter,
    "span_above_2_22": span_above,
    **{"no_rule_" + k: (lambda k=k: no_rule(k)) for k in ("min_dist_zero", "one_block_of_five", "all_empty", "one_rank")},
}
NAMES = list(BUILDERS)


@functools.lru_cache(None)
def case(name):
    c = BUILDERS[name]()
    c["name"] = name
    return c


@functools.lru_cache(None)
def reference(name):
    """(kept masks, merged set, undecidable pairs) of a case: computed once, shared by the tests, never changed"""
    c = case(name)
    masks, merged, und = mr.merge(c["blocks"], c["min_dist"])
    merged.setflags(write=False)
    return masks, merged, und
