"""Distance sets built to break the quantile selection of the outlier-filter chain (select.hip, nn.hip's level 0, loop.hip's last level,
common.h's rank lookups), for tests/test_selection_cpu.py and tests/test_gpu_selection_edges.py.  CPU only, plain numpy, one fixed seed
per set.

ARRAYS: named generators of (n, k) float32 arrays of squared distances.  Every case carries the ratio its TrimmedDist filter runs at, a
one-line statement of the property it guarantees and a function that asserts that property on the array handed to it -- the tests call
it on the array they use, so a case cannot silently lose its edge.

LOOP: the same sets as geometry, for the fused selection that only runs behind a matcher launch.  The map is a lattice of anchors 8 m
apart, symmetric about the origin (its mean is exactly 0: the centred frame is the caller's frame), every anchor k coincident map points
(a cluster of k: all k distances of a query are the bits of one float32 expression); a reading point is an anchor plus an offset along
one axis whose length is the square root of the wanted distance.  Offsets that must survive bit for bit (ties 2 ulp apart, denormal
squares, the low end of the wide sets) sit at the central anchor, where anchor + offset is exact; the other anchors carry what tolerates
the rounding of the sum.  Unless a case says otherwise a reading holds every point's eight mirror images, so that the point-to-point
step is the identity up to rounding and later iterations see the distances of the first.  Exact ties come from repeated reading points.
"""
import math

import numpy as np

RATIOS = (0.7, 0.85, 0.9, 0.95, 0.99)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
MAX_DIST = 2.0
INF = np.float32(np.inf)


# ------------------------------------------------------------------------------------------------------------------ ranks and bits
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ibits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def valid_sorted_bits(d2):
    """the multiset the selection works on: bit patterns of the finite positive entries, ascending"""
    v = np.asarray(d2, dtype=np.float32).ravel()
    return np.sort(bits(v[np.isfinite(v) & (v > 0)]))


def rank32(total, q):
    """getDistsQuantile's index: the float32 product, truncated"""
    if np.float32(q) == np.float32(1.0):
        return total - 1
    return min(int(np.float32(total) * np.float32(q)), total - 1)


def rank_exact(total, q):
    """the same index in exact arithmetic (a 24-bit by 24-bit product is exact in float64)"""
    if np.float32(q) == np.float32(1.0):
        return total - 1
    return min(int(float(total) * float(np.float32(q))), total - 1)


def ratio_for_rank(total, rank):
    """a float32 ratio whose float32 rank over `total` values is `rank`"""
    q = np.float32((rank + 0.5) / total)
    assert 0 < q < 1 and rank32(total, q) == rank, (total, rank, q)
    return float(q)


def float_rank_totals(multiple=48, limit=70_000):
    """{ratio: totals <= limit} where the float32 rank is not the exact rank, total and rank multiples of `multiple` (a loop case has
    k copies of every value: the rank must open a group for an off-by-one rank to change the bits)"""
    out = {}
    for q in RATIOS:
        out[q] = [t for t in range(multiple, limit + 1, multiple) if rank32(t, q) != rank_exact(t, q) and rank32(t, q) % multiple == 0]
    return out


# ------------------------------------------------------------------------------------------------------------------ the array cases
class Case:
    def __init__(self, cid, ratio, statement, make, check, invalid=False, vt=False):
        self.id, self.ratio, self.statement, self._make, self._check, self.invalid, self.vt = cid, float(ratio), statement, make, check, invalid, vt

    def make(self, k):
        """(n, k) float32"""
        flat = np.ascontiguousarray(self._make(k), dtype=np.float32).ravel()
        pad = (-flat.size) % k
        if pad:
            flat = np.r_[flat, np.full(pad, INF, np.float32)]
        return np.ascontiguousarray(flat.reshape(-1, k))

    def check(self, d2):
        """asserts the statement on d2"""
        self._check(np.asarray(d2, dtype=np.float32), self.ratio)


def _sel(d2, ratio):
    s = valid_sorted_bits(d2)
    return s, rank32(s.size, ratio)


def _log_uniform(rng, count, lo, hi):
    return np.exp2(rng.uniform(math.log2(lo), math.log2(hi), count)).astype(np.float32)


SMALLEST_NORMAL = float(np.finfo(np.float32).tiny)


def _all_equal():
    def make(k): return np.full(5000 * k, 0.37, np.float32)
    def check(d2, r):
        s, _ = _sel(d2, r)
        assert s.size >= 5000 and s[0] == s[-1]
    return [Case("all_equal", 0.85, "one positive value everywhere", make, check, vt=True)]


def _two_values():
    lo = ibits(0.3); hi = lo + 2
    out = []
    for name, where in (("inside", None), ("first_of_second", 0), ("last_of_first", -1)):
        def make(k, where=where):
            total = 6000 * k
            n1 = total // 2 if where is None else rank32(total, 0.85) - where
            v = np.r_[np.full(n1, lo, np.uint32), np.full(total - n1, hi, np.uint32)]
            np.random.default_rng(101).shuffle(v)
            return from_bits(v)
        def check(d2, r, where=where):
            s, rk = _sel(d2, r)
            assert set(np.unique(s).tolist()) == {lo, hi}
            n1 = int((s == lo).sum())
            if where is None: assert n1 < rk and n1 > 1000
            elif where == 0: assert rk == n1 and s[rk] == hi and s[rk - 1] == lo
            else: assert rk == n1 - 1 and s[rk] == lo and s[rk + 1] == hi
        out.append(Case(f"two_values-{name}", 0.85, "two values 2 ulp apart; the rank inside the second group / on its first / on the first group's last element",
                        make, check, vt=name == "inside"))
    return out


def _one_prefix():
    out = []
    for nbits, top in ((16, 0x3E9A0000), (24, 0x3E9A5500)):
        span = 1 << (32 - nbits)
        def make(k, top=top, span=span):
            return from_bits(np.uint32(top) + np.random.default_rng(102).integers(0, span, 7001 * k, dtype=np.uint32))
        def check(d2, r, nbits=nbits, top=top, span=span):
            s, _ = _sel(d2, r)
            assert ((s >> (32 - nbits)) == (top >> (32 - nbits))).all()
            assert np.unique(s).size > min(span, s.size) // 3     # the low bits are spread
        out.append(Case(f"one_prefix{nbits}", 0.7, f"every value shares the top {nbits} bits, the low bits are spread", make, check))
    return out


def _prefix_boundary():
    edge = 0x3F000000   # 0.5: the top 8 bits change from 0x3E to 0x3F
    out = []
    for side, ratio in (("below", 0.4), ("above", 0.6)):
        def make(k):
            rng = np.random.default_rng(103)
            half = 3000 * k
            return from_bits(np.r_[edge - 1 - rng.integers(0, 1 << 16, half, dtype=np.uint32), edge + rng.integers(0, 1 << 16, half, dtype=np.uint32)].astype(np.uint32)[rng.permutation(2 * half)])
        def check(d2, r, side=side):
            s, rk = _sel(d2, r)
            t8 = s >> 24
            assert set(np.unique(t8).tolist()) == {0x3E, 0x3F} and int(s.max() - s.min()) < (1 << 17)
            assert t8[rk] == (0x3E if side == "below" else 0x3F)
        out.append(Case(f"prefix_boundary-{side}", ratio, "values within 2^16 bit patterns of 0.5 on both sides (the top 8 bits change there); the rank " + side, make, check))
    return out


def wide_values(count, seed=104):
    return _log_uniform(np.random.default_rng(seed), count, SMALLEST_NORMAL, 3.0)


def check_wide(d2, r, ascending):
    s, _ = _sel(d2, r)
    v = from_bits(s).astype(np.float64)
    assert math.log2(v[-1] / v[0]) >= 60
    assert math.log2(v[int(0.9 * v.size)] / v[int(0.1 * v.size)]) > 32    # most values lie more than a 4096-bin window apart
    if ascending:
        flat = np.asarray(d2).ravel()
        flat = flat[np.isfinite(flat)]
        assert (np.diff(flat) >= 0).all()


def _wide():
    out = []
    for name in ("shuffled", "ascending"):
        def make(k, name=name):
            v = wide_values(20_011 * k)
            return np.sort(v) if name == "ascending" else v
        out.append(Case(f"wide-{name}", 0.85, "log-uniform over more than 60 octaves, from the smallest normal float32 to 3 (" + name + ")", make,
                        lambda d2, r, name=name: check_wide(d2, r, name == "ascending"), vt=name == "shuffled"))
    return out


TINY_TOP = 0x00040000   # bit patterns below this have top 16 bits 0..3 (all denormal)
NEAR_ONE = 0x3F800000


def _tiny():
    def make(k): return from_bits(np.random.default_rng(105).integers(1, TINY_TOP, 6007 * k, dtype=np.uint32))
    def check(d2, r):
        s, _ = _sel(d2, r)
        assert s.size >= 6007 and s[-1] < TINY_TOP and s[0] < (1 << 16)
    out = [Case("tiny", 0.85, "every value has top 16 bits 0..3 (denormals), some have top 16 bits 0", make, check)]
    for name, where in (("first_of_cluster", 0), ("last_tiny", -1)):
        def make(k, where=where):
            rng = np.random.default_rng(106)
            total = 6000 * k
            n1 = rank32(total, 0.5) - where
            v = np.r_[rng.integers(1, TINY_TOP, n1, dtype=np.uint32), NEAR_ONE - 0x8000 + rng.integers(0, 0x10000, total - n1, dtype=np.uint32)].astype(np.uint32)
            return from_bits(v[rng.permutation(total)])
        def check(d2, r, where=where):
            s, rk = _sel(d2, r)
            n1 = int((s < TINY_TOP).sum())
            assert n1 > 1000 and (s[n1:] >= NEAR_ONE - 0x8000).all() and s.size - n1 > 1000
            assert rk == n1 + (0 if where == 0 else -1)
        out.append(Case(f"tiny_mixed-{name}", 0.5, "denormals and a cluster near 1.0, the rank on the " + name.replace("_", " ") + " value", make, check))
    return out


def _mostly_invalid():
    def make(k):
        rng = np.random.default_rng(107)
        total = 20_000 * k
        v = _log_uniform(rng, total, 1e-3, 1.0)
        bad = rng.permutation(total)[: total * 9 // 10]
        v[bad[::2]] = INF
        v[bad[1::2]] = 0.0
        return v
    def check(d2, r):
        s, _ = _sel(d2, r)
        assert 0 < s.size * 10 <= d2.size + 10 and (d2 == 0).sum() > d2.size // 3 and np.isinf(d2).sum() > d2.size // 3
    out = [Case("mostly_invalid", 0.85, "90 % inf or exactly 0, 10 % valid", make, check, vt=True)]
    for name, val in (("all_inf", INF), ("all_zero", np.float32(0))):
        out.append(Case(name, 0.85, "no valid value", lambda k, val=val: np.full(300 * k, val, np.float32),
                        lambda d2, r: _assert(valid_sorted_bits(d2).size == 0), invalid=True))
    return out


def _assert(c):
    assert c


def ascending_distinct(count):
    return from_bits(np.uint32(0x3C000000) + np.uint32(16) * np.arange(count, dtype=np.uint32))


def float_rank_picks():
    """[(ratio, total)]: the smallest, a middle and the largest total of float_rank_totals() per ratio that has any"""
    out = []
    for q, ts in float_rank_totals().items():
        if ts:
            out += [(q, ts[0]), (q, ts[len(ts) // 2]), (q, ts[-1])]
    return out


def loop_float_rank_picks(limit=20_000):
    """[(ratio, total)]: per ratio the smallest total and the largest one up to `limit`"""
    out = []
    for q, ts in float_rank_totals(limit=limit).items():
        if ts:
            out += [(q, ts[0]), (q, ts[-1])]
    return out


def _float_rank():
    out = []
    for q, total in [(0.7, 10)] + float_rank_picks():
        def check(d2, r, total=total):
            s, rk = _sel(d2, r)
            assert s.size == total and rk == rank_exact(total, r) + 1 and (np.diff(s.astype(np.int64)) > 0).all()
            flat = np.asarray(d2).ravel()
            assert (np.diff(flat[:total]) > 0).all()
        out.append(Case(f"float_rank-{q}-{total}", q, "distinct values ascending by index; the float32 rank is the exact rank + 1", lambda k, total=total: ascending_distinct(total), check))
    return out


def _sizes():
    out = []
    for size in SIZES:
        def make(k, size=size): return _log_uniform(np.random.default_rng(108 + size), size, 1e-4, 1.0)
        def check(d2, r, size=size): assert valid_sorted_bits(d2).size == size
        out.append(Case(f"size-{size}", 0.85, f"{size} valid values", make, check, vt=size in (2047, 2048, 2049)))
    def make(k): return _log_uniform(np.random.default_rng(109), 3 * 2048 + 1, 1e-4, 1.0)
    out.append(Case("size-6145", 0.85, "3 x 2048 + 1 valid values", make, lambda d2, r: _assert(valid_sorted_bits(d2).size == 6145), vt=True))
    return out


ARRAYS = _all_equal() + _two_values() + _one_prefix() + _prefix_boundary() + _wide() + _tiny() + _mostly_invalid() + _float_rank() + _sizes()
ARRAY_IDS = [c.id for c in ARRAYS]


def array_case(cid):
    return ARRAYS[ARRAY_IDS.index(cid)]


# ------------------------------------------------------------------------------------------------------------------ the loop cases
SPACING = 8.0
AXES = np.eye(3)


def lattice_anchors():
    g = [(SPACING * i, SPACING * j, SPACING * l) for i in range(-2, 3) for j in range(-2, 3) for l in range(-1, 2)]
    return np.array(g, dtype=np.float64)


def lattice_map(k):
    """(map (75 k, 4) float32, normals (75 k, 3) float32): k coincident points per anchor; the normal of a cluster is the axis
    (i + j + l) mod 3 of its lattice index"""
    a = lattice_anchors()
    idx = np.rint(a / SPACING).astype(np.int64).sum(1) % 3
    pts = np.ones((a.shape[0] * k, 4), np.float32)
    pts[:, :3] = np.repeat(a, k, axis=0)
    return pts, np.ascontiguousarray(np.repeat(AXES[idx], k, axis=0), dtype=np.float32)


POSITIVE_ANCHORS = np.array([(SPACING * i, SPACING * j, SPACING * l) for i in range(3) for j in range(3) for l in range(2)][1:], dtype=np.float64)
FAR = np.array([4.0, 4.0, 4.0])     # offset of a point with no map point within MAX_DIST


def place(w, central=None, mirror=True, repeat=1):
    """reading (N, 4) float32 for the wanted squared distances w: point i = anchor + sqrt(w_i) e_(i mod 3); w_i = inf -> a point with no
    match, w_i = 0 -> the anchor itself.  central: bool mask of the points that go to the central anchor (default: w < 1e-6); the others
    cycle over the anchors of the positive octant.  mirror: all eight sign images of every point, in the points' order.  repeat: every
    point that many times."""
    w = np.asarray(w, dtype=np.float32)
    n = w.size
    if central is None:
        central = w < 1e-6
    a = np.where(np.asarray(central)[:, None], 0.0, POSITIVE_ANCHORS[np.arange(n) % POSITIVE_ANCHORS.shape[0]])
    s = np.sqrt(np.where(np.isfinite(w), w, 0).astype(np.float64)).astype(np.float32)
    off = s[:, None].astype(np.float64) * AXES[np.arange(n) % 3]
    off = np.where(np.isfinite(w)[:, None], off, FAR)
    p = (a.astype(np.float32) + off.astype(np.float32)).astype(np.float32)     # one float32 sum, as the reading holds it
    if mirror:
        signs = np.array([(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float32)
        p = (p[:, None, :] * signs[None, :, :]).reshape(-1, 3)
    if repeat > 1:
        p = np.repeat(p, repeat, axis=0)
    out = np.ones((p.shape[0], 4), np.float32)
    out[:, :3] = p
    return out


class LoopCase:
    """reading(k) -> (N, 4); ratio(k); check(d2, ratio, first): asserts the property on the distances the device selected over -- first:
    the first iteration (the distances as built), otherwise what survives a pose that is the identity up to rounding"""
    def __init__(self, cid, statement, reading, ratio, check, minimizer=1, T_init=None, ks=(1, 6, 16), invalid=False):
        self.id, self.statement, self.reading, self._ratio, self.check, self.minimizer, self.T_init, self.ks, self.invalid = cid, statement, reading, ratio, check, minimizer, T_init, ks, invalid

    def ratio(self, k):
        return float(self._ratio(k)) if callable(self._ratio) else float(self._ratio)


BALLAST = np.float32(0.0625)     # offset 0.25 m: exact at every anchor


def _ties_at_rank(d2, ratio, least):
    s, rk = _sel(d2, ratio)
    assert int((s == s[rk]).sum()) >= least, (int((s == s[rk]).sum()), least)
    return s, rk


def _loop_cases():
    out = []
    # --- one value: 0.25 = 0.5^2, exact at every anchor
    def check(d2, r, first):
        s, rk = _ties_at_rank(d2, r, 8)
        if first: assert s[0] == s[-1] == ibits(0.25)
    out.append(LoopCase("all_equal", "one value, 0.25, at every point (first iteration); later at least 8 bit-equal values at the rank",
                        lambda k: place(np.full(600, 0.25, np.float32), central=np.zeros(600, bool), repeat=8), 0.85, check))

    # --- two values 2 ulp apart at the central anchor (0.5^2 and (0.5 + 2^-24)^2), under them ballast at the other anchors for the solve
    lo, hi = np.float32(0.25), np.float32(0.25) + np.float32(2.0 ** -24)
    assert ibits(hi) - ibits(lo) == 2 and np.float32(np.sqrt(np.float64(hi))) ** 2 == hi
    NB, NLO, NHI, REP = 240, 90, 90, 4
    def two_reading(k):
        w = np.r_[np.full(NB, BALLAST), np.full(NLO, lo), np.full(NHI, hi)].astype(np.float32)
        return place(w, central=np.r_[np.zeros(NB, bool), np.ones(NLO + NHI, bool)], repeat=REP)
    for name, where in (("first_of_second", 0), ("last_of_first", -1)):
        def ratio(k, where=where):
            return ratio_for_rank(8 * REP * k * (NB + NLO + NHI), 8 * REP * k * (NB + NLO) + where)
        def check(d2, r, first, where=where):
            s, rk = _ties_at_rank(d2, r, 4 * REP)      # (a central point on an axis has two distinct mirror images, each four times per repeat)
            if first:
                assert set(np.unique(s).tolist()) == {ibits(BALLAST), ibits(lo), ibits(hi)}
                if where == 0: assert s[rk] == ibits(hi) and s[rk - 1] == ibits(lo)
                else: assert s[rk] == ibits(lo) and s[rk + 1] == ibits(hi)
        out.append(LoopCase(f"two_values-{name}", "the two largest values 2 ulp apart, the rank on the boundary between them", two_reading, ratio, check))

    # --- one 16-bit prefix: wanted values inside the middle of one prefix at every anchor (the rounding of anchor + offset moves low bits only)
    def p16_reading(k):
        b = np.uint32(0x3E9A0000) + np.random.default_rng(202).integers(0x2000, 0xE000, 2500, dtype=np.uint32)
        return place(from_bits(b), central=np.zeros(2500, bool))
    def check(d2, r, first):
        s, rk = _sel(d2, r)
        if first: assert ((s >> 16) == 0x3E9A).all() and np.unique(s).size > 1000
        else: assert ((s >> 16) == 0x3E9A).mean() > 0.9
    out.append(LoopCase("one_prefix16", "every value shares the top 16 bits", p16_reading, 0.7, check))

    # --- one 24-bit prefix at the central anchor (256 values, each many times), ballast under it
    def p24_reading(k):
        b = np.uint32(0x3E9A5500) + np.random.default_rng(203).integers(0, 256, 400, dtype=np.uint32)
        s = np.sqrt(from_bits(b).astype(np.float64)).astype(np.float32)
        w = np.r_[np.full(240, BALLAST), s * s].astype(np.float32)
        return place(w, central=np.r_[np.zeros(240, bool), np.ones(400, bool)], repeat=2)
    def check(d2, r, first):
        s, rk = _ties_at_rank(d2, r, 2 * 4)      # (a central point on an axis has four distinct mirror images, each twice)
        if first:
            top = s[s > ibits(BALLAST)]
            assert top.size >= 400 * 8 * 2 and int(top.max() - top.min()) < 1024 and np.unique(top).size > 100 and s[rk] > ibits(BALLAST)
    out.append(LoopCase("one_prefix24", "the values above the ballast lie within 1024 bit patterns: one 16-bit prefix, one or two coarse level-1 bins", p24_reading, 0.7, check))

    # --- values on both sides of 0.5 (top 8 bits 0x3E / 0x3F)
    def pb_reading(k):
        rng = np.random.default_rng(204)
        b = np.r_[0x3F000000 - 0x1000 - rng.integers(0, 0xE000, 1500, dtype=np.uint32), 0x3F000000 + 0x1000 + rng.integers(0, 0xE000, 1500, dtype=np.uint32)].astype(np.uint32)
        return place(from_bits(b[rng.permutation(3000)]), central=np.zeros(3000, bool))
    for side, ratio in (("below", 0.4), ("above", 0.6)):
        def check(d2, r, first, side=side):
            s, rk = _sel(d2, r)
            assert set(np.unique(s >> 24).tolist()) == {0x3E, 0x3F} and (s >> 24)[rk] == (0x3E if side == "below" else 0x3F)
        out.append(LoopCase(f"prefix_boundary-{side}", "values on both sides of 0.5, where the top 8 bits change; the rank " + side, pb_reading, ratio, check))

    # --- wide: the low end at the central anchor
    def wide_reading(k, ascending):
        w = wide_values(4000, seed=205)
        s = np.sqrt(w.astype(np.float64)).astype(np.float32)
        w = (s * s).astype(np.float32)
        w = w[w > 0]
        return place(np.sort(w) if ascending else w)
    def check_w(d2, r, first, ascending=False):
        s, rk = _sel(d2, r)
        v = from_bits(s).astype(np.float64)
        if first:
            assert math.log2(v[-1] / v[0]) >= 60 and math.log2(v[int(0.9 * v.size)] / v[int(0.1 * v.size)]) > 32
            if ascending:
                col = np.asarray(d2)[::8, 0].astype(np.float64)     # (anchor + offset rounds: ascending to within that rounding)
                assert (col[1:] >= col[:-1] * 0.98).all() and col[-1] > 1e30 * col[0]
        else:
            assert math.log2(v[-1] / v[0]) > 40
    out.append(LoopCase("wide-shuffled", "log-uniform over more than 60 octaves", lambda k: wide_reading(k, False), 0.85, check_w))
    out.append(LoopCase("wide-ascending", "log-uniform over more than 60 octaves, ascending by index", lambda k: wide_reading(k, True), 0.5,
                        lambda d2, r, first: check_w(d2, r, first, True)))

    # --- tiny at the central anchor: squares that are denormal, ballast above them; the rank inside the tiny group
    def tiny_w(count, seed):
        b = np.random.default_rng(seed).integers(1 << 10, TINY_TOP, count, dtype=np.uint32)
        s = np.sqrt(from_bits(b).astype(np.float64)).astype(np.float32)
        return s
    NT = 500
    def tiny_reading(k, cluster):
        s = tiny_w(NT, 206)
        p = place(np.r_[np.ones(NT, np.float32), np.full(240, cluster, np.float32)], central=np.r_[np.ones(NT, bool), np.zeros(240, bool)], mirror=False)
        p[:NT, :3] = s[:, None] * AXES[np.arange(NT) % 3].astype(np.float32)     # (the squares are not float32 numbers the offsets could be derived from)
        signs = np.array([(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float32)
        q = np.ones((p.shape[0] * 8, 4), np.float32)
        q[:, :3] = (p[:, None, :3] * signs[None, :, :]).reshape(-1, 3)
        return q
    def check_tiny(d2, r, first):
        s, rk = _sel(d2, r)
        if first: assert int((s < TINY_TOP).sum()) == 8 * NT * d2.shape[1] and s[rk] < TINY_TOP
        assert from_bits(s[rk:rk + 1])[0] < 1e-9
    out.append(LoopCase("tiny", "denormal squares at the central anchor (top 16 bits 0..3), ballast above; the rank inside the tiny group",
                        lambda k: tiny_reading(k, float(BALLAST)), lambda k: ratio_for_rank(8 * k * (NT + 240), 8 * k * NT * 6 // 10), check_tiny))
    for name, where in (("first_of_cluster", 0), ("last_tiny", -1)):
        def ratio(k, where=where): return ratio_for_rank(8 * k * (NT + 240), 8 * k * NT + where)
        def check(d2, r, first, where=where):
            s, rk = _sel(d2, r)
            v = from_bits(s)
            if where == 0: assert v[rk - 1] < 1e-9 and v[rk] > 0.5
            else: assert v[rk] < 1e-9 and v[rk + 1] > 0.5
            if first: assert int((s < TINY_TOP).sum()) == 8 * NT * d2.shape[1]
        out.append(LoopCase(f"tiny_mixed-{name}", "denormal squares and a cluster at 1.0, the rank on the " + name.replace("_", " ") + " value",
                            lambda k: tiny_reading(k, 1.0), ratio, check))

    # --- mostly invalid: 45 % without a match, 45 % exactly on an anchor
    def mi_reading(k):
        rng = np.random.default_rng(207)
        w = _log_uniform(rng, 3000, 1e-3, 1.0)
        bad = rng.permutation(3000)[:2700]
        w[bad[::2]] = INF
        w[bad[1::2]] = 0.0
        return place(w, central=np.zeros(3000, bool))
    def check(d2, r, first):
        s, _ = _sel(d2, r)
        assert s.size > 0 and np.isinf(d2).sum() > d2.size // 3
        if first: assert s.size * 10 <= d2.size + 10 and (d2 == 0).sum() > d2.size // 3
    out.append(LoopCase("mostly_invalid", "10 % valid, the rest without a match or (first iteration) exactly on a map point", mi_reading, 0.85, check))

    # --- the float32 rank: distinct ascending values, no mirror images (V = k n must be the total)
    for q, total in loop_float_rank_picks():
        def reading(k, total=total):
            n = total // k
            w = from_bits(np.uint32(0x3D000000) + np.uint32(2048) * np.arange(n, dtype=np.uint32))
            return place(w, central=np.zeros(n, bool), mirror=False)
        def check(d2, r, first, total=total):
            s, rk = _sel(d2, r)
            k = d2.shape[1]
            assert s.size == total and rk == rank_exact(total, r) + 1 and rk % k == 0
            assert s[rk] != s[rk - 1]
            if first: assert (np.diff(np.asarray(d2)[:, 0]) > 0).all()
        out.append(LoopCase(f"float_rank-{q}-{total}", "the float32 rank is the exact rank + 1 and opens a group of k equal values; first iteration: ascending by index",
                            reading, q, check))

    # --- small counts (no mirror images; three points and more: the point-to-point step needs them)
    for size in (63, 64, 65, 255, 256, 257, 2047, 2048, 2049):
        def reading(k, size=size):
            return place(_log_uniform(np.random.default_rng(300 + size), size, 1e-3, 1.0), central=np.zeros(size, bool), mirror=False)
        def check(d2, r, first, size=size): assert d2.shape[0] == size and valid_sorted_bits(d2).size == size * d2.shape[1]
        out.append(LoopCase(f"size-{size}", f"{size} queries, all matched", reading, 0.85, check))

    # --- readings that are NOT aligned (0.05 rad about z, 6 cm): the distances shrink from iteration to iteration and the selected prefix
    # leaves the window downwards.  On the CPU oracle the prefixes of iterations 2, 3, 4 at k = 6 are 15622, 15502, 15501 (point-to-point,
    # offsets of 1 cm .. 1.7 m) and 14241, 14133, 14121 (point-to-plane, offsets of 1 mm .. 1 cm under the linearisation's residual)
    def mis_reading(lo, hi):
        w = _log_uniform(np.random.default_rng(208), 2000, lo, hi)
        return place(w, central=np.zeros(w.size, bool))
    T = np.eye(4)
    c, s = math.cos(0.05), math.sin(0.05)
    T[:2, :2] = [[c, -s], [s, c]]; T[:3, 3] = [0.05, -0.03, 0.02]
    def check(d2, r, first): assert valid_sorted_bits(d2).size > d2.size // 2
    out.append(LoopCase("misaligned-p2p", "a reading 0.05 rad and 6 cm off: the distances change with every iteration", lambda k: mis_reading(1e-4, 3.0), 0.5, check,
                        T_init=T, ks=(6, 16)))
    out.append(LoopCase("misaligned-p2plane", "the same under point-to-plane, normals cycling over the axes, offsets of 1 mm .. 1 cm", lambda k: mis_reading(1e-6, 1e-4), 0.5,
                        check, minimizer=2, T_init=T, ks=(1, 6)))
    return out


LOOP = _loop_cases()
LOOP_IDS = [c.id for c in LOOP]


def loop_case(cid):
    return LOOP[LOOP_IDS.index(cid)]


def loop_reading(c, k):
    """the reading of a case as the registration receives it (moved by the case's misalignment)"""
    rd = c.reading(k)
    if c.T_init is not None:
        rd = rd.copy()
        rd[:, :3] = (rd[:, :3].astype(np.float64) @ c.T_init[:3, :3].T + c.T_init[:3, 3]).astype(np.float32)
    return np.ascontiguousarray(rd, dtype=np.float32)


def count_edge_reading(n):
    """n queries (no mirror images), wide distances ascending by index: the low end at the central anchor"""
    w = np.sort(wide_values(n, seed=209))
    s = np.sqrt(w.astype(np.float64)).astype(np.float32)
    return place((s * s).astype(np.float32), mirror=False)
