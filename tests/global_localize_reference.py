"""Integer restatement of the global localisation search (include/icpmi.h: icpmi_global_localize) in numpy, and the scene
its tests run on.  Pure numpy: nothing here touches the library.

The quantity.  Cells of side s0 in the handle's centred frame, per axis (int)floorf(x / s0) in float32, |i| < 2^19.  occ0 = the cells of
the map's points.  Rotation k of a list turns a reading point x into y = R_k x (per row fmaf(R[r][2], z, fmaf(R[r][1], y, R[r][0] * x)) in
float32) and its cell c = floorf(y / s0); score(k, a) = the number of points with c + a in occ0: the pose [R_k | mu + s0 a].
Level l's node (k, l, A) stands for the translations a in [A 2^l, A 2^l + 2^l - 1] per axis; bound(k, l, A) = the number of points with
(c >> l) + A in occB_l, where occC_l = {u >> l : u in occ0}, occB_0 = occ0 and occB_l = {w - e : w in occC_l, e in {0, 1}^3}.
bound >= the largest score in the cube, because (c + a) >> l is (c >> l) + A or that plus one per axis.
"""
import heapq
import itertools
import math

import numpy as np

import localizability_reference as lr
import voxel_reference as vr

F32 = np.float32
RANGE = 1 << 19              # |cell| < 2^19 on every axis, so that cell + offset fits the 21-bit fields of the key
BIAS = 1 << 20
TOP_CHUNK = 65536            # nodes one launch carries (icpmi_global_localize_shape says the same)
MAX_LEVELS = 8
AUTO_LEVELS_MAX = 6
E8 = np.array(list(itertools.product((0, 1), repeat=3)), np.int64)


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def fmaf(a, b, c):
    """float32 fused multiply-add, correctly rounded: the product of two float32 is exact in float64; the sum is rounded to odd in float64
    (TwoSum gives the sign of what the rounding dropped), which makes the second rounding to float32 the only one"""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, F32).astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def pack(ijk):
    """(n, 3) integer cells -> the 63-bit key, x in the top field: ascending keys are ascending (ix, iy, iz)"""
    b = np.asarray(ijk, np.int64) + BIAS
    return (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]


def unpack(keys):
    k = np.asarray(keys, np.int64)
    return np.stack([(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], 1) - BIAS


def first_slot(keys, capacity):
    """where a key's probe sequence starts (vox_hash): tests build colliding key sets from it"""
    return vr.first_slot(keys, capacity)


def capacity_of(n_keys):
    cap = 2
    while cap < 2 * n_keys:
        cap <<= 1
    return cap


def cells_of(xyz, s0):
    """(cells (n, 3) int64, taking part (n,) bool) of float32 coordinates"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor(np.asarray(xyz, F32)[:, :3] / F32(s0))
        ok = (np.abs(f) < RANGE).all(1)                      # (NaN and +-inf fail here too)
    return np.where(ok[:, None], f, 0).astype(np.int64), ok


def rotate(R, pts):
    """y = R x per row in float32 with the header's order of operations; R (3, 3) float32 as a matrix"""
    R = np.asarray(R, F32)
    p = np.asarray(pts, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([fmaf(R[r, 2], z, fmaf(R[r, 1], y, R[r, 0] * x)) for r in range(3)], 1)


def yaw_rotations(steps, roll=0.0, pitch=0.0):
    """Rz(2 pi i / steps) Ry(pitch) Rx(roll) in double -- every entry of a product summed left to right, Ry Rx first -- rounded to float32:
    (steps, 3, 3).  math.cos / math.sin: the C library's, as the host shell's"""
    cr, sr, cp, sp = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
    Rx = [[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]]
    Ry = [[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]]
    mul = lambda A, B: [[(A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]
    Ryx = mul(Ry, Rx)
    out = []
    for i in range(steps):
        a = 2.0 * math.pi * float(i) / float(steps)
        Rz = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
        out.append(np.array(mul(Rz, Ryx), np.float64).astype(F32))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------------------------ the pyramid
class Pyramid:
    """keys[l] = the ascending packed keys of occB_l for l = 0 .. levels - 1, of a centred float32 map (m, >= 3)"""

    def __init__(self, map_centred, s0, levels):
        c, ok = cells_of(map_centred, s0)
        if not ok.all():
            raise ValueError("a map point is out of the cell range")
        self.s0, self.levels = F32(s0), levels
        occ0 = np.unique(c, axis=0)
        self.cells = [occ0]
        for l in range(1, levels):
            occC = np.unique(occ0 >> l, axis=0)
            self.cells.append(np.unique((occC[:, None, :] - E8[None, :, :]).reshape(-1, 3), axis=0))
        self.keys = [np.sort(pack(c)) for c in self.cells]

    def has(self, l, ijk):
        """membership of (n, 3) cells in occB_l; a cell outside the key's fields is in no table"""
        ijk = np.asarray(ijk, np.int64)
        inside = (np.abs(ijk) < BIAS).all(1)
        k = pack(np.where(inside[:, None], ijk, 0))
        pos = np.searchsorted(self.keys[l], k)
        pos[pos >= self.keys[l].size] = 0
        return inside & (self.keys[l][pos] == k)


class Reading:
    """per rotation the cells of the reading, and per (rotation, level) the distinct shifted cells with their multiplicities"""

    def __init__(self, reading, rotations, s0):
        self.n = int(np.asarray(reading).shape[0])
        self.rot = np.asarray(rotations, F32).reshape(-1, 3, 3)
        self.cells, self.points = [], []
        for R in self.rot:
            c, ok = cells_of(rotate(R, reading), s0)
            self.cells.append(c[ok])
            self.points.append(int(ok.sum()))
        self._u = {}

    def shifted(self, k, l):
        if (k, l) not in self._u:
            self._u[(k, l)] = np.unique(self.cells[k] >> l, axis=0, return_counts=True) if self.cells[k].size else (np.zeros((0, 3), np.int64), np.zeros(0, np.int64))
        return self._u[(k, l)]


def bound(pyr, rd, k, l, A):
    """bound(k, l, A); score(k, a) at l = 0"""
    u, cnt = rd.shifted(k, l)
    return int(cnt[pyr.has(l, u + np.asarray(A, np.int64)[None, :])].sum())


def score_nodes(pyr, rd, nodes):
    """nodes (N, 5) = (k, l, Ax, Ay, Az) -> (N,) int64"""
    return np.array([bound(pyr, rd, int(q[0]), int(q[1]), q[2:5]) for q in np.asarray(nodes, np.int64)], np.int64)


def exhaustive(pyr, rd, a_min, a_max, ks=None):
    """score(k, a) over the whole window by correlation: (n_rot, nx, ny, nz) int64; ks: the rotations wanted (the others stay 0)"""
    a_min, a_max = np.asarray(a_min, np.int64), np.asarray(a_max, np.int64)
    shape = a_max - a_min + 1
    out = np.zeros((rd.rot.shape[0], *shape), np.int64)
    occ = pyr.cells[0]
    lo, hi = occ.min(0), occ.max(0)
    dense = np.zeros(hi - lo + 1, bool)
    dense[tuple((occ - lo).T)] = True
    for k in (range(rd.rot.shape[0]) if ks is None else ks):
        u, cnt = rd.shifted(k, 0)
        for c, w in zip(u, cnt):
            # cells c + a for a in the window, clipped to the dense grid
            s = c + a_min - lo                       # dense index of a = a_min
            b0 = np.maximum(0, -s)
            b1 = np.minimum(shape, np.asarray(dense.shape) - s)
            if (b1 <= b0).any():
                continue
            sl_out = tuple(slice(int(b0[j]), int(b1[j])) for j in range(3))
            sl_in = tuple(slice(int(s[j] + b0[j]), int(s[j] + b1[j])) for j in range(3))
            out[k][sl_out] += w * dense[sl_in]
    return out


# ------------------------------------------------------------------------------------------------------------------ the search
def window_of(lo, hi, mean, s0):
    """a_min, a_max of a box in the map frame, formed in double"""
    mu = np.asarray(mean, F32).astype(np.float64)
    s = float(F32(s0))
    return (np.floor((np.asarray(lo, np.float64) - mu) / s).astype(np.int64), np.floor((np.asarray(hi, np.float64) - mu) / s).astype(np.int64))


def auto_levels(a_min, a_max):
    side = int((np.asarray(a_max) - np.asarray(a_min) + 1).max())
    L = 1
    while L < AUTO_LEVELS_MAX and (1 << L) <= side:
        L += 1
    return L


def need_of(ratio, n):
    return int(np.ceil(float(F32(ratio)) * n))


def search(pyr, rd, a_min, a_max, levels, batch=64, min_score_ratio=0.0, max_nodes=0):
    """the driver: dict(found, proven, rotation, cell, score, points, levels, nodes_scored, leaves_scored, launches)"""
    a_min, a_max = np.asarray(a_min, np.int64), np.asarray(a_max, np.int64)
    L = auto_levels(a_min, a_max) if levels == 0 else levels
    best, leaf = need_of(min_score_ratio, rd.n) - 1, None
    st = dict(nodes=0, leaves=0, launches=0)
    heap = []

    def capped():
        return max_nodes > 0 and st["nodes"] > max_nodes

    def take(nodes):
        """one launch: score, then the leaves in the heap's order (strictly better only), then the inner nodes onto the heap"""
        nonlocal best, leaf
        st["launches"] += 1
        st["nodes"] += len(nodes)
        sc = score_nodes(pyr, rd, nodes)
        lv = [j for j in range(len(nodes)) if nodes[j][1] == 0]
        st["leaves"] += len(lv)
        if lv:
            i = min(lv, key=lambda j: (-sc[j], nodes[j]))
            if sc[i] > best:
                best, leaf = int(sc[i]), nodes[i]
        for q, s in zip(nodes, sc):
            if q[1] != 0 and s > best:
                heapq.heappush(heap, (-int(s), q[1], q[0], q[2], q[3], q[4]))

    t0, t1 = a_min >> (L - 1), a_max >> (L - 1)
    top = [(k, L - 1, x, y, z) for k in range(rd.rot.shape[0]) for x in range(t0[0], t1[0] + 1) for y in range(t0[1], t1[1] + 1)
           for z in range(t0[2], t1[2] + 1)]
    proven = True
    for i in range(0, len(top), TOP_CHUNK):
        take(top[i:i + TOP_CHUNK])
        if capped():
            proven = False
            break
    while proven and heap and -heap[0][0] > best:
        kids = []
        popped = 0
        while heap and popped < batch and -heap[0][0] > best:
            _, l, k, x, y, z = heapq.heappop(heap)
            popped += 1
            w = 1 << (l - 1)
            for e in E8:
                c = 2 * np.array([x, y, z]) + e
                if ((c * w + w - 1 >= a_min) & (c * w <= a_max)).all():
                    kids.append((k, l - 1, int(c[0]), int(c[1]), int(c[2])))
        take(kids)
        if capped():
            proven = False
    out = dict(found=int(leaf is not None), proven=int(proven), rotation=-1, cell=(0, 0, 0), score=0, points=0, levels=L, nodes_scored=st["nodes"],
               leaves_scored=st["leaves"], launches=st["launches"])
    if leaf is not None:
        out.update(rotation=leaf[0], cell=tuple(leaf[2:5]), score=best, points=rd.points[leaf[0]])
    return out


def pose_of(R, cell, mean, s0):
    """the (4, 4) float32 pose of a leaf: R and tau = mu + s0 a, rounded once"""
    T = np.eye(4, dtype=F32)
    T[:3, :3] = np.asarray(R, F32)
    T[:3, 3] = (np.asarray(mean, F32).astype(np.float64) + float(F32(s0)) * np.asarray(cell, np.float64)).astype(F32)
    return T


# ------------------------------------------------------------------------------------------------------------------ the scene
S0 = 0.5
YAW_STEPS = 64
WINDOW = ((-7, -22, -3), (6, 21, 2))            # not aligned to any block, on purpose: 14 x 44 x 6 cells, 236 544 leaves with 64 rotations
SENSOR, YAW = np.array([0.4, 1.0, 1.2]), 0.7


# what the prototype found (the issue's figures; tests/test_global_localize_cpu.py reproduces them): the only maximiser, the runner-up's score,
# and (levels, batch) -> (nodes scored, launches)
BEST = dict(score=1424, rotation=7, cell=(1, 1, 0), points=1428)
RUNNER_UP = 1359
LEAVES = 236544
COUNTS = {(3, 1): (7432, 162), (3, 64): (7432, 5), (3, 1024): (22528, 3), (4, 1): (3656, 370), (4, 64): (3656, 8), (4, 1024): (20256, 4),
          (0, 1): (5192, 1906), (0, 64): (5192, 31), (0, 1024): (21792, 6), (1, 1): (LEAVES, 4), (1, 64): (LEAVES, 4), (1, 1024): (LEAVES, 4)}
KEYS = (1235, 627, 144, 63)


def box_points(rng, k):
    """a 1.2 x 1.2 x 1.6 m box on the floor: top and three sides"""
    lo, hi = np.array([-1.75, 2.0, 0.0]), np.array([-0.55, 3.2, 1.6])
    out = []
    for _ in range(k):
        f = rng.integers(0, 4)
        u, v = rng.random(2)
        if f == 0:
            p = [lo[0] + u * (hi[0] - lo[0]), lo[1] + v * (hi[1] - lo[1]), hi[2]]
        elif f == 1:
            p = [hi[0], lo[1] + u * (hi[1] - lo[1]), v * hi[2]]
        elif f == 2:
            p = [lo[0] + u * (hi[0] - lo[0]), lo[1], v * hi[2]]
        else:
            p = [lo[0] + u * (hi[0] - lo[0]), hi[1], v * hi[2]]
        out.append(p)
    return np.array(out)


_cache = {}


def scene():
    """dict(map (8600, 4) float32, reading (1428, 4) float32 in the sensor frame, rotations (64, 3, 3)): the room with a box that breaks its
    symmetries, seen from SENSOR under YAW.  Generated once; callers must not write into the arrays."""
    if "scene" not in _cache:
        sc = lr.scene("room")
        rng = np.random.default_rng(5)
        mp = np.concatenate([sc["map"][:, :3].astype(np.float64), box_points(rng, 600)])
        world = np.concatenate([sc["reading"][:, :3].astype(np.float64), box_points(rng, 150)])
        world = world[np.linalg.norm(world - SENSOR, axis=1) < 7.0]
        R = lr.make_T((0, 0, YAW), SENSOR)[:3, :3]
        reading = ((world - SENSOR) @ R).astype(F32)
        f4 = lambda a: np.concatenate([a, np.ones((a.shape[0], 1))], 1).astype(F32)
        out = dict(map=f4(mp), reading=f4(reading), rotations=yaw_rotations(YAW_STEPS))
        for a in out.values():
            a.setflags(write=False)
        _cache["scene"] = out
    return _cache["scene"]


def scene_inputs(mean=None, levels=4):
    """the scene in a handle's centred frame: (Pyramid, Reading, mean)"""
    sc = scene()
    m = vr.map_mean(sc["map"]) if mean is None else np.asarray(mean, F32)
    key = (tuple(m.tolist()), levels)
    if key not in _cache:
        _cache[key] = (Pyramid(vr.centred(sc["map"], m), S0, levels), Reading(sc["reading"], sc["rotations"], S0), m)
    return _cache[key]
