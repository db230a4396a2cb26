"""The lane exchanges of the ICP iteration's tail kernels (csrc/common.h: wave_incl_scan, lane_xor): the rank finder's prefix sums
(block_find_rank256: the last level inside accumulate_kernel in registers, level 0 in sel2_scan_hist_kernel by shuffles) and the
transposed butterfly of the pair sums (accumulate_kernel's fold, pair_sums_fold) on DPP / permlane swaps.  A value taken from the wrong
lane moves a sum or a selected bin outright, so the checks are exact wherever the arithmetic is.

1. One live pair: of n = 600 reading points (three 256-thread pair-sum workgroups of 200 slots each; two 1024-thread ones at knn 3) exactly
   one, at position p, has a map point within maxDist.  icpmi_minimize_step's sums must hold that pair's products -- formed from the
   kernel's own float32 terms, exact in float64 -- to within 2^-40 absolute (the resolution of the fixed-point limbs a workgroup's sum
   joins the accumulator in, csrc/common.h: ICPMI_ACC_*), and every other entry must be exactly 0.
2. Full sums at counts around the wave and the workgroup: against float64 (tests/weights_reference.py) with the bar of
   tests/test_gpu_loop_weights.py, SUMS_REL * sum |w term|.
3. The rank finder at the wave seams: 4096 distances whose selected element has, at both radix levels, its coarse and its fine bin on a
   thread next to a wave boundary (0, 63, 64, 127, 128, 191, 192, 255).  The limit is one element of the multiset: bitwise against
   tests/selection_reference.py on the distances the device itself selected over, and the seam property is asserted on those.
   The coarse bin of level 0 is the float's top byte -- sign and seven exponent bits --, so positive values reach threads 0 .. 127 only and
   squared distances inside a matcher radius of 2 m threads 0 .. 64: level 0's coarse seams are 0, 63 and 64; the other three bytes take all
   eight seams.  A squared distance is the float32 square of a float32 offset (the central anchor of selection_cases' lattice: exact), which
   about half of all bit patterns are, so a case names the admissible bytes and the first pattern that is a square is used."""
import itertools

import numpy as np
import pytest

import selection_cases as sc
import selection_reference as sr
import weights_reference as wr

pytestmark = pytest.mark.gpu

F = np.float32
POSITIONS = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 257, 599)
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)
SEAMS = (0, 63, 64, 127, 128, 191, 192, 255)
QUANTUM = 2.0 ** -40
#         id            minimizer knn  entries of the model
CONFIGS = {"p2p": (1, 1, 16), "p2plane": (2, 1, 27), "p2plane_knn3": (2, 3, 27)}


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


_handles = {}


def handle(amd, minimizer, knn, per_anchor):
    """a handle without outlier filters on selection_cases' lattice (mean exactly 0: the centred frame is the caller's)"""
    key = (minimizer, knn, per_anchor)
    if key not in _handles:
        mp, nm = sc.lattice_map(per_anchor)
        icp = amd.ICPSequence(minimizer=minimizer, knn=knn, max_dist=sc.MAX_DIST, outliers=[])
        assert icp.setMap(mp, nm)
        assert np.array_equal(icp.getMapMean(), np.zeros(3, F))
        _handles[key] = (icp, mp, nm)
    return _handles[key]


def anchor_of(i):
    """(index into lattice_map(1), coordinates) of the positive-octant anchor reading point i sits at"""
    a = sc.POSITIVE_ANCHORS[i % sc.POSITIVE_ANCHORS.shape[0]]
    idx = int(np.nonzero((sc.lattice_anchors() == a).all(1))[0][0])
    return idx, a


def near_reading(n, seed):
    """(reading (n, 4), anchor index per point): every point 0.1 .. 0.5 m off its anchor on every axis -- no coordinate of p or of p - q near 0"""
    rng = np.random.default_rng(seed)
    off = (rng.uniform(0.1, 0.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    ids = np.empty(n, np.int64)
    rd = np.ones((n, 4), F)
    for i in range(n):
        ids[i], a = anchor_of(i)
        rd[i, :3] = a.astype(F) + off[i]
    return rd, ids


def pair_products(minimizer, p, q, nrm):
    """the 32 entries one pair of weight 1 adds, from the float32 terms accumulate_kernel forms (no contraction: -ffp-contract=off); every
    product below is one of two float32 numbers in float64, hence exact"""
    p, q, nrm = p.astype(F), q.astype(F), nrm.astype(F)
    e = np.zeros(32)
    e[27] = e[28] = 1.0
    if minimizer == 1:
        e[0] = 1.0
        e[1:4] = p; e[4:7] = q
        for c in range(3):
            for r in range(3):
                e[7 + 3 * c + r] = float(q[r]) * float(p[c])
        return e
    Fv = np.array([F(p[1] * nrm[2]) - F(p[2] * nrm[1]), F(p[2] * nrm[0]) - F(p[0] * nrm[2]), F(p[0] * nrm[1]) - F(p[1] * nrm[0]), nrm[0], nrm[1], nrm[2]], F)
    d = (p - q).astype(F)
    dot = F(F(F(d[0] * nrm[0]) + F(d[1] * nrm[1])) + F(d[2] * nrm[2]))
    idx = 0
    for a in range(6):
        for b in range(a, 6):
            e[idx] = float(Fv[a]) * float(Fv[b]); idx += 1
        e[21 + a] = -(float(Fv[a]) * float(dot))
    return e


# ------------------------------------------------------------------------------------------------------------------ 1. one live pair
@pytest.mark.parametrize("cid", list(CONFIGS))
def test_one_live_pair(amd, cid):
    minimizer, knn, nval = CONFIGS[cid]
    icp, mp, nm = handle(amd, minimizer, knn, 1)     # one map point per anchor: at knn 3 the second and third neighbours are 8 m away
    n = 600
    near, ids = near_reading(n, 11)
    far = np.ones((n, 4), F)
    for i in range(n):
        far[i, :3] = (anchor_of(i)[1] + sc.FAR).astype(F)     # 6.9 m from the nearest map point
    for pos in POSITIONS:
        rd = far.copy()
        rd[pos] = near[pos]
        _, sums = icp.minimizeStep(rd, np.eye(4))
        want = pair_products(minimizer, rd[pos, :3], mp[ids[pos], :3], nm[ids[pos]])
        live = np.zeros(32, bool)
        live[:nval] = True; live[27:29] = True
        assert not want[~live].any() and (want[:nval] != 0).sum() >= 8, (cid, pos, want)
        err = np.abs(sums - want)
        print(f"{cid} p={pos}: largest |sums - products| = {err.max():.3e} (2^-40 = {QUANTUM:.3e}), pairs {icp.stats.pairs}")
        assert icp.stats.pairs == 1 and sums[28] == 1.0 and sums[27] == 1.0, (cid, pos, icp.stats.pairs, sums[27], sums[28])
        assert (err[live] <= QUANTUM).all(), (cid, pos, np.nonzero(err > QUANTUM)[0].tolist(), sums.tolist(), want.tolist())
        assert not sums[~live].any(), (cid, pos, "entries outside the model", sums[~live].tolist())
        # a product that is exactly 0 (an axis-aligned normal) stays exactly 0: nothing arrived from another lane
        assert not sums[live & (want == 0)].any(), (cid, pos, sums.tolist())


# ------------------------------------------------------------------------------------------------------------------ 2. full sums
@pytest.mark.parametrize("cid", list(CONFIGS))
def test_full_sums(amd, cid):
    minimizer, knn, nval = CONFIGS[cid]
    icp, mp, nm = handle(amd, minimizer, knn, knn)   # knn coincident map points per anchor: every slot of every query is live
    for n in COUNTS:
        rd, aid = near_reading(n, 100 + n)
        _, sums = icp.minimizeStep(rd, np.eye(4))
        ids = aid[:, None] * knn + np.arange(knn)[None, :]
        terms = wr.pair_terms(minimizer, rd, mp, nm, ids)
        ref, rabs = wr.pair_sums(np.ones((n, knn)), terms)
        err = np.abs(sums - ref)
        tol = wr.SUMS_REL * rabs
        tol[28] = 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(rabs > 0, err / rabs, 0.0)
        print(f"{cid} n={n}: pairs {icp.stats.pairs}, largest |device - float64| / sum |w term| = {rel.max():.3e} (entry {int(rel.argmax())}), bar {wr.SUMS_REL:.1e}")
        assert icp.stats.pairs == n * knn == sums[28], (cid, n, icp.stats.pairs, sums[28])
        bad = np.nonzero(~(err <= tol))[0]
        assert bad.size == 0, (cid, n, bad.tolist(), sums[bad].tolist(), ref[bad].tolist())


# ------------------------------------------------------------------------------------------------------------------ 3. rank finder at the seams
def root_of(pattern):
    """a float32 s with float32(s * s) == the pattern, or None"""
    v = sc.from_bits(np.array([pattern], np.uint32))[0]
    s0 = F(np.sqrt(np.float64(v)))
    for s in (s0, np.nextafter(s0, F(0)), np.nextafter(s0, F(np.inf)), np.nextafter(np.nextafter(s0, F(0)), F(0)), np.nextafter(np.nextafter(s0, F(np.inf)), F(np.inf))):
        if s > 0 and sc.ibits(F(s * s)) == pattern:
            return F(s)
    return None


def first_square(b3s, b2s, b1s, b0s):
    for b3, b2, b1, b0 in itertools.product(b3s, b2s, b1s, b0s):
        pat = (b3 << 24) | (b2 << 16) | (b1 << 8) | b0
        if 0 < pat <= sc.ibits(3.9):
            s = root_of(pat)
            if s is not None:
                return pat, s
    raise AssertionError("no admissible pattern is a float32 square")


ANY3 = (63, 62, 61, 60, 59, 58)     # level 0's coarse bin away from a seam: the other three bytes are the case
# (all-v: the last byte is v where that is a square -- 0x3f000000 and its like, odd powers of two, are none -- else the next seam)
SEAM_CASES = [(f"all-{v}", ANY3, (v,), (v,), (v,) + tuple(x for x in SEAMS if x != v)) for v in SEAMS] + [
    ("top-63", (63,), SEAMS, (64, 191), (127, 192)),
    ("top-64", (64,), (0, 63, 64, 127), (255, 128), (0, 63)),
    ("top-0", (0,), (64, 63, 127, 128, 191, 192, 255), (191, 0, 255), (63, 64, 128)),
    ("mixed-a", ANY3, (255,), (0,), (128, 127)),
    ("mixed-b", ANY3, (0,), (255,), (191, 192)),
    ("mixed-c", ANY3, (127, 128), (63, 64), (0, 255)),
]
N_SEAM, N_BALLAST, N_PREFIX, N_TIES = 4096, 240, 600, 3


def seam_reading(case):
    """(reading (4096, 4), ratio, the selected pattern): offsets along the axes at the central anchor (d2 = float32(s * s), exact), ballast
    0.25 m off the other anchors for the solve"""
    cid, b3s, b2s, b1s, b0s = case
    pat, sT = first_square(b3s, b2s, b1s, b0s)
    rng = np.random.default_rng(pat % 100003)
    s = [np.full(N_TIES, sT, F)]
    # the nearest squares on both sides: the bins next to the selected one at level 1, over the seam where the selected bin is 0 or 255
    lo, hi = sT, sT
    for _ in range(6):
        lo, hi = np.nextafter(lo, F(0)), np.nextafter(hi, F(np.inf))
        s += [np.full(4, lo, F), np.full(2, hi, F)]
    # the selected 16-bit prefix, spread over level 1's 256 coarse bins
    lo16, hi16 = pat & 0xFFFF0000, pat | 0xFFFF
    inpre = np.sqrt(sc.from_bits(rng.integers(max(lo16, 1), hi16 + 1, N_PREFIX, dtype=np.uint32)).astype(np.float64)).astype(F)
    s.append(inpre)
    # level 0: log-uniform offsets, six octaves of d2 below the selected value and what fits under the matcher's radius above it
    rest = N_SEAM - N_BALLAST - sum(x.size for x in s)
    nb = rest * 4 // 5
    s.append((float(sT) * np.exp2(rng.uniform(-3.0, 0.0, nb))).astype(F))
    top = min(float(sT) * 8.0, 1.97)
    s.append((float(sT) * np.exp2(rng.uniform(0.0, np.log2(top / float(sT)), rest - nb))).astype(F) if top > float(sT) * 1.0001 else np.full(rest - nb, sT, F))
    s = np.concatenate(s)[rng.permutation(N_SEAM - N_BALLAST)]
    rd = np.ones((N_SEAM, 4), F)
    rd[:s.size, :3] = s[:, None] * sc.AXES[np.arange(s.size) % 3].astype(F)
    rd[s.size:] = sc.place(np.full(N_BALLAST, sc.BALLAST), central=np.zeros(N_BALLAST, bool), mirror=False)
    rd = rd[rng.permutation(N_SEAM)]
    # the distances as the matcher forms them, to aim the rank: the test asserts the property on the device's own
    d2 = np.r_[(s * s).astype(F), np.full(N_BALLAST, sc.BALLAST, F)]
    srt = sr.sorted_bits(d2)
    at = np.nonzero(srt == pat)[0]
    assert at.size >= N_TIES, (cid, hex(pat), at.size)
    return rd, sc.ratio_for_rank(srt.size, int(at[at.size // 2])), pat


def seam_bytes(pattern):
    return (pattern >> 24, (pattern >> 16) & 255, (pattern >> 8) & 255, pattern & 255)


@pytest.mark.parametrize("case", SEAM_CASES, ids=[c[0] for c in SEAM_CASES])
def test_rank_finder_at_wave_seams(amd, case):
    import torch
    cid, b3s, b2s, b1s, b0s = case
    rd, ratio, pat = seam_reading(case)
    mp, nm = sc.lattice_map(1)
    icp = amd.ICPSequence(minimizer=1, knn=1, max_dist=sc.MAX_DIST, outliers=[(sr.TRIMMED, ratio)], max_iterations=40, use_differential=0)
    assert icp.setMap(mp, nm)
    icp.keepSums(1)
    d = torch.from_numpy(rd).cuda()
    icp.registerDev(d.data_ptr(), N_SEAM, fixed_iterations=1)
    _, d2, T_used = icp.lastMatches()
    sums, limits, _, _ = icp.lastSums()
    assert np.array_equal(T_used, np.eye(4, dtype=F))
    ref = sr.quantile(d2, ratio)
    got = seam_bytes(sc.ibits(ref))
    print(f"{cid}: selected {sc.ibits(ref):#010x} (aimed at {pat:#010x}), level 0 threads {got[0]} / {got[1]}, level 1 threads {got[2]} / {got[3]}, "
          f"limit {float(limits[0])!r}, pairs {icp.stats.pairs}")
    # the property, on the distances the device selected over
    assert got[0] in b3s and got[1] in b2s and got[2] in b1s and got[3] in b0s, (cid, got)
    assert all(g in SEAMS for g in got[1:]) and (got[0] in SEAMS or b3s is ANY3), (cid, got)
    srt = sr.sorted_bits(d2)
    assert srt.size == N_SEAM and np.unique(srt >> 16).size > 100 and np.unique(srt[(srt >> 16) == (sc.ibits(ref) >> 16)] >> 8).size > 100, cid
    assert np.array([limits[0]], F).view(np.uint32)[0] == sc.ibits(ref), (cid, "limits[slot]", float(limits[0]), float(ref))
    assert np.array([icp.stats.trimmed_limit], F).view(np.uint32)[0] == sc.ibits(ref), (cid, "stats.trimmed_limit", float(icp.stats.trimmed_limit), float(ref))
    assert sums[28] == icp.stats.pairs == int((d2 <= ref).sum()), (cid, sums[28], icp.stats.pairs, int((d2 <= ref).sum()))
    icp.close()
