"""float64 numpy restatement of the outlier-filter chain and of the minimiser's pair sums, for ONE iteration of the registration loop
(CPU only).  Inputs are what that iteration worked on: its matches (ids, d2: (n, k), original map indices, +inf / -1 unfilled), the float32
queries p = T_used * (reading - mean) as the matcher formed them, the centred float32 map, map / reading normals, map / reading scalars,
T_used, and the d2 of the earlier iterations the robust scale is carried over from.

Binary decisions the device takes in float32 on float32 data are restated in float32 and are exact: d2 <= prm * prm, d2 >= prm * prm,
d2 <= limit (limit = the quantile element, or factor * median rounded once), v > prm, v < prm.  Everything else is float64: robust
functions, scale estimators and their recurrence, the point-to-plane residual, the rotated reading normal, soft weights, every product of
the sums.  Parameters and Bergstrom's constants enter as the float32 values the configuration holds, the robust scale -- state of the loop,
checked on its own against the float64 estimate -- as the float32 the state holds, scale^2 and tuning^2 as their float32 products.

Two decisions cannot be restated exactly -- SurfaceNormal's dot > cos(maxAngle) and the robust cut-offs e2 >= k2 / e2 >= apx^2, whose left
sides are float32 expressions of several roundings.  Pairs within UND_DOT of the cosine, or UND_REL relative of a cut-off, are returned as
UNDECIDABLE: their weight may be either side's, and a case may hold at most max(2, 1e-5 * pairs) of them.

The bar for pair sums.  The oracle (and the device) form the per-pair quantities F = (p x n, n) and (p - q) . n in float32 and accumulate
their products in double; this reference forms them in float64.  tests/test_weights_reference.py measures the largest
|oracle - reference| / sum |w * term| over all entries of A and b and all its cases:
    measured 7.122e-09  (60 000 x 6 000 scene as built and turned about a skew axis, 22 chains covering every filter type, k = 1 and k = 3;
    met on the turned scene, chain gen-ref-hard, k = 1).  On the scene as built the distance is exactly 0: its planes are axis-aligned,
    the map normals have one component +-1 and two zeros, and every float32 product of F and of the residual is exact -- which is why the
    measurement needs the turned scene, and why the device's distance on the as-built scenes of the GPU cases sits far below the bar.
SUMS_REL is eight times that -- the device forms the same float32 products but may contract them into FMAs -- to two digits (8 x 7.122e-09 = 5.70e-08).
The CPU test asserts the measured value stays below SUMS_REL / 8 and that the bar is sharp (one pair of weight >= 0.5 dropped, or two
weights that differ by >= 0.5 exchanged, among 6 000 pairs moves an entry by more than 10 * SUMS_REL of its scale).

Undecidable pairs per GPU case (CPU replay of iterations 1 - 4 on the oracle's matches, test_weights_reference.py): 0 in every case but the
SurfaceNormal ones, the robust cut-offs and `approximation` included; see UNDECIDABLE_SEEN below."""
import numpy as np

import match_reference as mr

MEASURED_SUMS_REL = 7.13e-9
SUMS_REL = 5.7e-8
UND_REL = 1e-5
UND_DOT = 1e-6
# the most undecidable pairs any iteration of a case showed in the CPU replay, by case id (cases not named: 0)
UNDECIDABLE_SEEN = {}

MAXDIST, MINDIST, MEDIAN, TRIMMED, SURFACENORMAL, GENERIC, ROBUST, VARTRIMMED = 1, 2, 3, 4, 5, 6, 7, 8
GEN_READING, GEN_SOFT, GEN_LARGER = 1, 2, 4
CAUCHY, WELSCH, SC, GM, TUKEY, HUBER, L1, STUDENT = range(8)
SCALE_NONE, SCALE_MAD, SCALE_BERG, SCALE_STD = 0, 1, 2, 3
BERG_K = {CAUCHY: np.float32(4.3040), TUKEY: np.float32(7.0589), HUBER: np.float32(2.0138)}


def f32(x):
    return np.float32(x)


def _o(o, i, default=0.0):
    return o[i] if len(o) > i else default


def max_undecidable(pairs):
    return max(2, int(1e-5 * pairs))


# ------------------------------------------------------------------------------------------------------------------ limits and scales
def median_limit(d2, factor):
    """MedianDistOutlierFilter: factor * median, one float32 rounding"""
    return float(f32(factor) * f32(mr.trimmed_quantile(d2, 0.5)))


def var_trimmed_ratio(d2, min_ratio, max_ratio, lam):
    """optimizeInlierRatio by brute force (tests/golden/make_recalled.py): the valid d2 sorted, FRMS(i) = cum(i) / ((i + 1) ((i + 1) / N)^(2 lam))
    in float64 over floor(minRatio N) <= i < min(floor(maxRatio N), V), N = every entry; the first minimum; ratio = i / N in float32"""
    v = np.asarray(d2, dtype=np.float32).ravel()
    N = v.size
    s = np.sort(v[np.isfinite(v) & (v > 0)]).astype(np.float64)
    if s.size == 0:
        return -1.0
    lo = int(np.floor(f32(min_ratio) * f32(N))); hi = min(int(np.floor(f32(max_ratio) * f32(N))), s.size)
    best = lo
    if hi > lo:
        i = np.arange(lo, hi, dtype=np.float64) + 1.0
        frms = np.cumsum(s)[lo:hi] / (i * (i / N) ** (2.0 * float(f32(lam))))
        best = lo + int(np.argmin(frms))
    return float(f32(best) / f32(N))


def scale_estimate(kind, d2, tuning=0.0):
    """RobustOutlierFilter's scale from one iteration's d2, float64: mad = sqrt(median |d2 - median d2|) over the finite entries (rank
    size / 2), std = (sum (d - mean)^2 / (size - 1))^(1/4) over EVERY entry (NaN with an infinite one), berg's first = 1.9 sqrt(median of
    the finite positive entries, rank (float32) size * 0.5)"""
    v = np.asarray(d2, dtype=np.float32).ravel().astype(np.float64)
    if kind == SCALE_NONE:
        return 1.0
    if kind == SCALE_MAD:
        fin = np.sort(v[np.isfinite(v)])
        med = fin[fin.size // 2]
        return float(np.sqrt(np.sort(np.abs(fin - med))[fin.size // 2]))
    if kind == SCALE_STD:
        if not np.isfinite(v).all():
            return float("nan")
        return float((((v - v.mean()) ** 2).sum() / (v.size - 1)) ** 0.25)
    if kind == SCALE_BERG:
        return 1.9 * float(np.sqrt(np.float64(mr.trimmed_quantile(d2, 0.5))))
    raise ValueError(kind)


def robust_scale(o, j, d2_of):
    """the scale iteration j (1-based) evaluates its weights with.  d2_of(i) = the d2 of iteration i.  The estimate is refreshed while
    i <= nbIterationForScale (always when that is 0) and kept afterwards; berg: estimate at iteration 1, then
    scale <- 0.85 (scale - tuning) + tuning at every refreshing iteration"""
    kind = (int(_o(o, 2)) >> 4) & 15
    nb = int(_o(o, 3))
    last = j if nb == 0 else min(j, nb)
    if kind == SCALE_BERG:
        s = scale_estimate(kind, d2_of(1))
        t = float(f32(o[1]))
        for _ in range(last - 1):
            s = 0.85 * (s - t) + t
        return s
    return scale_estimate(kind, d2_of(last))


def robust_weight(fct, e2, kk, k2=None):
    """the eight M-estimators of e2 with tuning kk (k2: its square as the caller holds it); returns (w, the cut-off its branch compares
    e2 with, or None)"""
    k2 = kk * kk if k2 is None else k2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if fct == CAUCHY: return 1.0 / (1.0 + e2 / k2), None
        if fct == WELSCH: return np.exp(-e2 / k2), None
        if fct == SC: return np.where(e2 >= kk, 4.0 * k2 / (kk + e2) ** 2, 1.0), kk
        if fct == GM: return k2 / (kk + e2) ** 2, None
        if fct == TUKEY: return np.where(e2 >= k2, 0.0, (1.0 - e2 / k2) ** 2), k2
        if fct == HUBER: return np.where(e2 >= k2, kk / np.sqrt(e2), 1.0), k2
        if fct == L1: return 1.0 / np.sqrt(e2), None
        return (1.0 + e2 / kk) ** (-(kk + 3.0) / 2.0) * (kk + 3.0) / (kk + e2), None


# ------------------------------------------------------------------------------------------------------------------ the chain
def chain_weights(outliers, ids, d2, p, map_c, map_normals=None, read_normals=None, T_used=None, map_scalar=None, read_scalar=None,
                  iteration=1, d2_of=None, scale_state=None):
    """Weights of one iteration.  scale_state: the float32 robust scale the loop state held in this iteration, once the caller has checked
    it against robust_scale() -- the weights are functions of the residual and of THAT number; without it the float64 estimate rounded to
    float32 stands in.  The two constants every pair of the iteration shares, scale^2 and tuning^2, are the float32 products of those float32
    values (like prm * prm of MaxDist): their rounding is no per-pair noise that averages out of a sum, it moves every weight the same way.
  Returns dict(w (n, k) float64 -- undecidable decisions taken as float64 takes them --, w_alt (n, k): the
    same with every undecidable decision PASSED (an upper bound of the pair's weight), und (n, k) bool, limits {filter slot: float},
    scale (float64 or None), vt_ratio).  An unfilled slot (d2 = +inf) weighs 0 as in the pair-sum kernel."""
    d2 = np.asarray(d2, dtype=np.float32); ids = np.asarray(ids)
    n, k = d2.shape
    valid = np.isfinite(d2) & (ids >= 0)
    sid = np.where(valid, ids, 0)
    w = valid.astype(np.float64); w_alt = w.copy()
    und = np.zeros((n, k), bool)
    limits, scale, vt_ratio = {}, None, -1.0
    if d2_of is None:
        d2_of = lambda i: d2
    P = np.asarray(p, dtype=np.float32)[:, None, :3].astype(np.float64)

    def both(m):
        nonlocal w, w_alt
        w = w * m; w_alt = w_alt * m

    for f, o in enumerate(outliers):
        t, prm = int(o[0]), f32(o[1])
        if t == MAXDIST: both(d2 <= prm * prm)
        elif t == MINDIST: both(d2 >= prm * prm)
        elif t in (MEDIAN, TRIMMED, VARTRIMMED):
            if t == TRIMMED: lim = mr.trimmed_quantile(d2, float(prm))
            elif t == MEDIAN: lim = median_limit(d2, prm)
            else:
                vt_ratio = var_trimmed_ratio(d2, prm, _o(o, 3), _o(o, 4))
                lim = mr.trimmed_quantile(d2, vt_ratio)
            limits[f] = lim
            both(d2 <= f32(lim))
        elif t == SURFACENORMAL:
            a = np.asarray(read_normals, dtype=np.float32).astype(np.float64)
            if T_used is not None:
                a = a @ np.asarray(T_used, dtype=np.float32).astype(np.float64)[:3, :3].T
            b = np.asarray(map_normals, dtype=np.float32).astype(np.float64)[sid]
            dot = (a[:, None, :] * b).sum(-1)
            c = np.cos(float(prm))
            u = valid & (np.abs(dot - c) <= UND_DOT)
            w = w * (dot > c); w_alt = w_alt * ((dot > c) | u)
            und |= u
        elif t == GENERIC:
            ip = int(_o(o, 2))
            v = np.broadcast_to(np.asarray(read_scalar, dtype=np.float32)[:, None], (n, k)) if ip & GEN_READING else np.asarray(map_scalar, dtype=np.float32)[sid]
            both(v.astype(np.float64) if ip & GEN_SOFT else ((v > prm) if ip & GEN_LARGER else (v < prm)))
        elif t == ROBUST:
            ip = int(_o(o, 2))
            fct, kind, plane = ip & 15, (ip >> 4) & 15, ((ip >> 8) & 15) == 1
            scale = robust_scale(o, iteration, d2_of)
            kk = float(BERG_K.get(fct, prm) if kind == SCALE_BERG else prm)
            res = d2.astype(np.float64)
            if plane:
                q = np.asarray(map_c, dtype=np.float32)[sid][..., :3].astype(np.float64)
                nn = np.asarray(map_normals, dtype=np.float32).astype(np.float64)[sid]
                res = (((P - q) * nn).sum(-1)) ** 2
            with np.errstate(invalid="ignore", divide="ignore"):
                s_used = f32(scale if scale_state is None else scale_state)
                e2 = np.where(valid, res, 0.0) / float(s_used * s_used)
            rw, cut = robust_weight(fct, e2, kk, float(f32(kk) * f32(kk)))
            rw = np.where(valid & ~(rw <= 0.0), rw, 0.0)
            u = np.zeros((n, k), bool)
            if cut is not None:   # (continuous at the cut-off except for the pair count: tukey reaches 0 there)
                u |= np.abs(e2 - cut) <= UND_REL * cut
            apx = float(f32(_o(o, 4)))
            ra = rw
            if apx > 0 and np.isfinite(apx):
                ua = np.abs(e2 - apx * apx) <= UND_REL * apx * apx
                rw = np.where(e2 >= apx * apx, 0.0, rw)
                ra = np.where(ua, ra, rw)
                u |= ua
            w = w * rw; w_alt = w_alt * np.maximum(ra, rw)
            und |= u & valid
        else:
            raise ValueError(t)
    und &= w_alt != 0     # a pair some exact filter of the chain rejects is decided
    w_alt = np.where(und, w_alt, w)
    return dict(w=w, w_alt=w_alt, und=und, limits=limits, scale=scale, vt_ratio=vt_ratio)


# ------------------------------------------------------------------------------------------------------------------ pair sums
def pair_terms(minimizer, p, map_c, map_normals, ids, force_2d=False):
    """(n, k, 32) float64: the term every pair contributes to entry e of the sums per unit weight, in icpmi_minimize_step's layout:
    point-to-plane [0..20] A upper triangle row-major, [21..26] b; point-to-point [0] 1, [1..3] p, [4..6] q, [7 + 3c + r] q_r p_c; always
    [27] 1 (sum w), [28] 1 (counted where w != 0: see pair_sums); force2D [29..31] b of the 2-D residual"""
    ids = np.asarray(ids)
    n, k = ids.shape
    sid = np.maximum(ids, 0)
    P = np.broadcast_to(np.asarray(p, dtype=np.float32)[:, None, :3].astype(np.float64), (n, k, 3))
    Q = np.asarray(map_c, dtype=np.float32)[sid][..., :3].astype(np.float64)
    t = np.zeros((n, k, 32))
    t[..., 27] = 1.0; t[..., 28] = 1.0
    if minimizer == 2:
        N = np.asarray(map_normals, dtype=np.float32).astype(np.float64)[sid]
        F = np.concatenate([np.cross(P, N), N], axis=-1)
        d = P - Q
        dot = (d * N).sum(-1)
        e = 0
        for a in range(6):
            for b in range(a, 6):
                t[..., e] = F[..., a] * F[..., b]; e += 1
            t[..., 21 + a] = -F[..., a] * dot
        if force_2d:
            dot2 = d[..., 0] * N[..., 0] + d[..., 1] * N[..., 1]
            for a in range(3):
                t[..., 29 + a] = -F[..., 2 + a] * dot2
    elif minimizer == 1:
        t[..., 0] = 1.0
        t[..., 1:4] = P; t[..., 4:7] = Q
        for c in range(3):
            for r in range(3):
                t[..., 7 + 3 * c + r] = Q[..., r] * P[..., c]
    return t


def pair_sums(w, terms):
    """(sums (32,), abs (32,)): sum w * term and sum |w * term| over the pairs with w != 0; [28] counts them"""
    w = np.asarray(w, dtype=np.float64)
    used = (w != 0) & np.isfinite(w)
    wt = np.where(used, w, 0.0)[..., None] * terms
    sums = wt.sum((0, 1)); ab = np.abs(wt).sum((0, 1))
    sums[28] = ab[28] = float(used.sum())
    return sums, ab


def undecidable_slack(res, terms):
    """(32,): what the undecidable pairs may add to or take from every entry -- their own |w * term| at the larger of their two weights"""
    return (np.where(res["und"], res["w_alt"], 0.0)[..., None] * np.abs(terms)).sum((0, 1))


def count_bounds(res):
    """(lo, hi) of the number of pairs with w != 0: the decided ones, plus every undecidable one"""
    lo = int(((res["w"] != 0) & ~res["und"]).sum())
    return lo, lo + int(res["und"].sum())


# ------------------------------------------------------------------------------------------------------------------ the step
def rodrigues(x):
    th = np.linalg.norm(x[:3])
    T = np.eye(4)
    if th > 0:
        kx = x[:3] / th
        K = np.array([[0, -kx[2], kx[1]], [kx[2], 0, -kx[0]], [-kx[1], kx[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = x[3:]
    return T


def step_from_sums(minimizer, sums, force_2d=False):
    """float64 weighted solve from the pair sums: point-to-plane x = A^-1 b through the angle-axis of x[:3] (force2D: the (yaw, tx, ty)
    sub-system with the 2-D b); point-to-point the weighted Kabsch step"""
    s = np.asarray(sums, dtype=np.float64)
    if minimizer == 2:
        A = np.zeros((6, 6)); e = 0
        for a in range(6):
            for b in range(a, 6):
                A[a, b] = A[b, a] = s[e]; e += 1
        if force_2d:
            x3 = np.linalg.solve(A[2:5, 2:5], s[29:32])
            return rodrigues(np.array([0, 0, x3[0], x3[1], x3[2], 0.0]))
        return rodrigues(np.linalg.solve(A, s[21:27]))
    W = s[0]
    mp, mq = s[1:4] / W, s[4:7] / W
    H = np.array([[s[7 + 3 * c + r] for c in range(3)] for r in range(3)]) - W * np.outer(mq, mp)   # H[r, c] = sum w (q - mq)_r (p - mp)_c
    U, _, Vt = np.linalg.svd(H)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        U[:, -1] *= -1; R = U @ Vt
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = mq - R @ mp
    return T
