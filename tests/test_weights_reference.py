"""tests/weights_reference.py is right before it judges the device (tests/test_gpu_loop_weights.py): its weights against the oracle's stage
call for every filter type at k = 1 and k = 3, its pair sums against the oracle's A and b for the same weights -- which is where SUMS_REL
comes from --, the sharpness of that bar, and the undecidable-pairs condition of every GPU case on the oracle's matches."""
import ctypes as C
import math

import numpy as np
import pytest

import loop_weights_cases as lwc
import weights_reference as wr
from loop_weights_cases import LARGER, READING, SOFT, gen, rob

U = 2.0 ** -24
# a soft weight is a float32 expression of at most eight roundings (residual, scale^2 with the scale's own rounding twice, the quotient, the
# function) whose condition in e2 is at most 1 for every function used here, or the descriptor value itself: 16 u of max(w, 1)
SOFT_REL = 16 * U

CHAINS = {
    "maxdist": [(wr.MAXDIST, 0.6)], "mindist": [(wr.MINDIST, 0.3)], "median": [(wr.MEDIAN, 1.5)], "trimmed": [(wr.TRIMMED, 0.7)],
    "two-quantiles": [(wr.TRIMMED, 0.9), (wr.MEDIAN, 2.5)],
    "vartrimmed": [(wr.VARTRIMMED, 0.05, 0, 0.99, 0.95)],
    "surfacenormal": [(wr.SURFACENORMAL, 0.9), (wr.TRIMMED, 0.85)],
    "gen-ref-hard": [gen(0.5, LARGER)], "gen-ref-smaller": [gen(0.5, 0)], "gen-ref-soft": [gen(0.0, SOFT)],
    "gen-read-hard": [gen(0.4, READING | LARGER)], "gen-read-soft": [gen(0.0, READING | SOFT), (wr.TRIMMED, 0.85)],
    "cauchy-mad": [rob("cauchy", 1.2, "mad")], "welsch-std": [rob("welsch", 1.2, "std"), (wr.TRIMMED, 0.85)],
    "sc-none": [rob("sc", 0.02)], "gm-none": [rob("gm", 0.05)], "tukey-berg-apx": [rob("tukey", 0.05, "berg", approximation=3.0)],
    "huber-mad-plane": [rob("huber", 1.2, "mad", dist="point2plane")], "huber-berg": [rob("huber", 0.05, "berg")],
    "cauchy-berg-plane": [rob("cauchy", 0.05, "berg", dist="point2plane")],
    "L1-none": [rob("L1", 1.0)], "student-mad-apx": [rob("student", 1.5, "mad", approximation=1.5)],
}


def oracle_weights(ob, outliers, d2, ids, inp, p, map_c, iteration=1, scale=1.0):
    """(weights, limit, scale) of the oracle's OutlierFilters::compute, the robust scale handed back"""
    lib = ob.load()
    cfg = ob.make_config(outliers=outliers)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d2 = f(d2); ids = np.ascontiguousarray(ids, dtype=np.int32)
    n, k = d2.shape
    keep = [f(inp["read_normals"]), f(inp["normals"]), f(inp["map_scalar"]), f(p), f(map_c), f(inp["read_scalar"])]
    w = np.empty_like(d2); lim = C.c_float(-1); sc = C.c_float(scale)
    lib.orc_set_reading_scalar(keep[5].ctypes.data)
    err = lib.orc_outlier_weights_ex(C.byref(cfg), d2.ctypes.data, ids.ctypes.data, k, n, *[a.ctypes.data for a in keep[:5]], int(iteration),
                                     C.byref(sc), w.ctypes.data, C.byref(lim))
    lib.orc_set_reading_scalar(None)
    assert err == 0, err
    # an unfilled slot (d2 = +inf, MinDist alone lets it pass) never becomes a pair: the minimiser skips it, the reference weighs it 0
    return np.where(np.isfinite(d2), w, np.float32(0)), float(lim.value), float(sc.value)


def turned(inp):
    """the scene under a rotation about no axis of its own: the synthetic scene's planes are axis-aligned, its map normals have one
    component +-1 and two zeros, and every float32 product of the pair sums is then exact -- no yardstick for float32 rounding"""
    from norlab_icp_mapper_amd import synth
    R = synth.rotvec_to_R((0.7, -0.4, 0.9))
    out = dict(inp)
    for key in ("map", "reading"):
        c = inp[key].copy(); c[:, :3] = (inp[key][:, :3].astype(np.float64) @ R.T).astype(np.float32); out[key] = c
    for key in ("normals", "read_normals"):
        out[key] = np.ascontiguousarray((inp[key].astype(np.float64) @ R.T).astype(np.float32))
    return out


@pytest.fixture(scope="module", params=["as-built", "turned"])
def stage(oracle, request):
    """the small scene's first iteration, as built and turned: centred map and reading, matches at k = 1 and k = 3 within 0.6 m and unbounded"""
    inp = lwc.inputs(lwc.CASES[0])
    if request.param == "turned":
        inp = turned(inp)
    mean = inp["map"][:, :3].astype(np.float64).mean(0).astype(np.float32)
    map_c = inp["map"].copy(); map_c[:, :3] -= mean[None, :]
    p = inp["reading"].copy(); p[:, :3] -= mean[None, :]
    m = {(k, md): oracle.knn(map_c, p, k=k, max_dist=md, nthreads=16) for k in (1, 3) for md in (0.6, math.inf)}
    assert not np.isfinite(m[(3, 0.6)][1]).all()     # unfilled slots are part of the comparison
    return dict(inp=inp, map_c=map_c, p=p, matches=m)


def both_sides(oracle, stage, name, k):
    chain = CHAINS[name]
    ids, d2 = stage["matches"][(k, math.inf if "std" in name else 0.6)]
    ow, olim, oscale = oracle_weights(oracle, chain, d2, ids, stage["inp"], stage["p"], stage["map_c"])
    inp = stage["inp"]
    res = wr.chain_weights(chain, ids, d2, stage["p"], stage["map_c"], inp["normals"], inp["read_normals"], None, inp["map_scalar"], inp["read_scalar"])
    return chain, ids, d2, ow, olim, oscale, res


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", list(CHAINS))
def test_weights_match_the_oracle(oracle, stage, name, k):
    chain, ids, d2, ow, olim, oscale, res = both_sides(oracle, stage, name, k)
    w, und = res["w"], res["und"]
    assert und.sum() <= wr.max_undecidable(int((w != 0).sum())), (name, int(und.sum()))
    soft = any(o[0] == wr.ROBUST or (o[0] == wr.GENERIC and o[2] & SOFT) for o in chain)
    ow64 = ow.astype(np.float64)
    if not soft:
        assert np.array_equal(ow64[~und], w[~und]), (name, int((ow64 != w).sum()))
    else:
        assert np.array_equal((ow64 != 0)[~und], (w != 0)[~und]), name
        err = np.abs(ow64 - w)[~und]
        print(f"{name} k={k}: largest |oracle - reference| of a soft weight {err.max():.3e} (weights up to {w.max():.3e})")
        assert np.all(err <= SOFT_REL * np.maximum(w[~und], 1.0)), (name, float((err / np.maximum(w[~und], 1.0)).max()))
    assert 0 < (w != 0).sum() and ((w == 0).any() or name in ("gen-ref-soft", "cauchy-mad", "gm-none", "L1-none", "huber-berg", "huber-mad-plane", "cauchy-berg-plane"))
    quant = [f for f, o in enumerate(chain) if o[0] in (wr.MEDIAN, wr.TRIMMED, wr.VARTRIMMED)]
    if quant:   # the oracle hands back the limit of the chain's last quantile filter
        assert np.float32(res["limits"][quant[-1]]) == np.float32(olim), (name, res["limits"], olim)
    if res["scale"] is not None and (chain[0][2] >> 4) & 15:
        assert abs(res["scale"] - oscale) <= 4 * np.spacing(np.float32(res["scale"])), (name, res["scale"], oscale)


def sums_distance(oracle, stage, name, k):
    """largest |oracle - reference| / sum |w * term| over A's 21 and b's 6 entries, for the ORACLE's weights on both sides"""
    chain, ids, d2, ow, _, _, _ = both_sides(oracle, stage, name, k)
    inp = stage["inp"]
    err, _, A, b, _, st = oracle.minimize(2, stage["p"], stage["map_c"], inp["normals"], ids, d2, ow)
    assert err == 0
    terms = wr.pair_terms(2, stage["p"], stage["map_c"], inp["normals"], ids)
    sums, ab = wr.pair_sums(ow.astype(np.float64), terms)
    assert int(sums[28]) == st.pairs
    osum = np.array([A[a, c] for a in range(6) for c in range(a, 6)] + list(b))
    diff, scale = np.abs(osum - sums[:27]), ab[:27]
    assert np.all(diff[scale == 0] == 0)     # (axis-aligned normals: n_x n_y is exactly zero for every pair)
    return float((diff[scale > 0] / scale[scale > 0]).max())


def test_pair_sums_match_the_oracle_and_set_the_bar(oracle, stage):
    worst = {}
    for name in CHAINS:
        for k in (1, 3):
            worst[(name, k)] = sums_distance(oracle, stage, name, k)
    top = max(worst, key=worst.get)
    print(f"largest |oracle - reference| / sum |w term| = {worst[top]:.3e} at {top}; SUMS_REL = {wr.SUMS_REL:.3e}")
    # SUMS_REL is eight times the measured distance (weights_reference.py states both): the measurement must stand
    assert worst[top] <= wr.MEASURED_SUMS_REL, worst[top]
    assert abs(wr.SUMS_REL / (8 * wr.MEASURED_SUMS_REL) - 1) < 0.01


def test_point_to_point_sums_match_the_oracle(oracle, stage):
    """the oracle hands back H = sum w (q - mq)(p - mp)^T rounded to float32: the reference's sums give the same H"""
    for name in ("trimmed", "cauchy-mad"):
        chain, ids, d2, ow, _, _, _ = both_sides(oracle, stage, name, 3)
        inp = stage["inp"]
        err, _, A, _, _, _ = oracle.minimize(1, stage["p"], stage["map_c"], None, ids, d2, ow)
        assert err == 0
        s, ab = wr.pair_sums(ow.astype(np.float64), wr.pair_terms(1, stage["p"], stage["map_c"], None, ids))
        H = np.array([[s[7 + 3 * c + r] - s[4 + r] / s[0] * s[1 + c] for c in range(3)] for r in range(3)])
        Ho = np.array([[A.T.ravel()[3 * c + r] for c in range(3)] for r in range(3)])
        scale = np.array([[ab[7 + 3 * c + r] for c in range(3)] for r in range(3)])
        assert np.all(np.abs(H - Ho) <= U * np.abs(H) + wr.SUMS_REL * scale), (name, np.abs(H - Ho).max())


def test_the_bar_is_sharp(oracle, stage):
    """one pair of weight >= 0.5 dropped, or two weights that differ by >= 0.5 exchanged, among 6 000 pairs: some entry leaves
    10 x SUMS_REL of its scale -- for EVERY such pair / EVERY one of 2 000 random such exchanges"""
    chain, ids, d2, ow, _, _, res = both_sides(oracle, stage, "cauchy-mad", 1)
    w = res["w"]
    assert w.size == 6000
    terms = wr.pair_terms(2, stage["p"], stage["map_c"], stage["inp"]["normals"], ids)
    sums, ab = wr.pair_sums(w, terms)
    bar = 10 * wr.SUMS_REL * ab
    contrib = w[..., None] * terms                              # (n, 1, 32)
    heavy = np.nonzero(w[:, 0] >= 0.5)[0]
    assert heavy.size > 1000
    moved = np.abs(contrib[heavy, 0, :28])                      # dropping pair i moves entry e by |w_i term_ie| ([28] by 1)
    moved[:, 28 - 1] = np.abs(contrib[heavy, 0, 27])
    assert np.all((moved > bar[None, :28]).any(1)), "a dropped pair would pass"
    rng = np.random.default_rng(3)
    a = rng.integers(0, 6000, 200000); b = rng.integers(0, 6000, 200000)
    far = np.abs(w[a, 0] - w[b, 0]) >= 0.5
    a, b = a[far][:2000], b[far][:2000]
    assert a.size == 2000
    dw = (w[a, 0] - w[b, 0])[:, None]
    moved = np.abs(dw * (terms[b, 0, :] - terms[a, 0, :]))      # exchanging w_a and w_b moves entry e by (w_a - w_b)(term_b - term_a)
    assert np.all((moved > bar[None, :]).any(1)), "an exchange of two weights would pass"


@pytest.mark.parametrize("cid", lwc.IDS)
def test_undecidable_pairs_of_the_gpu_cases(oracle, cid):
    """the condition every case of tests/test_gpu_loop_weights.py must meet: at most max(2, 1e-5 pairs) undecidable pairs per iteration,
    evaluated on the oracle's matches of the same scene (three iterations; two of the 135 000-point readings)"""
    c = lwc.CASES[lwc.IDS.index(cid)]
    seen = 0
    for j, res, pairs in lwc.cpu_replay(oracle, c, iterations=2 if c["scene"] == "big" else 3):
        u = int(res["und"].sum())
        seen = max(seen, u)
        assert u <= wr.max_undecidable(pairs), (cid, j, u, pairs)
        assert pairs > 0 and np.isfinite(res["w"]).all()
    print(f"{cid}: at most {seen} undecidable pairs in an iteration")
    assert seen == wr.UNDECIDABLE_SEEN.get(cid, 0)


@pytest.mark.parametrize("cid", [c["id"] for c in lwc.CASES if c["scene"] == "small"])
def test_float32_weights_sum_within_the_bar(oracle, cid):
    """what the GPU test asks of the device, asked of the oracle first: the sums over ITS float32 weights (first iteration of every
    small-scene case) lie within SUMS_REL of the sums over the reference's weights, evaluated at the float32 scale the oracle held.  With
    the float64 scale in its place every welsch weight moves the same way and b leaves the bar (5.7e-08 at robust-welsch-std-k2+trimmed)."""
    c = lwc.CASES[lwc.IDS.index(cid)]
    inp = lwc.inputs(c)
    mean = inp["map"][:, :3].astype(np.float64).mean(0).astype(np.float32)
    map_c = inp["map"].copy(); map_c[:, :3] -= mean[None, :]
    p = inp["reading"].copy(); p[:, :3] -= mean[None, :]
    ids, d2 = oracle.knn(map_c, p, k=c["knn"], max_dist=c["max_dist"], nthreads=16)
    ow, _, osc = oracle_weights(oracle, c["outliers"], d2, ids, inp, p, map_c)
    s64 = lwc.scale_of(c, 1, {1: d2})
    if s64 is not None:
        assert abs(osc - s64) <= 4 * np.spacing(np.float32(s64))
    res, terms, rsums, rabs = lwc.reference_iteration(c, inp, map_c, p, ids, d2, None, 1, {1: d2}, scale_state=np.float32(osc) if s64 is not None else None)
    osums, _ = wr.pair_sums(ow.astype(np.float64), terms)
    tol = wr.SUMS_REL * rabs + wr.undecidable_slack(res, terms)
    tol[28] = res["und"].sum()
    assert np.all(np.abs(osums - rsums) <= tol), (cid, np.nonzero(~(np.abs(osums - rsums) <= tol))[0].tolist())
