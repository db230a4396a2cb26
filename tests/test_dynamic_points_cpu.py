"""The yardsticks of tests/test_gpu_dynamic_points.py, proven before the GPU is asked: on every case of tests/dynamic_points_cases.py that
carries the float64 flag the oracle's brute-force search agrees with the project's float64 restatement of the reference
(tests/golden/make_recalled.py::dynamic_points_update, imported by path) within the case's tolerance, on at least 0.8 of the map points;
the deliberately ambiguous cases (ties, bucket edges, boundaries) deliver what their builders promise; and three mutations of the search
-- a wrapped azimuth, a bucket's last record dropped, the larger index on a tie -- are each rejected by the bars the GPU test applies.  CPU only."""
import numpy as np
import pytest

import dynamic_points_cases as dc

F32 = np.float32
FLAGGED = [c for c in dc.IDS if c in dc.MEASURED]


@pytest.fixture(scope="module")
def oracle_result(oracle):
    cache = {}

    def run(cid):
        if cid not in cache:
            T, beams, mp, nrm, p0, prm, _ = dc.case(cid)
            cache[cid] = oracle.dynamic_points_update(T, beams, mp, nrm, p0, nthreads=8, **dc.kwargs(prm))
            cache[cid].setflags(write=False)
        return cache[cid]
    return run


def test_every_flagged_case_has_a_measured_tolerance():
    assert sorted(FLAGGED) == sorted(c for c in dc.IDS if dc.case(c)[6]["float64"])
    assert all(dc.tol(c) >= 2e-4 for c in FLAGGED) and dc.tol("generic-b0.01") == 2e-4


@pytest.mark.parametrize("cid", FLAGGED)
def test_oracle_meets_the_float64_bar(oracle_result, cid):
    ref = oracle_result(cid)
    err, at, share = dc.float64_error(cid, ref)
    print(f"{cid}: oracle vs float64 {err:.3e} at map index {at}, sure share {share:.3f}, tol {dc.tol(cid):.3e}")
    assert share >= dc.SURE_SHARE, (cid, share)
    assert err <= dc.tol(cid), (cid, dc.case(cid)[5], err, at)
    prob0 = dc.case(cid)[4]
    expected, sure = dc.float64_reference(cid)
    assert ((expected != prob0) & sure).sum() >= 1 and np.isfinite(ref).all() and (ref >= 0).all() and (ref <= 1).all()


# ---- what the builders promise ------------------------------------------------------------------------------------------------------
def test_the_two_small_half_angles_straddle_the_side_scan_limit():
    """0.001 takes the three-kernel scan, 0.0011 the two-kernel one -- by the issue's formula and by the grid as the device lays it out"""
    for count in (dc.ncells_formula, lambda b: dc.grid(b)[1] * dc.grid(b)[2]):
        assert count(0.001) > dc.SIDE_SCAN_MAX_CELLS > count(0.0011), (count(0.001), count(0.0011))
        assert count(0.001) <= dc.MAX_CELLS < count(1e-4)
    assert dc.grid(0.5)[1:] == (8, 14) and dc.grid(2.0)[1:] == (3, 5)          # smaller than the 5 x 5 block
    assert dc.grid(0.001)[1] * dc.grid(0.001)[2] < 20_000_000                   # (the 160 MB table pair the GPU test allows itself)


def test_ties_are_bit_equal_and_decided_by_the_index(oracle_result):
    T, beams, mp, nrm, p0, prm, flags = dc.case("ties")
    e, a = dc.angles32(beams[:, :3])
    trio = flags["trio"]
    for j in (1, 2):
        assert np.array_equal(e[trio[:, 0]].view(np.uint32), e[trio[:, j]].view(np.uint32)) and np.array_equal(a[trio[:, 0]].view(np.uint32), a[trio[:, j]].view(np.uint32))
    r = np.linalg.norm(beams[:, :3].astype(np.float64), axis=1)
    assert np.allclose(r[trio[:, 1]], 2 * r[trio[:, 0]]) and np.allclose(r[trio[:, 2]], 0.5 * r[trio[:, 0]])
    best, _ = search("ties")
    hit = best >= 0
    assert hit.sum() >= 1500
    assert np.array_equal(best[hit], trio.min(axis=1)[np.arange(mp.shape[0])[hit] % trio.shape[0]])   # query j belongs to direction j mod K
    assert len({int(np.argmin(t)) for t in trio}) == 3                                                  # each of p, 2 p, p / 2 wins somewhere


def test_bucket_edge_angles_sit_on_the_edges():
    for b in (0.01, 0.0137):
        T, beams, mp, nrm, p0, prm, flags = dc.case(f"bucket_edges-b{b}")
        cell, ne, na = dc.grid(b)
        qe, qa = dc.angles32(mp[:, :3])
        be, ba = dc.angles32(beams[:, :3])
        # per angle: the queries of the first 70 pairs and the beams of the last 70 are within a few ulps of a bucket edge
        for qang, bang, idx, c in ((qe, be, flags["on_e"], dc.HALF_PI32), (qa, ba, flags["on_a"], dc.PI32)):
            for ang, sel in ((qang, idx[:70]), (bang, idx[70:])):
                v = ang[sel].astype(np.float64) + float(c)
                off = np.abs(v - np.rint(v / float(cell)) * float(cell)) / np.spacing(np.abs(ang[sel])).astype(np.float64)
                assert len(sel) == 70 and off.max() <= 5.0, (b, off.max())   # (2 ulps asked for, the float32 edge against the float64 one, an elevation asin cannot reach)
        # the partners: found and not found, at 2 b give or take a few ulps of the angles
        best, bd = search(f"bucket_edges-b{b}")
        hit = best >= 0
        assert 0.15 < hit.mean() < 0.85
        assert (np.abs(np.sqrt(bd[hit].astype(np.float64)) - float(F32(2) * F32(b))) < 6e-7).sum() >= 60
        # ... and the float32 bucket assignment puts such pairs two AND three buckets apart: the block of the search must still hold them
        ce, ca = dc.cells32(b, qe, qa)
        bce, bca = dc.cells32(b, be, ba)
        apart = np.maximum(np.abs(ce - bce), np.abs(ca - bca))[hit]
        assert apart.max() <= dc.RINGS, (b, apart.max())


def test_boundaries_hold_the_exact_values(oracle_result):
    for cid, rng_max in (("boundaries-r5", 5.0), ("boundaries-inf", np.inf)):
        T, beams, mp, nrm, p0, prm, flags = dc.case(cid)
        ref = oracle_result(cid)
        x, y, z = mp[:, 0], mp[:, 1], mp[:, 2]
        norm = np.sqrt((x * x + y * y) + z * z)
        at, inside, outside = int(flags["at_range"][0]), int(flags["inside"][0]), int(flags["outside"][0])
        assert norm[at] == F32(5.0) and norm[inside] < F32(5.0) < norm[outside] and prm["sensor_max_range"] == rng_max
        touched = ref.view(np.uint32) != p0.view(np.uint32)
        assert touched[inside] and touched[at] == (rng_max > 5.0) and touched[outside] == (rng_max > 5.0)
        thr = F32(prm["threshold_dynamic"])
        assert (p0 == thr).sum() >= 30 and (p0 == 0).sum() >= 30 and (p0 == 1).sum() >= 30
        latched = flags["latched"]
        eps = F32(0.0001)
        assert (ref[latched][touched[latched]] == (1 - eps) / ((1 - eps) + eps)).all() and touched[latched].sum() >= 40   # lastDyn == threshold: latched
        below = np.flatnonzero(p0 == np.nextafter(thr, F32(0)))
        assert (ref[below][touched[below]] < 0.999).all() and touched[below].sum() >= 10
        assert not nrm[flags["zero_normal"]].any() and touched[flags["zero_normal"]].sum() >= 10


# ---- the search in numpy, float32 operation by operation, and the three ways it is broken on purpose -----------------------------------
def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def to_sensor_frame(T, p):
    cols = []
    for r in range(3):
        cols.append(fma32(T[r, 3], p[:, 3], fma32(T[r, 2], p[:, 2], fma32(T[r, 1], p[:, 1], T[r, 0] * p[:, 0]))))
    return np.stack(cols, axis=1)


def search(cid, mutation=None):
    """(best beam or -1, squared angular distance) per map point: the oracle's brute force, or one of its mutations"""
    T, beams, mp, nrm, p0, prm, _ = dc.case(cid)
    b = prm["beam_half_angle"]
    bs, ms = to_sensor_frame(T, beams), to_sensor_frame(T, mp)
    be, ba = dc.angles32(bs)
    qe, qa = dc.angles32(ms)
    reach = F32(2) * F32(b)
    r2 = reach * reach
    d0 = qe[:, None] - be[None, :]
    d1 = qa[:, None] - ba[None, :]
    if mutation == "wrap_azimuth":                       # a search that takes the azimuth as periodic: the reference's kd-tree does not
        d1 = np.where(d1 > dc.PI32, d1 - dc.TWO_PI32, np.where(d1 < -dc.PI32, d1 + dc.TWO_PI32, d1)).astype(F32)
    d = d0 * d0 + d1 * d1
    ok = d <= r2
    if mutation == "drop_last_record":                   # every bucket loses the record with its largest beam index
        ce, ca = dc.cells32(b, be, ba)
        key = ce * dc.grid(b)[2] + ca
        last = {}
        for i, k in enumerate(key.tolist()):
            last[k] = i
        ok[:, sorted(last.values())] = False
    d = np.where(ok, d, F32(np.inf))
    bd = d.min(axis=1)
    if mutation == "larger_index_on_tie":
        best = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
    else:
        best = np.argmin(d, axis=1)                      # the first minimum: the smallest beam index
    x, y, z = ms[:, 0], ms[:, 1], ms[:, 2]
    in_range = np.sqrt((x * x + y * y) + z * z) < F32(prm["sensor_max_range"])
    best = np.where(np.isfinite(bd) & in_range, best, -1)
    return best, bd


def update(cid, best, bd):
    """the probabilities after the update with the given matches: orc_dynamic_points_update's arithmetic in numpy"""
    T, beams, mp, nrm, p0, prm, _ = dc.case(cid)
    thr, alpha, beta, bha, eps_a, eps_d = (F32(prm[k]) for k in dc.KEYS[:6])
    eps = F32(0.0001)
    eps64, one_m = np.float64(eps), 1.0 - np.float64(eps)
    bs, ms = to_sensor_frame(T, beams), to_sensor_frame(T, mp)
    hit = best >= 0
    ip = bs[np.maximum(best, 0)]
    inputNorm = np.sqrt((ip[:, 0] * ip[:, 0] + ip[:, 1] * ip[:, 1]) + ip[:, 2] * ip[:, 2])
    mapNorm = np.sqrt((ms[:, 0] * ms[:, 0] + ms[:, 1] * ms[:, 1]) + ms[:, 2] * ms[:, 2])
    dv = ip - ms
    delta = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    d_max = eps_a * inputNorm
    nr = np.stack([fma32(T[r, 2], nrm[:, 2], fma32(T[r, 1], nrm[:, 1], T[r, 0] * nrm[:, 0])) for r in range(3)], axis=1)
    with np.errstate(all="ignore"):
        ndot = ((nr[:, 0] * ms[:, 0] + nr[:, 1] * ms[:, 1]) + nr[:, 2] * ms[:, 2]) / mapNorm
        w_v = (eps64 + one_m * np.abs(ndot.astype(np.float64))).astype(F32)
        w_d1 = (eps64 + one_m * (1.0 - (np.sqrt(np.where(hit, bd, F32(0))) / (F32(2) * bha)).astype(np.float64))).astype(F32)
        offset = delta - eps_d
        w_d2 = np.where((delta < eps_d) | (mapNorm > inputNorm), eps, np.where(offset < d_max, eps + (F32(1) - eps) * offset / d_max, F32(1))).astype(F32)
        w_p2 = np.where(delta < eps_d, F32(1), np.where(offset < d_max, (eps64 + one_m * (1.0 - (offset / d_max).astype(np.float64))).astype(F32), eps)).astype(F32)
        c2 = w_v * w_d1
        c1 = F32(1) - c2
        pd = c1 * p0 + c2 * w_d2 * ((F32(1) - alpha) * (F32(1) - p0) + beta * p0)
        ps = c1 * (F32(1) - p0) + c2 * w_p2 * (alpha * (F32(1) - p0) + (F32(1) - beta) * p0)
        latched = ~(p0 < thr)
        pd = np.where(latched, F32(1) - eps, pd).astype(F32)
        ps = np.where(latched, eps, ps).astype(F32)
        new = (pd / (pd + ps)).astype(F32)
    return np.where(hit & ((inputNorm + eps_d + d_max) >= mapNorm), new, p0).astype(F32)


@pytest.mark.parametrize("cid", ["seam", "dense-r1", "generic-b0.5", "ties", "boundaries-r5", "bucket_edges-b0.01", "poles"])
def test_numpy_search_is_the_oracle(oracle_result, cid):
    """without a mutation the numpy search and update ARE the oracle, bit for bit: what a mutant differs by is its mutation"""
    got = update(cid, *search(cid))
    ref = oracle_result(cid)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (cid, dc.first_diff(got, ref))


# mutation -> (case whose constructed queries must differ bitwise, the group of those queries, flagged cases of which one must miss the float64 bar)
MUTATIONS = {
    "wrap_azimuth": ("seam", "across", ("seam",)),
    "drop_last_record": ("dense-r1", "at_last", ("dense-r1", "generic-b0.5")),
    # a float32 tie is a float64 near-tie, and those the float64 reference marks ambiguous by construction: bitwise only
    "larger_index_on_tie": ("ties", "decided", ()),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_rejects_each_mutation(oracle_result, mutation):
    cid, group, flagged = MUTATIONS[mutation]
    ref = oracle_result(cid)
    got = update(cid, *search(cid, mutation))
    queries = dc.case(cid)[6][group]
    differs = got.view(np.uint32)[queries] != ref.view(np.uint32)[queries]
    assert len(queries) >= 8 and differs.all(), (mutation, cid, int(differs.sum()), len(queries))
    if mutation == "larger_index_on_tie":   # ... and the mutant is wrong about nothing else: same distances, another beam of the trio
        assert np.array_equal(search(cid, mutation)[1], search(cid)[1])
    missed = []
    for fc in flagged:
        mutant = update(fc, *search(fc, mutation))
        err, at, _ = dc.float64_error(fc, mutant)
        print(f"{mutation} on {fc}: {err:.3e} at map index {at} against tol {dc.tol(fc):.3e}")
        if err > dc.tol(fc):
            missed.append(fc)
    assert len(missed) == len(flagged), (mutation, missed)
