"""The self k-NN grid (csrc/selfgrid.hip) against exact search, at its edges and after appends.

selfgrid.hip claims "the same k points in the same order whatever the grid".  Here that claim meets the clouds of tests/self_knn_cases.py
(each built for a branch: see that file) at every k where a kernel changes path, through two test seams:
  ICPSequence.debugSelfKnn        the search behind surfaceNormals, ids and d2 as the kernels left them, and the grid it built
  ICPSequence.debugResidentKthD2  the k-th distances the resident map remembers between appends -- what the subset search selects from
The reference is the oracle's exact search (bit for bit) and the float64 check of tests/match_reference.py (its bands unchanged); every query
is compared, nothing is sampled or excluded.  tests/test_self_knn_cases_cpu.py keeps the references and the clouds honest without a GPU."""
import numpy as np
import pytest

import match_reference as mr
import self_knn_cases as sc

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
REL32 = 2.0 ** -23       # a double result rounded once to float32 (2^-24) + the last bit of a float32 reference value (2^-24)
RANK_BAND = 1e-6         # around the rank threshold 3 eps32 lambda_2: the room between a double Jacobi and eigvalsh, far above either's error


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def shared(amd):
    """one handle for the exactness cases: whatever the previous cloud left in the grid's arrays and its tuner must not matter"""
    return amd.ICPSequence(minimizer=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_knn(got, ref, what):
    ids, d2 = got
    rids, rd2 = ref
    bad = np.nonzero((bits(d2) != bits(rd2)).any(1))[0]
    assert bad.size == 0, f"{what}: d2 differs from the reference at {bad.size} queries, first {int(bad[0])}: {d2[bad[0]].tolist()} vs {rd2[bad[0]].tolist()}"
    bad = np.nonzero((ids != rids).any(1))[0]
    assert bad.size == 0, f"{what}: ids differ from the reference at {bad.size} queries, first {int(bad[0])}: {ids[bad[0]].tolist()} vs {rids[bad[0]].tolist()}"


# ---- a. exactness on the edge cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", sc.CASES)
def test_exact_on_edge_case(shared, oracle, name, k):
    c = sc.make(name)
    ids, d2, info = shared.debugSelfKnn(c, k, with_info=True)
    assert_same_knn((ids, d2), sc.reference(name, k), f"{name} k={k}")
    mr.check_matches(c, c, ids, d2, k, np.inf, use_oracle=False, where=f"{name} k={k}")
    assert info["tsize"] <= 2 ** 24, info


@pytest.mark.parametrize("k", sc.KS)
def test_exact_on_tiny_clouds(shared, oracle, k):
    for m in sc.tiny_sizes(k):
        c = sc.tiny(m)
        ids, d2 = shared.debugSelfKnn(c, k)
        assert_same_knn((ids, d2), sc.reference_of(c, k), f"tiny m={m} k={k}")
        mr.check_matches(c, c, ids, d2, k, np.inf, use_oracle=False, where=f"tiny m={m} k={k}")
        assert ((ids >= 0).sum(1) == min(k, m)).all() and np.isinf(d2[ids < 0]).all()


# ---- b. the case reached its branch: only what the geometry forces, no tuned number ---------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
def test_case_reaches_its_branch(amd, oracle, name):
    icp = amd.ICPSequence(minimizer=1)
    c = sc.make(name)
    ids, d2, info = icp.debugSelfKnn(c, 10, with_info=True)
    assert_same_knn((ids, d2), sc.reference(name, 10), name)
    na = info["na"]
    assert info["tsize"] <= 2 ** 24 and info["trials"] >= 1 and info["cell"] > 0 and min(na) >= 1, info
    if name == "identical": assert na == (1, 1, 1), info
    if name == "line": assert na[1] == 1 and na[2] == 1 and na[0] > 1, info
    if name == "plane_z0": assert na[2] == 1 and na[0] > 1 and na[1] > 1, info
    if name in ("heavy", "clump_far"): assert info["queued"] > 0, info


def test_points_on_the_margin_of_the_cell_kernel(amd, oracle):
    """the rounding slack of sg_margin2: queries whose k-th candidate inside the 3 x 3 x 3 block is exactly as far as the margin WITHOUT slack
    allows, while a nearer point sits just outside the block (tests/self_knn_cases.py: margin_gadgets).  The gadgets are laid out for the
    grid they will meet: a warm-up cloud of the same size is searched until the tuner keeps its edge, and the next build takes that edge."""
    k = 2
    icp = amd.ICPSequence(minimizer=1)
    warm = sc.margin_warmup()
    cells = []
    while len(cells) < 24 and (len(cells) < 2 or cells[-1] != cells[-2]):     # (a line's occupancy grows with the edge, not its square: ~10 steps)
        ids, d2, info = icp.debugSelfKnn(warm, k, with_info=True)
        cells.append(info["cell"])
    assert cells[-1] == cells[-2], f"the tuner did not settle on the warm-up cloud: {cells}"
    assert_same_knn((ids, d2), sc.reference_of(warm, k), "margin warm-up")
    c, fired, edge = sc.margin_gadgets(cells[-1])
    assert fired >= 20, fired
    ids, d2, info = icp.debugSelfKnn(c, k, with_info=True)
    assert info["trials"] == 1 and info["cell"] == edge, (info, edge, cells)     # the grid the gadgets were laid out for, or they test nothing
    assert info["na"][1] == 1 and info["na"][2] == 1
    assert_same_knn((ids, d2), sc.reference_of(c, k), "margin gadgets")
    mr.check_matches(c, c, ids, d2, k, np.inf, use_oracle=False, where="margin gadgets")


# ---- c. grid independence -------------------------------------------------------------------------------------------------------------------------
def test_answer_does_not_depend_on_the_grid_history(amd, oracle):
    """One handle sees heavy -> heavy scaled by 0.01 -> offset -> heavy: the second build is of the size of the one before and starts from
    ITS cell edge (like_before: a hundred times too wide here), the third and the fourth are not and tune again on the arrays the others
    left.  A fresh handle tunes each cloud from scratch.  Same bits either way -- and the grids did differ, or the comparison would prove
    nothing."""
    k = 10
    heavy, offset = sc.make("heavy"), sc.make("offset")
    small = sc.scaled(heavy, 0.01)
    seq = [("heavy", heavy), ("heavy x 0.01", small), ("offset", offset), ("heavy again", heavy)]
    refs = [sc.reference("heavy", k), sc.reference_of(small, k), sc.reference("offset", k), sc.reference("heavy", k)]
    one = amd.ICPSequence(minimizer=1)
    cells_seq, cells_fresh = [], []
    for (what, c), ref in zip(seq, refs):
        a = one.debugSelfKnn(c, k, with_info=True)
        b = amd.ICPSequence(minimizer=1).debugSelfKnn(c, k, with_info=True)
        assert_same_knn(a[:2], ref, f"{what}, handle with a history")
        assert_same_knn(b[:2], ref, f"{what}, fresh handle")
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
        cells_seq.append(a[2]); cells_fresh.append(b[2])
    assert cells_seq[1]["trials"] == 1, cells_seq            # like_before: the previous edge, one build
    assert any(s["cell"] != f["cell"] for s, f in zip(cells_seq, cells_fresh)), (cells_seq, cells_fresh)


# ---- d. the normals kernel at its register-variant boundaries ---------------------------------------------------------------------------------------
def neighbourhood_moments(pts, ids):
    """float64, straight from include/icpmi.h: the centroid of each neighbour set (unfilled slots left out), its scatter matrix, the
    largest distance of a neighbour from the centroid, the distance of the point (its own first neighbour) from the centroid"""
    P = pts[:, :3].astype(np.float64)
    valid = ids >= 0
    nb = P[np.maximum(ids, 0)]
    cnt = valid.sum(1)
    mean = (nb * valid[:, :, None]).sum(1) / np.maximum(cnt, 1)[:, None]
    d = (nb - mean[:, None, :]) * valid[:, :, None]
    C = np.einsum("nki,nkj->nij", d, d)
    r = np.sqrt((d ** 2).sum(-1).max(1))
    md = np.linalg.norm(nb[:, 0] - mean, axis=1)
    # what one rounding of the float64 centroid moves a distance from it by: the reference's own last bit (the kernel's centroid, sum x (1 / k),
    # and this one, sum / k, are both correctly formed doubles and differ by it)
    # (k - 1 additions and one scaling, each rounded at 2^-53 of a partial sum of at most k |x|, over the k it is divided by)
    floor = 2.0 ** -52 * ids.shape[1] * np.abs(nb).max(axis=(1, 2))
    return cnt, C, r, md, floor


def check_normals(oracle, pts, ids, normals, what, planar=False):
    """every normal against the float64 spectrum of its reference neighbour set; returns the share of points skipped inside the rank band"""
    cnt, C, r, md, floor = neighbourhood_moments(pts, ids)
    n = pts.shape[0]
    fallback = (normals == np.array([1.0, 0.0, 0.0], dtype=np.float32)).all(1)
    if planar:   # the smaller eigenvector of the x-y pair, needed rank 1: any extent at all
        lam = np.linalg.eigvalsh(C[:, :2, :2])
        some = lam[:, 1] > 0
        assert fallback[~some].all(), what
        assert (normals[:, 2] == 0).all(), what
        nn = normals[:, :2].astype(np.float64)
        np.testing.assert_allclose(np.linalg.norm(nn, axis=1), 1.0, atol=2e-6, err_msg=what)
        ray = np.einsum("ni,nij,nj->n", nn, C[:, :2, :2], nn)
        excess = (ray - lam[:, 0]) / np.maximum(lam[:, 1], 1e-300)
        assert (excess[some] <= 2e-5).all(), (what, float(excess[some].max()))
        return 0.0
    lam = np.linalg.eigvalsh(C)
    thr = 3.0 * EPS32 * lam[:, 2]
    below = lam[:, 1] < thr * (1.0 - RANK_BAND)
    above = lam[:, 1] > thr * (1.0 + RANK_BAND)
    below |= lam[:, 2] == 0                                  # no extent at all: rank 0
    above &= ~below
    bad = np.nonzero(below & ~fallback)[0]
    assert bad.size == 0, f"{what}: {bad.size} rank-deficient neighbourhoods without the fallback normal (1, 0, 0), first {int(bad[0])}: {normals[bad[0]].tolist()}"
    sel = np.nonzero(above)[0]
    if sel.size:
        full = (ids[sel] >= 0).all(1)                        # (the oracle's checker takes whole rows; rows with unfilled slots: below)
        if full.any():
            rank2 = oracle.check_normals_are_smallest_eigenvectors(pts, ids[sel[full]], normals[sel[full]], what)
            assert rank2.all(), what
        part = sel[~full]
        if part.size:
            nn = normals[part].astype(np.float64)
            np.testing.assert_allclose(np.linalg.norm(nn, axis=1), 1.0, atol=2e-6, err_msg=what)
            excess = (np.einsum("ni,nij,nj->n", nn, C[part], nn) - lam[part, 0]) / lam[part, 2]
            assert (excess <= 2e-5).all(), (what, float(excess.max()))
    return float((~below & ~above).sum()) / n


def check_densities_and_mean_dist(pts, ids, dens, md, what):
    cnt, C, r, ref_md, floor = neighbourhood_moments(pts, ids)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref_dens = cnt / ((4.0 / 3.0) * np.pi * r ** 3)
        # density ~ r^-3: the centroid's last bit moves it by 3 floor / r (nothing where r is millimetres; everything where r = 0: inf == inf)
        rel = REL32 + 3.0 * floor / r
    zero = r == 0
    assert np.isinf(dens[zero]).all() and (dens[zero] > 0).all(), f"{what}: a neighbourhood of coincident points must have density +inf"
    err = np.abs(dens[~zero].astype(np.float64) - ref_dens[~zero])
    ok = (err <= rel[~zero] * ref_dens[~zero]) | (np.isinf(dens[~zero]) & (ref_dens[~zero] * (1 - rel[~zero]) > np.finfo(np.float32).max))
    assert ok.all(), f"{what}: {int((~ok).sum())} densities off, worst relative {float((err / ref_dens[~zero]).max()):.3e}"
    err = np.abs(md.astype(np.float64) - ref_md)
    ok = err <= REL32 * ref_md + floor
    assert ok.all(), f"{what}: {int((~ok).sum())} mean distances off, worst {float(err.max()):.3e}"


@pytest.mark.parametrize("k", [2, 3, 10, 11, 16, 17, 32])
@pytest.mark.parametrize("name", ["heavy", "piles", "plane_z0"])
def test_normals_at_the_register_variant_boundaries(amd, oracle, name, k):
    c = sc.make(name)
    rids, _ = sc.reference(name, k)
    icp = amd.ICPSequence(minimizer=1)
    nrm, dens, ids, md = icp.surfaceNormals(c, knn=k, with_densities=True, with_matched_ids=True, with_mean_dist=True)
    bad = np.nonzero((ids != rids).any(1))[0]
    assert bad.size == 0, f"{name} k={k}: matched ids differ from the reference at {bad.size} points, first {int(bad[0])}"
    skipped = check_normals(oracle, c, rids, nrm, f"{name} k={k}")
    assert skipped < 1e-3, skipped
    check_densities_and_mean_dist(c, rids, dens, md, f"{name} k={k}")
    if name == "heavy" and k in (11, 17):
        _, ev, _ = icp.surfaceNormalsEigen(c, knn=k)
        _, C, _, _, _ = neighbourhood_moments(c, rids)
        lam = np.linalg.eigvalsh(C)
        assert (lam[:, 1] > 3 * EPS32 * lam[:, 2] * (1 + RANK_BAND)).all()      # (no rank-deficient neighbourhood here: no zeroed rows)
        err = np.abs(ev.astype(np.float64) - lam)
        assert (err <= REL32 * lam[:, 2:3]).all(), float((err / lam[:, 2:3]).max())


# ---- e. the incremental path against an independent reference ----------------------------------------------------------------------------------------
def check_resident_map(amd, oracle, icp, k, counters, what, planar=False, fresh_pass=False):
    """after an update: the remembered k-th distances and every normal against the oracle's self k-NN of the downloaded map, and the path taken"""
    pts, nrm = icp.getMap(with_normals=True)
    m = pts.shape[0]
    rids, rd2 = sc.reference_of(pts, k)
    dk, knn = icp.debugResidentKthD2()
    assert knn == k and dk.shape == (m,)
    want = rd2[:, k - 1]
    assert np.isinf(want[rids[:, k - 1] < 0]).all()
    bad = np.nonzero(bits(dk) != bits(want))[0]
    assert bad.size == 0, f"{what}: the remembered k-th d2 differs from the reference at {bad.size} of {m} points, first {int(bad[0])}: {dk[bad[0]]} vs {want[bad[0]]}"
    skipped = check_normals(oracle, pts, rids, nrm, what, planar=planar)
    assert skipped < 1e-3 or m < 1000, (what, skipped)
    c = icp.debugCounters()
    assert (int(c[20]), int(c[21])) == counters, (what, int(c[20]), int(c[21]), counters)
    if fresh_pass:
        ref = amd.ICPSequence(minimizer=1, **({"is_2d": 1} if planar else {})).surfaceNormals(pts, knn=k)
        assert np.array_equal(nrm, ref), f"{what}: {int((nrm != ref).any(axis=1).sum())} normals differ from a pass over the whole map"
    return pts


def resident(amd, first, **kw):
    icp = amd.ICPSequence(minimizer=1, max_dist=2.0, max_iterations=5, **kw)
    assert icp.setMap(first)
    return icp


def lattice(nx, ny, nz, origin=(0.0, 0.0, 0.0), h=0.25):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return sc.cloud(g * h + np.array(origin))


@pytest.mark.parametrize("k", [3, 10, 17])
def test_append_tie_on_the_kth_sphere(amd, oracle, k):
    """a lattice grows by lattice layers: for the old points of the face an appended point lies EXACTLY on the k-th sphere (d2 0.0625, 0.125,
    0.1875 for k = 3, 10, 17 -- every coordinate a multiple of 0.25) and the tie goes to the old point, the smaller index"""
    rng = np.random.default_rng(3)
    first = lattice(10, 10, 10)
    icp = resident(amd, first[rng.permutation(first.shape[0])])
    layers = [lattice(2, 10, 10, origin=(-0.5, 0, 0)), lattice(1, 10, 10, origin=(2.5, 0, 0)), lattice(13, 1, 10, origin=(-0.5, -0.25, 0))]
    for step, layer in enumerate(layers):
        app, m = icp.mapUpdatePointDistance(layer[rng.permutation(layer.shape[0])], 0.1, normals_knn=k)
        assert app == layer.shape[0]
        pts = check_resident_map(amd, oracle, icp, k, (step, 1), f"tie k={k} step {step}", fresh_pass=True)
        if step == 1:   # the tie is there: old face points whose k-th distance an appended point equals
            old = pts[:m - app]; new = pts[m - app:]
            face = old[old[:, 0] == np.float32(2.25)]
            _, rd2 = sc.reference_of(old, k)
            kth = rd2[old[:, 0] == np.float32(2.25), k - 1]
            d = ((face[:, None, :3].astype(np.float64) - new[None, :, :3]) ** 2).sum(-1)
            assert (d == kth[:, None].astype(np.float64)).any(1).sum() > 50


def test_append_duplicates_of_resident_points(amd, oracle):
    k = 10
    rng = np.random.default_rng(5)
    base = sc.make("heavy")[:6000]
    icp = resident(amd, base)
    icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 500, 2.0)), 0.0, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (0, 1), "duplicates: first pass")
    for step in range(2):
        pts = icp.getMap()
        dup = pts[rng.choice(pts.shape[0], 400, replace=False)]
        app, m = icp.mapUpdatePointDistance(np.concatenate([dup, dup[:50]]), 0.0, normals_knn=k)      # (some of them twice in one scan)
        assert app == 450
        check_resident_map(amd, oracle, icp, k, (step + 1, 1), f"duplicates step {step}", fresh_pass=True)


@pytest.mark.parametrize("k", [3, 10])
def test_append_outside_the_box_on_the_negative_sides(amd, oracle, k):
    """the grid's origin moves with every append and the sorted copy the next build starts from was ordered for the old origin"""
    rng = np.random.default_rng(6)
    icp = resident(amd, sc.cloud(rng.uniform(0.0, 10.0, (6000, 3))))
    icp.mapUpdatePointDistance(sc.cloud(rng.uniform(0.0, 10.0, (500, 3))), 0.05, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (0, 1), "box growth: first pass")
    for step, axis in enumerate([0, 1, 2]):
        lo = np.zeros(3); hi = np.full(3, 10.0)
        lo[axis] = -4.0 - step; hi[axis] = 0.5
        app, m = icp.mapUpdatePointDistance(sc.cloud(rng.uniform(lo, hi, (1500, 3))), 0.05, normals_knn=k)
        assert app > 1000
        check_resident_map(amd, oracle, icp, k, (step + 1, 1), f"box growth k={k} axis {axis}", fresh_pass=(k == 10))


def test_append_a_far_point_then_into_the_core(amd, oracle):
    k = 17
    rng = np.random.default_rng(8)
    icp = resident(amd, sc.make("heavy"))
    icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 300, 2.0)), 0.02, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (0, 1), "far point: first pass")
    far = sc.cloud(np.array([[300.0, 40.0, 5.0]]))
    app, m = icp.mapUpdatePointDistance(far, 0.02, normals_knn=k)
    assert app == 1
    check_resident_map(amd, oracle, icp, k, (1, 1), "far point appended")
    app, m = icp.mapUpdatePointDistance(sc.cloud(rng.normal(0.0, 0.5, (2000, 3)) * np.array([1.0, 1.0, 0.15])), 0.02, normals_knn=k)
    assert app > 200
    check_resident_map(amd, oracle, icp, k, (2, 1), "far point: into the core", fresh_pass=True)


def test_append_that_doubles_the_map(amd, oracle):
    """m grows by more than 1.4 x: the build does not take the previous edge but tunes again, its trials reading the sorted copy + the tail"""
    k = 10
    rng = np.random.default_rng(10)
    icp = resident(amd, sc.cloud(sc.heavy_xyz(rng, 4000, 2.0)))
    icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 300, 2.0)), 0.01, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (0, 1), "growth: first pass")
    app, m = icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 7000, 1.0)), 0.01, normals_knn=k)
    assert m > 2 * (m - app)
    check_resident_map(amd, oracle, icp, k, (1, 1), "growth: doubled", fresh_pass=True)
    app, m = icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 500, 4.0)), 0.01, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (2, 1), "growth: the append after")


@pytest.mark.parametrize("k", [3, 10, 17])
def test_append_small_sizes(amd, oracle, k):
    """a map that grows from 2 points through k - 1, k and k + 1 (rows with unfilled slots, k-th distances +inf), then one point at a time"""
    rng = np.random.default_rng(20 + k)
    pts = sc.cloud(rng.uniform(-1.0, 1.0, (k + 4, 3)))
    icp = resident(amd, pts[:2])
    have, step = 2, 0
    for target in sorted({t for t in (k - 1, k, k + 1, k + 2, k + 3) if t > 2}):
        app, m = icp.mapUpdatePointDistance(pts[have:target], 0.0, normals_knn=k)
        assert app == target - have and m == target
        have = target
        check_resident_map(amd, oracle, icp, k, (step, 1), f"small k={k} m={m}", fresh_pass=True)
        step += 1
    # and one point into a map of thousands
    icp = resident(amd, sc.make("plane_z0"))
    icp.mapUpdatePointDistance(sc.cloud(np.array([[3.0, 3.0, 0.5]])), 0.0, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (0, 1), f"one point k={k}: first pass")
    app, m = icp.mapUpdatePointDistance(sc.cloud(np.array([[7.0, 7.0, 0.0]])), 0.0, normals_knn=k)
    assert app == 1
    check_resident_map(amd, oracle, icp, k, (1, 1), f"one point k={k}", fresh_pass=True)


def test_append_far_from_the_origin(amd, oracle):
    k = 10
    c = sc.make("offset")
    icp = resident(amd, c[:5000])
    for step, part in enumerate([c[5000:5200], c[5200:6500], c[6500:]]):
        app, m = icp.mapUpdatePointDistance(part, 0.05, normals_knn=k)
        assert app > 0
        check_resident_map(amd, oracle, icp, k, (step, 1), f"offset step {step}", fresh_pass=(step == 2))


def test_foreign_search_between_two_appends(amd, oracle):
    """surfaceNormals of ANOTHER cloud on the same handle between two appends takes the grid's sorted copy away, not the remembered k-th distances:
    the next append still runs the subset search, built from the caller's order"""
    k = 10
    rng = np.random.default_rng(12)
    icp = resident(amd, sc.cloud(sc.heavy_xyz(rng, 6000, 2.0)))
    icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 400, 2.0)), 0.01, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (0, 1), "foreign: first pass")
    icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 400, 1.0)), 0.01, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (1, 1), "foreign: before")
    other = sc.make("two_clusters")
    ids, _ = icp.debugSelfKnn(other, k)
    assert np.array_equal(ids, sc.reference("two_clusters", k)[0])
    icp.surfaceNormals(sc.make("lattice"), knn=k)
    icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 400, 3.0)), 0.01, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (2, 1), "foreign: after", fresh_pass=True)
    icp.mapUpdatePointDistance(sc.cloud(sc.heavy_xyz(rng, 400, 0.5)), 0.01, normals_knn=k)
    check_resident_map(amd, oracle, icp, k, (3, 1), "foreign: the append after")


def test_append_on_the_planar_handle(amd, oracle):
    k = 10
    rng = np.random.default_rng(14)
    def ring(n, r, jitter):
        a = rng.uniform(0, 2 * np.pi, n)
        return sc.cloud(np.c_[np.c_[r * np.cos(a), r * np.sin(a)] + rng.normal(0, jitter, (n, 2)), np.zeros(n)])
    icp = resident(amd, ring(8000, 10.0, 0.02), is_2d=1)
    for step, r in enumerate((10.5, 6.0)):
        app, m = icp.mapUpdatePointDistance(ring(1500, r, 0.05), 0.02, normals_knn=k)
        assert app > 0
        check_resident_map(amd, oracle, icp, k, (step, 1), f"planar step {step}", planar=True, fresh_pass=True)


def test_resident_kth_d2_is_refused_when_it_describes_nothing(amd):
    icp = resident(amd, sc.make("plane_z0"))
    with pytest.raises(Exception):
        icp.debugResidentKthD2()                       # no tracked normals pass yet
    icp.mapUpdatePointDistance(sc.cloud(np.array([[3.0, 3.0, 0.5]])), 0.0, normals_knn=5)
    assert icp.debugResidentKthD2()[1] == 5
    assert icp.setMap(sc.make("lattice"))              # the resident copy replaced
    with pytest.raises(Exception):
        icp.debugResidentKthD2()
