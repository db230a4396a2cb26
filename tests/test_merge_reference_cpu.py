"""The cases of tests/merge_cases.py and the reference of tests/merge_reference.py, checked on the CPU before any kernel is compared with
them: (a) the brute-force reference equals the composition the loopback test trusts -- the oracle's PointDistance rule applied block by
block; (b) no verdict of a case hangs on the last bit of a d2 (outside the threshold pairs, exact by construction); (c) the cases are not
trivial; (d) the properties a case was built for -- probes that wrap the table, keys that share a home slot, aliasing cells, filter false
positives, a span above the single launch's limit -- are really there.  Run with -s for the per-case figures."""
import numpy as np
import pytest

import merge_cases as mc
import merge_reference as mr
import residual_reference as rr

F = np.float32


def test_the_distance_chain_is_the_matchers():
    rng = np.random.default_rng(0)
    p, q = rng.normal(size=(500, 3)).astype(F), rng.normal(size=(300, 3)).astype(F)
    got = mr.d2_rows(p, q)
    for j in range(0, 300, 37):
        assert np.array_equal(got[:, j], rr.sqdist3_f32(p, np.broadcast_to(q[j], p.shape)))


@pytest.mark.parametrize("name", mc.NAMES)
def test_case(name, oracle):
    c = mc.case(name)
    blocks, md = c["blocks"], c["min_dist"]
    counts = [b.shape[0] for b in blocks]
    masks, merged, und = mc.reference(name)
    assert sum(counts) <= 21000 and all(b.dtype == F and b.shape[1] == 4 for b in blocks)
    assert all(n <= c["stride"] for n in counts)
    shares = [round(float(m.mean()), 3) if m.size else None for m in masks]
    facts = mr.hash_facts(blocks, md) if md > 0 and sum(counts) else {}
    shown = counts if len(counts) <= 16 else f"{len(counts)} blocks, {sum(1 for n in counts if n)} non-empty, largest {max(counts)}"
    print(f"\n{name}: min_dist {md} stride {c['stride']} blocks {shown}\n  kept shares {shares if len(counts) <= 16 else '...'}"
          f" merged {merged.shape[0]}\n  undecidable {len(und)} (exempt {len(c['exempt'])})\n  hash {facts}")
    # (a) the oracle's rule, block by block
    acc = np.zeros((0, 4), F)
    for b, m in zip(blocks, masks):
        if b.shape[0] == 0:
            continue
        k = np.ones(b.shape[0], bool) if acc.shape[0] == 0 or md <= 0 else oracle.point_distance_keep(acc, b, md, nthreads=4)
        assert np.array_equal(k, m)
        acc = np.concatenate([acc, b[k]])
    assert np.array_equal(acc.view(np.uint32), merged.view(np.uint32))
    # (b) decidable
    assert set(und) <= c["exempt"], sorted(set(und) - c["exempt"])[:5]
    for (r, i), (rq, iq) in c["exempt"]:
        p, q = blocks[r][i], blocks[rq][iq]
        assert p[1] == q[1] and p[2] == q[2] and q[0] == 0          # axis-aligned from x = 0: d2 = fl(p.x * p.x), one rounding
    # (c) not trivial
    if c["expect"] is not None:
        for m, e in zip(masks, c["expect"]):
            assert np.array_equal(m, e)
    if c["group"] not in ("chain", "thresholds", "no_rule"):
        first = next(r for r, n in enumerate(counts) if n)
        for r in range(first + 1, len(counts)):
            if counts[r] >= 100:
                assert 0.10 <= masks[r].mean() <= 0.90, (r, counts[r], masks[r].mean())
    # (d) certified
    cert = c["certify"]
    if "cap" in cert:
        assert facts["cap"] == cert["cap"]
    if cert.get("wrapped"):
        assert facts["wrapped"] and facts["cells"] > 2
    if "max_home_at_least" in cert:
        assert facts["max_home"] >= cert["max_home_at_least"]
    if "false_positives_at_least" in cert:
        assert facts["false_positives"] >= cert["false_positives_at_least"]
        assert facts["longest_miss"] >= cert["longest_miss_at_least"]
    if cert.get("alias"):
        cells = mr.point_cells(blocks, md)
        assert cells[1, 0] - cells[0, 0] == 2 ** 21 and np.array_equal(cells[1, 1:], cells[0, 1:])
        assert mr.cell_key(cells[1]) == mr.cell_key(cells[0])
    if cert.get("span_above"):
        assert c["stride"] * len(blocks) > mr.SINGLE_LAUNCH_SPAN and len(blocks) == 256
    elif sum(counts):
        assert c["stride"] * len(blocks) <= mr.SINGLE_LAUNCH_SPAN


def test_thresholds_are_the_ones_asked_for():
    """which d2 the axis-aligned pairs reach: fl(dx * dx) does not hit every float32, so say what was hit"""
    eps = mr.FLT_EPSILON
    for md in (0.5, 0.3):
        c = mc.case(f"thresholds_{md}")
        lim = float(F(md)) ** 2
        got = dict(c["pairs"])
        bits = lambda v: int(F(v).view(np.uint32))
        below = F(lim) if float(F(lim)) < lim else np.nextafter(F(lim), F(0))          # the largest float32 below lim
        print(f"\nthresholds_{md}: lim {lim!r}; d2 in ulps from FLT_EPSILON:", {k: bits(got[k]) - bits(eps) for k in ("at_eps", "above_eps")},
              "in ulps from the float32 below lim:", {k: bits(v) - bits(below) for k, v in got.items() if k.endswith("lim")})
        assert got["zero"] == 0 and got["at_eps"] <= eps < got["above_eps"]
        assert got["below_lim"] < lim <= got["above_lim"]
        # (2^-23 has no float32 square root and squares skip floats: each pair is within 2 ulps of its threshold, on the right side)
        assert bits(eps) - bits(got["at_eps"]) <= 2 and bits(got["above_eps"]) - bits(eps) <= 2
        assert bits(below) - bits(got["below_lim"]) <= 2 and bits(got["above_lim"]) - bits(below) <= 3
        if md == 0.5:
            assert lim == 0.25 and got["at_lim"] == 0.25                                # lim itself: kept, the comparison is strict


@pytest.mark.parametrize("md", [0.3, 0.05])
def test_cell_edge_margin_holds_at_the_faces_searched(md):
    """the margin h = 1.001 minDist + 1e-6: of all near pairs drawn across cell faces, far from the origin and at the power-of-two cell
    indices where the product's spacing doubles, none may end up two cells apart"""
    searched, widest, pairs = mc.face_search(md)
    print(f"\nmin_dist {md}: {searched} near pairs across faces at cells +-{mc.FACE_CELLS}; widest cell gap {widest}; {len(pairs)} kept as a case")
    assert searched > 1000000 and widest == 1
