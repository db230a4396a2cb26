"""The quantile selection of the outlier-filter chain on distances built to break it (tests/selection_cases.py), against the integer-exact
reference (tests/selection_reference.py, held to the oracle by tests/test_selection_cpu.py).  The limit is one element of the multiset of
positive finite d2 bit patterns and the pair count is a count: every comparison below is bitwise / exact, except the FRMS comparison of
VarTrimmedDist.

  (a) the legacy 11/11/10 selection (sel_hist_kernel / sel_scan_kernel) through icpmi_outlier_weights on the arrays themselves;
  (b) VarTrimmedDist (vt_*_kernel) through the same entry: the limit names a rank whose float64 FRMS is within 1e-12 relative of the
      reference's minimum -- the bound on two float64 summation orders over <= 1e5 terms, not a measurement; on tied data the ranks of one
      FRMS value are undecidable between summation orders;
  (c) the fused selection behind a matcher launch, on the lattice geometry of selection_cases.py: level 0 from the k = 1 matcher, from
      sel2_hist0_kernel and from nnk_wg_kernel's speculative window (default handle and sel_window_off = 1: the same bits), level 1 from
      sel2_scan_hist_kernel, the last level inside the pair-sum kernel.  After every fixed-iteration registration the distances the device
      selected over are read back (lastMatches) and the limit, the pair count and the used ratio are checked on THEM.  Which iterations the
      window serves follows from the reference's own prefixes (a window of seven 16-bit prefixes from max(previous prefix - 3, 0) on) and is
      compared with icpmi_debug_counters slots 12 / 13 run by run;
  (d) a batch (blockIdx.y = reading, per-reading histogram strides) against the same readings registered alone.

Order of the distances: the loop's matcher writes d2 in its tile-sorted query order, so `ascending by index` of a reading is not the order
sel2_hist0_kernel reads; the array cases of (a) keep their order."""
import numpy as np
import pytest

import selection_cases as sc
import selection_reference as sr
from test_selection_cpu import VT_CHAINS, chains_of, same_bits

pytestmark = pytest.mark.gpu

WIN_BINS = 7        # common.h: ICPMI_WIN_BINS
HIT, MISS = 12, 13  # icpmi_debug_counters: iterations served by the window / by the full level 0 behind a window that missed


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


# ------------------------------------------------------------------------------------------------------------------ (a) legacy, on arrays
@pytest.mark.parametrize("cid", sc.ARRAY_IDS)
def test_legacy_selection_on_the_arrays(amd, oracle, cid):
    from norlab_icp_mapper_amd.icp import ConvergenceError
    c = sc.array_case(cid)
    for k in (1, 6):
        d2 = c.make(k)
        c.check(d2)
        ids = np.zeros(d2.shape, np.int32)
        for chain in chains_of(c, d2):
            icp = amd.ICPSequence(minimizer=1, knn=k, max_dist=sc.MAX_DIST, outliers=chain)
            if c.invalid:
                err, _, _ = oracle.outlier_weights(oracle.make_config(outliers=chain), d2, ids)
                assert err == sr.ORACLE_NO_OUTLIER_TO_FILTER
                with pytest.raises(ConvergenceError, match="no outlier to filter"):
                    icp.outlierWeights(d2, ids)
                continue
            w, lim = icp.outlierWeights(d2, ids)
            rw, rlim = sr.chain(chain, d2)
            print(f"{cid} k={k} {chain}: limit {float(lim)!r} reference {float(rlim)!r}")
            assert same_bits(lim, rlim), (cid, k, chain, float(lim), float(rlim))
            assert np.array_equal(w, rw), (cid, k, chain, int((w != rw).sum()))


# ------------------------------------------------------------------------------------------------------------------ (b) VarTrimmedDist
@pytest.mark.parametrize("cid", [c.id for c in sc.ARRAYS if c.vt])
def test_var_trimmed_on_the_arrays(amd, cid):
    c = sc.array_case(cid)
    for k in (1, 6):
        d2 = c.make(k)
        c.check(d2)
        s = sr.sorted_bits(d2)
        fr, N = sr.frms(d2, 0.95)
        for chain in VT_CHAINS:
            _, minr, _, maxr, lam = chain[0]
            icp = amd.ICPSequence(minimizer=1, knn=k, max_dist=sc.MAX_DIST, outliers=chain)
            w, lim = icp.outlierWeights(d2, np.zeros(d2.shape, np.int32))
            lo = int(np.floor(np.float32(minr) * np.float32(N))); hi = min(int(np.floor(np.float32(maxr) * np.float32(N))), s.size)
            if hi > lo:     # every rank whose FRMS is the minimum to within the summation-order bound
                cand = lo + np.nonzero(fr[lo:hi] <= fr[lo:hi].min() * (1.0 + 1e-12))[0]
            else:
                cand = np.array([lo])
            limits = {int(s[sr.rank(s.size, np.float32(i) / np.float32(N))]) for i in cand.tolist()}
            got = int(np.array([lim], np.float32).view(np.uint32)[0])
            print(f"{cid} k={k} {chain}: limit {float(lim)!r}, {cand.size} ranks at the minimum, reference ratio {float(sr.var_trimmed(d2, minr, maxr, lam)[0])!r}")
            assert got in limits, (cid, k, chain, float(lim), cand[:8].tolist())
            assert np.array_equal(w, (d2 <= np.float32(lim)).astype(np.float32)), (cid, k, chain)


# ------------------------------------------------------------------------------------------------------------------ (c) fused, through the loop
def prefix_of(limit):
    return int(np.array([limit], np.float32).view(np.uint32)[0]) >> 16


def window_serves(prev_prefix, prefix):
    lo = prev_prefix - WIN_BINS // 2 if prev_prefix > WIN_BINS // 2 else 0
    return lo <= prefix < lo + WIN_BINS


def check_run(tag, c, k, j, ratio, n, icp, T):
    """one fixed-iteration registration against the reference on the distances it selected over; returns what two handles must share"""
    st = icp.stats
    ids, d2, T_used = icp.lastMatches()
    sums, limits, _, _ = icp.lastSums()
    assert st.iterations == j, (tag, st.iterations)
    if j == 1:
        assert np.array_equal(T_used, np.eye(4, dtype=np.float32)), tag
    if c is not None:
        c.check(d2, ratio, j == 1 and c.T_init is None)
    ref = sr.quantile(d2, ratio)
    pairs = int((d2 <= ref).sum())
    print(f"{tag}: limit {float(limits[0])!r} reference {float(ref)!r}, pairs {st.pairs} reference {pairs}, valid {sr.sorted_bits(d2).size}")
    assert same_bits(limits[0], ref), (tag, "limits[slot]", float(limits[0]), float(ref))
    assert same_bits(st.trimmed_limit, ref), (tag, "stats.trimmed_limit", float(st.trimmed_limit), float(ref))
    assert sums[28] == st.pairs == pairs, (tag, "pairs", sums[28], st.pairs, pairs)
    assert np.float32(st.weighted_point_used_ratio) == np.float32(sums[27] / (k * n)), (tag, st.weighted_point_used_ratio, sums[27] / (k * n))
    return dict(T=np.asarray(T).tobytes(), pairs=int(st.pairs), limit=prefix_of(ref), bits=np.float32(st.trimmed_limit).tobytes(),
                ratio=np.float32(st.weighted_point_used_ratio).tobytes(), sums=sums.tobytes(), d2=d2.tobytes())


_runs = {}


def run_loop_case(amd, cid, k, iterations=(1, 2, 3, 4)):
    """{j: (window hits, window misses, selected 16-bit prefix)} of the default handle's j-iteration run, every run checked; cached per (case, k)"""
    import torch
    if (cid, k) in _runs:
        return _runs[(cid, k)]
    c = sc.loop_case(cid)
    mp, nm = sc.lattice_map(k)
    rd = sc.loop_reading(c, k)
    n = rd.shape[0]
    ratio = c.ratio(k)
    kw = dict(minimizer=c.minimizer, knn=k, max_dist=sc.MAX_DIST, outliers=[(sr.TRIMMED, ratio)], max_iterations=40, use_differential=0)
    handles = [amd.ICPSequence(**kw)] + ([amd.ICPSequence(sel_window_off=1, **kw)] if k > 1 else [])
    for icp in handles:
        assert icp.setMap(mp, nm)
        assert np.array_equal(icp.getMapMean(), np.zeros(3, np.float32)), "the lattice is symmetric: the centred frame is the caller's"
        icp.keepSums(1)
    d = torch.from_numpy(rd).cuda()
    out, prefixes = {}, {}
    for j in iterations:
        got = []
        for h, icp in enumerate(handles):
            T = icp.registerDev(d.data_ptr(), n, fixed_iterations=j)
            got.append((check_run(f"{cid} k={k} j={j} handle {h}", c, k, j, ratio, n, icp, T), icp.debugCounters()))
        prefixes[j] = got[0][0]["limit"]
        hits, misses = int(got[0][1][HIT]), int(got[0][1][MISS])
        if k > 1:
            assert got[0][0] == got[1][0], (cid, k, j, "the default handle and sel_window_off = 1 differ")
            assert int(got[1][1][HIT]) == 0 and int(got[1][1][MISS]) == 0
            # iteration i >= 3 looks at the window around the prefix of iteration i - 1 (the last iteration of the (i - 1)-run)
            want = [window_serves(prefixes[i - 1], prefixes[i]) for i in range(3, j + 1)] if all(i in prefixes for i in range(2, j + 1)) else None
            print(f"{cid} k={k} j={j}: prefixes {prefixes}, window hits {hits} misses {misses}, expected {want}")
            assert hits + misses == max(j - 2, 0), (cid, k, j, hits, misses)
            if want is not None:
                assert (hits, misses) == (sum(want), len(want) - sum(want)), (cid, k, j, hits, misses, want, prefixes)
        else:
            assert hits == 0 and misses == 0
        out[j] = (hits, misses, prefixes[j])
    _runs[(cid, k)] = out
    return out


@pytest.mark.parametrize("cid,k", [(c.id, k) for c in sc.LOOP for k in c.ks])
def test_fused_selection_through_the_loop(amd, cid, k):
    """k = 1: the matcher builds level 0; k = 6, 16: sel2_hist0_kernel or the window, and the handle with the window off"""
    run_loop_case(amd, cid, k)


def test_window_hits_and_misses_are_both_covered(amd):
    """Over the committed k > 1 cases the window served some iteration and missed, after iteration 2, in another.  The mirrored readings
    keep the pose at the identity, so their prefix stays and the window serves them -- tiny_mixed with a window clamped to prefix 0
    (win_lo = 0: the header word is 1, the selected bin is lo1 - 1 + b) and, on the other side of the cluster boundary, around the prefix
    of 1.0.  The misses come from the readings whose distances move between iterations: the misaligned readings still shrink from
    iteration 2 to 3 (a miss `below`), the float_rank readings, without mirror images, settle upwards (a miss `above`)."""
    served = run_loop_case(amd, "all_equal", 6)
    assert served[4][:2] == (2, 0), served
    low = run_loop_case(amd, "tiny_mixed-last_tiny", 6)
    high = run_loop_case(amd, "tiny_mixed-first_of_cluster", 16)
    print("tiny_mixed:", low, high)
    assert low[4][0] > 0 and all(low[j][2] <= WIN_BINS // 2 for j in (2, 3, 4)), low      # hits inside a clamped window
    assert high[4][0] > 0 and high[4][2] == prefix_of(1.0), high
    missed = {cid: run_loop_case(amd, cid, 6) for cid in ("misaligned-p2p", "misaligned-p2plane", "float_rank-0.7-480", "float_rank-0.9-480")}
    print("window (hits, misses, prefix) by run:", missed)
    # the prefix steps of the iterations that missed (iteration j missed: the j-run counts one miss more than the (j - 1)-run)
    jumps = [runs[j][2] - runs[j - 1][2] for runs in missed.values() for j in (3, 4) if runs[j][1] > runs[j - 1][1]]
    assert any(d > WIN_BINS // 2 for d in jumps) and any(d < -(WIN_BINS // 2) for d in jumps), (jumps, missed)     # a miss above and a miss below


@pytest.mark.parametrize("n,window", [(65_537, True), (131_073, False)])
def test_count_edges(amd, n, window):
    """k = 16: the first count at which sel2_hist0_kernel's tail loop runs (16 n > 4096 x 256), and the first at which the window is off
    (16 n >= 2^21: slots 12 / 13 stay 0); wide distances"""
    import torch
    k = 16
    mp, nm = sc.lattice_map(k)
    rd = sc.count_edge_reading(n)
    assert (k * n > (1 << 21)) != window and k * n > (1 << 20)
    kw = dict(minimizer=1, knn=k, max_dist=sc.MAX_DIST, outliers=[(sr.TRIMMED, 0.5)], max_iterations=40, use_differential=0)
    handles = [amd.ICPSequence(**kw), amd.ICPSequence(sel_window_off=1, **kw)]
    d = torch.from_numpy(rd).cuda()
    prefixes = {}
    for icp in handles:
        assert icp.setMap(mp, nm)
        icp.keepSums(1)
    for j in (1, 2, 3):
        got = []
        for h, icp in enumerate(handles):
            T = icp.registerDev(d.data_ptr(), n, fixed_iterations=j)
            got.append((check_run(f"count edge n={n} j={j} handle {h}", None, k, j, 0.5, n, icp, T), icp.debugCounters()))
        assert got[0][0] == got[1][0]
        prefixes[j] = got[0][0]["limit"]
        d2 = np.frombuffer(got[0][0]["d2"], np.float32)
        if j == 1:
            sc.check_wide(d2, 0.5, False)
        hits, misses = int(got[0][1][HIT]), int(got[0][1][MISS])
        assert int(got[1][1][HIT]) == 0 and int(got[1][1][MISS]) == 0
        if not window or j < 3:
            assert hits == 0 and misses == 0, (n, j, hits, misses)
        else:
            want = window_serves(prefixes[2], prefixes[3])
            assert (hits, misses) == (int(want), int(not want)), (n, hits, misses, prefixes)


# ------------------------------------------------------------------------------------------------------------------ (d) batch
def batch_readings():
    inf_reading = sc.place(np.full(300, np.inf, np.float32), central=np.zeros(300, bool), mirror=False)
    return [("size-1", sc.place(np.array([0.04], np.float32), central=np.zeros(1, bool), mirror=False)),
            ("size-255", sc.loop_case("size-255").reading(1)),
            ("wide", sc.loop_case("wide-shuffled").reading(1)),
            ("all_inf", inf_reading),
            ("all_equal", sc.loop_case("all_equal").reading(1)),
            ("size-257", sc.loop_case("size-257").reading(1)),
            ("mostly_invalid", sc.loop_case("mostly_invalid").reading(1))]


@pytest.mark.parametrize("fixed", [1, 3])
def test_batch_equals_single(amd, fixed):
    import torch
    from norlab_icp_mapper_amd.icp import ConvergenceError
    mp, nm = sc.lattice_map(1)
    icp = amd.ICPSequence(minimizer=1, knn=1, max_dist=sc.MAX_DIST, outliers=[(sr.TRIMMED, 0.85)], max_iterations=40, use_differential=0)
    assert icp.setMap(mp, nm)
    rds = batch_readings()
    dev = [torch.from_numpy(r).cuda() for _, r in rds]
    single = []
    for (name, _), d in zip(rds, dev):
        try:
            T = icp.registerDev(d.data_ptr(), d.shape[0], fixed_iterations=fixed)
            single.append((T, int(icp.stats.iterations), int(icp.stats.pairs), np.float32(icp.stats.trimmed_limit)))
        except ConvergenceError as e:
            single.append(str(e))
        print(f"{name} alone: {single[-1] if isinstance(single[-1], str) else single[-1][1:]}")
    assert isinstance(single[3], str) and "no outlier to filter" in single[3]
    assert not isinstance(single[2], str) and not isinstance(single[4], str) and not isinstance(single[6], str)
    for rep in range(2):
        Ts, stats, status = icp.registerBatchDev([d.data_ptr() for d in dev], [d.shape[0] for d in dev], fixed_iterations=fixed)
        print("batch status", status)
        assert status[3] == sr.NO_OUTLIER_TO_FILTER and np.array_equal(Ts[3], np.eye(4, dtype=np.float32))
        for b, ((name, _), s) in enumerate(zip(rds, single)):
            if isinstance(s, str):
                assert status[b] != 0 and np.array_equal(Ts[b], np.eye(4, dtype=np.float32)), (name, status[b], s)
                continue
            T, it, pairs, lim = s
            assert status[b] == 0, (name, status[b])
            assert np.array_equal(Ts[b], T), (name, fixed, np.abs(Ts[b] - T).max())
            assert (int(stats[b].iterations), int(stats[b].pairs)) == (it, pairs), (name, stats[b].iterations, stats[b].pairs, it, pairs)
            assert same_bits(stats[b].trimmed_limit, lim), (name, float(stats[b].trimmed_limit), float(lim))
