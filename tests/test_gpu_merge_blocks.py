"""The rank-ordered merge of the map-growth epoch (csrc/ops.hip: merge_greedy) on blocks of DIFFERENT points, through the test seam
icpmi_debug_merge_blocks: every case of tests/merge_cases.py, in the per-block launches (mode 1) and in the epoch's own choice (mode 0),
against the brute-force reference of tests/merge_reference.py.  Everything is integer or bit-exact: no tolerances.
(tests/test_merge_reference_cpu.py certifies the cases and the reference without a GPU.)"""
import ctypes as C

import numpy as np
import pytest

import merge_cases as mc
import merge_reference as mr

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def icp(amd):
    """one handle for all cases: each meets the scratch, the status words and the filter the one before it left"""
    h = amd.ICPSequence(minimizer=1)
    yield h
    h.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def run(icp, c, mode):
    return icp.debugMergeBlocks(c["blocks"], c["min_dist"], stride=c["stride"], mode=mode)


def expected_path(c, mode):
    counts = [b.shape[0] for b in c["blocks"]]
    if sum(1 for n in counts if n) < 2 or c["min_dist"] <= 0:
        return 0
    return 2 if mode == 1 or c["stride"] * len(counts) > mr.SINGLE_LAUNCH_SPAN else 1


def check(c, got, mode):
    masks, merged, _ = mc.reference(c["name"])
    got_merged, got_kept, path = got
    assert path == expected_path(c, mode), (c["name"], mode, path)
    assert len(got_kept) == len(masks)
    for r, (g, m) in enumerate(zip(got_kept, masks)):
        assert np.array_equal(g, m), (c["name"], mode, "block", r, "differs at", np.nonzero(g != m)[0][:8])
    assert got_merged.shape[0] == merged.shape[0]
    assert np.array_equal(bits(got_merged), bits(merged))


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_in_both_modes(icp, name):
    c = mc.case(name)
    per_block, own = run(icp, c, 1), run(icp, c, 0)
    wrong = []
    for mode, got in ((1, per_block), (0, own)):        # (both are looked at before either fails: a fault names its kernel)
        try:
            check(c, got, mode)
        except AssertionError as e:
            wrong.append(f"mode {mode}: {str(e).splitlines()[0][:120]}")
    assert not wrong, "; ".join(wrong)
    assert np.array_equal(bits(per_block[0]), bits(own[0]))
    assert all(np.array_equal(a, b) for a, b in zip(per_block[1], own[1]))


def test_the_span_case_takes_the_per_block_launches_by_itself(icp):
    c = mc.case("span_above_2_22")
    assert c["stride"] * len(c["blocks"]) == 4194560
    assert run(icp, c, 0)[2] == 2


def test_copy_out_capacity_below_the_merged_set(icp):
    c = mc.case("ragged_stride_max_plus_1")
    _, merged, _ = mc.reference(c["name"])
    cap = merged.shape[0] // 3
    got, kept, path, full = icp.debugMergeBlocks(c["blocks"], c["min_dist"], stride=c["stride"], mode=0, capacity=cap)
    assert full == merged.shape[0] and got.shape[0] == cap and path == 1
    assert np.array_equal(bits(got), bits(merged[:cap]))
    got0, _, _, full0 = icp.debugMergeBlocks(c["blocks"], c["min_dist"], stride=c["stride"], mode=1, capacity=0)
    assert full0 == merged.shape[0] and got0.shape[0] == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_same_bits_twice_and_on_a_fresh_handle(amd, icp, mode):
    """the order inside a cell comes from atomics; the verdicts must not depend on it"""
    c = mc.case("hash_filter")
    a = run(icp, c, mode)
    b = run(icp, c, mode)
    fresh = amd.ICPSequence(minimizer=1)
    try:
        f = run(fresh, c, mode)
    finally:
        fresh.close()
    for other in (b, f):
        assert np.array_equal(bits(a[0]), bits(other[0])) and other[2] == a[2]
        assert all(np.array_equal(x, y) for x, y in zip(a[1], other[1]))
    check(c, a, mode)


@pytest.mark.parametrize("small", ["tpb_maxc_65_ranks_2", "chain_64_lines_70", "hash_wrap", "no_rule_one_block_of_five"])
def test_a_case_behind_a_larger_one(amd, small):
    """stale scratch, stale status words (2 = kept, all over the span) and a filter full of another case's cells"""
    h = amd.ICPSequence(minimizer=1)
    try:
        for mode in (0, 1):
            big = mc.case("hash_filter")
            check(big, run(h, big, 0), 0)
            c = mc.case(small)
            check(c, run(h, c, mode), mode)
    finally:
        h.close()


def test_the_seam_runs_the_epochs_merge(amd, small_scene, monkeypatch):
    """one loopback epoch of three simulated ranks: what icpmi_staged_merge_allgather merged is what the seam makes of the same three
    blocks, and what the reference makes of them"""
    shift, min_dist = 0.45, 0.3
    sc = small_scene
    monkeypatch.delenv("ICPMI_MERGE_BLOCK", raising=False)
    monkeypatch.setenv("ICPMI_COMM_LOOPBACK", "3")
    monkeypatch.setenv("ICPMI_COMM_LOOPBACK_SHIFT", repr(shift))
    h = amd.ICPSequence(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=30, use_differential=1)
    try:
        half, half_n = sc["map"][::2].copy(), sc["normals"][::2].copy()
        assert h.setMap(half, half_n)
        h.commInit(h.commUniqueId(), 1, 0)
        corr = h.registerWithPrior(sc["scan"], np.eye(4, dtype=F))
        keep, placed = h.stagedPointDistanceKeep(corr, min_dist)
        block0 = placed[keep]
        blocks = []
        for r in range(3):
            blk = block0.copy()
            if r:
                blk[:, 0] = blk[:, 0] + F(F(r) * F(shift))
            blocks.append(blk)
        mine, appended, _, epoch_merged = h.stagedMergeAllGather(corr, min_dist, normals_knn=0, return_merged=True)
        h.commDestroy()
        assert mine == block0.shape[0] and appended == epoch_merged.shape[0] > mine
        masks, merged, und = mr.merge(blocks, min_dist)
        assert not und
        assert np.array_equal(bits(epoch_merged), bits(merged))
        for mode in (0, 1):
            got, kept, path = h.debugMergeBlocks(blocks, min_dist, stride=32769, mode=mode)      # the one-collective layout's stride
            assert path == 1 + mode
            assert np.array_equal(bits(got), bits(epoch_merged))
            assert all(np.array_equal(k, m) for k, m in zip(kept, masks))
    finally:
        h.close()


def test_refusals(amd, icp):
    from norlab_icp_mapper_amd import _capi as capi
    lib, h = icp._lib, icp._h
    pts = np.zeros((8, 4), F)
    out = np.zeros((8, 4), F)
    mn, path = C.c_int64(0), C.c_int32(0)

    def call(pts_p, counts, n_ranks, stride, out_p=out.ctypes.data, cap=8):
        cnt = np.asarray(counts, np.int64)
        return lib.icpmi_debug_merge_blocks(h, pts_p, cnt.ctypes.data if cnt.size else None, n_ranks, stride, 0.2, 0, out_p, cap, C.byref(mn),
                                            None, C.byref(path))

    def refused(st, word):
        assert st == capi.ERR_INVALID_ARG
        assert word in lib.icpmi_last_error(h).decode()

    refused(call(pts.ctypes.data, [4, 4], 0, 4), "n_ranks")
    refused(call(pts.ctypes.data, [0] * 257, 257, 4), "n_ranks")
    refused(call(pts.ctypes.data, [4, -1], 2, 4), "counts[1]")
    refused(call(pts.ctypes.data, [4, 4], 2, 3), "stride")
    refused(call(None, [4, 4], 2, 4), "pts4")
    refused(call(pts.ctypes.data, [4, 4], 2, 4, out_p=None), "merged_out4")
    refused(call(pts.ctypes.data, [], 2, 4), "counts")
    with pytest.raises(amd.InvalidParameter, match="stride"):
        icp.debugMergeBlocks([pts[:4], pts[4:]], 0.2, stride=2)
    # the merge's own refusal: a span of 2^31 (nothing is allocated for it)
    st = call(pts.ctypes.data, [4, 4], 2, 1 << 30)
    assert st == capi.ERR_UNSUPPORTED and "too large" in lib.icpmi_last_error(h).decode()
    assert call(pts.ctypes.data, [4, 4], 2, 4) == capi.ICPMI_OK and mn.value == 8     # (coincident points: all kept)
