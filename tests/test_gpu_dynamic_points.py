"""DynamicPointsMapperModule on the device (csrc/dynpts.hip: a counting-sort bucket grid over (elevation, azimuth)) at the edges its search
can miss -- the cases of tests/dynamic_points_cases.py: both scan routes (half angles 0.001 / 0.0011), grids smaller than the 5 x 5 block,
the poles, the azimuth seam, angles on bucket edges, dense buckets, exact ties, wave-run shapes, the decision boundaries.  Bar: bit-equal
to the oracle's brute-force search, and on the flagged cases within the case's tolerance of the float64 restatement of the reference
(both yardsticks are held to each other by tests/test_dynamic_points_cpu.py).  Then the same module inside the resident map-update chain,
and the refusal of a half angle whose grid is too large: up front, with the resident map left whole."""
import numpy as np
import pytest

import dynamic_points_cases as dc
from test_gpu_map_chain import host_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def shared_handle(amd):
    """one handle for every case: the module's scratch is reused from table size to table size"""
    return amd.ICPSequence(minimizer=1)


def oracle_update(oracle, cid):
    T, beams, mp, nrm, p0, prm, _ = dc.case(cid)
    return oracle.dynamic_points_update(T, beams, mp, nrm, p0, nthreads=8, **dc.kwargs(prm))


def assert_bit_equal(got, ref, cid, what="device vs oracle"):
    prm = dc.case(cid)[5]
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
        f"{what}: case {cid}, parameters {prm}, first differing map indices {dc.first_diff(got, ref)} of {int((got.view(np.uint32) != ref.view(np.uint32)).sum())}"


@pytest.mark.parametrize("cid", dc.IDS)
def test_case_matches_oracle_and_float64(shared_handle, oracle, cid):
    T, beams, mp, nrm, p0, prm, flags = dc.case(cid)
    ref = oracle_update(oracle, cid)
    got = shared_handle.dynamicPointsUpdate(T, beams, mp, nrm, p0, **dc.kwargs(prm))
    assert_bit_equal(got, ref, cid)
    untouched = ref.view(np.uint32) == p0.view(np.uint32)
    assert np.array_equal(got.view(np.uint32)[untouched], p0.view(np.uint32)[untouched]), (cid, prm)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), (cid, prm)
    again = shared_handle.dynamicPointsUpdate(T, beams, mp, nrm, p0, **dc.kwargs(prm))     # the scatter order is arbitrary: the result is not
    assert_bit_equal(again, got, cid, "second call vs first")
    if flags["float64"]:
        err, at, share = dc.float64_error(cid, got)
        print(f"{cid}: device vs float64 {err:.3e} at map index {at}, sure share {share:.3f}, tol {dc.tol(cid):.3e}")
        assert share >= dc.SURE_SHARE, (cid, share)
        assert err <= dc.tol(cid), f"device vs float64: case {cid}, parameters {prm}, error {err:.3e} at map index {at}, tol {dc.tol(cid):.3e}"


def test_one_handle_across_grid_sizes(amd, oracle):
    """small -> huge (three-kernel scan) -> tiny -> small -> large (side scan) tables on one handle: no table sees another's counts"""
    icp = amd.ICPSequence(minimizer=1)
    for b in (0.03, 0.001, 2.0, 0.01, 0.0011):
        cid = f"generic-b{b}"
        T, beams, mp, nrm, p0, prm, _ = dc.case(cid)
        got = icp.dynamicPointsUpdate(T, beams, mp, nrm, p0, **dc.kwargs(prm))
        assert_bit_equal(got, oracle_update(oracle, cid), cid, "one handle across grid sizes")


# ---- inside the resident map-update chain ----------------------------------------------------------------------------------------------
def chain_shapes(dyn):
    return {"shipped": ([dyn, ("voxel", 0.3, 1)], [("surface_normals", 10), ("cut_scalar", 0.65, 1)]), "alone": ([dyn], [])}


def chain_inputs(b):
    T, beams, mp, nrm, p0, prm, _ = dc.case(f"generic-b{b}")
    scan_s = np.full(beams.shape[0], 0.6, np.float32)
    scan2 = beams.copy()
    scan2[:, :3] += np.float32(0.03)
    return T, beams, scan2, scan_s, mp, nrm, p0, prm


def assert_chain_equals(icp, oracle, what, m, src, ref):
    pts, nrm, sc, ref_src = ref
    got = icp.getMap()
    assert m == pts.shape[0] and got.shape[0] == pts.shape[0], (what, m, pts.shape[0])
    assert np.array_equal(src, ref_src), (what, np.flatnonzero(src != ref_src)[:10].tolist())
    assert np.array_equal(got.view(np.uint32), pts.view(np.uint32)), (what, "map", np.flatnonzero((got != pts).any(axis=1))[:10].tolist())
    gs = icp.getMapScalar()
    assert np.array_equal(gs.view(np.uint32), sc.view(np.uint32)), (what, "scalar", dc.first_diff(gs, sc))


@pytest.mark.parametrize("shape", ["shipped", "alone"])
@pytest.mark.parametrize("b", [0.001, 0.0011, 0.5])
def test_chain_equals_host_composition(amd, oracle, b, shape):
    """b = 0.001: the table is beyond the two-kernel scan, the chain may not fork the module onto its side stream; 0.0011 and 0.5 may"""
    T, scan, scan2, scan_s, mp, nrm, p0, prm = chain_inputs(b)
    modules, post = chain_shapes(dc.module(prm))[shape]
    icp = amd.ICPSequence(minimizer=1, max_dist=2.0, max_iterations=5)
    icp.setMap(mp, nrm)
    icp.setMapScalar(p0)
    src, m = icp.mapUpdateChain(scan, modules, post, scan_scalar=scan_s, to_sensor=T)
    ref = host_chain(oracle, mp, nrm, p0, scan, scan_s, T, modules, post)
    assert_chain_equals(icp, oracle, (b, shape, "first update"), m, src, ref)
    old = ref[3] < mp.shape[0]
    assert (ref[2][old] != p0[ref[3][old]]).sum() > 100             # the module moved the probabilities of old map points
    # a second scan on the same handle: the resident arrays are now the device's own product
    got, got_n = icp.getMap(with_normals=True)
    sc = icp.getMapScalar()
    src2, m2 = icp.mapUpdateChain(scan2, modules, post, scan_scalar=scan_s, to_sensor=T)
    ref2 = host_chain(oracle, got, got_n, sc.copy(), scan2, scan_s, T, modules, post)
    assert_chain_equals(icp, oracle, (b, shape, "second update"), m2, src2, ref2)


# ---- a half angle whose grid is too large ---------------------------------------------------------------------------------------------------
TOO_SMALL = 1e-4        # (pi / b + 2)(2 pi / b + 2) > 2^28


def test_stage_entry_refuses_a_too_small_half_angle(amd, oracle):
    cid = "generic-b0.01"
    T, beams, mp, nrm, p0, prm, _ = dc.case(cid)
    icp = amd.ICPSequence(minimizer=1)
    kw = dc.kwargs(prm)
    with pytest.raises(NotImplementedError, match="beamHalfAngle too small"):
        icp.dynamicPointsUpdate(T, beams, mp, nrm, p0, **dict(kw, beam_half_angle=TOO_SMALL))
    assert_bit_equal(icp.dynamicPointsUpdate(T, beams, mp, nrm, p0, **kw), oracle_update(oracle, cid), cid, "after a refused call")


@pytest.mark.parametrize("shape", ["shipped", "alone"])
def test_chain_refuses_a_too_small_half_angle_and_keeps_the_map(amd, oracle, shape):
    """the refusal comes before the chain touches anything: the resident map, its scalar and its normals are bit-identical afterwards,
    and the next valid update equals the host composition"""
    T, scan, _, scan_s, mp, nrm, p0, prm = chain_inputs(0.01)
    icp = amd.ICPSequence(minimizer=1, max_dist=2.0, max_iterations=5)
    icp.setMap(mp, nrm)
    icp.setMapScalar(p0)
    bad = dict(prm, beam_half_angle=TOO_SMALL)
    modules, post = chain_shapes(dc.module(bad))[shape]
    with pytest.raises(NotImplementedError, match="beamHalfAngle too small"):
        icp.mapUpdateChain(scan, modules, post, scan_scalar=scan_s, to_sensor=T)
    got, got_n = icp.getMap(with_normals=True)
    assert got.shape == mp.shape, "the refused update cost the caller the resident map"
    assert np.array_equal(got.view(np.uint32), mp.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(icp.getMapScalar().view(np.uint32), p0.view(np.uint32))
    modules, post = chain_shapes(dc.module(prm))[shape]
    src, m = icp.mapUpdateChain(scan, modules, post, scan_scalar=scan_s, to_sensor=T)
    assert_chain_equals(icp, oracle, (shape, "after a refused update"), m, src, host_chain(oracle, mp, nrm, p0, scan, scan_s, T, modules, post))
