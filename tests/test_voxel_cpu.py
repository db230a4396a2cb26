"""VoxelMatcher without a GPU: the float64 reference (tests/voxel_reference.py) against the plane-to-plane reference it degenerates to and
against the figures of the prototype the feature rests on; the record the GPU tests take their allowances from; both YAML front ends; the
C ABI's symbols, and the pinned size and version."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import localizability_reference as lr
import plane_to_plane_reference as pr
import voxel_cases as vc
import voxel_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_one_point_per_voxel_is_plane_to_plane_on_the_same_pairs():
    """every map point alone in its voxel: mu is the point, N = n n^T, and the sums are plane_to_plane_reference.reference_sums' on the
    pairs (reading point, the map point of its voxel)"""
    rng = np.random.default_rng(7)
    size = 0.5
    cells = rng.permutation(20 * 20 * 20)[:600]
    ijk = np.stack([cells // 400 - 10, (cells // 20) % 20 - 10, cells % 20 - 10], 1)
    mp = ((ijk + rng.uniform(0.1, 0.9, ijk.shape)) * size).astype(F32)
    # (map normals along the axes, scaled by powers of two: their float32 normalisation -- the table's -- is exact, so it is the float64
    # one of reference_sums; the reading's normals are arbitrary, both references normalise them in float64)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    mn = (axes[rng.integers(0, 6, 600)] * 2.0 ** rng.integers(-2, 3, (600, 1))).astype(F32)
    tab = vr.table(mp, mn, size)
    assert tab["keys"].size == 600 and (tab["count"] == 1).all()
    assert np.array_equal(tab["mu"], mp[np.argsort(vr.pack_keys(ijk))].astype(np.float64))
    rd = (mp[rng.integers(0, 600, 900)] + rng.normal(scale=0.05, size=(900, 3))).astype(F32)
    rn = rng.normal(size=rd.shape).astype(F32)
    vox = vr.lookup(tab, rd)
    assert (vox >= 0).sum() > 600 and (vox < 0).sum() > 0        # (some fall over a face into an empty voxel)
    order = np.argsort(vr.pack_keys(ijk))                         # table order -> map index
    hit = vox >= 0
    ours = vr.reference_sums(rd, rn, vox, tab, 1e-3)
    theirs = pr.reference_sums(rd[hit], mp[order[vox[hit]]], mn[order[vox[hit]]], rn[hit], 1e-3)
    assert ours[28] == theirs[28] == hit.sum()
    assert pr.rel_distance(ours, theirs) <= 1e-12                 # (float64 round-off: N = u u^T is formed in another order than C(n))


def test_keys_follow_the_float32_floor():
    size = 0.5
    q = np.array([[-0.125, 0.0, 0.5], [0.49999997, -0.5, -0.50000006], [np.nan, 0, 0], [0, np.inf, 0], [524287.75, 0, 0], [524288.0, 0, 0],
                  [-524288.0, 0, 0], [-524288.03125, 0, 0]], F32)
    ok, ijk = vr.voxel_index(q, size)
    assert ok.tolist() == [True, True, False, False, True, False, False, False]
    assert ijk[0].tolist() == [-1, 0, 1] and ijk[1].tolist() == [0, -1, -2] and ijk[4, 0] == 2 ** 20 - 1
    keys = vr.pack_keys(np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [-1, 0, 0]]))
    assert keys[4] < keys[0] < keys[1] < keys[2] < keys[3] and int(keys[3]) < 2 ** 63


def test_prototype_figures_are_reproduced_and_recorded():
    """the room registration of the issue's table, by the committed float64 loop, and profiles/voxel_tolerance.json holds what it gives"""
    rec = vc.recorded()
    sc, rd, rn, truth = vc.registration_inputs()
    for size, (pt, prot, pit, ppairs) in vc.PROTOTYPE.items():
        r = vr.register(sc["map"], sc["normals"], rd, rn, size, 64)
        et, er = vr.centroid_error(r["T"], truth, rd)
        print(f"size {size}: {et:.3e} m / {er:.3e} rad, {r['iterations']} iterations, {r['pairs'][0]} of {rd.shape[0]} pairs in the first")
        assert abs(et / pt - 1) <= vc.PROTOTYPE_REL
        if prot is not None:
            assert abs(er / prot - 1) <= vc.PROTOTYPE_REL
            assert r["iterations"] == pit and r["pairs"][0] == ppairs
        got = rec["registration_room"][str(size)]
        assert got["float64_trans_err"] == pytest.approx(et, rel=1e-6) and got["float64_iterations"] == r["iterations"]
        assert got["float64_pairs_first"] == r["pairs"][0]
    # the accuracy floor is the voxel-mean bias and grows with the voxel; the nearest-neighbour step sits below all of them
    e = [rec["registration_room"][s]["float64_trans_err"] for s in ("0.5", "1.0", "2.0")]
    assert e[0] < e[1] < e[2] and rec["nearest_neighbour_plane_to_plane_room"]["trans_err"] < e[0]
    assert abs(rec["nearest_neighbour_plane_to_plane_room"]["trans_err"] / 9.2e-6 - 1) <= vc.PROTOTYPE_REL
    # (its iteration count is 5 here against the prototype's 4: the last step sits at the Differential checker's threshold; not asserted)
    # the float32 loop's distance from the float64 loop is small against the method's own error (what the GPU registration test rests on)
    for s in ("0.5", "1.0"):
        assert 20 * rec["registration_room"][s]["float32_from_float64_trans"] <= rec["registration_room"][s]["float64_trans_err"]


def test_recorded_sum_tolerances_are_what_the_script_measures():
    rec = vc.recorded()
    assert set(rec["rel_sums"]) == {vc.case_key(*c) for c in vc.SUM_CASES}
    name, pose, size, variant = vc.SUM_CASES[3]
    c = vc.sum_inputs(name, pose, size, variant)
    d = pr.rel_distance(vr.float32_sums(c["p"], c["npr"], c["vox"], vr.table_f32(c["tab"])), vr.reference_sums(c["p"], c["npr"], c["vox"], c["tab"]))
    assert d == pytest.approx(rec["rel_sums"][vc.case_key(name, pose, size, variant)], rel=1e-6)
    assert 0 < max(rec["rel_sums"].values()) < 1e-3 and 0 < rec["max_rel_step"] < 1e-4


def test_float32_table_is_one_rounding_of_the_float64_one():
    c = vc.sum_inputs("room", "true", 1.0)
    t32 = vr.table_f32(c["tab"])
    assert t32["mu"].dtype == F32 and np.array_equal(t32["mu"], c["tab"]["mu"].astype(F32))
    assert c["tab"]["count"].sum() == c["mc"].shape[0] and (c["tab"]["N"][:, [0, 3, 5]].sum(1) <= 1 + 1e-6).all()


# ------------------------------------------------------------------------------------------------------------------ YAML (Python front end)
CHAIN = {"matcher": {"VoxelMatcher": {"voxelSize": 0.5}}, "errorMinimizer": {"PlaneToPlaneErrorMinimizer": {"epsilon": 0.01}},
         "transformationCheckers": [{"CounterTransformationChecker": {"maxIterationCount": 40}}]}


def _cfg(**over):
    from norlab_icp_mapper_amd import icp
    return icp.config_from_yaml_chain({**CHAIN, **over})


def test_python_yaml():
    from norlab_icp_mapper_amd import icp
    c = _cfg()
    assert c.voxel_size == 0.5 and c.minimizer == 3 and c.n_outlier == 0 and c.plane_epsilon == 0.01 and not hasattr(c, "plane_model")
    assert _cfg(matcher="VoxelMatcher").voxel_size == 1.0
    assert not hasattr(_cfg(matcher={"KDTreeMatcher": {"knn": 1}}), "voxel_size")
    for bad in ({"voxelSize": 0.5, "knn": 1}, {"voxelsize": 0.5}, {"maxDist": 1.0}):
        with pytest.raises(icp.InvalidParameter, match="VoxelMatcher: unknown parameter"):
            _cfg(matcher={"VoxelMatcher": bad})
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(icp.InvalidParameter, match="VoxelMatcher: voxelSize"):
            _cfg(matcher={"VoxelMatcher": {"voxelSize": bad}})
    with pytest.raises(icp.InvalidParameter, match="voxel matcher.*outlier filters"):
        _cfg(outlierFilters=[{"TrimmedDistOutlierFilter": {"ratio": 0.85}}])
    with pytest.raises(icp.InvalidParameter, match="voxel matcher.*PlaneToPlaneErrorMinimizer only"):
        _cfg(errorMinimizer="PointToPlaneErrorMinimizer")
    with pytest.raises(icp.InvalidParameter, match="voxel matcher.*PlaneToPlaneErrorMinimizer only"):
        _cfg(errorMinimizer="PointToPointErrorMinimizer")
    with pytest.raises(icp.InvalidParameter, match="voxel matcher.*symmetric pair model"):
        _cfg(errorMinimizer="SymmetricPointToPlaneErrorMinimizer")
    with pytest.raises(icp.InvalidParameter, match="voxelSize"):
        icp.ICPSequence(minimizer=3, voxel_size=-1.0)             # (checked before the handle is created)


# ------------------------------------------------------------------------------------------------------------------ the C++ shell
def parse_voxel_chain(yaml_icp):
    """nim_test_parse_voxel_chain (host/TestHooks.cpp): what loadFromYamlNode reads of the chain for VoxelMatcher, or RuntimeError"""
    import host_bindings as hb
    fn = hb.load().nim_test_parse_voxel_chain
    fn.restype = C.c_int
    size, mini, model = C.c_float(-1), C.c_int(-1), C.c_int(-1)
    err = C.create_string_buffer(512)
    if fn(yaml_icp.encode(), C.byref(size), C.byref(mini), C.byref(model), err, C.c_int(512)):
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(voxel_size=size.value, minimizer=mini.value, model=model.value)


P2PL = "errorMinimizer:\n  PlaneToPlaneErrorMinimizer:\n    epsilon: 0.01\n"


def test_cpp_yaml():
    assert parse_voxel_chain("matcher:\n  VoxelMatcher:\n    voxelSize: 0.5\n" + P2PL) == dict(voxel_size=0.5, minimizer=3, model=0)
    assert parse_voxel_chain("matcher: VoxelMatcher\n" + P2PL)["voxel_size"] == 1.0
    assert parse_voxel_chain("matcher:\n  KDTreeMatcher:\n    knn: 1\n" + P2PL)["voxel_size"] == 0.0
    for bad in ("knn: 1", "maxDist: 2.0", "voxelsize: 0.5"):
        with pytest.raises(RuntimeError, match="VoxelMatcher: unknown parameter"):
            parse_voxel_chain("matcher:\n  VoxelMatcher:\n    %s\n" % bad + P2PL)
    for bad in ("0", "-1.0"):
        with pytest.raises(RuntimeError, match="VoxelMatcher: voxelSize"):
            parse_voxel_chain("matcher:\n  VoxelMatcher:\n    voxelSize: %s\n" % bad + P2PL)
    vm = "matcher:\n  VoxelMatcher:\n    voxelSize: 0.5\n"
    with pytest.raises(RuntimeError, match="voxel matcher.*outlier filters"):
        parse_voxel_chain(vm + "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.85\n" + P2PL)
    with pytest.raises(RuntimeError, match="voxel matcher.*PlaneToPlaneErrorMinimizer only"):
        parse_voxel_chain(vm + "errorMinimizer: PointToPlaneErrorMinimizer\n")
    with pytest.raises(RuntimeError, match="voxel matcher.*symmetric pair model"):
        parse_voxel_chain(vm + "errorMinimizer: SymmetricPointToPlaneErrorMinimizer\n")


def test_front_ends_word_the_refusals_as_the_c_call_does():
    api = open(os.path.join(ROOT, "norlab_icp_mapper_amd", "csrc", "api.hip")).read()
    py = open(os.path.join(ROOT, "norlab_icp_mapper_amd", "icp.py")).read()
    cpp = open(os.path.join(ROOT, "norlab_icp_mapper_amd", "host", "IcpSequence.cpp")).read()
    for phrase in ("the voxel matcher (icpmi_set_voxel_matcher > 0) ", "is defined on PlaneToPlaneErrorMinimizer only",
                   "is not served with the symmetric pair model (SymmetricPointToPlaneErrorMinimizer)",
                   "is not served with outlier filters (a pair is a point and the voxel it falls into: there is no match distance to filter on)"):
        assert phrase in api and phrase in py and phrase in cpp, phrase


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_set_voxel_matcher", "icpmi_get_voxel_matcher", "icpmi_get_voxel_map", "icpmi_voxel_lookup")


def test_header_and_library_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported, sym
        assert sym in bound, sym
    assert "0x9E3779B97F4A7C15" in header and "Koide" in header
    assert vr.HASH_MUL == 0x9E3779B97F4A7C15


def test_config_size_and_version_are_unchanged(tmp_path):
    from norlab_icp_mapper_amd import _capi
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include "icpmi.h"\nint main(void) { printf("%zu %d\\n", sizeof(icpmi_config), (int)ICPMI_VERSION); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.Config), 4]
    assert got[0] == 5 * 4 + 8 * 20 + 15 * 4 + 8 * 4


def test_loop_cfg_did_not_grow():
    """the voxel size and the table travel as arguments of the new kernel alone: common.h's LoopCfg has no voxel field"""
    text = open(os.path.join(ROOT, "norlab_icp_mapper_amd", "csrc", "common.h")).read()
    body = text[text.index("struct LoopCfg {"):]
    body = body[:body.index("};")]
    assert "vox" not in body.lower()
    assert json.dumps(sorted(vc.recorded())) == json.dumps(sorted(["rel_sums", "max_rel_step", "registration_room", "nearest_neighbour_plane_to_plane_room", "note"]))
