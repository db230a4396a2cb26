"""KDTreeVarDistMatcher without a GPU: the YAML surface of icp.py and of the C++ host shell, the two new symbols of the C ABI, the layout of
icpmi_config::var_dist, and the inputs of the GPU tests (tests/var_dist_reference.py): the radii row built from every query's own exact
neighbour distances keeps clear of those distances, so that no comparison of test_gpu_var_dist.py hinges on the tie rule."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import var_dist_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ icp.py
def test_python_yaml_accepts_var_dist_matcher():
    from norlab_icp_mapper_amd import icp
    cfg = icp.config_from_yaml_chain({"matcher": {"KDTreeVarDistMatcher": {"knn": 6, "epsilon": 0, "searchType": 1, "maxDistField": "simpleSensorNoise"}}})
    assert cfg.var_dist == 1 and cfg.knn == 6 and cfg.max_dist_field == "simpleSensorNoise"
    cfg = icp.config_from_yaml_chain({"matcher": {"KDTreeVarDistMatcher": {}}})
    assert cfg.var_dist == 1 and cfg.knn == 1 and cfg.max_dist_field == "maxSearchDist"
    cfg = icp.config_from_yaml_chain({"matcher": "KDTreeVarDistMatcher"})
    assert cfg.var_dist == 1 and cfg.max_dist_field == "maxSearchDist"
    with pytest.raises(icp.InvalidParameter, match="KDTreeVarDistMatcher: unknown parameter maxDist"):
        icp.config_from_yaml_chain({"matcher": {"KDTreeVarDistMatcher": {"maxDist": 2.0}}})
    with pytest.raises(icp.InvalidParameter, match="unknown parameter bogus"):
        icp.config_from_yaml_chain({"matcher": {"KDTreeVarDistMatcher": {"bogus": 1}}})
    with pytest.raises(icp.InvalidParameter, match="unknown matcher NullMatcher"):
        icp.config_from_yaml_chain({"matcher": {"NullMatcher": {}}})


def test_python_yaml_leaves_kdtree_matcher_alone():
    from norlab_icp_mapper_amd import icp
    cfg = icp.config_from_yaml_chain({"matcher": {"KDTreeMatcher": {"knn": 3, "maxDist": 2.0, "maxDistField": "maxSearchDist"}}})
    assert cfg.var_dist == 0 and cfg.knn == 3 and cfg.max_dist == 2.0 and not hasattr(cfg, "max_dist_field")
    assert icp.config_from_yaml_chain({}).var_dist == 0


# ------------------------------------------------------------------------------------------------------------------ the C++ shell
def parse_matcher(yaml_matcher):
    """nim_test_parse_matcher (host/TestHooks.cpp): dict of what parseMatcher set, or RuntimeError with the exception's text"""
    import host_bindings as hb
    fn = hb.load().nim_test_parse_matcher
    fn.restype = C.c_int
    knn, var = C.c_int(0), C.c_int(0)
    eps, md = C.c_float(0), C.c_float(0)
    field = C.create_string_buffer(128); err = C.create_string_buffer(512)
    if fn(yaml_matcher.encode(), C.byref(knn), C.byref(eps), C.byref(md), C.byref(var), field, C.c_int(128), err, C.c_int(512)):
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(knn=knn.value, epsilon=eps.value, max_dist=md.value, var_dist=var.value, field=field.value.decode())


def test_cpp_yaml_accepts_var_dist_matcher():
    got = parse_matcher("KDTreeVarDistMatcher:\n  knn: 6\n  epsilon: 0\n  searchType: 1\n  maxDistField: simpleSensorNoise\n")
    assert got["var_dist"] == 1 and got["knn"] == 6 and got["field"] == "simpleSensorNoise"
    got = parse_matcher("KDTreeVarDistMatcher:\n  knn: 1\n")
    assert got["var_dist"] == 1 and got["knn"] == 1 and got["field"] == "maxSearchDist"
    with pytest.raises(RuntimeError, match="KDTreeVarDistMatcher: unknown parameter maxDist"):
        parse_matcher("KDTreeVarDistMatcher:\n  maxDist: 2.0\n")
    with pytest.raises(RuntimeError, match="unknown parameter bogus"):
        parse_matcher("KDTreeVarDistMatcher:\n  bogus: 1\n")
    with pytest.raises(RuntimeError, match="unknown matcher NullMatcher"):
        parse_matcher("NullMatcher:\n  knn: 1\n")


def test_cpp_yaml_leaves_kdtree_matcher_alone():
    got = parse_matcher("KDTreeMatcher:\n  knn: 3\n  maxDist: 2.0\n  maxDistField: maxSearchDist\n")
    assert got == dict(knn=3, epsilon=0.0, max_dist=2.0, var_dist=0, field="")
    assert math.isinf(parse_matcher("KDTreeMatcher:\n  knn: 1\n")["max_dist"])


# ------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("icpmi_set_reading_max_dist", "icpmi_knn_var")


def test_header_and_library_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert re.search(r"icpmi_status\s+%s\s*\(" % sym, header), sym
        assert sym in exported, sym
        assert sym in bound, sym


def test_var_dist_is_the_first_reserved_word(tmp_path):
    """a caller compiled before the field existed zeroes it with the tail: same size, same offsets, default 0"""
    from norlab_icp_mapper_amd import _capi
    assert _capi.Config.var_dist.offset == _capi.Config.reserved.offset == C.sizeof(_capi.Config) - 8
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "icpmi.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(icpmi_config), '
                   'offsetof(icpmi_config, var_dist), offsetof(icpmi_config, reserved)); return 0; }\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.Config), _capi.Config.var_dist.offset, _capi.Config.reserved.offset]
    cfg = _capi.Config()
    _capi.load().icpmi_config_default(C.byref(cfg))
    assert cfg.var_dist == 0 and list(cfg.reserved) == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_radii_row_keeps_clear_of_the_neighbour_distances(oracle):
    sc = vr.scene()
    assert sc["map"].shape == (vr.M, 4) and sc["scan"].shape == (vr.N, 4)
    o = oracle.OracleICP(oracle.make_config()); o.setMap(sc["map"])
    mean = o.getMapMean()
    mapc, q = vr.centred(sc["map"], mean), vr.centred(sc["scan"], mean)
    ids, d2 = vr.exact_rows(oracle, mapc, q)
    assert np.isfinite(d2).all() and (ids >= 0).all()
    r, kind = vr.radii_row(d2)
    assert vr.clear_of(r, d2).all()
    assert not np.isnan(r).any() and (r >= 0).all()
    for kd in range(5):   # the five kinds are all there (a query moved to +inf by the condition is the rare exception)
        assert (kind == kd).sum() >= vr.N // 5 - 10, (vr.KINDS[kd], int((kind == kd).sum()))
    for k in vr.KS:
        mids, md2 = vr.masked(ids, d2, r, k)
        assert np.array_equal((mids >= 0).sum(1), vr.expected_filled(kind, k)), k
        assert np.array_equal(mids >= 0, np.isfinite(md2))
    # a constant row masks exactly as the oracle's own radius search does
    for rc in (0.05, 0.5, math.inf):
        for k in (1, 6):
            mids, md2 = vr.masked(ids, d2, np.full(vr.N, rc, np.float32), k)
            rids, rd2 = oracle.knn(mapc, q, k=k, max_dist=rc, nthreads=16)
            assert np.array_equal(mids, rids) and np.array_equal(md2, rd2), (rc, k)
