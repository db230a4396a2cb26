"""MaxDensityDataPointsFilter without a GPU: the numpy restatement (tests/max_density_reference.py) held to the code that defines the
behaviour -- the host filter's serial std::minstd_rand loop, through the host shell's filter-chain seam --, its edge cases, and the new
symbols of the C ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import max_density_reference as mdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MDF = "MaxDensityDataPointsFilter"


@pytest.fixture(scope="module")
def host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb


def _cloud(n):
    c = np.ones((n, 4), F)
    c[:, 0] = np.arange(n)                                   # the index, exactly: the kept SET can be read off the output
    c[:, 1:3] = np.random.default_rng(2).normal(size=(n, 2))
    return c


def _host_kept(host, dens, params):
    cloud = _cloud(dens.shape[0])
    out, _, dout = host.filter_chain("[{%s: %s}]" % (MDF, params), cloud, desc_name="densities", desc=dens)
    kept = out[:, 0].astype(np.int64)
    assert np.array_equal(out, cloud[kept]) and np.array_equal(dout.view(np.uint32), dens[kept].view(np.uint32))
    return kept


def test_reference_equals_the_host_filter_on_5000_points(host):
    rng = np.random.default_rng(3)
    dens = mdr.log_uniform_densities(rng, 5000)
    dens[[7, 4100]] = np.nan
    dens[[19, 2500]] = np.inf
    dens[[33, 34, 4999]] = 10.0                              # equal to maxDensity: not dense
    for params, md, seed in (("{maxDensity: 10}", 10.0, 1), ("{maxDensity: 10, seed: 77}", 10.0, 77), ("{maxDensity: 2.5, seed: 0}", 2.5, 0),
                             ("{maxDensity: 150, seed: -5}", 150.0, -5), ("{maxDensity: 10, seed: 2147483647}", 10.0, 2147483647)):
        keep = mdr.max_density_keep(dens, md, seed)
        assert 0.05 < 1.0 - keep.mean() < 0.95               # the draw decides something
        assert np.array_equal(_host_kept(host, dens, params), np.nonzero(keep)[0]), params


def test_minstd_is_the_standard_generator():
    assert mdr.minstd_stream(1, 10_000)[-1] == 399268537     # [rand.predef]
    assert np.array_equal(mdr.minstd_stream(0, 50), mdr.minstd_stream(1, 50))
    assert np.array_equal(mdr.minstd_stream(2147483647, 50), mdr.minstd_stream(1, 50))
    assert np.array_equal(mdr.minstd_stream(-5, 50), mdr.minstd_stream((1 << 32) - 5, 50))
    assert not np.array_equal(mdr.minstd_stream(2, 50), mdr.minstd_stream(1, 50))


def test_reference_edge_cases():
    n = 1000
    assert mdr.max_density_keep(np.full(n, 5.0, F), 10.0).all()                     # none dense
    assert mdr.max_density_keep(np.full(n, 10.0, F), 10.0).all()                    # equal: not dense
    assert mdr.max_density_keep(np.full(n, np.nan, F), 10.0).all()                  # NaN: not dense
    assert not mdr.max_density_keep(np.full(n, np.inf, F), 10.0).any()              # u < 0 is false
    k = mdr.max_density_keep(np.full(n, 40.0, F), 10.0)                             # all dense: every point draws, a quarter survives
    u = mdr.minstd_stream(1, n).astype(F) / F(2147483645.0)
    assert np.array_equal(k, u < F(0.25)) and 0.15 < k.mean() < 0.35
    # only the dense points draw: a point that is not dense does not shift the stream
    d = np.full(n, 40.0, F); d[::2] = 1.0
    k2 = mdr.max_density_keep(d, 10.0)
    assert k2[::2].all() and np.array_equal(k2[1::2], (u < F(0.25))[:n // 2])


def test_header_library_and_ctypes_table_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    for sym, nargs in (("icpmi_max_density_keep", 6), ("icpmi_get_map_densities", 3)):
        m = re.search(r"icpmi_status\s+%s\s*\(([^;]*)\);" % sym, header)
        assert m and sym in exported, sym
        rows = [r for r in _capi.SYMBOLS if r[0] == sym]
        assert len(rows) == 1 and len(rows[0][2]) == len(m.group(1).split(",")) == nargs
    assert _capi.MOP_MAX_DENSITY == 6 and re.search(r"ICPMI_MOP_MAX_DENSITY\s*=\s*6\b", header)


def test_host_filter_still_needs_the_descriptor(host):
    with pytest.raises(RuntimeError, match="no densities found"):
        host.filter_chain("[%s]" % MDF, _cloud(10))
