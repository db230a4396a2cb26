"""NormalSpaceDataPointsFilter without a GPU: the closed form of the numpy restatement (tests/normal_space_reference.py) against a
literal simulation of upstream's round-robin, the buckets of a few normals worked out by hand, the generator of the GPU tests' normals,
the new symbol of the C ABI, and the YAML surface of the C++ host shell."""
import os
import re
import subprocess

import numpy as np
import pytest

import normal_space_reference as nsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _c4(xyz):
    xyz = np.asarray(xyz, F)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


# ---- the selection ----
def _both(buckets, nb, seed=1):
    buckets = np.asarray(buckets)
    r = nsr.minstd(seed, buckets.shape[0])
    a, b = nsr.closed_form(buckets, r, nb), nsr.round_robin(buckets, r, nb)
    assert a.tolist() == b.tolist(), (buckets.tolist(), nb)
    assert a.shape == (nb,) and (np.diff(a) > 0).all()
    return a


def test_minstd_is_the_standard_generator():
    assert nsr.minstd(1, 10_000)[-1] == 399268537                            # [rand.predef]
    r = nsr.minstd(1, 5000)
    assert len(set(r.tolist())) == 5000 and r.min() >= 1 and r.max() <= nsr.MINSTD_M - 1


@pytest.mark.parametrize("n", [2, 3, 7, 40])
def test_closed_form_equals_the_round_robin_on_the_edge_shapes(n):
    shapes = {"one bucket": np.zeros(n, int), "every point its own bucket": np.arange(n)[::-1] * 3,
              "populations 1 and n - 1": np.r_[np.full(n - 1, 5), 2], "1 and n - 1, the single one last": np.r_[np.full(n - 1, 5), 9]}
    for name, b in shapes.items():
        for nb in sorted({1, n // 2, n - 1} - {0}):
            _both(b, nb)


def test_one_bucket_is_the_nb_smallest_random_numbers():
    n, nb = 50, 17
    got = _both(np.full(n, 4), nb)
    assert got.tolist() == sorted(np.argsort(nsr.minstd(1, n))[:nb].tolist())


def test_own_buckets_keep_the_first_nb_buckets():
    b = np.array([9, 3, 7, 1, 5, 8])
    assert _both(b, 3).tolist() == [1, 3, 4]                                 # buckets 1, 3, 5: R* = 0, rem = 3


def test_rem_zero_and_rem_positive():
    b = np.repeat([2, 11, 30, 31], 50)                                       # four buckets of 50
    r = nsr.minstd(1, 200)
    got = _both(b, 120)                                                      # S(30) = 120 exactly: R* = 30, rem = 0
    for k in range(4):
        mine = np.arange(50 * k, 50 * k + 50)
        assert sorted(got[(got >= 50 * k) & (got < 50 * k + 50)].tolist()) == sorted(mine[np.argsort(r[mine])[:30]].tolist())
    got = _both(b, 122)                                                      # rem = 2: buckets 2 and 11 give 31, the others 30
    assert [int(((got >= 50 * k) & (got < 50 * k + 50)).sum()) for k in range(4)] == [31, 31, 30, 30]
    got = _both(np.r_[b, [40] * 3], 122)                                     # a bucket of 3 is exhausted: (122 - 3) = 119 = 29 * 4 + 3
    assert [int(((got >= 50 * k) & (got < 50 * k + 50)).sum()) for k in range(4)] + [int((got >= 200).sum())] == [30, 30, 30, 29, 3]


def test_random_populations():
    rng = np.random.default_rng(5)
    for _ in range(30):
        n = int(rng.integers(2, 120))
        b = rng.integers(0, int(rng.integers(1, 12)), n)
        for nb in {1, n // 3 or 1, n - 1}:
            _both(b, int(nb), seed=int(rng.integers(0, 1000)))


def test_seeds_0_1_and_the_modulus_are_the_same_state():
    rng = np.random.default_rng(6)
    nrm = nsr.safe_normals(rng, 500)
    xyz = _c4(rng.normal(size=(500, 3)))
    ref = nsr.normal_space_sampling(xyz, nrm, 100, seed=1)[0]
    for seed in (0, 2147483647):
        assert np.array_equal(nsr.normal_space_sampling(xyz, nrm, 100, seed=seed)[0], ref)
    assert not np.array_equal(nsr.normal_space_sampling(xyz, nrm, 100, seed=2)[0], ref)


def test_identity_when_nb_sample_covers_the_cloud_even_without_normals():
    xyz = _c4(np.zeros((50, 3)))
    for nb in (50, 51, 10_000):
        order, b = nsr.normal_space_sampling(xyz, None, nb)
        assert order.tolist() == list(range(50)) and b is None
    with pytest.raises(KeyError):
        nsr.normal_space_sampling(xyz, None, 49)


# ---- the buckets ----
def test_buckets_by_hand():
    eps = 0.09817
    assert nsr.stride_of(eps) == 64 and nsr.stride_of(0.04908) == 128 and nsr.stride_of(3.14159) == 2
    nrm = np.array([[0, 0, 1],             # north pole: theta 0, phi atan2(0, 0) = 0
                    [0, 0, -1],            # south pole: theta (float)pi -> floor(32.0015) = 32
                    [0, 0, 0],             # the zero normal: theta pi / 2 -> floor(16.0007) = 16, phi 0
                    [-1, -0.0, 0],         # atan2(-0, -1) = -pi -> + 2 pi = pi -> floor(32.0015) = 32
                    [-1, 0.0, 0],          # atan2(+0, -1) = +pi: the same bucket
                    [1, -1e-9, 0],         # phi = 2 pi - 1e-9 -> (float)(2 pi) -> floor(64.003) = 64 = stride: aliased into the next row
                    [0, 1, 0], [0, -1, 0], [0, 0, 2.5]], F)
    want = [0, 32 * 64, 16 * 64, 16 * 64 + 32, 16 * 64 + 32, 16 * 64 + 64, 16 * 64 + 16, 16 * 64 + 48, 0]
    assert nsr.buckets_of(nrm, eps).tolist() == want
    for e in nsr.EPSILONS:
        assert nsr.buckets_of(nrm, e).max() < nsr.table_size(e) < (1 << 14)
    assert nsr.table_size(0.04908) == 65 * 128 + 1 and nsr.table_size(eps) == 33 * 64 + 1 and nsr.table_size(3.14159) == 5


def test_the_largest_bucket_fits_the_table():
    # theta and phi at their largest: nz = -1 with ny just below zero
    nrm = np.array([[1e-30, -1e-38, -1], [1, -1e-30, -1], [-1, -1e-30, -1]], F)
    for e in nsr.EPSILONS + (0.05, 0.1, 0.7, 1.0, 2.0):
        assert nsr.buckets_of(nrm, e).max() <= nsr.table_size(e) - 1


def test_edge_margin():
    eps = np.float64(F(0.09817))
    on_edge = np.array([[np.sin(3 * eps), 0, np.cos(3 * eps)]], F)           # theta = 3 epsilon up to float32 rounding
    assert nsr.edge_margin(on_edge, 0.09817)[0] < 1e-5
    mid = np.array([[np.sin(3.5 * eps) * np.cos(2.5 * eps), np.sin(3.5 * eps) * np.sin(2.5 * eps), np.cos(3.5 * eps)]], F)
    assert nsr.edge_margin(mid, 0.09817)[0] > 0.49
    assert nsr.buckets_of(mid, 0.09817)[0] == 3 * 64 + 2


def test_the_generator_keeps_clear_of_the_bucket_edges():
    nrm = nsr.safe_normals(np.random.default_rng(7), 20_000)
    assert nrm.dtype == F and nrm.shape == (20_000, 3)
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6
    for e in nsr.EPSILONS:
        assert nsr.edge_margin(nrm, e).min() >= 1e-3
    assert np.unique(nsr.buckets_of(nrm, 0.09817)).size > 1500               # and still covers the sphere


# ---- the C ABI ----
def test_header_library_and_ctypes_table_agree_on_the_new_symbol():
    from norlab_icp_mapper_amd import _capi
    sym = "icpmi_normal_space_sampling"
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    m = re.search(r"icpmi_status\s+%s\s*\(([^;]*)\);" % sym, header)
    assert m and sym in exported
    rows = [r for r in _capi.SYMBOLS if r[0] == sym]
    assert len(rows) == 1
    assert len(rows[0][2]) == len(m.group(1).split(",")) == 10               # h, in4, n, normals3, nb_sample, seed, epsilon, order_out, n_out, bucket_out


# ---- the host shell (norlab_icp_mapper_amd/host): parameters and the paths that need no GPU context ----
@pytest.fixture(scope="module")
def host():
    import host_bindings as hb
    from test_host_cpp import _build_host
    _build_host()
    return hb


NSF = "NormalSpaceDataPointsFilter"


def test_host_accepts_the_filter_and_its_parameters(host):
    cloud = _c4(np.random.default_rng(8).normal(size=(5000, 3)))
    for y in ("[%s]" % NSF, "[{%s: {nbSample: 5000, seed: 0, epsilon: 0.04908}}]" % NSF,
              "[{%s: {nbSample: 6000, seed: 2147483647, epsilon: 3.14159}}]" % NSF):
        out, nrm, _ = host.filter_chain(y, cloud)                            # nbSample (default 5000) >= N: unchanged, no normals, no GPU
        assert np.array_equal(out, cloud) and nrm is None


@pytest.mark.parametrize("params,msg", [
    ("{nbSamples: 10}", "unknown parameter nbSamples"),
    ("{torqueNorm: 1}", "unknown parameter torqueNorm"),
    ("{nbSample: 0}", "nbSample must be >= 1"),
    ("{nbSample: -3}", "nbSample must be >= 1"),
    ("{seed: -1}", "seed must be in"),
    ("{seed: 2147483648}", "seed must be in"),
    ("{epsilon: 0.049}", "epsilon must be in"),
    ("{epsilon: 3.1416}", "epsilon must be in"),
    ("{epsilon: nan}", "epsilon must be in"),
])
def test_host_rejects_bad_parameters(host, params, msg):
    with pytest.raises(RuntimeError, match=msg):
        host.filter_chain("[{%s: %s}]" % (NSF, params), np.zeros((0, 4), F))


def test_host_default_sample_needs_normals_and_then_a_gpu_context(host):
    rng = np.random.default_rng(9)
    cloud = _c4(rng.normal(size=(5001, 3)))                                  # one more than the default nbSample
    with pytest.raises(RuntimeError, match="normals"):
        host.filter_chain("[%s]" % NSF, cloud)                               # InvalidField: no GPU context needed to say so
    with pytest.raises(RuntimeError, match="normals"):
        host.filter_chain("[{%s: {nbSample: 10}}]" % NSF, cloud[:11])
    with pytest.raises(RuntimeError, match="needs a GPU context"):
        host.filter_chain("[%s]" % NSF, cloud, desc_name="normals", desc=nsr.safe_normals(rng, 5001))
