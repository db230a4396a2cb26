"""The oracle's single step over a case of tests/solver_cases.py (pairs i -> i asserted with its kd-tree), shaped like the device's
icpmi_minimize_step output so that solver_reference.check_step takes either.  `oracle` is the oracle_bindings module."""
import numpy as np

import solver_reference as sr


def oracle_flag(kw):
    return 4 if kw.get("is_2d") else (2 if kw.get("force_2d") else (1 if kw.get("force_4dof") else 0))


def check_pairing(oracle, case, mc, rc):
    ids, d2 = oracle.knn(mc, rc, k=1)
    n = rc.shape[0]
    if case["pairing"] == "distance":       # every map point ties
        want = ((rc[:, :3].astype(np.float64) - mc[0, :3]) ** 2).sum(1)
        np.testing.assert_allclose(d2[:, 0], want, rtol=1e-6)
    else:
        assert np.array_equal(ids[:, 0], np.arange(n)), case["name"]
        disp = np.sqrt(d2[:, 0].astype(np.float64)).max()
        if case["pairing"] == "identity":
            assert case["spacing"] >= 4.0 * disp, (case["name"], case["spacing"], disp)
        else:                                # the octahedra: less than half the neighbour distance
            assert disp < 0.5 * case["spacing"], (case["name"], case["spacing"], disp)
    if case["exact_mean"]:
        mean = sr.centre(case["map4"], case["reading4"])[2]
        assert np.all(mean == np.round(mean * 1024) / 1024) and np.array_equal(mc[:, :3].astype(np.float64), case["map4"][:, :3].astype(np.float64) - mean), (case["name"], mean)
    return np.arange(n, dtype=np.int32).reshape(-1, 1), d2


def oracle_step(oracle, case):
    """(T, sums, mc, rc): the oracle's minimiser over the pairs i -> i; its A, b (doubles) packed like the device's sums"""
    mc, rc, _ = sr.centre(case["map4"], case["reading4"])
    ids, d2 = check_pairing(oracle, case, mc, rc)
    kw = case["kw"]
    w = np.ones_like(d2)
    err, T, A, b, x, st = oracle.minimize(kw["minimizer"], rc, mc, case["normals"], ids, np.where(np.isfinite(d2), d2, 0).astype(np.float32), w,
                                          force_4dof=oracle_flag(kw))
    assert err == 0 and st.pairs == case["pairs"], (case["name"], err, st.pairs)
    sums = sr.pair_sums(rc, mc, case["normals"], kw["minimizer"], bool(kw.get("force_2d")))
    if kw["minimizer"] == 2:
        sums[:21] = A[sr.IU]; sums[21:27] = b
    else:
        # point to point: `sums` stay the reference's own float64 sums -- assertion 1 of check_step says nothing about the oracle here.
        # The oracle hands out its float32 H only: the one the reference forms from the float64 sums must be that matrix to an ulp
        H32 = sr.h_from_sums(sums)[1]
        Ho = A.T.ravel()[:9].reshape(3, 3).T.astype(np.float32)
        np.testing.assert_allclose(Ho, H32, rtol=0, atol=2 * sr.EPS_F * max(np.abs(sums[7:16]).max(), 1e-30), err_msg=case["name"])
    return T, sums, mc, rc, x
