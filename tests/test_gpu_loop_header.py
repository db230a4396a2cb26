"""The loop header (common.h: LoopHdr) -- the words the per-iteration kernels read, fetched once per kernel as one dword per lane.

What can go wrong with it is not the workload's shape: a reading smaller than a wave, a reading of a batch other than the first, a `done`
raised by a kernel that is not the solve, a loop that stops early, the stamps of the NN launches, and the k > 1 kernels that still read the
moved fields by name.  Every case is a 4 000-point map and max_dist 2.0; results are compared bit for bit between the graph, the eager
(use_graph=0) and the profile handle, and against the CPU oracle within test_gpu_parity.py's pose tolerance."""
import numpy as np
import pytest

from test_gpu_parity import POSE_TOL_M, POSE_TOL_RAD

pytestmark = pytest.mark.gpu

TRIMMED = [(4, 0.85)]


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def scene(amd):
    return amd.synth.make_scene(m=4000, n=1000)


def handle(amd, sc, **kw):
    icp = amd.ICPSequence(max_dist=2.0, **kw)
    icp.setMap(sc["map"], sc["normals"])
    return icp


def outcome(icp, scan):
    """what a registration reports: the exception it raised (by name) or the pose bits, and the stats the header feeds"""
    try:
        T = np.asarray(icp(scan))
        err = None
    except Exception as e:  # the status, as the Python shell maps it
        T, err = np.zeros((4, 4), np.float32), type(e).__name__ + ": " + str(e)
    s = icp.stats
    return err, T.view(np.uint32).tolist(), s.iterations, s.pairs, np.float32(s.trimmed_limit).view(np.uint32).item(), \
        np.float32(s.weighted_point_used_ratio).view(np.uint32).item()


@pytest.mark.parametrize("minimizer", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_reading_sizes_agree_between_graph_eager_and_profile(amd, oracle, scene, n, minimizer):
    sc = scene
    kw = dict(minimizer=minimizer, outliers=TRIMMED, max_iterations=3, use_differential=0)
    scan = np.ascontiguousarray(sc["scan"][:n])
    got = {}
    for name, extra in (("graph", {}), ("eager", dict(use_graph=0)), ("profile", dict(profile=1))):
        icp = handle(amd, sc, **kw, **extra)
        got[name] = outcome(icp, scan)
        assert outcome(icp, scan) == got[name], (name, "second registration on the handle")
    assert got["graph"] == got["eager"], (n, minimizer)
    assert got["profile"] == got["eager"], (n, minimizer)
    if n >= 64:
        assert got["graph"][0] is None, got["graph"][0]
        o = oracle.OracleICP(oracle.make_config(nthreads=4, max_dist=2.0, **kw)); o.setMap(sc["map"], sc["normals"])
        err, T_ref = o(scan)
        assert err == 0
        T = np.array(got["graph"][1], dtype=np.uint32).view(np.float32).reshape(4, 4)
        dt, dr = amd.synth.pose_error(T, T_ref)
        print(f"n={n} minimizer={minimizer}: |dT| vs oracle {dt:.3e} m {dr:.3e} rad")
        assert got["graph"][2] == o.stats.iterations
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (n, minimizer, dt, dr)


def test_batch_equals_the_single_registrations(amd, scene):
    import torch
    sc = scene
    icp = handle(amd, sc, minimizer=2, outliers=TRIMMED, max_iterations=3, use_differential=0)
    # 65, 1 000 and 1 points (the issue's readings) and one of 40: fewer points than a wave in a slot that is not the first
    dev = [torch.from_numpy(np.ascontiguousarray(sc["scan"][a:a + n])).cuda() for a, n in ((0, 65), (0, 1000), (500, 1), (300, 40))]
    single = []
    for d in dev:
        try:
            T = icp.registerDev(d.data_ptr(), d.shape[0]); status = 0
        except amd.ConvergenceError:
            T, status = None, 1
        single.append((T, status, icp.stats.iterations, icp.stats.pairs, np.float32(icp.stats.trimmed_limit).view(np.uint32)))
    assert sum(st == 0 for _, st, _, _, _ in single) >= 3, [st for _, st, _, _, _ in single]   # at most the 1-point reading may fail to converge
    for rep in range(2):
        Ts, stats, status = icp.registerBatchDev([d.data_ptr() for d in dev], [d.shape[0] for d in dev])
        for b, (T, st, it, pairs, lim) in enumerate(single):
            assert (status[b] != 0) == (st != 0), (b, status[b])
            # a reading that fails reports the same iteration count, pairs and limit alone and in the batch; one that converges also the pose
            assert (stats[b].iterations, stats[b].pairs) == (it, pairs), (b, rep)
            assert np.float32(stats[b].trimmed_limit).view(np.uint32) == lim, (b, rep)
            if st == 0:
                assert np.array_equal(Ts[b].view(np.uint32), T.view(np.uint32)), (b, rep)


def test_done_raised_by_the_selection_kernel_and_the_next_reading(amd, scene):
    sc = scene
    kw = dict(minimizer=2, outliers=TRIMMED, max_iterations=3, use_differential=0)
    far = sc["scan"].copy(); far[:, :3] += np.float32(100.0)   # nothing within max_dist: the selection kernel raises `done`, not the solve
    icp = handle(amd, sc, **kw)
    ref = handle(amd, sc, use_graph=0, **kw)
    a, b = outcome(icp, far), outcome(ref, far)
    assert a[0] is not None and a == b
    fresh = handle(amd, sc, **kw)
    assert outcome(icp, sc["scan"]) == outcome(fresh, sc["scan"])   # the head re-initialises the header
    assert outcome(icp, sc["scan"])[0] is None


def test_early_stops_match_the_oracle_and_the_eager_loop(amd, oracle, scene):
    sc = scene
    # one iteration
    kw = dict(minimizer=2, outliers=TRIMMED, max_iterations=1, use_differential=0)
    icp, ref = handle(amd, sc, **kw), handle(amd, sc, use_graph=0, **kw)
    T, Tr = icp(sc["scan"]), ref(sc["scan"])
    o = oracle.OracleICP(oracle.make_config(nthreads=4, max_dist=2.0, **kw)); o.setMap(sc["map"], sc["normals"])
    o(sc["scan"])
    assert (icp.stats.iterations, icp.stats.stop_reason) == (o.stats.iterations, o.stats.stop_reason) == (1, o.stats.stop_reason)
    assert np.array_equal(T.view(np.uint32), Tr.view(np.uint32))
    # a Differential stop, scans of different difficulty in turn on one handle (the head graph follows the previous count)
    kw = dict(minimizer=2, outliers=TRIMMED, max_iterations=40, use_differential=1)
    scans = [sc["scan"]]
    for shift, yaw in ((0.02, 0.0), (0.6, 0.0), (0.0, 0.08)):
        cy, sy = np.float32(np.cos(yaw)), np.float32(np.sin(yaw))
        s2 = sc["scan"].copy()
        s2[:, 0], s2[:, 1] = cy * s2[:, 0] - sy * s2[:, 1] + np.float32(shift), sy * sc["scan"][:, 0] + cy * s2[:, 1] - np.float32(shift / 2)
        scans.append(s2)
    icp, ref = handle(amd, sc, **kw), handle(amd, sc, use_graph=0, **kw)
    o = oracle.OracleICP(oracle.make_config(nthreads=4, max_dist=2.0, **kw)); o.setMap(sc["map"], sc["normals"])
    for s in scans + scans[::-1]:
        T, Tr = icp(s), ref(s)
        o(s)
        assert (icp.stats.iterations, icp.stats.stop_reason) == (o.stats.iterations, o.stats.stop_reason)
        assert np.array_equal(T.view(np.uint32), Tr.view(np.uint32))


def test_nn_stamps_count_every_launch_once(amd, scene):
    import torch
    sc = scene
    icp = handle(amd, sc, minimizer=2, outliers=TRIMMED, max_iterations=5, use_differential=0)
    icp(sc["scan"])
    assert icp.stats.iterations == 5
    assert icp.stats.nn_launches == icp.stats.iterations and icp.stats.nn_ms_avg > 0
    # a batch and a residual pass open and close intervals of their own on the handle's states (icpmi_stats of a batch carries no stamps):
    # the registration behind each of them still counts exactly its own launches
    dev = [torch.from_numpy(np.ascontiguousarray(sc["scan"][:n])).cuda() for n in (1000, 300)]
    _, stats, status = icp.registerBatchDev([d.data_ptr() for d in dev], [d.shape[0] for d in dev])
    assert status == [0, 0] and [s.iterations for s in stats] == [5, 5]
    icp(sc["scan"])
    assert icp.stats.nn_launches == icp.stats.iterations == 5 and icp.stats.nn_ms_avg > 0
    icp.residual(sc["scan"])
    icp(sc["scan"])
    assert icp.stats.nn_launches == icp.stats.iterations == 5 and icp.stats.nn_ms_avg > 0


def test_knn3_trimmed_graph_equals_eager(amd, scene):
    sc = scene
    kw = dict(minimizer=2, knn=3, outliers=TRIMMED, max_iterations=4, use_differential=0)
    a, b = handle(amd, sc, **kw), handle(amd, sc, use_graph=0, **kw)
    for rep in range(2):
        assert outcome(a, sc["scan"]) == outcome(b, sc["scan"])
    assert outcome(a, sc["scan"])[0] is None
