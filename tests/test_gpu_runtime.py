"""The runtime around the kernels: loops that leave their graphs when the map changes behind every scan and come
back to them, the process-wide stream pool and device block cache under handle churn and two threads, the library with both switched
off, the self-search grid that follows what the points see.  None of it may change a bit of any result: every check is bitwise
against a handle that runs eagerly, against the same computation done first, or against the oracle.

Reference: the registrations stand behind Mapper::processInput (Mapper.cpp:213), the rebuild behind Map::updateLocalPointCloud ->
icp.setMap (Map.cpp:528), the normals behind the post filters (Map.cpp:523-525)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import norlab_icp_mapper_amd as pkg
    return pkg


def _bits(T):
    return np.asarray(T, dtype=np.float32).view(np.uint32).copy()


@pytest.mark.parametrize("checked", [1, 0])
def test_mapper_mode_leaves_its_graphs_and_comes_back_with_the_same_bits(amd, small_scene, checked):
    """A mapper replaces its map behind every scan: after two graph sets that served one registration each the handle runs its loops
    eagerly, and returns to graphs when a map is registered against twice.  Checked loops (Counter + Differential:
    segment graphs) and the Counter-only chain of the shipped configuration (one graph): every pose equals, bit for bit, the pose of a
    handle that never used a graph."""
    sc = small_scene
    kw = dict(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=40 if checked else 10, use_differential=checked)
    icp = amd.ICPSequence(**kw)
    ref = amd.ICPSequence(use_graph=0, **kw)
    rng = np.random.default_rng(11)
    m = sc["map"].shape[0]
    its = []
    for j in range(7):                      # seven different maps, one registration each: graphs are dropped every time
        keep = np.sort(rng.permutation(m)[: m - 500 * (j + 1)])
        for h in (icp, ref):
            h.setMap(sc["map"][keep], sc["normals"][keep])
        T, Tr = icp(sc["scan"]), ref(sc["scan"])
        assert icp.stats.iterations == ref.stats.iterations and icp.stats.stop_reason == ref.stats.stop_reason
        assert np.array_equal(_bits(T), _bits(Tr)), j
        its.append(icp.stats.iterations)
    first = None
    for rep in range(5):                    # ... then localisation against the last map: the same signature comes back, graphs pay again
        T, Tr = icp(sc["scan"]), ref(sc["scan"])
        assert np.array_equal(_bits(T), _bits(Tr)), rep
        first = _bits(T) if first is None else first
        assert np.array_equal(_bits(T), first)
    scan2 = sc["scan"][::2].copy()          # another reading size in between
    assert np.array_equal(_bits(icp(scan2)), _bits(ref(scan2)))
    assert np.array_equal(_bits(icp(sc["scan"])), first)
    assert min(its) >= 2


def test_handle_churn_through_the_block_cache_and_the_stream_pool(amd, small_scene):
    """Handles created and destroyed in turn, with maps of different sizes: released streams and device blocks are handed to the next
    handle (common.h: stream_acquire / dev_malloc).  A block that is larger than asked for, or that held another handle's map, must not
    show: every registration equals the first one made with that map size."""
    sc = small_scene
    kw = dict(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=8, use_differential=0)
    sizes = [60000, 20000, 45000, 60000, 9000, 45000, 20000, 60000, 9000, 30000, 45000, 60000]
    seen = {}
    for k, msz in enumerate(sizes):
        icp = amd.ICPSequence(**kw)
        icp.setMap(sc["map"][:msz], sc["normals"][:msz])
        T = _bits(icp(sc["scan"]))
        nrm = icp.surfaceNormals(sc["map"][: msz // 3], knn=7)
        if msz in seen:
            assert np.array_equal(T, seen[msz][0]), (k, msz)
            assert np.array_equal(nrm.view(np.uint32), seen[msz][1].view(np.uint32)), (k, msz)
        else:
            seen[msz] = (T, nrm.copy())
        if k % 3 != 2:
            icp.close()                     # (every third handle is left to the garbage collector)
    many = [amd.ICPSequence(**kw) for _ in range(20)]   # more streams than the pool keeps
    for h in many:
        h.close()
    icp = amd.ICPSequence(**kw)
    icp.setMap(sc["map"][:45000], sc["normals"][:45000])
    assert np.array_equal(_bits(icp(sc["scan"])), seen[45000][0])


def test_two_threads_two_handles(amd, small_scene):
    """One handle per thread (the contract of include/icpmi.h), both allocating and releasing through the shared cache and pool while
    the other registers and CAPTURES its loop graphs: same bits as the serial runs.  (On this runtime a hipDeviceSynchronize or a
    synchronous legacy-stream copy in one thread invalidates a thread-local stream capture in another -- scripts/r5/capture_threads.hip;
    the first version of this test caught dev_free doing exactly that: common.h capture_gate.)"""
    sc = small_scene
    kw = dict(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=40, use_differential=1)
    maps = [(sc["map"][:50000], sc["normals"][:50000]), (sc["map"][10000:], sc["normals"][10000:])]
    serial = []
    for mp, nr in maps:
        icp = amd.ICPSequence(**kw); icp.setMap(mp, nr); serial.append(_bits(icp(sc["scan"]))); icp.close()
    out = [[], []]
    errs = []

    def work(t):
        try:
            for rep in range(6):
                icp = amd.ICPSequence(**kw)
                icp.setMap(*maps[t])
                out[t].append(_bits(icp(sc["scan"])))
                out[t].append(_bits(icp(sc["scan"])))
                icp.close()
        except Exception as e:  # noqa: BLE001 -- reported below, in the main thread
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for t in (0, 1):
        assert len(out[t]) == 12
        for T in out[t]:
            assert np.array_equal(T, serial[t])


def test_a_thread_that_churns_handles_next_to_one_that_recaptures_its_graphs(amd, small_scene):
    """The mapper's two threads (Mapper.cpp:274-288: registration goes on while the map update runs): thread 0 replaces its map before
    every other registration, so its segment graphs are captured again and again; thread 1 creates handles, builds maps, computes normals
    and destroys them -- allocations, frees (device-wide synchronisations), fresh streams.  No capture may break, every pose of thread 0
    equals the serial pose for its map."""
    sc = small_scene
    kw = dict(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=40, use_differential=1)
    m = sc["map"].shape[0]
    keeps = [np.arange(m - 700 * j) for j in range(4)]
    serial = []
    for keep in keeps:
        icp = amd.ICPSequence(**kw); icp.setMap(sc["map"][keep], sc["normals"][keep]); serial.append(_bits(icp(sc["scan"]))); icp.close()
    errs, got = [], []
    done = threading.Event()

    def registrar():
        try:
            icp = amd.ICPSequence(**kw)
            for rep in range(40):
                j = rep % 4
                if rep % 2 == 0:
                    icp.setMap(sc["map"][keeps[j]], sc["normals"][keeps[j]])
                    cur = j
                got.append((cur, _bits(icp(sc["scan"]))))
            icp.close()
        except Exception as e:  # noqa: BLE001
            errs.append("registrar: " + repr(e))
        finally:
            done.set()

    def churner():
        try:
            k = 0
            while not done.is_set() and k < 400:
                h = amd.ICPSequence(**kw)
                sz = 8000 + 3000 * (k % 7)
                h.setMap(sc["map"][:sz], sc["normals"][:sz])
                h.surfaceNormals(sc["map"][:sz], knn=6)
                h.close()
                k += 1
        except Exception as e:  # noqa: BLE001
            errs.append("churner: " + repr(e))

    th = [threading.Thread(target=registrar), threading.Thread(target=churner)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert len(got) == 40
    for j, T in got:
        assert np.array_equal(T, serial[j])


_CHILD = r"""
import sys, hashlib
import numpy as np
sys.path.insert(0, %r)
import norlab_icp_mapper_amd as pkg
sc = pkg.synth.make_scene(m=60000, n=6000)
h = hashlib.sha256()
icp = pkg.ICPSequence(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=40, use_differential=1)
icp.setMap(sc["map"][::2], sc["normals"][::2])
icp.setMapScalar(np.full(sc["map"][::2].shape[0], 0.6, np.float32))
prior = np.eye(4, dtype=np.float32)
for k in range(4):
    scan = pkg.synth.make_scene(m=8, n=6000, seed_scan=900 + k)["scan"]
    corr = icp.registerWithPrior(scan, prior)
    pose = (corr @ prior).astype(np.float32)
    src, m = icp.mapUpdateChain(None, [("dynamic_points", 0.9, 0.8, 0.99, 0.01, 0.01, 0.01, 200.0), ("octree", 0.15, 1, 1)],
                                [("surface_normals", 10), ("cut_scalar", 0.65, 1)], scan_scalar=np.full(6000, 0.6, np.float32),
                                to_sensor=np.linalg.inv(pose), from_sensor=pose, staged_correction=corr)
    h.update(np.asarray(corr, np.float32).tobytes()); h.update(src.tobytes()); h.update(icp.getMapScalar().tobytes())
print("DIGEST", h.hexdigest(), m)
"""


def test_switches_off_same_bits():
    """The same four scans through registration + the shipped map-update chain in two fresh processes: defaults, and without the device
    block cache (ICPMI_ALLOC_CACHE_MB=0: every array a fresh hipMalloc, nothing handed from one use to the next).  One digest over every
    correction, every provenance vector and the surviving probabilities.  (Through r5 this test also switched graph adaptation, chain overlap,
    octree speculation and the fast finish off by environment variables; r6 removed those switches -- the paths they selected are the only
    ones left, held to the oracle by the rest of the suite.)"""
    def run(extra):
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("DIGEST")]
        assert line, r.stdout[-500:] + r.stderr[-500:]
        return line[0]
    a = run({})
    b = run({"ICPMI_ALLOC_CACHE_MB": "0"})
    assert a == b


def test_self_search_grid_follows_the_density_and_the_neighbours_do_not(amd, oracle):
    """A cloud with a heavy-tailed density (a dense patch along a 'trajectory', sparse far field): the single-level grid of the tiled self
    search is re-tuned from what the points of the previous search saw (sum of squared cell counts).  The search is exact whatever the
    grid: neighbour ids, normals and mean distances of the first, second and third call on ONE handle are identical, and the ids are the
    oracle's."""
    rng = np.random.default_rng(5)
    dense = np.c_[rng.uniform(-3, 3, 60000), rng.uniform(-3, 3, 60000), 0.02 * rng.standard_normal(60000)]
    ring = rng.uniform(0, 2 * np.pi, 25000); rad = rng.uniform(20, 120, 25000)
    far = np.c_[rad * np.cos(ring), rad * np.sin(ring), 0.5 * rng.standard_normal(25000) + 0.01 * rad]
    wall = np.c_[rng.uniform(-40, 40, 15000), np.full(15000, 35.0) + 0.03 * rng.standard_normal(15000), rng.uniform(0, 6, 15000)]
    pts = np.concatenate([dense, far, wall]).astype(np.float32)
    cloud = np.c_[pts, np.ones(len(pts), np.float32)].astype(np.float32)
    cloud = cloud[rng.permutation(len(cloud))]
    icp = amd.ICPSequence(minimizer=2)
    runs = [icp.surfaceNormals(cloud, knn=10, with_matched_ids=True, with_mean_dist=True) for _ in range(3)]
    for r in runs[1:]:
        for x, y in zip(r, runs[0]):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
    _, ids_o, md_o = oracle.surface_normals_extras(cloud, knn=10, nthreads=8)
    assert np.array_equal(runs[0][1], ids_o)
    assert np.array_equal(runs[0][2].view(np.uint32), md_o.view(np.uint32))


@pytest.mark.parametrize("checked", [1, 0])
def test_finished_state_reaches_the_host_by_itself(amd, small_scene, checked):
    """r5 fast finish: the solve that stops the loop mirrors the state into the handle's pinned block in front of the "done" word and
    loop_run returns on that word -- no copy, no drained stream, no event pair; stats.loop_ms comes from the device clocks the state
    carries.  Back-to-back registrations (the next one is enqueued while the previous graph's tail still runs), alternating scans and
    sizes: pose, iterations, stop reason, pair count, trim limit of every call equal the eager handle's, and the device time of the loop
    is positive and not longer than the call."""
    import time
    sc = small_scene
    kw = dict(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=40 if checked else 12, use_differential=checked)
    icp = amd.ICPSequence(**kw); icp.setMap(sc["map"], sc["normals"])
    ref = amd.ICPSequence(use_graph=0, **kw); ref.setMap(sc["map"], sc["normals"])
    scans = [sc["scan"], sc["scan"][::2].copy(), sc["scan"][: 3000].copy()]
    for rep in range(12):
        s = scans[rep % 3]
        t0 = time.perf_counter(); T = icp(s); wall = (time.perf_counter() - t0) * 1e3
        a = (icp.stats.iterations, icp.stats.stop_reason, icp.stats.pairs, icp.stats.trimmed_limit, icp.stats.weighted_point_used_ratio)
        lm = icp.stats.loop_ms
        Tr = ref(s)
        b = (ref.stats.iterations, ref.stats.stop_reason, ref.stats.pairs, ref.stats.trimmed_limit, ref.stats.weighted_point_used_ratio)
        assert a == b, rep
        assert np.array_equal(_bits(T), _bits(Tr)), rep
        assert 0.0 < lm <= wall * 1.05 + 0.05, (rep, lm, wall)
    # an error raised on the device travels the same way (no point within reach: "no point to minimize" / "no outlier to filter")
    far = sc["scan"].copy(); far[:, :3] += np.float32(500.0)
    for h in (icp, ref):
        with pytest.raises(Exception) as ei:
            h(far)
        assert "ConvergenceError" in str(ei.value)
    assert np.array_equal(_bits(icp(sc["scan"])), _bits(ref(sc["scan"])))   # ... and the handle goes on


@pytest.mark.parametrize("knn", [10, 5, 12])
def test_self_search_leftovers_of_a_sparse_periphery(amd, oracle, knn):
    """What a lidar map does to the self search: a dense patch and a few hundred isolated points scattered over hundreds of
    metres.  The isolated points' neighbours lie dozens of cells away: the tiled pass leaves them to the ring kernel (pruned by the k-th key
    of the rings before), six rings decide nothing, and the brute pass (bounded by the k-th key the ring kernel left in the row, eight
    candidates per trip) finds them.  Neighbour ids and mean distances are the oracle's, bit for bit; a second call on the same handle too."""
    rng = np.random.default_rng(31 + knn)
    dense = np.c_[rng.uniform(-4, 4, 40000), rng.uniform(-4, 4, 40000), 0.05 * rng.standard_normal(40000)]
    lone = rng.uniform(-300, 300, (400, 3)) * np.array([1.0, 1.0, 0.05])
    pairs = lone[:120] + rng.normal(0, 0.4, (120, 3))          # some of them in loose pairs: short lists that fill late
    line = np.c_[np.linspace(20, 250, 600), 0.2 * rng.standard_normal(600), 0.2 * rng.standard_normal(600)]   # a thin row of posts: neighbours along one axis only
    pts = np.concatenate([dense, lone, pairs, line]).astype(np.float32)
    cloud = np.c_[pts, np.ones(len(pts), np.float32)].astype(np.float32)
    cloud = cloud[rng.permutation(len(cloud))]
    icp = amd.ICPSequence(minimizer=2)
    first = icp.surfaceNormals(cloud, knn=knn, with_matched_ids=True, with_mean_dist=True)
    again = icp.surfaceNormals(cloud, knn=knn, with_matched_ids=True, with_mean_dist=True)
    _, ids_o, md_o = oracle.surface_normals_extras(cloud, knn=knn, nthreads=8)
    assert np.array_equal(first[1], ids_o)
    assert np.array_equal(first[2].view(np.uint32), md_o.view(np.uint32))
    for x, y in zip(first, again):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


_LIFE_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, %r)
import norlab_icp_mapper_amd as pkg
from norlab_icp_mapper_amd import _capi
lib = _capi.load()
sc = pkg.synth.make_scene(m=1_000_000, n=20000)
delta = pkg.synth.make_scene(m=8, n=20000, seed_scan=977)["scan"]
far = sc["scan"].copy(); far[:, 0] += np.float32(0.31)
kw = dict(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=8, use_differential=0)


def used():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def life():
    icp = pkg.ICPSequence(**kw)
    assert icp.setMap(sc["map"], sc["normals"])
    icp.setMapScalar(np.full(sc["map"].shape[0], 0.6, np.float32))
    icp(sc["scan"])                                                      # k = 1
    icp.setConfig(knn=6, **kw)
    icp(sc["scan"])                                                      # k = 6
    pose = np.eye(4, dtype=np.float32)
    icp.mapUpdateChain(sc["scan"], [("dynamic_points", 0.9, 0.8, 0.99, 0.01, 0.01, 0.01, 200.0), ("octree", 0.15, 1, 1)],
                       [("surface_normals", 10), ("cut_scalar", 0.65, 1)], scan_scalar=np.full(sc["scan"].shape[0], 0.6, np.float32),
                       to_sensor=pose, from_sensor=pose)
    icp.surfaceNormals(sc["map"][::4], knn=10)
    for d in (delta, far):                                               # appends: the private raw index, the insert's ping-pong set
        icp.mapUpdatePointDistance(d, 0.05, normals_knn=10)
    c = icp.debugCounters()
    icp.close()
    assert lib.icpmi_trim_cache() == 0
    return used(), c


used()                                                                   # (the runtime's own context before anything is measured)
u1, c1 = life()
u2, c2 = life()
print("LIFE", u1, u2, u2 - u1, c1[18] & 0xffffffff, c1[18] >> 32, c1[20], c1[21])
"""


# Growth of used device memory (torch.cuda.mem_get_info) from the end of life 1 to the end of life 2.  Measured on an MI355X with the
# hand-written free lists this test was added to replace: 0 bytes (884 998 144 used after either life); with the self-freeing arrays: 0 bytes.
_LIFE_GROWTH_BEFORE = 0
_LIFE_GRANULE = 2 << 20   # what the runtime maps a device allocation in; a forgotten array of the 1 M-point map is 16 MB


def test_a_destroyed_handle_gives_its_device_memory_back():
    """Every device array of a handle frees itself when the handle dies (common.h: DevArr); nothing else looks at device memory after a
    destroy, so a forgotten array would be a silent leak.  One life in a fresh process: a handle, a map of 1 M points with normals, a k = 1
    and a k = 6 registration, the shipped map-update chain, a SurfaceNormal pass, two appends (private handles, self grid, the insert's
    ping-pong set, operator scratch all exist), destroy, icpmi_trim_cache().  The first life warms the runtime; used memory after the
    second may exceed used memory after the first by what it did before this type existed plus one granule -- one forgotten array of the
    1 M-point map is 16 MB."""
    r = subprocess.run([sys.executable, "-c", _LIFE_CHILD % ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("LIFE")]
    assert line, r.stdout[-500:] + r.stderr[-500:]
    print(line[0])
    f = line[0].split()
    growth = int(f[3])
    assert int(f[4]) + int(f[5]) >= 1, line[0]       # an append did go through the incremental insert
    assert growth <= _LIFE_GROWTH_BEFORE + _LIFE_GRANULE, line[0]
