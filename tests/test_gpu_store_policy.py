"""The loop kernels' result stores and clears at the shapes where a wider or differently addressed store can go wrong (common.h: st_wt,
clear_words_wt and the ICPMI_WT_* sites): readings of 1, 63, 64, 65, 129 and 1 000 points -- one lane, a wave less one, exactly one
workgroup of the k = 1 matcher, one query into the next, two workgroups and one query, a partial sixteenth -- on a 4 096-point map.

  - three chains (point-to-point k = 1, point-to-plane k = 1, point-to-plane knn 3), three fixed iterations, from one graph and eagerly: the
    matches the last iteration left (icpmi_debug_last_matches) against a brute-force float64 search in numpy and the comparison of
    test_gpu_loop_matches.py (match_reference.check_matches: ids and d2 bitwise the oracle's), under the pose they were formed with; pose
    and matches bitwise equal between the two routes;
  - a batch of three readings (65, 1 and 200 points) through registerBatchDev: every item bitwise its single registration (slices at
    qstride offsets, partial last workgroups);
  - two registrations of different readings on one handle, the larger first: the second equals a fresh handle's (no stale tail of the
    longer reading survives in the per-query arrays or the histograms)."""
import numpy as np
import pytest

import match_reference as mr
from loop_driver import centring

pytestmark = pytest.mark.gpu

M_MAP, N_MAX, ITERS = 4096, 1000, 3
NS = (1, 63, 64, 65, 129, 1000)
MAX_DIST, RATIO = 2.0, 0.85
CHAINS = {
    "p2p_k1": dict(minimizer=1, knn=1),
    "p2plane_k1": dict(minimizer=2, knn=1),
    "p2plane_k3": dict(minimizer=2, knn=3),
}


class World:
    """the scene, its readings on the device and one handle per (chain, route), built once"""

    def __init__(self):
        import torch
        import norlab_icp_mapper_amd as pkg
        self.pkg = pkg
        sc = pkg.synth.make_scene(m=M_MAP, n=N_MAX)
        self.map, self.normals, self.scan = sc["map"], sc["normals"], sc["scan"]
        self.d_scan = torch.from_numpy(self.scan).cuda()   # a reading of n points is its first n
        self.handles = {}
        self.singles = {}

    def make(self, chain, use_graph=1):
        icp = self.pkg.ICPSequence(max_dist=MAX_DIST, outliers=[(4, RATIO)], max_iterations=40, use_differential=0, use_graph=use_graph, **CHAINS[chain])
        assert icp.setMap(self.map, self.normals)
        return icp

    def handle(self, chain, use_graph):
        key = (chain, use_graph)
        if key not in self.handles:
            self.handles[key] = self.make(chain, use_graph)
        return self.handles[key]

    def map_centred(self, icp):
        mean = icp.getMapMean()
        mc = self.map.copy(); mc[:, :3] = self.map[:, :3] - mean[None, :]
        return mean, mc

    def register(self, icp, n, offset=0):
        """(pose bytes, ids, d2, T_used, pairs, limit bits) of a fixed registration of points [offset, offset + n) of the scan, or the
        library's refusal (ConvergenceError: a reading the chain cannot minimise over -- every route must then say the same)"""
        try:
            T = icp.registerDev(self.d_scan.data_ptr() + 16 * offset, n, fixed_iterations=ITERS)
        except self.pkg.ConvergenceError as e:
            return ("error", str(e))
        assert int(icp.stats.iterations) == ITERS
        ids, d2, T_used = icp.lastMatches()
        return (np.asarray(T, np.float32).tobytes(), ids, d2, T_used, int(icp.stats.pairs), np.float32(icp.stats.trimmed_limit).tobytes())

    def single(self, chain, n, offset=0):
        """the single registration of that reading on the graph route's handle, run once and shared"""
        key = (chain, n, offset)
        if key not in self.singles:
            self.singles[key] = self.register(self.handle(chain, 1), n, offset)
        return self.singles[key]


@pytest.fixture(scope="module")
def world():
    return World()


def brute_force(map_c, q, k):
    """float64 squared distances of every query to every map point: (ids (n, k), d2 (n, k + 1)) ascending by (distance, index)"""
    d = ((q[:, None, :3].astype(np.float64) - map_c[None, :, :3].astype(np.float64)) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
    return order[:, :k], np.take_along_axis(d, order, axis=1)


def check_against_brute_force(tag, oracle, w, icp, n, offset, ids, d2, T_used, k):
    mean, map_c = w.map_centred(icp)
    q = oracle.transform(T_used, oracle.transform(centring(mean), w.scan[offset:offset + n]))
    bid, bd = brute_force(map_c, q, k)
    r2 = MAX_DIST ** 2
    for j in range(k):
        inside = bd[:, j] <= r2 * (1 - mr.MAXD_REL)
        outside = bd[:, j] > r2 * (1 + mr.MAXD_REL)
        assert (ids[inside, j] >= 0).all() and (ids[outside, j] == -1).all() and np.isinf(d2[outside, j]).all(), (tag, "filled exactly within maxDist", j)
        lo = bd[:, j - 1] if j else np.full(n, -np.inf)
        clear = inside & (bd[:, j] - lo > mr.RANK_REL * bd[:, j]) & (bd[:, j + 1] - bd[:, j] > mr.RANK_REL * bd[:, j + 1])
        assert np.array_equal(ids[clear, j], bid[clear, j].astype(np.int32)), (tag, "ids against the brute-force search", j)
        # float32 rounding of the pair's own distance (D2_REL), and two neighbours closer than RANK_REL may have swapped
        assert (np.abs(d2[inside, j].astype(np.float64) - bd[inside, j]) <= (mr.D2_REL + mr.RANK_REL) * bd[inside, j]).all(), (tag, "d2", j)
    # ids equal, d2 bitwise: the oracle's kd-tree over the same float32 arithmetic, and the float64 exact search (test_gpu_loop_matches.py)
    mr.check_matches(map_c, q, ids, d2, k, MAX_DIST, where=tag)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_matches_of_small_readings_graph_and_eager(world, oracle, chain, n):
    k = CHAINS[chain]["knn"]
    got = {}
    for use_graph in (1, 0):
        icp = world.handle(chain, use_graph)
        r = world.single(chain, n) if use_graph else world.register(icp, n)
        got[use_graph] = r
        if r[0] == "error":
            continue
        ids, d2, T_used = r[1:4]
        print(f"{chain} n={n} use_graph={use_graph}: {int((ids >= 0).sum())} of {n * k} slots filled")
        check_against_brute_force(f"{chain} n={n} use_graph={use_graph}", oracle, world, icp, n, 0, ids, d2, T_used, k)
    g, e = got[1], got[0]
    if g[0] == "error" or e[0] == "error":
        assert g[:2] == e[:2], (chain, n, "one route failed, the other did not, or they failed differently", g[:2], e[:2])
        return
    assert g[0] == e[0], (chain, n, "pose differs between the graph and the eager route")
    assert np.array_equal(g[1], e[1]) and g[2].tobytes() == e[2].tobytes() and np.array_equal(g[3], e[3]), (chain, n, "matches differ between the routes")
    assert g[4:] == e[4:], (chain, n, "pairs / trimmed limit differ between the routes")


@pytest.mark.parametrize("chain", list(CHAINS))
def test_batch_items_equal_their_single_registrations(world, chain):
    """readings of 65, 1 and 200 points (disjoint stretches of the scan) in one batch"""
    items = [(65, 0), (1, 65), (200, 66)]
    singles = [world.single(chain, n, off) for n, off in items]
    icp = world.make(chain)
    Ts, stats, status = icp.registerBatchDev([world.d_scan.data_ptr() + 16 * off for _, off in items], [n for n, _ in items], fixed_iterations=ITERS)
    for b, ((n, off), s) in enumerate(zip(items, singles)):
        if s[0] == "error":
            assert status[b] != 0, (chain, b, "the single registration failed, the batch item did not", s)
            continue
        assert status[b] == 0, (chain, b, status)
        assert np.asarray(Ts[b], np.float32).tobytes() == s[0], (chain, b, n, "batch item differs from its single registration")
        # pairs and limit of the item's last iteration: what its matches and its selection came to
        assert int(stats[b].pairs) == s[4], (chain, b, int(stats[b].pairs), s[4])
        assert np.float32(stats[b].trimmed_limit).tobytes() == s[5], (chain, b)


@pytest.mark.parametrize("chain", list(CHAINS))
def test_shorter_reading_after_a_longer_one(world, chain):
    """1 000 points, then 65 other points on the same handle: the second registration is a fresh handle's"""
    used = world.make(chain)
    first = world.register(used, 1000, 0)
    assert first[0] != "error"
    second = world.register(used, 65, 300)
    fresh = world.register(world.make(chain), 65, 300)
    assert second[0] != "error" and fresh[0] != "error", (second[:2], fresh[:2])
    assert second[0] == fresh[0], (chain, "pose after a longer reading on the same handle")
    assert np.array_equal(second[1], fresh[1]) and second[2].tobytes() == fresh[2].tobytes() and np.array_equal(second[3], fresh[3]), (chain, "matches")
    assert second[4:] == fresh[4:] and second[4] >= 1, (chain, "pairs / trimmed limit", second[4:], fresh[4:])
