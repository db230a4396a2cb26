"""The answer of a call does not depend on what the handle did before it.

Everything a launch of the matcher is asked travels in its own request (csrc/common.h: NnRequest) and what it decided comes back as its
outcome; nothing of either is kept on the handle.  So a call made as the n-th on a handle that has been through registrations with graphs,
stage searches, a var-dist row, k-lists in tile order, a single step and a batch answers bit for bit what the same call answers as the
first one on a fresh handle with the same map.

Scene: synth.make_scene(m=20_000, n=1_501) -- the reading is not a multiple of the 64 queries a workgroup owns, the map has more than
one pyramid level at maxDist 2.  Every handle is created with the first chain, takes the map, and changes chain through setConfig (the
pyramid is cut for the maxDist the handle had when the map arrived: the fresh handles share that with the two long-lived ones).  The
eleven steps run on ONE handle in the listed order, and on another handle in reverse order; each is compared with its fresh-handle
answer, computed once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIO = 0.85
K1 = dict(minimizer=2, knn=1, max_dist=2.0, outliers=[(4, RATIO)], max_iterations=40, use_differential=1, use_graph=1)
VAR = dict(minimizer=1, knn=1, var_dist=1, outliers=[(4, RATIO)], max_iterations=40, use_differential=1, use_graph=1)
K6 = dict(minimizer=2, knn=6, max_dist=2.0, outliers=[(4, RATIO)], max_iterations=40, use_differential=1, use_graph=0)


def bits(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.uint32) if a.dtype == np.float32 else a).tobytes()


def registered(icp, T):
    s = icp.stats
    return (bits(T), int(s.iterations), int(s.pairs), bits(np.float32(s.trimmed_limit)))


# ---- the steps: (chain the handle runs it under, call); each returns what is compared byte for byte
def register_twice(icp, w):
    return [registered(icp, icp(w["scan"])) for _ in range(2)]          # the second: the cached graphs


def knn1(icp, w):
    return [bits(a) for a in icp.knn(w["q"], k=1, max_dist=2.0)]


def knn_var1(icp, w):
    return [bits(a) for a in icp.knnVar(w["q"], w["row"], k=1)]


def register_var(icp, w):
    icp.setReadingMaxDist(w["row"])
    return registered(icp, icp(w["scan"]))


def knn6(icp, w):
    return [bits(a) for a in icp.knn(w["q"], k=6, max_dist=2.0)]


def register_k6(icp, w):
    return registered(icp, icp(w["scan"]))


def minimize_step(icp, w):
    T, sums = icp.minimizeStep(w["q"])
    return (bits(T), bits(sums), int(icp.stats.pairs), bits(np.float32(icp.stats.trimmed_limit)))


def last_matches(icp, w):
    r = registered(icp, icp(w["scan"]))
    ids, d2, T_used = icp.lastMatches()
    return (r, bits(ids), bits(d2), bits(T_used))


def register_batch(icp, w):
    Ts, stats, status = icp.registerBatchDev([d.data_ptr() for d in w["dev"]], [d.shape[0] for d in w["dev"]])
    return [(status[b], bits(Ts[b]), int(stats[b].iterations), int(stats[b].pairs), bits(np.float32(stats[b].trimmed_limit))) for b in range(2)]


def point_distance_keep(icp, w):
    return bits(icp.pointDistanceKeep(w["map"], w["scan"], w["min_dist"]))


STEPS = [
    ("k1 registration, graphs, twice", K1, register_twice),
    ("knn k=1", K1, knn1),
    ("knnVar k=1", K1, knn_var1),
    ("var_dist registration", VAR, register_var),
    ("knn k=6", VAR, knn6),
    ("k6 registration, eager, checked", K6, register_k6),
    ("minimizeStep", K6, minimize_step),
    ("lastMatches behind a registration", K6, last_matches),
    ("registerBatchDev of two", K1, register_batch),
    ("pointDistanceKeep", K1, point_distance_keep),
    ("the first registration again", K1, register_twice),
]


def handle(amd, w):
    icp = amd.ICPSequence(**K1)
    assert icp.setMap(w["map"], w["normals"])
    return icp, K1


def run(icp, current, step, w):
    name, chain, call = step
    if chain is not current:
        icp.setConfig(**chain)
    return call(icp, w), chain


@pytest.fixture(scope="module")
def world():
    import torch
    import norlab_icp_mapper_amd as amd
    sc = amd.synth.make_scene(m=20_000, n=1_501)
    w = dict(map=sc["map"], normals=sc["normals"], scan=sc["scan"])
    icp, _ = handle(amd, w)
    q = sc["scan"].copy()
    q[:, :3] -= icp.getMapMean()
    w["q"] = q
    rng = np.random.default_rng(5)
    w["row"] = (0.5 + 1.5 * rng.random(q.shape[0])).astype(np.float32)     # non-constant, every radius within maxDist 2
    _, d2 = icp.knn(q, k=1, max_dist=2.0)
    w["min_dist"] = float(np.sqrt(np.median(d2[np.isfinite(d2)])))         # a keep decision that splits the reading
    second = sc["scan"][:1_137].copy()
    second[:, :3] += np.float32(0.01)
    w["dev"] = [torch.from_numpy(sc["scan"]).cuda(), torch.from_numpy(np.ascontiguousarray(second)).cuda()]
    for a in (w["map"], w["normals"], w["scan"], w["q"], w["row"]):
        a.setflags(write=False)
    fresh = []
    for step in STEPS:
        f, cur = handle(amd, w)
        fresh.append(run(f, cur, step, w)[0])
        if step[2] is register_k6:
            assert f.stats.iterations > 3                                   # the window and nnk_wg_kernel are in play from iteration 2 on
        f.close()
    keep = np.frombuffer(fresh[9], dtype=np.bool_)
    assert 0 < keep.sum() < keep.size
    assert fresh[0] == fresh[10]
    w["fresh"] = fresh
    return amd, w


@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_a_call_answers_as_on_a_fresh_handle(world, order):
    amd, w = world
    idx = list(range(len(STEPS)))
    if order == "reversed":
        idx.reverse()
    icp, cur = handle(amd, w)
    differing = []
    for i in idx:
        got, cur = run(icp, cur, STEPS[i], w)
        if got != w["fresh"][i]:
            differing.append(STEPS[i][0])
    assert not differing, (order, differing)
