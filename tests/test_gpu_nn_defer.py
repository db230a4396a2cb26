"""Far-seeded queries of the k = 1 loop run in helper workgroups of eight (nn.hip: nn1_wg_kernel, `defer`): every output must keep its bits.

Map: 4 096 points in a slab 16 x 16 x 1 m.  A reading is a subset of the map points, a little noise on each, seen from a slightly wrong
pose.  Its HEAVY points are lifted out of the slab by 2.5 level-0 cells, alternately above and below it (so that no rigid motion brings
them back): their nearest map point is farther away than any 3 x 3 x 3 block of level 0 reaches around them -- block_margin is at most
1.5 cells -- so their search, seeded or not, ends above level 0 and the matcher's tail puts them on the next launch's defer list.  The
construction is checked on the CPU with that rule (exact nearest-neighbour distance > 2 cells for heavy points) before any of it is used.

Cases (share of heavy points): none; a few that are neighbours in space, hence in tile order; a few scattered; more than the lists hold
(a handle created under ICPMI_NN_DEFER_WGS=8: 64 entries); all.  Readings of 1, 63, 64, 65, 129 and 1 000 points.

Every case runs as fixed-count registrations of 1 ... 5 iterations (graph), of 2 and 3 (eager), twice in a row, and as a checked (Counter +
Differential) loop; a batch of 65 / 1 / 200 points against the single registrations; a short reading after a long one on one handle.  Pose,
pair count, trim limit, and the matches and d2 of every iteration (the last counted iteration of a j-iteration registration) are compared
bitwise with a handle created under ICPMI_NN_DEFER=0, and the matches against the oracle's kd-tree and an exact float64 search
(tests/match_reference.py).  icpmi_debug_counters 10 (queries served by helpers) is above zero wherever a third launch
runs and the level rule, applied on the CPU to the pose of launch 1, still finds heavy points (the one-point reading's first solve moves
its point home; what launch 0 marks depends on the unseeded search and is not relied on), 11 (heavy queries that found the list full) is above zero exactly in the capacity case with more than 64 heavy points, and both
are zero with the switch off."""
import contextlib
import os

import numpy as np
import pytest

import match_reference as mr
from loop_driver import centring

pytestmark = pytest.mark.gpu

SERVED, OVERFLOW = 10, 11   # icpmi_debug_counters
M = 4096
SIZES = [1, 63, 64, 65, 129, 1000]
CASES = ["none", "contiguous", "scattered", "capacity", "all"]
CFG = dict(minimizer=1, knn=1, outliers=[(4, 0.85)])


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


class World:
    """the map, the handles (created once per (mode, graph, checked): the switches are read when a handle is created), the readings"""
    def __init__(self, amd):
        self.amd = amd
        rng = np.random.default_rng(7)
        mp = np.ones((M, 4), np.float32)
        mp[:, :3] = rng.uniform(0.0, 1.0, (M, 3)) * np.array([16.0, 16.0, 1.0])
        self.map = mp
        self.handles = {}
        h = self.handle("on", 1, False)
        info = h.gridInfo()
        self.cell = float(info["cell"])
        assert min(info["dims"][:2]) > 3, ("a 3 x 3 x 3 block must not cover the grid", info)
        self.max_dist = 4.0 * self.cell
        self.handles.clear()          # (max_dist is part of the chain: the handles are made again with it)
        self.mean = self.handle("on", 1, False).getMapMean()
        self.mapc = mp.copy(); self.mapc[:, :3] = mp[:, :3] - self.mean[None, :]
        self.readings = {}

    def handle(self, mode, graph, checked):
        key = (mode, graph, checked)
        if key not in self.handles:
            env = {"on": dict(ICPMI_NN_DEFER=None, ICPMI_NN_DEFER_WGS=None), "off": dict(ICPMI_NN_DEFER="0", ICPMI_NN_DEFER_WGS=None),
                   "cap": dict(ICPMI_NN_DEFER=None, ICPMI_NN_DEFER_WGS="8")}[mode]
            with environ(**env):
                icp = self.amd.ICPSequence(**CFG, max_dist=getattr(self, "max_dist", 2.0), use_graph=graph, max_iterations=40, use_differential=1 if checked else 0)
            assert icp.setMap(self.map, None)
            self.handles[key] = icp
        return self.handles[key]

    def reading(self, n, case):
        """(reading (n, 4) f32, number of heavy points); the heavy points' distance to the map is checked here, on the CPU"""
        key = (n, case)
        if key in self.readings:
            return self.readings[key]
        from norlab_icp_mapper_amd import synth
        rng = np.random.default_rng(1000 * n + CASES.index(case))
        pick = rng.choice(M, n, replace=False)
        p = self.map[pick, :3].astype(np.float64) + rng.normal(0.0, 0.01 * self.cell, (n, 3))
        few = max(1, n // 16)
        if case == "none": heavy = np.zeros(0, np.int64)
        elif case == "contiguous": heavy = np.argsort(((p[:, :2] - p[0, :2]) ** 2).sum(1))[:few]   # the `few` points nearest to point 0
        elif case == "scattered": heavy = rng.choice(n, few, replace=False)
        elif case == "capacity": heavy = rng.choice(n, min(n, 100 if n < 1000 else 200), replace=False)
        else: heavy = np.arange(n)
        up = (np.arange(heavy.size) % 2) == 0
        p[heavy, 2] = np.where(up, 1.0 + 2.5 * self.cell, -2.5 * self.cell)
        # the model's level rule: a level-0 block reaches at most 1.5 cells from the query (common.h: block_margin), so a nearest map point
        # farther than that keeps the search from ending at level 0; 2 cells leave half a cell for the pose's motion.  Light points: the
        # map point they were drawn from is within a tenth of a cell.
        d = np.sqrt(((p[:, None, :] - self.map[None, :, :3].astype(np.float64)) ** 2).sum(-1).min(1))   # (n x 4 096 distances: plain numpy)
        is_heavy = np.zeros(n, bool); is_heavy[heavy] = True
        assert (d[is_heavy] > 2.0 * self.cell).all() and (d[is_heavy] < 0.9 * self.max_dist).all(), (n, case, d[is_heavy].min(), d[is_heavy].max())
        assert (d[~is_heavy] < 0.1 * self.cell).all(), (n, case)
        T = synth.make_T((0.002, -0.001, 0.003), (0.02 * self.cell, -0.03 * self.cell, 0.01 * self.cell))
        rd = np.ones((n, 4), np.float32)
        rd[:, :3] = (np.linalg.inv(T) @ np.c_[p, np.ones(n)].T).T[:, :3]
        self.readings[key] = (np.ascontiguousarray(rd), int(heavy.size))
        return self.readings[key]


@pytest.fixture(scope="module")
def world():
    import norlab_icp_mapper_amd as pkg
    return World(pkg)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def register(icp, dev, fixed):
    """what a registration leaves behind, as bits (the one-point reading, too small for the chain: the error's name, which both handles must
    agree on; an error at any other size fails the test here)"""
    try:
        T = icp.registerDev(dev.data_ptr(), dev.shape[0], fixed_iterations=fixed)
        ids, d2, T_used = icp.lastMatches()
    except Exception as e:  # noqa: BLE001
        assert dev.shape[0] == 1, ("only the one-point reading may be too small for the chain", dev.shape[0], fixed, repr(e))
        return dict(error=type(e).__name__)
    s = icp.stats
    return dict(T=bits(T), iterations=int(s.iterations), pairs=int(s.pairs), limit=bits(np.float32(s.trimmed_limit)), ids=ids.copy(), d2=bits(d2),
                T_used=bits(T_used), Tu=np.asarray(T_used, np.float32), d2f=d2.copy(), dbg=icp.debugCounters())


def same(a, b, where):
    assert a.get("error") == b.get("error"), (where, a.get("error"), b.get("error"))
    if "error" in a:
        return
    for k in ("T", "iterations", "pairs", "limit", "ids", "d2", "T_used"):
        assert np.array_equal(a[k], b[k]), (where, k, a[k], b[k])


def heavy_under(world, oracle, centred, Tu):
    """queries that the level rule makes heavy under pose Tu (the pose of launch 1, the first launch that marks): nearest map point
    farther than 1.5 level-0 cells, the most a level-0 block reaches.  The lifted points of a reading stay there unless the solve can move
    the reading onto them -- the one-point reading's single pair does exactly that -- so this is asked of the pose, not assumed."""
    q = oracle.transform(Tu, centred)[:, :3].astype(np.float64)
    d = np.sqrt(((q[:, None, :] - world.mapc[None, :, :3].astype(np.float64)) ** 2).sum(-1).min(1))
    return int((d > 1.5 * world.cell).sum())


def check_counters(r, mode, fixed, n_heavy, where):
    if "error" in r:
        return
    served, over = r["dbg"][SERVED], r["dbg"][OVERFLOW]
    print(where, "served", served, "overflow", over, "heavy", n_heavy)
    if mode == "off":
        assert served == 0 and over == 0, (where, served, over)
        return
    if n_heavy and (fixed == 0 or fixed >= 3):   # (what launch 1 marks under its pose, launch 2 serves)
        assert served > 0, (where, "the helper path was never taken", served)
    cap = 64 if mode == "cap" else 8 * 160
    if n_heavy > cap and (fixed == 0 or fixed >= 3): assert over > 0, (where, over)
    if r["ids"].shape[0] <= cap: assert over == 0, (where, over)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", SIZES)
def test_defer_keeps_every_bit(world, oracle, n, case):
    import torch
    rd, n_heavy = world.reading(n, case)
    dev = torch.from_numpy(rd).cuda()
    mode = "cap" if case == "capacity" else "on"
    on, off = world.handle(mode, 1, False), world.handle("off", 1, False)
    centred = oracle.transform(centring(world.mean), rd)
    ref = {}
    for j in (1, 2, 3, 4, 5):   # fixed counts, odd and even; the matches of every iteration
        where = f"n={n} {case}: {j} fixed iterations"
        a, b = register(on, dev, j), register(off, dev, j)
        same(a, b, where)
        if j == 3 and "error" not in ref[2]: n_heavy = heavy_under(world, oracle, centred, ref[2]["Tu"])   # (T_used of the 2-iteration run = the pose of launch 1)
        check_counters(a, mode, j, n_heavy, where); check_counters(b, "off", j, n_heavy, where)
        if "error" not in a:
            mr.check_matches(world.mapc, oracle.transform(a["Tu"], centred), a["ids"], a["d2f"], 1, world.max_dist, where=where)
        ref[j] = b
    same(register(on, dev, 5), ref[5], f"n={n} {case}: the same registration again")
    on_e = world.handle(mode, 0, False)
    for j in (2, 3):            # eager launches
        where = f"n={n} {case}: {j} eager iterations"
        a = register(on_e, dev, j)
        same(a, ref[j], where)
        check_counters(a, mode, j, n_heavy, where)
    for graph in (1, 0):        # Counter + Differential: segment graphs, eager run-ahead
        where = f"n={n} {case}: checked loop, use_graph={graph}"
        a, b = register(world.handle(mode, graph, True), dev, 0), register(world.handle("off", graph, True), dev, 0)
        same(a, b, where)
        check_counters(a, mode, 0 if a.get("iterations", 0) >= 3 else 1, n_heavy, where); check_counters(b, "off", 0, n_heavy, where)
        if "error" not in a:
            mr.check_matches(world.mapc, oracle.transform(a["Tu"], centred), a["ids"], a["d2f"], 1, world.max_dist, where=where)


@pytest.mark.parametrize("case", ["scattered", "all"])
def test_batch_against_single_registrations(world, case):
    """a batch keeps every query in its home workgroup (the lists belong to one reading): it answers what the single registrations answer"""
    import torch
    on = world.handle("on", 1, False)
    rds = [world.reading(n, case)[0] for n in (65, 1, 1000)]
    rds[2] = rds[2][:200]
    dev = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in rds]
    for fixed in (3, 4):
        single = [register(on, d, fixed) for d in dev]
        Ts, stats, status = on.registerBatchDev([d.data_ptr() for d in dev], [d.shape[0] for d in dev], fixed_iterations=fixed)
        for b, s in enumerate(single):
            assert (status[b] != 0) == ("error" in s), (case, fixed, b, status[b], s.get("error"))
            if "error" in s:
                continue
            assert np.array_equal(bits(Ts[b]), s["T"]), (case, fixed, b)
            assert (int(stats[b].iterations), int(stats[b].pairs)) == (s["iterations"], s["pairs"]), (case, fixed, b)
            assert np.array_equal(bits(np.float32(stats[b].trimmed_limit)), s["limit"]), (case, fixed, b)
        again = [register(on, d, fixed) for d in dev]      # ... and the lists of the single path are whole behind a batch
        for s, a in zip(single, again): same(a, s, f"{case}: single registration behind a batch")


@pytest.mark.parametrize("mode", ["on", "cap"])
def test_short_reading_after_long_one(world, oracle, mode):
    """the flags and lists a 1 000-point registration left behind mean nothing to the 63-point one that follows on the same handle"""
    import torch
    on, off = world.handle(mode, 1, False), world.handle("off", 1, False)
    long_rd, short_rd = world.reading(1000, "all")[0], world.reading(63, "contiguous")[0]
    dl, ds = torch.from_numpy(long_rd).cuda(), torch.from_numpy(short_rd).cuda()
    for j in (4, 3):
        register(on, dl, j); register(off, dl, j)
        a, b = register(on, ds, j), register(off, ds, j)
        same(a, b, f"{mode}: 63 points behind 1 000, {j} iterations")
        assert heavy_under(world, oracle, oracle.transform(centring(world.mean), short_rd), register(off, ds, 2)["Tu"]) > 0
        assert a["dbg"][SERVED] > 0 and b["dbg"][SERVED] == 0
