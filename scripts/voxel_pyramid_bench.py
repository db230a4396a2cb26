"""VoxelMatcher with a schedule of voxel sizes at the headline shape (100 k x 1 M): what a checked registration from a
start two voxels of the finest size off costs and where it ends, schedule by schedule, next to plane-to-plane through the k = 1 matcher;
what the tables of a schedule cost to build; and what the level read and the advance add to an iteration.

    python scripts/voxel_pyramid_bench.py [--rounds 15] [--warmup 3] [--out profiles/voxel_pyramid_bench.json]

The scene is synth.make_scene with the ground-truth translation stretched to 1.0 m (two voxels of 0.5 m; the rotation stays the scene's).
Handles on the same map -- the schedules (0.5), (1.0, 0.5), (4.0, 2.0, 1.0, 0.5) and plane-to-plane at knn 1 with maxDist 2 and no filter,
all on CounterTransformationChecker 40 + the Differential checker -- take turns, round after round, so that drift of the machine lands on
all alike; medians over the rounds.  Per handle: the whole call on the host clock, the loop's device time, the iterations (per level: the
handle's report) and the end pose's distance from the ground truth.
The time of an iteration at every level INSIDE a schedule: handles with the schedule's prefixes -- (4.0), (4.0, 2.0), (4.0, 2.0, 1.0) and the whole
of it -- run 4 fixed iterations per level from the same start in the same rounds; a prefix runs exactly what the longer schedule runs up to
its last level (the same poses, the same pair counts), so the difference of two neighbouring prefixes' loop times is the added level's four
iterations with its level switch.  (The first level's figure is a one-size handle's and carries the registration's head.)
The time of an iteration at a size on its own: one-size handles at 4.0, 2.0, 1.0 and 0.5 run 20 fixed iterations from the same start in the same
rounds (a level of a schedule runs the same pair work on the same table; its pair count follows the pose, so this is the level's cost at
the start pose, not along the schedule's own path).  What the level read and the advance cost: a (1.0, 0.5) handle at 10 fixed iterations
per level against the mean of the one-size 1.0 and 0.5 handles' 20, the same rounds.
The tables: the host clock around the first lookup after the schedule changed (every level is rebuilt), per schedule.
Nothing is compared against a threshold: the record says what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ITERS = 20
LEVEL_ITERS = 4
SCHEDULES = ((0.5,), (1.0, 0.5), (4.0, 2.0, 1.0, 0.5))
START_OFF = 1.0
CHECKED = dict(max_iterations=40, use_differential=1)


def name_of(sizes):
    return "voxel_" + "_".join(str(s) for s in sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_pyramid_bench.json"))
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    trans = np.asarray(amd.synth.T_GT_TRANS, np.float64)
    sc = amd.synth.make_scene(m=1_000_000, n=100_000, trans=tuple(trans / np.linalg.norm(trans) * START_OFF))
    d = torch.from_numpy(sc["scan"]).cuda()
    dn = torch.from_numpy(sc["scan_normals"]).cuda()
    n = sc["scan"].shape[0]
    new = lambda **kw: amd.ICPSequence(knn=1, max_dist=2.0, outliers=[], minimizer=3, **kw)
    checked = {name_of(s): new(voxel_sizes=list(s), **CHECKED) for s in SCHEDULES}
    checked["plane_to_plane_knn1"] = new(**CHECKED)
    fixed = {f"one_size_{s}": new(voxel_size=s) for s in SCHEDULES[-1]}
    fixed["two_level_1.0_0.5"] = new(voxel_sizes=[1.0, 0.5])
    prefixes = {s[:l]: new(voxel_sizes=list(s[:l])) for s in SCHEDULES[1:] for l in range(1, len(s) + 1)}
    for icp in list(checked.values()) + list(fixed.values()) + list(prefixes.values()):
        assert icp.setMap(sc["map"], sc["normals"])
    ploop, ppairs = {k: [] for k in prefixes}, {}
    wall, loop = {k: [] for k in checked}, {k: [] for k in checked}
    floop = {k: [] for k in fixed}
    end, fpairs = {}, {}
    for r in range(a.warmup + a.rounds):
        for key, icp in checked.items():
            t0 = time.perf_counter()
            try:
                T = icp.registerDev(d.data_ptr(), n, d_normals_ptr=dn.data_ptr())
                status = "ok"
            except amd.icp.ConvergenceError as e:
                T, status = None, str(e)
            t1 = time.perf_counter()
            end[key] = (T, status, int(icp.stats.iterations), int(icp.stats.stop_reason), int(icp.stats.pairs),
                        icp.voxelScheduleReport() if len(icp.getVoxelSchedule()) > 1 else None)
            if r >= a.warmup:
                wall[key].append((t1 - t0) * 1e3)
                loop[key].append(float(icp.stats.loop_ms))
        for key, icp in fixed.items():
            per_level = ITERS // 2 if key.startswith("two_level") else ITERS
            icp.registerDev(d.data_ptr(), n, fixed_iterations=per_level, d_normals_ptr=dn.data_ptr())
            assert icp.stats.iterations == ITERS
            fpairs[key] = int(icp.stats.pairs)
            if r >= a.warmup:
                floop[key].append(float(icp.stats.loop_ms))
        for key, icp in prefixes.items():
            icp.registerDev(d.data_ptr(), n, fixed_iterations=LEVEL_ITERS, d_normals_ptr=dn.data_ptr())
            assert icp.stats.iterations == LEVEL_ITERS * len(key)
            ppairs[key] = int(icp.stats.pairs)
            if r >= a.warmup:
                ploop[key].append(float(icp.stats.loop_ms))
    med = lambda v: float(np.median(v))
    res = dict(shape="100k x 1M; start 1.0 m off (two voxels of 0.5 m) plus the scene's rotation; Counter 40 + Differential(1e-3, 1e-3, 3); "
                     "plane-to-plane: knn 1, maxDist 2, no filter", rounds=a.rounds, registrations={}, iteration_at_a_size={}, level_read_and_advance={},
               tables={})
    for key in checked:
        T, status, its, stop, pairs, rep = end[key]
        rec = dict(status=status, iterations=its, stop_reason=stop, pairs_last=pairs, call_ms=med(wall[key]), call_ms_p10=float(np.percentile(wall[key], 10)),
                   call_ms_p90=float(np.percentile(wall[key], 90)), loop_ms=med(loop[key]), mean_iteration_us=med(loop[key]) / max(its, 1) * 1e3)
        if rep is not None:
            rec["levels"] = [dict(iterations=x[0], pairs_first=x[1], pairs_last=x[2]) for x in rep]
        if T is not None:
            dt, dr = amd.synth.pose_error(T, sc["T_gt"])
            rec.update(pose_err_m=float(dt), pose_err_rad=float(dr))
        res["registrations"][key] = rec
    # per level inside a schedule: the difference of neighbouring prefixes, round by round
    res["iteration_at_a_level"] = {}
    for s in SCHEDULES[1:]:
        rows = []
        for l in range(1, len(s) + 1):
            cur, prev = np.array(ploop[s[:l]]), (np.array(ploop[s[:l - 1]]) if l > 1 else 0.0)
            rows.append(dict(size=s[l - 1], iteration_us=float(np.median(cur - prev)) / LEVEL_ITERS * 1e3, pairs_last=ppairs[s[:l]]))
        res["iteration_at_a_level"][name_of(s)] = dict(fixed_iterations_per_level=LEVEL_ITERS, levels=rows)
    for key in fixed:
        res["iteration_at_a_size"][key] = dict(iteration_us=med(floop[key]) / ITERS * 1e3, pairs_last=fpairs[key], fixed_iterations=ITERS)
    one = 0.5 * (res["iteration_at_a_size"]["one_size_1.0"]["iteration_us"] + res["iteration_at_a_size"]["one_size_0.5"]["iteration_us"])
    two = res["iteration_at_a_size"]["two_level_1.0_0.5"]["iteration_us"]
    res["level_read_and_advance"] = dict(two_level_iteration_us=two, one_size_mean_iteration_us=one, difference_us=two - one,
                                         note="10 fixed iterations at 1.0 then 10 at 0.5 against the mean of 20 at either size alone; the poses, hence "
                                              "the pair counts, are not the same along the two")
    # the tables: every level is rebuilt by the first call that needs them after the schedule changed
    q = np.ascontiguousarray(sc["scan"][:1], dtype=np.float32)
    for s in SCHEDULES:
        icp = checked[name_of(s)]
        ms = []
        for _ in range(a.rounds):
            icp.setVoxelSchedule([v * 1.25 for v in s])
            icp.voxelLookup(q)
            icp.setVoxelSchedule(list(s))
            t0 = time.perf_counter()
            icp.voxelLookup(q)
            ms.append((time.perf_counter() - t0) * 1e3)
        voxels = [int(icp.voxelMap(l)[0].shape[0]) for l in range(len(s))]
        caps = [max(2, 1 << int(np.ceil(np.log2(2 * v)))) for v in voxels]
        res["tables"][name_of(s)] = dict(build_all_levels_ms=med(ms), voxels=voxels, table_bytes=[64 * c for c in caps], table_bytes_total=64 * sum(caps))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
