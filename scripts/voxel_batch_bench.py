"""Many readings, or many starts, in one loop on the voxel path at the headline shape (100 k x 1 M): what the batch saves
against the single calls it replaces, and what that makes of a voxel relocalisation.

    python scripts/voxel_batch_bench.py [--rounds 15] [--warmup 3] [--out profiles/voxel_batch_bench.json]

The scene and the start are scripts/voxel_pyramid_bench.py's: synth.make_scene with the ground-truth translation stretched to 1.0 m.  Two
handles, sizes (0.5) and (4.0, 2.0, 1.0, 0.5), both on CounterTransformationChecker 40 + the Differential checker.  The starts of a
multistart are the identity and offsets of it (up to 0.18 m and 0.02 rad, each its own); the record has the iterations every one of the
sixteen takes, since a batch runs as long as its slowest member.  Per handle, host clock around the whole call, medians over the rounds;
the routes take turns round after round:
  multistart_host    icpmi_voxel_register_multistart of S = 1, 4, 16 starts            against  S x (icpmi_transform + icpmi_register): the
                                                                                                 refinement of relocalizeVoxel before the batch
  multistart_dev     icpmi_voxel_register_multistart_dev                               against  S x icpmi_register_dev on readings already moved in HBM
  batch_dev          icpmi_voxel_register_batch_dev of B = 8, 16 different readings    against  B x icpmi_register_dev
  relocalize         relocalizeVoxel of 512 candidates, refine 4 and 16                against  the same call with the refinement made start after
                                                                                                 start (the code of the parent commit, on this build:
                                                                                                 the entry points it calls are unchanged)
Every pair of routes is checked to return the same bits before it is timed.  Nothing is compared against a threshold."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SCHEDULES = ((0.5,), (4.0, 2.0, 1.0, 0.5))
START_OFF = 1.0
CHECKED = dict(max_iterations=40, use_differential=1)
STARTS = (1, 4, 16)
BATCHES = (8, 16)
REFINE = (4, 16)
SOFT = (3, 4, 5, 6)


def name_of(sizes):
    return "voxel_" + "_".join(str(s) for s in sizes)


def offset(i):
    """start i: the identity, then small offsets of it, each its own"""
    T = np.eye(4, dtype=np.float64)
    if i:
        a = 0.01 * ((i % 5) - 2)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = (0.12 * ((i % 4) - 1.5), 0.08 * ((i % 3) - 1), 0.04 * (i % 2))
    return T.astype(np.float32)


def relocalize_start_after_start(amd, icp, scan, nrm, cand, refine):
    """ICPSequence.relocalizeVoxel as the parent commit has it: transform + icpmi_register per refined candidate"""
    from norlab_icp_mapper_amd import icp as I
    n = scan.shape[0]
    scores = icp.voxelScores(scan, nrm, cand, level=0)
    best = amd.rank_voxel_candidates(scores, n, 0.0)[:max(1, refine)]
    refined, status = [], []
    for i in best:
        moved, movedn = icp.transform(cand[i], scan, nrm)
        T = (C.c_float * 16)()
        st = icp._lib.icpmi_register(icp._h, moved.ctypes.data, n, movedn.ctypes.data, T, C.byref(icp.stats))
        if st in SOFT:
            refined.append(cand[i].copy()); status.append(int(st))
            continue
        icp._check(st)
        refined.append(I.compose_pose(np.array(T[:], np.float32).reshape(4, 4).T, cand[i])); status.append(0)
    refined = np.stack(refined)
    again = icp.voxelScores(scan, nrm, refined, level=None)
    again.status = [a if s == 0 else s for a, s in zip(again.status, status)]
    w = amd.rank_voxel_candidates(again, n, 0.0)[0]
    return refined[w], best[w]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_batch_bench.json"))
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    trans = np.asarray(amd.synth.T_GT_TRANS, np.float64)
    sc = amd.synth.make_scene(m=1_000_000, n=100_000, trans=tuple(trans / np.linalg.norm(trans) * START_OFF))
    scan, nrm = np.ascontiguousarray(sc["scan"], np.float32), np.ascontiguousarray(sc["scan_normals"], np.float32)
    n = scan.shape[0]
    d, dn = torch.from_numpy(scan).cuda(), torch.from_numpy(nrm).cuda()
    icps = {name_of(s): amd.ICPSequence(knn=1, max_dist=2.0, outliers=[], minimizer=3, voxel_sizes=list(s), **CHECKED) for s in SCHEDULES}
    for icp in icps.values():
        assert icp.setMap(sc["map"], sc["normals"])
    smax = max(STARTS + BATCHES)
    priors = np.stack([offset(i) for i in range(smax)])
    any_icp = next(iter(icps.values()))
    moved = [any_icp.transform(priors[i], scan, nrm) for i in range(smax)]               # the readings of a batch: the scan moved by every prior
    dmoved = [(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()) for p, q in moved]
    # 512 candidates around the truth: 8 x 8 x 8 offsets in x, y and yaw of the ground-truth correction
    T_gt = np.asarray(sc["T_gt"], np.float64)
    cand = []
    for yaw in np.linspace(-0.14, 0.14, 8):
        for dy in np.linspace(-1.75, 1.75, 8):
            for dx in np.linspace(-1.75, 1.75, 8):
                G = np.eye(4)
                G[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
                G[:2, 3] = (dx, dy)
                cand.append((G @ T_gt).astype(np.float32))
    cand = np.stack(cand)

    bits = lambda Ts: [np.ascontiguousarray(T, np.float32).view(np.uint32).tolist() for T in Ts]

    def singles_host(icp, S):
        out = []
        for i in range(S):
            p, q = icp.transform(priors[i], scan, nrm)
            T = (C.c_float * 16)()
            st = icp._lib.icpmi_register(icp._h, p.ctypes.data, n, q.ctypes.data, T, C.byref(icp.stats))
            out.append(np.array(T[:], np.float32).reshape(4, 4).T if st == 0 else np.eye(4, dtype=np.float32))
        return out

    def singles_dev(icp, S):
        out = []
        for i in range(S):
            T = (C.c_float * 16)()
            st = icp._lib.icpmi_register_dev(icp._h, dmoved[i][0].data_ptr(), n, dmoved[i][1].data_ptr(), T, C.byref(icp.stats))
            out.append(np.array(T[:], np.float32).reshape(4, 4).T if st == 0 else np.eye(4, dtype=np.float32))
        return out

    routes = {}
    for key, icp in icps.items():
        for S in STARTS:
            routes[(key, "multistart_host", S)] = (lambda icp=icp, S=S: icp.voxelRegisterMultiStart(scan, nrm, priors[:S])[0],
                                                   lambda icp=icp, S=S: singles_host(icp, S))
            routes[(key, "multistart_dev", S)] = (lambda icp=icp, S=S: icp.voxelRegisterMultiStartDev(d.data_ptr(), n, dn.data_ptr(), priors[:S])[0],
                                                  lambda icp=icp, S=S: singles_dev(icp, S))
        for B in BATCHES:
            routes[(key, "batch_dev", B)] = (lambda icp=icp, B=B: icp.voxelRegisterBatchDev([t[0].data_ptr() for t in dmoved[:B]], [n] * B,
                                                                                              [t[1].data_ptr() for t in dmoved[:B]])[0],
                                             lambda icp=icp, B=B: singles_dev(icp, B))
        for R in REFINE:
            routes[(key, "relocalize", R)] = (lambda icp=icp, R=R: [icp.relocalizeVoxel(scan, nrm, cand, refine=R).pose],
                                              lambda icp=icp, R=R: [relocalize_start_after_start(amd, icp, scan, nrm, cand, R)[0]])
    same = {}
    for k, (new, old) in routes.items():
        same[k] = bits(new()) == bits(old())
        assert same[k], k
    times = {k: ([], []) for k in routes}
    for r in range(a.warmup + a.rounds):
        for k, (new, old) in routes.items():
            order = ((0, new), (1, old)) if r % 2 == 0 else ((1, old), (0, new))
            for which, fn in order:
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if r >= a.warmup:
                    times[k][which].append((t1 - t0) * 1e3)
    its = {}
    for key, icp in icps.items():
        _, sts, status = icp.voxelRegisterMultiStartDev(d.data_ptr(), n, dn.data_ptr(), priors[:16])
        its[key] = dict(iterations=[int(s.iterations) for s in sts], status=status, batch_loop_ms=float(sts[0].loop_ms))
    med = lambda v: float(np.median(v))
    res = dict(shape="100k x 1M; start 1.0 m off plus the scene's rotation; Counter 40 + Differential(1e-3, 1e-3, 3); host clock around the whole call, ms",
               rounds=a.rounds, routes={}, sixteen_starts=its)
    for (key, what, count), (tn, to) in times.items():
        res["routes"].setdefault(key, {}).setdefault(what, {})[str(count)] = dict(
            one_loop_ms=med(tn), single_calls_ms=med(to), ratio=med(to) / med(tn), one_loop_p10_p90=[float(np.percentile(tn, 10)), float(np.percentile(tn, 90))],
            single_calls_p10_p90=[float(np.percentile(to, 10)), float(np.percentile(to, 90))], same_bits=bool(same[(key, what, count)]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
