"""The relocalisation case of tests/test_gpu_residual_poses.py and its float64 reference (tests/test_residual_poses_cpu.py checks on the
CPU that the reference separates the true candidate in BOTH rankings of a relocalisation, so the GPU test cannot pass by luck).

Scene: tests/residual_reference.py's box + pillars (5 000 map points with normals, 1 000 scan points, +-10 m, pillars 4 m apart).  The scan
lines up with the map under a pose close to NEAR; the caller's guess is off by three metres in x and y and by 0.4 rad in yaw, and the
generator's grid around the guess (one step of exactly that size per axis: 27 candidates) holds NEAR again.
- First ranking: within maxDist 2 m most points of a wrong candidate still find a match, so its point-to-plane residual grows with its
  offset instead of its pairs going away.
- Second ranking: the steps are wider than the registration's basin around the truth.  The runners-up do not refine onto the true pose
  (they settle a pillar spacing away, or turned), so the refined poses do not coincide and the last ranking is not a matter of last bits.
  (Steps of half a metre put all four starts into one basin; steps of two metres leave the first ranking's runner-up within a factor of
  two.)"""
import numpy as np

import residual_reference as rr

F = np.float32
CHAIN = dict(minimizer=2, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=30, use_differential=1)
CHAIN_YAML = """
matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 2.0
    epsilon: 0
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.85
errorMinimizer:
  PointToPlaneErrorMinimizer:
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 30
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.001
      smoothLength: 3
"""
NEAR_RV, NEAR_T = (0.010, -0.015, 0.030), (0.13, -0.10, 0.05)      # the scene's T_gt is (0.010, -0.015, 0.020), (0.10, -0.08, 0.05)
HALF_X, HALF_Y, HALF_YAW = 3.0, 3.0, 0.4
STEPS = (1, 1, 1)
TRUE_INDEX = 7                                                      # ix = -1, iy = +1, iyaw = -1 in the generator's order
TRIM = 0.85


def near_pose():
    from norlab_icp_mapper_amd import synth
    return synth.make_T(NEAR_RV, NEAR_T).astype(F)


def guess_pose():
    """NEAR turned by +HALF_YAW about z and shifted by (+HALF_X, -HALF_Y): the grid's corner (-1, +1, -1) undoes it"""
    P = near_pose().astype(np.float64)
    c, s = np.cos(HALF_YAW), np.sin(HALF_YAW)
    G = P.copy()
    G[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ P[:3, :3]
    G[0, 3] += HALF_X; G[1, 3] -= HALF_Y
    return G.astype(F)


def candidates():
    from norlab_icp_mapper_amd.icp import candidate_grid
    return candidate_grid(guess_pose(), HALF_X, HALF_Y, HALF_YAW, *STEPS)


def exact_nn(moved, ref, max_dist):
    """float64 exact nearest neighbour of every row of `moved` among `ref`: (ids, d2), id -1 / d2 inf beyond max_dist.  The three best by
    the expanded form |a|^2 + |b|^2 - 2 a.b (one matrix product) are told apart by their exact squared distances."""
    approx = (moved * moved).sum(1)[:, None] + (ref * ref).sum(1)[None, :] - 2.0 * (moved @ ref.T)
    top = np.argpartition(approx, 3, axis=1)[:, :3]
    top.sort(axis=1)                                                   # ties go to the lower index, as argmin would
    exact = ((moved[:, None, :] - ref[top]) ** 2).sum(2)
    pick = exact.argmin(1)
    rows = np.arange(moved.shape[0])
    ids = top[rows, pick].astype(np.int64); d2 = exact[rows, pick]
    out = d2 > float(max_dist) ** 2
    ids[out] = -1; d2[out] = np.inf
    return ids, d2


def reference_table(sc=None, cand=None):
    """(status, pairs, sum_abs) per candidate from float64 exact neighbours: MaxDist matches, TrimmedDist keeps d2 <= the element of rank
    int(count * ratio) (getDistsQuantile), residuals by rr.residuals_f64"""
    sc = rr.scene() if sc is None else sc
    cand = candidates() if cand is None else cand
    mp, nm, reading = sc["map"], sc["normals"], sc["scan"]
    ref = mp[:, :3].astype(np.float64)
    table = []
    for T in cand:
        T64 = T.astype(np.float64)
        moved = reading[:, :3].astype(np.float64) @ T64[:3, :3].T + T64[:3, 3]
        ids, d2 = exact_nn(moved, ref, CHAIN["max_dist"])
        ok = np.nonzero((ids >= 0) & (d2 > 0))[0]
        if ok.size == 0:
            table.append((4, 0, 0.0)); continue
        srt = np.sort(d2[ok])
        limit = srt[min(int(F(ok.size) * F(TRIM)), ok.size - 1)]
        keep = ok[d2[ok] <= limit]
        r = rr.residuals_f64(2, reading[keep], T, mp[ids[keep]], nm[ids[keep]])
        table.append((0, int(keep.size), float(r.sum())))
    return table


def refined_reference(oracle, order, refine=4, sc=None, cand=None):
    """what the second half of a relocalisation sees, on the CPU: the best `refine` candidates of `order` registered by the float32 CPU
    oracle (the loop the device is held to elsewhere), the refined poses and their float64 (status, pairs, sum_abs) rows"""
    from norlab_icp_mapper_amd.icp import compose_pose
    sc = rr.scene() if sc is None else sc
    cand = candidates() if cand is None else cand
    oicp = oracle.OracleICP(oracle.make_config(nthreads=8, **CHAIN))
    oicp.setMap(sc["map"], sc["normals"])
    poses, status = [], []
    for i in order[:refine]:
        moved = sc["scan"].copy()
        moved[:, :3] = sc["scan"][:, :3] @ cand[i][:3, :3].T + cand[i][:3, 3]
        err, T = oicp(np.ascontiguousarray(moved, F))
        status.append(int(err))
        poses.append(compose_pose(np.asarray(T, F), cand[i]) if err == 0 else np.eye(4, dtype=F))
    table = reference_table(sc=sc, cand=np.stack(poses))
    table = [row if st == 0 else (st, 0, 0.0) for row, st in zip(table, status)]
    return poses, table
