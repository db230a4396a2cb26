"""Float64 reference and float32 restatement of the scheduled VoxelMatcher registration (include/icpmi.h: icpmi_set_voxel_schedule;
DESIGN.md 4.21), built on tests/voxel_reference.py.  Pure numpy: nothing here touches the library.

The specification, restated: level l pairs with the table of sizes[l] (voxel_reference.table: key rule, records and lookup are 4.20's),
sums and step are 4.20's.  Every level is an ICP run of its own on the chain's checkers: the Counter and the Differential checker's
history start afresh at each level.  The first level's history begins with the pose the registration starts from, as the checker's
init() leaves it; the history of every later level begins EMPTY -- the pose carried over is not an entry, the first step measured is the
one between the level's first two poses, and such a level runs at least smoothLength + 1 iterations (the issue's prototype: 4 at each
of the two fine levels).  A stop by either at a level before
the last moves on to the next level with the pose unchanged; at the last level it ends the registration.  A level that finds no pair ends
the registration ("no point to minimize").  A fixed iteration count (no Differential checker) runs that count at every level.
"""
import numpy as np

import localizability_reference as lr
import plane_to_plane_reference as pr
import symmetric_reference as sr
import voxel_reference as vr

F32 = np.float32


def differential_values(start, poses, smooth):
    """(mean rotation step, mean translation step) over the last `smooth` steps of [start] + poses (start None: of poses alone), or None
    while fewer steps exist: the two numbers DifferentialTransformationChecker compares with its thresholds after the last pose of `poses`"""
    hist = ([] if start is None else [np.asarray(start, np.float64)]) + [np.asarray(p, np.float64) for p in poses]
    if len(hist) - 1 < smooth:
        return None
    rot, tr = [], []
    for a, b in zip(hist[-smooth:], hist[-smooth - 1:-1]):
        rot.append(np.linalg.norm(lr.step_from_T(a @ np.linalg.inv(b))[:3]))
        tr.append(np.linalg.norm(a[:3, 3] - b[:3, 3]))
    return float(np.mean(rot)), float(np.mean(tr))


def register(map4, normals, reading4, read_normals, sizes, precision=64, max_iter=vr.MAX_ITER, differential=vr.DIFFERENTIAL, eps=pr.EPS_DEFAULT,
             mean=None):
    """The scheduled registration of a reading against a map from the identity.  precision 64: float64 tables, sums and solves on the float32
    clouds; 32: the float32 restatements of voxel_reference.register.  differential: the checker's parameters, or None for a fixed count of
    max_iter iterations per level.  Returns dict(T: the pose in the clouds' frame (float64 4 x 4); iterations: the total; status: "ok" or
    "no point to minimize"; levels: one dict per level ENTERED with iterations, pairs (per iteration), pairs_first, pairs_last, stop
    ("differential" | "counter" | "no point to minimize"), checks (per iteration the two numbers of differential_values, or None))."""
    assert precision in (32, 64)
    sizes = [float(s) for s in sizes]
    assert 1 <= len(sizes) <= 4 and all(b < a for a, b in zip(sizes, sizes[1:]))
    mean = vr.map_mean(map4) if mean is None else np.asarray(mean, F32)
    mc, rc = vr.centred(map4, mean), vr.centred(reading4, mean)
    rn = np.asarray(read_normals, F32)
    T = np.eye(4, dtype=F32 if precision == 32 else np.float64)
    levels, status, total = [], "ok", 0
    for level, size in enumerate(sizes):
        tab = vr.table(mc, normals, size)
        if precision == 32:
            tab = vr.table_f32(tab)
        start = np.array(T, np.float64) if level == 0 else None
        poses, pairs, checks, stop = [], [], [], None
        for _ in range(max_iter):
            if precision == 32:
                p, npr = pr.xf_points(T, rc), pr.rot_normals(T, rn)
            else:
                p = rc[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
                npr = rn.astype(np.float64) @ T[:3, :3].T
            vox = vr.lookup(tab, p.astype(F32))
            pairs.append(int((vox >= 0).sum()))
            if pairs[-1] == 0:
                stop = "no point to minimize"
                break
            if precision == 32:
                T = (sr._float32_step_T(vr.float32_sums(p, npr, vox, tab, eps)) @ T).astype(F32)
            else:
                x = pr.solve_step(vr.reference_sums(p, npr, vox, tab, eps))
                T = lr.make_T(x[:3], x[3:]) @ T
            poses.append(np.array(T, np.float64))
            chk = differential_values(start, poses, differential["smooth"]) if differential else None
            checks.append(chk)
            if chk is not None and chk[0] < differential["min_rot"] and chk[1] < differential["min_trans"]:
                stop = "differential"
                break
        if stop is None:
            stop = "counter"
        total += len(poses)
        levels.append(dict(size=size, iterations=len(poses), pairs=pairs, pairs_first=pairs[0], pairs_last=pairs[-1], stop=stop, checks=checks))
        if stop == "no point to minimize":
            status = stop
            break
    Tw = np.array(T, np.float64)
    m64 = mean.astype(np.float64)
    Tw[:3, 3] = Tw[:3, 3] + m64 - Tw[:3, :3] @ m64      # centred frame -> the clouds' frame
    return dict(T=Tw, iterations=total, status=status, levels=levels)


def report(res):
    """the registration's report as icpmi_get_voxel_schedule_report hands it out: (iterations, pairs_first, pairs_last) per level entered; a
    level that found no pair on its first iteration reports (0, 0, 0)"""
    return [(lv["iterations"], lv["pairs_first"], lv["pairs_last"]) for lv in res["levels"]]


def margins(res64, res32, differential=vr.DIFFERENTIAL):
    """The condition under which the iteration counts of two evaluations of one specification may be compared exactly.  For every check of
    the float64 loop, d = |float32's number - float64's number| at the same iteration of the same level.  The stopping check needs both
    numbers further below their thresholds than d; every other check needs one number that is over its threshold by more than its d.
    Returns (ok, worst): worst = the smallest (margin - d) / threshold met, over the numbers that carry a decision."""
    thr = (differential["min_rot"], differential["min_trans"])
    if len(res64["levels"]) != len(res32["levels"]):
        return False, -np.inf
    worst = np.inf
    for a, b in zip(res64["levels"], res32["levels"]):
        if a["iterations"] != b["iterations"]:
            return False, -np.inf
        for i, (ca, cb) in enumerate(zip(a["checks"], b["checks"])):
            if ca is None:
                continue
            d = [abs(cb[j] - ca[j]) for j in range(2)]
            stopping = a["stop"] == "differential" and i == a["iterations"] - 1
            if stopping:
                slack = min((thr[j] - ca[j] - d[j]) / thr[j] for j in range(2))
            else:
                slack = max((ca[j] - thr[j] - d[j]) / thr[j] for j in range(2))
            worst = min(worst, slack)
    return worst > 0, float(worst)
