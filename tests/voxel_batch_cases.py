"""The cases shared by tests/test_voxel_batch_cpu.py and tests/test_gpu_voxel_batch.py: the members of a voxel batch, the
handles they run on, the priors of a multistart, and ctypes access to the host shell's hooks
(norlab_icp_mapper_amd/host/TestHooksVoxelBatch.cpp).  Inputs: the analytic room scene of the voxel tests (8000-point map, 2000-point
reading) and voxel_pyramid_cases' xK starts.  Arrays are computed once; callers must not write into them."""
import ctypes as C

import numpy as np

import host_bindings as hb
import localizability_reference as lr
import voxel_pyramid_cases as pc
import voxel_pyramid_reference as vpr
import voxel_reference as vr

F = np.float32
# (points, start): prefixes of the reading moved by xK.  2000, 600, 257 and 1 points take 8, 3, 2 and 1 pair-sum workgroups
MEMBERS = ((2000, 1), (600, 3), (257, 6), (1, 1))
HANDLES = ((1.0,), (0.5,), (1.0, 0.5), (4.0, 2.0, 1.0, 0.5))
SCHEDULES = tuple(h for h in HANDLES if len(h) > 1)
FOUR = (4.0, 2.0, 1.0, 0.5)
SIXTEEN = tuple((2000, k) for k in (1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 1, 2, 3, 4))     # x1 .. x6 and their repeats
MULTISTART = (1, 3, 6, 0)                                                               # priors x1, x3, x6 and the identity
ACC_THREADS, ACC_CAP = 256, 256                                                         # csrc/loop.hip: acc_blocks


def acc_blocks(n):
    """the pair-sum workgroups a reading of n points uses (csrc/loop.hip: acc_blocks)"""
    return max(1, min(ACC_CAP, (n + ACC_THREADS - 1) // ACC_THREADS))


def member(n, k):
    """(reading (n, 4), normals (n, 3)): the first n points of the room reading moved by the xK start"""
    _, rd, rn, _ = pc.registration_inputs(k)
    return np.ascontiguousarray(rd[:n]), np.ascontiguousarray(rn[:n])


def members(spec=MEMBERS):
    return [member(n, k) for n, k in spec]


def far_member(n=300):
    """a reading 500 m from the map: no point falls into a voxel"""
    rd, rn = member(n, 1)
    rd = rd.copy()
    rd[:, 0] += F(500.0)
    return rd, rn


def prior(k):
    """the xK start as a map-frame pose (float32 4 x 4), as voxel_pyramid_cases.registration_inputs moves the reading; k = 0: the identity"""
    if k == 0:
        return np.eye(4, dtype=F)
    sc = lr.scene("room")
    M = np.eye(4)
    M[:3, 3] = vr.map_mean(sc["map"]).astype(np.float64)
    return (M @ pc.start_pose(k) @ np.linalg.inv(M)).astype(F)


def priors(ks=MULTISTART):
    return np.stack([prior(k) for k in ks])


def unmoved():
    sc = lr.scene("room")
    return np.ascontiguousarray(sc["reading"]), np.ascontiguousarray(sc["reading_normals"])


_runs = {}


def reference_member(n, k, sizes):
    """voxel_pyramid_reference.register in float32 on member (n, k): computed once per case"""
    key = (n, k, tuple(sizes))
    if key not in _runs:
        sc = lr.scene("room")
        rd, rn = member(n, k)
        _runs[key] = vpr.register(sc["map"], sc["normals"], rd, rn, sizes, 32)
    return _runs[key]


def levels_at(report, iteration):
    """the level a member is at during its `iteration`-th iteration (1-based) by its report [(iterations, first, last), ...]; None: it has stopped"""
    done = 0
    for level, (its, _, _) in enumerate(report):
        done += its
        if iteration <= done:
            return level
    return None


# ---- the host shell's hooks ------------------------------------------------------------------------------------------------------
def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _poses(cand):
    c = np.asarray(cand, F).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.transpose(c, (0, 2, 1))).reshape(-1), c.shape[0]


def host_voxel_batch(yaml_icp, mp, mn, readings, priors_=None):
    """GpuICPSequence::registerVoxelBatch(readings) or, with priors_, registerVoxelMultiStart(readings[0], priors_):
    dict(T (B, 4, 4), status, iterations, pairs, stats_iterations)"""
    fn = hb.load().nim_test_icp_voxel_batch
    fn.restype = C.c_int
    arr = lambda a: np.ascontiguousarray(a, dtype=F)
    mp, mn = arr(mp), arr(mn)
    pts = arr(np.concatenate([r for r, _ in readings]))
    nrm = arr(np.concatenate([n for _, n in readings]))
    counts = np.array([r.shape[0] for r, _ in readings], np.int64)
    p16, S = _poses(priors_) if priors_ is not None else (None, 0)
    B = S if priors_ is not None else len(readings)
    T, status, its, pairs = np.zeros(16 * B, F), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int64)
    last, err = C.c_int32(-1), C.create_string_buffer(512)
    rc = fn(yaml_icp.encode(), _ptr(mp), C.c_int64(mp.shape[0]), _ptr(mn), _ptr(pts), _ptr(nrm), _ptr(counts), C.c_int(len(readings)),
            None if p16 is None else _ptr(p16), C.c_int(S), _ptr(T), _ptr(status), _ptr(its), _ptr(pairs), C.byref(last), err, C.c_int(512))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(T=np.transpose(T.reshape(B, 4, 4), (0, 2, 1)).copy(), status=status.tolist(), iterations=its.tolist(), pairs=pairs.tolist(),
                stats_iterations=last.value)


def host_relocalize_voxel_counted(yaml_icp, mp, mn, scan, scan_normals, cand, refine=4, level=0, beta=1.0):
    """GpuICPSequence::relocalizeVoxel with the handle's call counters around it:
    dict(pose, score, index, calls: (batch loops, members in them, single voxel registrations), stats_iterations)"""
    from norlab_icp_mapper_amd import _capi
    fn = hb.load().nim_test_icp_relocalize_voxel_counted
    fn.restype = C.c_int
    arr = lambda a: np.ascontiguousarray(a, dtype=F)
    mp, mn, scan, sn = arr(mp), arr(mn), arr(scan), arr(scan_normals)
    c16, k = _poses(cand)
    pose, score, index = np.zeros(16, F), _capi.VoxelScore(), C.c_int32(-1)
    calls, last, err = np.zeros(3, np.int64), C.c_int32(-1), C.create_string_buffer(512)
    rc = fn(yaml_icp.encode(), _ptr(mp), C.c_int64(mp.shape[0]), _ptr(mn), _ptr(scan), C.c_int64(scan.shape[0]), _ptr(sn), _ptr(c16), C.c_int(k),
            C.c_int(refine), C.c_int(level), C.c_float(beta), _ptr(pose), C.byref(score), C.byref(index), _ptr(calls), C.byref(last), err, C.c_int(512))
    if rc:
        raise RuntimeError(("ConvergenceError: " if rc == 2 else "") + err.value.decode(errors="replace"))
    return dict(pose=pose.reshape(4, 4).T.copy(), score=score, index=index.value, calls=tuple(int(c) for c in calls), stats_iterations=last.value)
