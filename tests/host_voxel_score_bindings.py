"""ctypes access to the host shell's test hooks of the voxel pose score (norlab_icp_mapper_amd/host/TestHooksVoxelScore.cpp)."""
import ctypes as C

import numpy as np

import host_bindings as hb

F = np.float32


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _poses(cand):
    c = np.asarray(cand, F).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.transpose(c, (0, 2, 1))).reshape(-1), c.shape[0]


def rank(rows, n, min_pairs_ratio=0.0):
    """nim::rankVoxelCandidates over (status, pairs, likelihood) rows: the list of indices"""
    fn = hb.load().nim_test_rank_voxel_candidates
    fn.restype = C.c_int
    k = len(rows)
    st = np.array([r[0] for r in rows], np.int32)
    pairs = np.array([r[1] for r in rows], np.int64)
    lik = np.array([r[2] for r in rows], np.float64)
    order = np.zeros(max(k, 1), np.int32)
    got = fn(_ptr(st), _ptr(pairs), _ptr(lik), C.c_int(k), C.c_int64(int(n)), C.c_float(min_pairs_ratio), _ptr(order))
    return order[:got].tolist()


def icp_relocalize_voxel(yaml_icp, mp, mn, scan, scan_normals, cand, refine=4, level=0, beta=1.0, min_pairs_ratio=0.0):
    """GpuICPSequence::relocalizeVoxel (refine >= 0) or voxelScores alone (refine < 0): dict(pose (4, 4), score, index, scores, status)"""
    from norlab_icp_mapper_amd import _capi
    fn = hb.load().nim_test_icp_relocalize_voxel
    fn.restype = C.c_int
    arr = lambda a: np.ascontiguousarray(a, dtype=F)
    mp, mn, scan, sn = arr(mp), arr(mn), arr(scan), arr(scan_normals)
    c16, k = _poses(cand)
    pose, score, index = np.zeros(16, F), _capi.VoxelScore(), C.c_int32(-1)
    scores, status, err = (_capi.VoxelScore * k)(), (C.c_int32 * k)(), C.create_string_buffer(512)
    rc = fn(yaml_icp.encode(), _ptr(mp), C.c_int64(mp.shape[0]), _ptr(mn), _ptr(scan), C.c_int64(scan.shape[0]), _ptr(sn), _ptr(c16), C.c_int(k),
            C.c_int(refine), C.c_int(level), C.c_float(beta), C.c_float(min_pairs_ratio), _ptr(pose), C.byref(score), C.byref(index), scores, status,
            err, C.c_int(512))
    if rc:
        raise RuntimeError(("ConvergenceError: " if rc == 2 else "") + err.value.decode(errors="replace"))
    return dict(pose=pose.reshape(4, 4).T.copy(), score=score, index=index.value, scores=list(scores), status=list(status))


def mapper_relocalize_voxel(config_path, mp, mn, scan, scan_normals, cand):
    """Mapper::relocalizeVoxel: dict(pose, get_pose, index, map_before, map_after)"""
    fn = hb.load().nim_test_mapper_relocalize_voxel
    fn.restype = C.c_int
    arr = lambda a: np.ascontiguousarray(a, dtype=F)
    mp, mn, scan, sn = arr(mp), arr(mn), arr(scan), arr(scan_normals)
    c16, k = _poses(cand)
    pose, get_pose, index = np.zeros(16, F), np.zeros(16, F), C.c_int32(-1)
    before, after, err = C.c_int64(0), C.c_int64(0), C.create_string_buffer(512)
    rc = fn(config_path.encode(), _ptr(mp), C.c_int64(mp.shape[0]), _ptr(mn), _ptr(scan), C.c_int64(scan.shape[0]), _ptr(sn), _ptr(c16), C.c_int(k),
            _ptr(pose), _ptr(get_pose), C.byref(index), C.byref(before), C.byref(after), err, C.c_int(512))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(pose=pose.reshape(4, 4).T.copy(), get_pose=get_pose.reshape(4, 4).T.copy(), index=index.value, map_before=before.value,
                map_after=after.value)
