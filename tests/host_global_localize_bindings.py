"""ctypes access to the host shell's test hooks of the global localisation (norlab_icp_mapper_amd/host/TestHooksGlobalLocalize.cpp)."""
import ctypes as C

import numpy as np

import host_bindings as hb

F = np.float32


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _r9(rotations):
    R = np.asarray(rotations, F).reshape(-1, 3, 3)
    return np.ascontiguousarray(np.transpose(R, (0, 2, 1))).reshape(-1), R.shape[0]


def _box(box):
    return None if box is None else np.ascontiguousarray(np.concatenate([np.asarray(b, np.float64).reshape(3) for b in box]))


def yaw_rotations(steps, roll=0.0, pitch=0.0):
    """nim::yawRotations: (steps, 3, 3) float32"""
    fn = hb.load().nim_test_yaw_rotations
    fn.restype = C.c_int
    out, err = np.zeros(9 * max(steps, 1), F), C.create_string_buffer(512)
    if fn(C.c_int(steps), C.c_double(roll), C.c_double(pitch), _ptr(out), err, C.c_int(512)):
        raise RuntimeError(err.value.decode(errors="replace"))
    return np.transpose(out[:9 * steps].reshape(-1, 3, 3), (0, 2, 1)).copy()


def icp_global_localize(yaml_icp, mp, mn, scan, scan_normals, rotations, cell, levels=0, ratio=0.0, max_nodes=0, batch=64, box=None, refine=False):
    """GpuICPSequence::globalLocalize (refine False) or relocalizeGlobal with one refined candidate: dict(result, pose (4, 4), residual,
    score, voxel)"""
    from norlab_icp_mapper_amd import _capi
    fn = hb.load().nim_test_icp_global_localize
    fn.restype = C.c_int
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F)
    mp, mn, scan, sn = arr(mp), arr(mn), arr(scan), arr(scan_normals)
    r9, k = _r9(rotations)
    b6 = _box(box)
    res, pose, resid, score, voxel = _capi.GlobalLocalizeResult(), np.zeros(16, F), _capi.Residual(), _capi.VoxelScore(), C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = fn(yaml_icp.encode(), _ptr(mp), C.c_int64(mp.shape[0]), _ptr(mn), _ptr(scan), C.c_int64(scan.shape[0]), _ptr(sn), _ptr(r9), C.c_int(k),
            C.c_float(cell), C.c_int(levels), C.c_float(ratio), C.c_int64(max_nodes), C.c_int(batch), _ptr(b6), C.c_int(1 if refine else 0),
            C.byref(res), _ptr(pose), C.byref(resid), C.byref(score), C.byref(voxel), err, C.c_int(512))
    if rc:
        raise RuntimeError(("ConvergenceError: " if rc == 2 else "") + err.value.decode(errors="replace"))
    return dict(result=res, pose=pose.reshape(4, 4).T.copy(), residual=resid, score=score, voxel=bool(voxel.value))


def mapper_relocalize_global(config_path, mp, mn, scan, scan_normals, rotations, cell, levels=0, box=None):
    """Mapper::relocalizeGlobal: dict(result, pose, get_pose, map_before, map_after)"""
    from norlab_icp_mapper_amd import _capi
    fn = hb.load().nim_test_mapper_relocalize_global
    fn.restype = C.c_int
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F)
    mp, mn, scan, sn = arr(mp), arr(mn), arr(scan), arr(scan_normals)
    r9, k = _r9(rotations)
    b6 = _box(box)
    res, pose, get_pose = _capi.GlobalLocalizeResult(), np.zeros(16, F), np.zeros(16, F)
    before, after, err = C.c_int64(0), C.c_int64(0), C.create_string_buffer(512)
    rc = fn(config_path.encode(), _ptr(mp), C.c_int64(mp.shape[0]), _ptr(mn), _ptr(scan), C.c_int64(scan.shape[0]), _ptr(sn), _ptr(r9), C.c_int(k),
            C.c_float(cell), C.c_int(levels), _ptr(b6), C.byref(res), _ptr(pose), _ptr(get_pose), C.byref(before), C.byref(after), err, C.c_int(512))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(result=res, pose=pose.reshape(4, 4).T.copy(), get_pose=get_pose.reshape(4, 4).T.copy(), map_before=before.value, map_after=after.value)
