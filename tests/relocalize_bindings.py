"""ctypes access to the relocalisation hooks of the C++ host shell (norlab_icp_mapper_amd/host/TestHooksRelocalize.cpp)."""
import ctypes as C

import numpy as np

import host_bindings as hb

F = np.float32
_RC = {2: "ConvergenceError", 3: "InvalidField", 4: "InvalidParameter"}


def _cm(poses):
    """(P, 4, 4) row-major -> column-major float32, 16 per pose"""
    P = np.asarray(poses, F).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.transpose(P, (0, 2, 1))).reshape(-1)


def _rm(buf, count):
    return np.transpose(np.asarray(buf, F).reshape(count, 4, 4), (0, 2, 1)).copy()


def rank_candidates(table, n, ratio):
    """nim::rankCandidates over (status, pairs, sum_abs) rows"""
    fn = hb.load().nim_test_rank_candidates
    fn.restype = C.c_int
    k = len(table)
    st = (C.c_int32 * max(k, 1))(*[int(r[0]) for r in table])
    pr = (C.c_int64 * max(k, 1))(*[int(r[1]) for r in table])
    sa = (C.c_double * max(k, 1))(*[float(r[2]) for r in table])
    out = (C.c_int32 * max(k, 1))()
    cnt = fn(st, pr, sa, C.c_int(k), C.c_int64(n), C.c_float(ratio), out)
    return [int(out[i]) for i in range(cnt)]


def candidate_grid(centre, hx, hy, hyaw, sx, sy, syaw, cap=4096):
    """nim::candidateGrid: (N, 4, 4) float32"""
    fn = hb.load().nim_test_candidate_grid
    fn.restype = C.c_int
    c = _cm(centre)
    out = np.empty(16 * cap, F)
    cnt = fn(C.c_void_p(c.ctypes.data), C.c_float(hx), C.c_float(hy), C.c_float(hyaw), C.c_int(sx), C.c_int(sy), C.c_int(syaw),
             C.c_void_p(out.ctypes.data), C.c_int(cap))
    if cnt < 0:
        raise RuntimeError("candidateGrid failed")
    return _rm(out[:16 * cnt], cnt)


def icp_relocalize(yaml_icp, mp, normals, scan, cand, ratio=0.5, refine=4, kind=0, ms_index=None):
    """GpuICPSequence::relocalize on a fresh object.  Returns dict(pose, residual (_capi.Residual), index, scores, status, batched
    [, ms_T, ms_status: registerMultiStart of candidate ms_index alone])."""
    from norlab_icp_mapper_amd import _capi
    fn = hb.load().nim_test_icp_relocalize
    fn.restype = C.c_int
    mp = np.ascontiguousarray(mp, F); scan = np.ascontiguousarray(scan, F)
    nm = None if normals is None else np.ascontiguousarray(normals, F)
    c = _cm(cand); k = c.shape[0] // 16
    pose = np.empty(16, F); res = _capi.Residual(); idx = C.c_int32(-1)
    scores = (_capi.Residual * k)(); status = (C.c_int32 * k)(); batched = C.c_int32(0)
    msT = np.empty(16, F); ms_st = C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = fn(yaml_icp.encode(), C.c_void_p(mp.ctypes.data), C.c_int64(mp.shape[0]), C.c_void_p(None if nm is None else nm.ctypes.data),
            C.c_void_p(scan.ctypes.data), C.c_int64(scan.shape[0]), C.c_void_p(c.ctypes.data), C.c_int(k), C.c_float(ratio), C.c_int(refine),
            C.c_int(kind), C.c_void_p(pose.ctypes.data), C.byref(res), C.byref(idx), scores, status, C.byref(batched),
            C.c_int(0 if ms_index is None else ms_index), C.c_void_p(None if ms_index is None else msT.ctypes.data), C.byref(ms_st), err, C.c_int(512))
    if rc:
        raise RuntimeError(_RC.get(rc, "error") + ": " + err.value.decode(errors="replace"))
    out = dict(pose=_rm(pose, 1)[0], residual=res, index=idx.value, scores=[scores[i] for i in range(k)], status=[int(s) for s in status],
               batched=batched.value)
    if ms_index is not None:
        out["ms_T"] = _rm(msT, 1)[0]; out["ms_status"] = ms_st.value
    return out


def mapper_relocalize(config_path, mp, normals, scan, cand):
    """Mapper::relocalize on a fresh offline mapper holding `mp`: dict(pose, get_pose, index, map_before, map_after)"""
    fn = hb.load().nim_test_mapper_relocalize
    fn.restype = C.c_int
    mp = np.ascontiguousarray(mp, F); scan = np.ascontiguousarray(scan, F)
    nm = None if normals is None else np.ascontiguousarray(normals, F)
    c = _cm(cand); k = c.shape[0] // 16
    pose = np.empty(16, F); gp = np.empty(16, F); idx = C.c_int32(-1); before = C.c_int64(0); after = C.c_int64(0)
    err = C.create_string_buffer(512)
    rc = fn(config_path.encode(), C.c_void_p(mp.ctypes.data), C.c_int64(mp.shape[0]), C.c_void_p(None if nm is None else nm.ctypes.data),
            C.c_void_p(scan.ctypes.data), C.c_int64(scan.shape[0]), C.c_void_p(c.ctypes.data), C.c_int(k), C.c_void_p(pose.ctypes.data),
            C.c_void_p(gp.ctypes.data), C.byref(idx), C.byref(before), C.byref(after), err, C.c_int(512))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    return dict(pose=_rm(pose, 1)[0], get_pose=_rm(gp, 1)[0], index=idx.value, map_before=before.value, map_after=after.value)
