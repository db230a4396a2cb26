"""Child process of tests/test_gpu_residual.py (host shell): replays scans through the C++ Mapper with Mapper::setScoreRegistrations
(host/TestHooks.cpp: nim_test_mapper_replay_scored) and saves poses and residuals.  NIM_RESIDENT_MAP_UPDATE is read once per process, so
the one-upload path and the host path each need a process of their own.

    python residual_replay.py <dataset dir> <config.yaml> <n scans> <out.npz>
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def replay(lib, data_dir, cfg, n_scans, score, freeze, by_hand):
    from config4_data import quat_T
    from norlab_icp_mapper_amd import _capi
    names = [ln.strip() for ln in open(os.path.join(data_dir, "names.txt")) if ln.strip()][:n_scans]
    traj = np.load(os.path.join(data_dir, "trajectory.npy"))[:n_scans]
    paths = [os.path.join(data_dir, "scans", nm) for nm in names]
    n = len(paths)
    poses = np.stack([quat_T(r[2:]).T.ravel() for r in traj]).astype(np.float32)     # column-major
    stamps = np.array([int(r[0]) * 1_000_000_000 + int(r[1]) for r in traj], np.int64)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    out = np.zeros((n, 16), np.float32); valid = np.zeros(n, np.int32); err = C.create_string_buffer(1024)
    res = (_capi.Residual * n)(); hand = (_capi.Residual * n)()
    fn = lib.nim_test_mapper_replay_scored
    fn.restype = C.c_int
    rc = fn(cfg.encode(), C.c_int(n), arr, C.c_void_p(poses.ctypes.data), C.c_void_p(stamps.ctypes.data), C.c_int(score), C.c_int(freeze),
            C.c_void_p(out.ctypes.data), res, C.c_void_p(valid.ctypes.data), hand if by_hand else None, err, C.c_int(1024))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    raw = lambda a: np.frombuffer(bytes(a), np.uint8).reshape(n, C.sizeof(_capi.Residual)).copy()
    return out, valid, raw(res), raw(hand)


if __name__ == "__main__":
    import host_bindings as hb
    lib = hb.load()
    data_dir, cfg, n_scans, dst = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    r = {}
    for name, score, freeze, by_hand in (("on", 1, 0, False), ("off", 0, 0, False), ("frozen", 1, 1, True)):
        poses, valid, res, hand = replay(lib, data_dir, cfg, n_scans, score, freeze, by_hand)
        r.update({name + "_poses": poses, name + "_valid": valid, name + "_res": res, name + "_hand": hand})
    np.savez(dst, **r)
