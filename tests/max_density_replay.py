"""Child process of tests/test_gpu_max_density.py (c): replays scans through the C++ Mapper (host/TestHooks.cpp:
nim_test_mapper_replay_map) and saves the poses, the final map with every descriptor, and the update counters.  NIM_RESIDENT_MAP_UPDATE
is read once per process, so each setting needs a process of its own.

    python max_density_replay.py <dataset dir> <config.yaml> <n scans> <out.npz>
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def replay(data_dir, cfg, n_scans):
    import host_bindings as hb
    from config4_data import quat_T
    lib = hb.load()
    names = [ln.strip() for ln in open(os.path.join(data_dir, "names.txt")) if ln.strip()][:n_scans]
    traj = np.load(os.path.join(data_dir, "trajectory.npy"))[:n_scans]
    paths = [os.path.join(data_dir, "scans", nm) for nm in names]
    n = len(paths)
    poses = np.stack([quat_T(r[2:]).T.ravel() for r in traj]).astype(np.float32)     # column-major
    stamps = np.array([int(r[0]) * 1_000_000_000 + int(r[1]) for r in traj], np.int64)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    cap, rows = 400_000, 16
    out = np.zeros((n, 16), np.float32); pts = np.empty((cap, 4), np.float32); desc = np.empty(rows * cap, np.float32)
    names_out = C.create_string_buffer(1024); err = C.create_string_buffer(1024)
    m = C.c_int64(0); upd = C.c_int64(0); res = C.c_int64(0)
    fn = lib.nim_test_mapper_replay_map
    fn.restype = C.c_int
    rc = fn(cfg.encode(), C.c_int(n), arr, C.c_void_p(poses.ctypes.data), C.c_void_p(stamps.ctypes.data), C.c_void_p(out.ctypes.data),
            C.c_void_p(pts.ctypes.data), C.c_int64(cap), C.c_void_p(desc.ctypes.data), C.c_int(rows), names_out, C.c_int(1024),
            C.byref(m), C.byref(upd), C.byref(res), err, C.c_int(1024))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    k = m.value
    result = {"poses": out, "points": pts[:k].copy(), "map_updates": np.int64(upd.value), "resident_updates": np.int64(res.value)}
    at = 0
    for item in names_out.value.decode().split(";"):
        if not item:
            continue
        name, span = item.split(":")
        span = int(span)
        result["desc_" + name] = desc[at * k:(at + span) * k].reshape(k, span).copy()    # (span x k) column-major = (k, span) row-major
        at += span
    return result


if __name__ == "__main__":
    r = replay(sys.argv[1], sys.argv[2], int(sys.argv[3]))
    np.savez(sys.argv[4], **r)
