"""ctypes access to the host shell's deskewing hook (norlab_icp_mapper_amd/host/TestHooks.cpp: nim_test_deskew), which runs
nim::deskewSweep -- the body of Mapper::deskew -- on a given icpmi handle."""
import ctypes as C
import os

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(_ROOT, "norlab_icp_mapper_amd", "libnorlab_icp_mapper_host.so")
_lib = None


class InvalidField(RuntimeError):
    """the hook caught nim::InvalidField"""


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIB)
        _lib.nim_test_deskew.restype = C.c_int
    return _lib


def deskew(handle, cloud, descriptors, stamps_ns, poses, stamp_ns=0, times=None, time_name="t", time_field="t", time_unit=1e-9, round_to_ns=0,
           extrapolate=False):
    """cloud (n, 4) float32; descriptors {name: (n,) or (n, span) array}; times: (n,) int64 absolute nanoseconds stored as the time
    row `time_name`, or None; stamps_ns (K,) int64 and poses (K, 7) the motion; stamp_ns the scan's stamp.
    Returns (cloud_out, {name: array} of every descriptor afterwards, the time row afterwards or None)."""
    lib = load()
    c = np.ascontiguousarray(cloud, dtype=np.float32); n = c.shape[0]
    names = list(descriptors)
    arrs = [np.ascontiguousarray(np.asarray(descriptors[k], dtype=np.float32).reshape(n, -1)) for k in names]
    spans = (C.c_int * max(1, len(names)))(*[a.shape[1] for a in arrs])
    cnames = (C.c_char_p * max(1, len(names)))(*[k.encode() for k in names])
    cdata = (C.c_void_p * max(1, len(names)))(*[a.ctypes.data for a in arrs])
    rows = sum(a.shape[1] for a in arrs)
    tin = None if times is None else np.ascontiguousarray(times, dtype=np.int64)
    tout = None if times is None else np.empty(n, np.int64)
    s = np.ascontiguousarray(stamps_ns, dtype=np.int64); p = np.ascontiguousarray(poses, dtype=np.float64)
    out = np.empty_like(c); dout = np.empty(max(1, rows) * max(1, n), np.float32)
    onames = C.create_string_buffer(1024); err = C.create_string_buffer(512)
    rc = lib.nim_test_deskew(C.c_void_p(handle), C.c_void_p(c.ctypes.data), C.c_int64(n), C.c_int(len(names)), cnames, spans, cdata,
                             time_name.encode(), C.c_void_p(None if tin is None else tin.ctypes.data), C.c_int(s.shape[0]), C.c_void_p(s.ctypes.data),
                             C.c_void_p(p.ctypes.data), C.c_int64(int(stamp_ns)), time_field.encode(), C.c_double(time_unit), C.c_int64(int(round_to_ns)),
                             C.c_int(1 if extrapolate else 0), C.c_void_p(out.ctypes.data), C.c_void_p(dout.ctypes.data), C.c_int(rows), onames, 1024,
                             C.c_void_p(None if tout is None else tout.ctypes.data), err, 512)
    if rc == 2:
        raise InvalidField(err.value.decode(errors="replace"))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    got, at = {}, 0
    for item in onames.value.decode().split(";"):
        if not item:
            continue
        name, span = item.rsplit(":", 1)
        span = int(span)
        got[name] = dout[at * n:(at + span) * n].reshape(n, span).copy()
        at += span
    return out, got, tout
