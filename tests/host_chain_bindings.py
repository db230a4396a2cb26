"""ctypes access to the host shell's multi-descriptor test hooks (norlab_icp_mapper_amd/host/TestHooks.cpp): a filter chain on a cloud with
any number of descriptors, every descriptor of the result handed back in the container's order; and one GpuICPSequence registration."""
import ctypes as C

import numpy as np

import host_bindings as hb
from norlab_icp_mapper_amd import _capi

F = np.float32


def filter_chain_descs(yaml_seq, cloud, descs=None, handle=None, rows_cap=32):
    """yaml_seq on cloud ((n, 4) float32) carrying descs = [(name, (n, span) or (n,) array), ...].  Returns (cloud_out, [(name, array)]) with
    the descriptors in the order the container holds them, each (m, span)."""
    lib = hb.load()
    fn = lib.nim_test_filter_chain_descs
    fn.restype = C.c_int
    c = np.ascontiguousarray(cloud, dtype=F); n = c.shape[0]
    descs = list(descs or [])
    arrs = [np.ascontiguousarray(a, dtype=F).reshape(n, -1) for _, a in descs]
    k = len(descs)
    names = (C.c_char_p * max(k, 1))(*[nm.encode() for nm, _ in descs])
    spans = (C.c_int * max(k, 1))(*[a.shape[1] for a in arrs])
    data = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in arrs])
    out = np.empty_like(c); dout = np.empty(rows_cap * max(n, 1), F)
    onames = C.create_string_buffer(1024); m = C.c_int64(0); err = C.create_string_buffer(512)
    rc = fn(C.c_void_p(handle), yaml_seq.encode(), C.c_void_p(c.ctypes.data), C.c_int64(n), C.c_int(k), names, spans, data, C.c_void_p(out.ctypes.data),
            C.c_void_p(dout.ctypes.data), C.c_int(rows_cap), onames, C.c_int(1024), C.byref(m), err, C.c_int(512))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    mm = m.value
    res, row = [], 0
    for item in onames.value.decode().split(";"):
        if not item:
            continue
        nm, span = item.rsplit(":", 1)
        span = int(span)
        res.append((nm, dout[row * mm:(row + span) * mm].reshape(mm, span).copy()))
        row += span
    return out[:mm].copy(), res


def icp_register(yaml_icp, map4, map_normals, scan4, scan_normals=None, noise=None):
    """GpuICPSequence: loadFromYamlNode, setMap, operator(); noise (n,) goes to icpmi_set_reading_sensor_noise first.  Returns (T (4, 4), Stats)."""
    lib = hb.load()
    fn = lib.nim_test_icp_register
    fn.restype = C.c_int
    mp = np.ascontiguousarray(map4, dtype=F); sc = np.ascontiguousarray(scan4, dtype=F)
    ptr = lambda a: C.c_void_p(None if a is None else a.ctypes.data)
    mn = None if map_normals is None else np.ascontiguousarray(map_normals, dtype=F)
    sn = None if scan_normals is None else np.ascontiguousarray(scan_normals, dtype=F)
    nz = None if noise is None else np.ascontiguousarray(noise, dtype=F)
    T = np.zeros(16, F); stats = _capi.Stats(); err = C.create_string_buffer(512)
    rc = fn(yaml_icp.encode(), ptr(mp), C.c_int64(mp.shape[0]), ptr(mn), ptr(sc), C.c_int64(sc.shape[0]), ptr(sn), ptr(nz), ptr(T), C.byref(stats), err,
            C.c_int(512))
    if rc:
        raise RuntimeError(err.value.decode(errors="replace"))
    return T.reshape(4, 4).T.copy(), stats
