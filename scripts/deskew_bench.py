"""Sweep deskewing (icpmi_deskew / icpmi_deskew_dev): call times at 100 k and 1 M points against one host thread doing the same arithmetic.

    python scripts/deskew_bench.py [--reps 50] [--warmup 5] [--out profiles/deskew_bench.json]

Per size, alternating so that the three share whatever else the machine is doing:
  host_call_ms   icpmi_deskew with host pointers: table preparation, upload of the points and their times, the kernel, the wait for the
                 error flag, download -- wall time of the call (it returns after a stream synchronisation)
  dev_call_ms    icpmi_deskew_dev in place on a cloud that is already in HBM: table preparation and upload, the kernel, the wait for the
                 error flag (the call returns after it) -- what a scan that arrives in HBM pays before icpmi_register_prior_dev
  host_loop_ms   one host thread, float32, the same arithmetic from the same table (TestHooks.cpp: nim_test_deskew_host_loop)
A motion of 21 poses at up to 3 rad/s and 30 m/s, ranges 0.5 - 120 m, times nearly ordered (tests/deskew_reference.py).  The device's
largest |out - float64| / (|x| + |p|) over the cloud is recorded next to the bound the tests use.  Nothing here is gated; not part of
bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [("synth100k", 100_000), ("synth1M", 1_000_000)]


def stats(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), p90=float(np.percentile(ts, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import norlab_icp_mapper_amd as amd
    import deskew_reference as dr
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    icp = amd.ICPSequence()
    host = C.CDLL(os.path.join(ROOT, "norlab_icp_mapper_amd", "libnorlab_icp_mapper_host.so"))
    stamps, poses = dr.make_motion(21, 5)
    rows = []
    for name, n in SIZES:
        pts, _, t = dr.make_points(n, n)
        m, keep = icp._sweepMotion(stamps, poses, 0.05, 1e-9, 0.0, False)
        d_pts = torch.from_numpy(pts).cuda()
        d_t = torch.from_numpy(t).cuda()
        torch.cuda.synchronize()
        out_loop = np.empty_like(pts)
        err = C.create_string_buffer(256)

        def host_call():
            return icp.deskew(pts, t, stamps, poses, ref=0.05)

        def dev_call():
            icp.deskewDev(d_pts.data_ptr(), n, d_t.data_ptr(), stamps, poses, ref=0.05)     # (in place, again and again: the time does not depend on the values)

        def host_loop():
            rc = host.nim_test_deskew_host_loop(C.c_void_p(pts.ctypes.data), C.c_int64(n), C.c_void_p(t.ctypes.data), C.byref(m),
                                                C.c_void_p(out_loop.ctypes.data), err, 256)
            assert rc == 0, err.value
        calls = dict(host_call_ms=host_call, dev_call_ms=dev_call, host_loop_ms=host_loop)
        ts = {k: [] for k in calls}
        for i in range(a.warmup + a.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    ts[k].append(dt)
        out = host_call()
        out64, _, pn = dr.deskew64(pts, t, stamps, poses, ref=0.05)
        den = np.linalg.norm(pts[:, :3].astype(np.float64), axis=1) + pn
        r = dict(case=name, n=n, poses=21, reps=a.reps, bytes_moved_by_the_kernel=n * (16 + 4 + 16),
                 device_rel_error=float((np.linalg.norm(out[:, :3] - out64, axis=1) / den).max()),
                 host_loop_rel_error=float((np.linalg.norm(out_loop[:, :3] - out64, axis=1) / den).max()),
                 test_bound=dr.device_bound(), **{k: stats(v) for k, v in ts.items()})
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
