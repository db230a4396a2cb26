#!/usr/bin/env python
"""Per-workgroup timeline of one steady nn1_wg_kernel launch of the headline registration (100 k x 1 M, point-to-point, 20 fixed iterations
replayed from one graph, as bench.py runs it).

Needs a timing library, built and loaded the way scripts/nn_phase.py's is: libicpmi.so compiled with -DICPMI_NN_TIMING in the package's place,
    make -C norlab_icp_mapper_amd/csrc clean all CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DICPMI_NN_TIMING -DICPMI_NN_TIMELINE_ONLY"
(-DICPMI_NN_TIMELINE_ONLY leaves the serialising phase clocks out, so that the workgroups run on the kernel's own schedule; without it the
timeline is that of the serialised kernel nn_phase.py measures).  Thread 0 of every workgroup stamps the 100 MHz constant clock at entry, behind
its last store and once the wave's stores have drained, and records its XCC and its piece count; the next kernel's first workgroup closes the
launch (nn_stamp_close).  Store-policy switches (-DICPMI_WT_MATCH=1 ...) go on the same command line.

usage: nn_wg_timeline.py [scan points = 100000] [launch = 10] [registrations = 5]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import norlab_icp_mapper_amd as pkg

TL_LAUNCHES, TL_WGS, TICK_US = 24, 2048, 0.01  # common.h: ICPMI_TL_LAUNCHES, nn.hip: NN_TL_WGS; wall_clock64 counts 100 MHz

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
launch = int(sys.argv[2]) if len(sys.argv) > 2 else 10
regs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ITERS = 20

sc = pkg.synth.make_scene(m=1_000_000, n=n, seed_scan=43)
icp = pkg.ICPSequence(minimizer=1, max_dist=2.0, outliers=[(4, 0.85)], max_iterations=ITERS)
d_map, d_nrm, d_scan = (torch.from_numpy(sc[k]).cuda() for k in ("map", "normals", "scan"))
assert icp.setMapDev(d_map.data_ptr(), d_map.shape[0], d_nrm.data_ptr())
lib = icp._lib
try:
    fn = lib.icpmi_debug_nn_timeline
except AttributeError:
    sys.exit("this libicpmi.so is not a timing build (-DICPMI_NN_TIMING): see the docstring")
fn.restype = C.c_int
fn.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]


def pct(a, q):
    return float(np.percentile(a, q))


def one_registration(verbose):
    icp.registerDev(d_scan.data_ptr(), d_scan.shape[0], fixed_iterations=ITERS)
    wg = np.zeros((TL_LAUNCHES, TL_WGS, 4), dtype=np.uint64)
    oc = np.zeros((2, TL_LAUNCHES), dtype=np.uint64)
    cnt = C.c_uint32(0)
    rc = fn(icp._h, wg.ctypes.data_as(C.POINTER(C.c_uint64)), oc.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(cnt))
    assert rc == 0 and cnt.value > launch + 1, (rc, cnt.value)
    w = wg[launch]
    w = w[w[:, 0] != 0]
    t0 = int(oc[0, launch])  # the launch's open stamp (workgroup 0's thread 0)
    first = int(w[:, 0].min())
    rel = lambda a: (a.astype(np.int64) - first) * TICK_US
    t_in, t_iss, t_drn = rel(w[:, 0]), rel(w[:, 1]), rel(w[:, 2])
    xcc = (w[:, 3] & np.uint64(0xff)).astype(np.int64)
    pieces = ((w[:, 3] >> np.uint64(8)) & np.uint64(0xffffffff)).astype(np.int64)
    passes = ((w[:, 3] >> np.uint64(40)) & np.uint64(0xffff)).astype(np.int64)
    life = t_drn - t_in
    close = (int(oc[1, launch]) - first) * TICK_US
    nxt_first = (int(wg[launch + 1][:, 0][wg[launch + 1][:, 0] != 0].min()) - first) * TICK_US
    prev_close = (int(oc[1, launch - 1]) - first) * TICK_US
    r = dict(wgs=len(w), open=(t0 - first) * TICK_US, prev_close=prev_close, start_last=float(t_in.max()), start_p50=pct(t_in, 50), start_p90=pct(t_in, 90),
             issued_p50=pct(t_iss, 50), issued_p90=pct(t_iss, 90), issued_max=float(t_iss.max()),
             end_p50=pct(t_drn, 50), end_p90=pct(t_drn, 90), end_max=float(t_drn.max()), drain_p50=pct(t_drn - t_iss, 50), drain_p90=pct(t_drn - t_iss, 90),
             drain_max=float((t_drn - t_iss).max()), life_p50=pct(life, 50), life_p90=pct(life, 90), life_max=float(life.max()),
             close=close, gap=close - float(t_drn.max()), next_nn_first=nxt_first)
    if verbose:
        print(f"launch {launch} of {cnt.value}, {len(w)} workgroups; times in us from the first workgroup's entry (100 MHz constant clock, 0.01 us a tick)")
        print(f"  previous kernel boundary: the launch before was closed at {prev_close:+.2f}")
        print(f"  workgroup start : first 0.00, p50 {r['start_p50']:.2f}, p90 {r['start_p90']:.2f}, last {r['start_last']:.2f}")
        print(f"  last store issued: p50 {r['issued_p50']:.2f}, p90 {r['issued_p90']:.2f}, p100 {r['issued_max']:.2f}")
        print(f"  workgroup end (stores drained): p50 {r['end_p50']:.2f}, p90 {r['end_p90']:.2f}, p100 {r['end_max']:.2f}")
        print(f"  issue -> drained: p50 {r['drain_p50']:.2f}, p90 {r['drain_p90']:.2f}, max {r['drain_max']:.2f}")
        print(f"  workgroup life  : p50 {r['life_p50']:.2f}, p90 {r['life_p90']:.2f}, max {r['life_max']:.2f}")
        print(f"  next kernel's first workgroup (close stamp): {close:.2f}  -> span from the last workgroup end: {r['gap']:.2f}")
        print(f"  next NN launch's first workgroup: {nxt_first:.2f} (one iteration)")
        print("  per XCC: workgroups, start p50 / last, end p50 / p100, life p50, pieces p50")
        for x in sorted(set(xcc.tolist())):
            m = xcc == x
            print(f"    xcc {x}: {int(m.sum()):4d}  start {pct(t_in[m], 50):6.2f} / {t_in[m].max():6.2f}  end {pct(t_drn[m], 50):6.2f} / {t_drn[m].max():6.2f}"
                  f"  life {pct(life[m], 50):5.2f}  pieces {pct(pieces[m], 50):.0f}")
        print("  pieces per workgroup against life (deciles of pieces): pieces, life p50, end p50")
        order = np.argsort(pieces, kind="stable")
        for d in range(10):
            sl = order[d * len(order) // 10:(d + 1) * len(order) // 10]
            if len(sl): print(f"    decile {d}: pieces {pieces[sl].min():4d}..{pieces[sl].max():4d}  life {pct(life[sl], 50):5.2f}  end {pct(t_drn[sl], 50):6.2f}")
        c = np.corrcoef(pieces, life)[0, 1] if len(w) > 2 else float("nan")
        print(f"  correlation pieces ~ life: {c:.2f}")
        print("  passes of the level loop per workgroup against life: passes, workgroups, life p50 / max, end p50 / max")
        for ps in sorted(set(passes.tolist())):
            m = passes == ps
            print(f"    {ps} passes: {int(m.sum()):4d}  life {pct(life[m], 50):5.2f} / {life[m].max():5.2f}  end {pct(t_drn[m], 50):6.2f} / {t_drn[m].max():6.2f}")
        late = np.argsort(t_drn)[-5:][::-1]
        print("  five last workgroups to end: " + "; ".join(f"start {t_in[i]:.2f} end {t_drn[i]:.2f} life {life[i]:.2f} pieces {pieces[i]} passes {passes[i]} xcc {xcc[i]}" for i in late))
    return r


for _ in range(3):
    icp.registerDev(d_scan.data_ptr(), d_scan.shape[0], fixed_iterations=ITERS)
rows = [one_registration(verbose=(i == 0)) for i in range(regs)]
print(f"medians over {regs} registrations (same launch):")
for k in rows[0]:
    if k != "wgs": print(f"  {k:14s} {np.median([r[k] for r in rows]):8.2f}   (min {min(r[k] for r in rows):.2f}, max {max(r[k] for r in rows):.2f})")
d = icp.debugCounters()
if d[23]:
    print(f"clock: {d[22]} shader ticks over {d[23]} ticks of 100 MHz in the sampled workgroups = {d[22] / d[23] * 0.1:.3f} GHz")
s = icp.stats
print(f"nn_ms_avg (open stamp -> close stamp, mean over the registration's launches): {getattr(s, 'nn_ms_avg', float('nan')) * 1e3:.2f} us")
