"""Writes deskew_scan0_slice.npz: every 8th point of the first bundled example scan (lexicographic file order, as the example
harness reads them) with its `t` row -- the per-point time in nanoseconds from the start of the sweep, the descriptor sweep
deskewing reads -- and its intensity.  Data the reference ships with its example (examples/data/scans/*.vtk; BSD-3).

Run by hand, with the reference's example data directory as the argument:

    python tests/golden/make_deskew_slice.py <reference>/examples/data

No test runs this; tests/test_gpu_deskew.py reads the .npz only.
"""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EVERY = 8


def read_vtk(path):
    """ASCII VTK POLYDATA in libpointmatcher's dialect: POINTS n float, then SCALARS blocks of n values each"""
    with open(path) as f:
        lines = f.read().split("\n")
    i = 0
    while not lines[i].startswith("POINTS"):
        i += 1
    n = int(lines[i].split()[1])
    pts = np.array([[float(v) for v in lines[i + 1 + r].split()] for r in range(n)], dtype=np.float32)
    scalars = {}
    j = i + 1 + n
    while j < len(lines):
        if lines[j].startswith("SCALARS"):
            scalars[lines[j].split()[1]] = np.array([float(lines[j + 2 + r]) for r in range(n)], dtype=np.float32)
            j += 2 + n
        else:
            j += 1
    return pts, scalars


def main(data_dir):
    scans = sorted(glob.glob(os.path.join(data_dir, "scans", "*.vtk")))
    pts, scalars = read_vtk(scans[0])
    if "t" not in scalars:
        raise SystemExit(scans[0] + " has no `t` row")
    sel = slice(0, None, EVERY)
    out = os.path.join(HERE, "deskew_scan0_slice.npz")
    np.savez_compressed(out, scan_name=np.array(os.path.basename(scans[0])), every=np.array(EVERY), n_full=np.array(len(pts)),
                        xyz=pts[sel], t=scalars["t"][sel], intensity=scalars.get("intensity", np.zeros(len(pts), np.float32))[sel])
    print("wrote", out, pts[sel].shape, "t in [%g, %g] ns" % (scalars["t"].min(), scalars["t"].max()))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
