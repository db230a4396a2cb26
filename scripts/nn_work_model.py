#!/usr/bin/env python
"""CPU model of the row phase of a steady nn1_wg_kernel launch of the headline registration (100 k x 1 M, point-to-point, TrimmedDist 0.85):
how many candidate pieces every query, and every workgroup of 64 queries in tile order, brings -- and what deferring the heavy queries to
helper workgroups of eight (nn.hip: `defer`) leaves in the home workgroups.  No GPU, no library: numpy; the matches come from scipy's cKDTree where scipy is present, else from a blocked distance matrix (minutes).

What it restates of the kernels: the seed rule (the first level whose 3 x 3 x 3 block holds the ball around the query through its previous
match: block_holds_ball), the rows of that block clipped by the ball (clip_row_x), pieces of 16 candidates per row (wg_rows_to_pieces), and
the queries' super-tile order (map_build.hip: st_key, 16 x 4 x 4 cells).  What it does not: the grid's exact origin and padding (the box of
the centred map, so cell boundaries sit within a cell of the library's), the own-row pass of the first seeded launch, passes beyond the
first for the few queries that climb a level inside the launch, and the overflow round of a workgroup with more than 1 024 pieces.  The
poses are a float64 trimmed point-to-point loop, which stalls where the device's float32 loop stalls (bench.py's pose_err_vs_ground_truth).

usage: nn_work_model.py [--cell 0.559] [--iteration 10] [--points 100000]
--cell: the level-0 cell edge the library chose for the map (ICPSequence.gridInfo()["cell"])."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from norlab_icp_mapper_amd import synth  # noqa: E402

STX, STY, STZ, Q, PIECE, CAP = 16, 4, 4, 64, 16, 1024


def kabsch(p, q):
    mp, mq = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((q - mq).T @ (p - mp))
    if np.linalg.det(U @ Vt) < 0: Vt[-1] *= -1
    T = np.eye(4); T[:3, :3] = U @ Vt; T[:3, 3] = mq - T[:3, :3] @ mp
    return T


class Level:
    def __init__(self, pts, lo, hi, cell, maxabs):
        self.cell, self.lo = cell, lo
        self.slack = cell * 1e-3 + maxabs * 2e-6
        self.n = np.maximum(np.ceil((hi - lo) / cell).astype(int), 1)
        c = np.minimum(((pts - lo) / cell).astype(int), self.n - 1)
        cnt = np.zeros(self.n[::-1], np.int64)                       # [z, y, x]
        np.add.at(cnt, (c[:, 2], c[:, 1], c[:, 0]), 1)
        self.px = np.concatenate([np.zeros(cnt.shape[:2] + (1,), np.int64), np.cumsum(cnt, axis=2)], axis=2)

    def pos(self, q):
        f = (q - self.lo) / self.cell
        fl = np.floor(f)
        fr = f - fl
        return fl.astype(int), fr, np.minimum(fr, 1.0 - fr).min(1)     # cell, fraction, mf

    def holds(self, q, ub):                                           # block_holds_ball
        return ub <= (1.0 + self.pos(q)[2]) * self.cell - 2.0 * self.slack

    def pieces(self, q, ub):
        """candidates and pieces of the 3 x 3 x 3 block's rows the ball of radius ub (+ slack) reaches"""
        c, fr, _ = self.pos(q)
        rub2 = (ub * 1.000001 + self.slack) ** 2
        cand = np.zeros(len(q), np.int64); pcs = np.zeros(len(q), np.int64)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                ddy = 0.0 if dy == 0 else (fr[:, 1] if dy < 0 else 1.0 - fr[:, 1]) * self.cell
                ddz = 0.0 if dz == 0 else (fr[:, 2] if dz < 0 else 1.0 - fr[:, 2]) * self.cell
                rem2 = rub2 - (ddy * ddy + ddz * ddz)
                y, z = c[:, 1] + dy, c[:, 2] + dz
                ok = (rem2 >= 0) & (y >= 0) & (y < self.n[1]) & (z >= 0) & (z < self.n[2])
                r = np.sqrt(np.maximum(rem2, 0.0))
                xa = np.maximum(np.maximum(np.floor((q[:, 0] - r - self.lo[0]) / self.cell).astype(int), c[:, 0] - 1), 0)
                xb = np.minimum(np.minimum(np.floor((q[:, 0] + r - self.lo[0]) / self.cell).astype(int), c[:, 0] + 1), self.n[0] - 1)
                ok &= xa <= xb
                yy, zz = np.clip(y, 0, self.n[1] - 1), np.clip(z, 0, self.n[2] - 1)
                k = np.where(ok, self.px[zz, yy, np.clip(xb + 1, 0, self.n[0])] - self.px[zz, yy, np.clip(xa, 0, self.n[0])], 0)
                cand += k; pcs += (k + PIECE - 1) // PIECE
        return cand, pcs


def nearest_fn(mp):
    """q -> (distance, index) of the nearest map point: scipy's cKDTree where present, else blocks of a float32 distance matrix (minutes)"""
    try:
        from scipy.spatial import cKDTree
        tree = cKDTree(mp)
        return lambda q: tree.query(q, workers=-1)
    except ImportError:
        m32, m2 = mp.astype(np.float32), (mp * mp).sum(1).astype(np.float32)
        def brute(q):
            idx = np.empty(len(q), np.int64)
            for i in range(0, len(q), 128):
                idx[i:i + 128] = (m2[None, :] - 2.0 * (q[i:i + 128].astype(np.float32) @ m32.T)).argmin(1)
            return np.linalg.norm(q - mp[idx], axis=1), idx    # (the winner of the float32 matrix, its distance in float64)
        return brute


def pct(a, qs=(50, 90, 99, 100)):
    return " / ".join(f"{np.percentile(a, q):.0f}" for q in qs) if len(a) else "-"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cell", type=float, default=0.559)
    ap.add_argument("--iteration", type=int, default=10)
    ap.add_argument("--points", type=int, default=100_000)
    args = ap.parse_args()
    sc = synth.make_scene(m=1_000_000, n=args.points)
    mp = sc["map"][:, :3].astype(np.float64); mp -= mp.mean(0)
    rd = sc["scan"][:, :3].astype(np.float64) - sc["map"][:, :3].astype(np.float64).mean(0)
    nearest = nearest_fn(mp)
    lo, hi, maxabs = mp.min(0), mp.max(0) + 1e-6, np.abs(mp).max()
    levels, cell = [], args.cell
    while True:
        levels.append(Level(mp, lo, hi, cell, maxabs))
        if levels[-1].cell - levels[-1].slack > 2.0 or (levels[-1].n <= 2).all(): break
        cell *= 2.0
    T, prev = np.eye(4), None
    for it in range(args.iteration + 1):
        q = rd @ T[:3, :3].T + T[:3, 3]
        d, idx = nearest(q)
        idx = np.where(d <= 2.0, idx, -1)
        if it == args.iteration: break
        ok = idx >= 0
        lim = np.sort(d[ok])[int(np.float32(ok.sum()) * np.float32(0.85))]
        w = ok & (d <= lim)
        T = kabsch(q[w], mp[idx[w]]) @ T
        prev = idx
    print(f"iteration {args.iteration}: match distance p50 / p99 {np.percentile(d[idx >= 0], 50):.3f} / {np.percentile(d[idx >= 0], 99):.3f} m, level-0 cell {args.cell} m, {len(levels)} levels")
    seeded = prev >= 0
    ub = np.where(seeded, np.linalg.norm(q - mp[np.maximum(prev, 0)], axis=1), np.inf)
    lev = np.full(len(q), len(levels) - 1)
    for l in range(len(levels) - 1, -1, -1):
        lev = np.where(levels[l].holds(q, ub), l, lev)
    cand = np.zeros(len(q), np.int64); pcs = np.zeros(len(q), np.int64)
    for l, L in enumerate(levels):
        m = lev == l
        if m.any(): cand[m], pcs[m] = L.pieces(q[m], np.where(np.isfinite(ub[m]), ub[m], 1e9))
    print(f"queries above level 0: {(lev > 0).sum()} ({100.0 * (lev > 0).mean():.2f} %); candidates per query p50 {np.percentile(cand, 50):.0f}, of those {pct(cand[lev > 0], (5, 50, 95))} (p5 / p50 / p95)")
    top = np.sort(cand)[::-1]
    print(f"the top 1 % of the queries carry {100.0 * top[:len(top) // 100].sum() / max(top.sum(), 1):.1f} % of all candidates")
    # tile order: the reading's own (centred, unmoved) points keyed on level 0, stable
    L0 = levels[0]
    c0 = np.clip(((rd - L0.lo) / L0.cell).astype(int), 0, L0.n - 1)
    tx, ty = (L0.n[0] + STX - 1) // STX, (L0.n[1] + STY - 1) // STY
    order = np.argsort(((c0[:, 2] // STZ) * ty + c0[:, 1] // STY) * tx + c0[:, 0] // STX, kind="stable")
    pcs_o, cand_o, lev_o = pcs[order], cand[order], lev[order]
    nwg = (len(q) + Q - 1) // Q
    pad = nwg * Q - len(q)
    wg = lambda a: np.concatenate([a, np.zeros(pad, a.dtype)]).reshape(nwg, Q).sum(1)  # noqa: E731
    home = wg(pcs_o)
    print(f"pieces per workgroup p50 / p90 / p99 / max: {pct(home)}; above 256: {(home > 256).sum()}, above 512: {(home > 512).sum()}, above {CAP}: {(home > CAP).sum()}")
    eighth = np.array_split(np.arange(nwg), 8)
    print("candidates per eighth of the query order (k): " + " ".join(f"{wg(cand_o)[e].sum() / 1e3:.0f}" for e in eighth))
    print("workgroups above 256 pieces per eighth:        " + " ".join(str(int((home[e] > 256).sum())) for e in eighth))
    print("\n| threshold | deferred | helpers of 8 | home max | home > 256 | helper pieces p50 / max | helpers of 16 above 256 |")
    print("|---|---|---|---|---|---|---|")
    for name, heavy in (("level >= 1", lev_o > 0), ("level >= 1 or > 8 pieces", (lev_o > 0) | (pcs_o > 8)), ("> 6 pieces", pcs_o > 6)):
        rest = wg(np.where(heavy, 0, pcs_o))
        hp = pcs_o[heavy]
        h8 = np.add.reduceat(hp, np.arange(0, len(hp), 8)) if len(hp) else np.zeros(0)
        h16 = np.add.reduceat(hp, np.arange(0, len(hp), 16)) if len(hp) else np.zeros(0)
        print(f"| {name} | {heavy.sum()} | {len(h8)} | {rest.max()} | {(rest > 256).sum()} | {pct(h8, (50, 100))} | {(h16 > 256).sum()} |")


if __name__ == "__main__":
    main()
