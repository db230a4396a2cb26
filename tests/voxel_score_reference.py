"""Float64 reference of the voxel pose score (include/icpmi.h: icpmi_voxel_score_poses) and a float32 restatement of the
header's arithmetic.  Pure numpy, built on tests/voxel_reference.py: nothing here touches the library.

Per reading point x and centred-frame pose Tc: p = Tc x, the voxel p falls into by the FLOAT32 key of the FLOAT32 point (none: no pair),
d = p - mu, u = unit_or_zero(R n_x), S = 2 I - (1 - eps)(N + u u^T), M = S^-1, r = d^T M d, l = exp(-beta / 2 r).  Per pose: pairs,
likelihood = sum l, sum_maha = sum r, max_maha = max r.
"""
import numpy as np

import plane_to_plane_reference as pr
import voxel_reference as vr

F32 = np.float32


def centred_pose(T, mean):
    """the pose the device scores under, from a map-frame correction T (4 x 4 float32) and the handle's mean (float32): [R | t + R mu - mu],
    the translation formed in double in the header's order and rounded once (api.hip: centred_pose)"""
    T = np.asarray(T, F32)
    m = [float(v) for v in np.asarray(mean, F32)]
    Tc = T.copy()
    for r in range(3):
        Tc[r, 3] = F32((float(T[r, 3]) + ((float(T[r, 0]) * m[0] + float(T[r, 1]) * m[1]) + float(T[r, 2]) * m[2])) - m[r])
    Tc[3] = (0, 0, 0, 1)
    return Tc


def map_frame_pose(Tc, mean):
    """a map-frame correction whose centred pose is (about) Tc: M Tc M^-1 with M the translation by the mean, float64"""
    M = np.eye(4)
    M[:3, 3] = np.asarray(mean, np.float64)
    return M @ np.asarray(Tc, np.float64) @ np.linalg.inv(M)


def pairing(Tc, rc, tab):
    """(p float32 (N, 3), vox (N,)): the points as the device forms them and the voxel of each by the float32 key (-1: no pair)"""
    p = pr.xf_points(np.asarray(Tc, F32), rc)
    return p, vr.lookup(tab, p)


def _result(r, l):
    if r.size == 0:
        return dict(pairs=0, likelihood=0.0, sum_maha=0.0, max_maha=r.dtype.type(0))
    assert l.dtype == r.dtype
    return dict(pairs=int(r.size), likelihood=float(l.astype(np.float64).sum()), sum_maha=float(r.astype(np.float64).sum()), max_maha=r.max())


def score64(Tc, rc, rn, tab, beta=1.0, eps=pr.EPS_DEFAULT, vox=None):
    """the float64 score of the float32 clouds under the pose Tc (its entries taken as they are): float64 table, points, inverse and sums;
    the pairing is the float32 key of the float32 point (vox: that pairing when the caller has it already)"""
    if vox is None:
        _, vox = pairing(Tc, rc, tab)
    sel = vox >= 0
    T = np.asarray(Tc, np.float64)
    x = np.asarray(rc, F32)[sel].astype(np.float64)
    p = x[:, :3] @ T[:3, :3].T + x[:, 3:4] * T[:3, 3]
    npr = np.asarray(rn, F32)[sel].astype(np.float64) @ T[:3, :3].T
    v = vox[sel]
    M = vr.pair_matrices(np.asarray(tab["N"], np.float64)[v], npr, eps)
    d = p - np.asarray(tab["mu"], np.float64)[v]
    r = np.einsum("ni,nij,nj->n", d, M, d)
    return _result(r, np.exp(-0.5 * float(beta) * r))


def score32(Tc, rc, rn, tab, beta=1.0, eps=pr.EPS_DEFAULT):
    """the header's arithmetic restated in float32: pr.xf_points / pr.rot_normals, the float32 table, the adjugate inverse of
    vr.float32_sums, r in the header's order, numpy's float32 exp, the sums in float64.  Differs from the kernel by expf and the order of
    the double sums."""
    Tc = np.asarray(Tc, F32)
    p, vox = pairing(Tc, rc, tab)
    sel = vox >= 0
    v = vox[sel]
    p = p[sel]
    up = pr.unit_or_zero(pr.rot_normals(Tc, np.asarray(rn, F32))[sel].copy())
    q, N6 = np.asarray(tab["mu"]).astype(F32)[v], np.asarray(tab["N"]).astype(F32)[v]
    g, two = F32(1) - F32(eps), F32(2)
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}

    def s(i, j):
        t = g * (N6[:, idx[(i, j)]] + up[:, i] * up[:, j])
        return two - t if i == j else -t

    sxx, syy, szz, sxy, sxz, syz = s(0, 0), s(1, 1), s(2, 2), s(0, 1), s(0, 2), s(1, 2)
    c00, c01, c02 = syy * szz - syz * syz, sxz * syz - sxy * szz, sxy * syz - sxz * syy
    c11, c12, c22 = sxx * szz - sxz * sxz, sxy * sxz - sxx * syz, sxx * syy - sxy * sxy
    idet = F32(1) / (sxx * c00 + sxy * c01 + sxz * c02)
    m00, m01, m02, m11, m12, m22 = c00 * idet, c01 * idet, c02 * idet, c11 * idet, c12 * idet, c22 * idet
    d = p - q
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    mdx, mdy, mdz = m00 * dx + m01 * dy + m02 * dz, m01 * dx + m11 * dy + m12 * dz, m02 * dx + m12 * dy + m22 * dz
    r = dx * mdx + dy * mdy + dz * mdz
    assert r.dtype == F32
    hb = F32(0.5) * F32(beta)
    out = _result(r, np.exp(-(hb * r)))
    out["vox"] = vox
    return out


def rel(a, b):
    """|a - b| / |b|; 0 when both vanish"""
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / abs(b)


def rank(table, n, min_pairs_ratio=0.0):
    """icp.rank_voxel_candidates restated: (status, pairs, likelihood) rows -> indices, likelihood / n descending, ties by the lower index"""
    need = float(F32(min_pairs_ratio)) * float(n)
    rows = [(-(float(l) / float(n)), i) for i, (st, pairs, l) in enumerate(table) if int(st) == 0 and int(pairs) > 0 and float(int(pairs)) >= need]
    return [i for _, i in sorted(rows)]
