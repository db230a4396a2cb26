"""VoxelGridDataPointsFilter{vSizeX, vSizeY, vSizeZ, useCentroid: 1, averageExistingDescriptors} restated in numpy float32, from the
formulation as recalled (include/icpmi.h, icpmi_voxel_grid), not from the kernels.  Every quantity is float32; numpy's
float32 division is IEEE correctly rounded and nothing is contracted.  The voxel sums are sequential: each accumulator starts from its
voxel's first member and np.add.at adds the other members one float32 add at a time, in ascending index order."""
import numpy as np

F = np.float32


class VoxelGridLimit(ValueError):
    """a cloud or a size outside the contract (what icpmi_voxel_grid rejects with ICPMI_ERR_INVALID_ARG)"""


def grid(xyz, vsize):
    """-> (minB, numDiv (uint32, 3), idx (uint32, n)) of the lattice, or VoxelGridLimit"""
    xyz = np.asarray(xyz, F)
    vs = np.broadcast_to(np.asarray(vsize, F), (3,)).copy()
    if not (np.isfinite(vs).all() and (vs > 0).all()):
        raise VoxelGridLimit("vSize must be finite and > 0")
    if not np.isfinite(xyz).all():
        raise VoxelGridLimit("non-finite coordinates")
    with np.errstate(over="ignore", invalid="ignore"):
        minB = xyz.min(0) / vs
        maxB = xyz.max(0) / vs
        nd_f = (F(1) + maxB) - minB                    # left to right, in float
    if not (nd_f < F(2 ** 24)).all():
        raise VoxelGridLimit("numDiv reaches 2^24")
    nd = [int(v) for v in nd_f]                        # truncation
    if nd[0] * nd[1] * nd[2] > 2 ** 32 - 1:
        raise VoxelGridLimit("numVox exceeds 2^32 - 1")
    ijk = np.floor(xyz / vs - minB).astype(np.uint32)
    d0 = np.uint32(nd[0])
    d01 = np.uint32((nd[0] * nd[1]) & 0xFFFFFFFF)
    idx = ijk[:, 0] + ijk[:, 1] * d0 + ijk[:, 2] * d01  # uint32 arrays: wraps like unsigned arithmetic
    return minB, np.array(nd, np.uint32), idx.astype(np.uint32)


def _seq_mean(rows, inv, first, counts):
    """per voxel: rows[first] + every other member in index order (one float32 add each), / (float)count"""
    acc = rows[first].astype(F).copy()
    rest = np.ones(rows.shape[0], bool)
    rest[first] = False
    np.add.at(acc, inv[rest], rows[rest])
    return acc / counts.astype(F).reshape((-1,) + (1,) * (rows.ndim - 1))


def voxel_grid(cloud4, vsize, average_descriptors=True, desc=None):
    """-> (order, out4, desc_out): the first-point index of every voxel (ascending), the centroids with the first point's
    homogeneous row, and the descriptor rows (averaged, or the first point's); desc_out is None without descriptors"""
    c = np.asarray(cloud4, F)
    n = c.shape[0]
    d = None if desc is None else np.asarray(desc, F).reshape(n, -1)
    _, _, idx = grid(c[:, :3], vsize) if n else grid(np.zeros((1, 3), F), vsize)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros((0, 4), F), (None if d is None else np.zeros((0, d.shape[1]), F))
    _, first, inv = np.unique(idx, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    counts = np.bincount(inv)
    xyz = _seq_mean(c[:, :3], inv, first, counts)
    perm = np.argsort(first, kind="stable")
    out4 = np.empty((len(first), 4), F)
    out4[:, :3] = xyz[perm]
    out4[:, 3] = c[first[perm], 3]
    dout = None
    if d is not None:
        dout = (_seq_mean(d, inv, first, counts) if average_descriptors else d[first])[perm]
    return first[perm].astype(np.int32), out4, dout


def planar_voxel_grid_2d(cloud4, vx, vy):
    """upstream's 2-D formula (is3D == false) written on its own: x and y only, idx = i + j numDivX, z of the output = 0"""
    c = np.asarray(cloud4, F)
    vs = np.array([vx, vy], F)
    minB = c[:, :2].min(0) / vs
    maxB = c[:, :2].max(0) / vs
    nd = ((F(1) + maxB) - minB).astype(np.uint32)
    ij = np.floor(c[:, :2] / vs - minB).astype(np.uint32)
    idx = ij[:, 0] + ij[:, 1] * nd[0]
    order, sums, counts = [], {}, {}
    for p in range(c.shape[0]):
        k = int(idx[p])
        if k not in sums:
            order.append(p)
            sums[k] = c[p, :2].copy()
            counts[k] = 1
        else:
            sums[k] = (sums[k] + c[p, :2]).astype(F)
            counts[k] += 1
    out = np.zeros((len(order), 4), F)
    for o, p in enumerate(order):
        k = int(idx[p])
        out[o, :2] = sums[k] / F(counts[k])
        out[o, 3] = c[p, 3]
    return np.array(order, np.int32), out
