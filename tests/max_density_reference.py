"""MaxDensityDataPointsFilter's draw, restated in numpy (the formulation in include/icpmi.h: icpmi_max_density_keep).  The definition is the
host filter (host/DataPointsFilters.cpp: MaxDensityFilter), which tests/test_max_density_cpu.py holds this file to; the GPU tests then hold
the kernel to this file.

  dense_i = densities[i] > maxDensity                (NaN: not dense)
  v       = std::minstd_rand seeded with (uint32) seed % 2147483647, 0 -> 1; only the dense points draw, in index order
  u_i     = float32(v_i) / float32(2147483645)       (one correctly rounded float32 division)
  keep_i  = dense_i ? u_i < maxDensity / densities[i] : 1     (float32)
"""
import numpy as np

F = np.float32
MINSTD_A, MINSTD_M = 48271, 2147483647


class MinStd:
    """std::minstd_rand: x <- 48271 x mod (2^31 - 1); the constructor's seed rule."""

    def __init__(self, seed):
        self.x = (int(seed) & 0xFFFFFFFF) % MINSTD_M
        if self.x == 0:
            self.x = 1

    def __call__(self):
        self.x = self.x * MINSTD_A % MINSTD_M
        return self.x


def minstd_stream(seed, count):
    g = MinStd(seed)
    return np.array([g() for _ in range(count)], dtype=np.uint32)


def max_density_keep(densities, max_density, seed=1):
    """bool keep mask of the filter on a (n,) float32 density row."""
    d = np.ascontiguousarray(densities, dtype=F)
    md = F(max_density)
    with np.errstate(invalid="ignore"):
        dense = d > md
    keep = np.ones(d.shape[0], dtype=bool)
    idx = np.nonzero(dense)[0]
    if idx.size:
        v = minstd_stream(seed, idx.size)
        u = v.astype(F) / F(2147483645.0)                       # uint32 -> float32 rounds to nearest, as the C++ cast
        with np.errstate(divide="ignore", over="ignore", under="ignore"):
            bound = (md / d[idx]).astype(F)
        keep[idx] = u < bound
    return keep


def log_uniform_densities(rng, n, lo=0.1, hi=1000.0):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(F)
