"""Integer-exact numpy reference of the quantile selection of the outlier-filter chain (Matches::getDistsQuantile and the filters built
on it).  The limit is ONE ELEMENT of the multiset of positive finite d2 bit patterns and the pair count is a count: nothing here has a
tolerance.  MedianDist's limit and VarTrimmedDist's ratio are weights_reference's (the same rules, stated once).

tests/test_selection_cpu.py holds this file to the oracle on every distance set of tests/selection_cases.py before the GPU is asked."""
import numpy as np

import weights_reference as wr

MAXDIST, MINDIST, MEDIAN, TRIMMED, VARTRIMMED = wr.MAXDIST, wr.MINDIST, wr.MEDIAN, wr.TRIMMED, wr.VARTRIMMED
NO_OUTLIER_TO_FILTER = 4            # ICPMI_ERR_NO_OUTLIER_TO_FILTER
ORACLE_NO_OUTLIER_TO_FILTER = 2     # ORC_ERR_NO_OUTLIER_TO_FILTER: the same ConvergenceError("no outlier to filter")


class NoValidDistance(ValueError):
    pass


def sorted_bits(d2):
    """uint32 bit patterns of the entries that are finite and > 0, ascending (positive floats order like their bit patterns)"""
    v = np.ascontiguousarray(d2, dtype=np.float32).ravel()
    return np.sort(v[np.isfinite(v) & (v > 0)].view(np.uint32))


def rank(total, q):
    """the index getDistsQuantile takes: total - 1 for q == 1, else the truncated FLOAT32 product, clamped"""
    if total == 0:
        raise NoValidDistance("no finite positive distance")
    if np.float32(q) == np.float32(1.0):
        return total - 1
    return min(int(np.float32(total) * np.float32(q)), total - 1)


def quantile(d2, q):
    """float32: the element of rank rank(total, q) of the sorted valid bit patterns; raises NoValidDistance when there is none"""
    s = sorted_bits(d2)
    return s[rank(s.size, q):][:1].view(np.float32)[0]


def median_limit(d2, factor):
    """MedianDistOutlierFilter: float32(factor) * median as one float32 product (weights_reference.median_limit)"""
    if sorted_bits(d2).size == 0:
        raise NoValidDistance("no finite positive distance")
    return np.float32(wr.median_limit(d2, factor))


def var_trimmed(d2, min_ratio, max_ratio, lam):
    """(ratio, limit) of VarTrimmedDistOutlierFilter: weights_reference.var_trimmed_ratio, then the quantile at that ratio"""
    if sorted_bits(d2).size == 0:
        raise NoValidDistance("no finite positive distance")
    ratio = np.float32(wr.var_trimmed_ratio(d2, min_ratio, max_ratio, lam))
    return ratio, quantile(d2, ratio)


def frms(d2, lam):
    """(float64 FRMS of every rank i < V of the sorted valid d2, N): cum(i) / ((i + 1) ((i + 1) / N)^(2 lam)), N = every entry"""
    N = np.asarray(d2).size
    s = sorted_bits(d2).view(np.float32).astype(np.float64)
    i = np.arange(1, s.size + 1, dtype=np.float64)
    return np.cumsum(s) / (i * (i / N) ** (2.0 * float(np.float32(lam)))), N


def chain(outliers, d2):
    """(weights (n, k) float32 of 0 / 1, limit of the LAST quantile-type filter as float32 or None) of a chain of MaxDist / MinDist /
    Median / Trimmed / VarTrimmed filters; every comparison is the float32 one the filters take"""
    d2 = np.ascontiguousarray(d2, dtype=np.float32)
    w = np.ones(d2.shape, bool)
    limit = None
    for o in outliers:
        t, prm = int(o[0]), np.float32(o[1])
        if t == MAXDIST: w &= d2 <= prm * prm
        elif t == MINDIST: w &= d2 >= prm * prm
        else:
            if t == TRIMMED: limit = quantile(d2, prm)
            elif t == MEDIAN: limit = median_limit(d2, prm)
            elif t == VARTRIMMED: limit = var_trimmed(d2, prm, o[3], o[4])[1]
            else: raise ValueError(t)
            w &= d2 <= limit
    return w.astype(np.float32), limit
