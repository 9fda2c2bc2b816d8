"""Brute-force numpy form of the outlier filters as treelearn_amd/util/outlier.py states them: the specification the
kernels of csrc/tl_outlier.hip are compared with.  open3d is not installed, so this -- not open3d -- is the reference.

All arithmetic is float64; d2(i, j) = (dx*dx + dy*dy) + dz*dz with numpy's separate multiplies and adds (no fma), d = sqrt(d2) (numpy's
sqrt is correctly rounded), the k smallest distances added column by column in ascending order, the two cloud sums with math.fsum."""
import math

import numpy as np

BLOCK = 512


def _d2_rows(xyz, a, e):
    dx = xyz[None, :, 0] - xyz[a:e, None, 0]
    dy = xyz[None, :, 1] - xyz[a:e, None, 1]
    dz = xyz[None, :, 2] - xyz[a:e, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def sorted_distances(xyz, k):
    """f64 [n, min(k, n)]: the min(k, n) smallest d(i, .) of every point, ascending (column 0 is the point itself, 0)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)[:, :3]
    n = len(xyz); kk = min(int(k), n)
    out = np.empty((n, kk), dtype=np.float64)
    for a in range(0, n, BLOCK):
        d2 = _d2_rows(xyz, a, min(a + BLOCK, n))
        part = np.partition(d2, kk - 1, axis=1)[:, :kk]
        out[a:a + BLOCK] = np.sqrt(np.sort(part, axis=1))
    return out


def mean_of_sorted(dist, k):
    """avg of the first min(k, columns) columns, added one after the other."""
    kk = min(int(k), dist.shape[1])
    s = np.zeros(len(dist), dtype=np.float64)
    for t in range(kk):
        s = s + dist[:, t]
    return s / np.float64(kk)


def knn_mean_dist(xyz, k):
    if len(xyz) == 0:
        return np.zeros(0)
    return mean_of_sorted(sorted_distances(xyz, k), k)


def sor_threshold(avg, s):
    n = len(avg)
    pos = avg[avg > 0]
    mean = math.fsum(pos) / n
    dev = pos - mean
    std = math.sqrt(math.fsum(dev * dev) / (n - 1))
    return mean + s * std


def sor_mask_from_avg(avg, s):
    if len(avg) <= 1:
        return np.zeros(len(avg), dtype=bool)
    return (avg > 0) & (avg < sor_threshold(avg, s))


def sor_mask(xyz, k, s):
    if k < 1 or not s > 0:
        raise ValueError("nb_neighbors must be >= 1 and std_ratio > 0")
    return sor_mask_from_avg(knn_mean_dist(xyz, k), s)


def radius_count(xyz, r):
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)[:, :3]
    n = len(xyz)
    r2 = np.float64(r) * np.float64(r)
    out = np.empty(n, dtype=np.int32)
    for a in range(0, n, BLOCK):
        out[a:a + BLOCK] = (_d2_rows(xyz, a, min(a + BLOCK, n)) < r2).sum(1)             # strict
    return out


def rad_mask(xyz, r, m):
    return radius_count(xyz, r) > m


def denoise(xyz, sor=None, rad=None):
    """sor = (k, s) or None, rad = (r, m) or None: the statistical filter first, the radius filter on its survivors."""
    xyz = np.asarray(xyz, dtype=np.float64)[:, :3]
    keep = np.ones(len(xyz), dtype=bool)
    if sor is not None:
        keep = sor_mask(xyz, *sor)
    if rad is not None:
        rows = np.flatnonzero(keep)
        keep = np.zeros(len(xyz), dtype=bool)
        keep[rows[rad_mask(xyz[rows], *rad)]] = True
    return keep
