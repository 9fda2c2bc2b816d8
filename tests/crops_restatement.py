"""Straightforward numpy statements of the four random-crop kernels' formulas (csrc/tl_crops.hip; reference
tree_learn/util/data_preparation.py:154-166, 571-586, 209-230, 264-289), written from the formulas and not from the kernels:
no step search, no scan.  Rotations are plain elementwise f64 products and sums (numpy does not fuse them), the same
operations the kernels perform with contraction off."""
import numpy as np


def occupancy(xy, x_steps, y_steps, x_dim, y_dim):
    """cell (i, j) = 1 when some point has x_steps[i] < x <= x_steps[i+1] and y_steps[j] < y <= y_steps[j+1]."""
    x = xy[:, 0].astype(np.float64); y = xy[:, 1].astype(np.float64)
    ix = np.full(len(xy), -1); iy = np.full(len(xy), -1)
    for i in range(x_dim):
        ix[(x > x_steps[i]) & (x <= x_steps[i + 1])] = i
    for j in range(y_dim):
        iy[(y > y_steps[j]) & (y <= y_steps[j + 1])] = j
    grid = np.zeros((x_dim, y_dim), np.uint8)
    ok = (ix >= 0) & (iy >= 0)
    grid[ix[ok], iy[ok]] = 1
    return grid


def fill(raw, how_far_fill, min_percent):
    out = raw.copy()
    X, Y = raw.shape
    for i in range(X):
        for j in range(Y):
            if raw[i, j]:
                continue
            win = raw[max(0, i - how_far_fill):min(X, i + how_far_fill + 1), max(0, j - how_far_fill):min(Y, j + how_far_fill + 1)]
            out[i, j] = np.float64(np.sum(win != 0)) / np.float64(win.size) >= min_percent
    return out


def rotate(s0, s1, r):
    """(s0, s1) @ r.T elementwise in f64: u = s0 r00 + s1 r01, v = s0 r10 + s1 r11."""
    return s0 * r[0, 0] + s1 * r[0, 1], s0 * r[1, 0] + s1 * r[1, 1]


def check(cell_x, cell_y, occ, centres, rinv, chunk_size, denominator, min_percent):
    """(sums f64[k], pass bool[k], band rows) over every (cell, candidate) pair; band = pairs within 1e-9 m of chunk_size / 2."""
    cx = np.repeat(cell_x, len(cell_y)); cy = np.tile(cell_y, len(cell_x)); o = occ.reshape(-1) != 0
    half = chunk_size / 2
    sums = np.empty(len(centres)); band = 0
    for k, (c, r) in enumerate(zip(centres, rinv)):
        u, v = rotate(cx - np.float64(c[0]), cy - np.float64(c[1]), r)
        d = np.maximum(np.abs(u), np.abs(v))
        sums[k] = np.float64(np.sum(o & (d <= half)))
        band += int(np.sum(np.abs(d - half) < 1e-9))
    return sums, sums / denominator > min_percent, band


def crop(xyz, centre, r, chunk_size):
    """(member bool[n], u f64[n], v f64[n], d f64[n]) of one crop: the f32 subtraction, then f64 rotation."""
    s0 = (xyz[:, 0] - np.float32(centre[0])).astype(np.float64)
    s1 = (xyz[:, 1] - np.float32(centre[1])).astype(np.float64)
    u, v = rotate(s0, s1, r)
    d = np.maximum(np.abs(u), np.abs(v))
    return d <= chunk_size / 2, u, v, d


def voxel_means(data, voxel_size):
    """The training generator's voxelization before its final rounding (data_preparation.py:60-79 with open3d's
    VoxelDownSampleAndTrace): coordinates rounded to 2 decimals, voxel = floor((p - min_bound) / voxel) with
    min_bound = -(max|p| + 100) - voxel / 2, per voxel the float64 sum of its points in input order over their number, the other
    columns of its first point.  Voxels in ascending (x, y, z) order.  Returns (means f64[M,3], other f64[M,C])."""
    data = np.asarray(data, np.float64)
    pts = np.round(data[:, :3], 2)
    vmin = -(np.max(np.abs(pts)) + 100) - 0.5 * voxel_size
    vox = np.floor((pts - vmin) / voxel_size).astype(np.int64)
    order = np.lexsort((np.arange(len(pts)), vox[:, 2], vox[:, 1], vox[:, 0]))
    sv = vox[order]
    head = np.r_[True, np.any(sv[1:] != sv[:-1], axis=1)]
    group = np.cumsum(head) - 1
    gid = np.empty(len(pts), np.int64); gid[order] = group
    sums = np.zeros((group[-1] + 1, 3))
    np.add.at(sums, gid, pts)                                   # unbuffered, in input order
    counts = np.bincount(gid).astype(np.float64)
    first = order[np.flatnonzero(head)]
    return sums / counts[:, None], data[first, 3:]
