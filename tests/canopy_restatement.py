"""The canopy height model of DESIGN §22 stated a second time, in numpy float64 with plain operators, walking the cloud row by row and the
grids cell by cell.  It imports nothing from the package: the tests hold csrc/tl_canopy.hip and util/canopy.py against it.

canopy_model(xyz, h, labels=None, **params) takes the height above ground of every row as it is (NaN: no ground under the row) and
returns a dict: both grids (ix0, iy0, nx, ny and metric_ix0 ...), n, top, owner, state, chm, tops_mask, tops (i, j, x, y, h, owner),
tops_per_tree (with labels), metric_n, metric_n_veg, cover, h_max, h_mean, h_sd, percentiles [ny, nx, P], layers [ny, nx, L],
n_no_ground, n_clipped.  Coordinates stay in the frame they come in."""
import math

import numpy as np

DEFAULTS = dict(cell=0.5, pit_depth=2.0, pit_min_neighbours=5, top_window=4, top_min_height=5.0, metric_cell=10.0, cutoff=2.0,
                percentiles=(25, 50, 75, 95, 99), layer=1.0, max_layers=64)
MAX_SIDE, MAX_CELLS = 32768, 1 << 26


def grid_of(x, y, c):
    """ix0, iy0, nx, ny of the grid of edge c over all rows (0, 0, 0, 0 without rows)."""
    if len(x) == 0:
        return 0, 0, 0, 0
    c = np.float64(c)
    ix0, iy0 = int(np.floor(np.min(x) / c)), int(np.floor(np.min(y) / c))
    nx, ny = int(np.floor(np.max(x) / c)) - ix0 + 1, int(np.floor(np.max(y) / c)) - iy0 + 1
    if nx > MAX_SIDE or ny > MAX_SIDE or nx * ny > MAX_CELLS:
        raise ValueError(f"{nx} x {ny} cells of {c} m")
    return ix0, iy0, nx, ny


def median_of_neighbours(top, j, i):
    """(k, m): the number of non-NaN values among the 8 neighbours of cell (j, i) inside the grid, and their median (NaN for k = 0)."""
    ny, nx = top.shape
    v = []
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            jj, ii = j + dj, i + di
            if (dj == 0 and di == 0) or jj < 0 or jj >= ny or ii < 0 or ii >= nx or np.isnan(top[jj, ii]):
                continue
            v.append(top[jj, ii])
    v.sort()
    k = len(v)
    if k == 0:
        return 0, np.float64("nan")
    if k % 2 == 1:
        return k, v[k // 2]
    return k, (v[k // 2 - 1] + v[k // 2]) / np.float64(2.0)


def canopy_model(xyz, h, labels=None, **params):
    for k in params:
        if k not in DEFAULTS:
            raise ValueError(f"unknown parameter {k!r}")
    p = dict(DEFAULTS, **params)
    xyz = np.asarray(xyz)
    x, y = np.asarray(xyz[:, 0], np.float64), np.asarray(xyz[:, 1], np.float64)
    h = np.asarray(h, np.float64) + np.float64(0.0)                      # -0.0 counts as 0.0
    n_rows = len(x)
    if not (np.isfinite(x).all() and np.isfinite(y).all()) or np.isinf(h).any():
        raise ValueError("a coordinate or a height is not finite")
    lab = None if labels is None else np.asarray(labels, np.int64)
    out = {}

    # ---- step A: cell maxima, rows per cell, owners
    c = np.float64(p["cell"])
    ix0, iy0, nx, ny = grid_of(x, y, c)
    n = np.zeros((ny, nx), np.int32)
    top = np.full((ny, nx), np.nan)
    owner = np.full((ny, nx), -1, np.int32)
    no_ground = 0
    for r in range(n_rows):
        if np.isnan(h[r]):
            no_ground += 1
            continue
        i, j = int(np.floor(x[r] / c)) - ix0, int(np.floor(y[r] / c)) - iy0
        n[j, i] += 1
        if np.isnan(top[j, i]) or h[r] > top[j, i]:
            top[j, i] = h[r]
    if lab is not None:
        for r in range(n_rows):
            if np.isnan(h[r]):
                continue
            i, j = int(np.floor(x[r] / c)) - ix0, int(np.floor(y[r] / c)) - iy0
            if h[r] == top[j, i] and lab[r] > owner[j, i]:
                owner[j, i] = lab[r]

    # ---- step B: pits and holes, against the raw maxima
    chm = np.full((ny, nx), np.nan)
    state = np.zeros((ny, nx), np.uint8)
    for j in range(ny):
        for i in range(nx):
            k, m = median_of_neighbours(top, j, i)
            enough = k >= p["pit_min_neighbours"]
            if n[j, i] > 0:
                if enough and m - top[j, i] > np.float64(p["pit_depth"]):
                    chm[j, i], state[j, i] = m, 2
                else:
                    chm[j, i], state[j, i] = top[j, i], 1
            elif enough:
                chm[j, i], state[j, i] = m, 3

    # ---- step C: tree tops
    w = int(p["top_window"])
    mask = np.zeros((ny, nx), np.uint8)
    for j in range(ny):
        for i in range(nx):
            v = chm[j, i]
            if np.isnan(v) or not v >= np.float64(p["top_min_height"]):
                continue
            is_top = True
            for jj in range(max(j - w, 0), min(j + w, ny - 1) + 1):
                for ii in range(max(i - w, 0), min(i + w, nx - 1) + 1):
                    o = chm[jj, ii]
                    if o > v or (o == v and jj * nx + ii < j * nx + i):
                        is_top = False
            mask[j, i] = 1 if is_top else 0
    tj, ti = np.nonzero(mask)                                            # row-major order
    tops = dict(i=ti.astype(np.int64), j=tj.astype(np.int64), x=((ix0 + ti) + np.float64(0.5)) * c, y=((iy0 + tj) + np.float64(0.5)) * c,
                h=chm[tj, ti], owner=owner[tj, ti])
    out.update(ix0=ix0, iy0=iy0, nx=nx, ny=ny, n=n, top=top, owner=owner, chm=chm, state=state, tops_mask=mask, tops=tops,
               n_no_ground=no_ground)
    if lab is not None:
        T = max(int(lab.max()), 0) if n_rows else 0
        per = np.zeros(T, np.int32)
        for o in tops["owner"]:
            if 1 <= o <= T:
                per[o - 1] += 1
        out["tops_per_tree"] = per

    # ---- step D: area metrics
    mc = np.float64(p["metric_cell"])
    mx0, my0, mnx, mny = grid_of(x, y, mc)
    qs = [np.float64(q) for q in p["percentiles"]]
    layer = np.float64(p["layer"])
    finite = h[~np.isnan(h)]
    L = 1
    if len(finite):
        L = max(1, min(int(p["max_layers"]), int(np.floor(np.max(finite) / layer)) + 1))
    cutoff = np.float64(p["cutoff"])
    rows = [[[] for _ in range(mnx)] for _ in range(mny)]
    for r in range(n_rows):
        if not np.isnan(h[r]):
            rows[int(np.floor(y[r] / mc)) - my0][int(np.floor(x[r] / mc)) - mx0].append(h[r])
    m_n, m_veg = np.zeros((mny, mnx), np.int32), np.zeros((mny, mnx), np.int32)
    cover, h_max, h_mean, h_sd = (np.full((mny, mnx), np.nan) for _ in range(4))
    pct = np.full((mny, mnx, len(qs)), np.nan)
    layers = np.zeros((mny, mnx, L), np.int32)
    clipped = 0
    for j in range(mny):
        for i in range(mnx):
            hs = sorted(rows[j][i])
            m_n[j, i] = len(hs)
            if not hs:
                continue
            for v in hs:
                l = 0 if v < 0 else min(int(np.floor(v / layer)), L - 1)
                layers[j, i, l] += 1
                if v >= np.float64(L) * layer:
                    clipped += 1
            veg = [v for v in hs if v > cutoff]
            m = len(veg)
            m_veg[j, i] = m
            cover[j, i] = np.float64(m) / np.float64(len(hs))
            h_max[j, i] = hs[-1]
            if m == 0:
                continue
            mean = math.fsum(veg) / np.float64(m)                        # the exactly rounded sum: the device's order is within the bound of it
            h_mean[j, i] = mean
            h_sd[j, i] = np.sqrt(math.fsum([(v - mean) * (v - mean) for v in veg]) / np.float64(m))
            for a, q in enumerate(qs):
                pos = (q / np.float64(100.0)) * np.float64(m - 1)
                lo = np.floor(pos)
                t = pos - lo
                lo = int(lo)
                pct[j, i, a] = veg[lo] + (veg[min(lo + 1, m - 1)] - veg[lo]) * t
    out.update(metric_ix0=mx0, metric_iy0=my0, metric_nx=mnx, metric_ny=mny, metric_n=m_n, metric_n_veg=m_veg, cover=cover, h_max=h_max,
               h_mean=h_mean, h_sd=h_sd, percentiles=pct, layers=layers, n_clipped=clipped)
    return out
