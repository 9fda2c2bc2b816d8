"""Terrain model of a labelled cloud, restated in numpy float64.  The yardstick of tl_dtm_min, tl_dtm_filter, tl_dtm_fill,
tl_dtm_sample and tl_tree_ground: it imports nothing from the package and uses plain operators only, one rounding per operation.

Candidates are the rows with label == 0 (every row without labels).  With c = cell:
  grid     spans all rows: ix0 = floor(xmin / c), nx = floor(xmax / c) - ix0 + 1, the same in y; a row's cell is (floor(x / c) - ix0,
           floor(y / c) - iy0); row-major [ny, nx]; N = 0 gives an empty grid
  step A   zmin[j, i] = the lowest candidate z of the cell; n_candidates[j, i] = their number; no candidate: empty (state 0)
  step B   p with a minimum is rejected (state 2) when another q with a minimum within Chebyshev distance `window` has
           zmin[p] - zmin[q] > max_slope * (c * sqrt(di*di + dj*dj)) + step_tol -- against the raw minima, strict; else ground (state 1)
  step C   every cell that is not ground: the first rho in 1 .. fill_radius whose Chebyshev window holds a ground cell gives
           sum(w z) / sum(w) over that window's ground cells in row-major order, w = 1 / (di*di + dj*dj); state 3 (was empty) or 4 (was
           rejected); no such rho: NaN, state kept
  sampling u = x / c - (ix0 + 0.5), i0 = floor(u), fx = u - i0, i0 and i0 + 1 clamped to 0 .. nx - 1, the same in y; four finite
           corners: (g00 (1 - fx) + g10 fx) (1 - fy) + (g01 (1 - fx) + g11 fx) fy; else the value of the cell that contains the point
           (indices clamped), NaN included
  trees    z_ground = ground_at(x, y) of the §16 position; height_ag = z_top - z_ground; base_gap = z_low - z_ground; dbh_ag* = the §16
           slice, fit and NaN rules with z_ground in place of z_low; all NaN and dbh_ag_n = 0 when z_ground is NaN; `offset` is added
           to z_ground, dbh_ag_x, dbh_ag_y at the end."""
import numpy as np

import inventory_restatement as inv

GROUND_COLUMNS = ("z_ground", "height_ag", "base_gap", "dbh_ag", "dbh_ag_x", "dbh_ag_y", "dbh_ag_n", "dbh_ag_rmse")
EMPTY, GROUND, REJECTED, FILLED_EMPTY, FILLED_REJECTED = 0, 1, 2, 3, 4


def terrain_model(coords, labels=None, *, cell=0.5, max_slope=1.0, step_tol=0.2, window=2, fill_radius=20):
    """dict: ix0, iy0, nx, ny, cell, z f64[ny, nx], state u8[ny, nx], n_candidates i32[ny, nx], zmin f64[ny, nx] (step A, NaN = empty)."""
    xyz = np.asarray(np.asarray(coords)[:, :3], np.float64)
    if not np.isfinite(xyz).all():
        raise ValueError("a coordinate is not finite")
    c, ms, tol = np.float64(cell), np.float64(max_slope), np.float64(step_tol)
    if len(xyz) == 0:
        return dict(ix0=0, iy0=0, nx=0, ny=0, cell=c, z=np.zeros((0, 0)), state=np.zeros((0, 0), np.uint8), n_candidates=np.zeros((0, 0), np.int32),
                    zmin=np.zeros((0, 0)))
    cx, cy = np.floor(xyz[:, 0] / c).astype(np.int64), np.floor(xyz[:, 1] / c).astype(np.int64)
    ix0, iy0 = int(cx.min()), int(cy.min())
    nx, ny = int(cx.max()) - ix0 + 1, int(cy.max()) - iy0 + 1
    cand = np.ones(len(xyz), bool) if labels is None else np.asarray(labels).astype(np.int64).reshape(-1) == 0
    flat = ((cy - iy0) * nx + (cx - ix0))[cand]
    low = np.full(ny * nx, np.inf)
    np.minimum.at(low, flat, xyz[cand, 2])
    count = np.bincount(flat, minlength=ny * nx).astype(np.int32).reshape(ny, nx)
    has = count > 0
    zmin = np.where(has, low.reshape(ny, nx), np.nan)

    # step B against the raw minima
    rejected = np.zeros((ny, nx), bool)
    w = int(window)
    pad = np.full((ny + 2 * w, nx + 2 * w), np.nan)
    pad[w:w + ny, w:w + nx] = zmin
    with np.errstate(invalid="ignore"):
        for dj in range(-w, w + 1):
            for di in range(-w, w + 1):
                if di == 0 and dj == 0:
                    continue
                q = pad[w + dj:w + dj + ny, w + di:w + di + nx]
                d = c * np.sqrt(np.float64(di * di + dj * dj))
                rejected |= (zmin - q) > ms * d + tol                  # NaN (no minimum on either side) compares false
    state = np.where(has, np.where(rejected, REJECTED, GROUND), EMPTY).astype(np.uint8)
    ground = state == GROUND

    # step C from the ground cells only
    z = np.where(ground, zmin, np.nan)
    out_state = state.copy()
    for j, i in zip(*np.nonzero(~ground)):
        for rho in range(1, int(fill_radius) + 1):
            j0, j1, i0, i1 = max(j - rho, 0), min(j + rho, ny - 1), max(i - rho, 0), min(i + rho, nx - 1)
            if not ground[j0:j1 + 1, i0:i1 + 1].any():
                if j0 == 0 and i0 == 0 and j1 == ny - 1 and i1 == nx - 1:
                    break                                              # the window is the whole grid: no ground cell anywhere
                continue
            sw, swz = np.float64(0.0), np.float64(0.0)
            for jj in range(j0, j1 + 1):                               # row-major
                for ii in range(i0, i1 + 1):
                    if ground[jj, ii]:
                        wt = np.float64(1.0) / np.float64((ii - i) * (ii - i) + (jj - j) * (jj - j))
                        swz = swz + wt * zmin[jj, ii]
                        sw = sw + wt
            z[j, i] = swz / sw
            out_state[j, i] = FILLED_EMPTY if state[j, i] == EMPTY else FILLED_REJECTED
            break
    return dict(ix0=ix0, iy0=iy0, nx=nx, ny=ny, cell=c, z=z, state=out_state, n_candidates=count, zmin=zmin)


def ground_at(t, x, y):
    """The ground under (x, y) (arrays or scalars), f64."""
    x, y = np.atleast_1d(np.asarray(x, np.float64)), np.atleast_1d(np.asarray(y, np.float64))
    out = np.full(x.shape, np.nan)
    nx, ny, c, g = t["nx"], t["ny"], np.float64(t["cell"]), t["z"]
    ok = np.isfinite(x) & np.isfinite(y)
    if nx == 0 or ny == 0 or not ok.any():
        return out
    x, y = x[ok], y[ok]
    u, v = x / c - (np.float64(t["ix0"]) + 0.5), y / c - (np.float64(t["iy0"]) + 0.5)
    fu, fv = np.floor(u), np.floor(v)
    fx, fy = u - fu, v - fv
    clamp = lambda a, n: np.clip(a, 0, n - 1).astype(np.int64)        # noqa: E731
    a0, a1, b0, b1 = clamp(fu, nx), clamp(fu + 1.0, nx), clamp(fv, ny), clamp(fv + 1.0, ny)
    g00, g10, g01, g11 = g[b0, a0], g[b0, a1], g[b1, a0], g[b1, a1]
    bil = (g00 * (1.0 - fx) + g10 * fx) * (1.0 - fy) + (g01 * (1.0 - fx) + g11 * fx) * fy
    own = g[clamp(np.floor(y / c) - np.float64(t["iy0"]), ny), clamp(np.floor(x / c) - np.float64(t["ix0"]), nx)]
    finite = np.isfinite(g00) & np.isfinite(g10) & np.isfinite(g01) & np.isfinite(g11)
    out[ok] = np.where(finite, bil, own)
    return out


def height_above_ground(t, coords):
    xyz = np.asarray(np.asarray(coords)[:, :3], np.float64)
    return xyz[:, 2] - ground_at(t, xyz[:, 0], xyz[:, 1])


def tree_inventory(coords, labels, t, *, slice_height=1.3, slice_thickness=0.2, dbh_max_radius=1.0, dbh_min_points=8, crown_cell=0.25,
                   offset=None):
    """The 16 columns of inventory_restatement.tree_inventory followed by GROUND_COLUMNS, for the terrain t in the frame of coords."""
    kw = dict(slice_height=slice_height, slice_thickness=slice_thickness, dbh_max_radius=dbh_max_radius, dbh_min_points=dbh_min_points,
              crown_cell=crown_cell)
    base = inv.tree_inventory(coords, labels, **kw)                    # the frame of coords: no offset yet
    xyz = np.asarray(np.asarray(coords)[:, :3], np.float64)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    T = len(base["tree_id"])
    out = {k: np.full(T, np.nan) for k in GROUND_COLUMNS}
    out["dbh_ag_n"] = np.zeros(T, np.int64)
    sh, half = np.float64(slice_height), np.float64(slice_thickness) / 2
    r2max = np.float64(dbh_max_radius) * np.float64(dbh_max_radius)
    zg_all = ground_at(t, base["x"], base["y"]) if T else np.zeros(0)
    for i in range(T):
        zg = zg_all[i]
        if base["n_points"][i] == 0 or np.isnan(zg):
            continue
        p = xyz[lab == i + 1]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        px, py = base["x"][i], base["y"][i]
        out["z_ground"][i], out["height_ag"][i], out["base_gap"][i] = zg, base["z_top"][i] - zg, base["z_low"][i] - zg
        # the slice and fit of inventory_restatement.tree_inventory, z_ground in place of z_low
        u, v = x - px, y - py
        w = u * u + v * v
        m = (z >= (zg + sh) - half) & (z < (zg + sh) + half) & (w < r2max)
        k = int(m.sum())
        out["dbh_ag_n"][i] = k
        if k >= dbh_min_points and k > 0:
            u, v, w = u[m], v[m], w[m]
            sol = inv.solve3([[(u * u).sum(), (u * v).sum(), u.sum()], [(u * v).sum(), (v * v).sum(), v.sum()], [u.sum(), v.sum(), np.float64(k)]],
                             [(u * w).sum(), (v * w).sum(), w.sum()])
            if sol is not None:
                cx, cy = sol[0] / 2, sol[1] / 2
                rr = (sol[2] + cx * cx) + cy * cy
                if rr > 0:
                    r = np.sqrt(rr)
                    du, dv = u - cx, v - cy
                    e = np.sqrt(du * du + dv * dv) - r
                    out["dbh_ag"][i], out["dbh_ag_x"][i], out["dbh_ag_y"][i] = 2 * r, cx + px, cy + py
                    out["dbh_ag_rmse"][i] = np.sqrt((e * e).sum() / np.float64(k))
    if offset is not None:
        o = np.asarray(offset, np.float64).reshape(3)
        base = inv.tree_inventory(coords, labels, offset=o, **kw)
        for k, a in (("z_ground", 2), ("dbh_ag_x", 0), ("dbh_ag_y", 1)):
            out[k] = out[k] + o[a]
    res = dict(base)
    res.update({k: out[k] for k in GROUND_COLUMNS})
    return res
