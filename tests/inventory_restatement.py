"""Per-tree inventory of a labelled cloud, restated in numpy float64.  The yardstick of tl_tree_inventory: it walks the
cloud once per tree, imports nothing from the package and uses plain operators only, one rounding per operation.

Trees are the labels 1..T, T = max(label) (no tree if none is >= 1); labels <= 0 are ignored; a label in 1..T without rows is a tree
of n_points = 0 with NaN in every float column.  Per tree, over its rows (x, y, z widened to f64 exactly):
  z_low   = np.sort(z)[3] for more than 11 rows (rank 3, duplicates counted: the tree-base rule of tl_train_item), else min z
  z_top   = np.sort(z)[-4] for more than 11 rows, else max z;  height = z_top - z_low
  x, y, z = mean of the base rows, z <= z_low + 0.5
  slice   = rows with (z_low + slice_height) - slice_thickness / 2 <= z < (z_low + slice_height) + slice_thickness / 2 and
            u*u + v*v < dbh_max_radius * dbh_max_radius, u = x - x_pos, v = y - y_pos;  dbh_n = their number
  circle  = Kasa fit: [[Suu, Suv, Su], [Suv, Svv, Sv], [Su, Sv, n]] [a, b, c]^T = [Suw, Svw, Sw], w = u*u + v*v, by Gaussian elimination
            with partial pivoting (`solve3`); cx = a / 2, cy = b / 2, r2 = (c + cx*cx) + cy*cy; dbh = 2 sqrt(r2), dbh_x = cx + x_pos,
            dbh_y = cy + y_pos, dbh_rmse = sqrt(sum((sqrt(du*du + dv*dv) - r)^2) / dbh_n), du = u - cx, dv = v - cy.
            NaN for dbh_n < dbh_min_points, a pivot below 1e-12 x the largest matrix entry, or r2 <= 0.
  crown   = crown_cells distinct (floor(x / c), floor(y / c)); crown_area = crown_cells * (c * c); crown_diameter = 2 sqrt(area / pi)
`offset` is added to x, y, z, z_low, z_top, dbh_x, dbh_y at the end."""
import numpy as np

FLOAT_COLUMNS = ("x", "y", "z", "z_low", "z_top", "height", "dbh", "dbh_x", "dbh_y", "dbh_rmse", "crown_area", "crown_diameter")
INT_COLUMNS = ("tree_id", "n_points", "dbh_n", "crown_cells")
COLUMNS = ("tree_id", "n_points", "x", "y", "z", "z_low", "z_top", "height", "dbh", "dbh_x", "dbh_y", "dbh_n", "dbh_rmse", "crown_cells",
           "crown_area", "crown_diameter")
PIVOT_TOL = 1e-12


def solve3(A, b):
    """x of A x = b (3 x 3, f64) by Gaussian elimination with partial pivoting (first largest entry of the column), or None when a pivot
    is below PIVOT_TOL x the largest |entry| of A."""
    A = [[float(v) for v in row] for row in A]
    b = [float(v) for v in b]
    tol = PIVOT_TOL * max(abs(v) for row in A for v in row)
    for k in range(3):
        p = k
        for i in range(k + 1, 3):
            if abs(A[i][k]) > abs(A[p][k]):
                p = i
        if abs(A[p][k]) < tol:
            return None
        A[k], A[p] = A[p], A[k]
        b[k], b[p] = b[p], b[k]
        for i in range(k + 1, 3):
            f = A[i][k] / A[k][k]
            for j in range(k + 1, 3):
                A[i][j] = A[i][j] - f * A[k][j]
            b[i] = b[i] - f * b[k]
    x2 = b[2] / A[2][2]
    x1 = (b[1] - A[1][2] * x2) / A[1][1]
    x0 = ((b[0] - A[0][1] * x1) - A[0][2] * x2) / A[0][0]
    return x0, x1, x2


def tree_inventory(coords, labels, *, slice_height=1.3, slice_thickness=0.2, dbh_max_radius=1.0, dbh_min_points=8, crown_cell=0.25,
                   offset=None):
    c = np.asarray(coords)
    xyz = np.asarray(c[:, :3], np.float64)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    assert len(xyz) == len(lab)
    T = int(lab.max()) if len(lab) and lab.max() >= 1 else 0
    out = {k: np.full(T, np.nan) for k in FLOAT_COLUMNS}
    out.update({k: np.zeros(T, np.int64) for k in INT_COLUMNS})
    out["tree_id"] = np.arange(1, T + 1, dtype=np.int64)
    sh, half, cell = np.float64(slice_height), np.float64(slice_thickness) / 2, np.float64(crown_cell)
    r2max = np.float64(dbh_max_radius) * np.float64(dbh_max_radius)
    for t in range(1, T + 1):
        p = xyz[lab == t]
        n = len(p)
        i = t - 1
        out["n_points"][i] = n
        if n == 0:
            continue
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        zs = np.sort(z)
        z_low, z_top = (zs[3], zs[-4]) if n > 11 else (zs[0], zs[-1])
        base = z <= z_low + 0.5
        nb = np.float64(base.sum())
        px, py, pz = x[base].sum() / nb, y[base].sum() / nb, z[base].sum() / nb
        out["z_low"][i], out["z_top"][i], out["height"][i] = z_low, z_top, z_top - z_low
        out["x"][i], out["y"][i], out["z"][i] = px, py, pz
        u, v = x - px, y - py
        w = u * u + v * v
        m = (z >= (z_low + sh) - half) & (z < (z_low + sh) + half) & (w < r2max)
        k = int(m.sum())
        out["dbh_n"][i] = k
        if k >= dbh_min_points and k > 0:
            u, v, w = u[m], v[m], w[m]
            sol = solve3([[(u * u).sum(), (u * v).sum(), u.sum()], [(u * v).sum(), (v * v).sum(), v.sum()], [u.sum(), v.sum(), np.float64(k)]],
                         [(u * w).sum(), (v * w).sum(), w.sum()])
            if sol is not None:
                cx, cy = sol[0] / 2, sol[1] / 2
                rr = (sol[2] + cx * cx) + cy * cy
                if rr > 0:
                    r = np.sqrt(rr)
                    du, dv = u - cx, v - cy
                    e = np.sqrt(du * du + dv * dv) - r
                    out["dbh"][i], out["dbh_x"][i], out["dbh_y"][i] = 2 * r, cx + px, cy + py
                    out["dbh_rmse"][i] = np.sqrt((e * e).sum() / np.float64(k))
        cells = np.unique(np.stack([np.floor(x / cell), np.floor(y / cell)], 1).astype(np.int64), axis=0)
        out["crown_cells"][i] = len(cells)
    finish(out, crown_cell, offset)
    return {k: out[k] for k in COLUMNS}


def finish(out, crown_cell, offset):
    """Crown area and diameter from the cell counts (NaN for an empty tree), then the offset."""
    cell = np.float64(crown_cell)
    area = out["crown_cells"].astype(np.float64) * (cell * cell)
    area[out["n_points"] == 0] = np.nan
    out["crown_area"] = area
    out["crown_diameter"] = 2 * np.sqrt(area / np.pi)
    if offset is not None:
        o = np.asarray(offset, np.float64).reshape(3)
        for k, a in (("x", 0), ("y", 1), ("z", 2), ("z_low", 2), ("z_top", 2), ("dbh_x", 0), ("dbh_y", 1)):
            out[k] = out[k] + o[a]
