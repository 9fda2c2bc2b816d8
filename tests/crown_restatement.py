"""Crown structure of a labelled cloud, restated in numpy float64.  The yardstick of tl_crown_voxel_keys and
tl_crown_structure: it walks the cloud once per tree and layer, imports nothing from the package and uses plain operators only, one
rounding per operation.

Per tree t (label t + 1) of the inventory (inventory_restatement.tree_inventory; terrain_restatement.tree_inventory with a terrain): the
position (px, py), z_top and the reference height z_ref = z_ground with a terrain, z_low without one.  H = z_top - z_ref.
  layers   L_t = min(floor(H / layer) + 1, max_layers), 0 unless H >= 0 (a NaN H, an empty tree).  A row of the tree is in layer
           l = floor((z - z_ref) / layer) when 0 <= l < L_t, else in none; its cell is (ix, iy) = (floor(x / cell), floor(y / cell)).
           n[l] = the layer's rows, cells[l] = its distinct (ix, iy), h[l] = l * layer.  L = the largest L_t: the profile width.
  base     l_min = the smallest l with l * layer >= min_height (counted up from 0, at most max_layers).  No crown when l_min >= L_t or no
           layer >= l_min holds a row.  Else cells_max = max cells[l] over l_min <= l < L_t, l_w the lowest l that reaches it; l_b = l_w,
           gap = 0, then for l = l_w - 1 down to l_min: cells[l] * 100 >= base_percent * cells_max (integers): l_b = l, gap = 0; else
           gap += 1 and the walk stops at gap > max_gap.
  columns  crown_layers = L_t; crown_base_h = l_b * layer; crown_length = H - crown_base_h; crown_ratio = crown_length / H;
           crown_widest_h = (l_w + 0.5) * layer; crown_voxels = sum of cells[l] over l >= l_b; crown_volume = crown_voxels * ((cell * cell)
           * layer); crown_proj_cells = c, the distinct (ix, iy) of the rows in layers >= l_b; crown_proj_area = c * (cell * cell);
           crown_x = ((sum(ix) / c) + 0.5) * cell over those cells (an integer sum), crown_y likewise; crown_offset = sqrt(dx*dx + dy*dy),
           dx = crown_x - px, dy = crown_y - py.
  sectors  per projection cell u = (ix + 0.5) * cell - px, v = (iy + 0.5) * cell - py, w = u*u + v*v; its sector by comparisons: u > 0,
           v >= 0: v < u ? 0 : 1; u <= 0, v > 0: -u < v ? 2 : 3; u < 0, v <= 0: -v < -u ? 4 : 5; u >= 0, v < 0: u < -v ? 6 : 7; u = v = 0: 0.
           radii[s] = sqrt(max w) of sector s, 0.0 for an empty one; crown_radius_max = the largest; crown_radius_mean = their sum in
           sector order / 8.0.  A tree without a crown has NaN in every float column and in its radii, 0 in crown_voxels and
           crown_proj_cells; its n and cells are still those of its layers.
  errors   ValueError when a row of a tree has a coordinate that is not finite, or a row in a layer has ix - floor(px / cell) (or the
           same in y) outside -4096 .. 4095: the key of the kernels cannot hold it.
`offset` is added to crown_x, crown_y at the end; heights are relative and get none.

Margins.  The integer columns depend on float decisions only through the inputs that differ between implementations: px, py (a float sum
whose order differs) and, with a terrain, z_ref = z_ground (sampled, equal to 1e-9).  `margins` holds the smallest distance of each kind
(inf where no such decision was taken); a fixture is admissible only when min(margins.values()) > 1e-6.  Kinds: sector (min(|u|, |v|,
||u| - |v||) over the projection cells); layer (the distance of (z - z_ref) / layer of a tree's rows, and of H / layer, from an integer;
tree_crowns sets it to inf without a terrain, where z_ref = z_low and z_top are ranks of the rows' own z: the same bits everywhere);
anchor (the distance of px / cell, py / cell from an integer, for a tree with a row on or next to the edge of the key's cell range:
there floor(px / cell) decides the error)."""
import numpy as np

import inventory_restatement as inv_ref

CROWN_DEFAULTS = dict(layer=0.5, cell=0.25, max_layers=256, min_height=1.0, base_percent=10, max_gap=1)
CROWN_COLUMNS = ("crown_layers", "crown_base_h", "crown_length", "crown_ratio", "crown_widest_h", "crown_voxels", "crown_volume",
                 "crown_proj_cells", "crown_proj_area", "crown_x", "crown_y", "crown_offset", "crown_radius_max", "crown_radius_mean")
CROWN_INT = ("crown_layers", "crown_voxels", "crown_proj_cells")
PROFILE_KEYS = ("h", "n", "cells", "radii")
MARGIN_KINDS = ("sector", "layer", "anchor")
MIN_MARGIN = 1e-6
CELL_HALF = 4096


def sector(u, v):
    if u > 0 and v >= 0:
        return 0 if v < u else 1
    if u <= 0 and v > 0:
        return 2 if -u < v else 3
    if u < 0 and v <= 0:
        return 4 if -v < -u else 5
    if u >= 0 and v < 0:
        return 6 if u < -v else 7
    return 0


def lowest_layer(p):
    """l_min: the smallest l with l * layer >= min_height, counted up from 0 and at most max_layers."""
    l = 0
    while l < int(p["max_layers"]) and np.float64(l) * np.float64(p["layer"]) < np.float64(p["min_height"]):
        l += 1
    return l


def crown_structure(coords, labels, px, py, z_ref, z_top, offset=None, **params):
    """The crown columns of the trees 1 .. T = len(px) from their per-tree inputs.  Returns a dict: CROWN_COLUMNS (arrays of length T),
    "crown_profile" (h f64, n, cells i64 [T, L] and radii f64 [T, 8]), "L_t" (i64 [T]) and "margins"."""
    p = dict(CROWN_DEFAULTS)
    for k, v in params.items():
        if k not in CROWN_DEFAULTS:
            raise ValueError(f"unknown crown parameter {k!r}")
        p[k] = v
    xyz = np.asarray(np.asarray(coords)[:, :3], np.float64)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    px, py, z_ref, z_top = (np.asarray(a, np.float64).reshape(-1) for a in (px, py, z_ref, z_top))
    T = len(px)
    layer, cell = np.float64(p["layer"]), np.float64(p["cell"])
    max_layers, base_percent, max_gap = int(p["max_layers"]), int(p["base_percent"]), int(p["max_gap"])
    margins = {k: np.inf for k in MARGIN_KINDS}

    def note(kind, v):
        v = float(np.min(v)) if np.size(v) else np.inf
        if v < margins[kind]:
            margins[kind] = v

    H = z_top - z_ref
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.minimum(np.floor(H / layer) + 1.0, np.float64(max_layers))
        L_t = np.where(H >= 0, q, 0.0).astype(np.int64) if T else np.zeros(0, np.int64)
    L = int(L_t.max()) if T else 0
    l_min = lowest_layer(p)
    prof = dict(h=np.full((T, L), np.nan), n=np.zeros((T, L), np.int64), cells=np.zeros((T, L), np.int64), radii=np.full((T, 8), np.nan))
    out = {k: (np.zeros(T, np.int64) if k in CROWN_INT else np.full(T, np.nan)) for k in CROWN_COLUMNS}
    out["crown_layers"] = L_t.copy()

    for t in range(T):
        rows = xyz[lab == t + 1]
        if len(rows) and not np.isfinite(rows).all():
            raise ValueError(f"tree {t + 1}: a coordinate is not finite")
        Lt = int(L_t[t])
        if Lt == 0:
            continue
        prof["h"][t, :Lt] = np.arange(Lt, dtype=np.float64) * layer
        x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
        ql = (z - z_ref[t]) / layer
        near = (ql >= -1.0) & (ql <= Lt + 1.0)
        note("layer", np.abs(ql - np.rint(ql))[near])
        note("layer", abs(H[t] / layer - np.rint(H[t] / layer)) if H[t] / layer < max_layers + 1 else np.inf)
        fl = np.floor(ql)
        inl = (fl >= 0) & (fl < Lt)
        l = fl[inl].astype(np.int64)
        ix, iy = np.floor(x[inl] / cell).astype(np.int64), np.floor(y[inl] / cell).astype(np.int64)
        bx, by = int(np.floor(px[t] / cell)), int(np.floor(py[t] / cell))
        rel = np.concatenate([ix - bx, iy - by])
        if rel.size:
            if rel.min() <= -CELL_HALF or rel.max() >= CELL_HALF - 1:
                note("anchor", min(abs(px[t] / cell - np.rint(px[t] / cell)), abs(py[t] / cell - np.rint(py[t] / cell))))
            if rel.min() < -CELL_HALF or rel.max() > CELL_HALF - 1:
                raise ValueError(f"tree {t + 1}: a row lies more than {CELL_HALF} cells of {p['cell']} m from the tree's position")
        for k in range(Lt):                                                  # once per layer, by brute force
            m = l == k
            prof["n"][t, k] = int(m.sum())
            prof["cells"][t, k] = len(set(zip(ix[m].tolist(), iy[m].tolist())))
        cells = prof["cells"][t]
        if l_min >= Lt or not (cells[l_min:Lt] > 0).any():
            continue
        cmax = int(cells[l_min:Lt].max())
        l_w = l_min + int(np.argmax(cells[l_min:Lt] == cmax))
        l_b, gap = l_w, 0
        for k in range(l_w - 1, l_min - 1, -1):
            if int(cells[k]) * 100 >= base_percent * cmax:
                l_b, gap = k, 0
            else:
                gap += 1
                if gap > max_gap:
                    break
        vox = int(cells[l_b:Lt].sum())
        m = l >= l_b
        proj = sorted(set(zip(ix[m].tolist(), iy[m].tolist())))
        c = len(proj)
        sx, sy = sum(a for a, _ in proj), sum(b for _, b in proj)
        base_h = np.float64(l_b) * layer
        out["crown_base_h"][t] = base_h
        out["crown_length"][t] = H[t] - base_h
        with np.errstate(invalid="ignore", divide="ignore"):
            out["crown_ratio"][t] = (H[t] - base_h) / H[t]
        out["crown_widest_h"][t] = (np.float64(l_w) + 0.5) * layer
        out["crown_voxels"][t] = vox
        out["crown_volume"][t] = np.float64(vox) * ((cell * cell) * layer)
        out["crown_proj_cells"][t] = c
        out["crown_proj_area"][t] = np.float64(c) * (cell * cell)
        cx = ((np.float64(sx) / np.float64(c)) + 0.5) * cell
        cy = ((np.float64(sy) / np.float64(c)) + 0.5) * cell
        out["crown_x"][t], out["crown_y"][t] = cx, cy
        dx, dy = cx - px[t], cy - py[t]
        out["crown_offset"][t] = np.sqrt(dx * dx + dy * dy)
        wmax = [-1.0] * 8
        for a, b in proj:
            u, v = (np.float64(a) + 0.5) * cell - px[t], (np.float64(b) + 0.5) * cell - py[t]
            w = u * u + v * v
            note("sector", min(abs(u), abs(v), abs(abs(u) - abs(v))))
            s = sector(u, v)
            if w > wmax[s]:
                wmax[s] = w
        r = [np.sqrt(np.float64(w)) if w >= 0 else np.float64(0.0) for w in wmax]
        prof["radii"][t] = r
        out["crown_radius_max"][t] = max(r)
        rs = np.float64(0.0)
        for v in r:
            rs = rs + v
        out["crown_radius_mean"][t] = rs / 8.0

    if offset is not None:
        o = np.asarray(offset, np.float64).reshape(3)
        out["crown_x"], out["crown_y"] = out["crown_x"] + o[0], out["crown_y"] + o[1]
    out["crown_profile"] = prof
    out["L_t"] = L_t
    out["margins"] = margins
    return out


def tree_crowns(coords, labels, terrain=None, offset=None, crown_cfg=None, **inventory_params):
    """The inventory of the restatements (the sixteen columns, and the eight ground columns with a terrain: a terrain_restatement.terrain_model
    dict in the frame of coords) followed by CROWN_COLUMNS, "crown_profile", "L_t" and "margins"."""
    if terrain is None:
        base = inv_ref.tree_inventory(coords, labels, **inventory_params)     # the frame of coords: no offset yet
        z_ref = base["z_low"]
        full = base if offset is None else inv_ref.tree_inventory(coords, labels, offset=offset, **inventory_params)
    else:
        import terrain_restatement as ter_ref
        base = ter_ref.tree_inventory(coords, labels, terrain, **inventory_params)
        z_ref = base["z_ground"]
        full = base if offset is None else ter_ref.tree_inventory(coords, labels, terrain, offset=offset, **inventory_params)
    cr = crown_structure(coords, labels, base["x"], base["y"], z_ref, base["z_top"], offset=offset, **(crown_cfg or {}))
    if terrain is None:
        cr["margins"]["layer"] = np.inf      # z_low and z_top are ranks of the rows' own z: the layer of a row is the same bits everywhere
    res = dict(full)
    res.update(cr)
    return res
