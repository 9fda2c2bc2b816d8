"""Per-tree inventory of a segmented forest on the device: where each tree stands, how tall it is, its stem diameter at breast height
(DBH) and how much ground its crown covers.

    python -m treelearn_amd.util.inventory --forest labelled.npy|npz|txt|las --out trees.csv [--slice-height 1.3 ...]

The semantics are the project's own; tests/inventory_restatement.py states them in numpy float64.  Trees are the labels 1..T with
T = max(label); labels <= 0 are ignored; a label in 1..T without rows is a tree of n_points = 0 with NaN in every float column.

  n_points
  z_low, z_top    the 4th smallest / 4th largest z (rank 3, duplicates counted: the tree-base rule of tl_train_item) for more than 11 rows,
                  else the minimum / maximum;  height = z_top - z_low
  x, y, z         position: the float64 mean of the base rows, z <= z_low + 0.5 (the reference's position rule evaluated in float64; not
                  bit-equal to the dataset's float32 np.mean)
  dbh, dbh_x, dbh_y, dbh_n, dbh_rmse
                  algebraic (Kasa) circle fit of the rows with z_low + slice_height - slice_thickness / 2 <= z < z_low + slice_height +
                  slice_thickness / 2 within dbh_max_radius (horizontally) of the position: diameter, centre, rows used, rms radial residual.
                  NaN (dbh_n still reported) for fewer than dbh_min_points rows, collinear or coincident rows, or a non-positive r^2.
  crown_cells, crown_area, crown_diameter
                  distinct (floor(x / c), floor(y / c)) cells of the tree's rows, c = crown_cell; area = cells * c^2; the diameter of the
                  circle of that area.  The cells are those of the frame the coordinates are given in.

One stable sort of the labels (torch) puts every tree's rows in one contiguous range; csrc/tl_inventory.hip gathers them as float64
(tl_inventory_gather), runs one workgroup per tree (tl_tree_inventory) and counts the distinct crown keys (tl_crown_keys, a torch sort,
tl_crown_count).  There is no CPU fallback.

With a terrain (util.terrain) the eight GROUND_COLUMNS follow the sixteen: z_ground (the terrain sampled at the tree's x, y),
height_ag = z_top - z_ground, base_gap = z_low - z_ground, and dbh_ag, dbh_ag_x, dbh_ag_y, dbh_ag_n, dbh_ag_rmse: the slice fit above with
z_ground in place of z_low (tl_tree_ground).  NaN, and dbh_ag_n = 0, where the terrain has no value under the tree.

With stem=True (util.stem) the seven STEM_COLUMNS follow them, and the key "stem_profile" holds the circle of every slab
along every stem: the stage runs on the same label-sorted rows and tree table, heights from z_ground with a terrain, else from z_low.

With crown=True (util.crown) the fourteen CROWN_COLUMNS follow them, and the key "crown_profile" holds the rows and cells of
every layer of every tree and its crown radii in eight sectors: the same rows, table and reference height.

With branches=True (util.branches) the thirteen BRANCH_COLUMNS follow them, and the key "skeleton" holds the node table of
every tree's skeleton: the same rows, table and reference height.

With wood=True (util.wood; implies branches=True) the nine WOOD_COLUMNS follow them, and the key "cylinders" holds the fitted
circle, the radius and the frustum of every skeleton node.

With leafwood=True (util.leafwood) the five LEAFWOOD_COLUMNS stand after the crown group and before the branch group, and the
key "leafwood" holds the wood flag of every input row; with its `filter` the branch and wood stages read the wood rows only."""
import argparse
import csv
import sys
import time

import numpy as np

DEFAULTS = dict(slice_height=1.3, slice_thickness=0.2, dbh_max_radius=1.0, dbh_min_points=8, crown_cell=0.25)
COLUMNS = ("tree_id", "n_points", "x", "y", "z", "z_low", "z_top", "height", "dbh", "dbh_x", "dbh_y", "dbh_n", "dbh_rmse", "crown_cells",
           "crown_area", "crown_diameter")
INT_COLUMNS = ("tree_id", "n_points", "dbh_n", "crown_cells")
_TABLE = ("z_low", "z_top", "height", "x", "y", "z", "dbh", "dbh_x", "dbh_y", "dbh_rmse")          # tl_tree_inventory's table columns
_SHIFTED = (("x", 0), ("y", 1), ("z", 2), ("z_low", 2), ("z_top", 2), ("dbh_x", 0), ("dbh_y", 1))
GROUND_COLUMNS = ("z_ground", "height_ag", "base_gap", "dbh_ag", "dbh_ag_x", "dbh_ag_y", "dbh_ag_n", "dbh_ag_rmse")
_GROUND_TABLE = ("z_ground", "height_ag", "base_gap", "dbh_ag", "dbh_ag_x", "dbh_ag_y", "dbh_ag_rmse")       # tl_tree_ground's table columns
_GROUND_SHIFTED = (("z_ground", 2), ("dbh_ag_x", 0), ("dbh_ag_y", 1))
MAX_TREES = (1 << 21) - 1                                                                         # the tree field of a crown key

__all__ = ["tree_inventory", "cloud_inventory", "write_inventory", "check_params", "DEFAULTS", "COLUMNS", "GROUND_COLUMNS"]


def check_params(cfg=None, **kw):
    """The five parameters as a dict of plain numbers (defaults filled in); ValueError for an unknown name, a non-positive thickness,
    radius or cell, a non-finite height or a negative point minimum.  Touches no GPU."""
    p = dict(DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in DEFAULTS:
                raise ValueError(f"unknown inventory parameter {k!r}; expected one of {tuple(DEFAULTS)}")
            if v is not None:
                p[k] = v
    for k in ("slice_thickness", "dbh_max_radius", "crown_cell"):
        p[k] = float(p[k])
        if not (p[k] > 0 and np.isfinite(p[k])):
            raise ValueError(f"{k} must be > 0, got {p[k]!r}")
    p["slice_height"] = float(p["slice_height"])
    if not np.isfinite(p["slice_height"]):
        raise ValueError(f"slice_height must be finite, got {p['slice_height']!r}")
    if int(p["dbh_min_points"]) != p["dbh_min_points"] or int(p["dbh_min_points"]) < 0:
        raise ValueError(f"dbh_min_points must be an integer >= 0, got {p['dbh_min_points']!r}")
    p["dbh_min_points"] = int(p["dbh_min_points"])
    return p


def _offset(offset):
    if offset is None:
        return None
    import torch
    o = offset.detach().cpu().numpy() if torch.is_tensor(offset) else np.asarray(offset)
    o = np.asarray(o, np.float64).reshape(-1)
    if o.shape != (3,):
        raise ValueError(f"offset must hold 3 values, got {o.shape}")
    return o


def _device_inputs(coords, labels):
    """(coords on the device as given: f32 / f64 [N, >= 3] with unit column stride, labels i64 [N])."""
    import torch
    c = coords if torch.is_tensor(coords) else torch.from_numpy(np.asarray(coords))
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError(f"coords must have shape [N, 3] (or [N, 4], the first three columns are used), got {tuple(c.shape)}")
    if c.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"coords must be float32 or float64, got {c.dtype}")
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)).astype(np.int64, copy=False))
    lab = lab.reshape(-1)
    if lab.shape[0] != c.shape[0]:
        raise ValueError(f"mismatched lengths: {c.shape[0]} coordinates for {lab.shape[0]} labels")
    if not torch.cuda.is_available():
        raise RuntimeError("treelearn_amd.util.inventory runs on the GPU (tl_tree_inventory); there is no CPU fallback")
    c = c.to("cuda")
    if len(c) and (c.stride(1) != 1 or c.stride(0) < 3):
        c = c.contiguous()
    return c, lab.to("cuda", torch.int64).contiguous()


def tree_inventory(coords, labels, *, slice_height=1.3, slice_thickness=0.2, dbh_max_radius=1.0, dbh_min_points=8, crown_cell=0.25,
                   offset=None, stages=None, terrain=None, stem=False, stem_cfg=None, crown=False, crown_cfg=None, branches=False,
                   branch_cfg=None, wood=False, wood_cfg=None, leafwood=False, leafwood_cfg=None, leafwood_scales=None,
                   leafwood_scales_min=None, light=False, light_cfg=None):
    """coords [N, 3] float32 or float64 (a row stride of 3 or 4 elements is read in place), labels [N] integers; numpy arrays or tensors,
    on the host or the device.  Returns a dict of numpy arrays of length T = max(label), keyed by COLUMNS (tree_id = 1..T).
    `offset` (3 values) is added to x, y, z, z_low, z_top, dbh_x, dbh_y at the end -- the un-centring of segment_forest.
    `stages`: a list that receives (name, seconds) per stage, each closed by a device synchronise (tools/dev_inventory.py).
    `terrain`: a util.terrain.Terrain in the frame of `coords`; the dict then holds GROUND_COLUMNS after COLUMNS (`offset` is added to
    z_ground, dbh_ag_x, dbh_ag_y as well).
    `stem`: True adds util.stem's STEM_COLUMNS after them and "stem_profile", a dict of [T, S] arrays (h, x, y, r, rmse, n, state;
    `offset` is added to its x, y); stem_cfg holds any of util.stem's parameters.
    `crown`: True adds util.crown's CROWN_COLUMNS after them and "crown_profile", a dict of [T, L] arrays (h, n, cells) and radii [T, 8]
    (`offset` is added to crown_x, crown_y); crown_cfg holds any of util.crown's parameters.
    `branches`: True adds util.branches' BRANCH_COLUMNS after them and "skeleton", the ragged node table of every tree's skeleton
    (`offset` is added to its xyz); branch_cfg holds any of util.branches' parameters.
    `wood`: True implies branches=True and adds util.wood's WOOD_COLUMNS after the branch group and "cylinders", the fitted circle, radius
    and frustum of every skeleton node (`offset` is added to its centre); wood_cfg holds any of util.wood's parameters.
    `leafwood`: True adds util.leafwood's LEAFWOOD_COLUMNS after the crown group and "leafwood", a dict of wood u8 [N] (the wood flag of
    every input row, 0 for a label < 1) and the parameters; leafwood_cfg holds any of util.leafwood's parameters; leafwood_scales (1 to 4
    ascending radii) and leafwood_scales_min make the seed a count over scales (util.leafwood.check_scales) and are recorded
    in that dict.  With its `filter`
    (the default) the branch and wood stages read the wood rows only.
    `light`: True adds util.light's LIGHT_COLUMNS after every other column: how much sky the top of the tree sees past its neighbours
    (DESIGN §28); light_cfg holds any of util.light's parameters."""
    if light:
        from . import light as _light
        light_cfg = _light.check_params(light_cfg)                                    # before any GPU work
    if leafwood:
        from . import leafwood as _leafwood
        leafwood_cfg = _leafwood.check_params(leafwood_cfg)                           # before any GPU work
        lw_scales = _leafwood.check_scales(scales=leafwood_scales, scales_min=leafwood_scales_min)
    if wood:
        from . import wood as _wood
        wood_cfg = _wood.check_params(wood_cfg)                                       # before any GPU work
        branches = True
    if branches:
        from . import branches as _branches
        branch_cfg = _branches.check_params(branch_cfg)                               # before any GPU work
    if crown:
        from . import crown as _crown
        crown_cfg = _crown.check_params(crown_cfg)                                    # before any GPU work
    if stem:
        from . import stem as _stem
        stem_cfg = _stem.check_params(stem_cfg)                                       # before any GPU work
    p = check_params(slice_height=slice_height, slice_thickness=slice_thickness, dbh_max_radius=dbh_max_radius,
                     dbh_min_points=dbh_min_points, crown_cell=crown_cell)
    off = _offset(offset)
    import torch
    from .. import _hip
    c, lab = _device_inputs(coords, labels)
    L, dev, n = _hip.lib(), c.device, len(c)
    t0 = [time.perf_counter()]

    def mark(name):
        if stages is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            stages.append((name, now - t0[0]))
            t0[0] = now

    # one stable sort; the rows of labels >= 1 in label order
    vals, order = torch.sort(lab, stable=True)
    T = max(int(vals[-1]), 0) if n else 0
    if T > MAX_TREES:
        raise ValueError(f"largest label {T}: the crown keys hold tree ids up to {MAX_TREES}")
    edges = torch.searchsorted(vals, torch.arange(1, T + 2, dtype=torch.int64, device=dev))
    first = int(edges[0]) if T else n
    start = (edges - first).contiguous()
    kept, kept_lab = order[first:].contiguous(), vals[first:].contiguous()
    m = len(kept)
    xyz = torch.empty((m, 3), dtype=torch.float64, device=dev)
    if m:
        _hip.check(L.tl_inventory_gather(_hip.ptr(c), int(c.dtype == torch.float64), c.stride(0), n, _hip.ptr(kept), m, _hip.ptr(xyz),
                                         _hip.stream()), "tl_inventory_gather")
    mark("sort + gather")

    table = torch.empty((T, len(_TABLE)), dtype=torch.float64, device=dev)
    counts = torch.empty((T, 2), dtype=torch.int64, device=dev)
    if T:
        _hip.check(L.tl_tree_inventory(_hip.ptr(xyz), m, _hip.ptr(start), T, p["slice_height"], p["slice_thickness"],
                                       p["dbh_max_radius"], p["dbh_min_points"], _hip.ptr(table), _hip.ptr(counts), _hip.stream()),
                   "tl_tree_inventory")
    mark("kernel")

    if terrain is not None:
        gtable = torch.empty((T, len(_GROUND_TABLE)), dtype=torch.float64, device=dev)
        gcount = torch.empty(T, dtype=torch.int64, device=dev)
        if T:
            zg = terrain.sample(table[:, 3:5])                                        # the positions, read in place from the table
            _hip.check(L.tl_tree_ground(_hip.ptr(xyz), m, _hip.ptr(start), T, _hip.ptr(table), _hip.ptr(zg), p["slice_height"],
                                        p["slice_thickness"], p["dbh_max_radius"], p["dbh_min_points"], _hip.ptr(gtable), _hip.ptr(gcount),
                                        _hip.stream()), "tl_tree_ground")
        mark("ground columns")

    cells = torch.zeros(T, dtype=torch.int64, device=dev)
    err = None
    if m:
        keys = torch.empty(m, dtype=torch.int64, device=dev)
        err = torch.empty(1, dtype=torch.int32, device=dev)
        _hip.check(L.tl_crown_keys(_hip.ptr(xyz), _hip.ptr(kept_lab), m, p["crown_cell"], _hip.ptr(keys), _hip.ptr(err), _hip.stream()),
                   "tl_crown_keys")
        keys = torch.sort(keys).values
        _hip.check(L.tl_crown_count(_hip.ptr(keys), m, T, _hip.ptr(cells), _hip.stream()), "tl_crown_count")
    mark("crown keys + count")

    if stem or crown or branches or leafwood:
        z_ref = gtable[:, 0] if terrain is not None else table[:, 0]
        tree = torch.stack([table[:, 3], table[:, 4], z_ref, table[:, 1]], 1).contiguous()
    if stem:
        stem_dev = _stem.stem_stage(xyz, kept_lab, T, tree, stem_cfg, mark)
    if crown:
        *crown_dev, crown_err = _crown.crown_stage(xyz, kept_lab, T, tree, crown_cfg, mark)
    wood_xyz, wood_lab = xyz, kept_lab
    if leafwood:
        lw_dev = _leafwood.leafwood_stage(xyz, kept_lab, T, tree, leafwood_cfg, mark, scales=lw_scales if lw_scales["scales"] is not None else None)
        lw_rows = torch.zeros(n, dtype=torch.uint8, device=dev)
        lw_rows[kept] = lw_dev["wood"]
        if leafwood_cfg["filter"] and branches:                                       # the wood rows in their order, as contiguous copies
            w = torch.nonzero(lw_dev["wood"]).reshape(-1)
            wood_xyz, wood_lab = xyz.index_select(0, w).contiguous(), kept_lab.index_select(0, w).contiguous()
        mark("leafwood scatter")
    if branches:
        branch_dev = _branches.branch_stage(wood_xyz, wood_lab, T, tree, branch_cfg, mark)
    if wood:
        wood_dev = _wood.wood_stage(wood_xyz, branch_dev, T, wood_cfg, mark)
    if light:
        light_out = _light.light_stage(c, lab, T, light_cfg, mark)

    table_h, counts_h, cells_h = table.cpu().numpy(), counts.cpu().numpy(), cells.cpu().numpy()
    if terrain is not None:
        gtable_h, gcount_h = gtable.cpu().numpy(), gcount.cpu().numpy()
    if stem:
        stem_out = _stem.to_columns(*(t.cpu().numpy() for t in stem_dev), off)
    if crown:
        crown_out = _crown.to_columns(*(t.cpu().numpy() for t in crown_dev), off)
        crown_bad = crown_err is not None and int(crown_err.item())
    if leafwood:
        lw_h = {k: lw_dev[k].cpu().numpy() for k in _leafwood.HOST_KEYS}
        lw_rows_h, lw_zref = lw_rows.cpu().numpy(), tree[:, 2].cpu().numpy()
        lw_bad = lw_dev["err"] is not None and int(lw_dev["err"].item())
    if branches:
        branch_h = {k: branch_dev[k].cpu().numpy() for k in ("kstart", "node_start", "xyz", "parent", "bin", "count")}
        branch_zref = tree[:, 2].cpu().numpy()
        branch_bad = branch_dev["err"] is not None and int(branch_dev["err"].item())
    if wood:
        wood_h = {k: wood_dev[k].cpu().numpy() for k in _wood.FIT_KEYS}
    bad = err is not None and int(err.item())
    mark("D2H")
    if bad:
        raise ValueError(f"a coordinate is not finite or lies beyond 2^20 crown cells of {p['crown_cell']} m from the origin: centre the cloud")
    if crown and crown_bad:
        raise _crown.crown_error(crown_cfg)
    if leafwood and lw_bad:
        from .branches import branch_error
        raise branch_error(leafwood_cfg)
    if branches and branch_bad:
        raise _branches.branch_error(branch_cfg)

    out = {k: np.ascontiguousarray(table_h[:, j]) for j, k in enumerate(_TABLE)}
    out["tree_id"] = np.arange(1, T + 1, dtype=np.int64)
    out["n_points"], out["dbh_n"], out["crown_cells"] = np.ascontiguousarray(counts_h[:, 0]), np.ascontiguousarray(counts_h[:, 1]), cells_h
    cell = np.float64(p["crown_cell"])
    area = cells_h.astype(np.float64) * (cell * cell)
    area[out["n_points"] == 0] = np.nan
    out["crown_area"] = area
    out["crown_diameter"] = 2 * np.sqrt(area / np.pi)
    if off is not None:
        for k, a in _SHIFTED:
            out[k] = out[k] + off[a]
    stem_keys = ()
    if stem:
        out.update(stem_out)
        stem_keys = _stem.STEM_COLUMNS + ("stem_profile",)
    if crown:
        out.update(crown_out)
        stem_keys = stem_keys + _crown.CROWN_COLUMNS + ("crown_profile",)
    if leafwood:
        out.update(_leafwood.to_columns(lw_h, lw_zref))
        out["leafwood"] = dict(leafwood_cfg, wood=lw_rows_h, **(lw_scales if lw_scales["scales"] is not None else {}))
        stem_keys = stem_keys + _leafwood.LEAFWOOD_COLUMNS + ("leafwood",)
    if branches:
        out.update(_branches.to_columns(branch_h, branch_zref, branch_cfg, off))
        mark("branch decomposition")
        stem_keys = stem_keys + _branches.BRANCH_COLUMNS + ("skeleton",)
    if wood:
        out.update(_wood.to_columns(dict(out["skeleton"], xyz=branch_h["xyz"]), wood_h, branch_zref, wood_cfg, branch_cfg, off))
        mark("wood radii")
        stem_keys = stem_keys + _wood.WOOD_COLUMNS + ("cylinders",)
    light_keys = ()
    if light:
        out.update(light_out)
        light_keys = _light.LIGHT_COLUMNS
    if terrain is None:
        return {k: out[k] for k in COLUMNS + stem_keys + light_keys}
    out.update({k: np.ascontiguousarray(gtable_h[:, j]) for j, k in enumerate(_GROUND_TABLE)})
    out["dbh_ag_n"] = gcount_h
    if off is not None:
        for k, a in _GROUND_SHIFTED:
            out[k] = out[k] + off[a]
    return {k: out[k] for k in COLUMNS + GROUND_COLUMNS + stem_keys + light_keys}


def cloud_inventory(points, terrain=False, terrain_cfg=None, stem=False, stem_cfg=None, crown=False, crown_cfg=None, branches=False,
                    branch_cfg=None, wood=False, wood_cfg=None, leafwood=False, leafwood_cfg=None, leafwood_scales=None,
                    leafwood_scales_min=None, light=False, light_cfg=None, **params):
    """The inventory of an N x 4 cloud (x y z label), as the command line computes it: the coordinates are centred on their float64 mean
    on the device, as segment_forest centres its input, and the mean is handed back as `offset`.  terrain=True builds the terrain of
    the label-0 rows in the same frame (util.terrain.terrain_model, parameters in terrain_cfg) and adds the GROUND_COLUMNS; stem=True
    adds util.stem's STEM_COLUMNS and "stem_profile" (parameters in stem_cfg); crown=True adds util.crown's CROWN_COLUMNS and
    "crown_profile" (parameters in crown_cfg); branches=True adds util.branches' BRANCH_COLUMNS and "skeleton" (parameters in branch_cfg);
    wood=True implies branches=True and adds util.wood's WOOD_COLUMNS and "cylinders" (parameters in wood_cfg); leafwood=True adds
    util.leafwood's LEAFWOOD_COLUMNS and "leafwood" (parameters in leafwood_cfg); light=True adds util.light's LIGHT_COLUMNS last
    (parameters in light_cfg)."""
    import torch
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if pts.ndim != 2 or pts.shape[1] != 4:
        raise ValueError(f"expected an N x 4 cloud (x y z label), got {tuple(pts.shape)}")
    check_params(**params)
    if terrain:
        from .terrain import check_params as check_terrain, terrain_model
        terrain_cfg = check_terrain(terrain_cfg)
    if stem:
        from .stem import check_params as check_stem
        stem_cfg = check_stem(stem_cfg)
    if crown:
        from .crown import check_params as check_crown
        crown_cfg = check_crown(crown_cfg)
    extra = {}
    if branches or wood:
        from .branches import check_params as check_branches
        extra = dict(branches=True, branch_cfg=check_branches(branch_cfg))
    if wood:
        from .wood import check_params as check_wood
        extra.update(wood=True, wood_cfg=check_wood(wood_cfg))
    if leafwood:
        from .leafwood import check_params as check_leafwood, check_scales
        extra.update(leafwood=True, leafwood_cfg=check_leafwood(leafwood_cfg), leafwood_scales=leafwood_scales, leafwood_scales_min=leafwood_scales_min)
        check_scales(scales=leafwood_scales, scales_min=leafwood_scales_min)
    if light:
        from .light import check_params as check_light
        extra.update(light=True, light_cfg=check_light(light_cfg))
    if not torch.cuda.is_available():
        raise RuntimeError("treelearn_amd.util.inventory runs on the GPU (tl_tree_inventory); there is no CPU fallback")
    pts = pts.to("cuda")
    xyz, lab = pts[:, :3].to(torch.float64), pts[:, 3].to(torch.int64)
    if len(xyz) == 0:
        return tree_inventory(xyz, lab, terrain=terrain_model(xyz, lab, **terrain_cfg) if terrain else None, stem=stem, stem_cfg=stem_cfg, crown=crown,
                              crown_cfg=crown_cfg, **extra, **params)
    mean = xyz.mean(0)
    centred = xyz - mean
    return tree_inventory(centred, lab, offset=mean, terrain=terrain_model(centred, lab, **terrain_cfg) if terrain else None, stem=stem,
                          stem_cfg=stem_cfg, crown=crown, crown_cfg=crown_cfg, **extra, **params)


def write_inventory(path, inv, categories=None):
    """CSV: a header row, then one row per tree; floats as repr (they read back to the same bits), NaN as `nan`.  `categories` (per tree:
    index into segment.CATEGORIES) adds a `category` column of names.  The columns are those the dict holds: COLUMNS, and GROUND_COLUMNS
    after them when the inventory was taken with a terrain, then util.stem's STEM_COLUMNS when it was taken with stem=True, then
    util.crown's CROWN_COLUMNS when it was taken with crown=True, then util.branches' BRANCH_COLUMNS when it was taken with branches=True,
    then util.wood's WOOD_COLUMNS when it was taken with wood=True; util.leafwood's LEAFWOOD_COLUMNS stand between the crown and the
    branch group when it was taken with leafwood=True; util.light's LIGHT_COLUMNS come last when it was taken with light=True (each group
    only when the dict holds all of it)."""
    from .branches import BRANCH_COLUMNS, BRANCH_INT_COLUMNS
    from .crown import CROWN_COLUMNS, CROWN_INT_COLUMNS
    from .leafwood import LEAFWOOD_COLUMNS, LEAFWOOD_INT_COLUMNS
    from .light import LIGHT_COLUMNS, LIGHT_INT_COLUMNS
    from .stem import STEM_COLUMNS
    from .wood import WOOD_COLUMNS, WOOD_INT_COLUMNS
    T = len(inv["tree_id"])
    columns = COLUMNS + (GROUND_COLUMNS if all(k in inv for k in GROUND_COLUMNS) else ()) + (STEM_COLUMNS if all(k in inv for k in STEM_COLUMNS) else ()) + \
        (CROWN_COLUMNS if all(k in inv for k in CROWN_COLUMNS) else ()) + (LEAFWOOD_COLUMNS if all(k in inv for k in LEAFWOOD_COLUMNS) else ()) + \
        (BRANCH_COLUMNS if all(k in inv for k in BRANCH_COLUMNS) else ()) + \
        (WOOD_COLUMNS if all(k in inv for k in WOOD_COLUMNS) else ()) + (LIGHT_COLUMNS if all(k in inv for k in LIGHT_COLUMNS) else ())
    ints = INT_COLUMNS + ("dbh_ag_n", "stem_slices") + CROWN_INT_COLUMNS + LEAFWOOD_INT_COLUMNS + BRANCH_INT_COLUMNS + WOOD_INT_COLUMNS + LIGHT_INT_COLUMNS
    names = None
    if categories is not None:
        from .segment import CATEGORIES
        cat = np.asarray(categories).reshape(-1)
        if len(cat) != T:
            raise ValueError(f"{len(cat)} categories for {T} trees")
        names = [CATEGORIES[int(v)] for v in cat]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(list(columns) + (["category"] if names is not None else []))
        for i in range(T):
            row = [str(int(inv[k][i])) if k in ints else repr(float(inv[k][i])) for k in columns]
            w.writerow(row + ([names[i]] if names is not None else []))
    return path


def add_arguments(ap):
    """The five parameters as command-line options (shared with util.segment)."""
    ap.add_argument("--slice-height", type=float, default=DEFAULTS["slice_height"], help="height of the DBH slice above the tree base, metres")
    ap.add_argument("--slice-thickness", type=float, default=DEFAULTS["slice_thickness"], help="thickness of the DBH slice, metres")
    ap.add_argument("--dbh-max-radius", type=float, default=DEFAULTS["dbh_max_radius"], help="slice rows farther than this from the tree position are left out")
    ap.add_argument("--dbh-min-points", type=int, default=DEFAULTS["dbh_min_points"], help="fewer slice rows than this: no DBH")
    ap.add_argument("--crown-cell", type=float, default=DEFAULTS["crown_cell"], help="edge of the crown-cover cells, metres")


def params_of(a):
    return {k: getattr(a, k) for k in DEFAULTS}


def main(argv=None):
    import os
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.inventory", description="per-tree inventory (position, height, DBH, crown) of a labelled cloud")
    ap.add_argument("--forest", required=True, help="labelled cloud: .npy / .npz / .txt / .las, N x 4 (x y z label)")
    ap.add_argument("--out", required=True, help="CSV to write")
    add_arguments(ap)
    ap.add_argument("--terrain", action="store_true", help="add the ground columns: terrain from the label-0 rows, height and DBH from the ground")
    from . import terrain as _terrain
    _terrain.add_arguments(ap)
    ap.add_argument("--stem", action="store_true", help="add the stem columns: slices, base and top height, volume, DBH, lean and taper of the stem profile")
    from . import stem as _stem
    _stem.add_arguments(ap)
    ap.add_argument("--crown", action="store_true", help="add the crown columns: crown base, length, ratio, volume, projection area, centroid and radii")
    from . import crown as _crown
    _crown.add_arguments(ap)
    ap.add_argument("--branches", action="store_true", help="add the branch columns: skeleton size and length, axis, branch count, length and order, first branch")
    from . import branches as _branches
    _branches.add_arguments(ap)
    ap.add_argument("--wood", action="store_true", help="add the wood columns: fitted nodes, wood length, volume and area, volume of the axis and of the branches (implies --branches)")
    from . import wood as _wood
    _wood.add_arguments(ap)
    ap.add_argument("--leafwood", action="store_true", help="add the leafwood columns: wood and leaf rows, wood components, wood share, highest wood; --branches and --wood then read the wood rows only")
    from . import leafwood as _leafwood
    _leafwood.add_arguments(ap)
    ap.add_argument("--light", action="store_true", help="add the light columns: how much sky the top of every tree sees past its neighbours")
    from . import light as _light
    _light.add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        params = check_params(params_of(a))
        light_cfg = _light.check_params(_light.params_of(a))
        leafwood_cfg = _leafwood.check_params(_leafwood.params_of(a))
        lw_scales = _leafwood.check_scales(_leafwood.scales_of(a))
        terrain_cfg = _terrain.check_params(_terrain.params_of(a))
        stem_cfg = _stem.check_params(_stem.params_of(a))
        crown_cfg = _crown.check_params(_crown.params_of(a))
        branch_cfg = _branches.check_params(_branches.params_of(a))
        wood_cfg = _wood.check_params(_wood.params_of(a))
    except ValueError as e:
        ap.error(str(e))
    if not os.path.exists(a.forest):
        ap.error(f"--forest {a.forest}: no such file")
    from .segment import load_forest
    data = load_forest(a.forest)
    if data.shape[1] != 4:
        ap.error(f"--forest {a.forest}: expected N x 4 (x y z label), got {data.shape}")
    inv = cloud_inventory(data, terrain=a.terrain, terrain_cfg=terrain_cfg if a.terrain else None, stem=a.stem, stem_cfg=stem_cfg if a.stem else None,
                          crown=a.crown, crown_cfg=crown_cfg if a.crown else None, branches=a.branches or a.wood,
                          branch_cfg=branch_cfg if a.branches or a.wood else None, wood=a.wood, wood_cfg=wood_cfg if a.wood else None,
                          leafwood=a.leafwood, leafwood_cfg=leafwood_cfg if a.leafwood else None,
                          leafwood_scales=lw_scales["scales"], leafwood_scales_min=lw_scales["scales_min"], light=a.light,
                          light_cfg=light_cfg if a.light else None, **params)
    write_inventory(a.out, inv)
    ok = int(np.isfinite(inv["dbh"]).sum())
    print(f"{a.forest}: {len(data)} points, {len(inv['tree_id'])} trees, {ok} with a DBH -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
