"""Crown structure of a segmented forest on the device: where the crown of every tree begins, how long it is, the volume it fills, the
ground it projects onto and its radius in eight directions.

    python -m treelearn_amd.util.crown --forest labelled.npy|npz|txt|las --out crowns.npz [--csv trees.csv] [--terrain] [--branches] [--wood] [--crown-layer 0.5 ...]

The semantics are the project's own; tests/crown_restatement.py states them in numpy float64.  The stage runs inside
util.inventory.tree_inventory(..., crown=True) on the label-sorted rows and the tree table that function already holds on the device.
Per tree with rows: the position (px, py), z_top and a reference height z_ref (z_ground with a terrain, z_low without); H = z_top - z_ref.

  grid     voxels of cell x cell x layer: layer l = floor((z - z_ref) / layer) for 0 <= l < L_t = min(floor(H / layer) + 1, max_layers),
           cell (floor(x / cell), floor(y / cell)) in the frame of the coordinates.  Per layer: its rows n, its distinct cells.
  base     among the layers whose bottom is at least min_height: the widest (most cells, the lowest of equals); from it downwards a layer
           is crown-like with cells * 100 >= base_percent * the widest's; max_gap thin layers in a row are bridged, one more ends the
           walk.  The lowest crown-like layer reached is the crown base.
  columns  crown_layers (L_t), crown_base_h, crown_length (H - base), crown_ratio (length / H), crown_widest_h (the middle of the widest
           layer), crown_voxels (cells of the layers from the base up), crown_volume (m^3), crown_proj_cells (distinct xy cells of those
           layers), crown_proj_area (m^2), crown_x, crown_y (the centroid of the projection cells), crown_offset (its distance from the
           position), crown_radius_max, crown_radius_mean (over eight 45 degree sectors around the position, counter-clockwise from +x;
           a sector's radius is its farthest projection cell centre, 0 for an empty sector).  NaN (0 in the integer columns) where
           there is no crown.
  profile  "crown_profile": [T, L] arrays h (f64, the layer bottom; NaN beyond the tree's last layer), n, cells (i64) and radii f64 [T, 8];
           L = the most layers any tree has.

Known limits: a tree taller than max_layers * layer is truncated; low vegetation labelled to the tree can be the widest layer; the stem
inside the crown counts as crown; a row farther than 4096 cells from its tree's position is an error.

csrc/tl_crown.hip gives every row a (tree, cell x, cell y, layer) key (tl_crown_voxel_keys); one torch sort makes every tree a contiguous
range of keys, which tl_crown_structure reads with one workgroup per tree.  There is no CPU fallback."""
import argparse
import sys

import numpy as np

CROWN_DEFAULTS = dict(layer=0.5, cell=0.25, max_layers=256, min_height=1.0, base_percent=10, max_gap=1)
CROWN_COLUMNS = ("crown_layers", "crown_base_h", "crown_length", "crown_ratio", "crown_widest_h", "crown_voxels", "crown_volume",
                 "crown_proj_cells", "crown_proj_area", "crown_x", "crown_y", "crown_offset", "crown_radius_max", "crown_radius_mean")
CROWN_INT_COLUMNS = ("crown_layers", "crown_voxels", "crown_proj_cells")
PROFILE_KEYS = ("h", "n", "cells", "radii")
_INT = ("max_layers", "base_percent", "max_gap")
_SUMMARY = tuple(k for k in CROWN_COLUMNS if k not in CROWN_INT_COLUMNS)                         # tl_crown_structure's summary columns
_TREE_SHIFT = 34                                                                                 # the tree field of a voxel key
_HELP = dict(layer="layer thickness, metres", cell="edge of the xy cells, metres", max_layers="most layers per tree (1..256)",
             min_height="layers whose bottom is below this take no part in finding the widest layer or the crown base, metres",
             base_percent="a layer is crown-like with at least this share of the widest layer's cells, percent (1..100)",
             max_gap="this many thin layers in a row are bridged on the way down to the crown base")

__all__ = ["CROWN_DEFAULTS", "CROWN_COLUMNS", "check_params", "add_arguments", "params_of", "write_crown_profiles"]


def check_params(cfg=None, **kw):
    """The six parameters as a dict of plain numbers (defaults filled in); ValueError for an unknown name or a value outside its
    constraint (the table of DESIGN §20).  Touches no GPU."""
    p = dict(CROWN_DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in CROWN_DEFAULTS:
                raise ValueError(f"unknown crown parameter {k!r}; expected one of {tuple(CROWN_DEFAULTS)}")
            if v is not None:
                p[k] = v
    for k in CROWN_DEFAULTS:
        if k in _INT:
            if isinstance(p[k], bool) or not np.isfinite(p[k]) or int(p[k]) != p[k]:
                raise ValueError(f"{k} must be an integer, got {p[k]!r}")
            p[k] = int(p[k])
        else:
            p[k] = float(p[k])
            if not np.isfinite(p[k]):
                raise ValueError(f"{k} must be finite, got {p[k]!r}")
    for k in ("layer", "cell"):
        if not p[k] > 0:
            raise ValueError(f"{k} must be > 0, got {p[k]!r}")
    if not p["min_height"] >= 0:
        raise ValueError(f"min_height must be >= 0, got {p['min_height']!r}")
    if not 1 <= p["max_layers"] <= 256:
        raise ValueError(f"max_layers must be in 1..256, got {p['max_layers']!r}")
    if not 1 <= p["base_percent"] <= 100:
        raise ValueError(f"base_percent must be in 1..100, got {p['base_percent']!r}")
    if not 0 <= p["max_gap"] < 1 << 62:
        raise ValueError(f"max_gap must be >= 0, got {p['max_gap']!r}")
    return p


def crown_stage(xyz, kept_lab, T, tree, p, mark):
    """The stage on the device.  xyz f64 [m, 3]: the gathered rows in label order, kept_lab i64 [m]: their labels, tree f64 [T, 4] = px, py,
    z_ref, z_top per tree, p: checked parameters, mark(name): closes a timed stage.  Returns the device tensors summary f64 [T, 11],
    counts i64 [T, 3], h f64 [T, L], pcount i64 [T, L, 2], radii f64 [T, 8] and err i32 [1] (or None: no rows); the caller raises
    crown_error() when err reads non-zero."""
    import torch
    from .. import _hip
    lib, dev, m = _hip.lib(), xyz.device, len(xyz)
    cp = _hip.CrownParams(**p)
    # the profile width: the most layers any tree has
    L = 0
    if T:
        H = tree[:, 3] - tree[:, 2]
        lt = torch.clamp(torch.floor(H / p["layer"]) + 1.0, max=float(p["max_layers"]))
        L = int(torch.where(H >= 0, lt, torch.zeros_like(lt)).max())
    summary = torch.full((T, len(_SUMMARY)), float("nan"), dtype=torch.float64, device=dev)
    counts = torch.zeros((T, 3), dtype=torch.int64, device=dev)
    h = torch.full((T, L), float("nan"), dtype=torch.float64, device=dev)
    pcount = torch.zeros((T, L, 2), dtype=torch.int64, device=dev)
    radii = torch.full((T, 8), float("nan"), dtype=torch.float64, device=dev)
    if T == 0 or L == 0:
        mark("crown voxel keys"); mark("crown sort + searchsorted"); mark("crown structure")
        return summary, counts, h, pcount, radii, None
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if m:
        _hip.check(lib.tl_crown_voxel_keys(_hip.ptr(xyz), _hip.ptr(kept_lab), m, _hip.ptr(tree), T, cp, _hip.ptr(keys), _hip.ptr(err),
                                           _hip.stream()), "tl_crown_voxel_keys")
    mark("crown voxel keys")
    skeys = torch.sort(keys).values
    kstart = torch.searchsorted(skeys, torch.arange(T + 1, dtype=torch.int64, device=dev) << _TREE_SHIFT).contiguous()
    if not m:
        skeys = torch.zeros(1, dtype=torch.int64, device=dev)                             # (a pointer to pass; no key is read)
    mark("crown sort + searchsorted")
    _hip.check(lib.tl_crown_structure(_hip.ptr(skeys), m, _hip.ptr(kstart), _hip.ptr(tree), T, L, cp, _hip.ptr(summary), _hip.ptr(counts),
                                      _hip.ptr(h), _hip.ptr(pcount), _hip.ptr(radii), _hip.stream()), "tl_crown_structure")
    mark("crown structure")
    return summary, counts, h, pcount, radii, err


def crown_error(p):
    return ValueError(f"a coordinate of a tree is not finite, or a row lies more than 4096 crown cells of {p['cell']} m from its tree's position")


def to_columns(summary_h, counts_h, h_h, pcount_h, radii_h, off):
    """The host arrays of crown_stage as the inventory's columns: CROWN_COLUMNS and "crown_profile" (`off`: 3 values, the first two added
    to crown_x, crown_y, or None)."""
    out = {k: np.ascontiguousarray(counts_h[:, j]) for j, k in enumerate(CROWN_INT_COLUMNS)}
    out.update({k: np.ascontiguousarray(summary_h[:, j]) for j, k in enumerate(_SUMMARY)})
    if off is not None:
        out["crown_x"], out["crown_y"] = out["crown_x"] + off[0], out["crown_y"] + off[1]
    out = {k: out[k] for k in CROWN_COLUMNS}
    out["crown_profile"] = dict(h=h_h, n=np.ascontiguousarray(pcount_h[:, :, 0]), cells=np.ascontiguousarray(pcount_h[:, :, 1]), radii=radii_h)
    return out


def write_crown_profiles(path, inv):
    """An .npz of tree_id [T], the [T, L] arrays h, n, cells and radii [T, 8] of an inventory taken with crown=True."""
    if "crown_profile" not in inv:
        raise ValueError("the inventory holds no crown profile: take it with crown=True")
    prof = inv["crown_profile"]
    with open(path, "wb") as f:
        np.savez(f, tree_id=np.asarray(inv["tree_id"], np.int64), **{k: prof[k] for k in PROFILE_KEYS})
    return path


def add_arguments(ap):
    """One --crown-... option per parameter (shared with util.segment, util.inventory and util.stem).  --crown-cell is the inventory's
    option of that name where the parser already has it: one cell edge then serves the crown cover of §16 and this stage."""
    for k, v in CROWN_DEFAULTS.items():
        opt = "--crown-" + k.replace("_", "-")
        if opt not in ap._option_string_actions:
            ap.add_argument(opt, type=int if k in _INT else float, default=v, help=_HELP[k])


def params_of(a):
    return {k: getattr(a, "crown_" + k) for k in CROWN_DEFAULTS}


def main(argv=None):
    import os
    from . import inventory as _inventory, terrain as _terrain
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.crown", description="crown structure (crown base, layered volume, crown radii) of a labelled cloud")
    ap.add_argument("--forest", required=True, help="labelled cloud: .npy / .npz / .txt / .las, N x 4 (x y z label)")
    ap.add_argument("--out", required=True, help=".npz to write: tree_id, the [T, L] arrays h, n, cells and radii [T, 8]")
    ap.add_argument("--csv", default=None, help="also write the tree inventory with the crown columns as CSV")
    _inventory.add_arguments(ap)
    add_arguments(ap)
    ap.add_argument("--terrain", action="store_true", help="measure heights from the terrain of the label-0 rows (z_ground) instead of z_low")
    _terrain.add_arguments(ap)
    ap.add_argument("--branches", action="store_true", help="add the branch columns (util.branches) to the CSV")
    from . import branches as _branches
    _branches.add_arguments(ap)
    ap.add_argument("--wood", action="store_true", help="add the wood columns (util.wood) to the CSV (implies --branches)")
    from . import wood as _wood
    _wood.add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        crown_cfg = check_params(params_of(a))
        branch_cfg = _branches.check_params(_branches.params_of(a))
        wood_cfg = _wood.check_params(_wood.params_of(a))
        params = _inventory.check_params(_inventory.params_of(a))
        terrain_cfg = _terrain.check_params(_terrain.params_of(a))
    except ValueError as e:
        ap.error(str(e))
    if not os.path.exists(a.forest):
        ap.error(f"--forest {a.forest}: no such file")
    from .segment import load_forest
    data = load_forest(a.forest)
    if data.shape[1] != 4:
        ap.error(f"--forest {a.forest}: expected N x 4 (x y z label), got {data.shape}")
    inv = _inventory.cloud_inventory(data, terrain=a.terrain, terrain_cfg=terrain_cfg if a.terrain else None, crown=True, crown_cfg=crown_cfg, branches=a.branches or a.wood,
                                     branch_cfg=branch_cfg if a.branches or a.wood else None, wood=a.wood, wood_cfg=wood_cfg if a.wood else None, **params)
    write_crown_profiles(a.out, inv)
    if a.csv:
        _inventory.write_inventory(a.csv, inv)
    ok = int((inv["crown_proj_cells"] > 0).sum())
    print(f"{a.forest}: {len(data)} points, {len(inv['tree_id'])} trees, {ok} with a crown, {int(inv['crown_voxels'].sum())} crown voxels -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
