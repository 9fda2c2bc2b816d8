"""Stem profiles of a segmented forest on the device: the diameter along the height of every tree (the taper curve), the stem volume, a
diameter at breast height interpolated on the profile, the lean and the taper.

    python -m treelearn_amd.util.stem --forest labelled.npy|npz|txt|las --out stems.npz [--csv trees.csv] [--terrain] [--crown] [--branches] [--wood] [--stem-step 0.5 ...]

The semantics are the project's own; tests/stem_restatement.py states them in numpy float64.  The stage runs inside
util.inventory.tree_inventory(..., stem=True) on the label-sorted rows and the tree table that function already holds on the device.
Per tree with rows: the position (px, py), z_top and a reference height z_ref (z_ground with a terrain, z_low without).

  slabs    h_k = first_height + k * step for k < max_slices while h_k <= z_top - z_ref; slab k is z_ref + h_k -+ thickness / 2 (lower bound
           in, upper out).  Rows within `corridor` (horizontally, strictly) of the position are stem candidates.
  walk     bottom-up from c = position, R = start_radius.  The search set of a slab: its candidates within R of c.  With at least
           min_points of them the algebraic (Kasa) circle fit of the inventory; the slab is accepted when the fit succeeds, its rms
           residual is <= max_rmse, min_radius <= r <= max_radius and r <= max_growth x the last accepted radius.  An accepted circle moves
           c to its centre and sets R = search_factor * r + search_margin; max_misses rejected slabs in a row end the walk.
  columns  stem_slices (accepted slabs), stem_base_h, stem_top_h (their lowest / highest h), stem_volume (a cylinder up to the first
           accepted slab, then conical frustums between consecutive accepted slabs; m^3), dbh_stem (the diameter interpolated at
           dbh_height), stem_lean (degrees from the vertical, first to last accepted centre), stem_taper (least-squares slope of the
           diameter on h, m per m, negative for a tapering stem).  NaN where there is nothing to compute them from.
  profile  "stem_profile": [T, S] arrays h, x, y, r, rmse (f64) and n, state (i64): S = the most slabs any tree has; state 1 accepted,
           2 rejected, 0 not visited (or beyond the tree's last slab, where h is NaN as well).

Known limits: a stem that leans out of the corridor is lost; `thickness` must span at least two voxel layers of a voxelised cloud; a
forked stem follows whichever fork the circle fit prefers; nothing is smoothed or fitted across slabs.

csrc/tl_stem.hip gives every row a (tree, slab) key (tl_stem_keys); one stable torch sort and tl_inventory_gather make every slab a
contiguous range; tl_stem_profile walks each tree with one workgroup.  There is no CPU fallback."""
import argparse
import sys

import numpy as np

STEM_DEFAULTS = dict(first_height=0.5, step=0.5, thickness=0.2, max_slices=128, corridor=1.5, start_radius=0.6, search_factor=1.5,
                     search_margin=0.10, min_points=8, max_rmse=0.03, min_radius=0.02, max_radius=1.0, max_growth=1.25, max_misses=3,
                     dbh_height=1.3)
STEM_COLUMNS = ("stem_slices", "stem_base_h", "stem_top_h", "stem_volume", "dbh_stem", "stem_lean", "stem_taper")
PROFILE_KEYS = ("h", "x", "y", "r", "rmse", "n", "state")
_INT = ("max_slices", "min_points", "max_misses")
_SUMMARY = STEM_COLUMNS[1:]                                                                      # tl_stem_profile's summary columns
_HELP = dict(first_height="height of the lowest slab above the tree's reference height, metres", step="distance between slab centres, metres",
             thickness="slab thickness, metres (at most the step)", max_slices="most slabs per tree (1..256)",
             corridor="rows farther than this from the tree position (horizontally) are no stem candidates, metres",
             start_radius="search radius before the first accepted slab, metres", search_factor="search radius = this x the last accepted radius + the margin",
             search_margin="added to the search radius, metres", min_points="fewer rows in a slab's search set: slab rejected",
             max_rmse="larger rms residual of the circle fit: slab rejected, metres", min_radius="smaller fitted radius: slab rejected, metres",
             max_radius="larger fitted radius: slab rejected, metres", max_growth="a radius above this x the last accepted radius: slab rejected",
             max_misses="this many rejected slabs in a row end the walk", dbh_height="height at which dbh_stem is interpolated, metres")

__all__ = ["STEM_DEFAULTS", "STEM_COLUMNS", "check_params", "add_arguments", "params_of", "write_stem_profiles"]


def check_params(cfg=None, **kw):
    """The fifteen parameters as a dict of plain numbers (defaults filled in); ValueError for an unknown name or a value outside its
    constraint (the table of DESIGN §19).  Touches no GPU."""
    p = dict(STEM_DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in STEM_DEFAULTS:
                raise ValueError(f"unknown stem parameter {k!r}; expected one of {tuple(STEM_DEFAULTS)}")
            if v is not None:
                p[k] = v
    for k in STEM_DEFAULTS:
        if k in _INT:
            if isinstance(p[k], bool) or not np.isfinite(p[k]) or int(p[k]) != p[k]:
                raise ValueError(f"{k} must be an integer, got {p[k]!r}")
            p[k] = int(p[k])
        else:
            p[k] = float(p[k])
            if not np.isfinite(p[k]):
                raise ValueError(f"{k} must be finite, got {p[k]!r}")
    for k in ("first_height", "step", "thickness", "corridor", "start_radius", "max_rmse", "min_radius", "max_radius", "dbh_height"):
        if not p[k] > 0:
            raise ValueError(f"{k} must be > 0, got {p[k]!r}")
    if p["thickness"] > p["step"]:
        raise ValueError(f"thickness must be at most the step ({p['step']!r}), got {p['thickness']!r}")
    if not 1 <= p["max_slices"] <= 256:
        raise ValueError(f"max_slices must be in 1..256, got {p['max_slices']!r}")
    for k in ("search_factor", "max_growth"):
        if not p[k] >= 1:
            raise ValueError(f"{k} must be >= 1, got {p[k]!r}")
    if not p["search_margin"] >= 0:
        raise ValueError(f"search_margin must be >= 0, got {p['search_margin']!r}")
    if p["min_points"] < 3:
        raise ValueError(f"min_points must be >= 3, got {p['min_points']!r}")
    if p["min_radius"] > p["max_radius"]:
        raise ValueError(f"min_radius must be at most max_radius ({p['max_radius']!r}), got {p['min_radius']!r}")
    if not 1 <= p["max_misses"] < 1 << 31:
        raise ValueError(f"max_misses must be >= 1, got {p['max_misses']!r}")
    return p


def stem_stage(xyz, kept_lab, T, tree, p, mark):
    """The stage on the device.  xyz f64 [m, 3]: the gathered rows in label order, kept_lab i64 [m]: their labels, tree f64 [T, 4] = px, py,
    z_ref, z_top per tree, p: checked parameters, mark(name): closes a timed stage.  Returns the device tensors profile f64 [T, S, 5],
    pcount i64 [T, S, 2], summary f64 [T, 6], slices i64 [T]."""
    import torch
    from .. import _hip
    L, dev, m = _hip.lib(), xyz.device, len(xyz)
    cp = _hip.StemParams(**p)
    # the profile width: the most slabs any tree has, h_k in one multiplication and one addition
    S = 0
    if T:
        hk = torch.from_numpy(np.float64(p["first_height"]) + np.arange(p["max_slices"], dtype=np.float64) * np.float64(p["step"])).to(dev)
        S = int((hk[None, :] <= (tree[:, 3] - tree[:, 2])[:, None]).sum(1).max())
    summary = torch.full((T, len(_SUMMARY)), float("nan"), dtype=torch.float64, device=dev)
    slices = torch.zeros(T, dtype=torch.int64, device=dev)
    profile = torch.empty((T, S, 5), dtype=torch.float64, device=dev)
    pcount = torch.empty((T, S, 2), dtype=torch.int64, device=dev)
    if T == 0 or S == 0:
        mark("stem keys"); mark("stem sort + gather + searchsorted"); mark("stem profile")
        return profile, pcount, summary, slices
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    if m:
        _hip.check(L.tl_stem_keys(_hip.ptr(xyz), _hip.ptr(kept_lab), m, _hip.ptr(tree), T, S, cp, _hip.ptr(keys), _hip.stream()), "tl_stem_keys")
    mark("stem keys")
    skeys, order = torch.sort(keys, stable=True)
    slab_start = torch.searchsorted(skeys, torch.arange(T * S + 1, dtype=torch.int64, device=dev)).contiguous()
    ms = int(slab_start[-1])                                                          # the rows below the sentinel
    stem_xyz = torch.empty((max(ms, 1), 3), dtype=torch.float64, device=dev)
    if ms:
        _hip.check(L.tl_inventory_gather(_hip.ptr(xyz), 1, 3, m, _hip.ptr(order), ms, _hip.ptr(stem_xyz), _hip.stream()), "tl_inventory_gather")
    mark("stem sort + gather + searchsorted")
    _hip.check(L.tl_stem_profile(_hip.ptr(stem_xyz), ms, _hip.ptr(slab_start), _hip.ptr(tree), T, S, cp, _hip.ptr(profile), _hip.ptr(pcount),
                                 _hip.ptr(summary), _hip.ptr(slices), _hip.stream()), "tl_stem_profile")
    mark("stem profile")
    return profile, pcount, summary, slices


def to_columns(profile_h, pcount_h, summary_h, slices_h, off):
    """The host arrays of stem_stage as the inventory's columns: STEM_COLUMNS and "stem_profile" (`off`: 3 values added to x, y, or None)."""
    out = {"stem_slices": slices_h}
    out.update({k: np.ascontiguousarray(summary_h[:, j]) for j, k in enumerate(_SUMMARY)})
    prof = {k: np.ascontiguousarray(profile_h[:, :, j]) for j, k in enumerate(PROFILE_KEYS[:5])}
    prof["n"], prof["state"] = np.ascontiguousarray(pcount_h[:, :, 0]), np.ascontiguousarray(pcount_h[:, :, 1])
    if off is not None:
        prof["x"], prof["y"] = prof["x"] + off[0], prof["y"] + off[1]
    out["stem_profile"] = prof
    return out


def write_stem_profiles(path, inv):
    """An .npz of tree_id [T] and the [T, S] arrays h, x, y, r, rmse, n, state of an inventory taken with stem=True."""
    if "stem_profile" not in inv:
        raise ValueError("the inventory holds no stem profile: take it with stem=True")
    prof = inv["stem_profile"]
    with open(path, "wb") as f:
        np.savez(f, tree_id=np.asarray(inv["tree_id"], np.int64), **{k: prof[k] for k in PROFILE_KEYS})
    return path


def add_arguments(ap):
    """One --stem-... option per parameter (shared with util.segment and util.inventory)."""
    for k, v in STEM_DEFAULTS.items():
        ap.add_argument("--stem-" + k.replace("_", "-"), type=int if k in _INT else float, default=v, help=_HELP[k])


def params_of(a):
    return {k: getattr(a, "stem_" + k) for k in STEM_DEFAULTS}


def main(argv=None):
    import os
    from . import inventory as _inventory, terrain as _terrain
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.stem", description="stem profiles (taper curve, stem volume, lean) of a labelled cloud")
    ap.add_argument("--forest", required=True, help="labelled cloud: .npy / .npz / .txt / .las, N x 4 (x y z label)")
    ap.add_argument("--out", required=True, help=".npz to write: tree_id and the [T, S] arrays h, x, y, r, rmse, n, state")
    ap.add_argument("--csv", default=None, help="also write the tree inventory with the stem columns as CSV")
    add_arguments(ap)
    _inventory.add_arguments(ap)
    ap.add_argument("--terrain", action="store_true", help="measure heights from the terrain of the label-0 rows (z_ground) instead of z_low")
    _terrain.add_arguments(ap)
    ap.add_argument("--crown", action="store_true", help="add the crown columns (util.crown) to the CSV")
    from . import crown as _crown
    _crown.add_arguments(ap)
    ap.add_argument("--branches", action="store_true", help="add the branch columns (util.branches) to the CSV")
    from . import branches as _branches
    _branches.add_arguments(ap)
    ap.add_argument("--wood", action="store_true", help="add the wood columns (util.wood) to the CSV (implies --branches)")
    from . import wood as _wood
    _wood.add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        crown_cfg = _crown.check_params(_crown.params_of(a))
        branch_cfg = _branches.check_params(_branches.params_of(a))
        wood_cfg = _wood.check_params(_wood.params_of(a))
        stem_cfg = check_params(params_of(a))
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
    inv = _inventory.cloud_inventory(data, terrain=a.terrain, terrain_cfg=terrain_cfg if a.terrain else None, stem=True, stem_cfg=stem_cfg,
                                    crown=a.crown, crown_cfg=crown_cfg if a.crown else None, branches=a.branches or a.wood,
                                    branch_cfg=branch_cfg if a.branches or a.wood else None, wood=a.wood, wood_cfg=wood_cfg if a.wood else None, **params)
    write_stem_profiles(a.out, inv)
    if a.csv:
        _inventory.write_inventory(a.csv, inv)
    ok = int((inv["stem_slices"] > 0).sum())
    print(f"{a.forest}: {len(data)} points, {len(inv['tree_id'])} trees, {ok} with a stem profile, {int(inv['stem_slices'].sum())} accepted slabs -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
