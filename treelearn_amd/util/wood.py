"""Cylinder model of a segmented forest on the device: how thick the wood of every skeleton is -- one circle fit per skeleton node, the
radii along the branches, and the wood volume of the stem, of the branches and by branch order.

    python -m treelearn_amd.util.wood --forest labelled.npy|npz|txt|las --out cylinders.npz [--csv trees.csv] [--terrain] [--leafwood] [--wood-max-rmse 0.03 ...]

The semantics are the project's own; tests/wood_restatement.py states them in plain Python.  The stage runs inside
util.inventory.tree_inventory(..., wood=True) behind the branch structure (util.branches, which it implies), on the same label-sorted rows.

  rows      a gathered row belongs to node i when its voxel key (tl_skel_voxel_keys') is a reached voxel (d >= 0) of node i.  Rows with
            key -1, rows of unreached voxels and rows of trees without a skeleton belong to no node.
  axis      of a node with a parent at the centroid distance seg = sqrt(dx dx + dy dy + dz dz) > 0: a = (c - c_parent) / seg; of a root,
            or with seg == 0: (0, 0, 1).
  basis     k = the index of the smallest |a_k| (the first among equals); w = a x e_k, e1 = w / |w|, e2 = a x e1.
  fit       over the node's rows p: q = p - c, u = q . e1, v = q . e2.  With n >= min_points the Kasa circle (cu, cv, r) and rmse =
            sqrt(rss / n).  state: 0 too few rows, 1 accepted, 2 rejected.  Accepted: the solve succeeded, min_radius <= r <= max_radius,
            rmse <= max_rmse and sqrt(cu^2 + cv^2) <= r (the centroid of points on a cylinder's surface lies inside it, also for a
            one-sided scan).  radius_fit, rmse and the centre c + cu e1 + cv e2 are NaN unless state is 1.
  radii     on the host, in node order (a parent's index is smaller than its child's), with util.branches' orders and branch ids.  A
            root takes its radius_fit; if that is NaN, the first finite radius_fit along its own branch; else NaN.  A node with a parent:
            cap = max_growth * radius[parent]; cap NaN: radius = radius_fit; radius_fit finite: min(radius_fit, cap); else cap.
  segments  a node with a parent and both radii finite is a frustum of length seg with the radii R (parent) and r (node): volume
            pi seg / 3 (R^2 + R r + r^2), lateral area pi (R + r) sqrt(seg^2 + (R - r)^2).  Every other node contributes nothing.
  columns   wood_nodes_fit (integer: the nodes whose radius == radius_fit), wood_length (seg over the modelled segments), wood_volume,
            wood_area, axis_volume (the segments whose node lies on the axis branch), branch_volume (on the counted branches: order >= 1
            and length >= util.branches' min_branch), branch_volume_1 (order 1 of them), axis_dbh (2 x the radius interpolated linearly in
            the height above z_ref at dbh_height, between the first (parent, child) pair of axis nodes with h_parent <= dbh_height <
            h_child and both radii finite; NaN without one), branch_base_diam_1 (the mean of 2 radius[first node] over the counted order-1
            branches with a finite value; NaN without one).  NaN (0 in the integer column) where there is no skeleton; 0.0 in the sums
            of a skeleton without a modelled segment.
  cylinders "cylinders": ragged like "skeleton", with its node_start: radius_fit, radius f64 [M], n i64, rmse f64, state i32, centre f64
            [M, 3], axis f64 [M, 3], length, volume f64 [M] (0.0 for a node that is no segment).  `offset` is added to centre, to z as well.

Known limits: leaves are rows like wood -- in leaf-on scans only the rmse and radius gates and the parent cap hold them back; a Kasa fit
on a short arc is biased (towards a smaller radius under noise); an unfitted tip inherits its parent's radius; a node's axis is the
parent -> node chord, not a fitted direction, so a node seen across a bend is fitted as an ellipse; with max_growth = 1 a perfectly
cylindrical stem sits on its cap (radius_fit and cap agree to rounding), so whether such a node counts in wood_nodes_fit is no property
of the input.

csrc/tl_wood.hip gives every row its node (tl_wood_row_nodes), one stable torch sort and one searchsorted make every node a contiguous
range of the permutation, tl_wood_fit runs one wavefront per node.  There is no CPU fallback."""
import argparse
import math
import sys

import numpy as np

WOOD_DEFAULTS = dict(min_points=8, max_rmse=0.03, min_radius=0.005, max_radius=1.0, max_growth=1.0, dbh_height=1.3)
WOOD_COLUMNS = ("wood_nodes_fit", "wood_length", "wood_volume", "wood_area", "axis_volume", "branch_volume", "branch_volume_1", "axis_dbh",
                "branch_base_diam_1")
WOOD_INT_COLUMNS = ("wood_nodes_fit",)
CYLINDER_KEYS = ("node_start", "radius_fit", "radius", "n", "rmse", "state", "centre", "axis", "length", "volume")
STAGES = ("wood row nodes", "wood sort", "wood fit")
FIT_KEYS = ("radius_fit", "n", "rmse", "state", "centre", "axis")
_HELP = dict(min_points="a node of fewer rows than this gets no fit", max_rmse="a fit with a larger residual than this is rejected, metres",
             min_radius="a fit of a smaller radius than this is rejected, metres", max_radius="a fit of a larger radius than this is rejected, metres",
             max_growth="a node's radius is at most this times its parent's", dbh_height="height above the reference at which axis_dbh is read, metres")

__all__ = ["WOOD_DEFAULTS", "WOOD_COLUMNS", "check_params", "add_arguments", "params_of", "write_cylinders"]


def check_params(cfg=None, **kw):
    """The six parameters as a dict of plain numbers (defaults filled in); ValueError for an unknown name or a value outside its
    constraint (the table of DESIGN §24).  Touches no GPU."""
    p = dict(WOOD_DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in WOOD_DEFAULTS:
                raise ValueError(f"unknown wood parameter {k!r}; expected one of {tuple(WOOD_DEFAULTS)}")
            if v is not None:
                p[k] = v
    for k in WOOD_DEFAULTS:
        if isinstance(p[k], bool) or not np.isfinite(p[k]):
            raise ValueError(f"{k} must be a finite number, got {p[k]!r}")
        if k == "min_points":
            if int(p[k]) != p[k]:
                raise ValueError(f"min_points must be an integer, got {p[k]!r}")
            p[k] = int(p[k])
        else:
            p[k] = float(p[k])
    if not 3 <= p["min_points"] < 1 << 62:
        raise ValueError(f"min_points must be >= 3, got {p['min_points']!r}")
    for k in ("max_rmse", "min_radius", "dbh_height"):
        if not p[k] >= 0:
            raise ValueError(f"{k} must be >= 0, got {p[k]!r}")
    if not p["min_radius"] < p["max_radius"]:
        raise ValueError(f"min_radius must be < max_radius, got {p['min_radius']!r} and {p['max_radius']!r}")
    if not p["max_growth"] >= 1:
        raise ValueError(f"max_growth must be >= 1, got {p['max_growth']!r}")
    return p


def wood_stage(xyz, branch_dev, T, p, mark):
    """The stage on the device, without a host synchronise.  xyz f64 [m, 3]: the gathered rows in label order, branch_dev: what
    util.branches.branch_stage returned for them, p: checked parameters, mark(name): closes a timed stage.  Returns a dict of device
    tensors: row_node i32 [m] and, per node, radius_fit f64 [M], n i64, rmse f64, state i32, centre f64 [M, 3], axis f64 [M, 3]."""
    import torch
    from .. import _hip
    lib, dev, m = _hip.lib(), xyz.device, len(xyz)
    M, U = len(branch_dev["xyz"]), len(branch_dev["voxel_keys"])
    f64, i64, i32 = (dict(dtype=t, device=dev) for t in (torch.float64, torch.int64, torch.int32))
    nan = float("nan")
    out = dict(row_node=torch.full((m,), -1, **i32), radius_fit=torch.full((M,), nan, **f64), n=torch.zeros(M, **i64), rmse=torch.full((M,), nan, **f64),
               state=torch.zeros(M, **i32), centre=torch.full((M, 3), nan, **f64), axis=torch.zeros((M, 3), **f64))
    if not (m and M):
        for name in STAGES:
            mark(name)
        return out
    _hip.check(lib.tl_wood_row_nodes(_hip.ptr(branch_dev["row_keys"]), m, _hip.ptr(branch_dev["voxel_keys"]), U, _hip.ptr(branch_dev["d"]),
                                     _hip.ptr(branch_dev["uf_parent"]), _hip.ptr(branch_dev["node_id"]), M, _hip.ptr(out["row_node"]), _hip.stream()),
               "tl_wood_row_nodes")
    mark(STAGES[0])
    vals, perm = torch.sort(out["row_node"], stable=True)
    start = torch.searchsorted(vals, torch.arange(M + 1, **i32)).contiguous()
    mark(STAGES[1])
    _hip.check(lib.tl_wood_fit(_hip.ptr(xyz), m, _hip.ptr(perm), _hip.ptr(start), _hip.ptr(branch_dev["xyz"]), _hip.ptr(branch_dev["parent"]),
                               _hip.ptr(branch_dev["node_start"]), T, M, _hip.WoodParams(**p), _hip.ptr(out["radius_fit"]), _hip.ptr(out["n"]),
                               _hip.ptr(out["rmse"]), _hip.ptr(out["state"]), _hip.ptr(out["centre"]), _hip.ptr(out["axis"]), _hip.stream()),
               "tl_wood_fit")
    mark(STAGES[2])
    return out


def radii(parent, branch, radius_fit, max_growth):
    """Step 5 on one tree's node table: parent (local, -1 for a root), branch: lists, radius_fit: a list of floats.  Returns the radii."""
    n = len(parent)
    radius = [math.nan] * n
    first = {}                                                                       # branch id -> its first finite radius_fit
    for i in range(n):
        if radius_fit[i] == radius_fit[i] and branch[i] not in first:
            first[branch[i]] = radius_fit[i]
    for i in range(n):
        q, rf = parent[i], radius_fit[i]
        if q < 0:
            radius[i] = rf if rf == rf else first.get(branch[i], math.nan)
            continue
        cap = max_growth * radius[q]
        if cap != cap:
            radius[i] = rf
        elif rf == rf:
            radius[i] = min(rf, cap)
        else:
            radius[i] = cap
    return radius


def to_columns(skeleton, fits, z_ref, p, branch_p, off):
    """Steps 5-8 on the host, float64.  skeleton: the "skeleton" table of util.branches.to_columns *without* the offset (node_start, xyz,
    parent, order, branch), fits: the host arrays of wood_stage (FIT_KEYS), z_ref f64 [T], p / branch_p: the checked wood and branch
    parameters, off: 3 values added to centre, or None.  Returns WOOD_COLUMNS and "cylinders"."""
    node_start, xyz = skeleton["node_start"], skeleton["xyz"]
    T, M = len(node_start) - 1, len(skeleton["parent"])
    col = {k: (np.zeros(T, np.int64) if k in WOOD_INT_COLUMNS else np.full(T, np.nan)) for k in WOOD_COLUMNS}
    radius, length, volume = np.full(M, np.nan), np.zeros(M), np.zeros(M)
    pi, growth, dbh_h, min_branch = math.pi, p["max_growth"], p["dbh_height"], branch_p["min_branch"]
    for t in range(T):
        a, b = int(node_start[t]), int(node_start[t + 1])
        n = b - a
        if n == 0:
            continue
        c, par, br, o = xyz[a:b], skeleton["parent"][a:b], skeleton["branch"][a:b], skeleton["order"][a:b]
        rf = fits["radius_fit"][a:b]
        up = np.maximum(par, 0)
        df = c - c[up]
        seg = np.sqrt(df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1] + df[:, 2] * df[:, 2])
        seg[par < 0] = 0.0
        r = np.asarray(radii(par.tolist(), br.tolist(), rf.tolist(), growth), np.float64)            # the one sequential rule
        # the branches as util.branches.decompose numbers and measures them: by their first node, seg added in node order
        b_first = np.unique(br, return_index=True)[1]
        b_len, b_order = np.bincount(br, weights=seg), o[b_first]
        counted = (b_order >= 1) & (b_len >= min_branch)
        roots = np.flatnonzero(par < 0)
        if len(roots) > 1:                                                            # the axis: the root with the largest down, the first among equals
            down, best_v, sg, pr = [0.0] * n, [-1.0] * n, seg.tolist(), par.tolist()
            for j in range(n - 1, -1, -1):
                q = pr[j]
                if q >= 0 and sg[j] + down[j] >= best_v[q]:
                    best_v[q] = down[q] = sg[j] + down[j]
            roots = [max(roots.tolist(), key=lambda i: (down[i], -i))]
        axis = br[roots[0]]
        R = r[up]
        seen = (par >= 0) & ~np.isnan(r) & ~np.isnan(R)                                 # the modelled segments
        vol = np.where(seen, pi * seg / 3.0 * (R * R + R * r + r * r), 0.0)
        area = np.where(seen, pi * (R + r) * np.sqrt(seg * seg + (R - r) * (R - r)), 0.0)
        on_axis, on_counted = seen & (br == axis), seen & counted[br]
        col["wood_length"][t], col["wood_volume"][t], col["wood_area"][t] = seg[seen].sum(), vol[seen].sum(), area[seen].sum()
        col["axis_volume"][t], col["branch_volume"][t] = vol[on_axis].sum(), vol[on_counted].sum()
        col["branch_volume_1"][t] = vol[on_counted & (b_order[br] == 1)].sum()
        zr = z_ref[t]
        hq, hi = c[up, 2] - zr, c[:, 2] - zr
        pair = np.flatnonzero(on_axis & (br[up] == axis) & (hq <= dbh_h) & (dbh_h < hi))
        if len(pair):
            i = pair[0]
            col["axis_dbh"][t] = 2.0 * (R[i] + (r[i] - R[i]) * ((dbh_h - hq[i]) / (hi[i] - hq[i])))
        base = 2.0 * r[b_first[counted & (b_order == 1)]]
        base = base[~np.isnan(base)]
        if len(base):
            col["branch_base_diam_1"][t] = base.sum() / len(base)
        col["wood_nodes_fit"][t] = int((r == rf).sum())
        radius[a:b], length[a:b], volume[a:b] = r, np.where(seen, seg, 0.0), vol
    out = {k: col[k] for k in WOOD_COLUMNS}
    centre = fits["centre"] + off[None, :] if off is not None else fits["centre"]
    out["cylinders"] = dict(node_start=node_start, radius_fit=fits["radius_fit"], radius=radius, n=fits["n"], rmse=fits["rmse"], state=fits["state"],
                            centre=centre, axis=fits["axis"], length=length, volume=volume)
    return out


def write_cylinders(path, inv):
    """An .npz of tree_id [T] and the ragged cylinder table (CYLINDER_KEYS) of an inventory taken with wood=True."""
    if "cylinders" not in inv:
        raise ValueError("the inventory holds no cylinders: take it with wood=True")
    cyl = inv["cylinders"]
    with open(path, "wb") as f:
        np.savez(f, tree_id=np.asarray(inv["tree_id"], np.int64), **{k: cyl[k] for k in CYLINDER_KEYS})
    return path


def add_arguments(ap):
    """One --wood-... option per parameter (shared with util.segment, util.inventory, util.stem, util.crown and util.branches)."""
    for k, v in WOOD_DEFAULTS.items():
        opt = "--wood-" + k.replace("_", "-")
        if opt not in ap._option_string_actions:
            ap.add_argument(opt, type=int if k == "min_points" else float, default=v, help=_HELP[k])


def params_of(a):
    return {k: getattr(a, "wood_" + k) for k in WOOD_DEFAULTS}


def main(argv=None):
    import os
    from . import branches as _branches, inventory as _inventory, terrain as _terrain
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.wood", description="cylinder model (node radii, wood volume by branch order) of a labelled cloud")
    ap.add_argument("--forest", required=True, help="labelled cloud: .npy / .npz / .txt / .las, N x 4 (x y z label)")
    ap.add_argument("--out", required=True, help=".npz to write: tree_id and the cylinder table (" + ", ".join(CYLINDER_KEYS) + ")")
    ap.add_argument("--csv", default=None, help="also write the tree inventory with the branch and wood columns as CSV")
    _inventory.add_arguments(ap)
    _branches.add_arguments(ap)
    add_arguments(ap)
    ap.add_argument("--leafwood", action="store_true", help="separate leaves from wood first (util.leafwood): the cylinders are those of the wood rows")
    from . import leafwood as _leafwood
    _leafwood.add_arguments(ap)
    ap.add_argument("--terrain", action="store_true", help="measure heights from the terrain of the label-0 rows (z_ground) instead of z_low")
    _terrain.add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        wood_cfg = check_params(params_of(a))
        leafwood_cfg = _leafwood.check_params(_leafwood.params_of(a))
        lw_scales = _leafwood.check_scales(_leafwood.scales_of(a))
        branch_cfg = _branches.check_params(_branches.params_of(a))
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
    inv = _inventory.cloud_inventory(data, terrain=a.terrain, terrain_cfg=terrain_cfg if a.terrain else None, branches=True, branch_cfg=branch_cfg,
                                     wood=True, wood_cfg=wood_cfg, leafwood=a.leafwood, leafwood_cfg=leafwood_cfg if a.leafwood else None,
                                     leafwood_scales=lw_scales["scales"], leafwood_scales_min=lw_scales["scales_min"], **params)
    write_cylinders(a.out, inv)
    if a.csv:
        _inventory.write_inventory(a.csv, inv)
    nodes = len(inv["cylinders"]["state"])
    print(f"{a.forest}: {len(data)} points, {len(inv['tree_id'])} trees, {nodes} nodes, {int((inv['cylinders']['state'] == 1).sum())} fitted, "
          f"{float(np.nansum(inv['wood_volume'])):.4f} m3 of wood -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
