"""Branch structure of a segmented forest on the device: the skeleton of every tree, how long its wood is, how many branches it has, of
which order, and where the first one leaves the stem.

    python -m treelearn_amd.util.branches --forest labelled.npy|npz|txt|las --out skeletons.npz [--csv trees.csv] [--terrain] [--wood] [--leafwood] [--branch-voxel 0.1 ...]

The semantics are the project's own; tests/branches_restatement.py states them in plain Python.  The stage runs inside
util.inventory.tree_inventory(..., branches=True) on the label-sorted rows and the tree table that function already holds on the device.
Per tree with rows: the position (px, py) and a reference height z_ref (z_ground with a terrain, z_low without).

  voxels    (ix, iy, iz) = floor(coordinate / voxel), one grid for all trees; a tree's voxels are the distinct voxels of its rows with
            iz >= izr, (ipx, ipy, izr) = floor((px, py, z_ref) / voxel).  More than max_voxels of them: skel_voxels and no skeleton.
  graph     an edge between two voxels of one tree with max(|dx|, |dy|, |dz|) <= reach, of the integer weight
            floor(sqrt(10000 * (dx^2 + dy^2 + dz^2))): 100, 141, 173, and 200 .. 346 with reach 2.  Never between two trees.
  sources   of the voxels with max(|ix - ipx|, |iy - ipy|) <= base_reach, those fewer than base_layers above the lowest of them.  None:
            no skeleton.
  distance  d(v): the shortest path from the sources, int32, 0 on them, -1 where no path leads.
  nodes     bin(v) = d(v) // (100 * level); a node is a connected component of reached voxels of one bin, numbered per tree in ascending
            (bin, smallest voxel); its centroid is ((double)sum / (double)count + 0.5) * voxel per axis.  The parent of a node of bin > 0 is
            the node of the predecessor of its voxel v* with the smallest (d, key): the neighbour u with d(u) + w(u, v*) = d(v*) of the
            smallest key.  Voxel keys order by (ix, iy, iz).
  branches  on the host, float64: seg[i] = the distance of node i's centroid from its parent's (0 for a root), path[i] = path[parent] +
            seg[i], down[i] = the largest seg[j] + down[j] over the children j (0 for a tip).  The child with the largest seg[j] + down[j]
            (the smallest index among equals) continues its parent's branch; every other child starts a branch of the next order; a root
            starts a branch of order 0.  The axis is the branch of the root with the largest down (the smallest index among equals).
            Branches are numbered by their first node; a branch's length is the sum of seg over its nodes, its attachment height the z
            of its first node's parent above z_ref; it is counted with an order >= 1 and a length >= min_branch.
  columns   skel_voxels, skel_reached, skel_nodes, skel_tips (integers); skel_length (the sum of every seg), axis_length, axis_top_h
            (the axis' last node above z_ref), path_mean_tips; branch_count, branch_count_1 (order 1), branch_length (the sum over the
            counted branches, 0.0 without one), branch_order_max (0 without one), first_branch_h (the lowest attachment height >=
            min_height among the counted order-1 branches that leave the axis; NaN without one).  NaN (0 in the integer columns)
            where there is no skeleton.
  skeleton  "skeleton": the ragged node table of all trees: node_start i64 [T + 1], xyz f64 [M, 3], parent i32 [M] (index local to the
            tree, -1 for a root), bin i32, count i64, order i32, branch i32 (local to the tree).  `offset` is added to xyz.

Known limits: an occlusion gap wider than reach leaves voxels unreached, which skel_reached < skel_voxels reports and nothing bridges;
leaves are voxels like wood; a loop in the graph is cut where the distances from both sides meet; low vegetation near the base joins the
sources; a row more than 2047 voxels from its tree's position in x or y, or 2047 or more above z_ref, is an error; max_voxels is at most
2^22 and level at most 10^6, so that every distance fits int32.

csrc/tl_skeleton.hip gives every row a (tree, ix, iy, iz) key (tl_skel_voxel_keys); one torch sort and unique makes every tree a
contiguous range of voxels; tl_skel_distance runs one workgroup per tree, tl_skel_nodes one thread per voxel, tl_skel_links one thread
per node.  There is no CPU fallback."""
import argparse
import sys

import numpy as np

BRANCH_DEFAULTS = dict(voxel=0.1, reach=1, base_reach=10, base_layers=5, level=3, min_branch=0.5, min_height=1.0, max_voxels=1 << 20)
BRANCH_COLUMNS = ("skel_voxels", "skel_reached", "skel_nodes", "skel_tips", "skel_length", "axis_length", "axis_top_h", "path_mean_tips",
                  "branch_count", "branch_count_1", "branch_length", "branch_order_max", "first_branch_h")
BRANCH_INT_COLUMNS = ("skel_voxels", "skel_reached", "skel_nodes", "skel_tips", "branch_count", "branch_count_1", "branch_order_max")
SKELETON_KEYS = ("node_start", "xyz", "parent", "bin", "count", "order", "branch")
STAGES = ("branch voxel keys", "branch sort + unique", "branch distance", "branch nodes", "branch links")
_INT = ("reach", "base_reach", "base_layers", "level", "max_voxels")
_TREE_SHIFT = 35                                                                                 # the tree field of a voxel key
MAX_VOXELS, MAX_LEVEL = 1 << 22, 10 ** 6
_HELP = dict(voxel="edge of the voxels, metres", reach="voxels within this many steps are neighbours (1 or 2)",
             base_reach="the stem base: voxels within this many of the tree's position in x and y (0..2047)",
             base_layers="the lowest this many voxel layers of the stem base are the sources of the distance",
             level="thickness of a level set of the distance, voxels", min_branch="a branch shorter than this is not counted, metres",
             min_height="a first branch attached below this is left out, metres",
             max_voxels="a tree of more voxels than this gets no skeleton (at most 2^22)")

__all__ = ["BRANCH_DEFAULTS", "BRANCH_COLUMNS", "check_params", "add_arguments", "params_of", "write_skeletons"]


def check_params(cfg=None, **kw):
    """The eight parameters as a dict of plain numbers (defaults filled in); ValueError for an unknown name or a value outside its
    constraint (the table of DESIGN §23).  Touches no GPU."""
    p = dict(BRANCH_DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in BRANCH_DEFAULTS:
                raise ValueError(f"unknown branch parameter {k!r}; expected one of {tuple(BRANCH_DEFAULTS)}")
            if v is not None:
                p[k] = v
    for k in BRANCH_DEFAULTS:
        if k in _INT:
            if isinstance(p[k], bool) or not np.isfinite(p[k]) or int(p[k]) != p[k]:
                raise ValueError(f"{k} must be an integer, got {p[k]!r}")
            p[k] = int(p[k])
        else:
            p[k] = float(p[k])
            if not np.isfinite(p[k]):
                raise ValueError(f"{k} must be finite, got {p[k]!r}")
    if not p["voxel"] > 0:
        raise ValueError(f"voxel must be > 0, got {p['voxel']!r}")
    for k in ("min_branch", "min_height"):
        if not p[k] >= 0:
            raise ValueError(f"{k} must be >= 0, got {p[k]!r}")
    if p["reach"] not in (1, 2):
        raise ValueError(f"reach must be 1 or 2, got {p['reach']!r}")
    if not 0 <= p["base_reach"] <= 2047:
        raise ValueError(f"base_reach must be in 0..2047, got {p['base_reach']!r}")
    if not 1 <= p["base_layers"] < 1 << 62:
        raise ValueError(f"base_layers must be >= 1, got {p['base_layers']!r}")
    if not 1 <= p["level"] <= MAX_LEVEL:
        raise ValueError(f"level must be in 1..{MAX_LEVEL}, got {p['level']!r}")
    if not 1 <= p["max_voxels"] <= MAX_VOXELS:
        raise ValueError(f"max_voxels must be in 1..{MAX_VOXELS}, got {p['max_voxels']!r}")
    return p


def branch_stage(xyz, kept_lab, T, tree, p, mark):
    """The stage on the device.  xyz f64 [m, 3]: the gathered rows in label order, kept_lab i64 [m]: their labels, tree f64 [T, 4] = px, py,
    z_ref, z_top per tree, p: checked parameters, mark(name): closes a timed stage.  Returns a dict of device tensors: voxel_keys i64 [U]
    (the distinct voxels, ascending), kstart i64 [T + 1], d i32 [U], rounds i32 [T], node_start i64 [T + 1], xyz f64 [M, 3], parent, bin
    i32 [M], count i64 [M], and err i32 [1] (or None: no rows); the caller raises branch_error() when err reads non-zero.  For util.wood
    also row_keys i64 [m] (every row's voxel key), uf_parent i32 [U] (the union-find forest of the nodes) and node_id i32 [U]."""
    import torch
    from .. import _hip
    lib, dev, m = _hip.lib(), xyz.device, len(xyz)
    sp = _hip.SkeletonParams(**p)
    i64, i32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.int32, device=dev)
    out = dict(voxel_keys=torch.zeros(0, **i64), kstart=torch.zeros(T + 1, **i64), d=torch.zeros(0, **i32), rounds=torch.zeros(T, **i32),
               node_start=torch.zeros(T + 1, **i64), xyz=torch.zeros((0, 3), dtype=torch.float64, device=dev), parent=torch.zeros(0, **i32),
               bin=torch.zeros(0, **i32), count=torch.zeros(0, **i64), err=None, row_keys=torch.zeros(0, **i64), uf_parent=torch.zeros(0, **i32),
               node_id=torch.zeros(0, **i32))
    U = 0
    if T and m:
        keys = torch.empty(m, **i64)
        out["err"], out["row_keys"] = torch.zeros(1, **i32), keys
        _hip.check(lib.tl_skel_voxel_keys(_hip.ptr(xyz), _hip.ptr(kept_lab), m, _hip.ptr(tree), T, sp, _hip.ptr(keys), _hip.ptr(out["err"]),
                                          _hip.stream()), "tl_skel_voxel_keys")
        mark(STAGES[0])
        vk = torch.unique_consecutive(torch.sort(keys).values)
        vk = vk[vk >= 0].contiguous()
        U = len(vk)
        if U >= 1 << 31:
            raise ValueError(f"{U} voxels: a voxel index is an int32; use a larger branch voxel")
        tree_ids = torch.arange(T + 1, **i64)
        out["voxel_keys"], out["kstart"] = vk, torch.searchsorted(vk, tree_ids << _TREE_SHIFT).contiguous()
        mark(STAGES[1])
    if not U:
        for name in STAGES[0 if not (T and m) else 2:]:
            mark(name)
        return out
    vk, kstart = out["voxel_keys"], out["kstart"]
    d = torch.empty(U, **i32)
    _hip.check(lib.tl_skel_distance(_hip.ptr(vk), U, _hip.ptr(kstart), T, sp, _hip.ptr(d), _hip.ptr(out["rounds"]), _hip.stream()), "tl_skel_distance")
    out["d"] = d
    mark(STAGES[2])
    parent, acc, vstar = torch.empty(U, **i32), torch.empty((U, 4), **i64), torch.empty(U, **i64)
    _hip.check(lib.tl_skel_nodes(_hip.ptr(vk), U, _hip.ptr(kstart), T, sp, _hip.ptr(d), _hip.ptr(parent), _hip.ptr(acc), _hip.ptr(vstar),
                                 _hip.stream()), "tl_skel_nodes")
    out["uf_parent"] = parent
    mark(STAGES[3])
    # the node order: (tree, bin, root) ascending -- the roots come out ascending, one stable sort by (tree, bin) does the rest
    roots = torch.nonzero((parent == torch.arange(U, **i32)) & (d >= 0)).reshape(-1)
    M = len(roots)
    if M:
        troot = vk[roots] >> _TREE_SHIFT
        order = torch.sort((troot << 32) | (d[roots].to(torch.int64) // (100 * p["level"])), stable=True).indices
        roots, troot = roots[order], troot[order].contiguous()
        node_id = torch.full((U,), -1, **i32)
        node_id[roots] = torch.arange(M, **i32)
        out["node_id"] = node_id
        out["node_start"] = torch.searchsorted(troot, tree_ids).contiguous()
        out["xyz"], out["count"] = torch.empty((M, 3), dtype=torch.float64, device=dev), torch.empty(M, **i64)
        out["parent"], out["bin"] = torch.empty(M, **i32), torch.empty(M, **i32)
        roots32 = roots.to(torch.int32).contiguous()
        _hip.check(lib.tl_skel_links(_hip.ptr(vk), U, _hip.ptr(kstart), _hip.ptr(tree), T, sp, _hip.ptr(d), _hip.ptr(parent), _hip.ptr(acc),
                                     _hip.ptr(vstar), _hip.ptr(roots32), M, _hip.ptr(node_id), _hip.ptr(out["node_start"]), _hip.ptr(out["xyz"]),
                                     _hip.ptr(out["parent"]), _hip.ptr(out["bin"]), _hip.ptr(out["count"]), _hip.stream()), "tl_skel_links")
    mark(STAGES[4])
    return out


def branch_error(p):
    return ValueError(f"a coordinate of a tree is not finite, or a row lies more than 2047 branch voxels of {p['voxel']} m from its tree's "
                      "position in x or y, or 2047 or more above its reference height")


def decompose(node_start, xyz, parent, z_ref, p):
    """Step 7 on the host, float64: the branches of every tree from its node table.  node_start i64 [T + 1], xyz f64 [M, 3], parent i32 [M]
    (local, -1 for a root; a parent's index is smaller than its child's), z_ref f64 [T].  Returns (columns: the float and branch columns of
    BRANCH_COLUMNS and skel_tips, each [T]; order i32 [M]; branch i32 [M])."""
    T, M = len(node_start) - 1, len(parent)
    nan = np.full(T, np.nan)
    col = {k: (np.zeros(T, np.int64) if k in BRANCH_INT_COLUMNS else nan.copy()) for k in BRANCH_COLUMNS[3:]}
    order, branch = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for t in range(T):
        a, b = int(node_start[t]), int(node_start[t + 1])
        n = b - a
        if n == 0:
            continue
        c, par = xyz[a:b], parent[a:b]
        df = c - c[np.maximum(par, 0)]
        seg = np.sqrt(df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1] + df[:, 2] * df[:, 2])
        seg[par < 0] = 0.0
        seg, par, cz = seg.tolist(), par.tolist(), c[:, 2].tolist()
        path, down, best, best_v = [0.0] * n, [0.0] * n, [-1] * n, [-1.0] * n
        for i in range(n):
            if par[i] >= 0:
                path[i] = path[par[i]] + seg[i]
        for j in range(n - 1, -1, -1):                                               # children before parents; equals: the smallest index stays
            q = par[j]
            if q >= 0:
                v = seg[j] + down[j]
                if v >= best_v[q]:
                    best[q], best_v[q], down[q] = j, v, v
        b_first, b_last, b_len, b_order, o, br = [], [], [], [], [0] * n, [0] * n     # branches, numbered by their first node
        for i in range(n):
            q = par[i]
            if q >= 0 and best[q] == i:
                o[i], br[i] = o[q], br[q]
                b_last[br[i]] = i
                b_len[br[i]] = b_len[br[i]] + seg[i]
            else:
                o[i], br[i] = (o[q] + 1 if q >= 0 else 0), len(b_first)
                b_first.append(i); b_last.append(i); b_len.append(seg[i]); b_order.append(o[i])
        order[a:b], branch[a:b] = o, br
        roots = [i for i in range(n) if par[i] < 0]
        axis = br[max(roots, key=lambda i: (down[i], -i))]
        tips = [i for i in range(n) if best[i] < 0]
        zr = float(z_ref[t])
        counted = [k for k in range(len(b_first)) if b_order[k] >= 1 and b_len[k] >= p["min_branch"]]
        firsts = [cz[par[b_first[k]]] - zr for k in counted if b_order[k] == 1 and br[par[b_first[k]]] == axis]
        firsts = [h for h in firsts if h >= p["min_height"]]
        col["skel_tips"][t] = len(tips)
        col["skel_length"][t] = sum(seg)
        col["axis_length"][t] = b_len[axis]
        col["axis_top_h"][t] = cz[b_last[axis]] - zr
        col["path_mean_tips"][t] = sum(path[i] for i in tips) / len(tips)
        col["branch_count"][t] = len(counted)
        col["branch_count_1"][t] = sum(1 for k in counted if b_order[k] == 1)
        col["branch_length"][t] = sum(b_len[k] for k in counted)
        col["branch_order_max"][t] = max((b_order[k] for k in counted), default=0)
        if firsts:
            col["first_branch_h"][t] = min(firsts)
    return col, order, branch


def to_columns(host, z_ref, p, off):
    """The host arrays of branch_stage (kstart, node_start, xyz, parent, bin, count as numpy) and z_ref f64 [T] as the inventory's columns:
    BRANCH_COLUMNS and "skeleton" (`off`: 3 values added to xyz, or None)."""
    node_start, count = host["node_start"], host["count"]
    col, order, branch = decompose(node_start, host["xyz"], host["parent"], z_ref, p)
    csum = np.concatenate([np.zeros(1, np.int64), np.cumsum(count, dtype=np.int64)])
    col["skel_voxels"] = np.diff(host["kstart"]).astype(np.int64)
    col["skel_reached"] = csum[node_start[1:]] - csum[node_start[:-1]]
    col["skel_nodes"] = np.diff(node_start).astype(np.int64)
    out = {k: col[k] for k in BRANCH_COLUMNS}
    xyz = host["xyz"] + off[None, :] if off is not None else host["xyz"]
    out["skeleton"] = dict(node_start=node_start, xyz=xyz, parent=host["parent"], bin=host["bin"], count=count, order=order, branch=branch)
    return out


def write_skeletons(path, inv):
    """An .npz of tree_id [T] and the ragged node table (SKELETON_KEYS) of an inventory taken with branches=True."""
    if "skeleton" not in inv:
        raise ValueError("the inventory holds no skeleton: take it with branches=True")
    sk = inv["skeleton"]
    with open(path, "wb") as f:
        np.savez(f, tree_id=np.asarray(inv["tree_id"], np.int64), **{k: sk[k] for k in SKELETON_KEYS})
    return path


def add_arguments(ap):
    """One --branch-... option per parameter (shared with util.segment, util.inventory, util.stem, util.crown, util.wood and util.leafwood)."""
    for k, v in BRANCH_DEFAULTS.items():
        opt = "--branch-" + k.replace("_", "-")
        if opt not in ap._option_string_actions:
            ap.add_argument(opt, type=int if k in _INT else float, default=v, help=_HELP[k])


def params_of(a):
    return {k: getattr(a, "branch_" + k) for k in BRANCH_DEFAULTS}


def main(argv=None):
    import os
    from . import inventory as _inventory, terrain as _terrain
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.branches", description="branch structure (skeleton, branch lengths, orders) of a labelled cloud")
    ap.add_argument("--forest", required=True, help="labelled cloud: .npy / .npz / .txt / .las, N x 4 (x y z label)")
    ap.add_argument("--out", required=True, help=".npz to write: tree_id and the node table (node_start, xyz, parent, bin, count, order, branch)")
    ap.add_argument("--csv", default=None, help="also write the tree inventory with the branch columns as CSV")
    _inventory.add_arguments(ap)
    add_arguments(ap)
    ap.add_argument("--wood", action="store_true", help="add the wood columns (util.wood) to the CSV")
    from . import wood as _wood
    _wood.add_arguments(ap)
    ap.add_argument("--leafwood", action="store_true", help="separate leaves from wood first (util.leafwood): the skeleton is that of the wood rows")
    from . import leafwood as _leafwood
    _leafwood.add_arguments(ap)
    ap.add_argument("--terrain", action="store_true", help="measure heights from the terrain of the label-0 rows (z_ground) instead of z_low")
    _terrain.add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        branch_cfg = check_params(params_of(a))
        wood_cfg = _wood.check_params(_wood.params_of(a))
        leafwood_cfg = _leafwood.check_params(_leafwood.params_of(a))
        lw_scales = _leafwood.check_scales(_leafwood.scales_of(a))
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
                                     wood=a.wood, wood_cfg=wood_cfg if a.wood else None, leafwood=a.leafwood,
                                     leafwood_cfg=leafwood_cfg if a.leafwood else None,
                                     leafwood_scales=lw_scales["scales"], leafwood_scales_min=lw_scales["scales_min"], **params)
    write_skeletons(a.out, inv)
    if a.csv:
        _inventory.write_inventory(a.csv, inv)
    ok = int((inv["skel_nodes"] > 0).sum())
    print(f"{a.forest}: {len(data)} points, {len(inv['tree_id'])} trees, {ok} with a skeleton, {int(inv['skel_nodes'].sum())} nodes, "
          f"{int(inv['branch_count'].sum())} branches -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
