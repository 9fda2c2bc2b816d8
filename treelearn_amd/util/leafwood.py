"""Leaf-wood separation of a segmented forest on the device: which rows of every tree are wood, so that the skeleton and the cylinder
model of a leaf-on scan are figures about wood and not about foliage.

    python -m treelearn_amd.util.leafwood --forest labelled.npy|npz|txt|las --out leafwood.npy [--csv trees.csv] [--terrain] [--leafwood-radius 0.2 ...]

The semantics are the project's own; tests/leafwood_restatement.py states them in numpy.  The stage runs inside
util.inventory.tree_inventory(..., leafwood=True) on the label-sorted rows and the tree table that function already holds on the device,
behind the crown stage and in front of util.branches.  All rules are per gathered row (label >= 1).

  features  linearity, planarity, verticality and number_of_neighbors of util.features at `radius`, over all gathered rows,
            whichever tree they belong to: one sorted_cells, one feature_pieces, one eigen_features_sorted.
  seed      s0 = 1 when number_of_neighbors >= min_neighbours, the three features are finite and (linearity >= linearity_min: a limb;
            or planarity >= planarity_min and verticality >= verticality_min: a patch of stem surface).  f32 widened to f64; NaN gives 0.
  vote      vote_iters synchronous rounds.  For a row p: a = the rows of the same tree with dx dx + dy dy + dz dz <= radius radius (f64, no
            contraction; p included), w = those of them whose flag is 1; the new flag is 1 exactly when 100 w >= vote_percent a.
  keys      every gathered row gets the voxel key of tl_skel_voxel_keys (`voxel`, `reach`; its error raises util.branches' ValueError);
            the rows whose flag is 0 then take -1.  One sort and unique_consecutive: the wood voxels per tree.
  components  under §23's edges (max(|dx|, |dy|, |dz|) <= reach, never between trees): tl_skel_nodes with d = 0 everywhere, so that every
            voxel is reached and in bin 0: a node is a component, acc its voxel count.  A component of fewer than min_component voxels is
            dropped: its rows get 0.  Rows with key -1 (below z_ref, a tree without a position) keep their voted flag.
  columns   lw_wood_points, lw_leaf_points, lw_components (the kept ones; integers), lw_wood_share = wood / (wood + leaf) (NaN for an empty
            tree), lw_wood_top_h = the largest z of a wood row minus z_ref (NaN without a wood row or without a finite z_ref).
  "leafwood"  a dict: wood u8 [N] in the input row order (0 for rows of a label < 1) and the parameters.
  filter    True: util.branches and util.wood read the wood rows only (the tree table stays that of all rows; the stem and crown stages
            are untouched: a crown is its leaves).  False: their outputs are the bits of a call without leafwood.

  scales    (tests/leafwood_scales_restatement.py) `scales` = 1 to 4 ascending radii and `scales_min`, beside the eleven parameters
            (check_scales; --leafwood-scales R [R ...] --leafwood-scales-min K): the features at every scale from one sorted_cells at
            max(scales) and one tl_eigen_features_scales; the seed rule per scale (a scale with fewer than min_neighbours neighbours does not
            hold); s0 = 1 when at least scales_min scales hold (tl_leafwood_seed_scales).  The vote keeps `radius`.  Without `scales`
            nothing changes.  Recommended for leaf-on broadleaves: scales 0.1 0.3 0.4 with scales_min 2 (the grid of §26).

Known limits: the seed is one scale unless `scales` is given; conifer needles along a twig are linear like the twig; a stem patch scanned from one side at long
range may fall under min_neighbours; the features see the neighbouring trees' rows while the vote does not; the thresholds are defaults,
not fitted to any species.

csrc/tl_leafwood.hip holds the seed rule (tl_leafwood_seed, one thread per row) and the vote (tl_leafwood_vote, one wave per piece of the
cell-sorted rows; the next round's tag is its second output).  There is no CPU fallback."""
import argparse
import sys

import numpy as np

LEAFWOOD_DEFAULTS = dict(radius=0.2, min_neighbours=5, linearity_min=0.6, planarity_min=0.3, verticality_min=0.2, vote_iters=2, vote_percent=50,
                         voxel=0.1, reach=1, min_component=20, filter=True)
LEAFWOOD_COLUMNS = ("lw_wood_points", "lw_leaf_points", "lw_components", "lw_wood_share", "lw_wood_top_h")
LEAFWOOD_INT_COLUMNS = ("lw_wood_points", "lw_leaf_points", "lw_components")
FEATURES = ("linearity", "planarity", "verticality", "number_of_neighbors")                     # the columns tl_leafwood_seed reads
MAX_VOTE_ITERS = 8
STAGES = ("leafwood cell sort", "leafwood features", "leafwood seed") + tuple(f"leafwood vote {i + 1}" for i in range(MAX_VOTE_ITERS)) + \
    ("leafwood keys + unique", "leafwood components")
_INT = ("min_neighbours", "vote_iters", "vote_percent", "reach", "min_component")
_UNIT = ("linearity_min", "planarity_min", "verticality_min")
_TREE_SHIFT = 35                                                                                 # the tree field of a voxel key
_HELP = dict(radius="radius of the feature and vote neighbourhoods, metres", min_neighbours="a row with fewer neighbours than this is no seed",
             linearity_min="a row at least this linear is a seed (a limb)", planarity_min="a row at least this planar ...",
             verticality_min="... and at least this vertical is a seed (a patch of stem surface)",
             vote_iters="rounds of the neighbourhood vote (0..8)", vote_percent="a row is wood when at least this share of its neighbours is, percent",
             voxel="edge of the voxels of the connectivity filter, metres", reach="voxels within this many steps are connected (1 or 2)",
             min_component="a connected component of fewer wood voxels than this is dropped",
             filter="1: the branch and wood stages read the wood rows only; 0: they read every row")

__all__ = ["LEAFWOOD_DEFAULTS", "LEAFWOOD_COLUMNS", "LEAFWOOD_INT_COLUMNS", "check_params", "add_arguments", "params_of", "write_leafwood",
           "LEAFWOOD_SCALE_DEFAULTS", "check_scales", "scales_of"]


def stages_of(p):
    """The stage names a call with the checked parameters p closes, in order."""
    return STAGES[:3 + p["vote_iters"]] + STAGES[-2:]


def check_params(cfg=None, **kw):
    """The eleven parameters as a dict of plain values (defaults filled in); ValueError for an unknown name or a value outside its
    constraint (the table of DESIGN §25).  Touches no GPU."""
    p = dict(LEAFWOOD_DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in LEAFWOOD_DEFAULTS:
                raise ValueError(f"unknown leafwood parameter {k!r}; expected one of {tuple(LEAFWOOD_DEFAULTS)}")
            if v is not None:
                p[k] = v
    if not isinstance(p["filter"], (bool, np.bool_)):
        raise ValueError(f"filter must be a bool, got {p['filter']!r}")
    p["filter"] = bool(p["filter"])
    for k in LEAFWOOD_DEFAULTS:
        if k == "filter":
            continue
        if isinstance(p[k], (bool, np.bool_)) or not isinstance(p[k], (int, float, np.integer, np.floating)) or not np.isfinite(p[k]):
            raise ValueError(f"{k} must be a finite number, got {p[k]!r}")
        if k in _INT:
            if int(p[k]) != p[k]:
                raise ValueError(f"{k} must be an integer, got {p[k]!r}")
            p[k] = int(p[k])
        else:
            p[k] = float(p[k])
    for k in ("radius", "voxel"):
        if not p[k] > 0:
            raise ValueError(f"{k} must be > 0, got {p[k]!r}")
    for k in _UNIT:
        if not 0 <= p[k] <= 1:
            raise ValueError(f"{k} must be in [0, 1], got {p[k]!r}")
    if not 3 <= p["min_neighbours"] < 1 << 62:
        raise ValueError(f"min_neighbours must be >= 3, got {p['min_neighbours']!r}")
    if not 0 <= p["vote_iters"] <= MAX_VOTE_ITERS:
        raise ValueError(f"vote_iters must be in 0..{MAX_VOTE_ITERS}, got {p['vote_iters']!r}")
    if not 1 <= p["vote_percent"] <= 100:
        raise ValueError(f"vote_percent must be in 1..100, got {p['vote_percent']!r}")
    if p["reach"] not in (1, 2):
        raise ValueError(f"reach must be 1 or 2, got {p['reach']!r}")
    if not 1 <= p["min_component"] < 1 << 62:
        raise ValueError(f"min_component must be >= 1, got {p['min_component']!r}")
    return p


LEAFWOOD_SCALE_DEFAULTS = dict(scales=None, scales_min=1)
MAX_SCALES = 4                                                                                   # TL_FEAT_MAX_SCALES


def check_scales(cfg=None, **kw):
    """The two scale parameters of the seed as a dict of plain values: `scales` None (the one-scale seed at `radius`) or a
    list of 1..4 finite radii > 0 in strictly ascending order, `scales_min` an integer in 1..len(scales) (1 with scales None).
    ValueError otherwise.  Touches no GPU."""
    s = dict(LEAFWOOD_SCALE_DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in LEAFWOOD_SCALE_DEFAULTS:
                raise ValueError(f"unknown leafwood scale parameter {k!r}; expected one of {tuple(LEAFWOOD_SCALE_DEFAULTS)}")
            if v is not None:
                s[k] = v
    m = s["scales_min"]
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, float, np.integer, np.floating)) or not np.isfinite(m) or int(m) != m:
        raise ValueError(f"scales_min must be an integer, got {m!r}")
    s["scales_min"] = int(m)
    if s["scales"] is None:
        if s["scales_min"] != 1:
            raise ValueError(f"scales_min must be 1 without scales, got {m!r}")
        return s
    from .features import check_radii
    try:
        s["scales"] = check_radii(s["scales"])
    except ValueError as e:
        raise ValueError(f"scales: {e}") from None
    if not 1 <= s["scales_min"] <= len(s["scales"]):
        raise ValueError(f"scales_min must be in 1..{len(s['scales'])}, got {m!r}")
    return s


def seed_flags_scales(feats, p, scales_min):
    """tl_leafwood_seed_scales: feats f32 [n, S, 4] on the device (FEATURES at every scale) -> u8 [n]."""
    import torch
    from .. import _hip
    n, S = feats.shape[0], feats.shape[1]
    flag = torch.empty(n, dtype=torch.uint8, device=feats.device)
    _hip.check(_hip.lib().tl_leafwood_seed_scales(_hip.ptr(feats), n, S, _lib_params(p), int(scales_min), _hip.ptr(flag), _hip.stream()),
               "tl_leafwood_seed_scales")
    return flag


def _lib_params(p):
    from .. import _hip
    return _hip.LeafwoodParams(**dict(p, filter=int(p["filter"])))


def seed_flags(feats, p):
    """tl_leafwood_seed: feats f32 [n, 4] on the device (FEATURES) -> u8 [n]."""
    import torch
    from .. import _hip
    n = len(feats)
    flag = torch.empty(n, dtype=torch.uint8, device=feats.device)
    _hip.check(_hip.lib().tl_leafwood_seed(_hip.ptr(feats), n, _lib_params(p), _hip.ptr(flag), _hip.stream()), "tl_leafwood_seed")
    return flag


def vote_rounds(sx, skeys, ext, pieces, tree_sorted, flag, p, mark=None):
    """vote_iters launches of tl_leafwood_vote on cell-sorted rows (util.prepare.sorted_cells at p["radius"]): tree_sorted i32 [n] (>= 0) and
    flag u8 [n] in sorted order -> the voted u8 [n].  The tag of the next round is the kernel's second output; two tag buffers alternate."""
    import ctypes
    import torch
    from .. import _hip
    n = len(sx)
    if not (n and p["vote_iters"]):
        for i in range(p["vote_iters"]):
            if mark:
                mark(STAGES[3 + i])
        return flag
    lib, lp, ext2 = _hip.lib(), _lib_params(p), (ctypes.c_int64 * 2)(ext[0], ext[1])
    tags = [(tree_sorted << 1) | flag.to(torch.int32), torch.empty(n, dtype=torch.int32, device=sx.device)]
    out = torch.empty(n, dtype=torch.uint8, device=sx.device)
    for i in range(p["vote_iters"]):
        _hip.check(lib.tl_leafwood_vote(_hip.ptr(sx), _hip.ptr(skeys), n, ext2, _hip.ptr(pieces), len(pieces), _hip.ptr(tags[i & 1]), lp, _hip.ptr(out),
                                        _hip.ptr(tags[1 - (i & 1)]), _hip.stream()), "tl_leafwood_vote")
        if mark:
            mark(STAGES[3 + i])
    return out


def leafwood_stage(xyz, kept_lab, T, tree, p, mark, scales=None):
    """The stage on the device, without a host synchronise apart from the lengths the sorts read back.  xyz f64 [m, 3]: the gathered rows in
    label order, kept_lab i64 [m]: their labels, tree f64 [T, 4] = px, py, z_ref, z_top per tree, p: checked parameters, mark(name): closes
    a timed stage (stages_of(p)).  Returns a dict of device tensors: wood u8 [m] (in label order), seed and voted u8 [m] (the flags behind
    rules 2 and 3), wood_points, rows, components i64 [T], top_z f64 [T] (-inf without a wood row) and err i32 [1] (or None: no rows); the
    caller raises util.branches.branch_error() when err reads non-zero.
    scales: None (the seed at `radius`, nothing else launched) or a checked dict of check_scales with a list of radii: the features of
    all of them from one sort at max(scales) and one tl_eigen_features_scales, the seed by tl_leafwood_seed_scales; the vote keeps
    `radius` and its own sort at `radius` (shared when max(scales) == radius).  The stage names do not change."""
    import torch
    from .. import _hip
    from . import branches as _branches
    from .features import FEATURE_NAMES
    from .prepare import eigen_features_scales_sorted, eigen_features_sorted, feature_pieces, sorted_cells
    lib, dev, m = _hip.lib(), xyz.device, len(xyz)
    i64, i32, u8 = (dict(dtype=t, device=dev) for t in (torch.int64, torch.int32, torch.uint8))
    out = dict(wood=torch.zeros(m, **u8), seed=torch.zeros(m, **u8), voted=torch.zeros(m, **u8), wood_points=torch.zeros(T, **i64),
               rows=torch.zeros(T, **i64), components=torch.zeros(T, **i64), top_z=torch.full((T,), -np.inf, dtype=torch.float64, device=dev), err=None)
    if not (T and m):
        for name in stages_of(p):
            mark(name)
        return out
    r = p["radius"]
    ids = [FEATURE_NAMES.index(k) for k in FEATURES]
    if scales is None or scales["scales"] is None:
        sx, skeys, perm, ext = sorted_cells(xyz, r)
        pieces = feature_pieces(skeys)
        mark(STAGES[0])
        feats = eigen_features_sorted(sx, skeys, ext, pieces, r, ids)
        mark(STAGES[1])
        seed = seed_flags(feats, p)
        mark(STAGES[2])
    else:
        radii = scales["scales"]
        fx, fkeys, fperm, fext = sorted_cells(xyz, radii[-1])
        fpieces = feature_pieces(fkeys)
        if radii[-1] == r:                                                             # the vote's sort is the features' sort
            sx, skeys, perm, ext, pieces = fx, fkeys, fperm, fext, fpieces
        else:
            sx, skeys, perm, ext = sorted_cells(xyz, r)
            pieces = feature_pieces(skeys)
        mark(STAGES[0])
        feats = eigen_features_scales_sorted(fx, fkeys, fext, fpieces, radii, ids)
        mark(STAGES[1])
        seed = seed_flags_scales(feats, p, scales["scales_min"])
        if fperm is not perm:                                                          # from the features' order to the vote's
            rows = torch.empty_like(seed)
            rows[fperm] = seed
            seed = rows.index_select(0, perm)
        mark(STAGES[2])
    voted = vote_rounds(sx, skeys, ext, pieces, kept_lab.index_select(0, perm).to(torch.int32), seed, p, mark)
    out["seed"][perm], out["voted"][perm] = seed, voted                                # back to label order
    flag = out["voted"]

    # the connectivity filter: the wood voxels per tree, their components, the rows of the small ones dropped
    sp = _hip.SkeletonParams(**dict(_branches.BRANCH_DEFAULTS, voxel=p["voxel"], reach=p["reach"], level=1))
    keys = torch.empty(m, **i64)
    out["err"] = torch.zeros(1, **i32)
    _hip.check(lib.tl_skel_voxel_keys(_hip.ptr(xyz), _hip.ptr(kept_lab), m, _hip.ptr(tree), T, sp, _hip.ptr(keys), _hip.ptr(out["err"]), _hip.stream()),
               "tl_skel_voxel_keys")
    keys = torch.where(flag != 0, keys, torch.full_like(keys, -1))
    vk = torch.unique_consecutive(torch.sort(keys).values)
    vk = vk[vk >= 0].contiguous()
    U = len(vk)
    if U >= 1 << 31:
        raise ValueError(f"{U} voxels: a voxel index is an int32; use a larger leafwood voxel")
    mark(STAGES[-2])
    wood = flag
    if U:
        kstart = torch.searchsorted(vk, torch.arange(T + 1, **i64) << _TREE_SHIFT).contiguous()
        d, parent, acc, vstar = torch.zeros(U, **i32), torch.empty(U, **i32), torch.empty((U, 4), **i64), torch.empty(U, **i64)
        _hip.check(lib.tl_skel_nodes(_hip.ptr(vk), U, _hip.ptr(kstart), T, sp, _hip.ptr(d), _hip.ptr(parent), _hip.ptr(acc), _hip.ptr(vstar), _hip.stream()),
                   "tl_skel_nodes")
        # every row's component: tl_wood_row_nodes with the identity as the node table hands back the root voxel of the row's voxel
        ident, row_root = torch.arange(U, **i32), torch.empty(m, **i32)
        _hip.check(lib.tl_wood_row_nodes(_hip.ptr(keys), m, _hip.ptr(vk), U, _hip.ptr(d), _hip.ptr(parent), _hip.ptr(ident), U, _hip.ptr(row_root),
                                         _hip.stream()), "tl_wood_row_nodes")
        size = acc[:, 0]
        keep_row = (row_root < 0) | (size[row_root.clamp(min=0).to(torch.int64)] >= p["min_component"])
        wood = flag * keep_row.to(torch.uint8)
        kept_root = (parent == ident) & (size >= p["min_component"])
        out["components"] = _range_sums(kept_root, kstart)
    # per tree: the rows are in label order and the voxels in key order, so every tree is a range -- sums by differences of one cumsum,
    # the maximum by a segment reduce (no atomics on T addresses)
    edges = torch.searchsorted(kept_lab, torch.arange(1, T + 2, **i64)).contiguous()
    out["wood"] = wood
    out["wood_points"], out["rows"] = _range_sums(wood, edges), edges[1:] - edges[:-1]
    z = torch.where(wood != 0, xyz[:, 2], torch.full((), -np.inf, dtype=torch.float64, device=dev))
    out["top_z"] = torch.segment_reduce(z, "max", offsets=edges, unsafe=True, initial=-np.inf)      # a maximum: the same bits in any order
    mark(STAGES[-1])
    return out


def _range_sums(v, edges):
    """i64 [len(edges) - 1]: the sums of v (bool or integer) over the ranges [edges[i], edges[i + 1])."""
    import torch
    cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=v.device), torch.cumsum(v.to(torch.int64), 0)])
    return cs[edges[1:]] - cs[edges[:-1]]


HOST_KEYS = ("wood_points", "rows", "components", "top_z")


def to_columns(host, z_ref):
    """The host arrays of leafwood_stage (HOST_KEYS as numpy) and z_ref f64 [T] as the inventory's LEAFWOOD_COLUMNS."""
    wood, rows = host["wood_points"].astype(np.int64), host["rows"].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = wood.astype(np.float64) / rows.astype(np.float64)
        top = np.where(wood > 0, host["top_z"], np.nan) - np.where(np.isfinite(z_ref), z_ref, np.nan)
    share[rows == 0] = np.nan
    return dict(lw_wood_points=wood, lw_leaf_points=rows - wood, lw_components=host["components"].astype(np.int64), lw_wood_share=share,
                lw_wood_top_h=top)


def write_leafwood(path, inv):
    """An .npy of the wood flag of every input row (u8 [N]) of an inventory taken with leafwood=True."""
    if "leafwood" not in inv:
        raise ValueError("the inventory holds no wood flags: take it with leafwood=True")
    with open(path, "wb") as f:
        np.save(f, np.ascontiguousarray(inv["leafwood"]["wood"], np.uint8))
    return path


def add_arguments(ap):
    """One --leafwood-... option per parameter (shared with util.segment, util.inventory, util.branches and util.wood)."""
    for k, v in LEAFWOOD_DEFAULTS.items():
        opt = "--leafwood-" + k.replace("_", "-")
        if opt not in ap._option_string_actions:
            ap.add_argument(opt, type=int if k in _INT + ("filter",) else float, default=int(v) if k == "filter" else v, help=_HELP[k])
    if "--leafwood-scales" not in ap._option_string_actions:
        ap.add_argument("--leafwood-scales", type=float, nargs="+", default=None, metavar="R",
                        help="1 to 4 ascending radii, metres: the seed rule is applied at each of them (the vote keeps --leafwood-radius)")
        ap.add_argument("--leafwood-scales-min", type=int, default=1, metavar="K", help="a row is a seed when the rule holds at K of the scales or more")


def scales_of(a):
    """The two scale options of add_arguments as check_scales takes them."""
    return dict(scales=a.leafwood_scales, scales_min=a.leafwood_scales_min)


def params_of(a):
    p = {k: getattr(a, "leafwood_" + k) for k in LEAFWOOD_DEFAULTS}
    if p["filter"] not in (0, 1):
        raise ValueError(f"--leafwood-filter must be 0 or 1, got {p['filter']!r}")
    p["filter"] = bool(p["filter"])
    return p


def main(argv=None):
    import os
    from . import inventory as _inventory, terrain as _terrain
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.leafwood", description="leaf-wood separation (a wood flag per point) of a labelled cloud")
    ap.add_argument("--forest", required=True, help="labelled cloud: .npy / .npz / .txt / .las, N x 4 (x y z label)")
    ap.add_argument("--out", required=True, help=".npy to write: the wood flag of every row, u8 [N]")
    ap.add_argument("--csv", default=None, help="also write the tree inventory with the leafwood columns as CSV")
    _inventory.add_arguments(ap)
    add_arguments(ap)
    ap.add_argument("--terrain", action="store_true", help="measure heights from the terrain of the label-0 rows (z_ground) instead of z_low")
    _terrain.add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        cfg = check_params(params_of(a))
        sc = check_scales(scales_of(a))
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
    inv = _inventory.cloud_inventory(data, terrain=a.terrain, terrain_cfg=terrain_cfg if a.terrain else None, leafwood=True, leafwood_cfg=cfg,
                                      leafwood_scales=sc["scales"], leafwood_scales_min=sc["scales_min"], **params)
    write_leafwood(a.out, inv)
    if a.csv:
        _inventory.write_inventory(a.csv, inv)
    print(f"{a.forest}: {len(data)} points, {len(inv['tree_id'])} trees, {int(inv['lw_wood_points'].sum())} wood and "
          f"{int(inv['lw_leaf_points'].sum())} leaf rows, {int(inv['lw_components'].sum())} components -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
