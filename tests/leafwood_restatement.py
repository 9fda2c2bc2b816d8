"""Leaf-wood separation of a labelled cloud, restated in numpy float64.  The yardstick of csrc/tl_leafwood.hip and
util/leafwood.py: scipy's cKDTree for the pairs within the radius, bincounts for the vote, a flood fill over a dict of voxels for the
components.  It imports nothing from the package.

All rules are per gathered row: a row with label >= 1, in label order (a stable sort of the labels).
  1 features   linearity, planarity, verticality, number_of_neighbors of features_restatement.restate at `radius`, over all gathered rows
               (features=None), or the [N, 4] array handed in (rows of the input, in the input's order; rows of a label < 1 are not read).
  2 seed       s0 = 1 when number_of_neighbors >= min_neighbours, the three features are finite and (linearity >= linearity_min, or planarity
               >= planarity_min and verticality >= verticality_min); compared in f64; NaN gives 0.
  3 vote       vote_iters synchronous rounds: a = the rows of the same tree with dx dx + dy dy + dz dz <= radius radius (the row itself
               included), w = those flagged in the round before; the new flag is 1 exactly when 100 w >= vote_percent a, in integers.
  4 components every gathered row's voxel key as branches_restatement packs it (ValueError for a coordinate that is not finite or a row
               beyond the key's range), -1 below z_ref and for a tree without a finite position; the voted rows' distinct keys are the wood
               voxels; components under max(|dx|, |dy|, |dz|) <= reach inside a tree; a component of fewer than min_component voxels is
               dropped (its rows get 0); rows with key -1 keep their voted flag.
  5 outputs    wood u8 [N] in the input order (0 for a label < 1); lw_wood_points, lw_leaf_points, lw_components (kept), lw_wood_share =
               wood / (wood + leaf) (NaN for an empty tree), lw_wood_top_h = the largest z of a wood row - z_ref (NaN without one or
               without a finite z_ref).
  6 filter     "rows": the positions (in the input) of the rows the branch and wood stages read: the wood rows in label order with
               `filter`, every gathered row without.

`margins`: radius = min | |d| - r | / r over the pairs of gathered rows with |d| < 1.02 r; voxel = the smallest distance, in voxels, of
a gathered row's coordinate / voxel from an integer; anchor = the same for px, py and z_ref of the trees with rows.  A cloud is
admissible for a comparison with the device when radius > 1e-10 and voxel, anchor > 1e-6."""
import numpy as np
from scipy.spatial import cKDTree

LEAFWOOD_DEFAULTS = dict(radius=0.2, min_neighbours=5, linearity_min=0.6, planarity_min=0.3, verticality_min=0.2, vote_iters=2, vote_percent=50,
                         voxel=0.1, reach=1, min_component=20, filter=True)
LEAFWOOD_COLUMNS = ("lw_wood_points", "lw_leaf_points", "lw_components", "lw_wood_share", "lw_wood_top_h")
LEAFWOOD_INT = ("lw_wood_points", "lw_leaf_points", "lw_components")
FEATURES = ("linearity", "planarity", "verticality", "number_of_neighbors")
MIN_RADIUS_MARGIN, MIN_FLOOR_MARGIN = 1e-10, 1e-6
HALF, Z_MAX = 2048, 2047


def seed(feats, p):
    """Rule 2 on [n, 4] features (FEATURES), any float dtype -> u8 [n]."""
    f = np.asarray(feats).astype(np.float64)
    lin, pla, ver, nn = f[:, 0], f[:, 1], f[:, 2], f[:, 3]
    with np.errstate(invalid="ignore"):
        ok = (nn >= np.float64(p["min_neighbours"])) & np.isfinite(lin) & np.isfinite(pla) & np.isfinite(ver)
        ok &= (lin >= np.float64(p["linearity_min"])) | ((pla >= np.float64(p["planarity_min"])) & (ver >= np.float64(p["verticality_min"])))
    return ok.astype(np.uint8)


def pairs_within(xyz, radius):
    """The pairs i < j of rows with dx dx + dy dy + dz dz <= radius radius, decided by this f64 expression."""
    r = np.float64(radius)
    cand = cKDTree(xyz).query_pairs(float(r) * (1.0 + 1e-9) + 1e-300, output_type="ndarray")
    if len(cand) == 0:
        return np.zeros((0, 2), np.int64)
    d = xyz[cand[:, 0]] - xyz[cand[:, 1]]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return cand[dx * dx + dy * dy + dz * dz <= r * r].astype(np.int64)


def vote(xyz, tree, flag, p):
    """Rule 3 on rows xyz f64 [n, 3] of the trees tree i64 [n] with the flags flag u8 [n] -> u8 [n]."""
    xyz, tree = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(tree, np.int64).reshape(-1)
    flag = np.asarray(flag).astype(np.int64).reshape(-1)
    n = len(xyz)
    if n == 0 or p["vote_iters"] == 0:
        return flag.astype(np.uint8)
    pr = pairs_within(xyz, p["radius"])
    pr = pr[tree[pr[:, 0]] == tree[pr[:, 1]]]
    i, j = pr[:, 0], pr[:, 1]
    a = 1 + np.bincount(i, minlength=n) + np.bincount(j, minlength=n)
    for _ in range(p["vote_iters"]):
        w = flag + np.bincount(i, weights=flag[j], minlength=n).astype(np.int64) + np.bincount(j, weights=flag[i], minlength=n).astype(np.int64)
        flag = (100 * w >= int(p["vote_percent"]) * a).astype(np.int64)
    return flag.astype(np.uint8)


def voxel_keys(xyz, lab, tree, voxel):
    """Every row's key (branches_restatement's packing), -1 below z_ref and for a tree without a finite anchor; and the floor margins."""
    vs = np.float64(voxel)
    keys = np.full(len(xyz), -1, np.int64)
    margins = dict(voxel=np.inf, anchor=np.inf)
    if len(xyz):
        q = xyz / vs
        margins["voxel"] = float(np.minimum(q - np.floor(q), np.floor(q) + 1.0 - q).min()) if np.isfinite(xyz).all() else 0.0
    for t in range(len(tree)):
        sel = np.flatnonzero(lab == t + 1)
        if len(sel) == 0:
            continue
        rows = xyz[sel]
        if not np.isfinite(rows).all():
            raise ValueError("a coordinate of a tree is not finite")
        anchor = tree[t, :3]
        if not np.isfinite(anchor).all():
            continue
        q = anchor / vs
        base = np.floor(q)
        margins["anchor"] = min(margins["anchor"], float(np.minimum(q - base, base + 1.0 - q).min()))
        ipx, ipy, izr = (int(v) for v in base)
        idx = np.floor(rows / vs).astype(np.int64)
        above = idx[:, 2] >= izr
        far = above & ((np.abs(idx[:, 0] - ipx) > 2047) | (np.abs(idx[:, 1] - ipy) > 2047) | (idx[:, 2] - izr >= Z_MAX))
        if far.any():
            raise ValueError("a row lies beyond the voxel key of its tree")
        k = (t << 35) | ((idx[:, 0] - ipx + HALF) << 23) | ((idx[:, 1] - ipy + HALF) << 11) | (idx[:, 2] - izr)
        keys[sel] = np.where(above, k, -1)
    return keys, margins


def components(vkeys, reach):
    """The distinct keys vkeys (any order) -> {key: component id}, {component id: voxels}; edges join keys of one tree with max(|dx|, |dy|,
    |dz|) <= reach."""
    def cell(k):
        return (k >> 35, (k >> 23) & 4095, (k >> 11) & 4095, k & 2047)
    cells = {cell(int(k)): int(k) for k in vkeys}
    comp, sizes = {}, {}
    steps = [(dx, dy, dz) for dx in range(-reach, reach + 1) for dy in range(-reach, reach + 1) for dz in range(-reach, reach + 1) if (dx, dy, dz) != (0, 0, 0)]
    for c0 in sorted(cells):
        if cells[c0] in comp:
            continue
        cid = len(sizes)
        comp[cells[c0]] = cid
        stack, count = [c0], 0
        while stack:
            t, x, y, z = stack.pop()
            count += 1
            for dx, dy, dz in steps:
                c = (t, x + dx, y + dy, z + dz)
                k = cells.get(c)
                if k is not None and k not in comp:
                    comp[k] = cid
                    stack.append(c)
        sizes[cid] = count
    return comp, sizes


def leafwood(xyz, labels, tree, p, features=None):
    """xyz f64 [N, 3], labels i64 [N], tree f64 [T, 4] (px, py, z_ref, z_top; T >= max(label)), p: the eleven parameters.  Returns wood, seed,
    voted u8 [N], LEAFWOOD_COLUMNS ([T] each), rows i64 (rule 6) and margins."""
    unknown = set(p) - set(LEAFWOOD_DEFAULTS)
    assert not unknown, unknown
    p = dict(LEAFWOOD_DEFAULTS, **p)
    xyz, lab = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(labels, np.int64).reshape(-1)
    tree = np.asarray(tree, np.float64).reshape(-1, 4)
    N, T = len(xyz), len(tree)
    order = np.argsort(lab, kind="stable")
    kept = order[lab[order] >= 1]
    g, glab = xyz[kept], lab[kept]
    assert len(glab) == 0 or glab.max() <= T
    if features is None:
        import features_restatement as feat_ref
        res = feat_ref.restate(g, p["radius"])
        f = res["features"][:, [feat_ref.COL[k] for k in FEATURES]] if len(g) else np.zeros((0, 4))
        radius_margin = res["margin"] if len(g) else 1.0
    else:
        import features_restatement as feat_ref
        f = np.asarray(features)[kept]
        radius_margin = feat_ref.radius_margin(g, p["radius"]) if len(g) else 1.0
    s0 = seed(f, p)
    voted = vote(g, glab, s0, p)
    keys, margins = voxel_keys(g, glab, tree, p["voxel"])
    margins["radius"] = radius_margin
    wkeys = np.where(voted != 0, keys, -1)
    comp, sizes = components(np.unique(wkeys[wkeys >= 0]), int(p["reach"]))
    wood = voted.copy()
    for r in np.flatnonzero(wkeys >= 0):
        if sizes[comp[int(wkeys[r])]] < p["min_component"]:
            wood[r] = 0
    col = {k: (np.zeros(T, np.int64) if k in LEAFWOOD_INT else np.full(T, np.nan)) for k in LEAFWOOD_COLUMNS}
    kept_comp = {}
    for k, cid in comp.items():
        if sizes[cid] >= p["min_component"]:
            kept_comp.setdefault(k >> 35, set()).add(cid)
    for t in range(T):
        sel = glab == t + 1
        n, nw = int(sel.sum()), int(wood[sel].sum())
        col["lw_wood_points"][t], col["lw_leaf_points"][t], col["lw_components"][t] = nw, n - nw, len(kept_comp.get(t, ()))
        if n:
            col["lw_wood_share"][t] = np.float64(nw) / np.float64(n)
        if nw and np.isfinite(tree[t, 2]):
            col["lw_wood_top_h"][t] = g[sel][wood[sel] != 0, 2].max() - tree[t, 2]
    out = dict(col)
    for name, v in (("wood", wood), ("seed", s0), ("voted", voted)):
        full = np.zeros(N, np.uint8)
        full[kept] = v
        out[name] = full
    out["rows"] = kept[wood != 0] if p["filter"] else kept
    out["margins"] = margins
    return out
