"""Leaf-wood separation with a seed over several scales, restated in numpy float64.  The yardstick of tl_leafwood_seed_scales
and of util.leafwood.leafwood_stage(..., scales=...).  Rules 3 to 6 (vote, keys, components, outputs, filter) are those of
leafwood_restatement and are imported from it; only rule 2 changes:

  2' seed      at every scale k the rule 2 of leafwood_restatement on that scale's four features (a scale whose number_of_neighbors is below
               min_neighbours, or with a feature that is not finite, does not hold); s0 = 1 exactly when at least scales_min scales hold.

The features: features_restatement.restate at every radius of `scales` over all gathered rows (features=None), or the [N, S, 4] array
handed in.  The vote keeps p["radius"].  It imports nothing from the package."""
import numpy as np

from leafwood_restatement import FEATURES, LEAFWOOD_COLUMNS, LEAFWOOD_DEFAULTS, LEAFWOOD_INT, components, seed, vote, voxel_keys

LEAFWOOD_SCALE_DEFAULTS = dict(scales=None, scales_min=1)


def seed_scales(feats, p, scales_min):
    """Rule 2' on [n, S, 4] features -> u8 [n]; and the number of scales that hold, i64 [n]."""
    f = np.asarray(feats)
    assert f.ndim == 3 and f.shape[2] == 4 and 1 <= int(scales_min) <= f.shape[1]
    hold = np.zeros(len(f), np.int64)
    for k in range(f.shape[1]):
        hold += seed(f[:, k, :], p).astype(np.int64)
    return (hold >= int(scales_min)).astype(np.uint8), hold


def restate_features(g, scales):
    """f64 [n, S, 4] (FEATURES) of the rows g at every radius of scales, and the smallest radius margin."""
    import features_restatement as feat_ref
    out, margin = np.zeros((len(g), len(scales), 4)), 1.0
    for k, r in enumerate(scales):
        res = feat_ref.restate(g, r)
        out[:, k, :] = res["features"][:, [feat_ref.COL[c] for c in FEATURES]]
        margin = min(margin, res["margin"])
    return out, margin


def leafwood_scales(xyz, labels, tree, p, scales, scales_min=1, features=None, margin=None):
    """leafwood_restatement.leafwood with the seed over `scales` (1..4 ascending radii).  features: None or [N, S, 4] in the input's order.
    margins["radius"]: over the radii at which this function decides a neighbourhood -- the vote's p["radius"], and the scales when it
    computes the features itself; `margin` hands it in where the caller has it already (it is costly).
    Returns what leafwood returns, and `hold` i64 [N] (the scales that hold per row, 0 for a label < 1)."""
    import features_restatement as feat_ref
    unknown = set(p) - set(LEAFWOOD_DEFAULTS)
    assert not unknown, unknown
    scales = [float(r) for r in scales]
    assert 1 <= len(scales) <= 4 and all(r > 0 and np.isfinite(r) for r in scales) and all(b > a for a, b in zip(scales, scales[1:]))
    p = dict(LEAFWOOD_DEFAULTS, **p)
    xyz, lab = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(labels, np.int64).reshape(-1)
    tree = np.asarray(tree, np.float64).reshape(-1, 4)
    N, T = len(xyz), len(tree)
    order = np.argsort(lab, kind="stable")
    kept = order[lab[order] >= 1]
    g, glab = xyz[kept], lab[kept]
    assert len(glab) == 0 or glab.max() <= T
    if features is None:
        f, radius_margin = restate_features(g, scales) if len(g) else (np.zeros((0, len(scales), 4)), 1.0)
    else:
        f = np.asarray(features)[kept]
        radius_margin = 1.0                                                # (no neighbourhood is decided here at the scales: only the vote's)
    if margin is not None:
        radius_margin = float(margin)
    elif len(g) and not (features is None and p["radius"] in scales):
        radius_margin = min(radius_margin, feat_ref.radius_margin(g, p["radius"]))
    s0, hold = seed_scales(f, p, scales_min)
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
    for name, v, dt in (("wood", wood, np.uint8), ("seed", s0, np.uint8), ("voted", voted, np.uint8), ("hold", hold, np.int64)):
        full = np.zeros(N, dt)
        full[kept] = v
        out[name] = full
    out["rows"] = kept[wood != 0] if p["filter"] else kept
    out["margins"] = margins
    return out
