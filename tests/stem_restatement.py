"""Stem profiles of a labelled cloud, restated in numpy float64.  The yardstick of tl_stem_keys and tl_stem_profile: it walks
the cloud once per tree and slab, imports nothing from the package and uses plain operators only, one rounding per operation.

Per tree t (label t + 1) of the inventory (inventory_restatement.tree_inventory; terrain_restatement.tree_inventory with a terrain): the
position (px, py), z_top and the reference height z_ref = z_ground with a terrain, z_low without one.  H = z_top - z_ref.
  slabs    h_k = first_height + k * step; S_t = the number of k in 0 .. max_slices - 1 with h_k <= H (0 for a NaN H or an empty tree);
           zc_k = z_ref + h_k, lo_k = zc_k - thickness / 2, hi_k = zc_k + thickness / 2.  S = the largest S_t: the profile width.
  rows     a row of the tree is a candidate when (x - px)^2 + (y - py)^2 < corridor^2; it belongs to the lowest k < S_t with
           lo_k <= z < hi_k (brute force over every k here).
  walk     c = (px, py), R = start_radius, r_prev = NaN, misses = 0; for k = 0 .. S_t - 1: after the walk stopped state 0, n = 0.  Else
           the search set: the slab's candidates with u*u + v*v < R*R, u = x - c.x, v = y - c.y; n = its size.  With n >= min_points the
           Kasa fit of inventory_restatement (the same nine moments, solve3, r2 = (c2 + cx*cx) + cy*cy, failure for r2 <= 0),
           rmse = sqrt(sum((sqrt(du*du + dv*dv) - r)^2) / n).  Accepted (state 1): the fit succeeded, rmse <= max_rmse,
           min_radius <= r <= max_radius, and r_prev is NaN or r <= max_growth * r_prev; then x = cx + c.x, y = cy + c.y, c = (x, y),
           r_prev = r, R = search_factor * r + search_margin, misses = 0.  Else state 2, misses += 1, stop at misses >= max_misses.
  summary  over the accepted slabs in ascending k (m of them): stem_slices = m; stem_base_h, stem_top_h = h of the first / last;
           stem_volume = (PI * (r0 * r0)) * h_first, then V = V + ((PI / 3.0) * (h_j - h_i)) * ((r_i*r_i + r_i*r_j) + r_j*r_j) per
           consecutive accepted pair; dbh_stem = 2.0 * (r_i + (r_j - r_i) * ((dbh_height - h_i) / (h_j - h_i))) for the first pair with
           h_i <= dbh_height <= h_j; stem_lean = atan2(sqrt(dx*dx + dy*dy), h_last - h_first) * (180.0 / PI); stem_taper =
           sum((h - hm)(d - dm)) / sum((h - hm)^2), d = 2.0 * r, hm = sum(h) / m, dm = sum(d) / m, the sums in ascending k.
           NaN for m = 0 (lean, taper: m < 2), dbh_stem NaN when no pair brackets dbh_height.
`offset` is added to the profile's x, y at the end; heights are relative and get none.

Margins.  Every decision that compares floats reports how far the deciding quantity was from its threshold; `margins` holds the smallest
per kind (inf where no such decision was taken).  A float fixture is admissible only when min(margins.values()) > 1e-6: then no
reordering of a sum (about 1e-12 here) can flip a decision.  Kinds: rmse (max_rmse - rmse or rmse - max_rmse); radius (r against
min_radius, max_radius and max_growth * r_prev); search (|u*u + v*v - R*R| over each visited slab's candidates); corridor (|corridor^2 - w|
over the tree's rows near a slab); pivot (|pivot| - its tolerance); r2 (the fitted r^2 against 0); slab (|z - lo_k|, |z - hi_k| of the
corridor rows, and |H - h_k|: these move with z_ref and z_top, exact without a terrain)."""
import numpy as np

import inventory_restatement as inv_ref

PI = 3.141592653589793
STEM_DEFAULTS = dict(first_height=0.5, step=0.5, thickness=0.2, max_slices=128, corridor=1.5, start_radius=0.6, search_factor=1.5,
                     search_margin=0.10, min_points=8, max_rmse=0.03, min_radius=0.02, max_radius=1.0, max_growth=1.25, max_misses=3,
                     dbh_height=1.3)
STEM_COLUMNS = ("stem_slices", "stem_base_h", "stem_top_h", "stem_volume", "dbh_stem", "stem_lean", "stem_taper")
PROFILE_FLOAT = ("h", "x", "y", "r", "rmse")
PROFILE_INT = ("n", "state")
MARGIN_KINDS = ("rmse", "radius", "search", "corridor", "pivot", "r2", "slab")
MIN_MARGIN = 1e-6


def _solve3(A, b, note):
    """inventory_restatement.solve3, reporting each pivot's distance from its tolerance through note("pivot", .)."""
    A = [[float(v) for v in row] for row in A]
    b = [float(v) for v in b]
    tol = inv_ref.PIVOT_TOL * max(abs(v) for row in A for v in row)
    for k in range(3):
        p = k
        for i in range(k + 1, 3):
            if abs(A[i][k]) > abs(A[p][k]):
                p = i
        note("pivot", abs(abs(A[p][k]) - tol))
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


def slab_heights(p):
    """h_k for k = 0 .. max_slices - 1: one multiplication and one addition each."""
    return np.float64(p["first_height"]) + np.arange(int(p["max_slices"]), dtype=np.float64) * np.float64(p["step"])


def stem_profiles(coords, labels, px, py, z_ref, z_top, offset=None, **params):
    """The profiles and summaries of the trees 1 .. T = len(px) from their per-tree inputs.  Returns a dict: STEM_COLUMNS (arrays of
    length T), "stem_profile" (a dict of [T, S] arrays: h, x, y, r, rmse f64 and n, state i64), "S_t" (i64 [T]) and "margins"."""
    p = dict(STEM_DEFAULTS)
    for k, v in params.items():
        if k not in STEM_DEFAULTS:
            raise ValueError(f"unknown stem parameter {k!r}")
        p[k] = v
    xyz = np.asarray(np.asarray(coords)[:, :3], np.float64)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    px, py, z_ref, z_top = (np.asarray(a, np.float64).reshape(-1) for a in (px, py, z_ref, z_top))
    T = len(px)
    margins = {k: np.inf for k in MARGIN_KINDS}

    def note(kind, v):
        v = float(np.min(v)) if np.size(v) else np.inf
        if v < margins[kind]:
            margins[kind] = v

    hk = slab_heights(p)
    half = np.float64(p["thickness"]) / 2
    corridor2 = np.float64(p["corridor"]) * np.float64(p["corridor"])
    H = z_top - z_ref
    with np.errstate(invalid="ignore"):
        S_t = (hk[None, :] <= H[:, None]).sum(1).astype(np.int64) if T else np.zeros(0, np.int64)
    for t in range(T):
        if lab.size == 0 or not (lab == t + 1).any():
            S_t[t] = 0
    S = int(S_t.max()) if T else 0
    prof = {k: np.full((T, S), np.nan) for k in PROFILE_FLOAT}
    prof.update({k: np.zeros((T, S), np.int64) for k in PROFILE_INT})
    out = {k: np.full(T, np.nan) for k in STEM_COLUMNS}
    out["stem_slices"] = np.zeros(T, np.int64)

    for t in range(T):
        St = int(S_t[t])
        if St == 0:
            continue
        note("slab", np.abs(H[t] - hk))
        rows = xyz[lab == t + 1]
        x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
        prof["h"][t, :St] = hk[:St]
        zc = z_ref[t] + hk[:St]
        lo, hi = zc - half, zc + half
        # the slab of every row: the lowest k with lo_k <= z < hi_k, by brute force
        inside = (z[:, None] >= lo[None, :]) & (z[:, None] < hi[None, :])
        slab = np.where(inside.any(1), inside.argmax(1), -1)
        w0 = (x - px[t]) * (x - px[t]) + (y - py[t]) * (y - py[t])
        cand = w0 < corridor2
        near = np.minimum(np.abs(z[:, None] - lo[None, :]), np.abs(z[:, None] - hi[None, :])).min(1) if len(z) else np.zeros(0)
        note("corridor", np.abs(corridor2 - w0)[(slab >= 0) | (near <= MIN_MARGIN)])
        note("slab", near[cand | (np.abs(corridor2 - w0) <= MIN_MARGIN)])

        c = (px[t], py[t])
        R, r_prev, misses, stopped = np.float64(p["start_radius"]), np.nan, 0, False
        acc = []                                                           # (k, h, x, y, r) of the accepted slabs
        for k in range(St):
            if stopped:
                continue                                                   # state 0, n = 0, NaN
            m = cand & (slab == k)
            u, v = x[m] - c[0], y[m] - c[1]
            w = u * u + v * v
            note("search", np.abs(w - R * R))
            s = w < R * R
            n = int(s.sum())
            prof["n"][t, k] = n
            ok = False
            if n >= int(p["min_points"]):
                u, v, w = u[s], v[s], w[s]
                sol = _solve3([[(u * u).sum(), (u * v).sum(), u.sum()], [(u * v).sum(), (v * v).sum(), v.sum()], [u.sum(), v.sum(), np.float64(n)]],
                              [(u * w).sum(), (v * w).sum(), w.sum()], note)
                if sol is not None:
                    cx, cy = sol[0] / 2, sol[1] / 2
                    rr = (sol[2] + cx * cx) + cy * cy
                    note("r2", abs(rr))
                    if rr > 0:
                        r = np.sqrt(rr)
                        du, dv = u - cx, v - cy
                        e = np.sqrt(du * du + dv * dv) - r
                        rmse = np.sqrt((e * e).sum() / np.float64(n))
                        note("rmse", abs(rmse - np.float64(p["max_rmse"])))
                        note("radius", min(abs(r - np.float64(p["min_radius"])), abs(np.float64(p["max_radius"]) - r)))
                        if not np.isnan(r_prev):
                            note("radius", abs(np.float64(p["max_growth"]) * r_prev - r))
                        ok = bool(rmse <= p["max_rmse"] and p["min_radius"] <= r <= p["max_radius"]
                                  and (np.isnan(r_prev) or r <= np.float64(p["max_growth"]) * r_prev))
            if ok:
                xa, ya = cx + c[0], cy + c[1]
                prof["state"][t, k] = 1
                prof["x"][t, k], prof["y"][t, k], prof["r"][t, k], prof["rmse"][t, k] = xa, ya, r, rmse
                acc.append((k, hk[k], xa, ya, r))
                c, r_prev, misses = (xa, ya), r, 0
                R = np.float64(p["search_factor"]) * r + np.float64(p["search_margin"])
            else:
                prof["state"][t, k] = 2
                misses += 1
                stopped = misses >= int(p["max_misses"])

        m = len(acc)
        out["stem_slices"][t] = m
        if m == 0:
            continue
        hs, rs = [a[1] for a in acc], [a[4] for a in acc]
        out["stem_base_h"][t], out["stem_top_h"][t] = hs[0], hs[-1]
        V = (PI * (rs[0] * rs[0])) * hs[0]
        dbh, dh = np.nan, np.float64(p["dbh_height"])
        for i in range(m - 1):
            hi_, hj, ri, rj = hs[i], hs[i + 1], rs[i], rs[i + 1]
            V = V + ((PI / 3.0) * (hj - hi_)) * ((ri * ri + ri * rj) + rj * rj)
            if np.isnan(dbh) and hi_ <= dh <= hj:
                dbh = 2.0 * (ri + (rj - ri) * ((dh - hi_) / (hj - hi_)))
        out["stem_volume"][t], out["dbh_stem"][t] = V, dbh
        if m < 2:
            continue
        dx, dy = acc[-1][2] - acc[0][2], acc[-1][3] - acc[0][3]
        out["stem_lean"][t] = np.arctan2(np.sqrt(dx * dx + dy * dy), hs[-1] - hs[0]) * (180.0 / PI)
        sh = sd = np.float64(0.0)
        for h, r in zip(hs, rs):
            sh, sd = sh + h, sd + 2.0 * r
        hm, dm = sh / np.float64(m), sd / np.float64(m)
        num = den = np.float64(0.0)
        for h, r in zip(hs, rs):
            eh, ed = h - hm, 2.0 * r - dm
            num, den = num + eh * ed, den + eh * eh
        out["stem_taper"][t] = num / den

    if offset is not None:
        o = np.asarray(offset, np.float64).reshape(3)
        prof["x"], prof["y"] = prof["x"] + o[0], prof["y"] + o[1]
    out["stem_profile"] = prof
    out["S_t"] = S_t
    out["margins"] = margins
    return out


def tree_stems(coords, labels, terrain=None, offset=None, stem_cfg=None, **inventory_params):
    """The inventory of the restatements (the sixteen columns, and the eight ground columns with a terrain: a terrain_restatement.terrain_model
    dict in the frame of coords) followed by STEM_COLUMNS, "stem_profile", "S_t" and "margins"."""
    if terrain is None:
        base = inv_ref.tree_inventory(coords, labels, **inventory_params)     # the frame of coords: no offset yet
        z_ref = base["z_low"]
        full = base if offset is None else inv_ref.tree_inventory(coords, labels, offset=offset, **inventory_params)
    else:
        import terrain_restatement as ter_ref
        base = ter_ref.tree_inventory(coords, labels, terrain, **inventory_params)
        z_ref = base["z_ground"]
        full = base if offset is None else ter_ref.tree_inventory(coords, labels, terrain, offset=offset, **inventory_params)
    st = stem_profiles(coords, labels, base["x"], base["y"], z_ref, base["z_top"], offset=offset, **(stem_cfg or {}))
    if terrain is None:
        st["margins"]["slab"] = np.inf       # z_low and z_top are ranks of the rows' own z: the slab bounds are the same bits everywhere
    res = dict(full)
    res.update(st)
    return res
