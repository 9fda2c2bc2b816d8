"""Cylinder model of a labelled cloud, restated in plain Python and numpy float64 on top of tests/branches_restatement.py.  The
yardstick of csrc/tl_wood.hip and util/wood.py.  It imports nothing from the package.  The voxel -> node map is the one
branches_restatement.nodes_of builds: branch_structure is run with that function wrapped, so that its node lists can be read.

Per tree with a skeleton (node table: centroids c, local parents, orders, branch ids from branches_restatement):
  rows      a row of the tree belongs to node i when its voxel floor(coordinate / voxel) is a reached voxel of node i; else to no node.
  axis      a = (c_i - c_parent) / seg with seg = sqrt(dx dx + dy dy + dz dz) > 0; a root, or seg == 0: (0, 0, 1).
  basis     k = the index of the smallest |a_k| (the first among equals); w = a x e_k, e1 = w / |w|, e2 = a x e1, the cross products
            written out component by component (cross() below: the same expressions as the kernel's).
  fit       q = p - c_i, u = q . e1, v = q . e2 (added left to right).  n >= min_points: the Kasa circle by Gaussian elimination with partial
            pivoting (inventory_restatement's rule), rmse = sqrt(rss / n).  state 0 / 1 / 2 = too few rows / accepted / rejected; accepted:
            solved, min_radius <= r <= max_radius, rmse <= max_rmse, sqrt(cu^2 + cv^2) <= r.  radius_fit, rmse, centre = c_i + cu e1 + cv e2
            are NaN unless state is 1.
  radii     in node order: a root takes its radius_fit, else the first finite radius_fit along its own branch, else NaN.  With a parent:
            cap = max_growth * radius[parent]; cap NaN: radius_fit; radius_fit finite: min(radius_fit, cap); else cap.
  segments  a node with a parent and both radii finite: length seg, volume pi seg / 3 (R^2 + R r + r^2), lateral area pi (R + r)
            sqrt(seg^2 + (R - r)^2).
  columns   WOOD_COLUMNS as util/wood.py's docstring states them; the sums here are math.fsum, the host side adds in node order.
`offset` is added to the skeleton's xyz and the cylinders' centre at the end.

Margins.  `margins` holds, next to the kinds of branches_restatement, the smallest distance of every float decision taken here from its
threshold (inf where none was taken): n (|n - (min_points - 1/2)|, never below 1/2: the counts are exact), radius (r against min_radius
and max_radius), rmse (against max_rmse), shift (sqrt(cu^2 + cv^2) against r), pivot (each pivot of the solve against its tolerance), r2
(the squared radius against 0), cap (radius_fit against max_growth * radius[parent]; not where the two are the same number), dbh (the heights of the axis pairs with two finite
radii against dbh_height), seg (seg against 0 for a node with a parent; an exact 0 is not counted).  A fixture is admissible only when
min(margins.values()) > 1e-6.
The choice of k is reported apart, as "basis_lead" (the smallest lead of the second smallest |a_k| over the smallest, exact ties left
out), and is no condition of admissibility: centroids on a voxel lattice make near-ties the rule (a chord with dx = dy in exact
arithmetic, apart by one rounding), both sides take the choice from the same bits (the centroids are pinned, division and square root
are correctly rounded), and another k only turns (e1, e2) within the plane, which leaves r, rmse, the centre and the axis where they
are up to rounding -- unlike every kind above, it cannot move a result across a threshold."""
import math

import numpy as np

import branches_restatement as ref
import inventory_restatement as inv_ref

PI = math.pi
WOOD_DEFAULTS = dict(min_points=8, max_rmse=0.03, min_radius=0.005, max_radius=1.0, max_growth=1.0, dbh_height=1.3)
WOOD_COLUMNS = ("wood_nodes_fit", "wood_length", "wood_volume", "wood_area", "axis_volume", "branch_volume", "branch_volume_1", "axis_dbh",
                "branch_base_diam_1")
WOOD_INT = ("wood_nodes_fit",)
CYLINDER_KEYS = ("node_start", "radius_fit", "radius", "n", "rmse", "state", "centre", "axis", "length", "volume")
MARGIN_KINDS = ("n", "radius", "rmse", "shift", "pivot", "r2", "cap", "dbh", "seg")
MIN_MARGIN = 1e-6


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def solve3(A, b, note):
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


def axis_of(c, cp, note):
    """(axis, seg) of a node at c with its parent at cp (None for a root)."""
    if cp is None:
        return (0.0, 0.0, 1.0), 0.0
    dx, dy, dz = (np.float64(c[k]) - np.float64(cp[k]) for k in range(3))
    seg = np.sqrt(dx * dx + dy * dy + dz * dz)
    if seg != 0:                                                  # (an exact 0 is the same 0 everywhere: the centroids are pinned)
        note("seg", abs(float(seg)))
    if seg > 0:
        return (float(dx / seg), float(dy / seg), float(dz / seg)), float(seg)
    return (0.0, 0.0, 1.0), float(seg)


def basis_of(a, note):
    mags = [abs(v) for v in a]
    k = mags.index(min(mags))
    rest = sorted(mags)
    if rest[1] != rest[0]:
        note("basis_lead", rest[1] - rest[0])
    ek = tuple(1.0 if j == k else 0.0 for j in range(3))
    w = tuple(np.float64(v) for v in cross(tuple(np.float64(v) for v in a), ek))
    wn = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    e1 = tuple(v / wn for v in w)
    e2 = cross(tuple(np.float64(v) for v in a), e1)
    return e1, e2


def fit_node(rows, c, a, p, note):
    """The fit of one node: rows f64 [n, 3], centroid c, axis a.  Returns dict(radius_fit, n, rmse, state, centre)."""
    nan = float("nan")
    e1, e2 = basis_of(a, note)
    n = len(rows)
    res = dict(radius_fit=nan, n=n, rmse=nan, state=0, centre=(nan, nan, nan))
    note("n", abs(n - (p["min_points"] - 0.5)))
    if n < p["min_points"]:
        return res
    res["state"] = 2
    qx, qy, qz = rows[:, 0] - c[0], rows[:, 1] - c[1], rows[:, 2] - c[2]
    u = qx * e1[0] + qy * e1[1] + qz * e1[2]
    v = qx * e2[0] + qy * e2[1] + qz * e2[2]
    w = u * u + v * v
    sol = solve3([[(u * u).sum(), (u * v).sum(), u.sum()], [(u * v).sum(), (v * v).sum(), v.sum()], [u.sum(), v.sum(), np.float64(n)]],
                 [(u * w).sum(), (v * w).sum(), w.sum()], note)
    if sol is None:
        return res
    cu, cv = sol[0] / 2.0, sol[1] / 2.0
    rr = (sol[2] + cu * cu) + cv * cv
    note("r2", abs(rr))
    if not rr > 0:
        return res
    r = math.sqrt(rr)
    du, dv = u - cu, v - cv
    e = np.sqrt(du * du + dv * dv) - r
    rmse = math.sqrt((e * e).sum() / np.float64(n))
    shift = math.sqrt(cu * cu + cv * cv)
    note("rmse", abs(rmse - p["max_rmse"]))
    note("radius", min(abs(r - p["min_radius"]), abs(p["max_radius"] - r)))
    note("shift", abs(shift - r))
    if p["min_radius"] <= r <= p["max_radius"] and rmse <= p["max_rmse"] and shift <= r:
        res.update(radius_fit=r, rmse=rmse, state=1, centre=tuple(float((c[k] + cu * e1[k]) + cv * e2[k]) for k in range(3)))
    return res


def radii_of(parent, branch, radius_fit, max_growth, note):
    n = len(parent)
    radius = [float("nan")] * n
    for i in range(n):
        q, rf = parent[i], radius_fit[i]
        if q < 0:
            chain = [radius_fit[j] for j in range(n) if branch[j] == branch[i] and not math.isnan(radius_fit[j])]
            radius[i] = rf if not math.isnan(rf) else (chain[0] if chain else float("nan"))
            continue
        cap = max_growth * radius[q]
        if math.isnan(cap):
            radius[i] = rf
        elif not math.isnan(rf):
            if rf != cap:                                         # (an exact tie: the cap is this very fit, handed down from an unfitted root at max_growth 1)
                note("cap", abs(rf - cap))
            radius[i] = min(rf, cap)
        else:
            radius[i] = cap
    return radius


def wood_of(xyz, parent, order, branch, radius_fit, z_ref, p, min_branch, note):
    """Steps 5-7 on one tree's node table.  Returns (columns of the tree, radius, length, volume per node)."""
    n = len(parent)
    seg = [0.0] * n
    for i, q in enumerate(parent):
        if q >= 0:
            dx, dy, dz = (float(xyz[i][k]) - float(xyz[q][k]) for k in range(3))
            seg[i] = math.sqrt(dx * dx + dy * dy + dz * dz)
    radius = radii_of(parent, branch, radius_fit, p["max_growth"], note)
    nb = max(branch) + 1
    b_nodes = [[i for i in range(n) if branch[i] == k] for k in range(nb)]
    b_len = [math.fsum(seg[i] for i in nodes) for nodes in b_nodes]
    b_order = [order[nodes[0]] for nodes in b_nodes]
    counted = [b_order[k] >= 1 and b_len[k] >= min_branch for k in range(nb)]
    kids = [[j for j in range(n) if parent[j] == i] for i in range(n)]
    down = [0.0] * n
    for i in range(n - 1, -1, -1):
        if kids[i]:
            down[i] = max(seg[j] + down[j] for j in kids[i])
    roots = [i for i in range(n) if parent[i] < 0]
    top = max(down[i] for i in roots)
    axis = branch[min(i for i in roots if down[i] == top)]
    modelled = [i for i in range(n) if parent[i] >= 0 and not math.isnan(radius[i]) and not math.isnan(radius[parent[i]])]
    vol, area = {}, {}
    for i in modelled:
        R, r, L = radius[parent[i]], radius[i], seg[i]
        vol[i] = PI * L / 3.0 * (R * R + R * r + r * r)
        area[i] = PI * (R + r) * math.sqrt(L * L + (R - r) * (R - r))
    dbh = float("nan")
    for i in modelled:
        q = parent[i]
        if branch[i] == axis and branch[q] == axis:
            hq, hi = float(xyz[q][2]) - z_ref, float(xyz[i][2]) - z_ref
            note("dbh", min(abs(hq - p["dbh_height"]), abs(hi - p["dbh_height"])))
            if math.isnan(dbh) and hq <= p["dbh_height"] < hi:
                dbh = 2.0 * (radius[q] + (radius[i] - radius[q]) * ((p["dbh_height"] - hq) / (hi - hq)))
    base = [2.0 * radius[b_nodes[k][0]] for k in range(nb) if counted[k] and b_order[k] == 1 and not math.isnan(radius[b_nodes[k][0]])]
    col = dict(wood_nodes_fit=sum(1 for i in range(n) if radius[i] == radius_fit[i]), wood_length=math.fsum(seg[i] for i in modelled),
               wood_volume=math.fsum(vol.values()), wood_area=math.fsum(area.values()),
               axis_volume=math.fsum(vol[i] for i in modelled if branch[i] == axis),
               branch_volume=math.fsum(vol[i] for i in modelled if counted[branch[i]]),
               branch_volume_1=math.fsum(vol[i] for i in modelled if counted[branch[i]] and b_order[branch[i]] == 1), axis_dbh=dbh,
               branch_base_diam_1=math.fsum(base) / len(base) if base else float("nan"))
    return col, radius, [seg[i] if i in vol else 0.0 for i in range(n)], [vol.get(i, 0.0) for i in range(n)]


def wood_structure(xyz, lab, px, py, z_ref, offset=None, branch_cfg=None, wood_cfg=None):
    """xyz f64 [N, 3], lab i64 [N], px, py, z_ref f64 [T].  Returns what branches_restatement.branch_structure returns, and WOOD_COLUMNS ([T]
    each), "cylinders" (CYLINDER_KEYS), "row_node" i32 [N] (the global node of every row in the order given, -1 for none), "margins"
    (both modules' kinds) and "basis_lead"."""
    unknown = set(wood_cfg or {}) - set(WOOD_DEFAULTS)
    assert not unknown, unknown
    p = dict(WOOD_DEFAULTS, **(wood_cfg or {}))
    bcfg = dict(ref.BRANCH_DEFAULTS, **(branch_cfg or {}))
    xyz, lab = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(lab, np.int64).reshape(-1)
    captured, nodes_of = [], ref.nodes_of

    def spy(d, cfg):
        captured.append(nodes_of(d, cfg))
        return captured[-1]
    ref.nodes_of = spy
    try:
        out = ref.branch_structure(xyz, lab, px, py, z_ref, **(branch_cfg or {}))
    finally:
        ref.nodes_of = nodes_of
    sk = out["skeleton"]
    T, M, vs = len(px), len(sk["parent"]), np.float64(bcfg["voxel"])
    margins = dict(out["margins"], **{k: np.inf for k in MARGIN_KINDS})
    apart = dict(basis_lead=np.inf)

    def note(kind, value):
        book = apart if kind in apart else margins
        book[kind] = min(book[kind], float(value))

    out.update({k: (np.zeros(T, np.int64) if k in WOOD_INT else np.full(T, np.nan)) for k in WOOD_COLUMNS})
    cyl = dict(node_start=sk["node_start"], radius_fit=np.full(M, np.nan), radius=np.full(M, np.nan), n=np.zeros(M, np.int64), rmse=np.full(M, np.nan),
               state=np.zeros(M, np.int32), centre=np.full((M, 3), np.nan), axis=np.zeros((M, 3)), length=np.zeros(M), volume=np.zeros(M))
    row_node = np.full(len(xyz), -1, np.int32)
    with_nodes = [t for t in range(T) if sk["node_start"][t + 1] > sk["node_start"][t]]
    assert len(with_nodes) == len(captured)
    for t, nodes in zip(with_nodes, captured):
        a0, b0 = int(sk["node_start"][t]), int(sk["node_start"][t + 1])
        assert b0 - a0 == len(nodes)
        owner = {v: i for i, nd in enumerate(nodes) for v in nd["voxels"]}
        at = np.flatnonzero(lab == t + 1)
        izr = int(np.floor(np.float64(z_ref[t]) / vs))
        idx = np.floor(xyz[at] / vs).astype(np.int64)
        local = np.array([owner.get(tuple(v), -1) if v[2] >= izr else -1 for v in idx.tolist()], np.int64).reshape(-1)
        row_node[at[local >= 0]] = (a0 + local[local >= 0]).astype(np.int32)
        c, parent = sk["xyz"][a0:b0], sk["parent"][a0:b0].tolist()
        for i in range(b0 - a0):
            a, _ = axis_of(c[i], c[parent[i]] if parent[i] >= 0 else None, note)
            f = fit_node(xyz[at[local == i]], c[i], a, p, note)
            g = a0 + i
            cyl["radius_fit"][g], cyl["n"][g], cyl["rmse"][g], cyl["state"][g], cyl["centre"][g], cyl["axis"][g] = \
                f["radius_fit"], f["n"], f["rmse"], f["state"], f["centre"], a
        col, radius, length, volume = wood_of(c, parent, sk["order"][a0:b0].tolist(), sk["branch"][a0:b0].tolist(),
                                              cyl["radius_fit"][a0:b0].tolist(), float(z_ref[t]), p, bcfg["min_branch"], note)
        for k, v in col.items():
            out[k][t] = v
        cyl["radius"][a0:b0], cyl["length"][a0:b0], cyl["volume"][a0:b0] = radius, length, volume
    if offset is not None:
        off = np.asarray(offset, np.float64).reshape(1, 3)
        out["skeleton"] = dict(sk, xyz=sk["xyz"] + off)
        cyl["centre"] = cyl["centre"] + off
    out["cylinders"] = {k: cyl[k] for k in CYLINDER_KEYS}
    out["row_node"], out["margins"], out["basis_lead"] = row_node, margins, apart["basis_lead"]
    return out


def tree_wood(coords, labels, terrain=None, offset=None, branch_cfg=None, wood_cfg=None, **inventory_params):
    """The inventory of the restatements (with the ground columns with a terrain) followed by the branch and wood results of
    wood_structure; z_ref = z_ground with a terrain, z_low without."""
    if terrain is None:
        base = inv_ref.tree_inventory(coords, labels, **inventory_params)
        z_ref = base["z_low"]
        full = base if offset is None else inv_ref.tree_inventory(coords, labels, offset=offset, **inventory_params)
    else:
        import terrain_restatement as ter_ref
        base = ter_ref.tree_inventory(coords, labels, terrain, **inventory_params)
        z_ref = base["z_ground"]
        full = base if offset is None else ter_ref.tree_inventory(coords, labels, terrain, offset=offset, **inventory_params)
    res = dict(full)
    res.update(wood_structure(coords, labels, base["x"], base["y"], z_ref, offset=offset, branch_cfg=branch_cfg, wood_cfg=wood_cfg))
    if terrain is None:
        res["margins"]["z_ref"] = np.inf
    return res
