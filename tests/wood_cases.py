"""Hand cases of the cylinder model.  A case is a dict of xyz f64 [N, 3], lab i64 [N], tree f64 [T, 4] (px, py, z_ref, z_top: the
case's own table, handed to the stages as it is), branch_cfg, wood_cfg and check(inv): assertions on the columns, "skeleton" and
"cylinders".  Voxels are 0.5 m wide and a level set is one voxel thick, so a stack of voxels is a chain of nodes whose centroids are the
voxel centres (exact in binary); a node's rows lie on a ring around its voxel's centre, across the chord to the voxel below, unless the
case says otherwise.  Positions are the centre of voxel column (0, 0), z_ref the middle of layer 0.
Unless a case sets it, max_growth is 1.5: on a perfect cylinder a cap of 1.0 x the parent's radius equals the fitted radius to rounding,
and which of the two is the smaller is then no property of the input.  The cases with max_growth 1 taper by 2 mm per node (TAPER)."""
import math

import numpy as np

V = 0.5
THIN = dict(voxel=V, base_reach=0, base_layers=1, level=1)    # the source is the lowest voxel of the tree's own column; a node per voxel
R0 = 0.15
TAPER = [0.15, 0.148, 0.146, 0.144, 0.142]
PI = math.pi


def centre(v):
    return (np.asarray(v, np.float64) + 0.5) * V


def ring(c, a, r, n, phase=0.1, arc=2 * PI, shift=(0.0, 0.0)):
    """n points on the circle of radius r around c + shift (in the plane's own basis), across the unit vector a; over `arc` radians."""
    a = np.asarray(a, np.float64) / np.linalg.norm(a)
    h = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(a, h); e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    phi = phase + arc * np.arange(n) / n
    return np.asarray(c, np.float64) + (shift[0] + r * np.cos(phi))[:, None] * e1 + (shift[1] + r * np.sin(phi))[:, None] * e2


def chain(voxels, radii, counts=16, first_axis=(0, 0, 1), **kw):
    """[(voxel, rows)] of a chain of voxels: a ring per voxel around its centre, across the chord from the voxel before."""
    radii = [radii] * len(voxels) if np.isscalar(radii) else radii
    counts = [counts] * len(voxels) if np.isscalar(counts) else counts
    out = []
    for j, v in enumerate(voxels):
        a = first_axis if j == 0 else np.subtract(v, voxels[j - 1])
        out.append((v, ring(centre(v), a, radii[j], counts[j], **kw)))
    return out


def pole(h, x=0, y=0, z0=0):
    return [(x, y, z0 + k) for k in range(h)]


def build(trees, check, branch_cfg=None, wood_cfg=None, positions=None, z_ref=None, seed=0):
    """trees: a list of [(voxel, rows)] lists (None: a label without rows)."""
    rows, lab, table = [], [], []
    for t, parts in enumerate(trees):
        pos = positions[t] if positions is not None else (0, 0)
        zr = z_ref[t] if z_ref is not None else 0
        if parts is None:
            table.append([np.nan] * 4)
            continue
        p = np.concatenate([r for _, r in parts])
        for v, r in parts:                                    # every row lies in the voxel it was made for (None: rows over several voxels)
            assert v is None or (np.floor(r / V) == np.asarray(v)).all(), v
        rows.append(p); lab.append(np.full(len(p), t + 1, np.int64))
        table.append([(pos[0] + 0.5) * V, (pos[1] + 0.5) * V, (zr + 0.5) * V, p[:, 2].max()])
    xyz, lab = np.concatenate(rows), np.concatenate(lab)
    q = np.random.default_rng(seed).permutation(len(xyz))
    return dict(xyz=np.ascontiguousarray(xyz[q]), lab=np.ascontiguousarray(lab[q]), tree=np.asarray(table, np.float64),
                branch_cfg=dict(THIN, **(branch_cfg or {})), wood_cfg=dict(wood_cfg or dict(max_growth=1.5)), check=check)


def frustum(L, R, r):
    return PI * L / 3.0 * (R * R + R * r + r * r)


def near(a, b, tol=1e-9):
    return bool(np.all(np.abs(np.asarray(a) - np.asarray(b)) <= tol))


def case_pole():
    """Six nodes of 16 points exactly on a circle of radius 0.15: every fit is 0.15, axis_dbh 0.30, the volume the cylinder's between
    the first and the last node (2.5 m).  The axis is (0, 0, 1) everywhere: the basis tie."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["state"].tolist() == [1] * 6 and cyl["n"].tolist() == [16] * 6 and near(cyl["radius_fit"], R0, 1e-12) and near(cyl["radius"], R0, 1e-12)
        assert near(cyl["rmse"], 0.0, 1e-12) and near(cyl["axis"], [[0, 0, 1]] * 6, 0) and near(cyl["centre"], inv["skeleton"]["xyz"], 1e-12)
        assert inv["wood_nodes_fit"][0] == 6 and near(inv["axis_dbh"][0], 0.30, 1e-12) and near(inv["wood_length"][0], 2.5, 1e-12)
        assert near(inv["wood_length"][0], inv["skel_length"][0]) and near(inv["wood_volume"][0], PI * R0 * R0 * 2.5, 1e-12)
        assert near(inv["axis_volume"][0], inv["wood_volume"][0]) and near(inv["wood_area"][0], 2 * PI * R0 * 2.5, 1e-12)
        assert inv["branch_volume"][0] == 0.0 and inv["branch_volume_1"][0] == 0.0 and np.isnan(inv["branch_base_diam_1"][0])
        assert near(cyl["length"], [0.0] + [0.5] * 5, 1e-12) and near(cyl["volume"][1:], PI * R0 * R0 * 0.5, 1e-12) and cyl["volume"][0] == 0.0
    return build([chain(pole(6), R0)], check)


def case_pole_tilted():
    """The same pole along (1, 0, 1): the rings lie across the chords (the root's across the vertical, its own axis), so every node is
    fitted at 0.15 in a plane that is not a coordinate plane."""
    def check(inv):
        cyl, s = inv["cylinders"], math.sqrt(0.5)
        assert cyl["state"].tolist() == [1] * 6 and near(cyl["radius_fit"], R0, 1e-12) and near(cyl["radius"], R0, 1e-12)
        assert near(cyl["axis"][1:], [[s, 0, s]] * 5, 1e-15) and near(cyl["axis"][0], [0, 0, 1], 0) and near(cyl["centre"], inv["skeleton"]["xyz"], 1e-12)
        assert near(cyl["length"][1:], V * math.sqrt(2.0), 1e-12) and near(inv["wood_volume"][0], PI * R0 * R0 * 5 * V * math.sqrt(2.0), 1e-12)
    return build([chain([(k, 0, k) for k in range(6)], R0)], check)


def case_half_cylinder():
    """Half rings (a one-sided scan) whose circle stands 5 cm beside the node's centroid: the shift 0.05 <= r accepts.  Node 3 is a
    full ring of radius 0.05 standing 0.12 beside the centroid: the shift rejects it and it takes its parent's radius."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["state"].tolist() == [1, 1, 1, 2, 1] and near(cyl["radius_fit"][[0, 1, 2, 4]], [0.15, 0.148, 0.146, 0.142], 1e-12)
        assert np.isnan(cyl["radius_fit"][3]) and np.isnan(cyl["rmse"][3]) and np.isnan(cyl["centre"][3]).all() and inv["wood_nodes_fit"][0] == 4
        rad = [0.15, 0.148, 0.146, 0.146, 0.142]
        assert near(cyl["radius"], rad, 1e-12)
        off = np.linalg.norm(cyl["centre"][[0, 1, 2, 4]] - inv["skeleton"]["xyz"][[0, 1, 2, 4]], axis=1)
        assert near(off, 0.05, 1e-12) and near(inv["wood_volume"][0], sum(frustum(V, rad[i], rad[i + 1]) for i in range(4)), 1e-12)
    parts = chain(pole(5), TAPER, counts=32, arc=PI, shift=(0.05, 0.0))
    parts[3] = ((0, 0, 3), ring(centre((0, 0, 3)), (0, 0, 1), 0.05, 32, shift=(0.12, 0.0)))
    return build([parts], check, wood_cfg=dict(max_growth=1.0))


def case_blob():
    """The top node is a cloud of 60 points scattered in a ball: the circle through it leaves an rmse beyond 3 cm and is rejected."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["state"].tolist() == [1, 1, 1, 2] and cyl["n"][3] == 60 and np.isnan(cyl["radius_fit"][3]) and near(cyl["radius"][3], 0.146, 1e-12)
    parts = chain(pole(3), TAPER[:3])
    rng = np.random.default_rng(4)
    d = rng.normal(size=(60, 3))
    parts.append(((0, 0, 3), centre((0, 0, 3)) + 0.2 * rng.uniform(0, 1, (60, 1)) ** (1 / 3) * d / np.linalg.norm(d, axis=1, keepdims=True)))
    return build([parts], check, wood_cfg=dict(max_growth=1.0))


def case_min_points():
    """Nodes of min_points - 1 = 7 and of 8 rows: no fit and a fit."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["n"].tolist() == [16, 7, 8, 16] and cyl["state"].tolist() == [1, 0, 1, 1] and np.isnan(cyl["radius_fit"][1])
        assert near(cyl["radius"], [0.15, 0.15, 0.146, 0.144], 1e-12) and inv["wood_nodes_fit"][0] == 3
    return build([chain(pole(4), TAPER[:4], counts=[16, 7, 8, 16])], check, wood_cfg=dict(max_growth=1.0))


def case_wave_strides():
    """Nodes of 63 / 64 / 65 / 129 rows: the edges of the wavefront's stride."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["n"].tolist() == [16, 63, 64, 65, 129] and cyl["state"].tolist() == [1] * 5 and near(cyl["radius_fit"], TAPER, 1e-12)
        assert near(cyl["radius"], TAPER, 1e-12) and inv["wood_nodes_fit"][0] == 5
    return build([chain(pole(5), TAPER, counts=[16, 63, 64, 65, 129])], check, wood_cfg=dict(max_growth=1.0))


def case_one_big_node():
    """5 000 rows in a single voxel: one node, a root, no segment: the sums are 0.0."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["n"].tolist() == [5000] and cyl["state"].tolist() == [1] and near(cyl["radius_fit"], 0.2, 1e-12) and inv["wood_nodes_fit"][0] == 1
        assert inv["wood_volume"][0] == 0.0 and inv["wood_length"][0] == 0.0 and inv["wood_area"][0] == 0.0 and np.isnan(inv["axis_dbh"][0])
    return build([chain(pole(1), 0.2, counts=5000)], check)


def y_tree():
    """A pole of 8 with an arm of 6 towards +x (radius 0.10: it carries the axis) and a thin limb of 4 towards -x (radius 0.04)."""
    stem = chain(pole(8), R0)
    arm = chain([(0, 0, 7)] + [(k, 0, 7 + k) for k in range(1, 7)], 0.10)[1:]
    limb = chain([(0, 0, 7)] + [(-k, 0, 7 + k) for k in range(1, 5)], 0.04)[1:]
    return stem + arm + limb


def case_y_thin_limb():
    def check(inv):
        L = V * math.sqrt(2.0)
        limb = frustum(L, R0, 0.04) + 3 * frustum(L, 0.04, 0.04)
        assert inv["branch_count"][0] == inv["branch_count_1"][0] == 1 and inv["wood_nodes_fit"][0] == 18
        assert near(inv["branch_volume_1"][0], limb, 1e-12) and near(inv["branch_volume"][0], limb, 1e-12) and near(inv["branch_base_diam_1"][0], 0.08, 1e-12)
        axis = PI * R0 * R0 * 3.5 + frustum(L, R0, 0.10) + 5 * frustum(L, 0.10, 0.10)
        assert near(inv["axis_volume"][0], axis, 1e-12) and near(inv["wood_volume"][0], axis + limb, 1e-12) and near(inv["axis_dbh"][0], 0.30, 1e-12)
    return build([y_tree()], check)


def _thick_child(growth):
    def check(inv):
        cyl = inv["cylinders"]
        fits = [0.15, 0.148, 0.146, 0.2, 0.142]
        assert near(cyl["radius_fit"], fits, 1e-12)
        assert near(cyl["radius"], [0.15, 0.148, 0.146, 0.146, 0.142] if growth == 1.0 else fits, 1e-12) and inv["wood_nodes_fit"][0] == (4 if growth == 1.0 else 5)
    return build([chain(pole(5), [0.15, 0.148, 0.146, 0.2, 0.142])], check, wood_cfg=dict(max_growth=growth))


def case_child_capped():
    """A child fitted thicker (0.20) than its parent (0.15) is capped with max_growth 1 ..."""
    return _thick_child(1.0)


def case_child_within_growth():
    """... and kept with max_growth 1.5 (cap 0.219); its own child is then fitted below its cap of 0.30."""
    return _thick_child(1.5)


def case_unfitted_tip():
    """A tip of three rows takes its parent's radius, and its segment is modelled."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["state"].tolist() == [1, 1, 1, 0] and near(cyl["radius"], [0.15, 0.148, 0.146, 0.146], 1e-12) and inv["wood_nodes_fit"][0] == 3
        assert near(inv["wood_volume"][0], frustum(V, 0.15, 0.148) + frustum(V, 0.148, 0.146) + frustum(V, 0.146, 0.146), 1e-12)
    return build([chain(pole(4), TAPER[:4], counts=[16, 16, 16, 3])], check, wood_cfg=dict(max_growth=1.0))


def case_unfitted_root():
    """The two lowest nodes have three rows each: the root takes the first fit along its branch (0.12), node 1 its cap of 1.5 x that."""
    def check(inv):
        cyl = inv["cylinders"]
        assert cyl["state"].tolist() == [0, 0, 1, 1] and near(cyl["radius"], [0.12, 0.18, 0.12, 0.118], 1e-12) and inv["wood_nodes_fit"][0] == 2
        assert near(inv["wood_volume"][0], frustum(V, 0.12, 0.18) + frustum(V, 0.18, 0.12) + frustum(V, 0.12, 0.118), 1e-12)
    return build([chain(pole(4), [0.12, 0.12, 0.12, 0.118], counts=[3, 3, 16, 16])], check)


def case_no_fit_at_all():
    """One row per node: a skeleton without a finite radius: 0.0 in the sums, 0 fitted nodes, NaN diameters."""
    def check(inv):
        assert inv["skel_nodes"][0] == 5 and inv["wood_nodes_fit"][0] == 0 and np.isnan(inv["cylinders"]["radius"]).all()
        for k in ("wood_length", "wood_volume", "wood_area", "axis_volume", "branch_volume", "branch_volume_1"):
            assert inv[k][0] == 0.0, k
        assert np.isnan(inv["axis_dbh"][0]) and np.isnan(inv["branch_base_diam_1"][0])
    return build([chain(pole(5), R0, counts=1)], check)


def two_trees():
    return [chain(pole(5), R0), chain(pole(6, x=1), 0.10)]


def case_two_trees():
    """Two poles in touching voxel columns: no row of one takes part in the other's fits."""
    def check(inv):
        assert near(inv["cylinders"]["radius_fit"], [R0] * 5 + [0.10] * 6, 1e-12) and inv["cylinders"]["n"].tolist() == [16] * 11
        assert near(inv["wood_volume"], [PI * R0 * R0 * 2.0, PI * 0.01 * 2.5], 1e-12)
    return build(two_trees(), check, positions=[(0, 0), (1, 0)])


def case_empty_slots():
    """Tree 1: a pole.  Label 2: no rows.  Tree 3: rows, none at its base column: no skeleton.  Tree 4: a pole."""
    def check(inv):
        assert inv["skel_nodes"].tolist() == [4, 0, 0, 3] and inv["wood_nodes_fit"].tolist() == [4, 0, 0, 3]
        assert inv["cylinders"]["node_start"].tolist() == [0, 4, 4, 4, 7] and len(inv["cylinders"]["radius"]) == 7
        for k in ("wood_length", "wood_volume", "wood_area", "axis_volume", "branch_volume", "branch_volume_1", "axis_dbh", "branch_base_diam_1"):
            assert np.isnan(inv[k][1:3]).all(), k
        assert near(inv["wood_volume"][[0, 3]], [PI * R0 * R0 * 1.5, PI * R0 * R0 * 1.0], 1e-12)
    return build([chain(pole(4), R0), None, chain(pole(4, x=5, y=5), R0), chain(pole(3, x=9), R0)], check,
                 positions=[(0, 0), (0, 0), (0, 0), (9, 0)])


def case_below_z_ref():
    """z_ref in layer 2: the rows of the two layers below it belong to no node."""
    def check(inv):
        assert inv["skel_nodes"][0] == 4 and inv["cylinders"]["n"].tolist() == [16] * 4 and near(inv["wood_length"][0], 1.5, 1e-12)
        assert near(inv["axis_dbh"][0], 0.30, 1e-12)                                  # 1.3 m above z_ref: between the nodes at 1.0 and 1.5 m
    return build([chain(pole(6), R0)], check, z_ref=[2])


def case_unreached():
    """A ring of rows in a voxel that hangs in the air: it is a voxel of the tree, unreached, and its rows belong to no node."""
    def check(inv):
        assert inv["skel_voxels"][0] == 5 and inv["skel_reached"][0] == 4 and inv["cylinders"]["n"].tolist() == [16] * 4
    return build([chain(pole(4), R0) + chain([(3, 0, 2)], 0.10)], check)


def case_seg_zero():
    """A plate of 3 x 3 voxels: the root is the centre voxel, and the ring of eight voxels around it is one node whose centroid is the
    root's: seg == 0, the axis is (0, 0, 1), and the segment has no length and no volume.  Its rows lie on a circle of radius 0.6,
    capped at 1.5 x the root's 0.15."""
    def check(inv):
        cyl, sk = inv["cylinders"], inv["skeleton"]
        assert sk["parent"].tolist() == [-1, 0] and sk["count"].tolist() == [1, 8] and (sk["xyz"][0] == sk["xyz"][1]).all()
        assert near(cyl["axis"], [[0, 0, 1]] * 2, 0) and cyl["n"].tolist() == [16, 64] and cyl["state"].tolist() == [1, 1]
        assert near(cyl["radius_fit"], [R0, 0.6], 1e-12) and near(cyl["radius"], [R0, 0.225], 1e-12) and inv["wood_nodes_fit"][0] == 1
        assert inv["wood_length"][0] == 0.0 and inv["wood_volume"][0] == 0.0 and near(inv["wood_area"][0], PI * (R0 + 0.225) * 0.075, 1e-12)
    c = centre((0, 0, 0))
    return build([[((0, 0, 0), ring(c, (0, 0, 1), R0, 16)), (None, ring(c, (0, 0, 1), 0.6, 64))]], check)


CASES = {
    "pole": case_pole, "pole_tilted": case_pole_tilted, "half_cylinder": case_half_cylinder, "blob": case_blob, "min_points": case_min_points,
    "wave_strides": case_wave_strides, "one_big_node": case_one_big_node, "y_thin_limb": case_y_thin_limb, "child_capped": case_child_capped,
    "child_within_growth": case_child_within_growth, "unfitted_tip": case_unfitted_tip, "unfitted_root": case_unfitted_root,
    "no_fit_at_all": case_no_fit_at_all, "two_trees": case_two_trees, "empty_slots": case_empty_slots, "below_z_ref": case_below_z_ref,
    "unreached": case_unreached, "seg_zero": case_seg_zero,
}


def surface_tree(seed=7, n_stem=24000, n_limb=4000):
    """A tapered trunk (8 m, radius 0.20 -> 0.08) and two straight limbs (1.5 m, radius 0.05), surface points only.  Returns xyz f64
    [N, 3] (shuffled), lab i64 [N] and the analytic figures: the trunk's radius at a height, the volume of the trunk and of a limb."""
    rng = np.random.default_rng(seed)
    H, ra, rb = 8.0, 0.20, 0.08

    def r_at(h):
        return ra + (rb - ra) * h / H
    z = rng.uniform(0.0, H, n_stem)
    phi = rng.uniform(0.0, 2 * PI, n_stem)
    parts = [np.column_stack([0.02 + r_at(z) * np.cos(phi), -0.03 + r_at(z) * np.sin(phi), z])]
    for h0, az in ((4.0, 0.3), (5.5, 2.6)):
        u = np.array([math.cos(az) * math.sin(1.0), math.sin(az) * math.sin(1.0), math.cos(1.0)])
        s = rng.uniform(0.0, 1.5, n_limb)
        parts.append(np.array([0.02, -0.03, h0]) + s[:, None] * u + _around(u, 0.05, rng.uniform(0.0, 2 * PI, n_limb)))
    xyz = np.concatenate(parts)
    xyz = xyz[rng.permutation(len(xyz))]
    return np.ascontiguousarray(xyz), np.ones(len(xyz), np.int64), dict(r_at=r_at, H=H, trunk_volume=PI * H / 3.0 * (ra * ra + ra * rb + rb * rb),
                                                                        limb_volume=PI * 0.05 * 0.05 * 1.5)


def _around(u, r, phi):
    h = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(u, h); e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    return r * np.cos(phi)[:, None] * e1 + r * np.sin(phi)[:, None] * e2


def generated_surface_tree(seed=3):
    """The stem-and-limb shape of the branch tests (12 m, three levels of four limbs, every limb tapering to half its radius) with rows on
    the limbs' surfaces only, at stations 2.5 cm apart: about 14 000 voxels of 0.1 m.  Returns xyz f64 [N, 3] (shuffled), lab i64 [N]."""
    rng = np.random.default_rng(seed)
    parts = []

    def limb(p0, u, length, r0, level):
        s = np.linspace(0.0, length, int(length / 0.025) + 1)
        per = max(8, int(40 * r0 / 0.1))
        r = r0 * (1.0 - 0.5 * s / length)
        phi = rng.uniform(0, 2 * PI, (len(s), per))
        h = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
        a = np.cross(u, h); a = a / np.linalg.norm(a)
        b = np.cross(u, a)
        p = p0 + s[:, None, None] * u + (r[:, None] * np.cos(phi))[:, :, None] * a + (r[:, None] * np.sin(phi))[:, :, None] * b
        parts.append(p.reshape(-1, 3))
        if level == 0:
            return
        for _ in range(4):
            at = rng.uniform(0.35, 0.95) * length
            az, tilt = rng.uniform(0, 2 * PI), rng.uniform(0.6, 1.2)
            w = np.cos(tilt) * u + np.sin(tilt) * (np.cos(az) * a + np.sin(az) * b)
            limb(p0 + at * u, w / np.linalg.norm(w), 0.55 * length, 0.55 * r0, level - 1)

    limb(np.array([0.03, -0.02, 0.0]), np.array([0.0, 0.0, 1.0]), 12.0, 0.34, 3)
    xyz = np.concatenate(parts)
    xyz = xyz[rng.permutation(len(xyz))]
    return np.ascontiguousarray(xyz), np.ones(len(xyz), np.int64)
