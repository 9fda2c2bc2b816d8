"""Hand cases of the branch structure: tens to hundreds of voxels each, built from lists of voxel indices.  A case is a dict of
xyz f64 [N, 3], lab i64 [N], tree f64 [T, 4] (px, py, z_ref, z_top: the case's own table, handed to the stage as it is), cfg (branch
parameters) and check(inv, d_of): assertions on the columns and on d_of(tree, (ix, iy, iz)), the distance of a voxel (None for a voxel the
tree does not have).  Rows sit at voxel centres, positions at the centre of voxel (0, 0) unless the case says otherwise, z_ref in the
middle of layer 0.  The voxel edge is 0.125 m (centres and single-voxel centroids are exact: the mirror case needs an exact tie) except
where a case sets 0.1 m."""
import numpy as np

V = 0.125
BLOCK = 1024                                                  # threads of tl_skel_distance's workgroup
THIN = dict(voxel=V, base_reach=0, base_layers=1, level=1)    # the source is the lowest voxel of the tree's own column; a node per step


def pole(h, x=0, y=0, z0=0):
    return [(x, y, z0 + k) for k in range(h)]


def build(trees, cfg, check, positions=None, z_ref=None, repeat=1, seed=0):
    """trees: a list of voxel lists (None: a label without rows).  Rows at voxel centres, `repeat` of them per voxel, shuffled."""
    v = cfg.get("voxel", 0.1)
    rows, lab, table = [], [], []
    for t, vox in enumerate(trees):
        pos = positions[t] if positions is not None else (0, 0)
        zr = z_ref[t] if z_ref is not None else 0
        if vox is None:
            table.append([np.nan] * 4)
            continue
        c = (np.asarray(vox, np.float64).reshape(-1, 3) + 0.5) * v
        rows.append(np.repeat(c, repeat, axis=0)); lab.append(np.full(len(c) * repeat, t + 1, np.int64))
        table.append([(pos[0] + 0.5) * v, (pos[1] + 0.5) * v, (zr + 0.5) * v, c[:, 2].max()])
    xyz, lab = np.concatenate(rows), np.concatenate(lab)
    p = np.random.default_rng(seed).permutation(len(xyz))
    return dict(xyz=np.ascontiguousarray(xyz[p]), lab=np.ascontiguousarray(lab[p]), tree=np.asarray(table, np.float64), cfg=cfg, check=check)


def case_pole():
    """30 voxels of 0.1 m, level 3: ten nodes three voxels apart, an axis of 9 x 0.3 m, no branch."""
    def check(inv, d_of):
        assert d_of(0, (0, 0, 29)) == 2900
        assert inv["skel_voxels"][0] == inv["skel_reached"][0] == 30 and inv["skel_nodes"][0] == 10 and inv["skel_tips"][0] == 1
        assert abs(inv["axis_length"][0] - 2.7) < 1e-9 and abs(inv["skel_length"][0] - 2.7) < 1e-9 and abs(inv["axis_top_h"][0] - 2.8) < 1e-9
        assert abs(inv["path_mean_tips"][0] - 2.7) < 1e-9
        assert inv["branch_count"][0] == 0 and inv["branch_order_max"][0] == 0 and inv["branch_length"][0] == 0.0 and np.isnan(inv["first_branch_h"][0])
        assert inv["skeleton"]["parent"].tolist() == [-1] + list(range(9)) and inv["skeleton"]["count"].tolist() == [3] * 10
    return build([pole(30)], dict(voxel=0.1, base_reach=0, base_layers=1, level=3), check)


def case_pole_defaults():
    """The same pole under the default parameters: five source layers, so bin 0 holds seven voxels."""
    def check(inv, d_of):
        assert [d_of(0, (0, 0, k)) for k in (0, 4, 5, 29)] == [0, 0, 100, 2500]
        assert inv["skel_nodes"][0] == 9 and inv["skeleton"]["count"].tolist() == [7] + [3] * 7 + [2]
    return build([pole(30)], dict(), check)


def case_weights():
    """A face arm, an edge-diagonal arm and a space-diagonal arm off one pole: 100, 141 and 173 per step."""
    arm_x = [(k, 0, 5) for k in range(1, 7)]
    arm_e = [(0, k, 8 + k) for k in range(1, 6)]
    arm_s = [(-k, -k, 2 + k) for k in range(1, 4)]

    def check(inv, d_of):
        assert [d_of(0, v) for v in arm_x] == [541] + [541 + 100 * k for k in range(1, 6)]          # (the first step comes up from (0, 0, 4))
        assert [d_of(0, v) for v in arm_e] == [800 + 141 * k for k in range(1, 6)]
        assert [d_of(0, v) for v in arm_s] == [200 + 173 * k for k in range(1, 4)]
        assert inv["skel_reached"][0] == inv["skel_voxels"][0] == 16 + 14
    return build([pole(16) + arm_x + arm_e + arm_s], dict(THIN), check)


def _plate(reach):
    def check(inv, d_of):
        assert d_of(0, (1, 1, 0)) == 141 and d_of(0, (2, 2, 0)) == 282 and d_of(0, (4, 4, 0)) == 564 and d_of(0, (4, 0, 0)) == 400
        assert d_of(0, (3, 1, 0)) == (341 if reach == 1 else 323) and d_of(0, (2, 1, 0)) == (241 if reach == 1 else 223)
        assert inv["skel_reached"][0] == 25
    return build([[(x, y, 0) for x in range(5) for y in range(5)]], dict(THIN, reach=reach), check)


def case_staircase():
    """A 5 x 5 plate from one corner: two diagonal steps (282) beat the face paths (400, 341) to (2, 2) and land in a later bucket."""
    return _plate(1)


def case_staircase_reach_2():
    return _plate(2)


def _y(n_minus, n_plus):
    return pole(10) + [(k, 0, 9 + k) for k in range(1, n_plus + 1)] + [(-k, 0, 9 + k) for k in range(1, n_minus + 1)]


def case_y_unequal():
    """Arms of 5 (towards -x) and 8 (towards +x) voxels: the longer one carries the axis."""
    def check(inv, d_of):
        sk = inv["skeleton"]
        top = np.flatnonzero(sk["branch"] == sk["branch"][0])[-1]
        assert sk["xyz"][top, 0] > 8 * V and inv["skel_tips"][0] == 2 and inv["branch_count"][0] == 1 and inv["branch_order_max"][0] == 1
        assert abs(inv["axis_top_h"][0] - 17 * V) < 1e-12
    return build([_y(5, 8)], dict(THIN), check)


def case_y_mirror():
    """Arms that are mirror images: an exact tie, and the arm of the lower node index (the smaller ix) carries the axis."""
    def check(inv, d_of):
        sk = inv["skeleton"]
        top = np.flatnonzero(sk["branch"] == sk["branch"][0])[-1]
        assert sk["xyz"][top, 0] < -5 * V and inv["branch_count"][0] == 1 and abs(inv["axis_length"][0] + inv["branch_length"][0] - inv["skel_length"][0]) < 1e-9
    return build([_y(6, 6)], dict(THIN), check)


def _gap(reach):
    arm = [(k, 0, 5) for k in range(2, 7)]

    def check(inv, d_of):
        if reach == 1:
            assert all(d_of(0, v) == -1 for v in arm) and inv["skel_reached"][0] == 10 and inv["skel_voxels"][0] == 15 and inv["branch_count"][0] == 0
        else:
            assert d_of(0, (1, 0, 5)) is None and d_of(0, arm[0]) == 582 and d_of(0, arm[-1]) == 982 and inv["skel_reached"][0] == 15
    return build([pole(10) + arm], dict(THIN, reach=reach, min_branch=0.3), check)


def case_gap():
    """An arm one empty voxel away from the pole: unreached with reach 1."""
    return _gap(1)


def case_gap_reach_2():
    """... and reached with reach 2, where the two-voxel edges weigh 200 (face), 223 and 282: the shortest way in is 300 + 282."""
    return _gap(2)


def case_blob():
    blob = [(x, y, z) for x in range(10, 13) for y in range(10, 13) for z in range(5, 8)]

    def check(inv, d_of):
        assert inv["skel_voxels"][0] == 12 + 27 and inv["skel_reached"][0] == 12 and all(d_of(0, v) == -1 for v in blob)
    return build([pole(12) + blob], dict(THIN), check)


def _ring(level):
    left, right = [(-1, 0, 6), (-2, 0, 7), (-2, 0, 8), (-1, 0, 9)], [(1, 0, 6), (2, 0, 7), (2, 0, 8), (1, 0, 9)]

    def check(inv, d_of):
        assert [d_of(0, v) for v in left] == [d_of(0, v) for v in right] == [641, 782, 882, 1023] and d_of(0, (0, 0, 10)) == 1164
        assert inv["skel_reached"][0] == 6 + 8 + 5
        if level == 1:                                    # the rejoining voxel hangs on the arm of the smaller key
            sk = inv["skeleton"]
            join = int(np.flatnonzero(sk["bin"] == 11)[0])
            assert sk["count"][join] == 1 and sk["xyz"][sk["parent"][join], 0] < 0
    return build([pole(6) + left + right + pole(5, z0=10)], dict(THIN, level=level), check)


def case_ring():
    """Two arms that part and rejoin: equal distances on both sides, the predecessor of the rejoining voxel is decided by the key."""
    return _ring(1)


def case_ring_level_3():
    """... and with level sets three voxels thick the two arms are one component of the bin they rejoin in."""
    return _ring(3)


def case_thick_trunk():
    """A trunk of 3 x 3 voxels: every level set is one node."""
    def check(inv, d_of):
        assert inv["skel_nodes"][0] == 4 and inv["skeleton"]["count"].tolist() == [27] * 4 and inv["skel_tips"][0] == 1
    return build([[(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in range(12)]], dict(voxel=V, base_reach=1, base_layers=1, level=3), check)


def two_trees():
    """Two poles three voxels apart whose arms end face to face: (2, 0, 5) of tree 1 touches (3, 0, 5) ... of tree 2's pole."""
    return [pole(10) + [(1, 0, 5), (2, 0, 5)], pole(10, x=3) + [(3, 1, 7), (2, 1, 7), (1, 1, 6)]]


def case_two_trees():
    def check(inv, d_of):
        assert d_of(0, (2, 0, 5)) == 641 and d_of(1, (3, 0, 5)) == 500 and d_of(0, (3, 0, 5)) is None
        assert inv["skel_reached"].tolist() == [12, 13] and inv["skel_voxels"].tolist() == [12, 13]
    return build(two_trees(), dict(THIN), check, positions=[(0, 0), (3, 0)])


def case_empty_slots():
    """Tree 1: a pole.  Label 2: no rows.  Tree 3: rows, none at its base column.  Tree 4: 30 voxels, more than max_voxels = 20."""
    def check(inv, d_of):
        assert inv["skel_voxels"].tolist() == [12, 0, 8, 30] and inv["skel_reached"].tolist() == [12, 0, 0, 0]
        assert inv["skel_nodes"].tolist() == [12, 0, 0, 0] and inv["skeleton"]["node_start"].tolist() == [0, 12, 12, 12, 12]
        for k in ("skel_length", "axis_length", "axis_top_h", "path_mean_tips", "branch_length", "first_branch_h"):
            assert np.isnan(inv[k][1:]).all(), k
        assert d_of(2, (5, 5, 0)) == -1 and d_of(3, (20, 0, 0)) == -1
    return build([pole(12), None, pole(8, x=5, y=5), pole(30, x=20)], dict(THIN, max_voxels=20), check, positions=[(0, 0), (0, 0), (0, 0), (20, 0)])


def case_below_z_ref():
    """z_ref in layer 3: the three layers below it take no part, and the sources start at layer 3."""
    def check(inv, d_of):
        assert inv["skel_voxels"][0] == 9 and d_of(0, (0, 0, 2)) is None and d_of(0, (0, 0, 3)) == 0 and d_of(0, (0, 0, 11)) == 800
    return build([pole(12)], dict(THIN), check, z_ref=[3])


def case_duplicates():
    """A thousand rows in one voxel."""
    def check(inv, d_of):
        assert inv["skel_voxels"][0] == inv["skel_reached"][0] == inv["skel_nodes"][0] == inv["skel_tips"][0] == 1
        assert inv["skel_length"][0] == 0.0 and inv["axis_length"][0] == 0.0 and inv["path_mean_tips"][0] == 0.0 and inv["branch_count"][0] == 0
    return build([[(0, 0, 0)]], dict(THIN), check, repeat=1000)


def _count(n):
    def case():
        def check(inv, d_of):
            assert inv["skel_voxels"][0] == inv["skel_reached"][0] == n and d_of(0, (0, 0, n - 1)) == 100 * (n - 1)
            assert inv["skel_nodes"][0] == (n + 2) // 3 and inv["skel_tips"][0] == 1
        return build([pole(n)], dict(voxel=V, base_reach=0, base_layers=1, level=3), check)
    case.__doc__ = f"A pole of {n} voxels: the strides of the kernels' loops."
    return case


def _arm(min_branch, min_height, counted, first):
    """A pole of 24 voxels with a horizontal arm of 8 at layer 12: 7.5 voxels (0.94 m) long, attached 1.5 m up."""
    def check(inv, d_of):
        assert inv["branch_count"][0] == inv["branch_count_1"][0] == inv["branch_order_max"][0] == int(counted)
        assert np.isnan(inv["first_branch_h"][0]) == (not first) and inv["skel_tips"][0] == 2
        if first:
            assert 1.0 < inv["first_branch_h"][0] < 2.0
    return build([pole(24) + [(k, 0, 12) for k in range(1, 9)]], dict(THIN, min_branch=min_branch, min_height=min_height), check)


CASES = {
    "pole": case_pole, "pole_defaults": case_pole_defaults, "weights": case_weights, "staircase": case_staircase,
    "staircase_reach_2": case_staircase_reach_2, "y_unequal": case_y_unequal, "y_mirror": case_y_mirror, "gap": case_gap,
    "gap_reach_2": case_gap_reach_2, "blob": case_blob, "ring": case_ring, "ring_level_3": case_ring_level_3, "thick_trunk": case_thick_trunk,
    "two_trees": case_two_trees, "empty_slots": case_empty_slots, "below_z_ref": case_below_z_ref, "duplicates": case_duplicates,
    "arm_counted": lambda: _arm(0.5, 1.0, True, True), "arm_too_short": lambda: _arm(1.5, 1.0, False, False),
    "arm_too_low": lambda: _arm(0.5, 2.0, True, False),
}
CASES.update({f"voxels_{n}": _count(n) for n in (1, 63, 64, 65, 257, BLOCK + 1)})


def d_lookup(case, keys, d):
    """d_of(tree, voxel) from the packed voxel keys (include/treelearn_hip.h) and their distances."""
    v = case["cfg"].get("voxel", 0.1)
    base = np.floor(case["tree"][:, :3] / v)
    table = dict(zip(np.asarray(keys).tolist(), np.asarray(d).tolist()))

    def d_of(t, vox):
        rel = [int(vox[k] - base[t, k]) for k in range(3)]
        return table.get((t << 35) | ((rel[0] + 2048) << 23) | ((rel[1] + 2048) << 11) | rel[2])
    return d_of


def _limbs(rng, origin, height, radius, depth, density=45):
    """Rows of a recursive stem-and-limb shape: a tapering limb with four limbs of its own, `depth` levels deep; the rows are scattered
    inside every limb at stations 2 cm apart, so that voxels of 0.1 m hang together."""
    parts = []

    def limb(p0, u, length, r0, level):
        s = np.linspace(0.0, length, int(length / 0.02) + 1)
        per = max(3, int(density * (r0 / 0.1) ** 2))
        a = np.cross(u, [0.0, 0.0, 1.0])
        a = a / np.linalg.norm(a) if np.linalg.norm(a) > 1e-6 else np.array([1.0, 0.0, 0.0])
        b = np.cross(u, a)
        r = r0 * (1.0 - 0.5 * s / length)
        rho = np.sqrt(rng.uniform(0, 1, (len(s), per))) * r[:, None]
        phi = rng.uniform(0, 2 * np.pi, (len(s), per))
        p = p0 + s[:, None, None] * u + (rho * np.cos(phi))[:, :, None] * a + (rho * np.sin(phi))[:, :, None] * b
        parts.append(p.reshape(-1, 3))
        if level == 0:
            return
        for _ in range(4):
            at = rng.uniform(0.35, 0.95) * length
            az, tilt = rng.uniform(0, 2 * np.pi), rng.uniform(0.6, 1.2)
            w = np.cos(tilt) * u + np.sin(tilt) * (np.cos(az) * a + np.sin(az) * b)
            limb(p0 + at * u, w / np.linalg.norm(w), 0.55 * length, 0.55 * r0, level - 1)

    limb(np.asarray(origin, np.float64), np.array([0.0, 0.0, 1.0]), height, radius, depth)
    return np.concatenate(parts)


def generated_tree(seed=3):
    """One tree of 12 m, three levels of limbs: about 15 000 voxels of 0.1 m.  Returns xyz f64 [N, 3] (shuffled) and lab i64 [N] (all 1)."""
    rng = np.random.default_rng(seed)
    xyz = _limbs(rng, [0.03, -0.02, 0.0], 12.0, 0.34, 3)
    xyz = xyz[rng.permutation(len(xyz))]
    return np.ascontiguousarray(xyz), np.ones(len(xyz), np.int64)


def three_trees(seed=11):
    """Three small trees (5 m, two levels of limbs) on sloping ground with its own rows (label 0) and a few unassigned rows (-1): an
    N x 4 cloud (x y z label) far from the origin, as a plot file holds it."""
    rng = np.random.default_rng(seed)
    surf = lambda x, y: 0.04 * x - 0.03 * y                               # noqa: E731
    rows, lab = [], []
    for t, (x, y) in enumerate([(-3.1, 0.4), (0.2, -1.3), (3.3, 1.1)]):
        p = _limbs(rng, [x, y, surf(x, y)], 5.0, 0.15, 2)
        rows.append(p); lab.append(np.full(len(p), t + 1, np.int64))
    gx, gy = rng.uniform(-7, 7, 6000), rng.uniform(-5, 5, 6000)
    rows.append(np.column_stack([gx, gy, surf(gx, gy) + rng.normal(0, 0.01, 6000)])); lab.append(np.zeros(6000, np.int64))
    rows.append(np.column_stack([rng.uniform(-7, 7, 200), rng.uniform(-5, 5, 200), rng.uniform(0, 6, 200)])); lab.append(np.full(200, -1, np.int64))
    xyz, lab = np.concatenate(rows), np.concatenate(lab)
    p = rng.permutation(len(xyz))
    return np.ascontiguousarray(np.column_stack([xyz[p] + np.array([1000.0, 2000.0, 50.0]), lab[p].astype(np.float64)]))
