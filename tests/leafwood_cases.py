"""Hand cases of the leaf-wood separation: the smallest shapes at which the seed rule, the vote and the connectivity filter can
go wrong, and a generated leaf-on tree with a known truth per row.

VOTE_CASES: name -> dict(xyz f64 [n, 3], tree i64 [n] (>= 0), flag u8 [n], p: parameters (radius, vote_iters, vote_percent), reverse: hand the
    piece table over reversed, want: the expected flags where the case states them by hand, else None: the restatement's).
SEED_CASES: (feats f32 [n, 4] = linearity, planarity, verticality, number_of_neighbors; want u8 [n]) at the parameters SEED_P.
COMPONENT_CASES: name -> dict(xyz, lab, tree f64 [T, 4], p, want: wood flags by group of rows).  Their thresholds make every row with
    three neighbours a seed (linearity_min 0) and vote_iters is 0, so that the flags in front of the filter are known."""
import math

import numpy as np

R = 0.2
PI = math.pi


def _vote(xyz, tree, flag, want=None, reverse=False, **p):
    return dict(xyz=np.ascontiguousarray(xyz, np.float64).reshape(-1, 3), tree=np.asarray(tree, np.int64).reshape(-1), flag=np.asarray(flag, np.uint8).reshape(-1),
                p=dict(dict(radius=R, vote_iters=1, vote_percent=50), **p), reverse=reverse, want=None if want is None else np.asarray(want, np.uint8))


def vote_alone():
    """A row with no other row within the radius: a = 1, w = its own flag: the flag stays, whatever it is."""
    return _vote([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0], [0.0, 7.0, 3.0]], [0, 0, 0], [1, 0, 1], want=[1, 0, 1], vote_iters=3)


def vote_pair(percent):
    """a = 2, w = 1: 100 >= 2 * 50 holds, 100 >= 2 * 51 does not."""
    return _vote([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]], [0, 0], [1, 0], want=[1, 1] if percent == 50 else [0, 0], vote_percent=percent)


def in_place(flag, percent, rounds):
    """The checkerboard line updated in place, left to right: what the kernel must NOT compute."""
    f = [int(v) for v in flag]
    for _ in range(rounds):
        for i in range(len(f)):
            nb = [j for j in (i - 1, i, i + 1) if 0 <= j < len(f)]
            f[i] = int(100 * sum(f[j] for j in nb) >= percent * len(nb))
    return np.asarray(f, np.uint8)


def vote_checkerboard(iters):
    """41 rows 0.15 apart on a line, flags 1 0 1 0 ...: every row sees itself and its two neighbours.  At 60 percent an inner row takes
    the flag of its neighbours, so the synchronous rounds flip the pattern; an update in place gives another answer."""
    n = 41
    xyz = np.zeros((n, 3)); xyz[:, 0] = -2.0 + 0.15 * np.arange(n)
    flag = (np.arange(n) % 2 == 0).astype(np.uint8)
    f = flag.astype(np.int64)
    for _ in range(iters):
        pad = np.concatenate([[0], f, [0]])
        a = np.full(n, 3); a[[0, -1]] = 2
        f = (100 * (pad[:-2] + pad[1:-1] + pad[2:]) >= 60 * a).astype(np.int64)
    if iters:
        assert not np.array_equal(f, in_place(flag, 60, iters))
    return _vote(xyz, np.zeros(n, np.int64), flag, want=f, vote_iters=iters, vote_percent=60)


def vote_two_trees_one_cell():
    """40 rows of two trees interleaved in a cube of 0.1 m, one tree flagged and one not: each row counts its own tree only, so the flags
    stay; counted together every row would see 50 percent and turn 1."""
    rng = np.random.default_rng(11)
    tree = np.arange(40) % 2
    return _vote(rng.uniform(0.0, 0.1, (40, 3)), tree, tree == 0, want=(tree == 0), vote_iters=2)


def vote_column_counts():
    """Four columns of cells with 63 / 64 / 65 / 129 rows: the edges of the wavefront and of the aligned 64-blocks."""
    rng = np.random.default_rng(12)
    parts = [np.array([3.0 * k, 0.0, 0.0]) + rng.uniform(0.0, [0.19, 0.19, 0.5], (c, 3)) for k, c in enumerate((63, 64, 65, 129))]
    xyz = np.concatenate(parts)
    return _vote(xyz, rng.integers(0, 2, len(xyz)), rng.integers(0, 2, len(xyz)), vote_iters=2)


def vote_blob():
    """3 000 rows in a cube of 1 m with a radius of 0.5 m: candidate ranges of more than 128 and of more than 256 rows."""
    rng = np.random.default_rng(13)
    return _vote(rng.uniform(0.0, 1.0, (3000, 3)), rng.integers(0, 3, 3000), rng.integers(0, 2, 3000), radius=0.5, vote_iters=2, vote_percent=40)


def vote_partial_tail():
    """200 rows in a cube of 0.3 m: the last piece holds 8 rows and the last chunk of every range is partly empty."""
    rng = np.random.default_rng(14)
    return _vote(rng.uniform(0.0, 0.3, (200, 3)), np.zeros(200, np.int64), rng.integers(0, 2, 200), vote_iters=1, vote_percent=45)


def vote_single_column():
    """One column of cells: the eight columns around it are empty ranges or lie outside the cloud."""
    rng = np.random.default_rng(15)
    return _vote(rng.uniform(0.0, [0.05, 0.05, 2.0], (150, 3)), np.zeros(150, np.int64), rng.integers(0, 2, 150), vote_iters=2)


def vote_negative_on_boundaries(reverse=False):
    """Negative coordinates, cells of 0.25 m from the origin -1.25: a lattice of rows 0.5 m apart lies exactly on cell boundaries (its rows
    are further than the radius from each other), 600 random rows fill the space between."""
    rng = np.random.default_rng(16)
    g = -1.0 + 0.5 * np.arange(3)
    lattice = np.array([[x, y, z] for x in g for y in g for z in g])
    xyz = np.concatenate([lattice, rng.uniform(-1.0, 0.0, (600, 3))])
    return _vote(xyz, rng.integers(0, 2, len(xyz)), rng.integers(0, 2, len(xyz)), radius=0.25, vote_iters=2, reverse=reverse)


VOTE_CASES = {
    "alone": vote_alone, "pair_50": lambda: vote_pair(50), "pair_51": lambda: vote_pair(51), "checkerboard_0": lambda: vote_checkerboard(0),
    "checkerboard_1": lambda: vote_checkerboard(1), "checkerboard_3": lambda: vote_checkerboard(3), "two_trees_one_cell": vote_two_trees_one_cell,
    "column_counts": vote_column_counts, "blob": vote_blob, "partial_tail": vote_partial_tail, "single_column": vote_single_column,
    "negative_on_boundaries": vote_negative_on_boundaries, "pieces_reversed": lambda: vote_negative_on_boundaries(reverse=True),
}


SEED_P = dict(linearity_min=0.7, planarity_min=0.6, verticality_min=0.7, min_neighbours=5)


def seed_cases():
    """Every branch of rule 2 at SEED_P (linearity 0.7, planarity 0.6 with verticality 0.7, five neighbours).  The f32 nearest to 0.7
    lies below the f64 0.7 and the f32 nearest to 0.6 above the f64 0.6: widened, the first fails its threshold and the second meets it."""
    nan, inf = float("nan"), float("inf")
    rows = [
        ((0.9, 0.0, 0.0, 50), 1),        # a limb
        ((0.1, 0.8, 0.9, 50), 1),        # a patch of stem surface
        ((0.1, 0.8, 0.1, 50), 0),        # planar, not vertical
        ((0.1, 0.1, 0.9, 50), 0),        # vertical, not planar
        ((0.1, 0.1, 0.1, 50), 0),        # neither
        ((0.9, 0.8, 0.9, 4), 0),         # min_neighbours - 1
        ((0.9, 0.8, 0.9, 5), 1),         # min_neighbours
        ((nan, 0.8, 0.9, 50), 0), ((0.9, nan, 0.0, 50), 0), ((0.9, 0.0, nan, 50), 0), ((0.9, 0.8, 0.9, nan), 0),
        ((inf, 0.0, 0.0, 50), 0), ((0.9, inf, 0.0, 50), 0), ((0.9, 0.0, -inf, 50), 0),
        ((0.7, 0.0, 0.0, 50), 0),        # f32(0.7) < 0.7
        ((0.75, 0.0, 0.0, 50), 1),
        ((0.0, 0.6, 0.75, 50), 1),       # f32(0.6) > 0.6
        ((0.0, 0.6, 0.7, 50), 0),        # f32(0.7) < 0.7
        ((1.0, 1.0, 1.0, 1e9), 1), ((0.0, 0.0, 0.0, 0), 0),
    ]
    rows = rows * 30 + rows[:7]                                               # 607 rows: more than one block, not a multiple of the block
    return np.asarray([r for r, _ in rows], np.float32), np.asarray([w for _, w in rows], np.uint8)


# ------------------------------------------------------------------------------------------------ the connectivity filter
V = 0.1
ALL_SEED = dict(radius=R, min_neighbours=3, linearity_min=0.0, planarity_min=1.0, verticality_min=1.0, vote_iters=0, voxel=V, reach=1)


def chain(rng, voxels, per=4):
    """`per` rows strictly inside each of the voxels (given as integer triples)."""
    v = np.repeat(np.asarray(voxels, np.float64), per, axis=0)
    return (v + rng.uniform(0.1, 0.9, v.shape)) * V


def pole(n, x=0, y=0, z0=0):
    return [(x, y, z0 + k) for k in range(n)]


def _anchor(x, y, z):
    return [(x + 0.5) * V, (y + 0.5) * V, (z + 0.5) * V, np.nan]


def _comp(groups, tree, **p):
    """groups: [(label, rows, wood flag expected for all of them)]."""
    xyz = np.concatenate([g[1] for g in groups])
    lab = np.concatenate([np.full(len(g[1]), g[0], np.int64) for g in groups])
    want = np.concatenate([np.full(len(g[1]), g[2], np.uint8) for g in groups])
    q = np.random.default_rng(21).permutation(len(xyz))
    return dict(xyz=np.ascontiguousarray(xyz[q]), lab=np.ascontiguousarray(lab[q]), want=want[q], tree=np.asarray(tree, np.float64).reshape(-1, 4),
                p=dict(ALL_SEED, **p))


def comp_threshold():
    """Two poles of one tree 3 m apart: 19 voxels (min_component - 1: dropped) and 20 voxels (kept)."""
    rng = np.random.default_rng(22)
    return _comp([(1, chain(rng, pole(19)), 0), (1, chain(rng, pole(20, x=30)), 1)], [_anchor(0, 0, 0)], min_component=20)


def comp_reach_2():
    """A pole of 20 voxels with every second voxel missing above the tenth: with reach 1 ten voxels hang together and ten are alone, with
    reach 2 all twenty."""
    rng = np.random.default_rng(23)
    vox = pole(10) + [(0, 0, 10 + 2 * k) for k in range(10)]
    return _comp([(1, chain(rng, vox, per=6), 1)], [_anchor(0, 0, 0)], min_component=20, reach=2)


def comp_reach_1_of_the_same():
    rng = np.random.default_rng(23)
    vox = pole(10) + [(0, 0, 10 + 2 * k) for k in range(10)]
    return _comp([(1, chain(rng, vox, per=6), 0)], [_anchor(0, 0, 0)], min_component=20, reach=1)


def comp_two_touching_trees():
    """Two poles of 15 voxels in touching voxel columns, one per tree: 30 voxels together, but no edge joins two trees: both dropped.
    A third tree's pole of 25 is kept."""
    rng = np.random.default_rng(24)
    return _comp([(1, chain(rng, pole(15)), 0), (2, chain(rng, pole(15, x=1)), 0), (3, chain(rng, pole(25, x=40)), 1)],
                 [_anchor(0, 0, 0), _anchor(1, 0, 0), _anchor(40, 0, 0)], min_component=20)


def comp_below_z_ref():
    """z_ref in layer 12 of a pole of 40: the 28 voxels from there on are a kept component; the rows below z_ref have no key and keep
    their voted flag.  A second pole of 10 voxels, all below z_ref, keeps its flags too although it is small."""
    rng = np.random.default_rng(25)
    return _comp([(1, chain(rng, pole(40)), 1), (1, chain(rng, pole(10, x=20)), 1)], [_anchor(0, 0, 12)], min_component=20)


def comp_small_above_z_ref():
    """The same with z_ref in layer 30: ten voxels above it: dropped; the 30 layers below keep their flags."""
    rng = np.random.default_rng(26)
    return _comp([(1, chain(rng, pole(30)), 1), (1, chain(rng, pole(10, z0=30)), 0)], [_anchor(0, 0, 30)], min_component=20)


def comp_no_position_and_empty_slots():
    """Tree 1: no position (NaN): no keys, the voted flags stay.  Label 2: no rows.  Tree 3: a pole of 5: dropped.  Label 4: no rows.  Tree
    5: a pole of 22: kept."""
    rng = np.random.default_rng(27)
    nan4 = [np.nan] * 4
    return _comp([(1, chain(rng, pole(5)), 1), (3, chain(rng, pole(5, x=20)), 0), (5, chain(rng, pole(22, x=40)), 1)],
                 [nan4, nan4, _anchor(20, 0, 0), nan4, _anchor(40, 0, 0)], min_component=20)


COMPONENT_CASES = {
    "threshold": comp_threshold, "reach_2": comp_reach_2, "reach_1_of_the_same": comp_reach_1_of_the_same, "two_touching_trees": comp_two_touching_trees,
    "below_z_ref": comp_below_z_ref, "small_above_z_ref": comp_small_above_z_ref, "no_position_and_empty_slots": comp_no_position_and_empty_slots,
}


# ------------------------------------------------------------------------------------------------ a generated leaf-on tree
def _basis(u):
    h = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    a = np.cross(u, h); a = a / np.linalg.norm(a)
    return a, np.cross(u, a)


def leaf_on_tree(seed=3, discs_per_tip=20, scatter_per_tip=300):
    """The stem-and-limb shape of the wood tests' generated tree (12 m, three levels of four limbs, every limb tapering to half its radius,
    rows on the limbs' surfaces at stations 2.5 cm apart, here 14 rows per station and 0.1 m of radius) with seeded foliage: around the
    outer half of every limb of the last level `discs_per_tip` leaves -- discs of 3 to 6 cm radius and random orientation, 20 to 40 rows
    each, within 0.6 m of the limb -- and `scatter_per_tip` loose rows in a ball of 0.5 m around its tip.  Rows closer than 2e-6 voxels
    (of 0.1 m) to a voxel boundary are left out, so that no floor of a row depends on its last bits.  Returns xyz f64 [N, 3] (shuffled),
    lab i64 [N] (all 1), truth u8 [N] (1: wood) and the summed length of all limbs' axes."""
    rng = np.random.default_rng(seed)
    wood, tips, total = [], [], [0.0]

    def limb(p0, u, length, r0, level):
        s = np.linspace(0.0, length, int(length / 0.025) + 1)
        per = max(8, int(14 * r0 / 0.1))
        r = r0 * (1.0 - 0.5 * s / length)
        phi = rng.uniform(0, 2 * PI, (len(s), per))
        a, b = _basis(u)
        p = p0 + s[:, None, None] * u + (r[:, None] * np.cos(phi))[:, :, None] * a + (r[:, None] * np.sin(phi))[:, :, None] * b
        wood.append(p.reshape(-1, 3))
        total[0] += length
        if level == 0:
            tips.append((p0, u, length))
            return
        for _ in range(4):
            at = rng.uniform(0.35, 0.95) * length
            az, tilt = rng.uniform(0, 2 * PI), rng.uniform(0.6, 1.2)
            w = np.cos(tilt) * u + np.sin(tilt) * (np.cos(az) * a + np.sin(az) * b)
            limb(p0 + at * u, w / np.linalg.norm(w), 0.55 * length, 0.55 * r0, level - 1)

    limb(np.array([0.03, -0.02, 0.0]), np.array([0.0, 0.0, 1.0]), 12.0, 0.34, 3)
    leaves = []
    for p0, u, length in tips:
        for _ in range(discs_per_tip):
            d = rng.normal(size=3); d = d / np.linalg.norm(d)
            c = p0 + rng.uniform(0.5, 1.05) * length * u + rng.uniform(0.1, 0.6) * d
            nrm = rng.normal(size=3); nrm = nrm / np.linalg.norm(nrm)
            a, b = _basis(nrm)
            k, rad = int(rng.integers(20, 41)), rng.uniform(0.03, 0.06)
            rr, ph = rad * np.sqrt(rng.uniform(0, 1, k)), rng.uniform(0, 2 * PI, k)
            leaves.append(c + (rr * np.cos(ph))[:, None] * a + (rr * np.sin(ph))[:, None] * b)
        d = rng.normal(size=(scatter_per_tip, 3)); d = d / np.linalg.norm(d, axis=1, keepdims=True)
        leaves.append(p0 + length * u + 0.5 * rng.uniform(0, 1, (scatter_per_tip, 1)) ** (1 / 3) * d)
    wood, leaves = np.concatenate(wood), np.concatenate(leaves)
    xyz = np.concatenate([wood, leaves])
    truth = np.concatenate([np.ones(len(wood), np.uint8), np.zeros(len(leaves), np.uint8)])
    q = xyz / 0.1
    ok = (np.minimum(q - np.floor(q), np.floor(q) + 1.0 - q) > 2e-6).all(1) & (xyz[:, 2] >= 0.0)
    xyz, truth = xyz[ok], truth[ok]
    o = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[o]), np.ones(len(xyz), np.int64), np.ascontiguousarray(truth[o]), total[0]
