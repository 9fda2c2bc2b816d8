"""Host tests of the leaf-wood separation (util/leafwood.py; no GPU): the hand cases through the numpy restatement, check_params on
every constraint, the argument parsers of the five command lines, the files, the header section and the exported symbols, the entry
points' argument checks on host memory, to_columns against the restatement's columns, and the generated leaf-on tree: recall and precision
of the wood flag and what the filter does to the skeleton's length."""
import argparse
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import leafwood_cases as cases
import leafwood_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tl_leafwood_seed": 5, "tl_leafwood_vote": 11}
# The generated leaf-on tree (leafwood_cases.leaf_on_tree: 175 421 rows, 118 144 of them wood) through the restatement at the default
# parameters, on the host: recall 0.8193, precision 0.7284 (DESIGN §25 holds the figures and the thresholds tried).  Asserted: the measured
# figures rounded down to two decimals; the generator is seeded, they do not move.
RECALL_MIN, PRECISION_MIN = 0.81, 0.72


@pytest.mark.parametrize("name", sorted(cases.VOTE_CASES))
def test_vote_cases_through_the_restatement(name):
    c = cases.VOTE_CASES[name]()
    got = ref.vote(c["xyz"], c["tree"], c["flag"], c["p"])
    if c["want"] is not None:
        assert np.array_equal(got, c["want"])
    assert got.dtype == np.uint8 and len(got) == len(c["flag"])
    import features_restatement as feat_ref
    assert feat_ref.radius_margin(c["xyz"], c["p"]["radius"]) > ref.MIN_RADIUS_MARGIN


def test_vote_checkerboard_is_not_the_update_in_place():
    c = cases.VOTE_CASES["checkerboard_3"]()
    assert not np.array_equal(ref.vote(c["xyz"], c["tree"], c["flag"], c["p"]), cases.in_place(c["flag"], 60, 3))


def test_vote_does_not_depend_on_the_row_order():
    c = cases.VOTE_CASES["blob"]()
    q = np.random.default_rng(1).permutation(len(c["flag"]))
    a, b = ref.vote(c["xyz"], c["tree"], c["flag"], c["p"]), ref.vote(c["xyz"][q], c["tree"][q], c["flag"][q], c["p"])
    assert np.array_equal(a[q], b)


def test_seed_cases_through_the_restatement():
    feats, want = cases.seed_cases()
    assert np.array_equal(ref.seed(feats, dict(ref.LEAFWOOD_DEFAULTS, **cases.SEED_P)), want)
    assert np.float64(np.float32(0.7)) < 0.7 and np.float64(np.float32(0.6)) > 0.6          # what the threshold rows rest on


@pytest.mark.parametrize("name", sorted(cases.COMPONENT_CASES))
def test_component_cases_through_the_restatement(name):
    c = cases.COMPONENT_CASES[name]()
    got = ref.leafwood(c["xyz"], c["lab"], c["tree"], c["p"])
    assert got["seed"].all() and np.array_equal(got["voted"], got["seed"])                 # every row is a seed; no vote
    assert np.array_equal(got["wood"], c["want"])
    m = got["margins"]
    assert m["radius"] > ref.MIN_RADIUS_MARGIN and min(m["voxel"], m["anchor"]) > ref.MIN_FLOOR_MARGIN, m
    for t in range(len(c["tree"])):
        sel = c["lab"] == t + 1
        assert got["lw_wood_points"][t] == c["want"][sel].sum() and got["lw_leaf_points"][t] == (1 - c["want"][sel]).sum()
        assert np.isnan(got["lw_wood_share"][t]) == (sel.sum() == 0)
    rows = got["rows"]
    assert np.array_equal(np.sort(rows), np.flatnonzero(got["wood"])) and (np.diff(c["lab"][rows]) >= 0).all()


def test_restatement_raises_like_the_branch_stage():
    c = cases.COMPONENT_CASES["threshold"]()
    xyz = c["xyz"].copy(); xyz[3, 0] += 300.0                                             # 3 000 voxels from the tree's position
    with pytest.raises(ValueError):
        ref.leafwood(xyz, c["lab"], c["tree"], c["p"], features=np.ones((len(xyz), 4), np.float32))


def test_check_params():
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS, LEAFWOOD_DEFAULTS, LEAFWOOD_INT_COLUMNS, check_params, stages_of
    assert LEAFWOOD_DEFAULTS == ref.LEAFWOOD_DEFAULTS and LEAFWOOD_COLUMNS == ref.LEAFWOOD_COLUMNS and LEAFWOOD_INT_COLUMNS == ref.LEAFWOOD_INT
    assert all(k.startswith("lw_") for k in LEAFWOOD_COLUMNS)
    p = check_params()
    assert p == LEAFWOOD_DEFAULTS and isinstance(p["filter"], bool) and isinstance(p["vote_iters"], int) and isinstance(p["radius"], float)
    assert check_params(dict(radius=0.3), vote_iters=0)["radius"] == 0.3 and check_params(radius=None) == p
    assert check_params(vote_iters=8.0)["vote_iters"] == 8 and check_params(filter=False)["filter"] is False
    for good in (dict(min_neighbours=3), dict(linearity_min=0), dict(linearity_min=1), dict(planarity_min=0.0), dict(verticality_min=1.0), dict(vote_iters=0),
                 dict(vote_percent=1), dict(vote_percent=100), dict(reach=2), dict(min_component=1), dict(voxel=1e-3)):
        check_params(good)
    assert len(stages_of(check_params(vote_iters=0))) == 5 and len(stages_of(check_params(vote_iters=8))) == 13
    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(min_neighbours=2), dict(min_neighbours=3.5), dict(min_neighbours=nan),
                dict(linearity_min=-0.01), dict(linearity_min=1.01), dict(linearity_min=nan), dict(planarity_min=-1), dict(planarity_min=2), dict(planarity_min=nan),
                dict(verticality_min=-0.5), dict(verticality_min=1.5), dict(verticality_min=nan), dict(vote_iters=-1), dict(vote_iters=9), dict(vote_iters=1.5),
                dict(vote_iters=nan), dict(vote_percent=0), dict(vote_percent=101), dict(vote_percent=50.5), dict(vote_percent=nan), dict(voxel=0), dict(voxel=nan),
                dict(voxel=inf), dict(reach=0), dict(reach=3), dict(reach=nan), dict(min_component=0), dict(min_component=nan), dict(min_component=2.5),
                dict(filter=1), dict(filter="yes"), dict(filter=nan), dict(radius=True), dict(radius="0.2"), dict(nothing=1)):
        with pytest.raises(ValueError):
            check_params(bad)


def test_argument_parsers(tmp_path):
    from treelearn_amd.util import branches, inventory, leafwood, segment, wood
    ap = argparse.ArgumentParser()
    leafwood.add_arguments(ap)
    leafwood.add_arguments(ap)                                            # a second call adds nothing
    assert leafwood.params_of(ap.parse_args([])) == leafwood.LEAFWOOD_DEFAULTS
    a = ap.parse_args(["--leafwood-radius", "0.3", "--leafwood-min-neighbours", "8", "--leafwood-linearity-min", "0.8", "--leafwood-planarity-min", "0.5",
                       "--leafwood-verticality-min", "0.6", "--leafwood-vote-iters", "3", "--leafwood-vote-percent", "40", "--leafwood-voxel", "0.05",
                       "--leafwood-reach", "2", "--leafwood-min-component", "10", "--leafwood-filter", "0"])
    assert leafwood.params_of(a) == dict(radius=0.3, min_neighbours=8, linearity_min=0.8, planarity_min=0.5, verticality_min=0.6, vote_iters=3, vote_percent=40,
                                         voxel=0.05, reach=2, min_component=10, filter=False)
    assert leafwood.check_params(leafwood.params_of(a))["filter"] is False
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 4)))
    # a parameter outside its constraint ends every command line before any GPU work, and nothing is written
    with pytest.raises(SystemExit):
        leafwood.main(["--forest", str(forest), "--out", str(tmp_path / "o.npy"), "--leafwood-vote-iters", "9"])
    with pytest.raises(SystemExit):
        leafwood.main(["--forest", str(forest), "--out", str(tmp_path / "o.npy"), "--leafwood-filter", "2"])
    with pytest.raises(SystemExit):
        leafwood.main(["--forest", str(forest)])
    with pytest.raises(SystemExit):
        branches.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--leafwood", "--leafwood-reach", "3"])
    with pytest.raises(SystemExit):
        wood.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--leafwood", "--leafwood-radius", "0"])
    with pytest.raises(SystemExit):
        inventory.main(["--forest", str(forest), "--out", str(tmp_path / "o.csv"), "--leafwood", "--leafwood-vote-percent", "0"])
    (tmp_path / "w.pth").write_bytes(b"")
    common = ["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    with pytest.raises(SystemExit):
        segment.parse_args(common + ["--leafwood", "--leafwood-min-component", "0"])
    a = segment.parse_args(common + ["--leafwood", "--leafwood-vote-iters", "4", "--leafwood-filter", "0"])
    assert a.leafwood and not a.branches and not a.wood and leafwood.params_of(a) == dict(leafwood.LEAFWOOD_DEFAULTS, vote_iters=4, filter=False)
    assert not segment.parse_args(common).leafwood and leafwood.params_of(segment.parse_args(common)) == leafwood.LEAFWOOD_DEFAULTS
    assert not (tmp_path / "o.npz").exists() and not (tmp_path / "o.csv").exists() and not (tmp_path / "o.npy").exists()
    with pytest.raises(ValueError):                                       # the API checks before any GPU work too
        segment.segment_forest(None, None, leafwood=True, leafwood_cfg=dict(reach=3))
    with pytest.raises(ValueError):
        inventory.tree_inventory(None, None, leafwood=True, leafwood_cfg=dict(vote_percent=0))
    with pytest.raises(ValueError):
        inventory.cloud_inventory(np.zeros((1, 4)), leafwood=True, leafwood_cfg=dict(nothing=1))


def _inventory_of(case):
    """An inventory dict as tree_inventory(..., leafwood=True) returns it, from the restatements (no GPU)."""
    import inventory_restatement as inv_ref
    res = dict(inv_ref.tree_inventory(case["xyz"], case["lab"]))
    got = ref.leafwood(case["xyz"], case["lab"], case["tree"], case["p"])
    res.update({k: got[k] for k in ref.LEAFWOOD_COLUMNS})
    res["leafwood"] = dict(ref.LEAFWOOD_DEFAULTS, **case["p"], wood=got["wood"])
    return res


def test_write_inventory_column_order(tmp_path):
    from treelearn_amd.util.inventory import COLUMNS, write_inventory
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS, LEAFWOOD_INT_COLUMNS
    inv = _inventory_of(cases.COMPONENT_CASES["no_position_and_empty_slots"]())
    rows = list(csv.reader(open(write_inventory(str(tmp_path / "w.csv"), inv), newline="")))
    assert rows[0] == list(COLUMNS + LEAFWOOD_COLUMNS) and len(rows) == 6
    at = len(COLUMNS)
    for i, row in enumerate(rows[1:]):
        for k, cell in zip(LEAFWOOD_COLUMNS, row[at:]):
            if k in LEAFWOOD_INT_COLUMNS:
                assert cell == str(int(inv[k][i])), k
            else:
                assert cell == "nan" if np.isnan(inv[k][i]) else float(cell) == inv[k][i], k
    assert [r[at] for r in rows[1:]] == ["20", "0", "0", "0", "88"]
    # between the crown and the branch group
    from treelearn_amd.util.branches import BRANCH_COLUMNS
    from treelearn_amd.util.crown import CROWN_COLUMNS
    wide = dict(inv, **{k: np.zeros(5) for k in CROWN_COLUMNS + BRANCH_COLUMNS})
    assert list(csv.reader(open(write_inventory(str(tmp_path / "x.csv"), wide), newline="")))[0] == list(COLUMNS + CROWN_COLUMNS + LEAFWOOD_COLUMNS + BRANCH_COLUMNS)
    # without all five: the columns of before, the same bytes
    plain = {k: inv[k] for k in COLUMNS}
    partial = dict(plain, lw_wood_share=inv["lw_wood_share"], leafwood=inv["leafwood"])
    assert open(write_inventory(str(tmp_path / "p.csv"), partial), "rb").read() == open(write_inventory(str(tmp_path / "q.csv"), plain), "rb").read()


def test_write_leafwood_round_trip(tmp_path):
    from treelearn_amd.util.leafwood import write_leafwood
    inv = _inventory_of(cases.COMPONENT_CASES["threshold"]())
    got = np.load(write_leafwood(str(tmp_path / "l.npy"), inv))
    assert got.dtype == np.uint8 and got.tobytes() == inv["leafwood"]["wood"].tobytes()
    with pytest.raises(ValueError):
        write_leafwood(str(tmp_path / "none.npy"), {k: v for k, v in inv.items() if k != "leafwood"})


@pytest.mark.parametrize("name", sorted(cases.COMPONENT_CASES))
def test_to_columns_against_the_restatement(name):
    """util.leafwood.to_columns on the per-tree sums the device part hands over, here taken from the restatement's flags."""
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS, to_columns
    c = cases.COMPONENT_CASES[name]()
    want = ref.leafwood(c["xyz"], c["lab"], c["tree"], c["p"])
    T = len(c["tree"])
    host = dict(wood_points=np.zeros(T, np.int64), rows=np.zeros(T, np.int64), components=want["lw_components"].copy(), top_z=np.full(T, -np.inf))
    for t in range(T):
        sel = c["lab"] == t + 1
        host["rows"][t], host["wood_points"][t] = sel.sum(), want["wood"][sel].sum()
        if want["wood"][sel].any():
            host["top_z"][t] = c["xyz"][sel][want["wood"][sel] != 0, 2].max()
    got = to_columns(host, c["tree"][:, 2])
    assert tuple(got) == LEAFWOOD_COLUMNS
    for k in LEAFWOOD_COLUMNS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k


def test_header_declares_and_library_exports_the_entry_points():
    """The two symbols are declared in a section of their own, bound with matching arity and exported; they refuse nulls, misaligned
    pointers, sizes and bad parameters before anything else, and return TL_OK without a launch for nothing to do (host memory: no GPU)."""
    from treelearn_amd import _hip, build as b
    from treelearn_amd.util.leafwood import check_params
    header = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    assert "csrc/tl_leafwood.hip, DESIGN §25" in header and "typedef struct tl_leafwood_params" in header
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES[name][1]), name
    L = ctypes.CDLL(b.build(verbose=False))
    assert all(hasattr(L, name) for name in ENTRY_POINTS)
    assert [f[0] for f in _hip.LeafwoodParams._fields_] == ["radius", "linearity_min", "planarity_min", "verticality_min", "voxel", "min_neighbours",
                                                           "vote_iters", "vote_percent", "reach", "min_component", "filter"]
    assert ctypes.sizeof(_hip.LeafwoodParams) == 88
    lib = _hip.lib()

    def params(**kw):
        return _hip.LeafwoodParams(**{**check_params(), "filter": 1, **kw})
    good = params()
    buf = (ctypes.c_char * 1024)()                                       # host memory: only its address and alignment are looked at
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    ext = (ctypes.c_int64 * 2)(3, 4)
    p, odd8, odd4, odd2, q = (ctypes.c_void_p(base + k) for k in (0, 8, 4, 2, 256))
    seed = lambda *a: lib.tl_leafwood_seed(*a, None)                      # noqa: E731
    vote = lambda *a: lib.tl_leafwood_vote(*a, None)                      # noqa: E731
    ok, bad = _hip.TL_OK, _hip.TL_ERR_ARG
    # nothing to do, found out after the argument checks and without a launch
    assert seed(p, 0, good, p) == ok and vote(p, p, 0, ext, p, 0, p, good, p, q) == ok and vote(p, p, 0, ext, p, 0, p, good, p, None) == ok
    # nulls, misaligned pointers, sizes
    assert seed(None, 0, good, p) == bad and seed(p, 0, good, None) == bad and seed(p, 0, None, p) == bad and seed(p, -1, good, p) == bad
    assert seed(odd8, 0, good, p) == bad and seed(odd4, 0, good, p) == bad and seed(p, 0, good, odd2) == ok
    for k in (0, 1, 3, 4, 6, 8):                                          # xyz, keys, extent2, pieces, tag, flag_out
        a = [p, p, 0, ext, p, 0, p, good, p, q]
        a[k] = None
        assert vote(*a) == bad, k
    for k, ptr in ((0, odd4), (1, odd4), (4, odd4), (6, odd2), (9, odd2)):
        a = [p, p, 0, ext, p, 0, p, good, p, q]
        a[k] = ptr
        assert vote(*a) == bad, k
    assert vote(p, p, 0, ext, p, 0, odd4, good, odd2, ctypes.c_void_p(base + 12)) == ok        # i32 tags on 4 bytes, the u8 flags anywhere
    assert vote(p, p, 0, ext, p, 0, p, good, p, p) == bad                 # tag_out must not be tag
    assert vote(p, p, -1, ext, p, 0, p, good, p, q) == bad and vote(p, p, 0, ext, p, -1, p, good, p, q) == bad
    assert vote(p, p, 0, ext, p, 1, p, good, p, q) == bad and vote(p, p, 1 << 40, ext, p, 1 << 31, p, good, p, q) == bad
    assert vote(p, p, 0, (ctypes.c_int64 * 2)(-1, 4), p, 0, p, good, p, q) == bad and vote(p, p, 0, (ctypes.c_int64 * 2)(3, 1 << 21), p, 0, p, good, p, q) == bad
    assert vote(p, p, 0, ext, p, 0, p, None, p, q) == bad
    nan, inf = float("nan"), float("inf")
    for wrong in (dict(radius=0.0), dict(radius=nan), dict(radius=inf), dict(radius=-1.0), dict(voxel=0.0), dict(voxel=nan), dict(voxel=inf), dict(min_neighbours=2),
                  dict(linearity_min=-0.1), dict(linearity_min=1.1), dict(linearity_min=nan), dict(planarity_min=-0.1), dict(planarity_min=1.1),
                  dict(planarity_min=nan), dict(verticality_min=-0.1), dict(verticality_min=1.1), dict(verticality_min=nan), dict(vote_iters=-1),
                  dict(vote_iters=9), dict(vote_percent=0), dict(vote_percent=101), dict(reach=0), dict(reach=3), dict(min_component=0)):
        with pytest.raises(ValueError):
            check_params(wrong)                                           # the host check and the library's agree
        assert seed(p, 0, params(**wrong), p) == bad and vote(p, p, 0, ext, p, 0, p, params(**wrong), p, q) == bad, wrong
    assert seed(p, 0, params(filter=2), p) == bad and seed(p, 0, params(filter=0), p) == ok


@pytest.fixture(scope="module")
def leaf_on():
    """The generated leaf-on tree, its tree table from the inventory's restatement and the restatement's flags (computed once)."""
    import inventory_restatement as inv_ref
    xyz, lab, truth, length = cases.leaf_on_tree()
    base = inv_ref.tree_inventory(xyz, lab)
    tree = np.column_stack([base["x"], base["y"], base["z_low"], base["z_top"]])
    return dict(xyz=xyz, lab=lab, truth=truth, length=length, tree=tree, got=ref.leafwood(xyz, lab, tree, {}))


def test_generated_leaf_on_tree_recall_and_precision(leaf_on):
    truth, wood, m = leaf_on["truth"], leaf_on["got"]["wood"], leaf_on["got"]["margins"]
    assert 150000 <= len(truth) <= 400000 and 0.5 < truth.mean() < 0.8
    assert m["radius"] > ref.MIN_RADIUS_MARGIN and min(m["voxel"], m["anchor"]) > ref.MIN_FLOOR_MARGIN, m
    tp = int((wood & truth).sum())
    recall, precision = tp / int(truth.sum()), tp / int(wood.sum())
    print(f"rows {len(truth)}, wood {int(truth.sum())}, flagged {int(wood.sum())}, recall {recall:.4f}, precision {precision:.4f}, "
          f"components {leaf_on['got']['lw_components'][0]}, margins {m}")
    assert recall >= RECALL_MIN and precision >= PRECISION_MIN


def test_generated_leaf_on_tree_skeleton_length(leaf_on):
    """skel_length of the branches restatement on the wood rows lies strictly closer to the summed length of the generator's limbs than
    skel_length on all rows (the tree table is that of all rows both times)."""
    import branches_restatement as br_ref
    xyz, lab, tree, rows = leaf_on["xyz"], leaf_on["lab"], leaf_on["tree"], leaf_on["got"]["rows"]
    every = br_ref.branch_structure(xyz, lab, tree[:, 0], tree[:, 1], tree[:, 2])["skel_length"][0]
    wood = br_ref.branch_structure(xyz[rows], lab[rows], tree[:, 0], tree[:, 1], tree[:, 2])["skel_length"][0]
    print(f"true limb length {leaf_on['length']:.3f} m, skel_length on all rows {every:.3f} m, on the wood rows {wood:.3f} m")
    assert abs(wood - leaf_on["length"]) < abs(every - leaf_on["length"])
