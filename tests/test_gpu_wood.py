"""GPU tests of the cylinder model (csrc/tl_wood.hip, util/wood.py) against the Python restatement of tests/wood_restatement.py.

Bounds.  Every integer is compared exactly: row_node, n, state, wood_nodes_fit, the node table underneath; so is every NaN pattern.  The
radii, rmse, centres, axes, segment lengths and volumes and every float column are compared to 1e-9 absolute, §19's bound and argument:
the formulas are the same, only the order of the f64 sums (at most 10^5 well-scaled terms per node) differs.  Each test first asserts
min(margins) > 1e-6 on the restatement: the float decisions (n against min_points, the radius bounds, rmse, the shift, the pivots, the cap,
the dbh bracket, and the branch rules' own) are then the same on both sides -- a condition on the inputs."""
import csv
import os

import numpy as np
import pytest
import torch

import wood_cases as cases
import wood_restatement as ref
import branches_restatement as br_ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9
FLOAT_COLUMNS = tuple(k for k in ref.WOOD_COLUMNS if k not in ref.WOOD_INT)
INT_CYL = ("node_start", "n", "state")


def _close(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"NaN pattern of {name}"
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{name}: max abs difference {err:.3e}")
    assert err <= ATOL, (name, err)


def _same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=True), name


def assert_admissible(want):
    print("margins:", {k: f"{v:.3e}" for k, v in want["margins"].items()}, "basis lead:", want["basis_lead"])
    assert min(want["margins"].values()) > ref.MIN_MARGIN, want["margins"]


def assert_wood(inv, want):
    from treelearn_amd.util.wood import CYLINDER_KEYS, WOOD_COLUMNS
    assert WOOD_COLUMNS == ref.WOOD_COLUMNS and tuple(inv["cylinders"]) == CYLINDER_KEYS == ref.CYLINDER_KEYS
    for k in br_ref.SKELETON_KEYS:
        _same(k, inv["skeleton"][k], want["skeleton"][k])
    for k in ref.WOOD_INT:
        _same(k, inv[k], want[k])
    for k in CYLINDER_KEYS:
        (_same if k in INT_CYL else _close)(k, inv["cylinders"][k], want["cylinders"][k])
    for k in FLOAT_COLUMNS:
        _close(k, inv[k], want[k])


def gathered(lab):
    """The positions of the rows of labels >= 1 in label order (the stable sort of tree_inventory)."""
    order = np.argsort(lab, kind="stable")
    return order[lab[order] >= 1]


def stage(xyz, lab, tree, branch_cfg, wood_cfg):
    """The rows in label order and a tree table through branch_stage and wood_stage, then the host rules: the branch and wood columns,
    "skeleton", "cylinders" and row_node i32 [m] (in label order)."""
    from treelearn_amd.util import branches, wood
    bp, wp = branches.check_params(branch_cfg), wood.check_params(wood_cfg)
    order = gathered(lab)
    rows = torch.from_numpy(xyz[order]).cuda()
    bdev = branches.branch_stage(rows, torch.from_numpy(lab[order]).cuda(), len(tree), torch.from_numpy(tree).cuda(), bp, lambda name: None)
    marks = []
    wdev = wood.wood_stage(rows, bdev, len(tree), wp, marks.append)
    assert tuple(marks) == wood.STAGES and not (bdev["err"] is not None and int(bdev["err"].item()))
    host = {k: bdev[k].cpu().numpy() for k in ("kstart", "node_start", "xyz", "parent", "bin", "count")}
    res = branches.to_columns(host, tree[:, 2], bp, None)
    res.update(wood.to_columns(res["skeleton"], {k: wdev[k].cpu().numpy() for k in wood.FIT_KEYS}, tree[:, 2], wp, bp, None))
    res["row_node"] = wdev["row_node"].cpu().numpy()
    return res


def restated(case):
    return ref.wood_structure(case["xyz"], case["lab"], case["tree"][:, 0], case["tree"][:, 1], case["tree"][:, 2], branch_cfg=case["branch_cfg"],
                              wood_cfg=case["wood_cfg"])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases_through_the_kernels(name):
    case = cases.CASES[name]()
    want = restated(case)
    assert_admissible(want)
    got = stage(case["xyz"], case["lab"], case["tree"], case["branch_cfg"], case["wood_cfg"])
    _same("row_node", got["row_node"], want["row_node"][gathered(case["lab"])])
    case["check"](got)
    assert_wood(got, want)


@pytest.mark.parametrize("name", ["pole", "pole_tilted", "y_thin_limb", "half_cylinder", "two_trees", "unfitted_root", "no_fit_at_all"])
def test_hand_cases_through_tree_inventory(name):
    """The same rows through tree_inventory(..., wood=True), which takes the positions and z_ref = z_low from the rows themselves, with
    a non-zero offset; the restatement takes them from the inventory's restatement."""
    from treelearn_amd.util.branches import BRANCH_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.wood import WOOD_COLUMNS
    case = cases.CASES[name]()
    off = np.array([1000.5, -2000.25, 50.0])
    want = ref.tree_wood(case["xyz"], case["lab"], offset=off, branch_cfg=case["branch_cfg"], wood_cfg=case["wood_cfg"])
    assert_admissible(want)
    inv = tree_inventory(case["xyz"], case["lab"], offset=off, wood=True, branch_cfg=case["branch_cfg"], wood_cfg=case["wood_cfg"])
    assert tuple(inv) == COLUMNS + BRANCH_COLUMNS + ("skeleton",) + WOOD_COLUMNS + ("cylinders",)
    assert_wood(inv, want)
    ok = inv["cylinders"]["state"] == 1                                   # the centres lie in the frame of the returned coordinates
    assert (np.abs(inv["cylinders"]["centre"][ok] - inv["skeleton"]["xyz"][ok]) < 0.2).all()


def test_two_touching_trees_each_equal_the_tree_alone():
    case = cases.CASES["two_trees"]()
    both = stage(case["xyz"], case["lab"], case["tree"], case["branch_cfg"], case["wood_cfg"])
    for t in (0, 1):
        keep = case["lab"] == t + 1
        alone = stage(case["xyz"][keep], case["lab"][keep], case["tree"], case["branch_cfg"], case["wood_cfg"])
        a, b = both["cylinders"]["node_start"][t], both["cylinders"]["node_start"][t + 1]
        for k in ref.CYLINDER_KEYS[1:]:
            assert alone["cylinders"][k].tobytes() == both["cylinders"][k][a:b].tobytes(), k
        for k in ref.WOOD_COLUMNS:
            assert alone[k][t].tobytes() == both[k][t].tobytes(), k


@pytest.fixture(scope="module")
def generated():
    """The generated stem-and-limb tree with surface rows and the restatement's result (computed once, never changed)."""
    xyz, lab = cases.generated_surface_tree()
    return dict(xyz=xyz, lab=lab, want=ref.tree_wood(xyz, lab))


def test_generated_tree(generated):
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab, want = generated["xyz"], generated["lab"], generated["want"]
    cyl = want["cylinders"]
    print(f"rows {len(xyz)}, voxels {want['skel_voxels'][0]}, nodes {want['skel_nodes'][0]}, states {np.bincount(cyl['state'], minlength=3).tolist()}, "
          f"largest node {cyl['n'].max()} rows, volume {want['wood_volume'][0]:.4f}")
    assert 10000 <= want["skel_voxels"][0] <= 20000 and (cyl["state"] == 1).sum() > 300 and (cyl["state"] == 2).sum() > 20 and cyl["n"].max() > 1000
    assert_admissible(want)
    inv = tree_inventory(xyz, lab, wood=True)
    assert_wood(inv, want)
    row_node = stage(xyz, lab, np.column_stack([inv["x"], inv["y"], inv["z_low"], inv["z_top"]]), None, None)["row_node"]
    _same("row_node", row_node, want["row_node"][gathered(lab)])
    # a second run gives the same bits
    again = tree_inventory(xyz, lab, wood=True)
    for k in ref.WOOD_COLUMNS:
        assert again[k].tobytes() == inv[k].tobytes(), k
    for k in ref.CYLINDER_KEYS:
        assert again["cylinders"][k].tobytes() == inv["cylinders"][k].tobytes(), k
    # the rows in another order: the same integers and states, the floats to 1e-9 (the sums of a node run in another order)
    p = np.random.default_rng(5).permutation(len(xyz))
    inv2 = tree_inventory(xyz[p], lab[p], wood=True)
    assert_wood(inv2, want)
    for k in INT_CYL:
        assert inv2["cylinders"][k].tobytes() == inv["cylinders"][k].tobytes(), k
    assert inv2["wood_nodes_fit"].tobytes() == inv["wood_nodes_fit"].tobytes()


def test_without_the_flag_nothing_changes(generated):
    """wood=False: the keys and the bits of the branches-only call, which are also those the wood call returns underneath."""
    from treelearn_amd.util.branches import BRANCH_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    xyz, lab = generated["xyz"][:60000], generated["lab"][:60000]
    plain = tree_inventory(xyz, lab, branches=True, wood=False)
    assert tuple(plain) == COLUMNS + BRANCH_COLUMNS + ("skeleton",)
    full = tree_inventory(xyz, lab, wood=True)
    for k in COLUMNS + BRANCH_COLUMNS:
        assert full[k].tobytes() == plain[k].tobytes(), k
    for k in plain["skeleton"]:
        assert full["skeleton"][k].tobytes() == plain["skeleton"][k].tobytes(), k
    assert tuple(tree_inventory(xyz, lab)) == COLUMNS


def test_empty_inputs():
    from treelearn_amd import _hip
    from treelearn_amd.util.branches import BRANCH_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.wood import CYLINDER_KEYS, WOOD_COLUMNS, check_params
    inv = tree_inventory(np.zeros((0, 3)), np.zeros(0, np.int64), wood=True)
    assert tuple(inv) == COLUMNS + BRANCH_COLUMNS + ("skeleton",) + WOOD_COLUMNS + ("cylinders",) and all(len(inv[k]) == 0 for k in WOOD_COLUMNS)
    assert tuple(inv["cylinders"]) == CYLINDER_KEYS and inv["cylinders"]["node_start"].tolist() == [0] and inv["cylinders"]["centre"].shape == (0, 3)
    inv = tree_inventory(np.ones((5, 3)), np.zeros(5, np.int64), wood=True)          # rows, no tree
    assert all(len(inv[k]) == 0 for k in WOOD_COLUMNS)
    # the entry points: nothing to do is TL_OK and leaves the outputs alone
    lib, wp = _hip.lib(), _hip.WoodParams(**check_params())
    buf = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    p = _hip.ptr(buf)
    assert lib.tl_wood_row_nodes(p, 0, p, 5, p, p, p, 3, p, _hip.stream()) == 0 and lib.tl_wood_row_nodes(p, 5, p, 5, p, p, p, 0, p, _hip.stream()) == 0
    assert lib.tl_wood_fit(p, 0, p, p, p, p, p, 2, 3, wp, p, p, p, p, p, p, _hip.stream()) == 0
    assert lib.tl_wood_fit(p, 5, p, p, p, p, p, 2, 0, wp, p, p, p, p, p, p, _hip.stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7).all())


def _same_npz(a, b):
    with np.load(a) as f, np.load(b) as g:
        assert set(f.files) == set(g.files) and all(f[k].tobytes() == g[k].tobytes() and f[k].dtype == g[k].dtype for k in g.files)


def test_segment_forest_and_files(tmp_path):
    """segment_forest(..., wood=True) on a 12 m plot of six trees with the pinned-head random model of tests/test_gpu_inventory.py: the
    inventory is that of tree_inventory on the centred cloud and the returned labels, and save_results writes cylinders.npz and the
    wood columns."""
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import make_tile, random_state_dict
    from treelearn_amd.util.branches import BRANCH_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory, write_inventory
    from treelearn_amd.util.segment import MODEL_CFG, save_results, segment_forest
    from treelearn_amd.util.wood import CYLINDER_KEYS, WOOD_COLUMNS, write_cylinders
    pts = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])
    sd = random_state_dict(7, channels=32, num_blocks=7)
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    m = TreeLearn(**MODEL_CFG).cuda().eval()
    m.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)
    wcfg = dict(max_growth=1.2, min_points=6)
    with torch.no_grad():
        res = segment_forest(pts, m, sample_cfg=dict(stride=1.0), grouping_cfg=cfg, return_type="original", wood=True, wood_cfg=wcfg)
    inv = res["inventory"]
    assert tuple(inv) == COLUMNS + BRANCH_COLUMNS + ("skeleton",) + WOOD_COLUMNS + ("cylinders",) and len(inv["tree_id"]) == len(res["categories"])
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    direct = tree_inventory(xyz - mean, res["labels"], offset=mean, wood=True, wood_cfg=wcfg)
    for k in WOOD_COLUMNS:
        assert inv[k].tobytes() == direct[k].tobytes(), k
    for k in CYLINDER_KEYS:
        assert inv["cylinders"][k].tobytes() == direct["cylinders"][k].tobytes(), k
    print("nodes", len(inv["cylinders"]["state"]), "states", np.bincount(inv["cylinders"]["state"], minlength=3).tolist())
    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    _same_npz(tmp_path / "api" / "cylinders.npz", write_cylinders(str(tmp_path / "want.npz"), inv))
    assert (tmp_path / "api" / "skeletons.npz").exists()
    rows = list(csv.reader(open(tmp_path / "api" / "tree_inventory.csv", newline="")))
    assert rows[0] == list(COLUMNS + BRANCH_COLUMNS + WOOD_COLUMNS) + ["category"] and len(rows) == 1 + len(res["categories"])
    want_rows = list(csv.reader(open(write_inventory(str(tmp_path / "want.csv"), inv), newline="")))
    assert [r[:-1] for r in rows[1:]] == want_rows[1:]
