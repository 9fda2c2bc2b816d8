"""GPU tests of the leaf-wood separation (csrc/tl_leafwood.hip, util/leafwood.py) against the numpy restatement of
tests/leafwood_restatement.py.

Bounds.  Every flag and every integer column is compared exactly, so is every NaN pattern.  lw_wood_share and lw_wood_top_h are compared to
1e-12 absolute: one division of two integers below 2^53 and one subtraction of two f64 that are the same bits on both sides.  The
restatement is fed the device's own f32 features (tl_eigen_features on the same rows in the same order), so that no decision rests on how
two eigen-solvers round; §21's tests pin the features themselves.  Each test first asserts the restatement's margins: no pair of rows
closer than 1e-10 (relative) to the radius, no floor of a row or of a tree's anchor closer than 1e-6 voxels to a boundary -- a condition
on the inputs."""
import os

import numpy as np
import pytest
import torch

import branches_restatement as br_ref
import features_restatement as feat_ref
import leafwood_cases as cases
import leafwood_restatement as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-12


def gathered(lab):
    """The positions of the rows of labels >= 1 in label order (the stable sort of tree_inventory)."""
    order = np.argsort(lab, kind="stable")
    return order[lab[order] >= 1]


def assert_admissible(margins):
    print("margins:", {k: f"{v:.3e}" for k, v in margins.items()})
    assert margins["radius"] > ref.MIN_RADIUS_MARGIN and min(margins["voxel"], margins["anchor"]) > ref.MIN_FLOOR_MARGIN, margins


def device_features(xyz, lab, radius):
    """f32 [N, 4] (ref.FEATURES) in the input's order: tl_eigen_features on the gathered rows in label order, as the stage runs it."""
    from treelearn_amd.util.features import FEATURE_NAMES
    from treelearn_amd.util.prepare import _eigen_features
    kept = gathered(lab)
    out = np.full((len(lab), 4), np.nan, np.float32)
    if len(kept):
        out[kept] = _eigen_features(xyz[kept], radius, [FEATURE_NAMES.index(k) for k in ref.FEATURES], replace_nan=False).cpu().numpy()
    return out


def device_vote(case):
    from treelearn_amd.util.leafwood import check_params, vote_rounds
    from treelearn_amd.util.prepare import feature_pieces, sorted_cells
    p = check_params(case["p"])
    sx, skeys, perm, ext = sorted_cells(torch.from_numpy(case["xyz"]).cuda(), p["radius"])
    pieces = feature_pieces(skeys)
    if case["reverse"]:
        pieces = pieces.flip(0).contiguous()
    tree = torch.from_numpy(case["tree"]).cuda().index_select(0, perm).to(torch.int32)
    flag = torch.from_numpy(case["flag"]).cuda().index_select(0, perm).contiguous()
    before = flag.clone()
    voted = vote_rounds(sx, skeys, ext, pieces, tree, flag, p)
    assert torch.equal(flag, before)                                      # the input flags are read, never written
    out = torch.empty_like(voted)
    out[perm] = voted
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(cases.VOTE_CASES))
def test_vote_cases_through_the_kernel(name):
    case = cases.VOTE_CASES[name]()
    margin = feat_ref.radius_margin(case["xyz"], case["p"]["radius"])
    print(f"radius margin {margin:.3e}")
    assert margin > ref.MIN_RADIUS_MARGIN
    want = ref.vote(case["xyz"], case["tree"], case["flag"], case["p"])
    if case["want"] is not None:
        assert np.array_equal(want, case["want"])
    got = device_vote(case)
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.flatnonzero(got != want)[:10]


def test_vote_is_the_same_for_any_row_order_and_piece_table():
    case = cases.VOTE_CASES["blob"]()
    q = np.random.default_rng(2).permutation(len(case["flag"]))
    a = device_vote(case)
    b = device_vote(dict(case, xyz=np.ascontiguousarray(case["xyz"][q]), tree=case["tree"][q], flag=case["flag"][q], reverse=True))
    assert np.array_equal(a[q], b)


def test_seed_cases_through_the_kernel():
    from treelearn_amd.util.leafwood import check_params, seed_flags
    feats, want = cases.seed_cases()
    p = check_params(cases.SEED_P)
    assert np.array_equal(ref.seed(feats, p), want)
    got = seed_flags(torch.from_numpy(feats).cuda(), p).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.flatnonzero(got != want)[:10]


def stage(xyz, lab, tree, cfg):
    """The rows in label order and a tree table through leafwood_stage: the wood flags in the input's order and the columns."""
    from treelearn_amd.util import leafwood
    p = leafwood.check_params(cfg)
    kept = gathered(lab)
    marks = []
    dev = leafwood.leafwood_stage(torch.from_numpy(xyz[kept]).cuda(), torch.from_numpy(lab[kept]).cuda(), len(tree), torch.from_numpy(tree).cuda(), p,
                                  marks.append)
    assert tuple(marks) == leafwood.stages_of(p) and not (dev["err"] is not None and int(dev["err"].item()))
    res = leafwood.to_columns({k: dev[k].cpu().numpy() for k in leafwood.HOST_KEYS}, tree[:, 2])
    for k in ("wood", "seed", "voted"):
        res[k] = np.zeros(len(lab), np.uint8)
        res[k][kept] = dev[k].cpu().numpy()
    return res


def assert_leafwood(got, want):
    for k in ("seed", "voted", "wood"):
        if k in got:
            assert got[k].dtype == np.uint8 and np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    for k in ref.LEAFWOOD_COLUMNS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"NaN pattern of {k}"
        if k in ref.LEAFWOOD_INT:
            assert np.array_equal(got[k], want[k]), k
        else:
            ok = ~np.isnan(want[k])
            err = float(np.abs(got[k][ok] - want[k][ok]).max()) if ok.any() else 0.0
            print(f"{k}: max abs difference {err:.3e}")
            assert err <= ATOL, (k, err)


@pytest.mark.parametrize("name", sorted(cases.COMPONENT_CASES))
def test_component_cases_through_the_stage(name):
    case = cases.COMPONENT_CASES[name]()
    want = ref.leafwood(case["xyz"], case["lab"], case["tree"], case["p"], features=device_features(case["xyz"], case["lab"], case["p"]["radius"]))
    assert_admissible(want["margins"])
    assert np.array_equal(want["wood"], case["want"])
    got = stage(case["xyz"], case["lab"], case["tree"], case["p"])
    assert_leafwood(got, want)


def test_a_row_beyond_the_key_raises_like_the_branch_stage():
    from treelearn_amd.util.inventory import tree_inventory
    case = cases.COMPONENT_CASES["threshold"]()
    xyz = case["xyz"].copy(); xyz[3, 0] += 300.0
    with pytest.raises(ValueError, match="2047 branch voxels"):
        tree_inventory(xyz, case["lab"], leafwood=True, leafwood_cfg=case["p"])


@pytest.fixture(scope="module")
def generated():
    """The generated leaf-on tree, its inventory through tree_inventory(..., leafwood=True) and the restatement fed the device's features
    (computed once, never changed)."""
    import inventory_restatement as inv_ref
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab, truth, length = cases.leaf_on_tree()
    base = inv_ref.tree_inventory(xyz, lab)
    tree = np.column_stack([base["x"], base["y"], base["z_low"], base["z_top"]])
    inv = tree_inventory(xyz, lab, leafwood=True, branches=True)
    want = ref.leafwood(xyz, lab, tree, {}, features=device_features(xyz, lab, ref.LEAFWOOD_DEFAULTS["radius"]))
    return dict(xyz=xyz, lab=lab, truth=truth, tree=tree, inv=inv, want=want)


def test_generated_tree(generated):
    from treelearn_amd.util.branches import BRANCH_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS, LEAFWOOD_DEFAULTS
    xyz, lab, truth, inv, want = (generated[k] for k in ("xyz", "lab", "truth", "inv", "want"))
    assert_admissible(want["margins"])
    assert tuple(inv) == COLUMNS + LEAFWOOD_COLUMNS + ("leafwood",) + BRANCH_COLUMNS + ("skeleton",)
    assert {k: v for k, v in inv["leafwood"].items() if k != "wood"} == LEAFWOOD_DEFAULTS
    wood = inv["leafwood"]["wood"]
    tp = int((wood & truth).sum())
    print(f"rows {len(xyz)}, flagged {int(wood.sum())}, recall {tp / truth.sum():.4f}, precision {tp / wood.sum():.4f}, components {inv['lw_components'][0]}")
    assert_leafwood(dict(inv, wood=wood), want)
    # a second run gives the same bits
    again = tree_inventory(xyz, lab, leafwood=True)
    assert again["leafwood"]["wood"].tobytes() == wood.tobytes()
    for k in LEAFWOOD_COLUMNS:
        assert again[k].tobytes() == inv[k].tobytes(), k


def test_generated_tree_rows_permuted(generated):
    """The first 60 000 rows in another order: the vote and the filter do not depend on it; the f32 features do in their last bit (their
    sums run in the order of the sorted array), so the restatement is fed the features of this order."""
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab = generated["xyz"][:60000], generated["lab"][:60000]
    q = np.random.default_rng(5).permutation(len(xyz))
    xq, lq = np.ascontiguousarray(xyz[q]), np.ascontiguousarray(lab[q])
    inv = tree_inventory(xq, lq, leafwood=True)
    tree = np.column_stack([inv["x"], inv["y"], inv["z_low"], inv["z_top"]])
    want = ref.leafwood(xq, lq, tree, {}, features=device_features(xq, lq, ref.LEAFWOOD_DEFAULTS["radius"]))
    assert_admissible(want["margins"])
    assert_leafwood(dict(inv, wood=inv["leafwood"]["wood"]), want)
    plain = tree_inventory(xyz, lab, leafwood=True)
    diff = int((plain["leafwood"]["wood"][q] != inv["leafwood"]["wood"]).sum())
    print(f"rows whose flag differs between the two orders: {diff} of {len(xyz)}")
    assert inv["lw_wood_points"][0] + inv["lw_leaf_points"][0] == len(xyz)


def test_filter_off_changes_no_branch_or_wood_output(generated):
    from treelearn_amd.util.branches import BRANCH_COLUMNS, SKELETON_KEYS
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS
    from treelearn_amd.util.wood import CYLINDER_KEYS, WOOD_COLUMNS
    xyz, lab = generated["xyz"][:60000], generated["lab"][:60000]
    plain = tree_inventory(xyz, lab, wood=True)
    off = tree_inventory(xyz, lab, wood=True, leafwood=True, leafwood_cfg=dict(filter=False))
    assert tuple(plain) == COLUMNS + BRANCH_COLUMNS + ("skeleton",) + WOOD_COLUMNS + ("cylinders",)
    assert tuple(off) == COLUMNS + LEAFWOOD_COLUMNS + ("leafwood",) + BRANCH_COLUMNS + ("skeleton",) + WOOD_COLUMNS + ("cylinders",)
    for k in COLUMNS + BRANCH_COLUMNS + WOOD_COLUMNS:
        assert off[k].tobytes() == plain[k].tobytes(), k
    for k in SKELETON_KEYS:
        assert off["skeleton"][k].tobytes() == plain["skeleton"][k].tobytes(), k
    for k in CYLINDER_KEYS:
        assert off["cylinders"][k].tobytes() == plain["cylinders"][k].tobytes(), k
    on = tree_inventory(xyz, lab, wood=True, leafwood=True)
    assert on["leafwood"]["wood"].tobytes() == off["leafwood"]["wood"].tobytes() and on["skel_voxels"][0] < plain["skel_voxels"][0]
    assert tuple(tree_inventory(xyz, lab)) == COLUMNS


def test_filter_on_the_branch_stage_reads_the_wood_rows(generated):
    """With `filter` the branch integers are those of the branches restatement on the wood rows with the tree table of all rows."""
    xyz, lab, tree, inv, want = (generated[k] for k in ("xyz", "lab", "tree", "inv", "want"))
    rows = want["rows"]
    assert np.array_equal(rows, gathered(lab)[inv["leafwood"]["wood"][gathered(lab)] != 0])
    br = br_ref.branch_structure(xyz[rows], lab[rows], tree[:, 0], tree[:, 1], tree[:, 2])
    print("branch margins:", br["margins"])
    assert min(br["margins"]["voxel"], br["margins"]["z_ref"]) > br_ref.MIN_MARGIN
    for k in br_ref.BRANCH_INT:
        print(k, inv[k].tolist())
        assert np.array_equal(inv[k], br[k]), k
    for k in ("node_start", "parent", "bin", "count"):
        assert np.array_equal(inv["skeleton"][k], br["skeleton"][k]), k


def test_empty_inputs():
    from treelearn_amd import _hip
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS, check_params
    inv = tree_inventory(np.zeros((0, 3)), np.zeros(0, np.int64), leafwood=True)
    assert tuple(inv) == COLUMNS + LEAFWOOD_COLUMNS + ("leafwood",) and all(len(inv[k]) == 0 for k in LEAFWOOD_COLUMNS) and len(inv["leafwood"]["wood"]) == 0
    inv = tree_inventory(np.ones((5, 3)), np.zeros(5, np.int64), leafwood=True)            # rows, no tree
    assert all(len(inv[k]) == 0 for k in LEAFWOOD_COLUMNS) and inv["leafwood"]["wood"].tolist() == [0] * 5
    inv = tree_inventory(np.ones((5, 3)) * np.arange(5)[:, None], np.array([0, 2, -1, 2, 0]), leafwood=True)     # an empty slot, rows of no tree
    assert inv["lw_wood_points"].tolist() == [0, 0] and inv["lw_leaf_points"].tolist() == [0, 2] and np.isnan(inv["lw_wood_share"][0])
    assert inv["lw_wood_share"][1] == 0.0 and np.isnan(inv["lw_wood_top_h"]).all() and inv["leafwood"]["wood"].tolist() == [0] * 5
    # the entry points: nothing to do is TL_OK and leaves the outputs alone
    lib, lp = _hip.lib(), _hip.LeafwoodParams(**dict(check_params(), filter=1))
    buf = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    p, q = _hip.ptr(buf), _hip.ptr(buf[32:])
    import ctypes
    ext = (ctypes.c_int64 * 2)(1, 1)
    assert lib.tl_leafwood_seed(p, 0, lp, p, _hip.stream()) == 0 and lib.tl_leafwood_vote(p, p, 0, ext, p, 0, p, lp, p, q, _hip.stream()) == 0
    assert lib.tl_leafwood_vote(p, p, 5, ext, p, 0, p, lp, p, q, _hip.stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7).all())


def test_segment_forest_and_files(tmp_path):
    """segment_forest(..., leafwood=True) on a 12 m plot of six trees with the pinned-head random model of tests/test_gpu_inventory.py: the
    flags are row-aligned with coords and those of tree_inventory on the centred cloud and the returned labels, and save_results writes
    leafwood.npy and the leafwood columns."""
    import csv
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import make_tile, random_state_dict
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS
    from treelearn_amd.util.segment import MODEL_CFG, save_results, segment_forest
    pts = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])
    sd = random_state_dict(7, channels=32, num_blocks=7)
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    m = TreeLearn(**MODEL_CFG).cuda().eval()
    m.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)
    lcfg = dict(min_component=5, vote_iters=1)
    with torch.no_grad():
        res = segment_forest(pts, m, sample_cfg=dict(stride=1.0), grouping_cfg=cfg, return_type="original", leafwood=True, leafwood_cfg=lcfg)
    inv = res["inventory"]
    assert tuple(inv) == COLUMNS + LEAFWOOD_COLUMNS + ("leafwood",) and len(inv["tree_id"]) == len(res["categories"])
    wood = inv["leafwood"]["wood"]
    assert wood.dtype == np.uint8 and wood.shape == (len(res["coords"]),) and not wood[res["labels"] < 1].any()
    assert inv["leafwood"]["min_component"] == 5 and inv["leafwood"]["vote_iters"] == 1
    assert np.array_equal(np.bincount(res["labels"][wood != 0], minlength=len(inv["tree_id"]) + 1)[1:], inv["lw_wood_points"])
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    direct = tree_inventory(xyz - mean, res["labels"], offset=mean, leafwood=True, leafwood_cfg=lcfg)
    assert direct["leafwood"]["wood"].tobytes() == wood.tobytes()
    for k in LEAFWOOD_COLUMNS:
        assert inv[k].tobytes() == direct[k].tobytes(), k
    print("wood rows", int(wood.sum()), "of", len(wood), "components", inv["lw_components"].tolist())
    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    saved = np.load(tmp_path / "api" / "leafwood.npy")
    assert saved.dtype == np.uint8 and saved.tobytes() == wood.tobytes()
    rows = list(csv.reader(open(tmp_path / "api" / "tree_inventory.csv", newline="")))
    assert rows[0] == list(COLUMNS + LEAFWOOD_COLUMNS) + ["category"] and len(rows) == 1 + len(res["categories"])
