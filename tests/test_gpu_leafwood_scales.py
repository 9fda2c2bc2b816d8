"""GPU tests of the leaf-wood seed over several scales (csrc/tl_leafwood.hip: tl_leafwood_seed_scales,
util/leafwood.leafwood_stage(..., scales=...)) against the numpy restatement of tests/leafwood_scales_restatement.py.

As in tests/test_gpu_leafwood.py every comparison is exact, and the restatement is fed the device's own f32 features (one
tl_eigen_features_scales on the same rows in the same order), so that no decision rests on how two eigen-solvers round."""
import os

import numpy as np
import pytest
import torch

import leafwood_cases as cases
import leafwood_restatement as ref
import leafwood_scales_restatement as sref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-12
SCALES, SCALES_MIN = (0.1, 0.3, 0.4), 2                                   # the recommended point of DESIGN §26


def gathered(lab):
    order = np.argsort(lab, kind="stable")
    return order[lab[order] >= 1]


def assert_admissible(margins):
    print("margins:", {k: f"{v:.3e}" for k, v in margins.items()})
    assert margins["radius"] > ref.MIN_RADIUS_MARGIN and min(margins["voxel"], margins["anchor"]) > ref.MIN_FLOOR_MARGIN, margins


def device_features(xyz, lab, scales):
    """f32 [N, S, 4] (ref.FEATURES) in the input's order: one multi-scale launch on the gathered rows in label order, as the stage runs it."""
    from treelearn_amd.util.prepare import compute_features_scales
    kept = gathered(lab)
    out = np.full((len(lab), len(scales), 4), np.nan, np.float32)
    if len(kept):
        out[kept] = compute_features_scales(xyz[kept], scales, list(ref.FEATURES), replace_nan=False).cpu().numpy()
    return out


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


SHIFTS = (0, 1, 6, 5)


def seed_rows(S):
    """The rows of leafwood_cases.seed_cases at S scales: scale k holds the rows shifted by SHIFTS[k], chosen so that every count 0..S
    occurs (asserted by the caller)."""
    feats, want = cases.seed_cases()
    f = np.stack([np.roll(feats, SHIFTS[k], axis=0) for k in range(S)], 1)
    hold = np.stack([np.roll(want.astype(np.int64), SHIFTS[k]) for k in range(S)], 1).sum(1)
    return np.ascontiguousarray(f), hold


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_seed_cases_over_scales(S):
    from treelearn_amd.util.leafwood import check_params, seed_flags, seed_flags_scales
    p = check_params(cases.SEED_P)
    f, hold = seed_rows(S)
    assert f.shape == (607, S, 4) and set(hold.tolist()) == set(range(S + 1))
    dev = torch.from_numpy(f).cuda()
    for k in range(1, S + 1):
        want, counted = sref.seed_scales(f, p, k)
        assert np.array_equal(counted, hold) and np.array_equal(want, (hold >= k).astype(np.uint8))
        got = seed_flags_scales(dev, p, k).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want), (k, np.flatnonzero(got != want)[:10])
    if S == 1:                                                            # one scale, one vote: the one-scale kernel
        assert np.array_equal(seed_flags_scales(dev, p, 1).cpu().numpy(), seed_flags(dev[:, 0, :].contiguous(), p).cpu().numpy())


def stage(xyz, lab, tree, cfg, **kw):
    """leafwood_stage on the rows in label order: every output of it as numpy, in label order."""
    from treelearn_amd.util import leafwood
    p = leafwood.check_params(cfg)
    kept = gathered(lab)
    marks = []
    dev = leafwood.leafwood_stage(torch.from_numpy(xyz[kept]).cuda(), torch.from_numpy(lab[kept]).cuda(), len(tree), torch.from_numpy(tree).cuda(), p,
                                  marks.append, **kw)
    assert tuple(marks) == leafwood.stages_of(p) and not (dev["err"] is not None and int(dev["err"].item()))
    return {k: v.cpu().numpy() for k, v in dev.items() if v is not None}


def test_scales_none_is_the_call_without_the_argument(monkeypatch):
    from treelearn_amd.util import leafwood, prepare
    c = cases.COMPONENT_CASES["two_touching_trees"]()
    plain = stage(c["xyz"], c["lab"], c["tree"], c["p"])
    monkeypatch.setattr(prepare, "eigen_features_scales_sorted", lambda *a, **k: pytest.fail("the multi-scale kernel was launched"))
    monkeypatch.setattr(leafwood, "seed_flags_scales", lambda *a, **k: pytest.fail("the multi-scale seed was launched"))
    for kw in (dict(scales=None), dict(scales=leafwood.check_scales())):
        got = stage(c["xyz"], c["lab"], c["tree"], c["p"], **kw)
        assert sorted(got) == sorted(plain)
        for k in plain:
            assert got[k].dtype == plain[k].dtype and got[k].tobytes() == plain[k].tobytes(), k


@pytest.fixture(scope="module")
def generated():
    """The generated leaf-on tree, its inventory at the recommended scales and the restatement fed the device's features (computed once)."""
    import inventory_restatement as inv_ref
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab, truth, length = cases.leaf_on_tree()
    base = inv_ref.tree_inventory(xyz, lab)
    tree = np.column_stack([base["x"], base["y"], base["z_low"], base["z_top"]])
    inv = tree_inventory(xyz, lab, leafwood=True, leafwood_scales=SCALES, leafwood_scales_min=SCALES_MIN)
    want = sref.leafwood_scales(xyz, lab, tree, {}, SCALES, SCALES_MIN, features=device_features(xyz, lab, SCALES))
    return dict(xyz=xyz, lab=lab, truth=truth, tree=tree, inv=inv, want=want)


def test_generated_tree(generated):
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS, LEAFWOOD_DEFAULTS
    xyz, lab, truth, inv, want = (generated[k] for k in ("xyz", "lab", "truth", "inv", "want"))
    assert_admissible(want["margins"])
    assert tuple(inv) == COLUMNS + LEAFWOOD_COLUMNS + ("leafwood",)
    assert {k: v for k, v in inv["leafwood"].items() if k != "wood"} == dict(LEAFWOOD_DEFAULTS, scales=list(SCALES), scales_min=SCALES_MIN)
    wood = inv["leafwood"]["wood"]
    tp = int((wood & truth).sum())
    print(f"rows {len(xyz)}, flagged {int(wood.sum())}, recall {tp / truth.sum():.4f}, precision {tp / wood.sum():.4f}, components {inv['lw_components'][0]}")
    assert_leafwood(dict(inv, wood=wood), want)
    # the stage's seed and voted flags too, not only what survives the filter
    got = stage(xyz, lab, generated["tree"], {}, scales=dict(scales=list(SCALES), scales_min=SCALES_MIN))
    kept = gathered(lab)
    for k in ("seed", "voted", "wood"):
        assert np.array_equal(got[k], want[k][kept]), (k, int((got[k] != want[k][kept]).sum()))
    # the one-scale call differs, and a second run gives the same bits
    assert tree_inventory(xyz, lab, leafwood=True)["leafwood"]["wood"].tobytes() != wood.tobytes()
    again = tree_inventory(xyz, lab, leafwood=True, leafwood_scales=SCALES, leafwood_scales_min=SCALES_MIN)
    assert again["leafwood"]["wood"].tobytes() == wood.tobytes()
    for k in LEAFWOOD_COLUMNS:
        assert again[k].tobytes() == inv[k].tobytes(), k


def test_largest_scale_equal_to_the_radius_shares_the_sort(generated, monkeypatch):
    """scales whose largest is the vote's radius: one cell sort serves both, and the result is the restatement's."""
    from treelearn_amd.util import inventory, prepare
    xyz, lab = generated["xyz"][:40000], generated["lab"][:40000]
    calls = []
    real = prepare.sorted_cells
    monkeypatch.setattr(prepare, "sorted_cells", lambda x, r: (calls.append(r), real(x, r))[1])
    inv = inventory.tree_inventory(xyz, lab, leafwood=True, leafwood_scales=(0.1, 0.2), leafwood_scales_min=1)
    assert calls == [0.2]
    calls.clear()
    inventory.tree_inventory(xyz, lab, leafwood=True, leafwood_scales=(0.1, 0.3), leafwood_scales_min=1)
    assert calls == [0.3, 0.2]
    monkeypatch.undo()
    tree = np.column_stack([inv["x"], inv["y"], inv["z_low"], inv["z_top"]])
    want = sref.leafwood_scales(xyz, lab, tree, {}, (0.1, 0.2), 1, features=device_features(xyz, lab, (0.1, 0.2)))
    assert_admissible(want["margins"])
    assert_leafwood(dict(inv, wood=inv["leafwood"]["wood"]), want)


def test_generated_tree_rows_permuted(generated):
    """The first 60 000 rows in another order: the vote and the filter do not depend on it; the f32 features do in their last bit (their
    sums run in the order of the sorted array), so the restatement is fed the features of this order."""
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab = generated["xyz"][:60000], generated["lab"][:60000]
    q = np.random.default_rng(5).permutation(len(xyz))
    xq, lq = np.ascontiguousarray(xyz[q]), np.ascontiguousarray(lab[q])
    kw = dict(leafwood=True, leafwood_scales=SCALES, leafwood_scales_min=SCALES_MIN)
    inv = tree_inventory(xq, lq, **kw)
    tree = np.column_stack([inv["x"], inv["y"], inv["z_low"], inv["z_top"]])
    want = sref.leafwood_scales(xq, lq, tree, {}, SCALES, SCALES_MIN, features=device_features(xq, lq, SCALES))
    assert_admissible(want["margins"])
    assert_leafwood(dict(inv, wood=inv["leafwood"]["wood"]), want)
    # fed the permuted order's seed, the vote and the components of the plain order are the same bits
    plain = tree_inventory(xyz, lab, **kw)
    diff = int((plain["leafwood"]["wood"][q] != inv["leafwood"]["wood"]).sum())
    print(f"rows whose flag differs between the two orders: {diff} of {len(xyz)}")
    assert inv["lw_wood_points"][0] + inv["lw_leaf_points"][0] == len(xyz)


def test_bad_scales_are_refused_before_any_gpu_work(monkeypatch):
    from treelearn_amd import _hip
    from treelearn_amd.util.inventory import cloud_inventory, tree_inventory
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was touched"))
    pts = np.zeros((10, 4)); pts[:, 3] = 1
    for kw in (dict(leafwood_scales=(0.4, 0.2)), dict(leafwood_scales=(0.2, 0.4), leafwood_scales_min=3), dict(leafwood_scales_min=2),
               dict(leafwood_scales=(0.1, 0.2, 0.3, 0.4, 0.5))):
        with pytest.raises(ValueError):
            tree_inventory(pts[:, :3], pts[:, 3].astype(np.int64), leafwood=True, **kw)
        with pytest.raises(ValueError):
            cloud_inventory(pts, leafwood=True, **kw)


def test_segment_forest_key():
    """segment_forest hands leafwood_scales / leafwood_scales_min to the inventory: checked before any model runs, recorded in the dict."""
    from treelearn_amd.util.segment import segment_forest

    class Model:
        use_feats, dim_feat = True, 1

    with pytest.raises(ValueError, match="scales"):
        segment_forest(np.zeros((10, 3)), Model(), leafwood=True, leafwood_scales=(0.4, 0.2))
    with pytest.raises(ValueError, match="scales_min"):
        segment_forest(np.zeros((10, 3)), Model(), leafwood=True, leafwood_scales=(0.2, 0.4), leafwood_scales_min=3)
    # the 12 m plot of six trees and the pinned-head random model of tests/test_gpu_leafwood.py
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import make_tile, random_state_dict
    from treelearn_amd.util.inventory import tree_inventory
    from treelearn_amd.util.leafwood import LEAFWOOD_COLUMNS
    from treelearn_amd.util.segment import MODEL_CFG
    pts = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])
    sd = random_state_dict(7, channels=32, num_blocks=7)
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    m = TreeLearn(**MODEL_CFG).cuda().eval()
    m.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)
    kw = dict(leafwood=True, leafwood_cfg=dict(min_component=5, vote_iters=1), leafwood_scales=(0.1, 0.2, 0.4), leafwood_scales_min=2)
    with torch.no_grad():
        res = segment_forest(pts, m, sample_cfg=dict(stride=1.0), grouping_cfg=cfg, return_type="original", **kw)
    lw = res["inventory"]["leafwood"]
    assert lw["scales"] == [0.1, 0.2, 0.4] and lw["scales_min"] == 2 and lw["min_component"] == 5
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    direct = tree_inventory(xyz - mean, res["labels"], offset=mean, **kw)
    assert direct["leafwood"]["wood"].tobytes() == lw["wood"].tobytes() and lw["wood"].any()
    for k in LEAFWOOD_COLUMNS:
        assert res["inventory"][k].tobytes() == direct[k].tobytes(), k
    one = tree_inventory(xyz - mean, res["labels"], offset=mean, leafwood=True, leafwood_cfg=kw["leafwood_cfg"])
    assert "scales" not in one["leafwood"] and one["leafwood"]["wood"].tobytes() != lw["wood"].tobytes()
