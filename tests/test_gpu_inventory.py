"""GPU tests of the per-tree inventory (csrc/tl_inventory.hip, util/inventory.py) against the numpy restatement of
tests/inventory_restatement.py.

Bounds.  n_points, z_low, z_top, height, dbh_n, crown_cells, crown_area (and crown_diameter, the same numpy expression of the same
count) and the NaN pattern are compared exactly: ranks, comparisons and integer counts do not depend on the order of a sum.  x, y, z,
dbh, dbh_x, dbh_y, dbh_rmse are compared to 1e-9 absolute: the formulas are identical and only the order of the f64 sums differs
(<= 1e5 terms of magnitude <= 1e2 at 1.1e-16 each); the stems of the test clouds are full circles, so the 3 x 3 system is benign."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inventory_cases as cases
import inventory_restatement as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("tree_id", "n_points", "z_low", "z_top", "height", "dbh_n", "crown_cells", "crown_area", "crown_diameter")
CLOSE = ("x", "y", "z", "dbh", "dbh_x", "dbh_y", "dbh_rmse")
ATOL = 1e-9


def assert_matches(inv, want, exact=EXACT, close=CLOSE):
    assert tuple(inv) == ref.COLUMNS
    for k in exact:
        assert inv[k].dtype == want[k].dtype and np.array_equal(inv[k], want[k], equal_nan=True), k
    for k in close:
        assert np.array_equal(np.isnan(inv[k]), np.isnan(want[k])), f"NaN pattern of {k}"
        ok = ~np.isnan(want[k])
        err = np.abs(inv[k][ok] - want[k][ok]).max() if ok.any() else 0.0
        print(f"{k}: max abs difference {err:.3e}")
        assert err <= ATOL, (k, err)


def _tree(rng, n, cx, cy, z0):
    """n rows of a tree at (cx, cy): a stem of full circles (random angles, radius 0.1 .. 0.3) from the ground to 2 m and a crown blob
    above it, z quantised to 0.1 so that ranks hit ties."""
    ns = n if n < 40 else int(0.4 * n) if n < 1000 else int(0.2 * n)
    a = rng.uniform(0, 2 * np.pi, ns)
    r = rng.uniform(0.1, 0.3)
    stem = np.column_stack([cx + r * np.cos(a), cy + r * np.sin(a), z0 + rng.uniform(0.0, 2.0, ns)])
    nc = n - ns
    crown = np.column_stack([cx + rng.normal(0, 1.5, nc), cy + rng.normal(0, 1.5, nc), z0 + rng.uniform(2.0, 14.0, nc)])
    p = np.concatenate([stem, crown])
    p[:, 2] = np.round(p[:, 2] * 10) / 10
    return p


SIZES = (1, 4, 11, 12, 13, 255, 256, 257, 70001)


def _edge_cloud():
    """Trees of SIZES rows under the labels 1..10 without 6 (a gap), plus rows labelled 0 and -1, shuffled; coordinates centred."""
    rng = np.random.default_rng(11)
    ids = [t for t in range(1, 11) if t != 6]
    rows, lab = [], []
    for k, (t, n) in enumerate(zip(ids, SIZES)):
        rows.append(_tree(rng, n, -32.0 + 8.0 * k + rng.uniform(-1, 1), rng.uniform(-20, 20), rng.uniform(-3, 3)))
        lab.append(np.full(n, t))
    for other in (0, -1):
        rows.append(rng.uniform(-40, 40, (5000, 3)))
        lab.append(np.full(5000, other))
    xyz, lab = np.concatenate(rows), np.concatenate(lab).astype(np.int64)
    p = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[p]), np.ascontiguousarray(lab[p])


@pytest.fixture(scope="module")
def edge_cloud():
    xyz, lab = _edge_cloud()
    x32 = xyz.astype(np.float32)
    return dict(lab=lab, f64=xyz, f32=x32, want64=ref.tree_inventory(xyz, lab), want32=ref.tree_inventory(x32, lab))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("stride", [3, 4])
def test_edge_sizes(edge_cloud, dtype, stride):
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab, want = edge_cloud[dtype], edge_cloud["lab"], edge_cloud["want" + dtype[1:]]
    assert want["n_points"].tolist() == list(SIZES[:5]) + [0] + list(SIZES[5:])
    assert np.isnan(want["x"][5]) and not np.isnan(want["dbh"][-1]) and not np.isnan(want["dbh"][6:9]).any()
    if stride == 4:
        wide = np.full((len(xyz), 4), 7.0, xyz.dtype)
        wide[:, :3] = xyz
        dev = torch.from_numpy(wide).cuda()[:, :3]
        assert dev.stride() == (4, 1)
        inv = tree_inventory(dev, torch.from_numpy(lab).cuda())
        host = tree_inventory(wide[:, :3], lab)
    else:
        inv = tree_inventory(torch.from_numpy(xyz).cuda(), torch.from_numpy(lab).cuda())
        host = tree_inventory(xyz, lab.astype(np.int32))
    assert_matches(inv, want)
    for k in ref.COLUMNS:                                           # host arrays and device tensors: the same bits
        assert np.array_equal(inv[k], host[k], equal_nan=True), k


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases_through_the_kernel(name):
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab, check = cases.CASES[name]()
    inv = tree_inventory(xyz, lab)
    check(inv)
    assert_matches(inv, ref.tree_inventory(xyz, lab))


def test_offset_and_parameters():
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab, off, check = cases.offset_case()
    check(tree_inventory(xyz, lab, offset=off), tree_inventory(xyz, lab))
    check(tree_inventory(xyz, lab, offset=torch.from_numpy(off).cuda()), tree_inventory(xyz, lab))
    for kw in (dict(slice_height=1.25, slice_thickness=0.05), dict(dbh_min_points=65), dict(dbh_max_radius=0.1), dict(crown_cell=10.0),
               dict(slice_height=0.9, slice_thickness=1.0, dbh_max_radius=0.2, dbh_min_points=3, crown_cell=0.01)):
        assert_matches(tree_inventory(xyz, lab, **kw), ref.tree_inventory(xyz, lab, **kw))
    with pytest.raises(ValueError):                                 # a crown cell index beyond 2^20: refused, not wrapped
        tree_inventory(xyz + np.array([3e5, 0, 0]), lab, crown_cell=0.25)


def test_determinism_and_row_order(edge_cloud):
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab = edge_cloud["f64"], edge_cloud["lab"]
    a, b = tree_inventory(xyz, lab), tree_inventory(xyz, lab)
    for k in ref.COLUMNS:
        assert a[k].tobytes() == b[k].tobytes(), k                  # bit-identical, NaN payloads included
    p = np.random.default_rng(3).permutation(len(xyz))
    assert_matches(tree_inventory(xyz[p], lab[p]), a)


def _small_plot():
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=24, voxel=0.1, n_trees=20, fill=0.10, seed=5)
    return t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0]), t["instance_label"].astype(np.int64)


def test_labelled_synthetic_tile():
    """make_tile(extent=24, voxel=0.1, n_trees=20, fill=0.10, seed=5) with its ground-truth labels, as float32 points.
    Checked on the CPU before the seed was fixed: the restatement alone gives 20 trees, all of more than 11 rows, 0 of them with a NaN dbh
    (dbh 0.27 .. 0.65 m from 10 .. 33 slice rows each)."""
    from treelearn_amd.synth import make_tile
    from treelearn_amd.util.inventory import tree_inventory
    t = make_tile(extent=24, voxel=0.1, n_trees=20, fill=0.10, seed=5)
    xyz, lab = t["points"], t["instance_label"].astype(np.int64)
    want = ref.tree_inventory(xyz, lab)
    inv = tree_inventory(torch.from_numpy(xyz).cuda(), torch.from_numpy(lab).cuda())
    assert_matches(inv, want)
    big = inv["n_points"] > 11
    assert big.sum() >= 10 and (inv["height"][big] > 0).all()
    n_nan = int(np.isnan(inv["dbh"][big]).sum())
    print(f"trees: {len(big)}, of more than 11 rows: {int(big.sum())}, without a DBH: {n_nan}")
    assert n_nan <= big.sum() / 4


def test_segment_forest_inventory_files_and_cli(tmp_path):
    """segment_forest(..., inventory=True) on the small plot with the pinned-head random model.  The inventory is computed in the centred
    frame and un-centred; crown cells are those of that frame (floor(x / c) of centred x), so the restatement is held to it in the same
    frame: the test centres the cloud as segment_forest does (the same torch expression on the same device) and passes offset = mean.
    The columns that do not depend on the frame are also compared with the restatement of the returned input-frame coords.  The
    flagged call passes an inventory_cfg (crown_cell 0.5), so that path is the one compared."""
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import random_state_dict
    from treelearn_amd.util.inventory import cloud_inventory, write_inventory
    from treelearn_amd.util.segment import CATEGORIES, MODEL_CFG, save_results, segment_forest
    pts, _ = _small_plot()
    sd = random_state_dict(7, channels=32, num_blocks=7)
    # random backbone; heads pinned so that every point is a tree point with a zero offset, so grouping finds clusters to carry through
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    model = TreeLearn(**MODEL_CFG).cuda().eval()
    model.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)   # random weights: group every tree point
    with torch.no_grad():
        res = segment_forest(pts, model, grouping_cfg=cfg, return_type="original", inventory=True, inventory_cfg=dict(crown_cell=0.5))
        plain = segment_forest(pts, model, grouping_cfg=cfg, return_type="original")
    assert set(plain) == {"coords", "labels", "categories"} and set(res) == set(plain) | {"inventory"}
    for k in plain:
        assert np.array_equal(plain[k], res[k]), k
    inv, T = res["inventory"], len(res["categories"])
    assert T >= 1 and inv["tree_id"].tolist() == list(range(1, T + 1))
    # the centred frame, as segment_forest builds it
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    centred = (xyz - mean).cpu().numpy()
    assert np.array_equal((xyz - mean + mean).cpu().numpy(), res["coords"])
    assert_matches(inv, ref.tree_inventory(centred, res["labels"], offset=mean.cpu().numpy(), crown_cell=0.5))
    # the columns that no rounding of the frame change can touch, against the returned coords (z + mean is monotone: ranks survive);
    # positions in the input frame, near (1000, 2000, 50)
    assert_matches(inv, ref.tree_inventory(res["coords"], res["labels"], crown_cell=0.5), exact=("tree_id", "n_points", "z_low", "z_top"), close=())
    seen = inv["n_points"] > 0
    assert seen.all()
    assert (np.abs(inv["x"] - 1000) < 13).all() and (np.abs(inv["y"] - 2000) < 13).all() and (np.abs(inv["z"] - 50) < 30).all()
    # save_results: one CSV row per category entry, the category names in the last column
    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    rows = list(csv.reader(open(tmp_path / "api" / "tree_inventory.csv", newline="")))
    assert rows[0] == list(ref.COLUMNS) + ["category"] and len(rows) == 1 + T
    assert [r[-1] for r in rows[1:]] == [CATEGORIES[int(c)] for c in res["categories"]]
    assert [int(r[1]) for r in rows[1:]] == inv["n_points"].tolist() and [float(r[2]) for r in rows[1:]] == inv["x"].tolist()
    save_results(plain, str(tmp_path / "plain"), "plot", ["npy"], save_treewise=False)
    assert not (tmp_path / "plain" / "tree_inventory.csv").exists()

    # the command line in a child process on the saved N x 4 file: the CSV of cloud_inventory + write_inventory, byte for byte
    forest = tmp_path / "api" / "full_forest" / "plot.npy"
    write_inventory(str(tmp_path / "want.csv"), cloud_inventory(np.load(forest)))
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "treelearn_amd.util.inventory", "--forest", str(forest), "--out",
                        str(tmp_path / "cli.csv")], capture_output=True, text=True, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO))
    assert p.returncode == 0 and f"{T} trees" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    assert (tmp_path / "cli.csv").read_bytes() == (tmp_path / "want.csv").read_bytes()
    cli = list(csv.reader(open(tmp_path / "cli.csv", newline="")))
    assert [r[:2] for r in cli[1:]] == [r[:2] for r in rows[1:]]                      # the same trees and point counts as the segmenter's CSV
    assert np.allclose([float(r[2]) for r in cli[1:]], inv["x"], rtol=0, atol=1e-9)
