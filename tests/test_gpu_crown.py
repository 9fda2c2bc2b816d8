"""GPU tests of the crown structure (csrc/tl_crown.hip, util/crown.py) against the numpy restatement of tests/crown_restatement.py.

Bounds.  The profile width L, crown_layers, h, n, cells, crown_base_h, crown_widest_h, crown_voxels, crown_volume, crown_proj_cells,
crown_proj_area, crown_x, crown_y and every NaN pattern are compared exactly: they are integer counts on the voxel grid and products of
them, once every float decision is farther than 1e-6 from its threshold, which each test asserts on the restatement's margins first (a
condition on the inputs).  Without a terrain crown_length and crown_ratio are exact as well (z_low and z_top are ranks of the rows' own
z).  radii, crown_radius_max, crown_radius_mean and crown_offset are compared to 1e-9 absolute, §16's bound: the formulas are identical and
only the position (px, py), a float sum whose order differs, and with a terrain the sampled z_ground (then crown_length and crown_ratio
too) differ between the kernels and the restatement."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crown_cases as cases
import crown_restatement as ref
import inventory_restatement as inv_ref
import terrain_restatement as ter_ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9
EXACT = ("crown_layers", "crown_base_h", "crown_widest_h", "crown_voxels", "crown_volume", "crown_proj_cells", "crown_proj_area", "crown_x", "crown_y")
HEIGHTS = ("crown_length", "crown_ratio")                                 # exact without a terrain
CLOSE = ("crown_offset", "crown_radius_max", "crown_radius_mean")


def _close(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"NaN pattern of {name}"
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{name}: max abs difference {err:.3e}")
    assert err <= ATOL, (name, err)


def _same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=True), name


def assert_admissible(want):
    print("margins:", {k: f"{v:.3e}" for k, v in want["margins"].items()})
    assert min(want["margins"].values()) > ref.MIN_MARGIN, want["margins"]


def assert_crowns(inv, want, ground=False):
    from treelearn_amd.util.crown import CROWN_COLUMNS, PROFILE_KEYS
    assert CROWN_COLUMNS == ref.CROWN_COLUMNS and tuple(inv["crown_profile"]) == PROFILE_KEYS == ref.PROFILE_KEYS
    got_p, want_p = inv["crown_profile"], want["crown_profile"]
    for k in ("h", "n", "cells"):
        _same(k, got_p[k], want_p[k])
    assert np.array_equal((~np.isnan(got_p["h"])).sum(1), want["L_t"])
    for k in EXACT + (() if ground else HEIGHTS):
        _same(k, inv[k], want[k])
    _close("radii", got_p["radii"], want_p["radii"])
    for k in CLOSE + (HEIGHTS if ground else ()):
        _close(k, inv[k], want[k])


def inventory(xyz, lab, **kw):
    from treelearn_amd.util.inventory import tree_inventory
    return tree_inventory(xyz, lab, crown=True, **kw)


def _through_stage(case):
    """A hand case that sets its own z_ref: the inventory's table, the case's reference height in it, through util.crown.crown_stage."""
    from treelearn_amd.util.crown import check_params, crown_stage, to_columns
    from treelearn_amd.util.inventory import tree_inventory
    plain = tree_inventory(case["xyz"], case["lab"])
    order = np.argsort(case["lab"], kind="stable")
    order = order[case["lab"][order] >= 1]
    tree = np.column_stack([plain["x"], plain["y"], case["z_ref"], plain["z_top"]])
    *dev, err = crown_stage(torch.from_numpy(case["xyz"][order]).cuda(), torch.from_numpy(case["lab"][order]).cuda(), len(tree),
                            torch.from_numpy(tree).cuda(), check_params(case["cfg"]), lambda name: None)
    assert int(err.item()) == 0
    res = dict(plain)
    res.update(to_columns(*(t.cpu().numpy() for t in dev), None))
    want = dict(inv_ref.tree_inventory(case["xyz"], case["lab"]))
    want.update(ref.crown_structure(case["xyz"], case["lab"], want["x"], want["y"], case["z_ref"], want["z_top"], **case["cfg"]))
    return res, want


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases_through_the_kernels(name):
    from treelearn_amd.util.crown import CROWN_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS
    case = cases.CASES[name]()
    if "z_ref" in case:
        inv, want = _through_stage(case)
    else:
        inv = inventory(case["xyz"], case["lab"], crown_cfg=case["cfg"])
        want = ref.tree_crowns(case["xyz"], case["lab"], crown_cfg=case["cfg"])
        assert tuple(inv) == COLUMNS + CROWN_COLUMNS + ("crown_profile",)
    # admissible: the positions are the same bits (the anchor centres, crown_cases.py), so no float decision sees a different input
    for k in ("x", "y", "z_low", "z_top"):
        _same(k, inv[k], want[k])
    case["check"](inv)
    assert_crowns(inv, want)
    _same("radii", inv["crown_profile"]["radii"], want["crown_profile"]["radii"])      # from the same bits by the same operations: equal
    for k in CLOSE:
        _same(k, inv[k], want[k])


# ------------------------------------------------------------------ one cloud built for the edges of the kernels, on sloping ground
SIZES = {1: 70001, 2: 1, 3: 12, 4: 13, 6: 255, 7: 256, 8: 257, 9: 70001}   # rows per tree; label 5 is missing
VOXEL_TREE, COLUMN_TREE, LAYERS_256, TALLER, HOLE_TREE = 9, 10, 11, 12, 13
COLUMN_ROWS = (300, 212, 1, 255, 256, 257, 3)                              # rows per xy column of COLUMN_TREE
TERRAIN_CFG = dict(fill_radius=2)
N_TREES = 13


def _surf(x, y):
    return 0.05 * x + 0.02 * y


def _q(z):
    """Heights on a lattice of 1/64 m (exact in float32 too): with a sampled z_ground the rows of a tree then take 32 values of
    (z - z_ground) / layer modulo 1, and the layer margin is a property of the tree, not of its 70 001 rows."""
    return np.round(np.asarray(z) * 64.0) / 64.0


def _edge_cloud():
    rng = np.random.default_rng(20)
    rows, lab = [], []

    def add(p, l):
        rows.append(np.asarray(p, np.float64).reshape(-1, 3)); lab.append(np.full(len(rows[-1]), l, np.int64))

    centre = {t: (-18.0 + 3.0 * (t - 1) + rng.uniform(-0.1, 0.1), rng.uniform(-1, 1)) for t in range(1, N_TREES + 1)}

    def stem_and_crown(t, n, top=16.0):
        cx, cy = centre[t]
        z0 = _surf(cx, cy)
        ns = int(0.2 * n)
        a, h = rng.uniform(0, 2 * np.pi, ns), rng.uniform(0.0, 0.75 * top, ns)
        add(np.column_stack([cx + 0.2 * np.cos(a), cy + 0.2 * np.sin(a), _q(z0 + h)]), t)
        nc = n - ns
        add(np.column_stack([cx + rng.normal(0, 1.5, nc), cy + rng.normal(0, 1.5, nc), _q(z0 + rng.uniform(0.5 * top, top, nc))]), t)

    stem_and_crown(1, SIZES[1])
    for t in (2, 3, 4):                                                   # 1, 12 and 13 rows: small blobs, up to 3 m tall
        cx, cy = centre[t]
        n = SIZES[t]
        add(np.column_stack([cx + rng.normal(0, 0.3, n), cy + rng.normal(0, 0.3, n), _q(_surf(cx, cy) + rng.uniform(0.0, 3.0, n))]), t)
    for t in (6, 7, 8):                                                   # 255, 256, 257 rows: one workgroup stride, one less, one more
        stem_and_crown(t, SIZES[t], top=8.0)
    # 70 001 rows in one voxel: inside one cell and one layer above z_low, three rows (of rank 0 .. 2) just below it
    cx, cy = centre[VOXEL_TREE]
    ix, iy, z0 = np.floor(cx / 0.25), np.floor(cy / 0.25), _q(_surf(cx, cy))
    n = SIZES[VOXEL_TREE] - 3
    add(np.column_stack([(ix + rng.uniform(0.05, 0.95, n)) * 0.25, (iy + rng.uniform(0.05, 0.95, n)) * 0.25, z0 + rng.integers(0, 28, n) / 64.0]), VOXEL_TREE)
    add([[(ix + 0.5) * 0.25, (iy + 0.5) * 0.25, z0 - d] for d in (0.25, 0.5, 1.0)], VOXEL_TREE)
    # xy columns of 300, 212, 1, ... rows: in the sorted keys a column starts and ends anywhere in the 256-thread stride
    cx, cy = centre[COLUMN_TREE]
    z0 = _surf(cx, cy)
    add([[cx, cy, _q(z0)]] * 4, COLUMN_TREE)
    for k, n in enumerate(COLUMN_ROWS):
        x, y = (np.floor(cx / 0.25) + 2 * k - 6 + 0.5) * 0.25, (np.floor(cy / 0.25) + (k % 3) + 0.5) * 0.25
        add(np.column_stack([np.full(n, x), np.full(n, y), _q(z0 + rng.uniform(0.0, 12.0, n))]), COLUMN_TREE)
    # exactly 256 layers (127.5 <= H < 128 from z_low and from the ground alike) and a taller tree, cut at 256
    for t, H in ((LAYERS_256, 127.75), (TALLER, 140.0)):
        cx, cy = centre[t]
        z0 = _q(_surf(cx, cy))
        add([[cx, cy, z0]] * 4 + [[cx, cy, z0 + H]] * 4, t)
        n = 4000
        add(np.column_stack([cx + rng.normal(0, 1.0, n), cy + rng.normal(0, 1.0, n), _q(z0 + rng.uniform(0.0, H, n))]), t)
    stem_and_crown(HOLE_TREE, 6000)
    # the ground (label 0) with a hole of 3 m around HOLE_TREE, and unassigned rows (-1) anywhere, crowns included
    gx, gy = rng.uniform(-21, 21, 24000), rng.uniform(-6, 6, 24000)
    hx, hy = centre[HOLE_TREE]
    keep = (gx - hx) ** 2 + (gy - hy) ** 2 > 3.0 ** 2
    add(np.column_stack([gx, gy, _surf(gx, gy) + rng.normal(0, 0.01, 24000)])[keep], 0)
    add(np.column_stack([rng.uniform(-21, 21, 3000), rng.uniform(-6, 6, 3000), rng.uniform(0, 20, 3000)]), -1)
    xyz, lab = np.concatenate(rows), np.concatenate(lab)
    p = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[p]), np.ascontiguousarray(lab[p])


def _check_edge_fixture(w, ground):
    n = w["n_points"].tolist()
    assert len(n) == N_TREES and [n[t - 1] for t in sorted(SIZES)] == [SIZES[t] for t in sorted(SIZES)] and n[4] == 0
    assert n[COLUMN_TREE - 1] == 4 + sum(COLUMN_ROWS)
    lay = w["crown_layers"]
    assert lay[LAYERS_256 - 1] == 256 and lay[TALLER - 1] == 256 and w["crown_profile"]["h"].shape == (N_TREES, 256) and lay[4] == 0
    H = (w["z_top"] - (w["z_ground"] if ground else w["z_low"]))
    assert 127.5 <= H[LAYERS_256 - 1] < 128.0 and H[TALLER - 1] > 128.0
    assert w["crown_profile"]["n"][TALLER - 1].sum() < n[TALLER - 1] - 100                   # rows above the cut
    assert w["crown_proj_cells"][COLUMN_TREE - 1] >= 4 and w["crown_voxels"][0] > 1000
    if not ground:                                                       # (from the ground the voxel may straddle two layers)
        assert lay[VOXEL_TREE - 1] == 1 and w["crown_profile"]["n"][VOXEL_TREE - 1, 0] == SIZES[VOXEL_TREE] - 3
        assert w["crown_profile"]["cells"][VOXEL_TREE - 1, 0] == 1 and np.isnan(w["crown_base_h"][VOXEL_TREE - 1])
    if ground:
        assert np.isnan(w["z_ground"][HOLE_TREE - 1]) and lay[HOLE_TREE - 1] == 0 and np.isnan(w["crown_x"][HOLE_TREE - 1])
        assert not np.isnan(np.delete(w["z_ground"], [4, HOLE_TREE - 1])).any()
    else:
        assert w["crown_voxels"][HOLE_TREE - 1] > 100


@pytest.fixture(scope="module")
def edge_cloud():
    """The cloud as f64 and f32, each with the restatement's result without and with the terrain (computed once, never changed)."""
    xyz, lab = _edge_cloud()
    d = dict(lab=lab, f64=xyz, f32=xyz.astype(np.float32))
    for dt in ("f64", "f32"):
        t = ter_ref.terrain_model(d[dt], lab, **TERRAIN_CFG)
        d["terrain_" + dt] = t
        d["plain_" + dt] = ref.tree_crowns(d[dt], lab)
        d["ground_" + dt] = ref.tree_crowns(d[dt], lab, terrain=t)
        _check_edge_fixture(d["plain_" + dt], False)
        _check_edge_fixture(d["ground_" + dt], True)
    return d


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("ground", [False, True])
def test_edge_cloud(edge_cloud, dtype, stride, ground):
    from treelearn_amd.util.crown import CROWN_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, GROUND_COLUMNS, tree_inventory
    from treelearn_amd.util.stem import STEM_COLUMNS
    from treelearn_amd.util.terrain import terrain_model
    xyz, lab = edge_cloud[dtype], edge_cloud["lab"]
    want = edge_cloud[("ground_" if ground else "plain_") + dtype]
    assert_admissible(want)
    if stride == 4:
        wide = np.full((len(xyz), 4), 7.0, xyz.dtype)
        wide[:, :3] = xyz
        dev = torch.from_numpy(wide).cuda()[:, :3]
        assert dev.stride() == (4, 1)
    else:
        dev = torch.from_numpy(xyz).cuda()
    dlab = torch.from_numpy(lab).cuda()
    off = np.array([500.0, -300.0, 120.0])
    t = terrain_model(dev, dlab, **TERRAIN_CFG) if ground else None
    inv = tree_inventory(dev, dlab, terrain=t, crown=True, offset=off)
    old = COLUMNS + (GROUND_COLUMNS if ground else ())
    assert tuple(inv) == old + CROWN_COLUMNS + ("crown_profile",)
    moved = dict(want, crown_x=want["crown_x"] + off[0], crown_y=want["crown_y"] + off[1])
    assert_crowns(inv, moved, ground)
    plain = tree_inventory(dev, dlab, terrain=t, offset=off)              # the sixteen and the eight old columns: bit for bit
    assert tuple(plain) == old
    for k in old:
        assert inv[k].tobytes() == plain[k].tobytes(), k
    if stride == 3:                                                       # together with the stem profiles: every column of both, bit for bit
        both = tree_inventory(dev, dlab, terrain=t, stem=True, crown=True, offset=off)
        stems = tree_inventory(dev, dlab, terrain=t, stem=True, offset=off)
        assert tuple(both) == old + STEM_COLUMNS + ("stem_profile",) + CROWN_COLUMNS + ("crown_profile",) and tuple(stems) == old + STEM_COLUMNS + ("stem_profile",)
        for k in old + STEM_COLUMNS:
            assert both[k].tobytes() == stems[k].tobytes(), k
        for k in CROWN_COLUMNS:
            assert both[k].tobytes() == inv[k].tobytes(), k
        for k in stems["stem_profile"]:
            assert both["stem_profile"][k].tobytes() == stems["stem_profile"][k].tobytes(), k
        for k in inv["crown_profile"]:
            assert both["crown_profile"][k].tobytes() == inv["crown_profile"][k].tobytes(), k
    if stride == 3 and not ground:                                        # host arrays and device tensors: the same bits
        host = tree_inventory(xyz, lab.astype(np.int32), crown=True, offset=off)
        for k in CROWN_COLUMNS:
            assert host[k].tobytes() == inv[k].tobytes(), k
        for k in inv["crown_profile"]:
            assert host["crown_profile"][k].tobytes() == inv["crown_profile"][k].tobytes(), k


def test_determinism_and_row_order(edge_cloud):
    xyz, lab = edge_cloud["f64"], edge_cloud["lab"]
    a, b = inventory(xyz, lab), inventory(xyz, lab)
    for k in ref.CROWN_COLUMNS:
        assert a[k].tobytes() == b[k].tobytes(), k                        # bit-identical, NaN payloads included
    for k in a["crown_profile"]:
        assert a["crown_profile"][k].tobytes() == b["crown_profile"][k].tobytes(), k
    # a row permutation reorders the sum behind the position only: every integer and lattice value the same, the radii to the tolerance
    assert_admissible(edge_cloud["plain_f64"])
    p = np.random.default_rng(3).permutation(len(xyz))
    c = inventory(xyz[p], lab[p])
    assert_crowns(c, dict(edge_cloud["plain_f64"], **{k: a[k] for k in ref.CROWN_COLUMNS}, crown_profile=a["crown_profile"]))


def test_parameters(edge_cloud):
    """Other grids, thresholds and caps on the same cloud; each admissible by its own margins."""
    xyz, lab = edge_cloud["f64"], edge_cloud["lab"]
    for cfg in (dict(layer=0.25, cell=0.5, min_height=0.0), dict(max_layers=7, base_percent=100, max_gap=0),
                dict(layer=2.0, cell=0.1, min_height=3.0, base_percent=1, max_gap=5), dict(min_height=0.0, max_layers=1, cell=1.0)):
        want = ref.tree_crowns(xyz, lab, crown_cfg=cfg)
        assert_admissible(want)
        if cfg.get("min_height") == 0.0:                                  # the tree of one voxel has a crown of one cell now
            assert want["crown_voxels"][VOXEL_TREE - 1] in (1, 2) and want["crown_proj_cells"][VOXEL_TREE - 1] == 1
        assert_crowns(inventory(xyz, lab, crown_cfg=cfg), want)


def test_error_flag_at_the_edge_of_the_key():
    """A row 4096 cells west / south or 4095 cells east / north of its tree's cell still has a key; one cell farther, or a coordinate that
    is not finite, raises.  The lollipop's position is exactly the centre of cell (12, -8)."""
    case = cases.CASES["lollipop"]()

    def with_row(row):
        return np.concatenate([case["xyz"], [row]]), np.concatenate([case["lab"], [1]])

    for row in ([(12 - 4096 + 0.5) / 4, -1.875, 4.25], [(12 + 4095 + 0.5) / 4, -1.875, 4.25], [3.125, (-8 - 4096 + 0.5) / 4, 4.25],
                [3.125, (-8 + 4095 + 0.5) / 4, 4.25]):
        xyz, lab = with_row(row)
        want = ref.tree_crowns(xyz, lab)
        assert want["margins"]["anchor"] == 0.5 and want["crown_proj_cells"][0] == 17
        inv = inventory(xyz, lab)
        assert inv["x"].tobytes() == want["x"].tobytes() and inv["y"].tobytes() == want["y"].tobytes()
        assert_crowns(inv, want)
    for row in ([(12 - 4097 + 0.5) / 4, -1.875, 4.25], [(12 + 4096 + 0.5) / 4, -1.875, 4.25], [3.125, (-8 - 4097 + 0.5) / 4, 4.25],
                [3.125, (-8 + 4096 + 0.5) / 4, 4.25], [3.125, -1.875, np.inf]):
        xyz, lab = with_row(row)
        with pytest.raises(ValueError):
            ref.tree_crowns(xyz, lab)
        with pytest.raises(ValueError):
            inventory(xyz, lab)
    # the same far row in no layer (above the tree) is no error: it has no key
    xyz, lab = with_row([(12 + 5000 + 0.5) / 4, -1.875, 7.0])
    assert_crowns(inventory(xyz, lab), ref.tree_crowns(xyz, lab))


def test_labelled_synthetic_tile():
    """make_tile(extent=20.0, voxel=0.1, n_trees=20, seed=0) with its ground-truth labels, as float32 points.  Checked on the CPU before
    the seed was fixed: the restatement alone is admissible and gives every one of the 20 trees a crown."""
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=20.0, voxel=0.1, n_trees=20, seed=0)
    xyz, lab = t["points"], t["instance_label"].astype(np.int64)
    want = ref.tree_crowns(xyz, lab)
    assert_admissible(want)
    assert len(want["tree_id"]) == 20 and want["crown_proj_cells"].min() >= 1 and not np.isnan(want["crown_base_h"]).any()
    inv = inventory(torch.from_numpy(xyz).cuda(), torch.from_numpy(lab).cuda())
    assert_crowns(inv, want)


# ------------------------------------------------------------------ segment_forest, save_results, the command lines
def _small_plot():
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)
    return t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])


SAMPLE = dict(stride=1.0)                                                 # tiles side by side: four cover the plot
CFG = dict(layer=0.25, max_gap=2)


@pytest.fixture(scope="module")
def segmented():
    """segment_forest on a 12 m plot of six trees with the pinned-head random model of tests/test_gpu_inventory.py: once with crown=True
    (which implies the inventory), once without any flag."""
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import random_state_dict
    from treelearn_amd.util.segment import MODEL_CFG, segment_forest
    pts = _small_plot()
    sd = random_state_dict(7, channels=32, num_blocks=7)
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    m = TreeLearn(**MODEL_CFG).cuda().eval()
    m.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)
    with torch.no_grad():
        res = segment_forest(pts, m, sample_cfg=SAMPLE, grouping_cfg=cfg, return_type="original", crown=True, crown_cfg=CFG)
        plain = segment_forest(pts, m, sample_cfg=SAMPLE, grouping_cfg=cfg, return_type="original")
        with pytest.raises(ValueError):                                  # parameters are checked before any GPU work
            segment_forest(None, None, crown=True, crown_cfg=dict(layer=0.0))
    return pts, res, plain


def test_segment_forest_without_the_flag_returns_the_same_keys(segmented):
    _, res, plain = segmented
    assert set(plain) == {"coords", "labels", "categories"} and set(res) == set(plain) | {"inventory"}
    for k in plain:
        assert np.array_equal(plain[k], res[k]), k


def test_segment_forest_crown_files_and_cli(segmented, tmp_path):
    """The stage runs in the centred frame and the centroid is un-centred; the restatement is held to it in the same frame: the test
    centres the cloud as segment_forest does (the same torch expression on the same device) and passes offset = mean."""
    from treelearn_amd.util.crown import CROWN_COLUMNS, PROFILE_KEYS, write_crown_profiles
    from treelearn_amd.util.inventory import COLUMNS, cloud_inventory, write_inventory
    from treelearn_amd.util.segment import save_results
    pts, res, plain = segmented
    inv = res["inventory"]
    assert tuple(inv) == COLUMNS + CROWN_COLUMNS + ("crown_profile",)
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    centred, mean_h = (xyz - mean).cpu().numpy(), mean.cpu().numpy()
    want = ref.tree_crowns(centred, res["labels"], offset=mean_h, crown_cfg=CFG)
    assert_admissible(want)
    print("crown base per tree:", inv["crown_base_h"].tolist())
    assert_crowns(inv, want)

    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    rows = list(csv.reader(open(tmp_path / "api" / "tree_inventory.csv", newline="")))
    assert rows[0] == list(COLUMNS + CROWN_COLUMNS) + ["category"] and len(rows) == 1 + len(res["categories"])
    assert [int(r[16]) for r in rows[1:]] == inv["crown_layers"].tolist() and [int(r[21]) for r in rows[1:]] == inv["crown_voxels"].tolist()
    assert [int(r[23]) for r in rows[1:]] == inv["crown_proj_cells"].tolist()
    assert [float(r[22]) for r in rows[1:] if r[22] != "nan"] == inv["crown_volume"][~np.isnan(inv["crown_volume"])].tolist()
    with np.load(tmp_path / "api" / "crown_profiles.npz") as f:
        assert set(f.files) == {"tree_id"} | set(PROFILE_KEYS) and np.array_equal(f["tree_id"], inv["tree_id"])
        assert all(f[k].tobytes() == inv["crown_profile"][k].tobytes() for k in PROFILE_KEYS)
    save_results(plain, str(tmp_path / "plain"), "plot", ["npy"], save_treewise=False)
    assert not (tmp_path / "plain" / "crown_profiles.npz").exists() and not (tmp_path / "plain" / "tree_inventory.csv").exists()

    # the command lines in child processes on the saved N x 4 file, against the same calls made here
    forest = tmp_path / "api" / "full_forest" / "plot.npy"
    data = np.load(forest)
    env = dict(os.environ, PYTHONPATH=REPO)
    run = lambda *a: subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", *a], capture_output=True, text=True, cwd=REPO, env=env)  # noqa: E731
    p = run("treelearn_amd.util.crown", "--forest", str(forest), "--out", str(tmp_path / "cli.npz"), "--csv", str(tmp_path / "cli_crown.csv"),
            "--terrain", "--cell", "1.0", "--crown-layer", "0.25", "--crown-max-gap", "2")
    assert p.returncode == 0 and f"{len(inv['tree_id'])} trees" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    here = cloud_inventory(data, terrain=True, terrain_cfg=dict(cell=1.0), crown=True, crown_cfg=CFG)
    write_crown_profiles(str(tmp_path / "want.npz"), here)
    write_inventory(str(tmp_path / "want_crown.csv"), here)
    with np.load(tmp_path / "cli.npz") as f, np.load(tmp_path / "want.npz") as g:
        assert set(f.files) == set(g.files) and all(f[k].tobytes() == g[k].tobytes() for k in g.files)
    assert (tmp_path / "cli_crown.csv").read_bytes() == (tmp_path / "want_crown.csv").read_bytes()
    p = run("treelearn_amd.util.inventory", "--forest", str(forest), "--out", str(tmp_path / "cli.csv"), "--crown", "--crown-layer", "0.25",
            "--crown-max-gap", "2")
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    write_inventory(str(tmp_path / "want.csv"), cloud_inventory(data, crown=True, crown_cfg=CFG))
    assert (tmp_path / "cli.csv").read_bytes() == (tmp_path / "want.csv").read_bytes()
    assert list(csv.reader(open(tmp_path / "cli.csv", newline="")))[0] == list(COLUMNS + CROWN_COLUMNS)
    p = run("treelearn_amd.util.stem", "--forest", str(forest), "--out", str(tmp_path / "stems.npz"), "--csv", str(tmp_path / "cli_both.csv"),
            "--crown", "--crown-layer", "0.25", "--crown-max-gap", "2")
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    write_inventory(str(tmp_path / "want_both.csv"), cloud_inventory(data, stem=True, crown=True, crown_cfg=CFG))
    assert (tmp_path / "cli_both.csv").read_bytes() == (tmp_path / "want_both.csv").read_bytes()
    # without the flag: the old columns and the bytes of the flagged file's first sixteen
    write_inventory(str(tmp_path / "old.csv"), cloud_inventory(data))
    old, new = (list(csv.reader(open(tmp_path / n, newline=""))) for n in ("old.csv", "cli.csv"))
    assert old[0] == list(COLUMNS) and old == [r[:16] for r in new]
