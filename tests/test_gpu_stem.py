"""GPU tests of the stem profiles (csrc/tl_stem.hip, util/stem.py) against the numpy restatement of tests/stem_restatement.py.

Bounds.  The profile width S, every tree's slab count, h, n, state, stem_slices, stem_base_h, stem_top_h and every NaN pattern are compared
exactly: comparisons and integer counts do not depend on the order of a sum once every decision is farther than 1e-6 from its
threshold, which each test asserts on the restatement's margins first (a condition on the inputs).  x, y, r, rmse, stem_volume, dbh_stem,
stem_lean and stem_taper are compared to 1e-9 absolute: the formulas are identical and only the order of the f64 sums of at most 1e5
terms of magnitude <= 1e2 differs (the bound and reasoning of §16 and §17)."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inventory_restatement as inv_ref
import stem_cases as cases
import stem_restatement as ref
import terrain_restatement as ter_ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9
EXACT = ("stem_slices", "stem_base_h", "stem_top_h")
CLOSE = ("stem_volume", "dbh_stem", "stem_lean", "stem_taper")


def _close(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"NaN pattern of {name}"
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{name}: max abs difference {err:.3e}")
    assert err <= ATOL, (name, err)


def assert_admissible(want):
    print("margins:", {k: f"{v:.3e}" for k, v in want["margins"].items()})
    assert min(want["margins"].values()) > ref.MIN_MARGIN, want["margins"]


def assert_stems(inv, want):
    from treelearn_amd.util.stem import PROFILE_KEYS, STEM_COLUMNS
    assert STEM_COLUMNS == ref.STEM_COLUMNS and tuple(inv["stem_profile"]) == PROFILE_KEYS == ref.PROFILE_FLOAT + ref.PROFILE_INT
    got_p, want_p = inv["stem_profile"], want["stem_profile"]
    for k in ("h", "n", "state"):
        assert got_p[k].shape == want_p[k].shape and got_p[k].dtype == want_p[k].dtype, (k, got_p[k].shape, want_p[k].shape)
        assert np.array_equal(got_p[k], want_p[k], equal_nan=True), k
    assert np.array_equal((~np.isnan(got_p["h"])).sum(1), want["S_t"])
    for k in EXACT:
        assert inv[k].dtype == want[k].dtype and np.array_equal(inv[k], want[k], equal_nan=True), k
    for k in ("x", "y", "r", "rmse"):
        _close(k, got_p[k], want_p[k])
    for k in CLOSE:
        _close(k, inv[k], want[k])


def inventory(xyz, lab, **kw):
    from treelearn_amd.util.inventory import tree_inventory
    return tree_inventory(xyz, lab, stem=True, **kw)


def _through_stage(case):
    """A hand case that sets its own z_ref: the inventory's table, the case's reference height in it, through util.stem.stem_stage."""
    from treelearn_amd.util.inventory import tree_inventory
    from treelearn_amd.util.stem import check_params, stem_stage, to_columns
    plain = tree_inventory(case["xyz"], case["lab"])
    order = np.argsort(case["lab"], kind="stable")
    order = order[case["lab"][order] >= 1]
    tree = np.column_stack([plain["x"], plain["y"], case["z_ref"], plain["z_top"]])
    dev = stem_stage(torch.from_numpy(case["xyz"][order]).cuda(), torch.from_numpy(case["lab"][order]).cuda(), len(tree),
                     torch.from_numpy(tree).cuda(), check_params(case["cfg"]), lambda name: None)
    res = dict(plain)
    res.update(to_columns(*(t.cpu().numpy() for t in dev), None))
    want = dict(inv_ref.tree_inventory(case["xyz"], case["lab"]))
    want.update(ref.stem_profiles(case["xyz"], case["lab"], want["x"], want["y"], case["z_ref"], want["z_top"], **case["cfg"]))
    return res, want


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases_through_the_kernels(name):
    from treelearn_amd.util.inventory import COLUMNS
    from treelearn_amd.util.stem import STEM_COLUMNS
    case = cases.CASES[name]()
    if "z_ref" in case:
        inv, want = _through_stage(case)
    else:
        inv = inventory(case["xyz"], case["lab"], stem_cfg=case["cfg"])
        want = ref.tree_stems(case["xyz"], case["lab"], stem_cfg=case["cfg"])
        assert tuple(inv) == COLUMNS + STEM_COLUMNS + ("stem_profile",)
    if not case.get("exact"):
        assert_admissible(want)
    case["check"](inv)
    assert_stems(inv, want)


# ------------------------------------------------------------------ one cloud of noisy cylinders on sloping ground
COUNTS = (64, 0, 1, 63, 7, 8, 65, 255, 256, 257, 1000)                    # rows in the search sets of the slabs of tree 1
SIZES = {2: 1, 3: 12, 4: 13, 6: 70001}                                    # rows of the trees 2, 3, 4, 6; label 5 is missing
HOLE_TREE = 7                                                             # stands where the terrain has no value
TERRAIN_CFG = dict(fill_radius=2)


def _surf(x, y):
    return 0.05 * x + 0.02 * y


def _noisy_ring(rng, cx, cy, r, z, n, dz=0.03):
    """n rows on a circle of radius r (evenly spaced angles from a random phase, radial noise 1e-3) at heights z -+ dz."""
    a = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(n) / max(n, 1)
    rr = r + rng.normal(0, 1e-3, n)
    return np.column_stack([cx + rr * np.cos(a), cy + rr * np.sin(a), z + rng.uniform(-dz, dz, n)])


def _edge_cloud():
    rng = np.random.default_rng(19)
    rows, lab = [], []

    def add(p, l):
        rows.append(p); lab.append(np.full(len(p), l, np.int64))

    centre = {t: (-12.0 + 4.0 * (t - 1), rng.uniform(-1, 1)) for t in range(1, 8)}
    # tree 1: a cylinder of radius 0.2 whose slabs hold COUNTS rows; 20 base rows just above the ground, four rows at the top
    cx, cy = centre[1]
    z0 = _surf(cx, cy)
    add(_noisy_ring(rng, cx, cy, 0.2, z0 + 0.01, 20, dz=0.01), 1)
    for k, n in enumerate(COUNTS):
        add(_noisy_ring(rng, cx, cy, 0.2, z0 + 0.5 + 0.5 * k, n), 1)
    add(np.column_stack([cx + rng.uniform(-1, 1, 6), cy + rng.uniform(-1, 1, 6), np.full(6, z0 + 5.75)]), 1)
    # trees of 1, 12 and 13 rows: small blobs
    for t in (2, 3, 4):
        cx, cy = centre[t]
        n = SIZES[t]
        add(np.column_stack([cx + rng.normal(0, 0.1, n), cy + rng.normal(0, 0.1, n), _surf(cx, cy) + rng.uniform(0.0, 1.5, n)]), t)
    # trees 6 and 7: a tapering stem of rows at any height, under a crown blob that swamps the search set higher up
    for t, n in ((6, SIZES[6]), (HOLE_TREE, 6000)):
        cx, cy = centre[t]
        z0 = _surf(cx, cy)
        ns = int(0.2 * n)
        h = rng.uniform(0.0, 12.0, ns)
        a = rng.uniform(0, 2 * np.pi, ns)
        rr = (0.25 - 0.01 * h) + rng.normal(0, 1e-3, ns)
        add(np.column_stack([cx + rr * np.cos(a), cy + rr * np.sin(a), z0 + h]), t)
        nc = n - ns
        add(np.column_stack([cx + rng.normal(0, 1.5, nc), cy + rng.normal(0, 1.5, nc), z0 + rng.uniform(8.0, 16.0, nc)]), t)
    # the ground (label 0) with a hole of 3 m around HOLE_TREE, and unassigned rows (-1) anywhere, stems included
    gx, gy = rng.uniform(-15, 15, 20000), rng.uniform(-6, 6, 20000)
    hx, hy = centre[HOLE_TREE]
    keep = (gx - hx) ** 2 + (gy - hy) ** 2 > 3.0 ** 2
    add(np.column_stack([gx, gy, _surf(gx, gy) + rng.normal(0, 0.01, 20000)])[keep], 0)
    add(np.column_stack([rng.uniform(-15, 15, 2000), rng.uniform(-6, 6, 2000), rng.uniform(0, 10, 2000)]), -1)
    add(_noisy_ring(rng, centre[1][0], centre[1][1], 0.1, _surf(*centre[1]) + 1.0, 50), -1)
    xyz, lab = np.concatenate(rows), np.concatenate(lab)
    p = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[p]), np.ascontiguousarray(lab[p])


@pytest.fixture(scope="module")
def edge_cloud():
    """The cloud as f64 and f32, each with the restatement's result without and with the terrain (computed once, never changed)."""
    xyz, lab = _edge_cloud()
    d = dict(lab=lab, f64=xyz, f32=xyz.astype(np.float32))
    for dt in ("f64", "f32"):
        t = ter_ref.terrain_model(d[dt], lab, **TERRAIN_CFG)
        d["terrain_" + dt] = t
        d["plain_" + dt] = ref.tree_stems(d[dt], lab)
        d["ground_" + dt] = ref.tree_stems(d[dt], lab, terrain=t)
        for k in ("plain_", "ground_"):
            w = d[k + dt]
            assert w["n_points"].tolist()[1:6] == [1, 12, 13, 0, 70001] and w["stem_profile"]["n"][0, :11].tolist() == list(COUNTS)
            assert w["stem_profile"]["state"][0, :11].tolist() == [1, 2, 2, 1, 2, 1, 1, 1, 1, 1, 1]
            assert w["stem_slices"][5] >= 8 and (w["stem_profile"]["state"][5] == 0).any() and (w["stem_profile"]["state"][5] == 2).any()
        assert np.isnan(d["ground_" + dt]["z_ground"][HOLE_TREE - 1]) and d["ground_" + dt]["stem_slices"][HOLE_TREE - 1] == 0
        assert d["plain_" + dt]["stem_slices"][HOLE_TREE - 1] >= 8 and not np.isnan(d["ground_" + dt]["z_ground"][:4]).any()
    return d


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("ground", [False, True])
def test_edge_cloud(edge_cloud, dtype, stride, ground):
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
    inv = tree_inventory(dev, dlab, terrain=t, stem=True, offset=off)
    old = COLUMNS + (GROUND_COLUMNS if ground else ())
    assert tuple(inv) == old + STEM_COLUMNS + ("stem_profile",)
    moved = dict(want, stem_profile=dict(want["stem_profile"], x=want["stem_profile"]["x"] + off[0], y=want["stem_profile"]["y"] + off[1]))
    assert_stems(inv, moved)
    plain = tree_inventory(dev, dlab, terrain=t, offset=off)              # the sixteen and the eight old columns: bit for bit
    assert tuple(plain) == old
    for k in old:
        assert inv[k].tobytes() == plain[k].tobytes(), k
    if stride == 3 and not ground:                                        # host arrays and device tensors: the same bits
        host = tree_inventory(xyz, lab.astype(np.int32), stem=True, offset=off)
        for k in STEM_COLUMNS:
            assert host[k].tobytes() == inv[k].tobytes(), k
        for k in inv["stem_profile"]:
            assert host["stem_profile"][k].tobytes() == inv["stem_profile"][k].tobytes(), k


def test_determinism_and_row_order(edge_cloud):
    xyz, lab = edge_cloud["f64"], edge_cloud["lab"]
    a, b = inventory(xyz, lab), inventory(xyz, lab)
    for k in ref.STEM_COLUMNS:
        assert a[k].tobytes() == b[k].tobytes(), k                        # bit-identical, NaN payloads included
    for k in a["stem_profile"]:
        assert a["stem_profile"][k].tobytes() == b["stem_profile"][k].tobytes(), k
    # a row permutation reorders the sums inside a slab (the stable sort keeps input order): the float tolerance, the same decisions
    assert_admissible(edge_cloud["plain_f64"])
    p = np.random.default_rng(3).permutation(len(xyz))
    c = inventory(xyz[p], lab[p])
    assert_stems(c, dict(edge_cloud["plain_f64"], **{k: a[k] for k in ref.STEM_COLUMNS}, stem_profile=a["stem_profile"]))


def test_parameters(edge_cloud):
    """Other slabs, radii and limits on the same cloud; each admissible by its own margins."""
    xyz, lab = edge_cloud["f64"], edge_cloud["lab"]
    for cfg in (dict(first_height=0.3, step=0.25, thickness=0.25, max_slices=40), dict(max_misses=1, min_points=3, corridor=0.5),
                dict(max_rmse=0.0005, max_growth=1.0, search_factor=1.0, search_margin=0.3, dbh_height=2.75),
                dict(min_radius=0.21, max_radius=0.26, start_radius=0.3, max_slices=256, step=0.2, first_height=0.2)):
        want = ref.tree_stems(xyz, lab, stem_cfg=cfg)
        assert_admissible(want)
        assert_stems(inventory(xyz, lab, stem_cfg=cfg), want)


def test_labelled_synthetic_tile():
    """make_tile(extent=20.0, voxel=0.1, n_trees=20, seed=0) with its ground-truth labels, as float32 points.  Checked on the CPU before
    the seed was fixed: the restatement alone gives every one of the 20 trees 16 .. 34 accepted slabs."""
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=20.0, voxel=0.1, n_trees=20, seed=0)
    xyz, lab = t["points"], t["instance_label"].astype(np.int64)
    want = ref.tree_stems(xyz, lab)
    assert_admissible(want)
    assert len(want["tree_id"]) == 20 and want["stem_slices"].min() >= 16 and want["stem_slices"].max() <= 34
    inv = inventory(torch.from_numpy(xyz).cuda(), torch.from_numpy(lab).cuda())
    assert_stems(inv, want)


# ------------------------------------------------------------------ segment_forest, save_results, the command lines
def _small_plot():
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)
    return t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])


SAMPLE = dict(stride=1.0)                                                 # tiles side by side: four cover the plot


@pytest.fixture(scope="module")
def segmented():
    """segment_forest on a 12 m plot of six trees with the pinned-head random model of tests/test_gpu_inventory.py: once with stem=True
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
        res = segment_forest(pts, m, sample_cfg=SAMPLE, grouping_cfg=cfg, return_type="original", stem=True, stem_cfg=dict(max_misses=4))
        plain = segment_forest(pts, m, sample_cfg=SAMPLE, grouping_cfg=cfg, return_type="original")
        with pytest.raises(ValueError):                                  # parameters are checked before any GPU work
            segment_forest(None, None, stem=True, stem_cfg=dict(step=0.0))
    return pts, res, plain


def test_segment_forest_without_the_flag_returns_the_same_keys(segmented):
    _, res, plain = segmented
    assert set(plain) == {"coords", "labels", "categories"} and set(res) == set(plain) | {"inventory"}
    for k in plain:
        assert np.array_equal(plain[k], res[k]), k


def test_segment_forest_stem_files_and_cli(segmented, tmp_path):
    """The stage runs in the centred frame and the centres are un-centred; the restatement is held to it in the same frame: the test
    centres the cloud as segment_forest does (the same torch expression on the same device) and passes offset = mean."""
    from treelearn_amd.util.inventory import COLUMNS, cloud_inventory, write_inventory
    from treelearn_amd.util.segment import save_results
    from treelearn_amd.util.stem import PROFILE_KEYS, STEM_COLUMNS, write_stem_profiles
    pts, res, plain = segmented
    inv = res["inventory"]
    assert tuple(inv) == COLUMNS + STEM_COLUMNS + ("stem_profile",)
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    centred, mean_h = (xyz - mean).cpu().numpy(), mean.cpu().numpy()
    want = ref.tree_stems(centred, res["labels"], offset=mean_h, stem_cfg=dict(max_misses=4))
    assert_admissible(want)
    print("accepted slabs per tree:", inv["stem_slices"].tolist())
    assert_stems(inv, want)

    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    rows = list(csv.reader(open(tmp_path / "api" / "tree_inventory.csv", newline="")))
    assert rows[0] == list(COLUMNS + STEM_COLUMNS) + ["category"] and len(rows) == 1 + len(res["categories"])
    assert [int(r[16]) for r in rows[1:]] == inv["stem_slices"].tolist()
    assert [float(r[19]) for r in rows[1:] if r[19] != "nan"] == inv["stem_volume"][~np.isnan(inv["stem_volume"])].tolist()
    with np.load(tmp_path / "api" / "stem_profiles.npz") as f:
        assert set(f.files) == {"tree_id"} | set(PROFILE_KEYS) and np.array_equal(f["tree_id"], inv["tree_id"])
        assert all(f[k].tobytes() == inv["stem_profile"][k].tobytes() for k in PROFILE_KEYS)
    save_results(plain, str(tmp_path / "plain"), "plot", ["npy"], save_treewise=False)
    assert not (tmp_path / "plain" / "stem_profiles.npz").exists() and not (tmp_path / "plain" / "tree_inventory.csv").exists()

    # the two command lines in child processes on the saved N x 4 file, against the same calls made here
    forest = tmp_path / "api" / "full_forest" / "plot.npy"
    data = np.load(forest)
    env = dict(os.environ, PYTHONPATH=REPO)
    run = lambda *a: subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", *a], capture_output=True, text=True, cwd=REPO, env=env)  # noqa: E731
    p = run("treelearn_amd.util.stem", "--forest", str(forest), "--out", str(tmp_path / "cli.npz"), "--csv", str(tmp_path / "cli_stem.csv"),
            "--terrain", "--cell", "1.0", "--stem-max-misses", "4")
    assert p.returncode == 0 and f"{len(inv['tree_id'])} trees" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    here = cloud_inventory(data, terrain=True, terrain_cfg=dict(cell=1.0), stem=True, stem_cfg=dict(max_misses=4))
    write_stem_profiles(str(tmp_path / "want.npz"), here)
    write_inventory(str(tmp_path / "want_stem.csv"), here)
    with np.load(tmp_path / "cli.npz") as f, np.load(tmp_path / "want.npz") as g:
        assert set(f.files) == set(g.files) and all(f[k].tobytes() == g[k].tobytes() for k in g.files)
    assert (tmp_path / "cli_stem.csv").read_bytes() == (tmp_path / "want_stem.csv").read_bytes()
    p = run("treelearn_amd.util.inventory", "--forest", str(forest), "--out", str(tmp_path / "cli.csv"), "--stem", "--stem-max-misses", "4")
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    write_inventory(str(tmp_path / "want.csv"), cloud_inventory(data, stem=True, stem_cfg=dict(max_misses=4)))
    assert (tmp_path / "cli.csv").read_bytes() == (tmp_path / "want.csv").read_bytes()
    assert list(csv.reader(open(tmp_path / "cli.csv", newline="")))[0] == list(COLUMNS + STEM_COLUMNS)
    # without the flag: the old columns and the bytes of the flagged file's first sixteen
    write_inventory(str(tmp_path / "old.csv"), cloud_inventory(data))
    old, new = (list(csv.reader(open(tmp_path / n, newline=""))) for n in ("old.csv", "cli.csv"))
    assert old[0] == list(COLUMNS) and old == [r[:16] for r in new]
