"""GPU tests of the terrain model (csrc/tl_terrain.hip, tl_tree_ground of csrc/tl_inventory.hip, util/terrain.py) against
the numpy restatement of tests/terrain_restatement.py.

Bounds.  nx, ny, ix0, iy0, n_candidates, state, the value of every ground cell, dbh_ag_n and every NaN pattern are compared exactly:
minima, comparisons and integer counts do not depend on the order of a sum.  Filled values, sampled ground, height_above_ground,
z_ground, height_ag, base_gap and dbh_ag* are compared to 1e-9 absolute: the formulas are identical and only the order of f64 sums of
at most (2 * 20 + 1)^2 terms of magnitude <= 1e2 can differ, at 1.1e-16 each, about 2e-11 (the bound and reasoning of §16)."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inventory_restatement as inv_ref
import terrain_cases as cases
import terrain_restatement as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9
GROUND_CLOSE = ("z_ground", "height_ag", "base_gap", "dbh_ag", "dbh_ag_x", "dbh_ag_y", "dbh_ag_rmse")


def _close(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"NaN pattern of {name}"
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{name}: max abs difference {err:.3e}")
    assert err <= ATOL, (name, err)


def _view(t):
    """A util.terrain.Terrain as the dict + sampler the hand cases and assert_terrain take."""
    d = dict(ix0=t.ix0, iy0=t.iy0, nx=t.nx, ny=t.ny, z=t.z.cpu().numpy(), state=t.state.cpu().numpy(), n_candidates=t.n_candidates.cpu().numpy())
    return d, lambda xy: t.sample(np.ascontiguousarray(xy, dtype=np.float64)).cpu().numpy()


def assert_terrain(t, want):
    got, _ = _view(t)
    for k in ("ix0", "iy0", "nx", "ny"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("n_candidates", "state"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    g = want["state"] == 1
    assert np.array_equal(got["z"][g], want["z"][g]), "ground cells"
    _close("z", got["z"], want["z"])


def assert_rows(t, xyz, want):
    """Sampled ground and height above ground of every row (xyz: a host array or a device tensor)."""
    host = xyz.cpu().numpy() if torch.is_tensor(xyz) else xyz
    _close("ground", t.sample(xyz).cpu().numpy(), ref.ground_at(want, np.asarray(host[:, 0], np.float64), np.asarray(host[:, 1], np.float64)))
    _close("height_above_ground", t.height_above_ground(xyz).cpu().numpy(), ref.height_above_ground(want, host))


def model(xyz, lab=None, **kw):
    from treelearn_amd.util.terrain import terrain_model
    return terrain_model(xyz, lab, **kw)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases_through_the_kernels(name):
    xyz, lab, params, check = cases.CASES[name]()
    t = model(xyz, lab, **params)
    check(*_view(t))
    want = ref.terrain_model(xyz, lab, **params)
    assert_terrain(t, want)
    assert_rows(t, xyz, want)


def test_empty_cloud_and_non_finite_rows():
    t = model(np.zeros((0, 3)))
    assert (t.nx, t.ny) == (0, 0) and tuple(t.z.shape) == (0, 0) and t.to_host()["z"].shape == (0, 0)
    assert np.isnan(t.sample(np.array([[1.0, 2.0]])).cpu().numpy()).all()
    xyz = cases.CASES["plane"]()[0]
    for col, bad in ((0, np.nan), (1, np.inf), (2, np.nan), (2, -np.inf)):
        b = xyz.copy()
        b[5, col] = bad
        with pytest.raises(ValueError, match="not finite"):
            model(b)
    with pytest.raises(ValueError, match="cells of 1e-06 m"):                        # the extent and the cell are named, nothing is allocated
        model(xyz, cell=1e-6)
    t = model(xyz)
    assert np.isnan(t.sample(np.array([[np.nan, 1.0], [1.0, np.inf]])).cpu().numpy()).all()


def _patch(rng, n, lx, ly):
    """n rows over lx x ly m: gentle noisy ground, a few rows 2 m up (stumps where they are alone in a cell), z quantised to 0.01."""
    x, y = rng.uniform(0, lx, n), rng.uniform(0, ly, n)
    z = 0.1 * x - 0.05 * y + rng.normal(0, 0.05, n) + 2.0 * (rng.uniform(size=n) < 0.05)
    return np.column_stack([x, y, np.round(z * 100) / 100])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts(n):
    xyz = _patch(np.random.default_rng(n), n, 4.0, 3.0)
    lab = (np.random.default_rng(n + 1).uniform(size=n) < 0.2).astype(np.int64) * 2
    for labels in (None, lab):
        want = ref.terrain_model(xyz, labels)
        t = model(xyz, labels)
        assert_terrain(t, want)
        assert_rows(t, xyz, want)


@pytest.mark.parametrize("lead", [0, 1, 37])
def test_wave_runs(lead):
    """64 consecutive rows in one cell next to 64 rows in 64 different cells, after `lead` rows elsewhere, so that the run starts on a
    wave boundary or straddles one: the run-aggregated and the one-lane-per-cell paths of tl_dtm_min."""
    rng = np.random.default_rng(5 + lead)
    one = np.column_stack([rng.uniform(2.0, 2.5, 64), rng.uniform(1.0, 1.5, 64), np.round(rng.normal(0, 0.1, 64), 2)])
    many = np.column_stack([0.25 + 0.5 * (np.arange(64) % 8), 0.25 + 0.5 * (np.arange(64) // 8), np.round(rng.normal(0, 0.1, 64), 2)])
    head = np.column_stack([rng.uniform(0, 4, lead), rng.uniform(0, 4, lead), np.zeros(lead)])
    xyz = np.concatenate([head, one, many])
    lab = np.zeros(len(xyz), np.int64)
    lab[lead + 10] = 4                                                   # a non-candidate splits the run
    for labels in (None, lab):
        want = ref.terrain_model(xyz, labels)
        assert want["n_candidates"].max() >= 63
        assert_terrain(model(xyz, labels), want)


@pytest.mark.parametrize("shape", [(70, 3), (3, 70)])
def test_long_thin_grids(shape):
    """70 x 3 and 3 x 70 cells: windows of the filter and the fill clipped at both short sides, holes wider than the grid is high."""
    nx, ny = shape
    rng = np.random.default_rng(nx)
    xyz = _patch(rng, 1500, nx * 0.5, ny * 0.5)
    long = xyz[:, 0] if nx > ny else xyz[:, 1]
    short = xyz[:, 1] if nx > ny else xyz[:, 0]
    xyz[(np.floor(long / 0.5) == 30) & (np.floor(short / 0.5) == 1), 2] += 2.0        # a stump: every row of one cell 2 m up
    xyz = xyz[~((long > 8) & (long < 11)) & ~((long > 20) & (long < 20.6))]
    corners = np.array([[0.0, 0.0, 0.0], [nx * 0.5 - 1e-9, ny * 0.5 - 1e-9, 0.0]])
    xyz = np.concatenate([xyz, corners])
    for kw in ({}, dict(window=4, fill_radius=2)):
        want = ref.terrain_model(xyz, None, **kw)
        assert (want["nx"], want["ny"]) == shape and (want["state"] == 2).any() + (want["state"] == 4).any() and (want["state"] == 3).any()
        t = model(xyz, None, **kw)
        assert_terrain(t, want)
        assert_rows(t, xyz, want)
    assert (want["state"] == 0).any()                                    # fill_radius = 2 leaves the 3 m gap partly unfilled


# ------------------------------------------------------------------ one cloud of about 2e5 rows over 40 x 30 m
TREE_SIZES = (1, 12, 13, 257, 800, 1500, 1500, 1500, 1500, 1500, 1500, 1500)
FOOT_TREE = 6                                                            # the tree whose foot rows are labelled 0


def _tree(rng, n, cx, cy, z0):
    """n rows of a tree at (cx, cy) standing on z0: a stem of full circles up to 2.5 m and a crown blob above it."""
    ns = n if n < 40 else int(0.4 * n)
    a = rng.uniform(0, 2 * np.pi, ns)
    r = rng.uniform(0.1, 0.3)
    stem = np.column_stack([cx + r * np.cos(a), cy + r * np.sin(a), z0 + rng.uniform(0.0, 2.5, ns)])
    nc = n - ns
    crown = np.column_stack([cx + rng.normal(0, 1.2, nc), cy + rng.normal(0, 1.2, nc), z0 + rng.uniform(2.5, 14.0, nc)])
    return np.concatenate([stem, crown])


def _big_cloud():
    rng = np.random.default_rng(17)
    n = 212_000
    x, y = rng.uniform(-20, 20, n), rng.uniform(-15, 15, n)
    surf = lambda x, y: 0.15 * x + 0.08 * y                               # noqa: E731
    z = surf(x, y) + rng.normal(0, 0.03, n)
    keep = x < 16.0                                                       # the strip beyond holds single-candidate cells only
    centres = [(-16.0 + 10.0 * (k % 4) + rng.uniform(-1, 1), -10.0 + 10.0 * (k // 4) + rng.uniform(-1, 1)) for k in range(12)]
    for cx, cy in centres:                                                # discs without ground under the trees
        keep &= (x - cx) ** 2 + (y - cy) ** 2 > 1.5 ** 2
    ci, cj = np.floor(x / 0.5), np.floor(y / 0.5)
    for si, sj in ((-30, -20), (-11, 7), (0, 0), (13, -28), (25, 21)):    # stumps: every row of the cell 2 m up
        z = z + 2.0 * ((ci == si) & (cj == sj))
    rows, lab = [np.column_stack([x, y, z])[keep]], [np.zeros(int(keep.sum()), np.int64)]
    sx, sy = rng.uniform(16.0, 20.0, 150), rng.uniform(-15, 15, 150)      # about one row per cell, most cells none
    rows.append(np.column_stack([sx, sy, surf(sx, sy)]))
    lab.append(np.zeros(150, np.int64))
    for t, ((cx, cy), size) in enumerate(zip(centres, TREE_SIZES), start=1):
        p = _tree(rng, size, cx, cy, surf(cx, cy))
        p[:, 0], p[:, 1] = np.clip(p[:, 0], -19.9, 19.9), np.clip(p[:, 1], -14.9, 14.9)         # crowns stay inside the plot
        l = np.full(size, t, np.int64)
        if t == FOOT_TREE:
            l[p[:, 2] < surf(cx, cy) + 0.5] = 0
        rows.append(p)
        lab.append(l)
    ux, uy = rng.uniform(-20, 20, 3000), rng.uniform(-15, 15, 3000)       # unassigned rows below the ground: never a minimum
    rows.append(np.column_stack([ux, uy, surf(ux, uy) - rng.uniform(0.5, 3.0, 3000)]))
    lab.append(np.full(3000, -1, np.int64))
    xyz, lab = np.concatenate(rows), np.concatenate(lab)
    xyz[:, 2] = np.round(xyz[:, 2] * 100) / 100                           # minima tie
    order = np.lexsort((np.floor(xyz[:, 0] / 0.5), np.floor(xyz[:, 1] / 0.5)))          # spatially sorted, as tiles and results come
    return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(lab[order])


@pytest.fixture(scope="module")
def big():
    xyz, lab = _big_cloud()
    x32 = xyz.astype(np.float32)
    want64, want32 = ref.terrain_model(xyz, lab), ref.terrain_model(x32, lab)
    s = want64["state"]
    assert 190_000 <= len(xyz) <= 210_000 and (want64["nx"], want64["ny"]) == (80, 60)
    assert all((s == k).any() for k in (1, 3, 4)) and (want64["n_candidates"] == 1).sum() >= 50
    return dict(lab=lab, f64=xyz, f32=x32, want64=want64, want32=want32)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("stride", [3, 4])
def test_big_cloud(big, dtype, stride):
    xyz, lab, want = big[dtype], big["lab"], big["want" + dtype[1:]]
    if stride == 4:
        wide = np.full((len(xyz), 4), 7.0, xyz.dtype)
        wide[:, :3] = xyz
        dev = torch.from_numpy(wide).cuda()[:, :3]
        assert dev.stride() == (4, 1)
        t = model(dev, torch.from_numpy(lab).cuda())
        assert_rows(t, dev, want)
    else:
        t = model(torch.from_numpy(xyz).cuda(), torch.from_numpy(lab).cuda())
        assert_rows(t, xyz, want)
        host = model(xyz, lab.astype(np.int32))                          # host arrays and device tensors: the same bits
        assert host.z.cpu().numpy().tobytes() == t.z.cpu().numpy().tobytes()
    assert_terrain(t, want)
    h = t.to_host()
    assert set(h) == {"x0", "y0", "cell", "z", "state", "n_candidates"} and h["x0"] == -20.0 and h["y0"] == -15.0 and h["cell"] == 0.5


def test_determinism_and_row_order(big):
    xyz, lab = big["f64"], big["lab"]
    a, b = model(xyz, lab), model(xyz, lab)
    p = np.random.default_rng(3).permutation(len(xyz))
    c = model(xyz[p], lab[p])
    for k in ("z", "state", "n_candidates"):
        ref_bits = getattr(a, k).cpu().numpy().tobytes()
        assert getattr(b, k).cpu().numpy().tobytes() == ref_bits, k     # bit-identical, NaN payloads included
        assert getattr(c, k).cpu().numpy().tobytes() == ref_bits, k     # and under a row permutation: every step is order-independent
    assert a.sample(xyz).cpu().numpy().tobytes() == b.sample(xyz).cpu().numpy().tobytes()
    assert c.height_above_ground(xyz[p]).cpu().numpy().tobytes() == a.height_above_ground(xyz).cpu().numpy()[p].tobytes()


def _assert_ground_columns(inv, want):
    from treelearn_amd.util.inventory import COLUMNS, GROUND_COLUMNS
    assert tuple(inv) == COLUMNS + GROUND_COLUMNS == inv_ref.COLUMNS + ref.GROUND_COLUMNS
    assert inv["dbh_ag_n"].dtype == want["dbh_ag_n"].dtype and np.array_equal(inv["dbh_ag_n"], want["dbh_ag_n"])
    for k in GROUND_CLOSE:
        _close(k, inv[k], want[k])


@pytest.mark.parametrize("fill_radius", [20, 1])
def test_tree_columns(big, fill_radius):
    """The eight ground columns of the big cloud's trees (1, 12, 13, 257 ... rows, standing on the slope over discs without ground; one
    with its foot rows labelled 0).  fill_radius = 1 leaves the middle of every disc without a value: trees there have NaN columns and
    dbh_ag_n = 0.  The sixteen columns of the same call are those of tree_inventory without a terrain, bit for bit."""
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    xyz, lab = big["f64"], big["lab"]
    off = np.array([500.0, -300.0, 120.0])
    t_ref = big["want64"] if fill_radius == 20 else ref.terrain_model(xyz, lab, fill_radius=1)
    want = ref.tree_inventory(xyz, lab, t_ref, offset=off)
    assert want["n_points"][:4].tolist() == list(TREE_SIZES[:4]) and want["n_points"][FOOT_TREE - 1] < TREE_SIZES[FOOT_TREE - 1]
    nan = np.isnan(want["z_ground"])
    assert (nan.any() and not nan.all() and (want["dbh_ag_n"][nan] == 0).all()) if fill_radius == 1 else not nan.any()
    assert np.isfinite(want["dbh_ag"]).sum() >= (1 if fill_radius == 1 else 6)
    t = model(torch.from_numpy(xyz).cuda(), torch.from_numpy(lab).cuda(), fill_radius=fill_radius)
    inv = tree_inventory(xyz, lab, offset=off, terrain=t)
    _assert_ground_columns(inv, want)
    plain = tree_inventory(xyz, lab, offset=off)
    assert tuple(plain) == COLUMNS
    for k in COLUMNS:
        assert inv[k].tobytes() == plain[k].tobytes(), k


def test_hand_tree_on_flat_ground():
    from treelearn_amd.util.inventory import tree_inventory
    xyz, lab, check = cases.tree_on_flat_ground()
    inv = tree_inventory(xyz, lab, terrain=model(xyz, lab))
    check(inv)
    _assert_ground_columns(inv, ref.tree_inventory(xyz, lab, ref.terrain_model(xyz, lab)))
    none = tree_inventory(xyz, lab, terrain=model(xyz, np.where(lab == 0, -1, lab)))
    assert none["dbh_ag_n"].tolist() == [0] and all(np.isnan(none[k][0]) for k in GROUND_CLOSE)


# ------------------------------------------------------------------ segment_forest, save_results, the command lines
def _small_plot():
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=24, voxel=0.1, n_trees=20, fill=0.10, seed=5)
    return t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])


@pytest.fixture(scope="module")
def segmented():
    """segment_forest on the small plot of tests/test_gpu_inventory.py with the pinned-head random model: once with terrain and inventory,
    once without any flag."""
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
        res = segment_forest(pts, m, grouping_cfg=cfg, return_type="original", inventory=True, terrain=True, terrain_cfg=dict(cell=1.0))
        plain = segment_forest(pts, m, grouping_cfg=cfg, return_type="original")
        with pytest.raises(ValueError):                                  # parameters are checked before any GPU work
            segment_forest(None, None, terrain=True, terrain_cfg=dict(cell=0.0))
    return pts, res, plain


def test_segment_forest_without_flags_returns_the_same_keys(segmented):
    _, res, plain = segmented
    assert set(plain) == {"coords", "labels", "categories"}
    assert set(res) == set(plain) | {"inventory", "terrain", "height_above_ground"}
    for k in plain:
        assert np.array_equal(plain[k], res[k]), k


def test_segment_forest_terrain_files_and_cli(segmented, tmp_path):
    """The terrain is computed in the centred frame and un-centred; the restatement is held to it in the same frame: the test centres
    the cloud as segment_forest does (the same torch expression on the same device)."""
    from treelearn_amd.util.inventory import cloud_inventory, write_inventory
    from treelearn_amd.util.segment import save_results
    from treelearn_amd.util.terrain import cloud_terrain
    pts, res, plain = segmented
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    centred, mean_h = (xyz - mean).cpu().numpy(), mean.cpu().numpy()
    assert np.array_equal((xyz - mean + mean).cpu().numpy(), res["coords"])
    want = ref.terrain_model(centred, res["labels"], cell=1.0)
    got = res["terrain"]
    assert set(got) == {"x0", "y0", "cell", "z", "state", "n_candidates"} and got["cell"] == 1.0
    assert got["x0"] == want["ix0"] * 1.0 + mean_h[0] and got["y0"] == want["iy0"] * 1.0 + mean_h[1]
    assert np.array_equal(got["state"], want["state"]) and np.array_equal(got["n_candidates"], want["n_candidates"])
    _close("terrain z", got["z"], want["z"] + mean_h[2])
    hag = res["height_above_ground"]
    assert hag.dtype == np.float64 and hag.shape == (len(res["coords"]),)
    _close("height_above_ground", hag, ref.height_above_ground(want, centred))
    _assert_ground_columns(res["inventory"], ref.tree_inventory(centred, res["labels"], want, offset=mean_h))

    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    with np.load(tmp_path / "api" / "terrain.npz") as f:
        assert set(f.files) == set(got) and all(np.array_equal(f[k], got[k], equal_nan=True) for k in got)
    assert np.array_equal(np.load(tmp_path / "api" / "height_above_ground.npy"), hag, equal_nan=True)
    rows = list(csv.reader(open(tmp_path / "api" / "tree_inventory.csv", newline="")))
    assert rows[0] == list(inv_ref.COLUMNS + ref.GROUND_COLUMNS) + ["category"] and len(rows) == 1 + len(res["categories"])
    save_results(plain, str(tmp_path / "plain"), "plot", ["npy"], save_treewise=False)
    assert not (tmp_path / "plain" / "terrain.npz").exists() and not (tmp_path / "plain" / "height_above_ground.npy").exists()

    # the two command lines in child processes on the saved N x 4 file, against the same calls made here
    forest = tmp_path / "api" / "full_forest" / "plot.npy"
    data = np.load(forest)
    env = dict(os.environ, PYTHONPATH=REPO)
    run = lambda *a: subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", *a], capture_output=True, text=True, cwd=REPO, env=env)  # noqa: E731
    p = run("treelearn_amd.util.terrain", "--forest", str(forest), "--out", str(tmp_path / "dtm.npz"), "--hag", str(tmp_path / "hag.npy"), "--cell", "1.0")
    assert p.returncode == 0 and "cells of 1.0 m" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    t, c = cloud_terrain(data, cell=1.0)
    h = t.to_host()
    with np.load(tmp_path / "dtm.npz") as f:
        assert set(f.files) == set(h) and all(np.array_equal(f[k], h[k], equal_nan=True) for k in h)
    cli_hag = np.load(tmp_path / "hag.npy")
    assert cli_hag.shape == (len(data), 4) and np.array_equal(cli_hag[:, :3], data[:, :3])
    assert np.array_equal(cli_hag[:, 3], t.height_above_ground(c).cpu().numpy(), equal_nan=True)
    p = run("treelearn_amd.util.inventory", "--forest", str(forest), "--out", str(tmp_path / "cli.csv"), "--terrain", "--cell", "1.0")
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    write_inventory(str(tmp_path / "want.csv"), cloud_inventory(data, terrain=True, terrain_cfg=dict(cell=1.0)))
    assert (tmp_path / "cli.csv").read_bytes() == (tmp_path / "want.csv").read_bytes()
    assert list(csv.reader(open(tmp_path / "cli.csv", newline="")))[0] == list(inv_ref.COLUMNS + ref.GROUND_COLUMNS)
