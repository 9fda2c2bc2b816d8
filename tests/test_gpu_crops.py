"""GPU tests of the random training-crop generator (util/crops.py, csrc/tl_crops.hip) and of CropDataset in a training step:
golden G15 (the reference's own generate_random_crops, tests/golden/make_golden_crops.py), each kernel against
tests/crops_restatement.py on larger inputs, one training step on generated crops, and the error paths."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crops_restatement as R
from treelearn_amd.util import crops as C

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 1e-9


def _sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_crops.npz"))


def _cfg(g):
    return dict(json.loads(str(g["cfg"])), **json.loads(str(g["sample"])))


def _prewrite(g, base):
    """The reference's cache directories as the golden generator wrote them (its open3d and jakteristics steps are skipped)."""
    os.makedirs(os.path.join(base, "forests"))
    vdir = os.path.join(base, f"forests_voxelized{_cfg(g)['voxel_size']}"); fdir = os.path.join(base, "features")
    os.makedirs(vdir); os.makedirs(fdir)
    for n in g["plots"]:
        np.savez_compressed(os.path.join(vdir, f"{n}.npz"), points=g[f"in/{n}/points"], labels=g[f"in/{n}/labels"])
        np.savez_compressed(os.path.join(fdir, f"{n}.npz"), features=g[f"in/{n}/features"])


def _ulps(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ============================================================================================ 1. golden G15, end to end
def test_generate_random_crops_matches_reference(g15, tmp_path):
    base = str(tmp_path)
    _prewrite(g15, base)
    written = C.generate_random_crops(base, _cfg(g15), seed=int(g15["seed"]))
    names = [str(n) for n in g15["crops"]]
    npz_dir, json_dir = os.path.join(base, "random_crops", "npz"), os.path.join(base, "random_crops", "json")
    assert sorted(os.listdir(npz_dir)) == sorted(n + ".npz" for n in names)
    assert sorted(os.listdir(json_dir)) == sorted(n + ".json" for n in names)
    assert sum(written.values()) == len(names) and written["plot_c"] == 0
    n_values = n_exact = n_rows = 0
    worst = 0
    for n in names:
        assert json.load(open(os.path.join(json_dir, n + ".json"))) == json.loads(str(g15[f"json/{n}"])), n
        d = np.load(os.path.join(npz_dir, n + ".npz"))
        assert list(d.keys()) == [str(k) for k in g15[f"keys/{n}"]], n
        for k in d.keys():
            assert d[k].dtype.str == str(g15[f"dtype/{n}/{k}"]) and list(d[k].shape) == list(g15[f"shape/{n}/{k}"]), (n, k)
        for k in ("feat", "instance_label", "center"):
            assert _sha1(d[k]) == str(g15[f"sha1/{n}/{k}"]), (n, k)
        assert _sha1(d["points"][:, 2]) == str(g15[f"sha1/{n}/z"]), n                 # z, row count and row order
        # rotated x / y: the reference's own expression on this host (its BLAS may fuse) vs the kernel's plain f64, one f32 ulp at most
        plot, k = n.rsplit("_", 1)
        ok = g15[f"stage/{plot}/filter"]; ind = g15[f"stage/{plot}/inds"][int(k)]
        c, r = g15[f"stage/{plot}/centers"][ok][ind], g15[f"stage/{plot}/rinv"][ok][ind]
        p = g15[f"in/{plot}/points"]
        a = (p[:, :2] - c) @ r.T
        ref = a[np.linalg.norm(a, ord=np.inf, axis=1) <= _cfg(g15)["chunk_size"] / 2].astype(np.float32)
        u = _ulps(d["points"][:, :2], ref)
        worst = max(worst, int(u.max(initial=0)))
        n_values += u.size; n_exact += int((u == 0).sum()); n_rows += len(ref)
        if f"full/{n}/points" in g15.files:
            assert _ulps(d["points"][:, :2], g15[f"full/{n}/points"][:, :2]).max(initial=0) <= 1, n
            assert np.array_equal(d["feat"], g15[f"full/{n}/feat"]) and np.array_equal(d["instance_label"], g15[f"full/{n}/instance_label"])
    print(f"\nG15: {len(names)} crops, {n_rows} rows; rotated x/y values not bit-identical to the reference expression: "
          f"{n_values - n_exact} of {n_values} (max {worst} ulp)")
    assert worst <= 1
    # occupancy grids as written to the cache: bit-identical to the reference's
    for plot in g15["plots"]:
        grid = np.load(os.path.join(base, "occupancy", f"{plot}.npz"))["occupancy_grid"]
        ref = g15[f"stage/{plot}/grid"]
        assert grid.dtype == ref.dtype and np.array_equal(grid, ref), plot


def test_stages_match_reference_grids_and_filter(g15):
    """Raw and filled grids from the reference's random stream, and the candidate filter from its candidates, bit for bit."""
    cfg = _cfg(g15)
    rs = np.random.RandomState(int(g15["seed"]))
    for plot in g15["plots"]:
        o = C.occupancy_grid(g15[f"in/{plot}/points"], g15[f"in/{plot}/labels"], rs, cfg["occupancy_res"], cfg["n_points_to_calculate_occupancy"],
                             cfg["how_far_fill"], cfg["min_percent_occupied_fill"])
        assert np.array_equal(o["raw"], g15[f"stage/{plot}/raw"]) and np.array_equal(o["filled"], g15[f"stage/{plot}/filled"]), plot
        assert np.array_equal(o["grid"], g15[f"stage/{plot}/grid"]), plot
        sums, ok = C.check_occupancy(g15[f"stage/{plot}/grid"], g15[f"stage/{plot}/centers"], g15[f"stage/{plot}/rinv"], cfg["chunk_size"],
                                     cfg["occupancy_res"], cfg["min_percent_occupied_choose"])
        assert np.array_equal(ok, g15[f"stage/{plot}/filter"]), plot


# ============================================================================================ 2. kernels vs restatement
def _steps(lo, n, h):
    return lo + h * np.arange(n + 1, dtype=np.float64)


def test_occupancy_and_fill_vs_restatement():
    from treelearn_amd import _hip
    rng = np.random.default_rng(151)
    X = Y = 200
    xs, ys = _steps(100.0, X, 0.37), _steps(-20.0, Y, 0.41)
    n = 1_000_000
    xy = np.stack([rng.uniform(xs[0] - 1, xs[-1] + 1, n), rng.uniform(ys[0] - 1, ys[-1] + 1, n)], 1).astype(np.float32)
    # exactly on (f32-representable) step values, on steps[0], beyond steps[-1]
    xs[::7] = xs[::7].astype(np.float32); ys[::5] = ys[::5].astype(np.float32)
    m = 20000
    xy[:m, 0] = xs[rng.integers(0, X + 1, m)].astype(np.float32); xy[:m, 1] = ys[rng.integers(0, Y + 1, m)].astype(np.float32)
    xy[m:m + 500, 0] = np.float32(xs[0]); xy[m + 500:m + 1000, 1] = np.float32(ys[0])
    xy[m + 1000:m + 1500, 0] = np.nextafter(np.float32(xs[-1]), np.float32(np.inf))
    xy[m + 1500:m + 1600] = np.float32(np.nan)
    exact = np.isin(xy[:m, 0].astype(np.float64), xs).sum()
    assert exact > 1000                                                              # the boundary rows are really on step values
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    L = _hip.lib()
    g = torch.empty((X, Y), dtype=torch.uint8, device="cuda")
    dxy, dxs, dys = dev(xy, torch.float32), dev(xs, torch.float64), dev(ys, torch.float64)
    _hip.check(L.tl_crops_occupancy(_hip.ptr(dxy), n, _hip.ptr(dxs), X, _hip.ptr(dys), Y, _hip.ptr(g), _hip.stream()), "occ")
    raw = g.cpu().numpy()
    ref = R.occupancy(xy, xs, ys, X, Y)
    assert np.array_equal(raw, ref)
    # a sparse grid so that filling decides many cells
    sparse = (rng.uniform(size=(X, Y)) < 0.8).astype(np.uint8)
    dsp = dev(sparse, torch.uint8)
    for h in (0, 3, 9):
        for pct in (0.9, 0.5):
            f = torch.empty_like(g)
            _hip.check(L.tl_crops_fill(_hip.ptr(dsp), X, Y, h, pct, _hip.ptr(f), _hip.stream()), "fill")
            assert np.array_equal(f.cpu().numpy(), R.fill(sparse, h, pct)), (h, pct)


def _rinv(angles):
    return C.inverse_rotations(np.asarray(angles, np.float64))


def test_check_occupancy_vs_restatement():
    rng = np.random.default_rng(152)
    X = Y = 200
    xs, ys = _steps(300.0, X, 1.0), _steps(-50.0, Y, 1.0)
    cxs, cys = C.cell_centres(xs, X), C.cell_centres(ys, Y)
    occ = (rng.uniform(size=(X, Y)) < 0.6).astype(np.float64)
    grid = np.ones((X, Y, 3)) * 10
    grid[:, :, 0] = cxs[:, None]; grid[:, :, 1] = cys[None, :]; grid[:, :, 2] = occ
    k = 5000
    centres = np.round(np.stack([rng.uniform(xs[0], xs[-1], k), rng.uniform(ys[0], ys[-1], k)], 1).astype(np.float32), 2)
    angles = np.round(rng.uniform(0, 2 * np.pi, k), 2)
    angles[:4] = [0.0, np.pi / 2, np.pi, 2 * np.pi - 0.01]
    rinv = _rinv(angles)
    chunk, res, pct = 35, 1, 0.45
    sums, ok = C.check_occupancy(grid, centres, rinv, chunk, res, pct)
    rs, rok, band = R.check(cxs, cys, occ, centres, rinv, chunk, (chunk / res) ** 2, pct)
    print(f"\ncheck_occupancy: {k} candidates x {X * Y} cells, (cell, candidate) pairs within 1e-9 m of the edge: {band}")
    assert np.array_equal(sums, rs) and np.array_equal(ok, rok)
    assert 0 < ok.sum() < k


def test_extract_crops_vs_restatement():
    rng = np.random.default_rng(153)
    n = 1_000_000
    xyz = np.stack([rng.uniform(500, 600, n), rng.uniform(-40, 60, n), rng.uniform(0, 30, n)], 1)
    xyz = np.round(xyz, 2).astype(np.float32)
    labels = rng.integers(-1, 40, n).astype(np.float32)
    feats = np.stack([np.arange(n, dtype=np.float32), rng.uniform(0, 1, n).astype(np.float32)], 1)      # column 0 = source row
    nc = 40                                                                                             # two batches: 32 + 8
    centres = np.round(np.stack([rng.uniform(520, 580, nc), rng.uniform(-20, 40, nc)], 1).astype(np.float32), 2)
    angles = np.round(rng.uniform(0, 2 * np.pi, nc), 2)
    angles[:4] = [0.0, np.pi / 2, np.pi, 2 * np.pi - 0.01]
    centres[4] = xyz[123, :2]                                                                           # a centre on a point
    rinv = _rinv(angles)
    chunk = 35
    out = list(C.extract_crops(xyz, labels, feats, centres, rinv, chunk))
    assert len(out) == nc
    in_band = 0
    for c in range(nc):
        member, u, v, d = R.crop(xyz, centres[c], rinv[c], chunk)
        band = np.abs(d - chunk / 2) < BAND
        in_band += int(band.sum())
        pts, lab, ft = out[c]
        rows = ft[:, 0].astype(np.int64)
        assert np.all(np.diff(rows) > 0), c                                                             # plot row order
        got = np.zeros(n, bool); got[rows] = True
        assert np.array_equal(got[~band], member[~band]), c
        assert np.array_equal(pts[:, 0], u[rows].astype(np.float32)) and np.array_equal(pts[:, 1], v[rows].astype(np.float32)), c
        assert np.array_equal(pts[:, 2], xyz[rows, 2]) and np.array_equal(ft, feats[rows]), c
        assert lab.dtype == np.int32 and np.array_equal(lab, labels[rows].astype(np.int32)), c
    print(f"\nextract_crops: {nc} crops of {n} points, rows within 1e-9 m of the edge: {in_band}")


# ============================================================================================ 2b. voxelization in the generator's order
def _clustered_cloud(seed=21):
    """Several points per 0.1 m voxel at large coordinates, so that voxel means fall near 2-decimal rounding boundaries."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 1, size=(30000, 3)) * np.array([30.0, 30.0, 4.0])
    pts = np.repeat(base, 4, axis=0) + rng.uniform(-0.04, 0.04, size=(120000, 3))
    pts += np.array([431.77, -212.33, 5.0])
    lab = np.repeat(rng.integers(-1, 12, size=30000), 4).astype(np.float64)
    return np.hstack([pts, lab[:, None]])


def test_voxelize_round_first_vs_restatement(tmp_path):
    """prepare.voxelize(round_first=True) and the forests_voxelized<v>/ file generate_random_crops writes equal the generator's
    np.round(<f64 voxel means>, 2).astype(np.float32), bit for bit for points and labels; the cloud has voxels where that order and
    the default one (float32 first, then rounded) differ, so the test tells the two apart."""
    from treelearn_amd.util.prepare import voxelize
    data = _clustered_cloud()
    means, other = R.voxel_means(data, 0.1)
    want = np.round(means, 2).astype(np.float32)
    default = np.round(means.astype(np.float32), 2)
    differ = int(np.any(want != default, axis=1).sum())
    print(f"\nvoxelize: {len(want)} voxels, {differ} differ between round-then-cast and cast-then-round")
    assert differ > 0
    out, _ = voxelize(data, 0.1, round_first=True)
    out = out.cpu().numpy()
    assert out.shape == (len(want), 4)
    assert np.array_equal(out[:, :3].astype(np.float32), want) and np.array_equal(out[:, :3], want.astype(np.float64))
    assert np.array_equal(out[:, 3], other[:, 0])
    out_default, _ = voxelize(data, 0.1)
    assert np.array_equal(out_default.cpu().numpy()[:, :3].astype(np.float32), default)
    # the cache file the generator writes from the same cloud
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "forests"))
    np.save(os.path.join(base, "forests", "cloud.npy"), data)
    C.generate_random_crops(base, dict(chunk_size=10, n_samples_total=2, n_points_to_calculate_occupancy=5000, how_far_fill=2), seed=0)
    f = np.load(os.path.join(base, "forests_voxelized0.1", "cloud.npz"))
    assert f["points"].dtype == np.float32 and f["labels"].dtype == np.float32
    assert np.array_equal(f["points"], want) and np.array_equal(f["labels"], np.round(other[:, 0], 2).astype(np.float32))


# ============================================================================================ 3. one training step on generated crops
def _write_forest(base, extent=30.0, seed=5, name="synthetic_plot"):
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=extent, voxel=0.2, n_trees=int(extent * extent / 60), seed=seed)
    p = t["points"].astype(np.float64) + np.array([250.0, -140.0, 3.0])
    lab = t["instance_label"].astype(np.float64)
    lab[np.random.default_rng(seed).uniform(size=len(lab)) < 0.05] = -1
    os.makedirs(os.path.join(base, "forests"), exist_ok=True)
    np.save(os.path.join(base, "forests", f"{name}.npy"), np.hstack([p, lab[:, None]]))


def test_generated_crops_train_one_step(tmp_path):
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import random_state_dict
    from treelearn_amd.util.dataset import ALL_AUGMENTATIONS, CropDataset, collate
    base = str(tmp_path)
    _write_forest(base)
    written = C.generate_random_crops(base, dict(chunk_size=15, n_samples_total=4, n_points_to_calculate_occupancy=20000, how_far_fill=3), seed=3)
    assert sum(written.values()) == 4
    for d in ("forests_voxelized0.1", "features", "occupancy"):
        assert os.listdir(os.path.join(base, d)) == ["synthetic_plot.npz"]
    ds = CropDataset(os.path.join(base, "random_crops", "npz"), 8, True, ALL_AUGMENTATIONS, seed=0)
    batch = collate([ds[0], ds[1]])
    assert batch["batch_size"] == 2 and batch["masks_off"].any()
    model = TreeLearn(use_feats=False, use_coords=False, spatial_shape=[500, 500, 1000], voxel_size=0.1, compute_dtype=torch.float32)
    model.load_state_dict(random_state_dict(7, channels=32, num_blocks=7), strict=True)
    model = model.cuda().train()
    loss, ld = model(batch, return_loss=True)
    loss.backward()
    assert torch.isfinite(loss.detach()).item()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


# ============================================================================================ 4. arguments and errors
def test_error_paths(tmp_path):
    for k in ("n_neigh_sor", "multiplier_sor", "rad", "npoints_rad"):
        with pytest.raises(NotImplementedError, match=k):
            C.generate_random_crops(str(tmp_path), {k: 1.0})
    base = str(tmp_path / "nolabels")
    os.makedirs(os.path.join(base, "forests"))
    p = np.random.default_rng(0).uniform(0, 20, size=(5000, 3))
    np.save(os.path.join(base, "forests", "unlabelled.npy"), np.hstack([p, -np.ones((5000, 1))]))
    with pytest.raises(ValueError, match="no valid points"):
        C.generate_random_crops(base, dict(chunk_size=10, n_samples_total=2, n_points_to_calculate_occupancy=100))
    base = str(tmp_path / "narrow")
    os.makedirs(os.path.join(base, "forests"))
    p = np.random.default_rng(1).uniform(0, 1, size=(5000, 3)) * np.array([20.0, 0.5, 5.0])
    np.save(os.path.join(base, "forests", "narrow.npy"), np.hstack([p, np.ones((5000, 1))]))
    with pytest.raises(ValueError, match="occupancy_res"):
        C.generate_random_crops(base, dict(chunk_size=10, n_samples_total=2, n_points_to_calculate_occupancy=100))


def test_cli_writes_the_expected_files(tmp_path):
    base = str(tmp_path)
    _write_forest(base, extent=20.0, seed=9, name="tiny")
    r = subprocess.run([sys.executable, "-m", "treelearn_amd.util.crops", "--base-dir", base, "--seed", "4", "--n-samples-total", "3",
                        "--chunk-size", "10", "--n-points-to-calculate-occupancy", "5000", "--how-far-fill", "2"],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    npz = sorted(os.listdir(os.path.join(base, "random_crops", "npz"))); js = sorted(os.listdir(os.path.join(base, "random_crops", "json")))
    assert npz == [f"tiny_{k}.npz" for k in range(3)] and js == [f"tiny_{k}.json" for k in range(3)]
    meta = json.load(open(os.path.join(base, "random_crops", "json", "tiny_0.json")))
    assert meta["chunk_size"] == 10 and meta["how_far_fill"] == 2 and meta["n_neigh_sor"] is None
