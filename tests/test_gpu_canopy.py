"""GPU tests of the canopy height model (csrc/tl_canopy.hip, util/canopy.py) against the numpy restatement of
tests/canopy_restatement.py.

Bounds.  Grid shapes and origins, n, n_veg, layers, n_no_ground, n_clipped, top, owner, state, chm, the tops mask and list,
tops_per_tree, h_max, cover, every percentile and every NaN pattern are compared exactly, dtype included: maxima, comparisons, integer
counts, the median of at most 8 values and single divisions do not depend on a summation order, and the interpolation is one fixed
expression under the contract.  h_mean and h_sd are compared to 1e-9 absolute: the formulas are identical and only the order of f64
sums can differ; for at most 2e4 terms of magnitude <= 50 m that is at most 2e4 * 1.1e-16 * 50, about 1.1e-10 on a mean (the reasoning
of §16).  No metrics cell of these tests holds more than 2e4 rows."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import canopy_cases as cases
import canopy_restatement as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9
SCALARS = ("ix0", "iy0", "nx", "ny", "metric_ix0", "metric_iy0", "metric_nx", "metric_ny", "n_no_ground", "n_clipped")
EXACT = ("n", "top", "owner", "state", "chm", "tops_mask", "metric_n", "metric_n_veg", "cover", "h_max", "percentiles", "layers")
CLOSE = ("h_mean", "h_sd")
DEVICE_ARRAYS = EXACT + CLOSE


def model(xyz, h, lab=None, **kw):
    from treelearn_amd.util.canopy import canopy_model
    return canopy_model(xyz, labels=lab, height_above_ground=h, **kw)


def _view(c):
    """A util.canopy.Canopy as the dict the hand cases and the restatement use."""
    d = {k: getattr(c, k) for k in SCALARS}
    d.update({k: getattr(c, k).cpu().numpy() for k in DEVICE_ARRAYS})
    d["tops"] = {k: v.cpu().numpy() for k, v in c.tops.items()}
    if c.tops_per_tree is not None:
        d["tops_per_tree"] = c.tops_per_tree.cpu().numpy()
    return d


def _exact(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), name


def assert_canopy(c, want):
    got = _view(c)
    for k in SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in EXACT:
        _exact(k, got[k], want[k])
    assert set(got["tops"]) == set(want["tops"]) == {"i", "j", "x", "y", "h", "owner"}
    for k in want["tops"]:
        _exact("tops " + k, got["tops"][k], want["tops"][k])
    assert ("tops_per_tree" in got) == ("tops_per_tree" in want)
    if "tops_per_tree" in want:
        _exact("tops_per_tree", got["tops_per_tree"], want["tops_per_tree"])
    for k in CLOSE:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"NaN pattern of {k}"
        ok = ~np.isnan(want[k])
        err = float(np.abs(got[k][ok] - want[k][ok]).max()) if ok.any() else 0.0
        print(f"{k}: max abs difference {err:.3e}")
        assert err <= ATOL, (k, err)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases_through_the_kernels(name):
    from treelearn_amd.util.canopy import canopy_model
    from treelearn_amd.util.terrain import terrain_model
    case = cases.CASES[name]()
    xyz, lab = case["xyz"], case["labels"]
    if case["terrain_cfg"] is None:
        h = case["h"]
        c = model(xyz, h, lab, **case["params"])
    else:
        t = terrain_model(xyz, lab, **case["terrain_cfg"])
        h = t.height_above_ground(xyz).cpu().numpy()
        c = canopy_model(xyz, t, lab, **case["params"])
    case["check"](_view(c))
    assert_canopy(c, ref.canopy_model(xyz, h, lab, **case["params"]))


# ------------------------------------------------------------------ a random cloud of about 20 000 rows over 12 x 9 m
PARAMS = dict(cell=0.5, metric_cell=4.0)


def _random_cloud():
    rng = np.random.default_rng(22)
    n = 20_000
    x, y = rng.uniform(0.0, 12.0, n), rng.uniform(0.0, 9.0, n)
    x[:2], y[:2] = (0.0, 11.999), (0.0, 8.999)                            # the grid is 24 x 18 cells whatever the rounding to f32 does
    crown = 6.0 + 18.0 * np.exp(-((x % 4.0 - 2.0) ** 2 + (y % 4.5 - 2.25) ** 2) / 1.5)
    h = np.where(rng.uniform(size=n) < 0.3, rng.uniform(0.0, 1.0, n), crown * rng.uniform(0.2, 1.0, n) ** 0.3)
    h = np.clip(np.round(h * 100) / 100, 0.0, 30.0)                       # maxima tie
    h[rng.choice(n, 12, replace=False)] = -np.round(rng.uniform(0.01, 0.4, 12) * 100) / 100
    pit = (np.floor(x / 0.5) == 9) & (np.floor(y / 0.5) == 7)             # a pit: every row of one cell near the ground
    h[pit] = np.minimum(h[pit], 0.5)
    hole = (np.floor(x / 0.5) == 15) & (np.floor(y / 0.5) == 4)           # a hole: no ground under one cell
    h[hole] = np.nan
    h[rng.choice(n, 30, replace=False)] = np.nan
    lab = rng.integers(0, 7, n).astype(np.int64)
    xyz = np.column_stack([x, y, h + 100.0])
    order = np.lexsort((np.floor(x / 0.5), np.floor(y / 0.5)))            # spatially sorted, as tiles and results come
    return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(h[order]), np.ascontiguousarray(lab[order])


@pytest.fixture(scope="module")
def cloud():
    xyz, h, lab = _random_cloud()
    x32 = xyz.astype(np.float32)
    want64, want32 = ref.canopy_model(xyz, h, lab, **PARAMS), ref.canopy_model(x32, h, lab, **PARAMS)
    assert (want64["nx"], want64["ny"], want64["metric_nx"], want64["metric_ny"]) == (24, 18, 3, 3) and want64["metric_n"].max() <= 20_000
    assert all((want64["state"] == k).any() for k in (1, 2, 3)) and len(want64["tops"]["h"]) >= 4 and want64["n_no_ground"] >= 30
    assert (want64["tops_per_tree"] > 0).any() and want64["layers"][:, :, 0].min() > 0
    return dict(xyz=xyz, x32=x32, h=h, lab=lab, want64=want64, want32=want32)


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_random_cloud(cloud, dtype, stride, order):
    xyz, want = (cloud["xyz"], cloud["want64"]) if dtype == "f64" else (cloud["x32"], cloud["want32"])
    h, lab = cloud["h"], cloud["lab"]
    if order == "shuffled":
        p = np.random.default_rng(4).permutation(len(h))
        xyz, h, lab = xyz[p], h[p], lab[p]
    if stride == 4:
        wide = np.full((len(xyz), 4), 7.0, xyz.dtype)
        wide[:, :3] = xyz
        dev = torch.from_numpy(wide).cuda()[:, :3]
        assert dev.stride() == (4, 1)
    else:
        dev = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    c = model(dev, torch.from_numpy(h).cuda(), torch.from_numpy(lab).cuda(), **PARAMS)
    assert_canopy(c, want)
    if stride == 3 and order == "sorted":
        host = model(xyz, h, lab.astype(np.int32), **PARAMS)              # host arrays and device tensors: the same bits
        assert host.h_mean.cpu().numpy().tobytes() == c.h_mean.cpu().numpy().tobytes()
        nolab = model(dev, h, None, **PARAMS)
        assert nolab.tops_per_tree is None and bool((nolab.owner == -1).all()) and nolab.chm.cpu().numpy().tobytes() == c.chm.cpu().numpy().tobytes()


def test_row_order_does_not_change_a_bit(cloud):
    xyz, h, lab = cloud["xyz"], cloud["h"], cloud["lab"]
    p = np.random.default_rng(9).permutation(len(h))
    a, b = model(xyz, h, lab, **PARAMS), model(xyz[p], h[p], lab[p], **PARAMS)
    for k in DEVICE_ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), k          # NaN payloads included
        if x.is_floating_point():                                         # (torch.equal takes a NaN as unequal to itself)
            assert torch.equal(torch.isnan(x), torch.isnan(y)), k
            x, y = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
        assert torch.equal(x, y), k
    for k in a.tops:
        assert torch.equal(a.tops[k], b.tops[k]), k
    assert torch.equal(a.tops_per_tree, b.tops_per_tree) and (a.n_no_ground, a.n_clipped) == (b.n_no_ground, b.n_clipped)


@pytest.mark.parametrize("lead", [0, 1, 37])
def test_wave_runs(lead):
    """64 consecutive rows in one cell, 64 rows in 64 different cells and 64 rows that alternate between two cells, after `lead` rows
    elsewhere, so that the run starts on a wave boundary or straddles one: the run-aggregated and the one-lane-per-cell paths of
    tl_chm_max.  A row without a height splits the run."""
    rng = np.random.default_rng(5 + lead)
    hq = lambda m: np.round(rng.uniform(0.0, 20.0, m), 1)                 # noqa: E731
    one = np.column_stack([rng.uniform(2.0, 2.5, 64), rng.uniform(1.0, 1.5, 64)])
    many = np.column_stack([0.25 + 0.5 * (np.arange(64) % 8), 0.25 + 0.5 * (np.arange(64) // 8)])
    alt = np.column_stack([3.25 + 0.5 * (np.arange(64) % 2), np.full(64, 3.75)])
    head = np.column_stack([rng.uniform(0, 4, lead), rng.uniform(0, 4, lead)])
    xy = np.concatenate([head, one, many, alt])
    h = hq(len(xy))
    h[lead + 10] = np.nan
    lab = rng.integers(0, 4, len(xy)).astype(np.int64)
    xyz = np.column_stack([xy, h])
    want = ref.canopy_model(xyz, h, lab, top_window=1)
    assert want["n"].max() >= 63 and want["n_no_ground"] == 1
    assert_canopy(model(xyz, h, lab, top_window=1), want)


def test_range_sizes_of_the_metrics_cells():
    """Metrics cells of 1, 2, 63, 64, 65, 257 and 5 000 rows in one cloud (and one without a row): one cell loops the workgroup of 256
    threads several times, others leave most of its lanes idle."""
    rng = np.random.default_rng(8)
    sizes = (1, 2, 63, 64, 0, 65, 257, 5000)
    x = np.concatenate([rng.uniform(k, k + 1.0, m) for k, m in enumerate(sizes)])
    y = rng.uniform(0.0, 1.0, len(x))
    h = np.round(rng.uniform(0.0, 40.0, len(x)), 2)
    x[0], y[0] = 0.0, 0.0                                                 # the grid starts at 0
    p = rng.permutation(len(x))
    xyz, h = np.column_stack([x, y, h])[p], h[p]
    kw = dict(metric_cell=1.0, percentiles=(0, 1, 33.3, 50, 99.9, 100), layer=0.5, max_layers=70)
    want = ref.canopy_model(xyz, h, None, **kw)
    assert want["metric_n"].tolist() == [list(sizes)] and want["n_clipped"] > 0 and want["layers"].shape == (1, 8, 70)
    assert_canopy(model(xyz, h, None, **kw), want)


def test_empty_cloud_and_refused_inputs():
    from treelearn_amd.util.canopy import stand_summary
    c = model(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int64))
    assert_canopy(c, ref.canopy_model(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int64)))
    host = c.to_host()
    assert host["chm"].shape == (0, 0) and host["layers"].shape == (0, 0, 1) and host["tops_x"].shape == (0,)
    s = stand_summary(c)
    assert s["area_ha"] == 0.0 and s["n_tops"] == 0 and np.isnan(s["canopy_cover"])
    case = cases.CASES["flat"]()
    xyz, h = case["xyz"], case["h"]
    for what, col, bad in (("xyz", 0, np.nan), ("xyz", 1, np.inf), ("h", None, np.inf), ("h", None, -np.inf)):
        b, bh = xyz.copy(), h.copy()
        if what == "xyz":
            b[5, col] = bad
        else:
            bh[5] = bad
        with pytest.raises(ValueError, match="not finite"):
            model(b, bh)
    free = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=r"2 x 2 m: \d+ x \d+ CHM cells of 1e-06 m"):   # the extent and the cell are named
        model(xyz, h, cell=1e-6)
    with pytest.raises(ValueError, match="metrics cells of 1e-06 m"):
        model(xyz, h, metric_cell=1e-6)
    assert torch.cuda.memory_allocated() <= free + (1 << 20)                         # no grid of 2e12 cells was allocated
    with pytest.raises(ValueError, match="one of the two"):
        from treelearn_amd.util.canopy import canopy_model
        canopy_model(xyz)


def test_c_entry_points_null_and_zero_size():
    from treelearn_amd import _hip
    L, P = _hip.lib(), _hip.ptr
    dev = "cuda"
    pts = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    h = torch.zeros(4, dtype=torch.float64, device=dev)
    lab = torch.zeros(4, dtype=torch.int64, device=dev)
    keys = torch.full((4,), 7, dtype=torch.int64, device=dev)
    i32 = torch.full((8,), 7, dtype=torch.int32, device=dev)
    f64 = torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    u8 = torch.full((4,), 7, dtype=torch.uint8, device=dev)
    start = torch.zeros(2, dtype=torch.int64, device=dev)
    q = (ctypes.c_double * 1)(50.0)
    s = _hip.stream()
    ERR = _hip.TL_ERR_ARG
    # null pointers for required arrays
    assert L.tl_chm_max(None, 1, 3, 4, P(h), 0.5, 0, 0, 2, 2, P(keys), P(i32), P(i32), s) == ERR
    assert L.tl_chm_max(P(pts), 1, 3, 4, None, 0.5, 0, 0, 2, 2, P(keys), P(i32), P(i32), s) == ERR
    assert L.tl_chm_max(P(pts), 1, 3, 4, P(h), 0.5, 0, 0, 2, 2, None, P(i32), P(i32), s) == ERR
    assert L.tl_chm_owner(P(pts), 1, 3, 4, P(h), None, 0.5, 0, 0, 2, 2, P(keys), P(i32), P(i32), s) == ERR
    assert L.tl_chm_pits(None, 2, 2, 2.0, 5, P(f64), P(f64[8:]), P(u8), s) == ERR
    assert L.tl_chm_pits(P(keys), 2, 2, 2.0, 10, P(f64), P(f64[8:]), P(u8), s) == ERR
    assert L.tl_chm_tops(P(f64), 2, 2, 1, 5.0, None, s) == ERR
    assert L.tl_chm_tops(P(f64), 2, 2, 0, 5.0, P(u8), s) == ERR
    assert L.tl_canopy_keys(P(pts), 1, 3, 4, P(h), 0.5, 0, 0, 2, 2, None, P(i32), s) == ERR
    assert L.tl_canopy_keys(P(pts), 1, 3, 4, P(h), 0.0, 0, 0, 2, 2, P(keys), P(i32), s) == ERR
    assert L.tl_grid_metrics(P(h), 4, P(start), 1, 2.0, None, 1, 1.0, 1, P(f64), P(i32), P(i32[4:]), P(i32[6:]), s) == ERR
    assert L.tl_grid_metrics(P(h), 4, P(start), 1, 2.0, q, 1, 1.0, 257, P(f64), P(i32), P(i32[4:]), P(i32[6:]), s) == ERR
    assert L.tl_chm_max(P(pts), 1, 3, 4, P(h), 0.5, 0, 0, 0, 0, P(keys), P(i32), P(i32), s) == ERR          # rows without a grid
    # zero sizes: TL_OK without a launch, the arrays keep their 7s
    assert L.tl_chm_max(P(pts), 1, 3, 0, P(h), 0.5, 0, 0, 0, 0, P(keys), P(i32), P(i32[4:]), s) == 0
    assert L.tl_chm_owner(P(pts), 1, 3, 0, P(h), P(lab), 0.5, 0, 0, 0, 0, P(keys), P(i32), P(i32[6:]), s) == 0
    assert L.tl_chm_pits(P(keys), 0, 5, 2.0, 5, P(f64), P(f64[8:]), P(u8), s) == 0
    assert L.tl_chm_tops(P(f64), 5, 0, 1, 5.0, P(u8), s) == 0
    assert L.tl_canopy_keys(P(pts), 1, 3, 0, P(h), 0.5, 0, 0, 2, 2, P(keys), P(i32), s) == 0
    assert L.tl_grid_metrics(P(h), 0, P(start), 0, 2.0, q, 1, 1.0, 1, P(f64), P(i32), P(i32[2:]), P(i32[6:]), s) == 0
    torch.cuda.synchronize()
    assert keys.tolist() == [7] * 4 and f64.tolist() == [7.0] * 16 and u8.tolist() == [7] * 4
    assert i32.tolist() == [7, 7, 7, 7, 0, 0, 0, 7]                                   # flags and *n_clipped are cleared, nothing else


def test_row_kernels_skip_and_flag_what_they_refuse():
    """The device side of the refusals, which canopy_model's host checks come before: a row with a NaN x, an infinite h or a cell outside
    the grid is skipped by tl_chm_max, tl_chm_owner and tl_canopy_keys and sets the flag; a NaN h is skipped and counted."""
    from treelearn_amd import _hip
    L, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    nan, inf = float("nan"), float("inf")
    pts = torch.tensor([[0.1, 0.1, 0.0], [nan, 0.1, 0.0], [0.2, 0.2, 0.0], [5.0, 0.1, 0.0], [0.6, 0.7, 0.0], [0.7, 0.6, 0.0], [0.1, -0.2, 0.0]],
                       dtype=torch.float64, device="cuda")
    h = torch.tensor([1.0, 2.0, inf, 3.0, nan, 4.0, 5.0], dtype=torch.float64, device="cuda")
    lab = torch.tensor([3, 9, 9, 9, 9, 1 << 40, 9], dtype=torch.int64, device="cuda")
    keys = torch.full((2, 2), 7, dtype=torch.int64, device="cuda")
    count = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
    owner = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
    flags = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    assert L.tl_chm_max(P(pts), 1, 3, 7, P(h), 0.5, 0, 0, 2, 2, P(keys), P(count), P(flags), s) == 0
    assert flags.tolist() == [1, 1] and count.tolist() == [[1, 0], [0, 1]]
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.tl_chm_owner(P(pts), 1, 3, 7, P(h), P(lab), 0.5, 0, 0, 2, 2, P(keys), P(owner), P(err), s) == 0
    assert owner.tolist() == [[3, -1], [-1, -1]] and err.item() == 1                  # the label beyond 32 bits owns nothing and is flagged
    top, chm = torch.empty((2, 2), dtype=torch.float64, device="cuda"), torch.empty((2, 2), dtype=torch.float64, device="cuda")
    state = torch.empty((2, 2), dtype=torch.uint8, device="cuda")
    assert L.tl_chm_pits(P(keys), 2, 2, 2.0, 5, P(top), P(chm), P(state), s) == 0
    assert np.array_equal(top.cpu().numpy(), [[1.0, nan], [nan, 4.0]], equal_nan=True) and state.tolist() == [[1, 0], [0, 1]]
    mkeys = torch.full((7,), 7, dtype=torch.int64, device="cuda")
    err.zero_()
    assert L.tl_canopy_keys(P(pts), 1, 3, 7, P(h), 0.5, 0, 0, 2, 2, P(mkeys), P(err), s) == 0
    assert mkeys.tolist() == [0, -1, -1, -1, -1, 3, -1] and err.item() == 1


# ------------------------------------------------------------------ segment_forest, save_results, the command line
def _small_plot(labelled=False):
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)
    pts = t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])
    return np.column_stack([pts, t["instance_label"].astype(np.float64)]) if labelled else pts


SAMPLE = dict(stride=1.0)                                                 # tiles side by side: four cover the plot
CANOPY_CFG = dict(metric_cell=8.0, top_window=3)


@pytest.fixture(scope="module")
def segmented():
    """segment_forest on the 12 m plot of six trees of tests/test_gpu_crown.py with the pinned-head random model of
    tests/test_gpu_inventory.py: once with canopy and inventory, once without any flag.  The pinned head calls every row a tree, so the
    terrain of the result has no ground candidate and every row is one without ground; the labelled plot goes through the command line."""
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
        res = segment_forest(pts, m, sample_cfg=SAMPLE, grouping_cfg=cfg, return_type="original", inventory=True, canopy=True, canopy_cfg=CANOPY_CFG)
        plain = segment_forest(pts, m, sample_cfg=SAMPLE, grouping_cfg=cfg, return_type="original")
    return pts, res, plain


def test_segment_forest_without_the_flag_returns_the_same_keys(segmented):
    _, res, plain = segmented
    assert set(plain) == {"coords", "labels", "categories"}
    assert set(res) == set(plain) | {"inventory", "terrain", "height_above_ground", "canopy", "stand"}
    for k in plain:
        assert np.array_equal(plain[k], res[k]), k


def test_segment_forest_canopy_files_and_cli(segmented, tmp_path):
    """The canopy of segment_forest is canopy_model on the returned coords and labels in the frame segment_forest works in: the test
    centres the cloud as segment_forest does (the same torch expression on the same device)."""
    from treelearn_amd.util.canopy import canopy_model, cloud_canopy, stand_summary
    from treelearn_amd.util.segment import save_results
    from treelearn_amd.util.terrain import terrain_model
    pts, res, plain = segmented
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    assert np.array_equal((xyz - mean + mean).cpu().numpy(), res["coords"])
    centred = xyz - mean
    t = terrain_model(centred, res["labels"], offset=mean)
    c = canopy_model(centred, t, res["labels"], offset=mean, **CANOPY_CFG)
    want, got = c.to_host(), res["canopy"]
    assert set(got) == set(want) and "tops_per_tree" in got and got["metric_cell"] == 8.0
    for k in want:
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.array_equal(got[k], want[k], equal_nan=np.asarray(want[k]).dtype.kind == "f"), k
    mean_h = mean.cpu().numpy()
    assert got["x0"] == c.ix0 * 0.5 + mean_h[0] and got["metric_y0"] == c.metric_iy0 * 8.0 + mean_h[1]
    assert np.array_equal(got["tops_x"], c.tops["x"].cpu().numpy() + mean_h[0])
    assert json.dumps(res["stand"]) == json.dumps(stand_summary(got, res["inventory"]))
    assert res["stand"]["n_trees"] == int((res["inventory"]["n_points"] > 0).sum()) and "n_dbh" in res["stand"]
    assert got["n_no_ground"] + got["n"].sum() == len(res["coords"]) == got["metric_n"].sum() + got["n_no_ground"]

    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    with np.load(tmp_path / "api" / "canopy.npz") as f:
        assert set(f.files) == set(got) and all(np.array_equal(f[k], got[k], equal_nan=f[k].dtype.kind == "f") for k in got)
    stand = json.load(open(tmp_path / "api" / "stand.json"))
    assert list(stand) == list(res["stand"]) and stand["n_tops"] == len(got["tops_h"])
    save_results(plain, str(tmp_path / "plain"), "plot", ["npy"], save_treewise=False)
    assert not (tmp_path / "plain" / "canopy.npz").exists() and not (tmp_path / "plain" / "stand.json").exists()

    # the command line in a child process on the plot with its true labels (label 0 = ground), against the same call made here
    forest = tmp_path / "labelled.npy"
    data = _small_plot(labelled=True)
    np.save(forest, data)
    env = dict(os.environ, PYTHONPATH=REPO)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "treelearn_amd.util.canopy", "--forest", str(forest), "--out",
                        str(tmp_path / "cli.npz"), "--stand", str(tmp_path / "cli.json"), "--canopy-metric-cell", "8", "--canopy-top-window", "3"],
                       capture_output=True, text=True, cwd=REPO, env=env)
    assert p.returncode == 0 and "tree tops" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    h = cloud_canopy(data, **CANOPY_CFG)[0].to_host()
    with np.load(tmp_path / "cli.npz") as f:
        assert set(f.files) == set(h) and all(np.array_equal(f[k], h[k], equal_nan=f[k].dtype.kind == "f") for k in h)
    cli = json.load(open(tmp_path / "cli.json"))
    assert cli["n_tops"] == len(h["tops_h"]) >= 1 and cli["n_trees"] == 6 and cli["area_ha"] > 0.005 and "lorey_height" in cli
    assert cli["trees_with_one_top"] + cli["trees_without_top"] + cli["trees_with_several_tops"] == 6 and h["n_no_ground"] < len(data) // 10
