"""CPU tests of the random-crop generator's host stages and of CropDataset / collate against golden G15
(tests/golden/make_golden_crops.py: the reference's own generate_random_crops and TreeDataset(training=True)), bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from treelearn_amd.util import crops as C
from treelearn_amd.util.dataset import CropDataset, collate


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_crops.npz"))


def _plots(g):
    return [str(p) for p in g["plots"]]


def _ranges(g, name):
    return C.get_ranges(g[f"in/{name}/points"])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_steps_and_cell_centres_match_reference(g15):
    cfg = json.loads(str(g15["cfg"]))
    for name in _plots(g15):
        xs, ys, X, Y = C.grid_steps(*_ranges(g15, name), cfg["occupancy_res"])
        assert _same(xs, g15[f"stage/{name}/x_steps"]) and _same(ys, g15[f"stage/{name}/y_steps"]), name
        assert xs.dtype == np.float64
        assert [X, Y] == list(g15[f"stage/{name}/dims"])
        grid = g15[f"stage/{name}/grid"]
        assert _same(C.cell_centres(xs, X), grid[:, 0, 0]) and _same(C.cell_centres(ys, Y), grid[0, :, 1]), name


def _draws(g):
    """Replays the reference's draw order with one RandomState: randint per plot, then uniform + choice per plot."""
    cfg = json.loads(str(g["cfg"]))
    rs = np.random.RandomState(int(g["seed"]))
    occupied = {}
    for name in _plots(g):
        C.occupancy_sample(int((g[f"in/{name}/labels"] != -1).sum()), rs, cfg["n_points_to_calculate_occupancy"])
        occupied[name] = np.sum(g[f"stage/{name}/filled"])
    n_samples = C.apportion(occupied, cfg["n_samples_total"])
    out = {}
    for name in _plots(g):
        centres, angles, rinv = C.crop_candidates(*_ranges(g, name), rs, cfg["n_samples_total"], n_samples[name])
        ok = g[f"stage/{name}/filter"]
        inds = C.choose(rs, int(ok.sum()), n_samples[name])
        out[name] = (centres, angles, rinv, inds, n_samples[name])
    return out, n_samples


def test_apportioning_matches_reference(g15):
    cfg = json.loads(str(g15["cfg"]))
    draws, n_samples = _draws(g15)
    assert sum(n_samples.values()) == cfg["n_samples_total"]
    for name, (centres, _, _, inds, n) in draws.items():
        k = int(np.sqrt(np.max([cfg["n_samples_total"], 5 * n]))) ** 2
        assert len(g15[f"stage/{name}/angles"]) == k
        assert len(g15[f"stage/{name}/inds"]) == min(n, int(g15[f"stage/{name}/filter"].sum()))
    written = {}
    for c in g15["crops"]:
        written[str(c).rsplit("_", 1)[0]] = written.get(str(c).rsplit("_", 1)[0], 0) + 1
    assert written == {n: len(g15[f"stage/{n}/inds"]) for n in _plots(g15) if len(g15[f"stage/{n}/inds"])}


def test_candidates_inverse_matrices_and_draws_match_reference(g15):
    draws, _ = _draws(g15)
    for name, (centres, angles, rinv, inds, _) in draws.items():
        assert centres.dtype == np.float32 and _same(centres, g15[f"stage/{name}/centers"]), name
        assert _same(angles, g15[f"stage/{name}/angles"]), name
        assert _same(rinv, g15[f"stage/{name}/rinv"]), name
        assert _same(np.asarray(inds, np.int64), g15[f"stage/{name}/inds"]), name
    assert len(draws["plot_c"][3]) == 0 and not g15["stage/plot_c/filter"].any()       # the strip: nothing passes, choice still drawn


def test_golden_filter_is_self_consistent(g15):
    """A self-check of golden G15 (no project code): its stored filter is the f64 threshold of its stored grid, candidates and
    inverse matrices, so the GPU test of tl_crops_check against the same arrays compares like with like."""
    cfg = json.loads(str(g15["cfg"]))
    for name in _plots(g15):
        grid = g15[f"stage/{name}/grid"]
        cells = grid.reshape(-1, 3)
        sums = []
        for c, r in zip(g15[f"stage/{name}/centers"], g15[f"stage/{name}/rinv"]):
            u = (cells[:, :2] - c) @ r.T
            sums.append(np.sum(cells[:, 2][np.linalg.norm(u, ord=np.inf, axis=1) <= cfg["chunk_size"] / 2]))
        assert _same(np.array(sums) / (cfg["chunk_size"] / cfg["occupancy_res"]) ** 2 > cfg["min_percent_occupied_choose"],
                     g15[f"stage/{name}/filter"])


def _write_full(g, d):
    names = sorted({str(k).split("/")[1] for k in g.files if str(k).startswith("full/")})
    for n in names:
        np.savez(os.path.join(d, n + ".npz"), **{k: g[f"full/{n}/{k}"] for k in g[f"keys/{n}"]})
    return names


FIELDS = ("xyz", "input_feat", "instance_label", "semantic_label", "pt_offset_label", "center", "mask_inner", "mask_off", "mask_sem")


def test_dataset_items_and_batch_match_reference(g15, tmp_path):
    names = _write_full(g15, str(tmp_path))
    assert len(names) == 3
    ds = CropDataset(str(tmp_path), int(g15["ds/inner"]), True, json.loads(str(g15["ds/aug"])), seed=int(g15["ds/seed"]))
    items = [ds[i] for i in range(3)]
    for i, it in enumerate(items):
        for k, v in zip(FIELDS, it):
            assert _same(v.numpy(), g15[f"item/{i}/{k}"]), (i, k)
    batch = collate([items[0], items[1]])
    keys = sorted(str(k)[6:] for k in g15.files if str(k).startswith("batch/"))
    assert sorted(batch) == keys
    for k in keys:
        v = batch[k]
        assert _same(v.numpy() if torch.is_tensor(v) else np.array(v), g15[f"batch/{k}"]), k


def test_dataset_test_mode_and_disabled_augmentations_draw_nothing(g15, tmp_path):
    _write_full(g15, str(tmp_path))
    off = dict(jitter=False, flip=False, rot=False, scaled=False, point_jitter=False)
    ds = CropDataset(str(tmp_path), 4, True, off, seed=3)
    state = ds.rs.get_state()[1].copy()
    it = ds[0]
    assert np.array_equal(ds.rs.get_state()[1], state)
    assert it[0].dtype == torch.float64 and np.array_equal(it[0].numpy(), g15["full/plot_a_0/points"].astype(np.float64))
    te = CropDataset(str(tmp_path), 4, False)[0]
    assert te[0].dtype == torch.float32 and np.array_equal(te[5].numpy(), np.ones((len(te[0]), 3)) * g15["full/plot_a_0/center"])


def test_dataset_runs_in_dataloader_workers(g15, tmp_path):
    """Workers draw from (seed, worker id, torch's worker seed): a seeded DataLoader repeats a run, and a new epoch of
    non-persistent workers draws new augmentations."""
    _write_full(g15, str(tmp_path))
    ds = CropDataset(str(tmp_path), 4, True, json.loads(str(g15["ds/aug"])), seed=5)

    def epochs(gen_seed, n=2):
        dl = torch.utils.data.DataLoader(ds, batch_size=1, num_workers=2, collate_fn=collate, shuffle=False,
                                         generator=torch.Generator().manual_seed(gen_seed))
        return [[b["coords"] for b in dl] for _ in range(n)]
    e1, e2 = epochs(11), epochs(11)
    assert len(e1[0]) == 3 and all(torch.isfinite(c).all() for c in e1[0])
    assert all(torch.equal(a, b) for ea, eb in zip(e1, e2) for a, b in zip(ea, eb))        # seeded loader: the same run
    assert not all(torch.equal(a, b) for a, b in zip(e1[0], e1[1]))                        # epoch 2 is augmented anew
    a = CropDataset(str(tmp_path), 4, True, json.loads(str(g15["ds/aug"])), seed=5)
    b = CropDataset(str(tmp_path), 4, True, json.loads(str(g15["ds/aug"])), seed=5)
    assert all(torch.equal(a[i][0], b[i][0]) for i in range(3))                     # same seed, same process: same items


def test_sor_and_radius_filters_are_refused_by_name(tmp_path):
    for k in ("n_neigh_sor", "multiplier_sor", "rad", "npoints_rad"):
        with pytest.raises(NotImplementedError, match=k):
            C.generate_random_crops(str(tmp_path), {k: 3})
    assert not os.listdir(str(tmp_path))                                              # refused before anything is written


def test_plot_narrower_than_occupancy_res_is_refused():
    with pytest.raises(ValueError, match="occupancy_res"):
        C.grid_steps(np.array([10.0, 30.0], np.float32), np.array([5.0, 5.5], np.float32), 1)


def test_no_valid_points_is_refused():
    with pytest.raises(ValueError, match="no valid points"):
        C.occupancy_sample(0, np.random.RandomState(0), 10)


def test_cli_validates_arguments(tmp_path, capsys):
    with pytest.raises(SystemExit):
        C.parse_args(["--base-dir", str(tmp_path)])                                   # no forests/
    os.makedirs(tmp_path / "forests")
    for bad in (["--chunk-size", "0"], ["--n-samples-total", "2.5"], ["--how-far-fill", "-1"], ["--min-percent-occupied-fill", "1.5"]):
        with pytest.raises(SystemExit):
            C.parse_args(["--base-dir", str(tmp_path)] + bad)
    a = C.parse_args(["--base-dir", str(tmp_path), "--chunk-size", "10", "--occupancy-res", "0.5"])
    assert a.chunk_size == 10 and isinstance(a.chunk_size, int) and a.occupancy_res == 0.5 and a.how_far_fill == C.TRAIN_CFG["how_far_fill"]


def test_explicit_layout_equals_the_reference_expressions_on_random_plots():
    """The explicit-dtype lay-out (steps, candidate centres) against the reference's expressions as this numpy evaluates them,
    on 1 000 random float32 plot ranges at several resolutions: bit for bit, dtypes included."""
    rng = np.random.default_rng(12)
    for t in range(1000):
        lo = rng.uniform(-5000, 5000); ext = rng.uniform(3.0, 150); res = [1, 0.5, 0.3, 2, 0.25][t % 5]          # y extent 0.7 ext >= 2.1 > res
        xr = np.round(np.array([lo, lo + ext]), 2).astype(np.float32)
        yr = np.round(np.array([lo / 3, lo / 3 + ext * 0.7]), 2).astype(np.float32)
        xs, ys, X, Y = C.grid_steps(xr, yr, res)
        for r, steps, dim in ((xr, xs, X), (yr, ys, Y)):
            diff = np.abs(r[0] - r[1]); times_fit = np.floor(diff / res)
            ref = np.arange(r[0], r[1] + 1e-3, step=diff / times_fit)
            assert dim == int(times_fit) and _same(steps, ref), (t, r, res)
            assert _same(C.cell_centres(steps, dim), np.array([np.mean(ref[i:i + 2]) for i in range(dim)])), t
        n = int(rng.integers(1, 40))
        centres, _, _ = C.crop_candidates(xr, yr, np.random.RandomState(t), n * n, 0)
        ref_x = np.round(np.repeat(np.linspace(xr[0], xr[1], n), n), 2); ref_y = np.round(np.tile(np.linspace(yr[0], yr[1], n), n), 2)
        assert _same(centres, np.hstack([ref_x.reshape(-1, 1), ref_y.reshape(-1, 1)])), t
