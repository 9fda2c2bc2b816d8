"""The outlier filters on the GPU (csrc/tl_outlier.hip, util/outlier.py) against the brute-force restatement of
tests/outlier_restatement.py -- the specification, since open3d is not installed -- and their wiring into write_tiles,
generate_random_crops, PlotTiler and segment_forest."""
import functools
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlier_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4097                                   # no multiple of any block size
SEEDS = (0, 1, 2)
KS = (1, 2, 6, 20, 64)
SOR = ((2, 1.0), (64, 0.5))
RAD = (0.25, 5)
BAND = 1e-9                                # worst-case relative rounding of an n-term f64 sum, n up to about 1e6 (n * 2^-53 = 1.1e-10 at 1e6)


@functools.lru_cache(maxsize=None)
def cloud(seed):
    """Five Gaussian trunks (sigma 0.15 m, z in 0..6), a thin ground sheet and 40 scattered high points, all within +-6 m, rounded to
    2 decimals through float32, de-duplicated, 4 097 rows in shuffled order; returned widened to float64 (read-only)."""
    rng = np.random.default_rng(seed)
    cx = rng.uniform(-5, 5, size=(5, 2))
    trunks = np.concatenate([np.column_stack([c + rng.normal(0, 0.15, size=(560, 2)), rng.uniform(0, 6, size=560)]) for c in cx])
    ground = np.column_stack([rng.uniform(-6, 6, size=(1700, 2)), rng.normal(0, 0.02, size=1700)])
    high = np.column_stack([rng.uniform(-6, 6, size=(40, 2)), rng.uniform(2, 6, size=40)])
    body = np.unique(np.round(np.clip(np.concatenate([trunks, ground]), -6, 6).astype(np.float32), 2), axis=0)
    high = np.unique(np.round(high.astype(np.float32), 2), axis=0)
    body = body[~(body[:, None, :] == high[None, :, :]).all(2).any(1)]
    assert len(body) + len(high) >= N
    body = body[rng.permutation(len(body))[:N - len(high)]]
    xyz = np.concatenate([body, high])[rng.permutation(N)].astype(np.float64)
    assert len(np.unique(xyz, axis=0)) == N and np.abs(xyz).max() <= 6 and (xyz < 0).any()
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def ref_sorted(seed):
    d = R.sorted_distances(cloud(seed), 64)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def ref_count(seed):
    c = R.radius_count(cloud(seed), RAD[0])
    c.setflags(write=False)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _gpu_avg(xyz, k, **kw):
    from treelearn_amd.util import outlier as O
    return O.knn_mean_dist(xyz, k, **kw).cpu().numpy()


# ============================================================================================ 1. kernels
@pytest.mark.parametrize("seed", SEEDS)
def test_knn_mean_dist_is_bit_equal_to_the_restatement(seed):
    xyz = cloud(seed)
    perm = np.random.default_rng(100 + seed).permutation(N)
    for k in KS:
        want = R.mean_of_sorted(ref_sorted(seed), k)
        got = _gpu_avg(xyz, k)
        assert np.array_equal(_bits(got), _bits(want)), (k, int((got != want).sum()), float(np.abs(got - want).max()))
        got_p = _gpu_avg(xyz[perm], k)
        assert np.array_equal(_bits(got_p), _bits(want[perm])), ("permuted", k)
    # the result does not depend on the cell size either (a coarse and a very fine grid: one level, and many levels)
    want = R.mean_of_sorted(ref_sorted(seed), 6)
    for cell in (3.0, 0.02):
        assert np.array_equal(_bits(_gpu_avg(xyz, 6, cell=cell)), _bits(want)), cell


@pytest.mark.parametrize("n", (1, 2, 5, 63))
def test_knn_mean_dist_with_fewer_points_than_neighbours(n):
    xyz = cloud(0)[:n]
    got = _gpu_avg(xyz, 64)
    assert np.array_equal(_bits(got), _bits(R.knn_mean_dist(xyz, 64)))
    if n == 1:
        assert got[0] == 0


def test_knn_mean_dist_with_one_point_far_from_the_rest():
    xyz = np.concatenate([cloud(1)[:1500], [[60.0, -3.0, 2.0]]])
    for k in (2, 20):
        got = _gpu_avg(xyz, k)
        assert np.array_equal(_bits(got), _bits(R.knn_mean_dist(xyz, k))), k
        assert got[-1] > 25                                       # its neighbours are the far cloud's points


def test_knn_mean_dist_refuses_k_outside_1_to_64():
    from treelearn_amd.util import outlier as O
    for k in (0, 65):
        with pytest.raises(RuntimeError, match="tl_knn_mean_dist"):
            O.knn_mean_dist(cloud(0)[:100], k, cell=0.5)
    with pytest.raises(ValueError):
        O.sor_filter(cloud(0)[:100], 0, 1.0)
    with pytest.raises(ValueError):
        O.sor_filter(cloud(0)[:100], 2, 0.0)


@pytest.mark.parametrize("seed", SEEDS)
def test_sor_keep_matches_the_restatement_and_is_reproducible(seed):
    import torch
    from treelearn_amd.util import outlier as O
    for k, s in SOR:
        avg = R.mean_of_sorted(ref_sorted(seed), k)
        thr = R.sor_threshold(avg, s)
        gap = np.abs(avg - thr) / thr
        print(f"seed {seed} k {k} s {s}: thr {thr:.9f} kept {int(R.sor_mask_from_avg(avg, s).sum())} of {N}, smallest relative gap {gap.min():.3e}")
        assert gap.min() > BAND                                   # no point in the rounding band: the comparison below is exact
        a = torch.from_numpy(avg).cuda()
        keep1, thr1 = O.sor_keep(a, s)
        keep2, thr2 = O.sor_keep(a.clone(), s)
        assert np.array_equal(keep1.cpu().numpy(), R.sor_mask_from_avg(avg, s))
        assert abs(float(thr1) - thr) <= BAND * thr
        assert torch.equal(keep1, keep2) and _bits(thr1.cpu().numpy())[0] == _bits(thr2.cpu().numpy())[0]
        # the public entry, from the points
        assert np.array_equal(O.sor_filter(cloud(seed), k, s), R.sor_mask_from_avg(avg, s))
    assert not O.sor_filter(cloud(seed), 1, 1.0).any()           # k = 1: every avg is 0
    assert not O.sor_filter(cloud(seed)[:1], 2, 1.0).any()       # n = 1


@pytest.mark.parametrize("seed", SEEDS)
def test_radius_count_equals_the_restatement(seed):
    import torch
    from treelearn_amd.util import outlier as O
    xyz = cloud(seed)
    want = ref_count(seed)
    got = O.radius_count(xyz, RAD[0]).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), int((got != want).sum())
    keep = O.rad_filter(xyz.astype(np.float32), *RAD)             # f32 input is widened: the same f64 values here
    assert isinstance(keep, np.ndarray) and keep.dtype == bool and np.array_equal(keep, want > RAD[1])
    print(f"seed {seed}: radius {RAD} keeps {int(keep.sum())} of {N}")
    assert 0 < keep.sum() < N
    dev = O.rad_filter(torch.from_numpy(xyz.copy()).cuda(), *RAD)
    assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), keep)


def test_radius_count_on_the_integer_lattice():
    from treelearn_amd.util import outlier as O
    g = np.arange(-2, 3, dtype=np.float64)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    assert (O.radius_count(xyz, 1.0).cpu().numpy() == 1).all()    # d2 == r * r exactly: not inside
    got = O.radius_count(xyz, np.sqrt(2.0)).cpu().numpy()         # r * r rounds to 2.0000000000000004: the 12 edge neighbours at d2 = 2 are inside
    assert np.array_equal(got, R.radius_count(xyz, np.sqrt(2.0))) and got.max() == 19


@pytest.mark.parametrize("seed", SEEDS)
def test_denoise_is_sor_then_radius_on_the_survivors(seed):
    from treelearn_amd.util import outlier as O
    xyz = cloud(seed)
    sor = (6, 1.0)
    cfg = dict(n_neigh_sor=sor[0], multiplier_sor=sor[1], rad=RAD[0], npoints_rad=RAD[1])
    avg = R.mean_of_sorted(ref_sorted(seed), sor[0])
    assert (np.abs(avg - R.sor_threshold(avg, sor[1])) / R.sor_threshold(avg, sor[1])).min() > BAND
    first = R.sor_mask_from_avg(avg, sor[1])
    rows = np.flatnonzero(first)
    want = np.zeros(N, dtype=bool); want[rows[R.rad_mask(xyz[rows], *RAD)]] = True
    got = O.denoise(xyz, cfg)
    assert np.array_equal(got, want) and 0 < want.sum() < first.sum() < N
    assert O.denoise(xyz, dict()).all()
    assert np.array_equal(O.denoise(xyz, dict(rad=RAD[0], npoints_rad=RAD[1])), ref_count(seed) > RAD[1])


# ============================================================================================ 2. wiring
FILTERS = dict(n_neigh_sor=6, multiplier_sor=1.0, rad=0.35, npoints_rad=3)
SAMPLE = dict(voxel_size=0.1, inner_edge=3.5, outer_edge=0.5, stride=1)


def _forest(seed=3):
    """About 14 x 14 m, about 20 k points on a 0.2 m lattice (so voxelising at 0.1 m keeps them), labelled, with noise sprinkled in."""
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=14.0, voxel=0.2, n_trees=4, fill=0.10, seed=seed)
    rng = np.random.default_rng(seed)
    noise = np.column_stack([rng.uniform(-7, 7, size=(300, 2)), rng.uniform(0, 20, size=300)])
    p = np.concatenate([t["points"].astype(np.float64), noise]) + np.array([250.0, -140.0, 3.0])
    lab = np.concatenate([t["instance_label"].astype(np.float64), np.zeros(300)])
    lab[rng.uniform(size=len(lab)) < 0.05] = -1
    return np.hstack([p, lab[:, None]])


def _mask(points):
    return R.denoise(points.astype(np.float64), (FILTERS["n_neigh_sor"], FILTERS["multiplier_sor"]), (FILTERS["rad"], FILTERS["npoints_rad"]))


def _no_band(points):
    """The restatement's statistical step has no point in the rounding band (else a mask could legitimately differ there)."""
    avg = R.knn_mean_dist(points.astype(np.float64), FILTERS["n_neigh_sor"])
    thr = R.sor_threshold(avg, FILTERS["multiplier_sor"])
    return (np.abs(avg - thr) / thr).min() > BAND


def _same_with_mask(off, on, what):
    keep = _mask(off["points"])
    assert _no_band(off["points"]), what
    for key in ("points", "feat", "instance_label"):
        assert on[key].dtype == off[key].dtype and np.array_equal(on[key], off[key][keep]), (what, key)
    assert np.array_equal(on["center"], off["center"]), what
    return int((~keep).sum())


def test_write_tiles_with_filters_equals_masked_unfiltered_tiles(tmp_path):
    from treelearn_amd.util.tiles import write_tiles
    forest = _forest()
    n = {}
    for tag, gen in (("off", None), ("on", FILTERS)):
        os.makedirs(str(tmp_path / tag / "forest"))
        np.save(str(tmp_path / tag / "forest" / "plot.npy"), forest)
        n[tag] = write_tiles(str(tmp_path / tag / "forest" / "plot.npy"), dict(SAMPLE, **({"sample_generator": gen} if gen else {})))
    assert n["on"] == n["off"] >= 9
    assert 10000 <= len(np.load(str(tmp_path / "off" / "forest_voxelized0.1" / "plot.npz"))["points"]) <= 40000
    lost = []
    for i in range(n["off"]):
        off = np.load(str(tmp_path / "off" / "tiles" / "npz" / f"plot_{i}.npz")); on = np.load(str(tmp_path / "on" / "tiles" / "npz" / f"plot_{i}.npz"))
        lost.append(_same_with_mask(off, on, f"tile {i}"))
        meta = json.load(open(str(tmp_path / "on" / "tiles" / "json" / f"plot_{i}.json")))
        assert {k: meta[k] for k in FILTERS} == FILTERS
    print("rows lost per tile:", lost)
    assert sum(v > 0 for v in lost) >= 2


def test_generate_random_crops_with_filters_equals_masked_unfiltered_crops(tmp_path):
    from treelearn_amd.util import crops as C
    forest = _forest()
    cfg = dict(chunk_size=5, n_samples_total=3, n_points_to_calculate_occupancy=5000, how_far_fill=2, min_percent_occupied_choose=0.3)
    for tag, extra in (("off", {}), ("on", FILTERS)):
        os.makedirs(str(tmp_path / tag / "forests"))
        np.save(str(tmp_path / tag / "forests" / "plot.npy"), forest)
        assert sum(C.generate_random_crops(str(tmp_path / tag), dict(cfg, **extra), seed=4).values()) == 3
    lost = 0
    for k in range(3):
        off = np.load(str(tmp_path / "off" / "random_crops" / "npz" / f"plot_{k}.npz")); on = np.load(str(tmp_path / "on" / "random_crops" / "npz" / f"plot_{k}.npz"))
        lost += _same_with_mask(off, on, f"crop {k}")
        m_off = json.load(open(str(tmp_path / "off" / "random_crops" / "json" / f"plot_{k}.json")))
        m_on = json.load(open(str(tmp_path / "on" / "random_crops" / "json" / f"plot_{k}.json")))
        assert {k2: m_on[k2] for k2 in FILTERS} == FILTERS and m_on["rotation_angle"] == m_off["rotation_angle"]     # the filters draw no random numbers
    assert lost > 0


ROW_KEYS = ("coords", "input_feats", "batch_ids", "semantic_labels", "instance_labels", "masks_inner", "masks_off", "masks_sem", "offset_labels",
            "centers")


@pytest.mark.parametrize("mode", ("none", "device"))
def test_plot_tiler_batches_with_filters_equal_masked_unfiltered_batches(mode):
    import torch
    from treelearn_amd.util.tiles import PlotTiler
    rng = np.random.default_rng(8)
    # a 12 x 12 m sheet of lattice points with labels and scattered high points; the sheet has a hole over the middle tile's inner square
    # (3.77 .. 8.03 m), where only one lone point and a few of the scattered ones lie
    g = np.arange(0, 12, 0.2)
    sheet = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    sheet = sheet[~((sheet[:, 0] > 3.6) & (sheet[:, 0] < 8.2) & (sheet[:, 1] > 3.6) & (sheet[:, 1] < 8.2))]
    pts = np.concatenate([np.column_stack([sheet, np.round(rng.uniform(0, 0.3, size=len(sheet)), 2)]),
                          np.column_stack([rng.uniform(0.5, 11.5, size=(150, 2)), rng.uniform(3, 9, size=150)]).round(2),
                          [[5.9, 5.9, 1.0]]]).astype(np.float32)
    lab = np.where(pts[:, 2] > 0.15, 1.0 + (pts[:, 0] > 6), 0.0).astype(np.float32)
    feats = rng.uniform(size=(len(pts), 1)).astype(np.float32)
    tiler = PlotTiler(pts, lab, feats)
    args = (4.0, 1.0, 1, 4.0)
    def run(**kw):
        out = {}
        for b in tiler.tiles(*args, offset_labels=mode, **kw):
            b["_ready_event"].synchronize()
            out[b["tile_index"]] = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in b.items() if k != "_ready_event"}
        return out
    off, on = run(), run(sample_generator=FILTERS)
    assert all(np.array_equal(v[k], off[t][k]) for t, v in run(sample_generator=dict(FILTERS, rad=None, npoints_rad=None, n_neigh_sor=None,
                                                                                      multiplier_sor=None)).items() for k in ROW_KEYS)
    assert sorted(on) == sorted(off) and len(on) >= 4             # the numbering and the skipping are decided before the filter
    emptied = 0
    for t in sorted(off):
        keep = _mask(off[t]["coords"])
        assert _no_band(off[t]["coords"]), t
        # device mode: the offset labels are derived from the tile's surviving rows, so they may differ from the unfiltered tile's
        same = ROW_KEYS if mode == "none" else ("coords", "input_feats", "batch_ids", "semantic_labels", "instance_labels", "masks_inner", "masks_sem",
                                                "centers")
        for k in same:
            assert np.array_equal(on[t][k], off[t][k][keep]), (t, k)
        assert len(on[t]["offset_labels"]) == len(on[t]["masks_off"]) == int(keep.sum())
        assert on[t]["batch_size"] == 1
        emptied += bool(off[t]["masks_inner"].any() and not on[t]["masks_inner"].any())
    assert emptied >= 1                                            # a tile whose inner square only the filter empties is still yielded


def test_segment_forest_runs_with_a_complete_pair():
    import torch
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import make_tile, random_state_dict
    from treelearn_amd.util.segment import MODEL_CFG, segment_forest
    t = make_tile(extent=16, voxel=0.2, n_trees=5, fill=0.10, seed=5)
    pts = t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])
    sd = random_state_dict(7, channels=32, num_blocks=7)
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    model = TreeLearn(**MODEL_CFG).cuda().eval()
    model.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)
    with torch.no_grad():
        res = segment_forest(pts, model, sample_cfg=dict(sample_generator=FILTERS), grouping_cfg=cfg, return_type="original")
    assert len(res["labels"]) == len(pts) == len(res["coords"]) and res["labels"].dtype == np.int64
    with pytest.raises(NotImplementedError, match="^rad is set"):
        segment_forest(pts, model, sample_cfg=dict(sample_generator=dict(rad=0.3)), grouping_cfg=cfg)
