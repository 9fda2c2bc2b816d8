"""Random training crops from labelled forests on the device: the reference's `generate_random_crops`
(tools/data_gen/gen_train_data.py:15-97) and the random-crop half of `SampleGenerator`
(tree_learn/util/data_preparation.py:136-330), DESIGN §12.

    python -m treelearn_amd.util.crops --base-dir DIR [--seed S] [--n-samples-total N] [--chunk-size M] [...]

  occupancy_grid   <- SampleGenerator.get_occupancy_grid (:136-172) + fill_holes (:571-586): tl_crops_occupancy, tl_crops_fill
  crop_candidates  <- SampleGenerator.generate_candidates (:176-205) and invert_rotate_and_shift's matrices (:535-545): host
  check_occupancy  <- SampleGenerator.check_occupancy (:209-230): tl_crops_check
  extract_crops    <- SampleGenerator.save (:234-289): tl_crops_count + tl_crops_extract, up to 32 crops per read of the plot

The grid and candidate lay-out is cheap and stays on the host: the reference's numpy expressions, restated with an explicit
dtype for every intermediate as numpy 2.2.6 evaluates them (the steps come out float64, the candidate centres float32),
so the kernels receive exactly the arrays the reference computes with, whatever numpy's promotion rules.  All randomness comes from one `np.random.RandomState(seed)`, drawn with the reference's
methods, arguments and order; with the same seed the files equal those the reference writes after `np.random.seed(seed)`.
"""
import argparse
import json
import os
import os.path as osp
import sys

import numpy as np
import torch

from .. import _hip

IGNORE_LABEL = -1                                   # gen_train_data.py:9
MAX_BATCH = 32                                      # crops per read of the plot (tl_crops_count)
f32, f64 = np.float32, np.float64

# configs/data_gen/gen_train_data.yaml + configs/_modular/sample_generation.yaml of the reference (ints stay ints: they reach the json files)
TRAIN_CFG = dict(occupancy_res=1, n_points_to_calculate_occupancy=100000, min_percent_occupied_fill=0.9, how_far_fill=9,
                 min_percent_occupied_choose=0.45, n_samples_total=25000, chunk_size=35, voxel_size=0.1, search_radius_features=0.6,
                 n_neigh_sor=None, multiplier_sor=None, rad=None, npoints_rad=None, feature_names=["verticality"])
_FILTER_KEYS = ("n_neigh_sor", "multiplier_sor", "rad", "npoints_rad")


def _dev(a, dtype):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device="cuda", dtype=dtype).contiguous()


def get_ranges(points):
    """data_preparation.py:497-508 for one cloud: (x_range, y_range), each the float32 pair (min, max)."""
    p = points if torch.is_tensor(points) else torch.from_numpy(np.asarray(points))
    mn = p[:, :2].amin(0).cpu().numpy(); mx = p[:, :2].amax(0).cpu().numpy()
    return np.array([mn[0], mx[0]], dtype=f32), np.array([mn[1], mx[1]], dtype=f32)


def adjust_res(rng, res):
    """data_preparation.py:564-568 on the float32 range: (float32 adjusted resolution, int number of cells)."""
    diff = np.abs(f32(rng[0]) - f32(rng[1]))
    times_fit = np.floor(diff / f32(res))
    return f32(diff / times_fit), int(times_fit)


def _arange(start, stop, step):
    """np.arange(start, stop, step) of float32 scalars under numpy 2.2.6, written out: the length ceil((stop - start) / step)
    and the second value start + step are float32 arithmetic, the result is float64 filled as start + i * (second - start)."""
    start, stop, step = f32(start), f32(stop), f32(step)
    n = max(int(np.ceil(f32(f32(stop - start) / step))), 0)
    out = np.empty(n, dtype=f64)
    if n > 0:
        out[0] = f64(start)
    if n > 1:
        second = f64(f32(start + step))
        out[1] = second
        out[2:] = f64(start) + np.arange(2, n, dtype=f64) * (second - f64(start))
    return out


def _linspace(start, stop, num):
    """np.linspace(start, stop, num) of float32 scalars under numpy 2.2.6, written out in float32 (numpy's own algorithm)."""
    start, stop = f32(start), f32(stop)
    delta = f32(stop - start)
    y = np.arange(num, dtype=f32)
    if num > 1:
        step = f32(delta / f32(num - 1))
        y = (y / f32(num - 1)) * delta if step == 0 else y * step
    else:
        y = y * delta
    y = y + start
    if num > 1:
        y[-1] = stop
    return y


def _round2_f32(a):
    """np.round(a, 2) of a float32 array: rint(a * 100) / 100 in float32."""
    return np.rint(a * f32(100)) / f32(100)


def grid_steps(x_range, y_range, occupancy_res):
    """data_preparation.py:149-151: (x_steps f64, y_steps f64, x_dim, y_dim).  Every intermediate has an explicit dtype (the
    reference's expressions as numpy 2.2.6 evaluates them; golden G15 pins the values), so numpy's promotion rules do not enter."""
    for name, r in (("x", x_range), ("y", y_range)):
        if not np.abs(f32(r[0]) - f32(r[1])) >= f32(occupancy_res):
            raise ValueError(f"plot extent in {name} ({float(np.abs(f32(r[0]) - f32(r[1])))} m) is below occupancy_res ({occupancy_res} m): "
                             "no occupancy cell fits")
    (x_res, x_dim), (y_res, y_dim) = adjust_res(x_range, occupancy_res), adjust_res(y_range, occupancy_res)
    y_steps = _arange(y_range[0], f32(y_range[1]) + f32(1e-3), y_res)
    x_steps = _arange(x_range[0], f32(x_range[1]) + f32(1e-3), x_res)
    if len(x_steps) < x_dim + 1 or len(y_steps) < y_dim + 1:            # the reference would index past the steps here
        raise ValueError("occupancy steps do not cover the grid")
    return x_steps, y_steps, x_dim, y_dim


def cell_centres(steps, dim):
    """data_preparation.py:166: np.mean(steps[i:i+2]) per cell = (steps[i] + steps[i+1]) / 2 in float64."""
    s = np.asarray(steps, dtype=f64)
    return (s[:dim] + s[1:dim + 1]) / f64(2)


def occupancy_sample(n_valid, rs, n_points_to_calculate_occupancy):
    """data_preparation.py:154-157: indices of the valid points that mark the occupancy grid (one draw from rs)."""
    if n_valid == 0:
        raise ValueError("no valid points (every label is -1): the occupancy grid is undefined")
    return rs.randint(0, n_valid, size=n_points_to_calculate_occupancy)


def choose(rs, n_passing, n_samples_plot):
    """data_preparation.py:245-248: which passing candidates become crops (one draw from rs, also when none passes)."""
    if n_samples_plot <= n_passing:
        return rs.choice(range(n_passing), n_samples_plot, replace=False)
    return rs.choice(range(n_passing), n_passing, replace=False)


def occupancy_grid(points, labels, rs, occupancy_res, n_points_to_calculate_occupancy, how_far_fill, min_percent_occupied_fill,
                   ignore_for_occupancy=IGNORE_LABEL):
    """get_occupancy_grid + fill_holes without the cache file.  points f32[N,3] and labels f32[N] (device or host).
    Draws rs.randint(0, n_valid, size=n_points_to_calculate_occupancy).  Returns dict(grid f64[X,Y,3] as the reference
    saves it, raw u8[X,Y], filled u8[X,Y], x_steps, y_steps)."""
    pts = _dev(points, torch.float32); lab = _dev(labels, torch.float32).reshape(-1)
    x_range, y_range = get_ranges(pts)
    x_steps, y_steps, X, Y = grid_steps(x_range, y_range, occupancy_res)
    valid = pts[lab != ignore_for_occupancy]
    idx = occupancy_sample(len(valid), rs, n_points_to_calculate_occupancy)
    xy = valid[:, :2].index_select(0, torch.from_numpy(idx).to(valid.device)).contiguous()
    L = _hip.lib()
    xs, ys = _dev(x_steps[:X + 1], torch.float64), _dev(y_steps[:Y + 1], torch.float64)
    raw = torch.empty((X, Y), dtype=torch.uint8, device=pts.device); filled = torch.empty_like(raw)
    _hip.check(L.tl_crops_occupancy(_hip.ptr(xy), len(xy), _hip.ptr(xs), X, _hip.ptr(ys), Y, _hip.ptr(raw), _hip.stream()), "tl_crops_occupancy")
    _hip.check(L.tl_crops_fill(_hip.ptr(raw), X, Y, int(how_far_fill), float(min_percent_occupied_fill), _hip.ptr(filled), _hip.stream()),
               "tl_crops_fill")
    raw, filled = raw.cpu().numpy(), filled.cpu().numpy()
    grid = np.ones((X, Y, 3)) * 10
    grid[:, :, 0] = cell_centres(x_steps, X)[:, None]
    grid[:, :, 1] = cell_centres(y_steps, Y)[None, :]
    grid[:, :, 2] = filled
    return dict(grid=grid, raw=raw, filled=filled, x_steps=x_steps, y_steps=y_steps)


def inverse_rotations(rotation_angles):
    """invert_rotate_and_shift's matrices (data_preparation.py:535-541), one np.linalg.inv per candidate: f64[k,2,2]."""
    out = np.empty((len(rotation_angles), 2, 2), dtype=np.float64)
    for k, a in enumerate(rotation_angles):
        cosine = np.cos(a).item(); sine = np.sin(a).item()
        out[k] = np.linalg.inv(np.array([[cosine, -sine], [sine, cosine]]))
    return out


def crop_candidates(x_range, y_range, rs, n_samples_total, n_samples_plot):
    """generate_candidates (data_preparation.py:176-205): centres float32 [k,2], rotation angles float64 [k], inverse
    rotations float64 [k,2,2].  Draws rs.uniform(0, 2 pi, size=k).  (The rotated vertices only bound the reference's
    generous ±3 m pre-selection, which the kernels do not need.)"""
    n_samples_sqrt = int(np.sqrt(f64(max(int(n_samples_total), 5 * int(n_samples_plot)))))
    x_centers = _round2_f32(np.repeat(_linspace(x_range[0], x_range[1], n_samples_sqrt), n_samples_sqrt))
    y_centers = _round2_f32(np.tile(_linspace(y_range[0], y_range[1], n_samples_sqrt), n_samples_sqrt))
    centers = np.stack([x_centers, y_centers], axis=1).astype(f32)
    rotation_angles = np.asarray(rs.uniform(0, 2 * np.pi, size=n_samples_sqrt * n_samples_sqrt), dtype=f64)
    rotation_angles = np.rint(rotation_angles * f64(100)) / f64(100)                  # np.round(., 2) in float64
    return centers, rotation_angles, inverse_rotations(rotation_angles)


def check_occupancy(grid, centres, rinv, chunk_size, occupancy_res, min_percent_occupied_choose):
    """check_occupancy (data_preparation.py:209-230) for every candidate: (occupied kept cells f64[k], filter bool[k])."""
    g = np.asarray(grid)
    X, Y = g.shape[:2]
    occ = g[:, :, 2]
    if not np.all((occ == 0) | (occ == 1)):
        raise ValueError("occupancy grid values must be 0 or 1")
    k = len(centres)
    if k == 0:
        return np.zeros(0), np.zeros(0, bool)
    cx, cy = _dev(g[:, 0, 0], torch.float64), _dev(g[0, :, 1], torch.float64)
    o = _dev(occ.astype(np.uint8), torch.uint8)
    c = _dev(np.asarray(centres, np.float32), torch.float32); r = _dev(np.asarray(rinv, np.float64), torch.float64)
    sums = torch.empty(k, dtype=torch.float64, device=c.device); ok = torch.empty(k, dtype=torch.uint8, device=c.device)
    denominator = (chunk_size / occupancy_res) ** 2
    _hip.check(_hip.lib().tl_crops_check(_hip.ptr(cx), X, _hip.ptr(cy), Y, _hip.ptr(o), _hip.ptr(c), _hip.ptr(r), k, float(chunk_size),
                                         float(denominator), float(min_percent_occupied_choose), _hip.ptr(sums), _hip.ptr(ok), _hip.stream()),
               "tl_crops_check")
    return sums.cpu().numpy(), ok.cpu().numpy().astype(bool)


def extract_crops(points, labels, feats, centres, rinv, chunk_size, batch=MAX_BATCH, filters=None):
    """save's selection (data_preparation.py:264-289) for the chosen crops, in order: yields (points f32[n,3] = rotated xy and z,
    instance_label int32[n], feat f32[n,F]) per crop, rows in plot order.  The plot is read once per `batch` crops.
    `filters` (a sample_generator section, or what outlier.active_filters returned): the outlier filters of :281-287, run on the
    device on each extracted crop before it is copied to the host; they draw no random numbers and only remove rows."""
    from . import outlier
    filters = outlier.active_filters(filters)
    denoise = filters["sor"] is not None or filters["rad"] is not None
    pts = _dev(points, torch.float32); lab = _dev(labels, torch.float32).reshape(-1)
    n = len(pts)
    ft = _dev(feats, torch.float32).reshape(n, -1)
    F = ft.shape[1]
    batch = max(1, min(int(batch), MAX_BATCH, (2 ** 31 - 1) // max(n, 1)))
    L = _hip.lib()
    c_all = np.ascontiguousarray(centres, np.float32).reshape(-1, 2); r_all = np.ascontiguousarray(rinv, np.float64).reshape(-1, 2, 2)
    ws = torch.empty(int(L.tl_crops_ws_words(n, batch)), dtype=torch.int32, device=pts.device)
    counts = torch.empty(batch, dtype=torch.int32, device=pts.device)
    for b0 in range(0, len(c_all), batch):
        nc = min(batch, len(c_all) - b0)
        c = _dev(c_all[b0:b0 + nc], torch.float32); r = _dev(r_all[b0:b0 + nc], torch.float64)
        _hip.check(L.tl_crops_count(_hip.ptr(pts), n, nc, _hip.ptr(c), _hip.ptr(r), float(chunk_size), _hip.ptr(counts), _hip.ptr(ws), _hip.stream()),
                   "tl_crops_count")
        cnt = counts[:nc].cpu().numpy().astype(np.int64)
        total = int(cnt.sum())
        cap = max(total, 1)
        oxyz = torch.empty((cap, 3), dtype=torch.float32, device=pts.device); olab = torch.empty(cap, dtype=torch.int32, device=pts.device)
        ofeat = torch.empty((cap, max(F, 1)), dtype=torch.float32, device=pts.device)
        _hip.check(L.tl_crops_extract(_hip.ptr(pts), _hip.ptr(lab), _hip.ptr(ft), n, F, nc, _hip.ptr(c), _hip.ptr(r), float(chunk_size), _hip.ptr(ws),
                                      cap, _hip.ptr(oxyz), _hip.ptr(olab), _hip.ptr(ofeat), _hip.stream()), "tl_crops_extract")
        off = np.concatenate([[0], np.cumsum(cnt)])
        if denoise:
            for i in range(nc):
                a, e = int(off[i]), int(off[i + 1])
                keep = outlier.denoise(oxyz[a:e], filters)
                yield oxyz[a:e][keep].cpu().numpy(), olab[a:e][keep].cpu().numpy(), ofeat[a:e, :F][keep].cpu().numpy()
            continue
        hx, hl, hf = oxyz.cpu().numpy(), olab.cpu().numpy(), ofeat[:, :F].cpu().numpy()
        for i in range(nc):
            a, e = off[i], off[i + 1]
            yield hx[a:e], hl[a:e], hf[a:e]


def apportion(n_occupied_locations, n_samples_total):
    """gen_train_data.py:70-76: crops per plot by occupied cells; the rounding remainder goes to the last plot."""
    n_samples = dict()
    n_occupied_total = sum(n_occupied_locations.values())
    plot = None
    for plot in n_occupied_locations:
        n_samples[plot] = int(np.round((n_occupied_locations[plot] / n_occupied_total) * n_samples_total))
    if not sum(n_samples.values()) == n_samples_total:
        n_samples[plot] = int(n_samples[plot] + (n_samples_total - sum(n_samples.values())))
    return n_samples


def _meta(plot_name, rotation_angle, cfg):
    """data_preparation.py:292-303, same keys in the same order."""
    return {"plot_name": plot_name, "rotation_angle": float(rotation_angle), "occupancy_res": cfg["occupancy_res"],
            "min_percent_occupied_fill": cfg["min_percent_occupied_fill"], "how_far_fill": cfg["how_far_fill"], "chunk_size": cfg["chunk_size"],
            "min_percent_occupied_choose": cfg["min_percent_occupied_choose"], "n_neigh_sor": cfg["n_neigh_sor"],
            "multiplier_sor": cfg["multiplier_sor"], "rad": cfg["rad"], "npoints_rad": cfg["npoints_rad"]}


def _load_plot(path_vox, path_feat, feature_names=("verticality",)):
    from .features import load_feature_cache
    d = np.load(path_vox)
    data = np.hstack((d["points"], d["labels"][:, np.newaxis]))                   # data_preparation.py:113-119
    feats = load_feature_cache(path_feat, feature_names)                          # ValueError: a cache written for another list
    return data[:, :3], data[:, 3], feats


def check_cfg(cfg):
    """The outlier-filter pairs of the config (util/outlier.py): a complete pair is accepted, a half-set one refused by name."""
    from .outlier import active_filters
    return active_filters({k: cfg.get(k) for k in _FILTER_KEYS})


def generate_random_crops(base_dir, cfg=None, seed=0, logger=None):
    """gen_train_data.py:15-97 on the device.  Reads base_dir/forests/* (segment.load_forest), writes the reference's
    forests_voxelized<v>/, features/, occupancy/ and random_crops/{npz,json}/; an intermediate file that already exists is
    reused, as in the reference (a cached occupancy grid also skips its random draw).

    Plots are processed in file-name order; the reference uses os.listdir order, which the file system decides.
    Returns {plot: number of crops written}."""
    from .features import check_feature_names, save_feature_cache
    from .prepare import compute_features, voxelize
    from .segment import load_forest
    cfg = dict(TRAIN_CFG, **(cfg or {}))
    filters = check_cfg(cfg)
    names = check_feature_names(cfg["feature_names"], for_model=True)             # before anything is written
    rs = np.random.RandomState(seed)
    say = (lambda m: logger.info(m)) if logger is not None else (lambda m: None)
    forests_dir = osp.join(base_dir, "forests")
    voxelized_dir = osp.join(base_dir, f"forests_voxelized{cfg['voxel_size']}")
    features_dir = osp.join(base_dir, "features")
    occupancy_dir = osp.join(base_dir, "occupancy")
    save_dir = osp.join(base_dir, "random_crops")
    for d in (voxelized_dir, features_dir, occupancy_dir, save_dir, osp.join(save_dir, "npz"), osp.join(save_dir, "json")):
        os.makedirs(d, exist_ok=True)

    say("voxelizing forests...")
    for plot_file in sorted(os.listdir(forests_dir)) if osp.isdir(forests_dir) else []:
        save_path = osp.join(voxelized_dir, f"{plot_file[:-4]}.npz")
        if osp.exists(save_path):
            continue
        data = load_forest(osp.join(forests_dir, plot_file))
        if data.shape[1] == 3:                                                    # load_data: unlabelled clouds get -1
            data = np.hstack([data, IGNORE_LABEL * np.ones(len(data))[:, np.newaxis]])
        vox, _ = voxelize(data, cfg["voxel_size"], round_first=True)
        vox = vox.cpu().numpy()
        np.savez_compressed(save_path, points=vox[:, :3].astype(np.float32), labels=np.round(vox[:, 3], 2).astype(np.float32))

    plot_files = sorted(os.listdir(voxelized_dir))
    say("calculating features...")
    for plot_file in plot_files:
        save_path = osp.join(features_dir, f"{plot_file[:-4]}.npz")
        if osp.exists(save_path):
            continue
        d = np.load(osp.join(voxelized_dir, plot_file))
        feats = compute_features(d["points"].astype(np.float64), search_radius=cfg["search_radius_features"], feature_names=names)
        save_feature_cache(save_path, feats.cpu().numpy(), names)

    say("calculating occupancy...")
    grids, n_occupied = {}, {}
    for plot_file in plot_files:
        occupancy_path = osp.join(occupancy_dir, plot_file)
        if osp.exists(occupancy_path):
            grid = np.load(occupancy_path)["occupancy_grid"]
        else:
            points, labels, _ = _load_plot(osp.join(voxelized_dir, plot_file), osp.join(features_dir, plot_file), names)
            grid = occupancy_grid(points, labels, rs, cfg["occupancy_res"], cfg["n_points_to_calculate_occupancy"], cfg["how_far_fill"],
                                  cfg["min_percent_occupied_fill"])["grid"]
            np.savez_compressed(occupancy_path, occupancy_grid=grid)
        grids[plot_file] = grid
        n_occupied[plot_file.replace(".npz", "")] = np.sum(grid[:, :, 2])
    n_samples = apportion(n_occupied, cfg["n_samples_total"])

    say("getting chunks...")
    written = {}
    for plot_file in plot_files:
        plot_name = osp.basename(plot_file)[:-4]
        points, labels, feats = _load_plot(osp.join(voxelized_dir, plot_file), osp.join(features_dir, plot_file), names)
        n_plot = n_samples[plot_file.replace(".npz", "")]
        x_range, y_range = get_ranges(points)
        centres, angles, rinv = crop_candidates(x_range, y_range, rs, cfg["n_samples_total"], n_plot)
        _, ok = check_occupancy(grids[plot_file], centres, rinv, cfg["chunk_size"], cfg["occupancy_res"], cfg["min_percent_occupied_choose"])
        n_pass = int(ok.sum())
        inds = choose(rs, n_pass, n_plot)
        written[plot_name] = len(inds)
        if len(inds) == 0:
            say(f"No valid candidates for plot {plot_name}")
            continue
        centres, angles, rinv = centres[ok][inds], angles[ok][inds], rinv[ok][inds]
        crops = extract_crops(points, labels, feats, centres, rinv, cfg["chunk_size"], filters=filters)
        for k, (xyz, inst, feat) in enumerate(crops):
            center = centres[k]
            data = dict(points=xyz, feat=feat, instance_label=inst, center=np.array([center[0], center[1], 0]))
            np.savez(osp.join(save_dir, "npz", f"{plot_name}_{k}.npz"), **data)
            with open(osp.join(save_dir, "json", f"{plot_name}_{k}.json"), "w") as f:
                json.dump(_meta(plot_name, angles[k], cfg), f)
    return written


# ------------------------------------------------------------------------------------------------ command line
def _number(s):
    """An int literal stays an int (it reaches the json files as the reference's yaml value would), anything else is a float."""
    try:
        return int(s)
    except ValueError:
        return float(s)


def parse_args(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.crops", description="generate random training crops from labelled forests")
    ap.add_argument("--base-dir", required=True, help="directory holding forests/ (npy / npz / txt / las, N x 4 with labels)")
    ap.add_argument("--seed", type=int, default=0)
    for k in ("n_samples_total", "chunk_size", "occupancy_res", "n_points_to_calculate_occupancy", "how_far_fill", "min_percent_occupied_fill",
              "min_percent_occupied_choose", "voxel_size", "search_radius_features"):
        ap.add_argument("--" + k.replace("_", "-"), type=_number, default=TRAIN_CFG[k])
    for k in _FILTER_KEYS:                                      # the outlier filters of util/outlier.py: off unless both keys of a pair are given
        ap.add_argument("--" + k.replace("_", "-"), type=_number, default=None)
    ap.add_argument("--feature-names", nargs="+", default=list(TRAIN_CFG["feature_names"]),
                    help="point features of the crops (util/features.py), at most 5, verticality last")
    a = ap.parse_args(argv)
    try:
        check_cfg({k: getattr(a, k) for k in _FILTER_KEYS})
        from .features import check_feature_names
        check_feature_names(a.feature_names, for_model=True)
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))
    for k in ("n_samples_total", "chunk_size", "occupancy_res", "n_points_to_calculate_occupancy", "voxel_size", "search_radius_features"):
        if not getattr(a, k) > 0:
            ap.error(f"--{k.replace('_', '-')} must be > 0")
    for k in ("n_samples_total", "n_points_to_calculate_occupancy", "how_far_fill"):
        if not isinstance(getattr(a, k), int):
            ap.error(f"--{k.replace('_', '-')} must be an integer")
    if a.how_far_fill < 0:
        ap.error("--how-far-fill must be >= 0")
    for k in ("min_percent_occupied_fill", "min_percent_occupied_choose"):
        if not 0 <= getattr(a, k) <= 1:
            ap.error(f"--{k.replace('_', '-')} must be in [0, 1]")
    if not osp.isdir(osp.join(a.base_dir, "forests")):
        ap.error(f"--base-dir {a.base_dir}: no forests/ directory")
    return a


def main(argv=None):
    import logging
    a = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    cfg = {k: getattr(a, k) for k in TRAIN_CFG if hasattr(a, k)}
    written = generate_random_crops(a.base_dir, cfg, seed=a.seed, logger=logging.getLogger("treelearn_amd.crops"))
    print(f"{sum(written.values())} crops from {len(written)} plots -> {osp.join(a.base_dir, 'random_crops')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
