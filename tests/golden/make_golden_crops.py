"""Generate tests/golden/g15_crops.npz (random training crops) by RUNNING the reference's own
tools/data_gen/gen_train_data.py:generate_random_crops and tree_learn/dataset/dataset.py:TreeDataset(training=True).
Run where the reference checkout is importable (only the .npz is committed):

    python tests/golden/make_golden_crops.py

Reuses make_golden.py's inert mocks (open3d and jakteristics are not installed: the voxelized and feature files are
pre-written into the reference's cache directories, so neither library is reached).  os.listdir is patched to sorted
order (the reference's plot order is the file system's).  Inputs: three seeded labelled plots from synth.make_tile pieces,
offset from the origin, about 5 % of the labels -1: 24 x 20 m, 30 x 30 m, and a 30 x 3 m strip on which no candidate passes.

Recorded per plot: occupancy steps, raw and filled grid, candidate centres / angles / inverse matrices, the filter and the
chosen indices; per crop: the json, the arrays' dtypes, shapes and SHA-1 digests; three crops in full; three TreeDataset
items after np.random.seed(S2) with every augmentation on and one collate_fn batch of two; the numpy version.

Boundary condition: no (cell, candidate) and no (point, chosen crop) pair may lie within 1e-9 m of chunk_size / 2 by
numpy's own values (the reference's BLAS and the kernels may round the rotated coordinates differently in the last bit);
seeds are tried in order until the inputs satisfy it.
"""
import hashlib
import importlib.util
import json
import logging
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402,F401  (mocks, reference and repository on sys.path)

from tree_learn.util import data_preparation as dp                               # noqa: E402
from tree_learn.dataset.dataset import TreeDataset                               # noqa: E402
from treelearn_amd.synth import make_tile                                        # noqa: E402

import tree_learn                                                                 # noqa: E402
REF_ROOT = os.path.dirname(os.path.abspath(list(tree_learn.__path__)[0]))         # the reference checkout make_golden put on sys.path
_spec = importlib.util.spec_from_file_location("gen_train_data", os.path.join(REF_ROOT, "tools", "data_gen", "gen_train_data.py"))
gtd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gtd)

CFG = dict(occupancy_res=1, n_points_to_calculate_occupancy=4000, min_percent_occupied_fill=0.9, how_far_fill=3,
           min_percent_occupied_choose=0.45, n_samples_total=12, chunk_size=10)
SAMPLE = dict(voxel_size=0.1, search_radius_features=0.6)
BAND = 1e-9
S2 = 7
FULL = ("plot_a_0", "plot_a_1", "plot_b_0")
AUG = dict(jitter=True, flip=True, rot=True, scaled=True, point_jitter=True)


class NS(dict):
    """The reference reads cfg.x and sets cfg.sample_generation.sample_generator.plot_path, then unpacks it with **."""
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def make_plots():
    rng = np.random.default_rng(15)
    out = {}
    for name, (ext, half_y, n_trees, seed, off, n_keep) in dict(plot_a=(24, 10.0, 5, 151, (412.37, -87.61), 6000),
                                                               plot_b=(30, 15.0, 8, 152, (-233.5, 1020.25), 7000),
                                                               plot_c=(30, 1.5, 2, 153, (58.1, 77.9), 1500)).items():
        t = make_tile(extent=ext, voxel=0.25, n_trees=n_trees, seed=seed)
        keep = np.abs(t["points"][:, 1]) <= half_y
        p, lab, f = t["points"][keep].astype(np.float64), t["instance_label"][keep], t["feat"][keep]
        sel = np.sort(rng.choice(len(p), size=min(n_keep, len(p)), replace=False))
        p, lab, f = p[sel], lab[sel].astype(np.float64), f[sel]
        p[:, 0] += off[0]; p[:, 1] += off[1]
        lab[rng.uniform(size=len(lab)) < 0.05] = -1
        out[name] = (np.round(p, 2).astype(np.float32), lab.astype(np.float32), f.astype(np.float32))
    return out


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(seed, plots):
    rec = {}
    base = tempfile.mkdtemp(prefix="tl_g15_")
    os.makedirs(os.path.join(base, "forests"))
    vdir = os.path.join(base, f"forests_voxelized{SAMPLE['voxel_size']}"); fdir = os.path.join(base, "features")
    os.makedirs(vdir); os.makedirs(fdir)
    for name, (p, lab, f) in plots.items():
        np.savez_compressed(os.path.join(vdir, f"{name}.npz"), points=p, labels=lab)
        np.savez_compressed(os.path.join(fdir, f"{name}.npz"), features=f)

    SG = dp.SampleGenerator
    orig = dict(get_occupancy_grid=SG.get_occupancy_grid, check_occupancy=SG.check_occupancy, save=SG.save, fill_holes=dp.fill_holes,
                choice=np.random.choice, listdir=os.listdir)

    def get_occupancy_grid(self, occupancy_path, res, n, how_far_fill, min_pct, ignore_for_occupancy):
        if not os.path.exists(occupancy_path):             # the reference's own step expressions (data_preparation.py:149-151)
            (x_res, x_dim), (y_res, y_dim) = dp.adjust_res(self.x_range, res), dp.adjust_res(self.y_range, res)
            r = rec.setdefault(self.plot_name, {})
            r["y_steps"] = np.arange(self.y_range[0], self.y_range[1] + 1e-3, step=y_res)
            r["x_steps"] = np.arange(self.x_range[0], self.x_range[1] + 1e-3, step=x_res)
            r["dims"] = np.array([x_dim, y_dim])
            rec["_current"] = self.plot_name
        return orig["get_occupancy_grid"](self, occupancy_path, res, n, how_far_fill, min_pct, ignore_for_occupancy)

    def fill_holes(grid, how_far_fill, min_pct):
        out = orig["fill_holes"](grid, how_far_fill, min_pct)
        r = rec[rec["_current"]]
        r["raw"] = grid[:, :, 2].copy(); r["filled"] = out[:, :, 2].copy(); r["grid"] = out.copy()
        return out

    def check_occupancy(self, min_pct_choose):
        orig["check_occupancy"](self, min_pct_choose)
        r = rec[self.plot_name]
        r["centers"] = self.centers.copy(); r["angles"] = self.rotation_angles.copy(); r["filter"] = self.filter.copy()
        r["rinv"] = np.stack([np.linalg.inv(np.array([[np.cos(a).item(), -np.sin(a).item()], [np.sin(a).item(), np.cos(a).item()]]))
                              for a in self.rotation_angles])
        cells = self.occupancy_grid.reshape(-1, 3)
        for a, c in zip(self.rotation_angles, self.centers):           # every (cell, candidate) pair, the reference's expressions
            d = np.linalg.norm(dp.invert_rotate_and_shift(cells[:, :2], a, c), ord=np.inf, axis=1)
            if np.any(np.abs(d - self.chunk_size / 2) < BAND):
                raise AssertionError("cell on a candidate's edge")

    def save(self, compressed=False):
        rec["_current"] = self.plot_name
        orig["save"](self, compressed)

    def choice(*a, **k):
        out = orig["choice"](*a, **k)
        rec[rec["_current"]]["inds"] = np.asarray(out, dtype=np.int64)
        return out

    SG.get_occupancy_grid, SG.check_occupancy, SG.save, dp.fill_holes = get_occupancy_grid, check_occupancy, save, fill_holes
    np.random.choice = choice
    os.listdir = lambda p=".": sorted(orig["listdir"](p))
    try:
        cfg = NS(base_dir=base, **CFG, sample_generation=NS(**SAMPLE, sample_generator=NS(n_neigh_sor=None, multiplier_sor=None, rad=None,
                                                                                                npoints_rad=None)))
        np.random.seed(seed)
        gtd.generate_random_crops(cfg)
    finally:
        SG.get_occupancy_grid, SG.check_occupancy, SG.save, dp.fill_holes = (orig["get_occupancy_grid"], orig["check_occupancy"], orig["save"],
                                                                             orig["fill_holes"])
        np.random.choice = orig["choice"]
        os.listdir = orig["listdir"]
    # every (point, chosen crop) pair, the reference's expressions on the whole plot
    for name, (p, lab, f) in plots.items():
        r = rec[name]
        ok = r["filter"]
        for k in r["inds"]:
            a, c = r["angles"][ok][k], r["centers"][ok][k]
            d = np.linalg.norm(dp.invert_rotate_and_shift(p[:, :2], a, c), ord=np.inf, axis=1)
            if np.any(np.abs(d - CFG["chunk_size"] / 2) < BAND):
                raise AssertionError("point on a crop's edge")
    rec.pop("_current")
    return base, rec


def main():
    plots = make_plots()
    for seed in range(15, 40):
        try:
            base, rec = run(seed, plots)
            break
        except AssertionError as e:
            print("seed", seed, "rejected:", e)
    else:
        raise SystemExit("no seed satisfies the boundary condition")
    OUT = {"numpy_version": np.array(np.__version__), "seed": seed, "cfg": np.array(json.dumps(CFG)), "sample": np.array(json.dumps(SAMPLE)),
           "plots": np.array(sorted(plots))}
    for name, (p, lab, f) in plots.items():
        OUT[f"in/{name}/points"], OUT[f"in/{name}/labels"], OUT[f"in/{name}/features"] = p, lab, f
        for k, v in rec[name].items():
            OUT[f"stage/{name}/{k}"] = v
    npz_dir = os.path.join(base, "random_crops", "npz"); json_dir = os.path.join(base, "random_crops", "json")
    names = sorted(f[:-4] for f in os.listdir(npz_dir))
    assert sorted(f[:-5] for f in os.listdir(json_dir)) == names
    OUT["crops"] = np.array(names)
    for n in names:
        d = np.load(os.path.join(npz_dir, n + ".npz"))
        OUT[f"json/{n}"] = np.array(open(os.path.join(json_dir, n + ".json")).read())
        OUT[f"keys/{n}"] = np.array(list(d.keys()))
        for k in d.keys():
            a = d[k]
            OUT[f"dtype/{n}/{k}"] = np.array(a.dtype.str); OUT[f"shape/{n}/{k}"] = np.array(a.shape)
            OUT[f"sha1/{n}/{k}"] = np.array(sha1(a))
        OUT[f"sha1/{n}/z"] = np.array(sha1(d["points"][:, 2]))
        OUT[f"sha1/{n}/xy"] = np.array(sha1(d["points"][:, :2]))
        if n in FULL:
            for k in d.keys():
                OUT[f"full/{n}/{k}"] = d[k]
    # TreeDataset(training=True) on the three full crops
    tmp = tempfile.mkdtemp(prefix="tl_g15_ds_")
    for n in FULL:
        shutil.copy(os.path.join(npz_dir, n + ".npz"), tmp)
    ds = TreeDataset(tmp, 4, True, logging.getLogger("golden"), data_augmentations=AUG)
    ds.data_paths = [os.path.join(tmp, n + ".npz") for n in FULL]
    np.random.seed(S2)
    items = [ds[i] for i in range(len(FULL))]
    batch = ds.collate_fn([items[0], items[1]])
    fields = ("xyz", "input_feat", "instance_label", "semantic_label", "pt_offset_label", "center", "mask_inner", "mask_off", "mask_sem")
    for i, it in enumerate(items):
        for k, v in zip(fields, it):
            OUT[f"item/{i}/{k}"] = v.numpy()
    for k, v in batch.items():
        OUT[f"batch/{k}"] = v.numpy() if torch.is_tensor(v) else np.array(v)
    OUT["ds/seed"], OUT["ds/inner"], OUT["ds/aug"] = S2, 4, np.array(json.dumps(AUG))
    shutil.rmtree(tmp); shutil.rmtree(base)
    path = os.path.join(HERE, "g15_crops.npz")
    np.savez_compressed(path, **OUT)
    print(path, os.path.getsize(path), "bytes; seed", seed, "crops", names)


if __name__ == "__main__":
    main()
