"""Generate tests/golden/g14_edge.npz (plot edge handling and propagation) by IMPORTING the reference's tree_learn/util/pipeline.py.
Run in the build container only (needs the reference checkout; only the .npz travels):

    python tests/golden/make_golden_edge.py

Reuses make_golden.py's inert mocks (geopandas, alphashape, shapely, laspy are not installed; none is touched by what runs here).
Inputs are seeded and stored; outputs are the reference's own:
  grid_points (0.25 m) on centred xy, get_cluster_means (float32 rows, pandas groupby), make_labels_consecutive after an outer removal,
  get_hash_values / get_hash_mapping / propagate_preds_hash_full (voxels without an ensemble row; the dictionary has no entry for a row
  without a voxel) / propagate_preds_hash_vox on a float32 cloud with rounding collisions,
  duplicates and unmatched points, and save_treewise(..., "npy", ...) into a temporary directory (file names per category, row counts).
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402,F401  (mocks, reference and repository on sys.path)

from tree_learn.util import pipeline as rp                                       # noqa: E402

OUT = {}
rng = np.random.default_rng(14)

# grid_points: 6 000 points of a 30 m plot at UTM-like magnitude, centred as get_hull does; some exact cell-boundary values
xy = rng.uniform(0, 30, size=(6000, 2)) + np.array([500000.0, 5500000.0])
xy[:200] = np.round(xy[:200] * 4) / 4
xyc = xy - np.mean(xy, axis=0, dtype=np.float64)
OUT["grid/in"] = xyc
OUT["grid/out"] = rp.grid_points(xyc, grid_size=0.25)

# get_cluster_means: float32 rows, labels 1..40 in random order
cm = (rng.normal(size=(10000, 3)) * np.array([20, 20, 5]) + np.array([3.0, -2.0, 10.0])).astype(np.float32)
cl = rng.integers(1, 41, size=10000)
OUT["means/coords"], OUT["means/labels"] = cm, cl
OUT["means/out"] = rp.get_cluster_means(cm, cl)

# make_labels_consecutive after an outer removal: tree labels with gaps where whole trees were removed
lab = rng.integers(0, 60, size=5000)
keep = rng.uniform(size=5000) < 0.7
keep &= ~np.isin(lab, [3, 17, 18, 41])
after = lab[keep].copy()
after[after != 0], _ = rp.make_labels_consecutive(after[after != 0], start_num=1)
OUT["consec/labels"], OUT["consec/keep"], OUT["consec/out"] = lab, keep, after

# hash propagation: voxel coordinates on a 0.01 m lattice (float32, as generate_tiles writes them), with duplicate voxels;
# ensemble rows = a shuffled subset of the voxels plus jitter below half a centimetre (rounding collisions), duplicates and misses
nv = 4000
vox = (np.round(rng.uniform(-20, 20, size=(nv, 3)) * 100) / 100).astype(np.float32)
vox[nv - 50:] = vox[:50]                                                   # 50 duplicate voxels (same rounded coordinates)
n_orig = 12000
p2v = np.concatenate([np.arange(nv), rng.integers(0, nv, size=n_orig - nv)])
rng.shuffle(p2v)
original_idx = [np.flatnonzero(p2v == v) for v in range(nv)]
hashes = rp.get_hash_values(vox)
mapping = rp.get_hash_mapping(hashes, original_idx)
sel = rng.choice(nv - 50, size=3000, replace=False)
ens = vox[sel] + rng.uniform(-0.004, 0.004, size=(3000, 3)).astype(np.float32)
ens = np.vstack([ens, ens[:100], (rng.uniform(-20, 20, size=(100, 3))).astype(np.float32)])   # duplicates, then rows without a voxel
preds = rng.integers(0, 30, size=len(ens))
coords_to_return = rng.normal(size=(n_orig, 3))
n_hit = 3100                                                               # the hash dictionary has no entry for the last 100 rows (KeyError)
full_pred, full_miss = rp.propagate_preds_hash_full(ens[:n_hit], preds[:n_hit], coords_to_return, mapping)
vox_pred, vox_miss = rp.propagate_preds_hash_vox(ens, preds, vox)
OUT.update({"hash/vox": vox, "hash/p2v": p2v, "hash/ens": ens, "hash/preds": preds, "hash/n_hit": n_hit,
            "hash/full_miss": full_miss, "hash/full_pred_matched": np.where(full_miss, -1, full_pred),
            "hash/vox_pred": vox_pred, "hash/vox_miss": vox_miss})

# save_treewise into a temporary directory, recorded as file names per category and row counts
ncl = 12
tc = rng.normal(size=(1500, 3)) * 10 + 100.0
tp = rng.integers(0, ncl + 1, size=1500)
within = rng.uniform(size=ncl) < 0.7
not_edge = rng.uniform(size=ncl) < 0.6
with tempfile.TemporaryDirectory() as d:
    rp.save_treewise(tc, tp, within, not_edge, "npy", d, 0)
    names, rows = [], []
    for root, _, files in os.walk(d):
        for f in sorted(files):
            names.append(os.path.relpath(os.path.join(root, f), d))
            rows.append(len(np.load(os.path.join(root, f))))
order = np.argsort(names)
OUT.update({"treewise/coords": tc, "treewise/preds": tp, "treewise/within": within, "treewise/not_edge": not_edge,
            "treewise/files": np.array(names)[order], "treewise/rows": np.array(rows)[order]})

path = os.path.join(HERE, "g14_edge.npz")
np.savez_compressed(path, **OUT)
print(path, os.path.getsize(path), "bytes")
