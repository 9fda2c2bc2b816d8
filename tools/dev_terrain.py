"""Stage times of the terrain model on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m, about
1.89 M points, 64 trees, centred f32 coordinates resident on the device; its ground is a sloped, noisy surface): cell minima
(tl_dtm_min), slope filter (tl_dtm_filter), fill (tl_dtm_fill), the ground under every row (tl_dtm_sample), the tree stage (the ground
under the 64 positions + tl_tree_ground, as the difference of tree_inventory with and without a terrain) and the copies to the host
-- wall clock, each stage closed by a device synchronise, median of 3 calls after a warm-up.  For tl_dtm_min and tl_dtm_sample also
the bytes they move per second (rows read, results written; the grid stays in cache).  For comparison the numpy restatement of
tests/terrain_restatement.py on the same tile on the host's cores (one run; a CPU-host number).

    python tools/dev_terrain.py [restatement=1]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from treelearn_amd.synth import make_tile
from treelearn_amd.util.inventory import tree_inventory
from treelearn_amd.util.terrain import terrain_model

RESTATEMENT = int(sys.argv[1]) if len(sys.argv) > 1 else 1
REPS = 3

t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
n = len(xyz)
res = {"n_points": n, "n_trees": int(lab.max()), "n_candidates": int((lab == 0).sum())}


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


dtm = terrain_model(xyz, lab); dtm.height_above_ground(xyz); tree_inventory(xyz, lab, terrain=dtm); torch.cuda.synchronize()      # warm-up
runs = []
for _ in range(REPS):
    st = []
    dtm = terrain_model(xyz, lab, stages=st)
    r = dict(st)
    _, r["sample"] = timed(lambda: dtm.height_above_ground(xyz))
    _, with_t = timed(lambda: tree_inventory(xyz, lab, terrain=dtm))
    _, without = timed(lambda: tree_inventory(xyz, lab))
    r["tree stage"] = with_t - without
    host, r["D2H"] = timed(dtm.to_host)
    runs.append(r)
for name in runs[0]:
    res[name.replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs])), 3)
res["grid"] = [dtm.nx, dtm.ny]
res["cells_by_state"] = np.bincount(host["state"].reshape(-1), minlength=5).tolist()
esize = xyz.element_size()
res["min_bytes"] = n * (3 * esize + 8)                                   # x y z + the label per row
res["sample_bytes"] = n * (3 * esize + 8)                                # x y z per row, one f64 written
res["min_GBps"] = round(res["min_bytes"] / (res["min_ms"] * 1e-3) / 1e9, 1)
res["sample_GBps"] = round(res["sample_bytes"] / (res["sample_ms"] * 1e-3) / 1e9, 1)

if RESTATEMENT:
    import terrain_restatement as ref
    h_xyz, h_lab = t["points"], t["instance_label"].astype(np.int64)
    t0 = time.perf_counter()
    want = ref.terrain_model(h_xyz, h_lab)
    hag = ref.height_above_ground(want, h_xyz)
    res["numpy_restatement_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["state_equal"] = bool(np.array_equal(host["state"], want["state"]))
    res["max_abs_difference_z"] = float(np.nanmax(np.abs(host["z"] - want["z"])))
    res["max_abs_difference_hag"] = float(np.nanmax(np.abs(dtm.height_above_ground(xyz).cpu().numpy() - hag)))
print(json.dumps(res))
