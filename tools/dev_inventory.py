"""Stage times of the per-tree inventory on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m,
about 1.89 M points, 64 trees, centred f32 coordinates resident on the device): label sort + gather, tl_tree_inventory, crown keys +
sort + count, the copies to the host -- wall clock, each stage closed by a device synchronise, median of 3 calls after a warm-up --
and the whole call.  For comparison the numpy restatement of tests/inventory_restatement.py on the same tile on the host's cores
(one run; a CPU-host number).

    python tools/dev_inventory.py [restatement=1]"""
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

RESTATEMENT = int(sys.argv[1]) if len(sys.argv) > 1 else 1
REPS = 3

t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
res = {"n_points": len(xyz), "n_trees": int(lab.max())}

tree_inventory(xyz, lab); torch.cuda.synchronize()                   # warm-up: code objects, torch's sort
runs, whole = [], []
for _ in range(REPS):
    st = []
    tree_inventory(xyz, lab, stages=st)
    runs.append(dict(st))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    inv = tree_inventory(xyz, lab)
    whole.append(time.perf_counter() - t0)
for name in runs[0]:
    res[name.replace(" + ", "_").replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs])), 3)
res["whole_call_ms"] = round(1e3 * float(np.median(whole)), 3)
res["rows_of_trees"] = int(inv["n_points"].sum())
res["largest_tree_rows"] = int(inv["n_points"].max())
res["trees_with_dbh"] = int(np.isfinite(inv["dbh"]).sum())

if RESTATEMENT:
    import inventory_restatement as ref
    h_xyz, h_lab = t["points"], t["instance_label"].astype(np.int64)
    t0 = time.perf_counter(); want = ref.tree_inventory(h_xyz, h_lab); res["numpy_restatement_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["max_abs_difference"] = float(max(np.nanmax(np.abs(inv[k] - want[k])) for k in ("x", "y", "z", "dbh", "dbh_x", "dbh_y", "dbh_rmse")))
    res["exact_columns_equal"] = bool(all(np.array_equal(inv[k], want[k], equal_nan=True) for k in ("n_points", "z_low", "z_top", "height", "dbh_n", "crown_cells")))
print(json.dumps(res))
