"""Stage times of the crown structure on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m,
about 1.89 M points, 64 trees, centred f32 coordinates resident on the device): tl_crown_voxel_keys, the key sort + searchsorted,
tl_crown_structure and the copies to the host (those of the whole inventory with the profile) -- wall clock, each stage closed by a
device synchronise, median of 3 calls after a warm-up -- and the whole call with and without the stage.  For comparison the numpy
restatement of tests/crown_restatement.py (the crown columns alone, from the inventory's table) on the same tile on the host's cores (one
run; a CPU-host number) and the largest difference between the two.

    python tools/dev_crown.py [restatement=1]"""
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

tree_inventory(xyz, lab, crown=True); torch.cuda.synchronize()       # warm-up: code objects, torch's sort
runs, whole, plain = [], [], []
for _ in range(REPS):
    st = []
    tree_inventory(xyz, lab, crown=True, stages=st)
    runs.append(dict(st))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    inv = tree_inventory(xyz, lab, crown=True)
    whole.append(time.perf_counter() - t0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    tree_inventory(xyz, lab)
    plain.append(time.perf_counter() - t0)
for name in ("crown voxel keys", "crown sort + searchsorted", "crown structure", "D2H"):
    res[name.replace(" + ", "_").replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs])), 3)
res["whole_call_with_crown_ms"] = round(1e3 * float(np.median(whole)), 3)
res["whole_call_without_crown_ms"] = round(1e3 * float(np.median(plain)), 3)
res["profile_width"] = int(inv["crown_profile"]["h"].shape[1])
res["crown_voxels"] = int(inv["crown_voxels"].sum())
res["trees_with_a_crown"] = int((inv["crown_proj_cells"] > 0).sum())

if RESTATEMENT:
    import crown_restatement as ref
    h_xyz, h_lab = t["points"], t["instance_label"].astype(np.int64)
    t0 = time.perf_counter()
    want = ref.crown_structure(h_xyz, h_lab, inv["x"], inv["y"], inv["z_low"], inv["z_top"])
    res["numpy_restatement_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["smallest_margin"] = float(min(v for k, v in want["margins"].items() if k != "layer"))     # (z_ref = z_low: the layers are exact)
    res["integers_equal"] = bool(all(np.array_equal(inv[k], want[k]) for k in ref.CROWN_INT) and
                                 all(np.array_equal(inv["crown_profile"][k], want["crown_profile"][k]) for k in ("n", "cells")))
    with np.errstate(invalid="ignore"):
        res["max_abs_difference"] = float(max([np.nanmax(np.abs(inv["crown_profile"]["radii"] - want["crown_profile"]["radii"]))] +
                                              [np.nanmax(np.abs(inv[k] - want[k])) for k in ref.CROWN_COLUMNS if k not in ref.CROWN_INT]))
print(json.dumps(res))
