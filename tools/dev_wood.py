"""Stage times of the cylinder model on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m, about
1.89 M points, 64 trees, centred f32 coordinates resident on the device): tl_wood_row_nodes, the stable sort + searchsorted, tl_wood_fit
and the host rules (radii, frusta, columns) -- wall clock, each stage closed by a device synchronise, median of 3 calls after a
warm-up -- and the whole call with wood=True, with branches=True only and without either.  Then the number of nodes, the share fitted
(state 1), rejected (2) and without enough rows (0), the rows that belong to a node, the largest node's rows, and the stage times
against the bytes the stage must move: m (8 + 4) B for the keys and the map, two passes of m (24 + 8) B for the fit.

    python tools/dev_wood.py [reach=1]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from treelearn_amd.synth import make_tile
from treelearn_amd.util.inventory import tree_inventory
from treelearn_amd.util.wood import STAGES

REACH = int(sys.argv[1]) if len(sys.argv) > 1 else 1
REPS = 3
BCFG = dict(reach=REACH)

t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
res = {"n_points": len(xyz), "n_trees": int(lab.max()), "reach": REACH}

tree_inventory(xyz, lab, wood=True, branch_cfg=BCFG); torch.cuda.synchronize()       # warm-up: code objects, torch's sort
runs, whole, branches_only, plain = [], [], [], []
for _ in range(REPS):
    st = []
    tree_inventory(xyz, lab, wood=True, branch_cfg=BCFG, stages=st)
    runs.append(dict(st))
    for cost, kw in ((whole, dict(wood=True, branch_cfg=BCFG)), (branches_only, dict(branches=True, branch_cfg=BCFG)), (plain, {})):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        inv = tree_inventory(xyz, lab, **kw)
        cost.append(time.perf_counter() - t0)
for name in STAGES + ("D2H", "branch decomposition", "wood radii"):
    res[name.replace(" + ", "_").replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs])), 3)
res["whole_call_with_wood_ms"] = round(1e3 * float(np.median(whole)), 3)
res["whole_call_with_branches_ms"] = round(1e3 * float(np.median(branches_only)), 3)
res["whole_call_without_either_ms"] = round(1e3 * float(np.median(plain)), 3)

inv = tree_inventory(xyz, lab, wood=True, branch_cfg=BCFG)
cyl = inv["cylinders"]
m = int((t["instance_label"] >= 1).sum())
states = np.bincount(cyl["state"], minlength=3)
res["rows_of_trees"], res["nodes"] = m, len(cyl["state"])
res["share_fitted"], res["share_rejected"], res["share_too_few_rows"] = (round(float(v) / max(len(cyl["state"]), 1), 4) for v in (states[1], states[2], states[0]))
res["rows_in_a_node"], res["largest_node_rows"] = int(cyl["n"].sum()), int(cyl["n"].max()) if len(cyl["n"]) else 0
res["nodes_radius_is_fit"], res["wood_volume_m3"] = int(inv["wood_nodes_fit"].sum()), round(float(np.nansum(inv["wood_volume"])), 4)
res["bytes_row_nodes"], res["bytes_fit"] = m * (8 + 4), 2 * m * (24 + 8)
for name, b in (("wood row nodes", res["bytes_row_nodes"]), ("wood fit", res["bytes_fit"])):
    res[name.replace(" ", "_") + "_GBps"] = round(b / (1e6 * res[name.replace(" ", "_") + "_ms"]), 1)
print(json.dumps(res))
