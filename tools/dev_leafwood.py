"""Stage times of the leaf-wood separation on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m, about
1.89 M points, 64 trees, centred f32 coordinates resident on the device): the cell sort, the features, the seed rule, every vote round,
the voxel keys + unique, the components and the scatter -- wall clock, each stage closed by a device synchronise, median of 3 calls after a
warm-up -- and the whole call with and without leafwood, with branches=True with the filter, without it and without leafwood (and what
the filter does to tl_skel_distance).  Then the candidates tl_leafwood_vote stages per round (the same ranges tl_eigen_features stages),
the bytes it must move (28 B per staged candidate, 1 + 4 B stored per row) and the rates they give.

    python tools/dev_leafwood.py [vote_iters=2]"""
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
from treelearn_amd.util.leafwood import check_params, stages_of
from treelearn_amd.util.prepare import feature_pieces, sorted_cells

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 2
REPS = 3
CFG = check_params(vote_iters=ITERS)

t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
res = {"n_points": len(xyz), "n_trees": int(lab.max()), "vote_iters": ITERS}

CALLS = (("leafwood", dict(leafwood=True, leafwood_cfg=CFG)), ("plain", {}),
         ("branches_filter", dict(branches=True, leafwood=True, leafwood_cfg=CFG)),
         ("branches_no_filter", dict(branches=True, leafwood=True, leafwood_cfg=dict(CFG, filter=False))), ("branches_only", dict(branches=True)))
for _, kw in CALLS:
    tree_inventory(xyz, lab, **kw)                                                    # warm-up: code objects, torch's sort
torch.cuda.synchronize()
runs, cost = {name: [] for name, _ in CALLS}, {name: [] for name, _ in CALLS}
for _ in range(REPS):
    for name, kw in CALLS:
        st = []
        tree_inventory(xyz, lab, stages=st, **kw)
        runs[name].append(dict(st))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        tree_inventory(xyz, lab, **kw)
        cost[name].append(time.perf_counter() - t0)


def med(name, stage):
    return round(1e3 * float(np.median([r[stage] for r in runs[name]])), 3)


for stage in stages_of(CFG) + ("leafwood scatter",):
    res[stage.replace(" + ", "_").replace(" ", "_") + "_ms"] = med("leafwood", stage)
for name, _ in CALLS:
    res[f"whole_call_{name}_ms"] = round(1e3 * float(np.median(cost[name])), 3)
for name in ("branches_filter", "branches_no_filter", "branches_only"):
    res[f"branch_distance_{name}_ms"] = med(name, "branch distance")

inv = tree_inventory(xyz, lab, leafwood=True, leafwood_cfg=CFG)
m = int((t["instance_label"] >= 1).sum())
res["rows_of_trees"], res["wood_rows"], res["components"] = m, int(inv["lw_wood_points"].sum()), int(inv["lw_components"].sum())

# the candidates one vote round stages: per piece the nine ranges of tl_leafwood_vote / tl_eigen_features
g = xyz[lab >= 1].double()
sx, keys, perm, ext = sorted_cells(g, CFG["radius"])
pieces = feature_pieces(keys)
n, B, mask = len(keys), 21, (1 << 21) - 1
last = torch.cat([pieces[1:], torch.tensor([n], device=keys.device)]) - 1
k0, k1 = keys[pieces], keys[last]
cx, cy, z0, z1 = k0 >> (2 * B), (k0 >> B) & mask, ((k0 & mask) - 1).clamp(min=0), ((k1 & mask) + 1).clamp(max=mask)
staged = 0
for dx in (-1, 0, 1):
    for dy in (-1, 0, 1):
        x, y = cx + dx, cy + dy
        ok = (x >= 0) & (x <= ext[0]) & (y >= 0) & (y <= ext[1])
        kb = (x << (2 * B)) | (y << B)
        lo, hi = torch.searchsorted(keys, kb | z0), torch.searchsorted(keys, (kb | z1) + 1)
        staged += int(((hi - lo) * ok).sum())
res["pieces"], res["candidates_staged_per_round"] = len(pieces), staged
res["bytes_vote_round"] = 28 * staged + 5 * m
vote_ms = float(np.median([res[f"leafwood_vote_{i + 1}_ms"] for i in range(ITERS)])) if ITERS else float("nan")
res["vote_GBps"] = round(res["bytes_vote_round"] / (1e6 * vote_ms), 1) if ITERS else None
res["vote_candidates_per_us"] = round(staged / (1e3 * vote_ms), 1) if ITERS else None
res["features_candidates_per_us"] = round(staged / (1e3 * res["leafwood_features_ms"]), 1)
print(json.dumps(res))
