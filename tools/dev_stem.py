"""Stage times of the stem profiles on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m,
about 1.89 M points, 64 trees, centred f32 coordinates resident on the device): tl_stem_keys, the key sort + gather + searchsorted,
tl_stem_profile and the copies to the host (those of the whole inventory with the profile) -- wall clock, each stage closed by a
device synchronise, median of 3 calls after a warm-up -- and the whole call with and without the stage.  For comparison the numpy
restatement of tests/stem_restatement.py (the profiles alone, from the inventory's table) on the same tile on the host's cores (one run;
a CPU-host number).

    python tools/dev_stem.py [restatement=1]"""
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

tree_inventory(xyz, lab, stem=True); torch.cuda.synchronize()        # warm-up: code objects, torch's sort
runs, whole, plain = [], [], []
for _ in range(REPS):
    st = []
    tree_inventory(xyz, lab, stem=True, stages=st)
    runs.append(dict(st))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    inv = tree_inventory(xyz, lab, stem=True)
    whole.append(time.perf_counter() - t0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    tree_inventory(xyz, lab)
    plain.append(time.perf_counter() - t0)
for name in ("stem keys", "stem sort + gather + searchsorted", "stem profile", "D2H"):
    res[name.replace(" + ", "_").replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs])), 3)
res["whole_call_with_stem_ms"] = round(1e3 * float(np.median(whole)), 3)
res["whole_call_without_stem_ms"] = round(1e3 * float(np.median(plain)), 3)
res["profile_width"] = int(inv["stem_profile"]["h"].shape[1])
res["accepted_slabs"] = int(inv["stem_slices"].sum())
res["trees_with_a_profile"] = int((inv["stem_slices"] > 0).sum())

if RESTATEMENT:
    import stem_restatement as ref
    h_xyz, h_lab = t["points"], t["instance_label"].astype(np.int64)
    t0 = time.perf_counter()
    want = ref.stem_profiles(h_xyz, h_lab, inv["x"], inv["y"], inv["z_low"], inv["z_top"])
    res["numpy_restatement_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["smallest_margin"] = float(min(want["margins"].values()))
    res["states_equal"] = bool(np.array_equal(inv["stem_profile"]["state"], want["stem_profile"]["state"]))
    res["max_abs_difference"] = float(max([np.nanmax(np.abs(inv["stem_profile"][k] - want["stem_profile"][k])) for k in ("x", "y", "r", "rmse")] +
                                          [np.nanmax(np.abs(inv[k] - want[k])) for k in ("stem_volume", "dbh_stem", "stem_lean", "stem_taper")]))
print(json.dumps(res))
