"""Stage times of the branch structure on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m,
about 1.89 M points, 64 trees, centred f32 coordinates resident on the device): tl_skel_voxel_keys, the key sort + unique,
tl_skel_distance, tl_skel_nodes, the node order + tl_skel_links, the copies to the host (those of the whole inventory with the node
table) and the branch rules on the host -- wall clock, each stage closed by a device synchronise, median of 3 calls after a warm-up --
and the whole call with and without the stage.  Then the reached share at reach 1 and reach 2, the bucket rounds, and the tree of the
most voxels alone: its rounds and the time of tl_skel_distance on it, which is what the stage waits for (one workgroup per tree).  For
comparison the Python restatement of tests/branches_restatement.py on the largest tree on the host (one run; a CPU-host number).

    python tools/dev_branches.py [restatement=1]"""
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
from treelearn_amd.util.branches import STAGES, branch_stage, check_params
from treelearn_amd.util.inventory import tree_inventory

RESTATEMENT = int(sys.argv[1]) if len(sys.argv) > 1 else 1
REPS = 3

t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
res = {"n_points": len(xyz), "n_trees": int(lab.max())}

tree_inventory(xyz, lab, branches=True); torch.cuda.synchronize()     # warm-up: code objects, torch's sort
runs, whole, plain = [], [], []
for _ in range(REPS):
    st = []
    tree_inventory(xyz, lab, branches=True, stages=st)
    runs.append(dict(st))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    inv = tree_inventory(xyz, lab, branches=True)
    whole.append(time.perf_counter() - t0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    tree_inventory(xyz, lab)
    plain.append(time.perf_counter() - t0)
for name in STAGES + ("D2H", "branch decomposition"):
    res[name.replace(" + ", "_").replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs])), 3)
res["whole_call_with_branches_ms"] = round(1e3 * float(np.median(whole)), 3)
res["whole_call_without_branches_ms"] = round(1e3 * float(np.median(plain)), 3)
res["voxels"], res["nodes"], res["branches"] = int(inv["skel_voxels"].sum()), int(inv["skel_nodes"].sum()), int(inv["branch_count"].sum())
res["reached_share_reach_1"] = round(float(inv["skel_reached"].sum() / inv["skel_voxels"].sum()), 5)
inv2 = tree_inventory(xyz, lab, branches=True, branch_cfg=dict(reach=2))
res["reached_share_reach_2"] = round(float(inv2["skel_reached"].sum() / inv2["skel_voxels"].sum()), 5)

# the stage once more on the device tensors for the rounds, and on the largest tree alone
order = torch.sort(lab, stable=True).indices
order = order[lab[order] >= 1]
rows, rlab = xyz[order].double().contiguous(), lab[order].contiguous()
table = torch.from_numpy(np.column_stack([inv["x"], inv["y"], inv["z_low"], inv["z_top"]])).cuda()
big = int(np.argmax(inv["skel_voxels"]))
res["largest_tree_voxels"] = int(inv["skel_voxels"][big])
for reach in (1, 2):
    p = check_params(reach=reach)
    dev = branch_stage(rows, rlab, len(table), table, p, lambda name: None)
    rounds = dev["rounds"].cpu().numpy()
    res[f"rounds_max_reach_{reach}"], res[f"rounds_largest_tree_reach_{reach}"] = int(rounds.max()), int(rounds[big])
    keep = rlab == big + 1
    one_rows, one_lab = rows[keep].contiguous(), rlab[keep].contiguous()
    branch_stage(one_rows, one_lab, len(table), table, p, lambda name: None)
    times = []
    for _ in range(REPS):
        st = []
        torch.cuda.synchronize(); t0 = [time.perf_counter()]

        def mark(name):
            torch.cuda.synchronize()
            now = time.perf_counter()
            st.append((name, now - t0[0]))
            t0[0] = now
        branch_stage(one_rows, one_lab, len(table), table, p, mark)
        times.append(dict(st)["branch distance"])
    res[f"largest_tree_distance_ms_reach_{reach}"] = round(1e3 * float(np.median(times)), 3)

if RESTATEMENT:
    import branches_restatement as ref
    keep = t["instance_label"] == big + 1
    h_xyz, h_lab = t["points"][keep].astype(np.float64), np.full(int(keep.sum()), big + 1, np.int64)
    t0 = time.perf_counter()
    want = ref.branch_structure(h_xyz, h_lab, inv["x"], inv["y"], inv["z_low"])
    res["python_restatement_largest_tree_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["smallest_margin"] = float(min(v for k, v in want["margins"].items() if k != "z_ref"))
    a, b = int(inv["skeleton"]["node_start"][big]), int(inv["skeleton"]["node_start"][big + 1])
    res["integers_equal"] = bool(all(inv[k][big] == want[k][big] for k in ref.BRANCH_INT) and
                                 all(np.array_equal(inv["skeleton"][k][a:b], want["skeleton"][k]) for k in ref.SKELETON_KEYS[1:]))
print(json.dumps(res))
