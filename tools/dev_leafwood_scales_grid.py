"""The grid behind the recommended leaf-wood scales, on the host, through the numpy restatements only
(tests/leafwood_scales_restatement.py, tests/features_restatement.py, tests/branches_restatement.py): the generated leaf-on tree of
tests/leafwood_cases.leaf_on_tree(), thresholds at their defaults, the vote at 0.2 m; every subset of {0.1, 0.2, 0.3, 0.4} with 2 or 3
members and every scales_min.  Per point: recall and precision of the wood flag, the kept components and skel_length on the wood rows.
One JSON line per point, the single-scale figure of §25 first.  No GPU.

    python tools/dev_leafwood_scales_grid.py"""
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np

import branches_restatement as br_ref
import inventory_restatement as inv_ref
import leafwood_cases as cases
import leafwood_restatement as ref
import leafwood_scales_restatement as sref

RADII = (0.1, 0.2, 0.3, 0.4)
xyz, lab, truth, length = cases.leaf_on_tree()
base = inv_ref.tree_inventory(xyz, lab)
tree = np.column_stack([base["x"], base["y"], base["z_low"], base["z_top"]])
order = np.argsort(lab, kind="stable")
kept = order[lab[order] >= 1]
feats = np.zeros((len(xyz), len(RADII), 4))
feats[kept], margin = sref.restate_features(xyz[kept], RADII)


def point(got, **tag):
    wood = got["wood"]
    tp = int((wood & truth).sum())
    rows = got["rows"]
    skel = float(br_ref.branch_structure(xyz[rows], lab[rows], tree[:, 0], tree[:, 1], tree[:, 2])["skel_length"][0])
    res = dict(tag, recall=round(tp / int(truth.sum()), 4), precision=round(tp / max(1, int(wood.sum())), 4), components=int(got["lw_components"][0]),
               skel_length=round(skel, 1))
    print(json.dumps(res), flush=True)


print(json.dumps(dict(rows=len(truth), wood=int(truth.sum()), true_limb_length=round(float(length), 1), radius_margin=margin)), flush=True)
point(ref.leafwood(xyz, lab, tree, {}, features=feats[:, 1, :]), scales=None, scales_min=1)
for size in (2, 3):
    for sub in itertools.combinations(range(len(RADII)), size):
        for k in range(1, size + 1):
            got = sref.leafwood_scales(xyz, lab, tree, {}, [RADII[i] for i in sub], k, features=feats[:, list(sub), :], margin=margin)
            point(got, scales=[RADII[i] for i in sub], scales_min=k)
