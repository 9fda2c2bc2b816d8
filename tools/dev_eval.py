"""Forest scoring stage by stage on the 68 m synthetic plot (synth.make_plot: about 5.4 M points, 185 trees): one JSON line of per-stage
milliseconds of treelearn_amd.util.eval.evaluate_forest -- propagation (5-NN vote onto the ground-truth points), contingency table,
Hungarian matching with the failure analysis, xy bands, z bands, total.  The prediction cloud is a jittered 70 % subsample of the plot
with a merge, a split and 5 % label noise.  The median of `--reps` timed runs after one warm-up run.

    python tools/dev_eval.py [--reps 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from treelearn_amd.synth import make_plot  # noqa: E402
from treelearn_amd.util.eval import evaluate_forest  # noqa: E402


def prediction(xyz, labels, seed=0):
    rng = np.random.default_rng(seed)
    keep = rng.random(len(xyz)) < 0.7
    pxyz = (xyz[keep] + rng.normal(0, 0.005, (keep.sum(), 3))).astype(np.float32)
    lab = labels[keep].astype(np.int64).copy()
    ids = np.unique(lab[lab > 0])
    lab[lab == ids[1]] = ids[0]                                              # merge
    t = lab == ids[2]
    lab[t & (pxyz[:, 0] > np.median(pxyz[t, 0]))] = ids.max() + 1          # split
    flip = rng.random(len(lab)) < 0.05
    lab[flip] = rng.choice(np.concatenate([[0], ids]), flip.sum())         # noise
    return pxyz, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    t = make_plot()
    xyz, lab = t["points"], t["instance_label"].astype(np.int64)
    pxyz, plab = prediction(xyz, lab)
    gxyz = xyz.astype(np.float64)
    evaluate_forest(gxyz, lab, pxyz, plab, frames=False)                     # warm-up (library load, allocator, scipy import)
    runs = []
    for _ in range(a.reps):
        tm = {}
        res, _ = evaluate_forest(gxyz, lab, pxyz, plab, frames=False, timings=tm)
        runs.append(tm)
    keys = ["inputs", "propagation", "contingency", "hungarian", "xy", "z", "aggregate"]
    med = {k: float(np.median([r[k] for r in runs])) for k in keys}
    med["total"] = float(np.median([sum(r[k] for k in keys) for r in runs]))
    out = {"points": int(len(xyz)), "pred_points": int(len(pxyz)), "gt_trees": int(len(np.unique(lab[lab > 0]))), "reps": a.reps,
           "ms": {k: round(v, 2) for k, v in med.items()},
           "f1": float(res["detection_results"]["f1_score"]), "coverage": float(res["segmentation_results"]["iou"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
