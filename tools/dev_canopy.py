"""Stage times of the canopy height model on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m,
about 1.89 M points, 64 trees, centred f32 coordinates resident on the device) with its terrain built beforehand: height above ground
(tl_dtm_sample), the extents, cell maxima (tl_chm_max), owners (tl_chm_owner), pits (tl_chm_pits), tops (tl_chm_tops, nonzero and the
gathers), keys (tl_canopy_keys), the two sorts with the gathers and range starts, the metrics (tl_grid_metrics) and the copies to the
host -- wall clock, each stage closed by a device synchronise, median of 3 calls after a warm-up.  For the row passes also the bytes
they move per second (rows read, results written; the grids stay in cache).  For comparison the numpy restatement of
tests/canopy_restatement.py on every 16th row of the tile on the host's cores (one run; a CPU-host number).

    python tools/dev_canopy.py [restatement=1]"""
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
from treelearn_amd.util.canopy import canopy_model, stand_summary
from treelearn_amd.util.terrain import terrain_model

RESTATEMENT = int(sys.argv[1]) if len(sys.argv) > 1 else 1
REPS = 3

t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
n = len(xyz)
res = {"n_points": n, "n_trees": int(lab.max())}


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


dtm = terrain_model(xyz, lab)
canopy_model(xyz, dtm, lab).to_host(); torch.cuda.synchronize()                     # warm-up
runs = []
for _ in range(REPS):
    st = []
    c = canopy_model(xyz, dtm, lab, stages=st)
    r = dict(st)
    host, r["D2H"] = timed(c.to_host)
    runs.append(r)
for name in runs[0]:
    res[name.replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs])), 3)
res["total_ms"] = round(sum(v for k, v in res.items() if k.endswith("_ms")), 3)
res["chm_grid"] = [c.nx, c.ny]
res["metrics_grid"] = [c.metric_nx, c.metric_ny, int(c.layers.shape[2])]
res["cells_by_state"] = np.bincount(host["state"].reshape(-1), minlength=4).tolist()
res["n_tops"] = int(len(host["tops_h"]))
res["n_no_ground"], res["n_clipped"] = c.n_no_ground, c.n_clipped
res["stand"] = stand_summary(host)
esize = xyz.element_size()
# bytes per row of each row pass: x y (z rides along in the same lines: 3 values counted) + h read; what the pass writes per row
res["bytes"] = dict(hag=n * (3 * esize + 8), maxima=n * (3 * esize + 8), owners=n * (3 * esize + 8), keys=n * (3 * esize + 8 + 8),
                    sorts=n * (8 + 8 + 8) * 2 + n * (8 + 8 + 8), metrics=n * 8 * 3)
for k, b in res["bytes"].items():
    res[k + "_GBps"] = round(b / (res[k + "_ms"] * 1e-3) / 1e9, 1)

if RESTATEMENT:
    import canopy_restatement as ref
    sub = slice(None, None, 16)
    h_xyz, h_lab = t["points"][sub], t["instance_label"].astype(np.int64)[sub]
    h_h = dtm.height_above_ground(xyz).cpu().numpy()[sub]
    t0 = time.perf_counter()
    want = ref.canopy_model(h_xyz, h_h, h_lab)
    res["numpy_restatement_of_every_16th_row_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    got = canopy_model(h_xyz, labels=h_lab, height_above_ground=h_h)
    res["chm_equal"] = bool(np.array_equal(got.chm.cpu().numpy(), want["chm"], equal_nan=True))
    res["percentiles_equal"] = bool(np.array_equal(got.percentiles.cpu().numpy(), want["percentiles"], equal_nan=True))
    res["max_abs_difference_h_mean"] = float(np.nanmax(np.abs(got.h_mean.cpu().numpy() - want["h_mean"])))
print(json.dumps(res))
