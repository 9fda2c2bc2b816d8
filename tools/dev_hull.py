"""Timing of the plot-edge path on one GPU: the ring lists + tl_ring_classify for 20 M f64 points against a 20 000-vertex
ring at r = 0.3 and 13.5, and the stages of segment_forest on a synthetic 68 m plot (random-init weights).  Median of 3 after a warm-up.

    python tools/dev_hull.py [n_points=20000000] [plot_edge_m=68]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from treelearn_amd.util import hull as H
from treelearn_amd.util import segment as S

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
E = float(sys.argv[2]) if len(sys.argv) > 2 else 68.0


def med(fn, reps=3):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


rng = np.random.default_rng(0)
V = 20001
a = np.sort(rng.uniform(0, 2 * np.pi, V - 1))
rad = 30 * (1 + 0.25 * np.sin(3 * a) + 0.02 * rng.normal(size=V - 1))
ring = np.column_stack([rad * np.cos(a), rad * np.sin(a)]); ring = np.vstack([ring, ring[:1]])
pts = (torch.rand((N, 3), dtype=torch.float64, device="cuda") - 0.5) * 90.0
for r in (0.3, 13.5):
    idx = {}
    t_build = med(lambda: idx.update(H._ring_index(ring, r, pts.device)))
    t_cls = med(lambda: H.ring_classify(pts, ring, r, idx))
    ent = idx["entries"]
    gb = (N * 24 + ent * 4 + (idx["grid"].nx * idx["grid"].ny + idx["grid"].nslab) * 8) / t_cls / 1e9
    print(f"r={r:5.1f}: lists {t_build * 1e3:7.2f} ms ({ent} entries, {idx['grid'].nx}x{idx['grid'].ny} cells, {idx['grid'].nslab} slabs); "
          f"classify {N / 1e6:.0f} M points {t_cls * 1e3:7.2f} ms = {gb:6.1f} GB/s of points + lists", flush=True)

from treelearn_amd.model import TreeLearn
from treelearn_amd.synth import make_tile, random_state_dict
t = make_tile(extent=E, voxel=0.1, n_trees=int(64 * (E / 40) ** 2), fill=0.10, seed=9)
plot = t["points"].astype(np.float64)
model = TreeLearn(**S.MODEL_CFG).cuda().eval(); model.load_state_dict(random_state_dict(7, channels=32, num_blocks=7))
T = {}
orig = {k: getattr(S, k) for k in ("voxelize", "compute_features", "get_pointwise_preds", "ensemble", "get_instances_device", "segment_from_pointwise")}


def timed(name, fn):
    def w(*a, **k):
        torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(*a, **k); torch.cuda.synchronize()
        T.setdefault(name, []).append(time.perf_counter() - t0)
        return out
    return w


for k, f in orig.items():
    setattr(S, k, timed(k, f))
shape = dict(outer_remove=5.0)
with torch.no_grad():
    tot = med(lambda: S.segment_forest(plot, model, grouping_cfg=dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20), shape_cfg=shape))
print(f"segment_forest, {E:.0f} m plot, {len(plot)} points, outer_remove 5 m: {tot:.2f} s (median of 3)")
for k, v in T.items():
    print(f"  {k:24s} {np.median(v[1:]) * 1e3:9.1f} ms")
