"""Stage times of the outlier filters on one GPU, on the bench tile (synth.make_tile: 40 x 40 m, about 1.87 M points,
the centred f32 coordinates a tile crop hands to the filter): cell keys + sort + gather, tl_knn_mean_dist for k in {2, 20},
tl_sor_keep, tl_radius_count at r = 0.25, a whole `denoise` per setting (median of 5 after a warm-up, events on the stream for the
kernels, wall clock with a synchronise for the host-level calls), scipy's cKDTree on the host's cores for context, and the per-tile
time of PlotTiler.tiles with and without the filters.

    python tools/dev_outlier.py [tiles=1] [kdtree=1]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from treelearn_amd import _hip
from treelearn_amd.synth import make_tile
from treelearn_amd.util import outlier as O
from treelearn_amd.util.tiles import PlotTiler

TILES = int(sys.argv[1]) if len(sys.argv) > 1 else 1
KDTREE = int(sys.argv[2]) if len(sys.argv) > 2 else 1
KS, RAD, NB, S = (2, 20), 0.25, 5, 1.0


def wall(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def ev(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda().double().contiguous()
n = len(xyz)
L = _hip.lib()
res = {"n_points": n}
for k in KS:
    g = O._Grid(xyz, O.knn_cell(k))
    avg = torch.empty(n, dtype=torch.float64, device="cuda")
    res[f"k{k}_cell_m"] = g.h
    res[f"k{k}_sort_ms"] = wall(lambda: O._Grid(xyz, O.knn_cell(k)))
    res[f"k{k}_knn_kernel_ms"] = ev(lambda: _hip.check(L.tl_knn_mean_dist(_hip.ptr(g.xyz), _hip.ptr(g.keys), _hip.ptr(g.perm), n, g.lo, g.h, g.dims, k,
                                                                          _hip.ptr(avg), _hip.stream()), "knn"))
    res[f"k{k}_sor_keep_ms"] = ev(lambda: O.sor_keep(avg, S))
    res[f"k{k}_sor_filter_ms"] = wall(lambda: O.sor_filter(xyz, k, S))
    res[f"k{k}_kept"] = int(O.sor_filter(xyz, k, S).sum())
    res[f"k{k}_denoise_both_ms"] = wall(lambda: O.denoise(xyz, dict(n_neigh_sor=k, multiplier_sor=S, rad=RAD, npoints_rad=NB)))
g = O._Grid(xyz, 1.001 * RAD)
cnt = torch.empty(n, dtype=torch.int32, device="cuda")
res["rad_sort_ms"] = wall(lambda: O._Grid(xyz, 1.001 * RAD))
res["rad_count_kernel_ms"] = ev(lambda: _hip.check(L.tl_radius_count(_hip.ptr(g.xyz), _hip.ptr(g.keys), _hip.ptr(g.perm), n, g.lo, g.h, g.dims, RAD,
                                                                     _hip.ptr(cnt), _hip.stream()), "radius"))
res["rad_filter_ms"] = wall(lambda: O.rad_filter(xyz, RAD, NB))
res["rad_kept"] = int(O.rad_filter(xyz, RAD, NB).sum())
res["rad_mean_count"] = float(cnt.double().mean())

if KDTREE:
    try:
        from scipy.spatial import cKDTree
        h = xyz.cpu().numpy()
        t0 = time.perf_counter(); tree = cKDTree(h); res["kdtree_build_ms"] = 1e3 * (time.perf_counter() - t0)
        for k in KS:
            t0 = time.perf_counter(); tree.query(h, k=k, workers=16); res[f"kdtree_k{k}_query_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter(); tree.query_ball_point(h, RAD, workers=16, return_length=True); res["kdtree_radius_ms"] = 1e3 * (time.perf_counter() - t0)
    except ImportError:
        res["kdtree"] = "scipy is not installed"

if TILES:
    tiler = PlotTiler(t["points"], t["instance_label"].astype(np.float32), t["feat"])

    def run(gen):
        def go():
            for b in tiler.tiles(8.0, 13.5, 1.0, 8.0, offset_labels="none", sample_generator=gen):
                b["_ready_event"].synchronize()
        return go
    n_tiles = sum(1 for _ in tiler.tiles(8.0, 13.5, 1.0, 8.0, offset_labels="none"))
    res["tiles"] = n_tiles
    res["tile_ms_no_filter"] = wall(run(None), reps=3) / n_tiles
    for k in KS:
        res[f"tile_ms_sor_k{k}"] = wall(run(dict(n_neigh_sor=k, multiplier_sor=S)), reps=3) / n_tiles
    res["tile_ms_rad"] = wall(run(dict(rad=RAD, npoints_rad=NB)), reps=3) / n_tiles
print(json.dumps(res))
