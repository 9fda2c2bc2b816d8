"""Timing of the random training-crop generator on one GPU: the stages of util/crops.py on the synthetic 68 m plot
(synth.make_plot, ~5.5 M points) with the default config (chunk 35 m, occupancy 1 m, 100 000 occupancy points, fill 9), median of 3
after a warm-up; extraction also as GB/s of its algorithmic bytes (the plot read once per batch + the rows written), npz / json writing
per crop, and the host cost of one CropDataset item.

    python tools/dev_crops.py [n_crops=64] [work_dir=a new temporary directory]"""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from treelearn_amd import _hip
from treelearn_amd.synth import make_plot
from treelearn_amd.util import crops as C
from treelearn_amd.util.dataset import ALL_AUGMENTATIONS, CropDataset

NC = int(sys.argv[1]) if len(sys.argv) > 1 else 64
OUT = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="tl_dev_crops_")
cfg = C.TRAIN_CFG


def med(fn, reps=3):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


t = make_plot()
pts = torch.from_numpy(t["points"]).cuda(); lab = torch.from_numpy(t["instance_label"].astype(np.float32)).cuda()
feat = torch.from_numpy(t["feat"]).cuda()
n, F = len(pts), feat.shape[1]
res = {"n_points": n}
o = {}
res["occupancy_ms"] = 1e3 * med(lambda: o.update(C.occupancy_grid(pts, lab, np.random.RandomState(0), cfg["occupancy_res"],
                                                                   cfg["n_points_to_calculate_occupancy"], cfg["how_far_fill"],
                                                                   cfg["min_percent_occupied_fill"])))
X, Y = o["raw"].shape
raw = torch.from_numpy(o["raw"]).cuda(); filled = torch.empty_like(raw)
res["fill_kernel_ms"] = 1e3 * med(lambda: _hip.check(_hip.lib().tl_crops_fill(_hip.ptr(raw), X, Y, cfg["how_far_fill"], cfg["min_percent_occupied_fill"],
                                                                               _hip.ptr(filled), _hip.stream()), "fill"))
xr, yr = C.get_ranges(pts)
cand = {}
res["candidates_host_ms"] = 1e3 * med(lambda: cand.update(zip(("c", "a", "r"), C.crop_candidates(xr, yr, np.random.RandomState(1), NC, NC))))
ok = {}
res["check_ms"] = 1e3 * med(lambda: ok.update(zip(("s", "ok"), C.check_occupancy(o["grid"], cand["c"], cand["r"], cfg["chunk_size"], cfg["occupancy_res"],
                                                                                  cfg["min_percent_occupied_choose"]))))
res.update(grid=[X, Y], candidates=len(cand["c"]), passing=int(ok["ok"].sum()))
sel = np.flatnonzero(ok["ok"])[:NC]
c, r = cand["c"][sel], cand["r"][sel]
crops = []
t_ex = med(lambda: crops.__setitem__(slice(None), list(C.extract_crops(pts, lab, feat, c, r, cfg["chunk_size"]))))
rows = sum(len(p) for p, _, _ in crops)
batches = -(-len(sel) // C.MAX_BATCH)
algo = batches * n * (12 + 4 + 4 * F) + rows * (12 + 4 + 4 * F)
res.update(crops=len(sel), rows_per_crop=rows / len(sel), extract_ms_per_crop=1e3 * t_ex / len(sel), extract_gbps_incl_d2h=algo / t_ex / 1e9)

# the kernels alone (count + extract of one batch of 32, no D2H), events on the stream
L = _hip.lib(); nc = min(C.MAX_BATCH, len(sel))
dc = torch.from_numpy(np.ascontiguousarray(c[:nc])).cuda(); dr = torch.from_numpy(np.ascontiguousarray(r[:nc])).cuda()
ws = torch.empty(int(L.tl_crops_ws_words(n, nc)), dtype=torch.int32, device="cuda"); cnt = torch.empty(nc, dtype=torch.int32, device="cuda")
cap = sum(len(p) for p, _, _ in crops[:nc])
ox = torch.empty((cap, 3), device="cuda"); ol = torch.empty(cap, dtype=torch.int32, device="cuda"); of = torch.empty((cap, F), device="cuda")


def kernels():
    _hip.check(L.tl_crops_count(_hip.ptr(pts), n, nc, _hip.ptr(dc), _hip.ptr(dr), float(cfg["chunk_size"]), _hip.ptr(cnt), _hip.ptr(ws), _hip.stream()), "count")
    _hip.check(L.tl_crops_extract(_hip.ptr(pts), _hip.ptr(lab), _hip.ptr(feat), n, F, nc, _hip.ptr(dc), _hip.ptr(dr), float(cfg["chunk_size"]), _hip.ptr(ws),
                                  cap, _hip.ptr(ox), _hip.ptr(ol), _hip.ptr(of), _hip.stream()), "extract")


def ev_time():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); kernels(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kernels(); torch.cuda.synchronize()
t_k = float(np.median([ev_time() for _ in range(5)])) / 1e3
res.update(kernels_ms_per_batch32=1e3 * t_k, kernels_ms_per_crop=1e3 * t_k / nc, kernels_gbps=(n * (12 + 4 + 4 * F) + cap * (12 + 4 + 4 * F)) / t_k / 1e9)

# npz + json per crop (the reference's np.savez, uncompressed), then one CropDataset item from a written crop
d = os.path.join(OUT, "npz"); os.makedirs(d, exist_ok=True)
nw = min(8, len(crops))


def write():
    for k in range(nw):
        p, il, f = crops[k]
        np.savez(os.path.join(d, f"plot_{k}.npz"), points=p, feat=f, instance_label=il, center=np.array([c[k][0], c[k][1], 0]))
        with open(os.path.join(OUT, f"plot_{k}.json"), "w") as fh:
            json.dump(C._meta("plot", 0.5, cfg), fh)


res["write_ms_per_crop"] = 1e3 * med(write) / nw
ds = CropDataset(d, 8, True, ALL_AUGMENTATIONS, seed=0)
res["dataset_item_ms"] = 1e3 * med(lambda: [ds[k] for k in range(nw)]) / nw
shutil.rmtree(OUT)
print(json.dumps(res))
