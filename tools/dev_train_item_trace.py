"""Dev: the passes of tl_train_item one by one, and how often numpy's partition pick is not rank 3.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/dev_train_item_trace.py item --mode training [--offset 1]
    python tools/dev_train_item_trace.py rank3

  item   tl_train_item on the config-2 seed-0 tile (40 m, 1.89 M rows, 65 labels), `--reps` calls after a warm-up round.  Inputs (6 copies)
         and outputs (4 batches) rotate, so about 600 MB lie between two uses of the same buffer and no call finds its rows in the 256 MB
         Infinity Cache.  One mode per process: under rocprofv3 the kernel statistics are then per pass of that mode.  `--offset` is the
         batch row the item starts at (0: 16-byte input loads in k_write; 1: the row-by-row loads a batch's second item takes).
         Without rocprofv3 it prints the whole call's time from device events.
  rank3  host only: the 64 overlapping 40 m tiles of the 68 m synthetic plot; per tree instance of more than 11 rows,
         np.partition(z, 10)[3] against np.sort(z)[3], for the stored z and for the z of the RandomState(3) matrix.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def item(a):
    import torch
    from treelearn_amd.synth import make_tile
    from treelearn_amd.util.device_dataset import ItemWorkspace, alloc_batch, train_item
    dev = torch.device("cuda")
    t = make_tile(seed=0)
    n = len(t["points"])
    res = [(torch.from_numpy(t["points"]).to(dev), torch.from_numpy(t["instance_label"]).to(dev)) for _ in range(6)]
    outs = [alloc_batch(n + a.offset, 1, dev) for _ in range(4)]
    ws = ItemWorkspace(dev)
    m = center = None
    if a.mode == "training":
        m = _matrix()
    else:
        center = np.zeros(3)
    times = []
    for rep in range(len(res) + a.reps):
        x, l = res[rep % len(res)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); train_item(x, l, outs[rep % len(outs)], a.offset, 4.0, ws, m=m, center=center); e1.record()
        torch.cuda.synchronize()
        if rep >= len(res):
            times.append(e0.elapsed_time(e1))
    print(f"tl_train_item {a.mode} offset {a.offset}: {n} rows, {len(times)} calls, median {statistics.median(times):.3f} ms, min {min(times):.3f} ms", flush=True)


def _matrix():
    """The scale + flip + rot + jitter matrix the tests draw from RandomState(3)."""
    import types
    from treelearn_amd.util.dataset import ALL_AUGMENTATIONS, CropDataset
    return CropDataset.augmentation_matrix(types.SimpleNamespace(data_augmentations=dict(ALL_AUGMENTATIONS)), np.random.RandomState(3), aug_prob=1.0)


def rank3(a):
    from treelearn_amd.synth import make_plot, plot_squares
    p = make_plot(seed=0)
    pts, lab = p["points"], p["instance_label"]
    _, outer = plot_squares()
    m = _matrix()
    print(f"numpy {np.__version__}; plot {len(pts)} rows, {len(outer)} tiles", flush=True)
    total = {"stored z (test mode)": [0, 0], "RandomState(3) matrix (training mode)": [0, 0]}
    for x0, x1, y0, y1 in outer:
        keep = (pts[:, 0] >= x0) & (pts[:, 0] <= x1) & (pts[:, 1] >= y0) & (pts[:, 1] <= y1)
        xyz, l = pts[keep], lab[keep]
        order = np.argsort(l, kind="stable")
        ls = l[order]
        starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
        ends = np.r_[starts[1:], len(ls)]
        for name, z in (("stored z (test mode)", xyz[:, 2]), ("RandomState(3) matrix (training mode)", np.matmul(xyz, m)[:, 2])):
            zs = z[order]
            for s, e in zip(starts, ends):
                if ls[s] == 0 or e - s <= 11:
                    continue
                zi = zs[s:e]
                total[name][0] += 1
                total[name][1] += int(np.partition(zi, 10)[3] != np.sort(zi)[3])
    for name, (cnt, diff) in total.items():
        print(f"{name}: {diff} of {cnt} instances (over all tiles) where np.partition(z, 10)[3] != np.sort(z)[3]", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("item", "rank3"))
    ap.add_argument("--mode", choices=("training", "test"), default="training")
    ap.add_argument("--offset", type=int, default=0); ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    (item if a.what == "item" else rank3)(a)
