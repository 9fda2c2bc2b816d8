"""Dev: what feeding the training step costs -- BASELINE config 3 (batches of two 40 m crops, bf16).

    python tools/dev_train_input.py [--crops 6] [--extent 40] [--rounds 3] [--workers 2] [--dir DIR]

  1. host path, one worker: CropDataset.__getitem__ per item, collate + pinned copy + H2D per batch (host clock, device synchronised)
  2. device path: tl_train_item alone on a resident crop (device events, median, inputs rotating over the crops), and a whole batch through
     DeviceCropLoader (file read + H2D + kernels; host clock around a synchronised iteration)
  3. steps/s of train_epoch fed by (a) resident batches, (b) build_dataloader with --workers, (c) DeviceCropLoader, in alternating rounds
"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from treelearn_amd.model import TreeLearn
from treelearn_amd.synth import make_tile, random_state_dict
from treelearn_amd.util.dataset import ALL_AUGMENTATIONS, CropDataset, collate
from treelearn_amd.util.device_dataset import DeviceCropLoader, ItemWorkspace, alloc_batch, train_item
from treelearn_amd.util.train import build_cosine_scheduler, build_dataloader, build_optimizer
from treelearn_amd.util.trainer import _grad_scaler, train_epoch

INNER = 8


class _Log:
    def __init__(self): self.seconds = None
    def info(self, msg):
        m = re.search(r"time ([0-9.]+)s", msg)
        if m:
            self.seconds = float(m.group(1))


class _Writer:
    def add_scalar(self, *a): pass
    def flush(self): pass


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=6); ap.add_argument("--extent", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--workers", type=int, default=2); ap.add_argument("--dir")   # (2: configs/training/train.yaml of the reference)
    a = ap.parse_args()
    root = a.dir or tempfile.mkdtemp(prefix="tl_train_input_")
    data = os.path.join(root, "crops"); os.makedirs(data, exist_ok=True)
    for k in range(a.crops):
        p = os.path.join(data, f"synth_{k}.npz")
        if not os.path.exists(p):
            t = make_tile(extent=a.extent, voxel=0.1, n_trees=int(64 * (a.extent / 40) ** 2), fill=0.10, seed=k)
            np.savez(p, points=t["points"], feat=t["feat"], instance_label=t["instance_label"], center=t["center"])
    aug = dict(ALL_AUGMENTATIONS)
    dev = torch.device("cuda")

    # ---- 1. host path, one worker
    ds = CropDataset(data, INNER, True, aug, seed=1)
    t_item, t_batch, items = [], [], []
    for i in range(len(ds)):
        t0 = time.perf_counter(); items.append(ds[i]); t_item.append(time.perf_counter() - t0)
    for i in range(0, len(items) - 1, 2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        b = collate(items[i:i + 2])
        g = {k: (v.pin_memory().to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in b.items()}
        torch.cuda.synchronize(); t_batch.append(time.perf_counter() - t0)
    rows = [len(it[0]) for it in items]
    print(f"host path : rows/item {int(med(rows))}, __getitem__ median {med(t_item) * 1e3:.1f} ms/item ({med(t_item) / med(rows) * 1e9:.1f} ms per 1e6 rows), "
          f"collate + pin + H2D median {med(t_batch) * 1e3:.1f} ms/batch of 2", flush=True)
    resident = []
    for i in range(0, len(items) - 1, 2):
        b = collate(items[i:i + 2])
        resident.append({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()})
    del items, g

    # ---- 2. device path
    files = [np.load(p) for p in ds.data_paths]
    res = [(torch.from_numpy(f["points"]).to(dev), torch.from_numpy(f["instance_label"]).to(dev)) for f in files]
    ws = ItemWorkspace(dev)
    n_max = max(len(x) for x, _ in res)
    outs = [alloc_batch(n_max, 1, dev) for _ in range(4)]       # inputs AND outputs rotate: 63 B/row of outputs x 4 buffers + the inputs of all crops
    rot = 4 * 63 * n_max + sum(16 * len(x) for x, _ in res)      # lie between two uses of the same buffer -- well above the 256 MB Infinity Cache
    print(f"rotation: {rot / 1e6:.0f} MB touched between two uses of the same buffer", flush=True)
    m = ds.augmentation_matrix(np.random.RandomState(3), aug_prob=1.0)
    for mode, mm in (("training", m), ("test", None)):
        times = []
        for rep in range(4 * len(res)):
            x, l = res[rep % len(res)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); train_item(x, l, outs[rep % len(outs)], 0, INNER / 2, ws, m=mm, center=None if mm is not None else np.zeros(3)); e1.record()
            torch.cuda.synchronize()
            if rep >= len(res):
                times.append(e0.elapsed_time(e1))
        print(f"tl_train_item ({mode}): median {med(times):.3f} ms, min {min(times):.3f} ms per item of {len(res[0][0])} rows "
              f"(ws {ws.buf.numel() / 2**20:.0f} MiB)", flush=True)
    del outs
    loader = DeviceCropLoader(data, INNER, True, aug, seed=1, batch_size=2)
    per = []
    for ep in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for b in loader:
            torch.cuda.current_stream().wait_event(b["_ready_event"]); torch.cuda.synchronize()
            t1 = time.perf_counter(); per.append(t1 - t0); t0 = t1
    per = per[len(loader):]
    print(f"device path: DeviceCropLoader median {med(per) * 1e3:.1f} ms/batch of 2 (file read + H2D + kernels, nothing consuming)", flush=True)
    t_read = []
    for p in ds.data_paths:
        t0 = time.perf_counter(); f = np.load(p); _ = f["points"], f["feat"], f["instance_label"]; t_read.append(time.perf_counter() - t0)
    from treelearn_amd.util.device_dataset import _Staging
    st, t_fill = _Staging(), []
    for p in list(ds.data_paths) * 2:
        t0 = time.perf_counter(); st.fill(p); t_fill.append(time.perf_counter() - t0)
    t_fill = t_fill[len(ds.data_paths):]                         # (the first round grows the pinned buffers)
    print(f"reader thread's work per crop: np.load median {med(t_read) * 1e3:.1f} ms, np.load + copy into pinned staging median {med(t_fill) * 1e3:.1f} ms", flush=True)
    del res, st

    # ---- 3. train_epoch, three sources
    model = TreeLearn(use_feats=False, use_coords=False, spatial_shape=[1000, 1000, 1000], voxel_size=0.1, compute_dtype=torch.bfloat16)   # (an augmented 40 m crop spans up to 75 m)
    model.load_state_dict(random_state_dict(7, channels=32, num_blocks=7)); model = model.cuda()
    cfg = dict(fp16=False, dataloader=dict(train=dict(batch_size=2)), grad_norm_clip=True, examples_per_epoch=10 ** 9, epochs=1,
               work_dir=os.path.join(root, "work"), save_frequency=10 ** 9)
    os.makedirs(cfg["work_dir"], exist_ok=True)
    optimizer = build_optimizer(model, dict(type="AdamW", lr=1e-4, weight_decay=1e-3))
    scheduler = build_cosine_scheduler(dict(t_initial=1000, lr_min=5e-5, cycle_decay=1, warmup_lr_init=1e-5, warmup_t=2, cycle_limit=1, t_in_epochs=True), optimizer)
    scaler = _grad_scaler(False)
    sources = {
        "a resident": lambda: resident * 2,
        f"b DataLoader({a.workers} workers)": lambda: build_dataloader(CropDataset(data, INNER, True, aug, seed=1), training=True, batch_size=2, num_workers=a.workers,
                                                                      generator=torch.Generator().manual_seed(1)),
        "c DeviceCropLoader": lambda: DeviceCropLoader(data, INNER, True, aug, seed=1, batch_size=2, generator=torch.Generator().manual_seed(1)),
    }
    log = _Log()
    train_epoch(cfg, 1, model, optimizer, scheduler, scaler, resident, log, _Writer())               # warm-up
    for r in range(a.rounds):
        for name, make in sources.items():
            src = make()
            n = len(src)
            train_epoch(cfg, 1, model, optimizer, scheduler, scaler, src, log, _Writer())
            print(f"round {r} {name}: {n} steps in {log.seconds:.2f} s = {log.seconds / n * 1e3:.1f} ms/step, {n / log.seconds:.2f} steps/s", flush=True)


if __name__ == "__main__":
    main()
