"""Crops as training (or test) batches prepared on the GPU, DESIGN §14: what `CropDataset.__getitem__` + `collate` (util/dataset.py, the
reference's tree_learn/dataset/dataset.py:34-226) build row by row in numpy comes out of one `tl_train_item` call per crop -- semantic
labels, the augmentation matrix, offset labels, the three masks, batch ids and centres, written at the crop's row offset of the batch.

    loader = DeviceCropLoader(data_root, inner_square_edge_length, training, data_augmentations, seed, batch_size, generator)
    for batch in loader:                      # collate's keys and dtypes, device tensors, plus `_ready_event` (as PlotTiler's tiles)
        torch.cuda.current_stream().wait_event(batch["_ready_event"])

Files are read (`np.load`) by a background thread into pinned staging, copied and processed on the loader's own stream; batch k + 1 is
enqueued before batch k is handed out, so it is prepared while the caller trains on batch k.

What differs from `CropDataset`:
  * offset labels follow the device rule (the tree base starts at the 4th smallest z, duplicates counted; numpy's `np.partition(z, 10)[3]`
    is an implementation-defined element among the ten lowest) and an exact sum instead of numpy's float32 one -- include/treelearn_hip.h;
  * the augmentation draws stay on the host, from the same `RandomState(seed)` in the reference's order (the point-jitter coin, then the
    matrix draws: `CropDataset.point_jitter_coin` / `.augmentation_matrix`), so with `point_jitter` off a seeded loader applies the matrices
    `CropDataset(seed)` applies when iterated in the same order in one process.  When the coin says jitter, the stream yields a 64-bit key
    for `tl_point_jitter` (two 32-bit draws) instead of 3 n normals: from the first jittered item on the two streams part, and the jitter
    itself comes from the kernel's counter-based generator, not from numpy;
  * order: file-name order; with `training`, shuffled by `generator` when one is given (file order otherwise) and the last incomplete batch
    dropped, as `build_dataloader` does.
There is no CPU fallback: without a GPU the constructor raises.
"""
import ctypes
import queue
import threading

import numpy as np
import torch

from .. import _hip
from .dataset import CropDataset

_F3 = ctypes.c_float * 3
_D9 = ctypes.c_double * 9


def alloc_batch(n, n_feat, device):
    """Uninitialised batch tensors of `n` rows with collate's keys and dtypes."""
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)                     # noqa: E731
    return dict(coords=e((n, 3), torch.float32), input_feats=e((n, n_feat), torch.float32), batch_ids=e((n,), torch.int64),
                semantic_labels=e((n,), torch.int64), instance_labels=e((n,), torch.int64), masks_inner=e((n,), torch.bool),
                masks_off=e((n,), torch.bool), masks_sem=e((n,), torch.bool), offset_labels=e((n, 3), torch.float32), centers=e((n, 3), torch.float32))


class ItemWorkspace:
    """tl_train_item's workspace, grown on demand and reused."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, n):
        need = int(_hip.lib().tl_train_item_ws_bytes(n))
        if need <= 0:
            raise ValueError(f"tl_train_item: unsupported row count {n}")
        if self.buf is None or self.buf.numel() < need:
            self.buf = None                                                             # (give the old block back before asking for the larger one)
            self.buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.buf


def train_item(xyz, inst, out, row_offset, half_inner, ws, m=None, center=None, batch_id=0):
    """One `tl_train_item` call on torch's current stream: xyz f32[n,3] and inst i32[n] on the device -> rows [row_offset, row_offset + n) of
    the tensors of `out` (alloc_batch).  `m`: the float64 3 x 3 matrix of a training item, None for test mode; `center`: 3 numbers, None
    for the training dummy of ones."""
    n = int(xyz.shape[0])
    _hip.require_cuda(xyz, "xyz"); _hip.require_cuda(inst, "instance_label")
    if xyz.dtype != torch.float32 or inst.dtype != torch.int32 or tuple(xyz.shape) != (n, 3) or tuple(inst.shape) != (n,):
        raise ValueError(f"train_item: xyz {xyz.dtype}{tuple(xyz.shape)}, instance_label {inst.dtype}{tuple(inst.shape)}")
    if row_offset < 0 or row_offset + n > out["coords"].shape[0]:
        raise ValueError(f"train_item: rows {row_offset}..{row_offset + n} do not fit a batch of {out['coords'].shape[0]}")
    mp = None if m is None else _D9(*[float(v) for v in np.asarray(m, np.float64).reshape(9)])
    cp = None if center is None else _F3(*[float(v) for v in np.asarray(center, np.float32).reshape(3)])
    p = _hip.ptr
    _hip.check(_hip.lib().tl_train_item(p(xyz), p(inst), n, mp, float(half_inner), cp, int(batch_id), int(row_offset), p(out["coords"]),
                                        p(out["semantic_labels"]), p(out["instance_labels"]), p(out["offset_labels"]), p(out["masks_inner"]),
                                        p(out["masks_off"]), p(out["masks_sem"]), p(out["batch_ids"]), p(out["centers"]), p(ws.get(n)),
                                        _hip.stream()), "tl_train_item")


def point_jitter(xyz, key):
    """`tl_point_jitter` in place on xyz f32[n,3] (device), on torch's current stream."""
    _hip.require_cuda(xyz, "xyz")
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"point_jitter: xyz {xyz.dtype}{tuple(xyz.shape)}")
    _hip.check(_hip.lib().tl_point_jitter(_hip.ptr(xyz), int(xyz.shape[0]), int(key) & 0xFFFFFFFFFFFFFFFF, _hip.stream()), "tl_point_jitter")


class _Staging:
    """One crop in pinned host memory (grown on demand), and the event after which it may be overwritten."""

    def __init__(self):
        self.xyz = self.feat = self.inst = None
        self.n = self.n_feat = 0
        self.center = None
        self.free = None

    def fill(self, path):
        if self.free is not None:
            self.free.synchronize()                                                     # the copies out of this slot have finished
            self.free = None
        data = np.load(path)
        xyz, feat, inst = data["points"], data["feat"], data["instance_label"]
        n = len(xyz)
        feat = feat.reshape(n, -1)
        if self.xyz is None or self.xyz.shape[0] < n or self.feat.shape[1] != feat.shape[1]:
            cap = max(n, int(1.25 * self.n))
            self.xyz = torch.empty((cap, 3), dtype=torch.float32).pin_memory()
            self.feat = torch.empty((cap, feat.shape[1]), dtype=torch.float32).pin_memory()
            self.inst = torch.empty(cap, dtype=torch.int32).pin_memory()
        self.xyz[:n].numpy()[...] = xyz
        self.feat[:n].numpy()[...] = feat
        self.inst[:n].numpy()[...] = inst
        self.n, self.n_feat = n, feat.shape[1]
        self.center = np.asarray(data["center"], np.float64).reshape(3) if "center" in data.files else np.zeros(3)
        return self


class DeviceCropLoader:
    def __init__(self, data_root, inner_square_edge_length, training, data_augmentations=None, seed=0, batch_size=1, generator=None, prefetch=2):
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceCropLoader needs the HIP library and a GPU; the HIP path has no CPU fallback")
        _hip.lib()
        self.dataset = CropDataset(data_root, inner_square_edge_length, training, data_augmentations, seed=seed)    # the file list and the draws
        self.training = bool(training)
        self.half_inner = inner_square_edge_length / 2
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.generator = generator
        self.prefetch = max(1, int(prefetch))
        self.device = torch.device("cuda", torch.cuda.current_device())
        self._stream = torch.cuda.Stream(device=self.device)
        self._ws = ItemWorkspace(self.device)
        self._xyz = self._inst = None                                                   # device staging of one item
        self._slots = [_Staging() for _ in range(self.batch_size * (self.prefetch + 2))]

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.training else -(-n // self.batch_size)

    def _batches(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if (self.training and self.generator is not None) else list(range(n))
        bs = self.batch_size
        out = [order[i:i + bs] for i in range(0, n, bs)]
        if self.training and out and len(out[-1]) < bs:
            out.pop()
        return out

    def _reader(self, batches, free, ready, stop):
        try:
            for idx in batches:
                items = []
                for i in idx:
                    slot = None
                    while slot is None:
                        if stop.is_set():
                            return
                        try:
                            slot = free.get(timeout=0.1)
                        except queue.Empty:
                            pass
                    items.append(slot.fill(self.dataset.data_paths[i]))
                ready.put(items)
            ready.put(None)
        except BaseException as e:                                                      # noqa: BLE001  (handed to the consumer, which raises it)
            ready.put(e)

    def _prepare(self, items, main):
        """Enqueue one batch on the loader's stream; returns the batch dict."""
        ds, rs = self.dataset, self.dataset.rs
        total = sum(s.n for s in items)
        n_max = max(s.n for s in items)
        with torch.cuda.stream(self._stream):
            if self._xyz is None or self._xyz.shape[0] < n_max:
                self._xyz = self._inst = None
                self._xyz = torch.empty((n_max, 3), dtype=torch.float32, device=self.device)
                self._inst = torch.empty(n_max, dtype=torch.int32, device=self.device)
            out = alloc_batch(total, items[0].n_feat, self.device)
            row = 0
            for b, s in enumerate(items):
                n = s.n
                xyz, inst = self._xyz[:n], self._inst[:n]
                xyz.copy_(s.xyz[:n], non_blocking=True)
                inst.copy_(s.inst[:n], non_blocking=True)
                out["input_feats"][row:row + n].copy_(s.feat[:n], non_blocking=True)
                m = center = None
                if self.training:
                    if ds.point_jitter_coin(rs):
                        hi, lo = (int(v) for v in rs.randint(0, 1 << 32, 2, dtype=np.uint64))
                        point_jitter(xyz, (hi << 32) | lo)
                    m = ds.augmentation_matrix(rs)
                else:
                    center = s.center
                train_item(xyz, inst, out, row, self.half_inner, self._ws, m=m, center=center, batch_id=b)
                s.free = torch.cuda.Event(); s.free.record(self._stream)
                row += n
            ready = torch.cuda.Event(); ready.record(self._stream)
        for v in out.values():
            v.record_stream(main)                                                       # allocated on the loader's stream, consumed on the caller's
        out["batch_size"] = len(items)
        out["_ready_event"] = ready
        return out

    def __iter__(self):
        batches = self._batches()
        if not batches:
            return
        main = torch.cuda.current_stream()
        free, ready, stop = queue.Queue(), queue.Queue(maxsize=self.prefetch), threading.Event()
        for s in self._slots:
            free.put(s)
        th = threading.Thread(target=self._reader, args=(batches, free, ready, stop), daemon=True)
        th.start()
        try:
            ahead = None
            while True:
                items = ready.get()
                if isinstance(items, BaseException):
                    raise items
                if items is None:
                    break
                nxt = self._prepare(items, main)
                for s in items:
                    free.put(s)                                                         # (the reader waits for s.free before it overwrites the slot)
                if ahead is not None:
                    yield ahead
                ahead = nxt
            if ahead is not None:
                yield ahead
        finally:
            stop.set()
            while th.is_alive():                                                        # a reader blocked on a full queue: drain it
                try:
                    ready.get(timeout=0.05)
                except queue.Empty:
                    pass
            th.join()
