"""Train a model: the reference's tools/training/train.py on this package, DESIGN §13.

    python -m treelearn_amd.util.trainer --config train.yaml [--resume work_dirs/x/epoch_40.pth] [--work_dir name]

  train_epoch    <- train (train.py:19-58): the loss terms are summed on the device and read back once per epoch
  validate       <- validate (:61-86): one tl_pointwise_eval call per tile adds to a 64-byte device state, nothing per point is kept
  pointwise_eval <- pointwise_eval (:89-102) for already-gathered tensors, on the same kernel
  fit            <- main (:110-142)
  ScalarLog      stands where the tensorboard SummaryWriter does: JSON lines in <work_dir>/scalars.jsonl

The config keys are the reference's (configs/training/train.yaml over configs/_modular/{model,dataset_train,dataset_test}.yaml) plus an
optional `seed` and an optional `device_batches` (default false: true builds the batches on the GPU, util/device_dataset.py).  Crops come from util/crops.py, validation tiles from util/tiles.write_tiles; checkpoints are the reference's
{'net', 'optimizer', 'epoch'} files.  Not offered: distributed training (--dist).
"""
import argparse
import json
import logging
import math
import os
import os.path as osp
import sys
import time

import torch

from .. import _hip
from .train import build_cosine_scheduler, build_dataloader, build_optimizer, checkpoint_save, is_multiple, load_checkpoint

TREE_CLASS_IN_DATASET = 0          # train.py:14-16
NON_TREE_CLASS_IN_DATASET = 1
TREE_CONF_THRESHOLD = 0.5          # the kernel's decision threshold (csrc/tl_train_eval.hip)


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class ScalarLog:
    """`add_scalar(tag, value, step)` / `flush()` as a tensorboard writer has them; one JSON object per line, appended to
    <work_dir>/scalars.jsonl (a resumed run continues the file)."""

    def __init__(self, work_dir, name="scalars.jsonl"):
        os.makedirs(work_dir, exist_ok=True)
        self.path = osp.join(work_dir, name)
        self._f = open(self.path, "a")

    def add_scalar(self, tag, value, step):
        self._f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")

    def flush(self):
        self._f.flush()

    def close(self):
        self._f.close()

    @staticmethod
    def read(path):
        with open(path) as f:
            return [json.loads(line) for line in f if line.strip()]


class EvalState:
    """The running validation metrics on the device: tl_pointwise_eval's 64-byte state and its workspace.  `add` per tile, `read` once."""

    def __init__(self, device="cuda"):
        self.state = torch.zeros(8, dtype=torch.int64, device=device)
        self.ws = None

    def add(self, logits, offsets, semantic_labels, offset_labels, mask=None):
        dev = self.state.device
        mv = lambda t: t if t.is_cuda else t.to(dev, non_blocking=True)                      # noqa: E731
        logits, offsets = mv(logits), mv(offsets)
        if logits.dtype != offsets.dtype or logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            logits, offsets = logits.float(), offsets.float()
        logits, offsets = logits.contiguous(), offsets.contiguous()
        sem = mv(semantic_labels).long().contiguous()
        lab = mv(offset_labels).float().contiguous()
        n = logits.shape[0]
        if tuple(logits.shape) != (n, 2) or tuple(offsets.shape) != (n, 3) or tuple(sem.shape) != (n,) or tuple(lab.shape) != (n, 3):
            raise ValueError(f"pointwise_eval: shapes {tuple(logits.shape)}, {tuple(offsets.shape)}, {tuple(sem.shape)}, {tuple(lab.shape)}")
        m = None
        if mask is not None:
            m = mv(mask)
            if tuple(m.shape) != (n,):
                raise ValueError(f"pointwise_eval: mask shape {tuple(m.shape)} for {n} rows")
            m = (m if m.dtype in (torch.bool, torch.uint8) else m != 0).contiguous().view(torch.uint8)
        if n == 0:                                             # nothing to add (an empty tensor has no address to hand over)
            return
        L = _hip.lib()
        need = int(L.tl_pointwise_eval_ws_bytes(n))
        if self.ws is None or self.ws.numel() * 8 < need:
            self.ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        _hip.check(L.tl_pointwise_eval(_hip.ptr(logits), _hip.ptr(offsets), _hip.dtype_code(logits.dtype), _hip.ptr(sem), _hip.ptr(lab),
                                       _hip.ptr(m), n, _hip.ptr(self.state), _hip.ptr(self.ws), _hip.stream()), "tl_pointwise_eval")

    def read(self):
        """The one read-back: dict(tp, fp, tn, fn, n_off as int, sum_off as float)."""
        host = self.state.cpu()
        out = {k: int(host[i]) for i, k in enumerate(("tp", "fp", "tn", "fn", "n_off"))}
        out["sum_off"] = float(host[5:6].view(torch.float64)[0])
        return out


def _report(st, config, epoch, writer, logger):
    """train.py:102-107 from the counts: acc is NaN without a counted row (written as 0), Offset_MAE is 0 without a tree row
    (the reference's `0 * sum`)."""
    total = st["tp"] + st["fp"] + st["fn"] + st["tn"]
    acc = (st["tp"] + st["tn"]) / total if total else float("nan")
    offset_loss = st["sum_off"] / st["n_off"] if st["n_off"] else 0.0
    if logger is not None:
        logger.info(f"[VALIDATION] [{epoch}/{_get(config, 'epochs')}] val/semantic_acc {acc * 100:.2f}, val/offset_loss {offset_loss:.3f}")
    if writer is not None:
        writer.add_scalar("val/acc", acc if not math.isnan(acc) else 0, epoch)
        writer.add_scalar("val/Offset_MAE", offset_loss, epoch)
    return dict(st, acc=acc, offset_mae=offset_loss)


def pointwise_eval(semantic_prediction_logits, offset_predictions, semantic_labels, offset_labels, config, epoch, writer, logger):
    """The reference's argument list; every row counts.  Returns dict(acc, offset_mae, tp, fp, tn, fn, n_off, sum_off)."""
    state = EvalState()
    state.add(semantic_prediction_logits, offset_predictions, semantic_labels, offset_labels)
    return _report(state.read(), config, epoch, writer, logger)


def validate(config, epoch, model, val_source, logger, writer):
    """`val_source`: a DataLoader over tile files (CropDataset(training=False)) or any iterable of batch dicts, host or device
    (PlotTiler.tiles(...)).  Rows with `masks_sem` count, as in train.py:72-77."""
    state = EvalState()
    with torch.no_grad():
        model.eval()
        for batch in val_source:
            if batch.get("_ready_event") is not None:          # device-resident tile produced on another stream (PlotTiler)
                torch.cuda.current_stream().wait_event(batch["_ready_event"])
            output = model(batch, return_loss=False)
            state.add(output["semantic_prediction_logits"], output["offset_predictions"], batch["semantic_labels"], batch["offset_labels"],
                      batch["masks_sem"])
    return _report(state.read(), config, epoch, writer, logger)


def train_epoch(config, epoch, model, optimizer, scheduler, scaler, train_loader, logger, writer):
    model.train()
    start = time.time()
    fp16 = bool(_get(config, "fp16"))
    batch_size = _get(_get(_get(config, "dataloader"), "train"), "batch_size")
    clip = _get(config, "grad_norm_clip")
    sums, steps = {}, 0
    for i, batch in enumerate(train_loader, start=1):
        if _get(config, "examples_per_epoch") < (i * batch_size):          # a fixed number of samples per epoch
            break
        if batch.get("_ready_event") is not None:                          # device-resident batch produced on another stream (DeviceCropLoader)
            torch.cuda.current_stream().wait_event(batch["_ready_event"])
        scheduler.step(epoch)
        optimizer.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
            loss, loss_dict = model(batch, return_loss=True)
        for key, value in loss_dict.items():                                # summed where they are: no read-back in the step
            v = value.detach().float()
            sums[key] = sums[key] + v if key in sums else v
        steps += 1
        scaler.scale(loss).backward()
        if clip:
            torch.nn.utils.clip_grad_norm_(model.parameters(), float(clip), norm_type=2)       # `True` acts as 1.0
        scaler.step(optimizer)
        scaler.update()

    average = {}
    if steps:
        host = (torch.stack([sums[k] for k in sums]) / steps).cpu()        # the epoch's one read-back (it also ends the timing)
        average = {k: float(host[j]) for j, k in enumerate(sums)}
    epoch_time = time.time() - start
    lr = optimizer.param_groups[0]["lr"]
    writer.add_scalar("train/learning_rate", lr, epoch)
    for k, v in average.items():
        writer.add_scalar(f"train/{k}", v, epoch)
    if fp16:
        writer.add_scalar("train/grad_scale", scaler.get_scale(), epoch)
    log_str = f"[TRAINING] [{epoch}/{_get(config, 'epochs')}], time {epoch_time:.2f}s"
    for k, v in average.items():
        log_str += f", {k}: {v:.2f}"
    logger.info(log_str)
    checkpoint_save(epoch, model, optimizer, _get(config, "work_dir"), _get(config, "save_frequency"))
    return average


def _grad_scaler(enabled):
    if hasattr(torch, "amp") and hasattr(torch.amp, "GradScaler"):
        return torch.amp.GradScaler("cuda", enabled=enabled)
    return torch.cuda.amp.GradScaler(enabled=enabled)


def fit(config, resume=None, logger=None, writer=None):
    """Build everything from `config` (attribute or dict access; `config.work_dir` is where checkpoints and scalars go), optionally
    resume (model, optimizer, epoch) or load `config.pretrain` (model only), run the epochs.  Returns the model."""
    from ..model import TreeLearn
    from .config import to_dict
    from .dataset import CropDataset
    work_dir = _get(config, "work_dir")
    os.makedirs(work_dir, exist_ok=True)
    logger = logger or logging.getLogger("treelearn_amd.trainer")
    own_writer = writer is None
    writer = writer or ScalarLog(work_dir)
    seed = _get(config, "seed")
    generator = None
    if seed is not None:
        torch.manual_seed(int(seed))
        generator = torch.Generator().manual_seed(int(seed))

    model = TreeLearn(**to_dict(_get(config, "model"))).cuda()
    optimizer = build_optimizer(model, _get(config, "optimizer"))
    scheduler = build_cosine_scheduler(_get(config, "scheduler"), optimizer)
    scaler = _grad_scaler(bool(_get(config, "fp16")))
    ds_seed = {} if seed is None else dict(seed=int(seed))
    loaders = _get(config, "dataloader")
    if _get(config, "device_batches", False):              # batches prepared on the GPU (util/device_dataset.py); num_workers does not apply
        from .device_dataset import DeviceCropLoader
        shuffle = generator if generator is not None else torch.Generator().manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        train_loader = DeviceCropLoader(**dict(ds_seed, **to_dict(_get(config, "dataset_train"))), generator=shuffle,
                                        batch_size=_get(_get(loaders, "train"), "batch_size", 1))
        val_loader = DeviceCropLoader(**dict(ds_seed, **to_dict(_get(config, "dataset_test"))), batch_size=_get(_get(loaders, "test"), "batch_size", 1))
    else:
        train_set = CropDataset(**dict(ds_seed, **to_dict(_get(config, "dataset_train"))))
        val_set = CropDataset(**dict(ds_seed, **to_dict(_get(config, "dataset_test"))))
        train_loader = build_dataloader(train_set, training=True, generator=generator, **to_dict(_get(loaders, "train")))
        val_loader = build_dataloader(val_set, training=False, **to_dict(_get(loaders, "test")))

    start_epoch = 1
    if resume:
        logger.info(f"Resume from {resume}")
        start_epoch = load_checkpoint(resume, logger, model, optimizer=optimizer)
    elif _get(config, "pretrain"):
        logger.info(f"Load pretrain from {_get(config, 'pretrain')}")
        load_checkpoint(_get(config, "pretrain"), logger, model)

    logger.info("Training")
    try:
        for epoch in range(start_epoch, _get(config, "epochs") + 1):
            train_epoch(config, epoch, model, optimizer, scheduler, scaler, train_loader, logger, writer)
            if is_multiple(epoch, _get(config, "validation_frequency")):
                optimizer.zero_grad()
                logger.info("Validation")
                torch.cuda.empty_cache()
                validate(config, epoch, model, val_loader, logger, writer)
            writer.flush()
    finally:
        if own_writer:
            writer.close()
    return model


# ------------------------------------------------------------------------------------------------ command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.trainer", description="train a TreeLearn model")
    ap.add_argument("--config", type=str, required=True, help="path to config file")
    ap.add_argument("--resume", type=str, help="checkpoint to resume from (model, optimizer, epoch)")
    ap.add_argument("--work_dir", type=str, help="name under ./work_dirs (default: the config file's name)")
    return ap.parse_args(argv)


def work_dir_of(args):
    """util/parser.py:48-51."""
    return osp.join("./work_dirs", args.work_dir if args.work_dir is not None else osp.splitext(osp.basename(args.config))[0])


def main(argv=None):
    import yaml
    from .config import get_config, to_dict
    args = parse_args(argv)
    config = get_config(args.config)
    config.work_dir = work_dir_of(args)
    os.makedirs(config.work_dir, exist_ok=True)
    stamp = time.strftime("%Y%m%d_%H%M%S")
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s",
                        handlers=[logging.StreamHandler(), logging.FileHandler(osp.join(config.work_dir, f"{stamp}.log"))])
    with open(osp.join(config.work_dir, osp.basename(args.config)), "w") as f:
        yaml.safe_dump(to_dict(config), f)
    fit(config, resume=args.resume)
    return 0


if __name__ == "__main__":
    sys.exit(main())
