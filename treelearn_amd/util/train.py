"""Host utilities the model path and the training program need, mirroring reference tree_learn/util/train.py:
`cuda_cast` (:28-43), `point_wise_loss` (:145-166), `load_checkpoint` key handling (:65-102), and for util/trainer.py `is_multiple` (:10-11),
`weights_to_cpu` (:14-25), `checkpoint_save` (:46-62), `build_optimizer` (:105-110), `build_cosine_scheduler` (:113-122, without timm),
`build_dataloader` (:125-141)."""
import functools
import math
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F


def cuda_cast(func):
    """Move every tensor argument to the current GPU (non_blocking: pinned batches overlap the copy)."""
    @functools.wraps(func)
    def wrapper(*args, **kwargs):
        mv = lambda x: x.cuda(non_blocking=True) if isinstance(x, torch.Tensor) and not x.is_cuda else x
        return func(*[mv(a) for a in args], **{k: mv(v) for k, v in kwargs.items()})
    return wrapper


@cuda_cast
def point_wise_loss(semantic_prediction_logits, offset_predictions, masks_sem, masks_off, semantic_labels, offset_labels, weights=None, mask_rows=None):
    return point_wise_loss_impl(semantic_prediction_logits, offset_predictions, masks_sem, masks_off, semantic_labels, offset_labels, weights, mask_rows)


def loss_mask_rows(masks_sem, masks_off):
    """Row indices of the two loss masks.  They depend on the batch only, so `TreeLearn.forward` takes them BEFORE the network is enqueued: the
    boolean indexing and the `mask.sum() == 0` tests of the reference's loss (util/train.py:147,153,159,163) each read a count back from the
    device, i.e. wait for the whole forward and then drain the queue four to six times; taken up front the reads find an idle device (or,
    for host-resident masks, no device at all) and the loss itself enqueues without a wait."""
    rows = []
    for m in (masks_sem, masks_off):
        idx = m.nonzero(as_tuple=False).view(-1)
        rows.append(idx if idx.is_cuda or not torch.cuda.is_available() else idx.cuda(non_blocking=True))
    return tuple(rows)


def point_wise_loss_impl(logits, offsets, masks_sem, masks_off, semantic_labels, offset_labels, weights=None, mask_rows=None):
    """Masked CE (sum / count) and masked mean L2 offset error; an empty mask yields `0 * sum`
    so the graph stays connected (train.py:147-148,159-160).  `mask_rows` = loss_mask_rows(masks_sem, masks_off): the masks as row lists
    (`x[mask]` == `x.index_select(0, rows)`, same order, same values) -- no read-back between the forward and the loss."""
    if mask_rows is None:
        mask_rows = loss_mask_rows(masks_sem, masks_off)
    sem_rows, off_rows = (r.to(logits.device) for r in mask_rows)
    n_sem = sem_rows.numel()
    if n_sem == 0:
        semantic_loss = 0 * logits.sum()
    else:
        ce = F.cross_entropy(logits.index_select(0, sem_rows), semantic_labels.index_select(0, sem_rows), reduction='sum' if weights is None else 'none')
        semantic_loss = (ce if weights is None else (ce * weights).sum()) / n_sem
    if off_rows.numel() == 0:
        offset_loss = 0 * offsets.sum()
    else:
        offset_loss = (offsets.index_select(0, off_rows) - offset_labels.index_select(0, off_rows)).pow(2).sum(1).sqrt().mean()
    return semantic_loss, offset_loss


def load_checkpoint(checkpoint, logger, model, optimizer=None, strict=False):
    """Load a reference `.pth` ({'net','optimizer','epoch'}): size-mismatched keys are dropped,
    `strict=False`, returns epoch + 1 (train.py:65-102)."""
    if hasattr(model, 'module'):
        model = model.module
    state = torch.load(checkpoint, map_location='cpu')
    src = state['net']
    tgt = model.state_dict()
    skipped = [k for k in src if k in tgt and src[k].size() != tgt[k].size()]
    for k in skipped:
        del src[k]
    missing, unexpected = model.load_state_dict(src, strict=strict)
    if logger is not None:
        if skipped:
            logger.info(f'removed keys in source state_dict due to size mismatch: {", ".join(skipped)}')
        if missing:
            logger.info(f'missing keys in source state_dict: {", ".join(missing)}')
        if unexpected:
            logger.info(f'unexpected key in source state_dict: {", ".join(unexpected)}')
    if optimizer is not None:
        assert 'optimizer' in state
        optimizer.load_state_dict(state['optimizer'])
    return state.get('epoch', 0) + 1


def is_multiple(num, multiple):
    return num != 0 and num % multiple == 0


def weights_to_cpu(state_dict):
    """A copy of a state dict with every tensor on the host."""
    return OrderedDict((k, v.cpu()) for k, v in state_dict.items())


def checkpoint_save(epoch, model, optimizer, work_dir, save_freq=1):
    """work_dir/epoch_<epoch>.pth = {'net', 'optimizer', 'epoch'}; the previous epoch's file is removed unless that epoch is a multiple of
    save_freq (train.py:46-62)."""
    if hasattr(model, 'module'):
        model = model.module
    torch.save({'net': weights_to_cpu(model.state_dict()), 'optimizer': optimizer.state_dict(), 'epoch': epoch},
               os.path.join(work_dir, f'epoch_{epoch}.pth'))
    previous = os.path.join(work_dir, f'epoch_{epoch - 1}.pth')
    if os.path.isfile(previous) and not is_multiple(epoch - 1, save_freq):
        os.remove(previous)


def build_optimizer(model, optim_cfg):
    """`type` names a class of torch.optim, the other keys are its arguments; parameters that do not require a gradient are left out."""
    assert 'type' in optim_cfg
    cfg = dict(optim_cfg)
    optim = getattr(torch.optim, cfg.pop('type'))
    return optim(filter(lambda p: p.requires_grad, model.parameters()), **cfg)


class CosineSchedule:
    """timm 0.6.12's CosineLRScheduler for the arguments the reference passes (cycle_mul = 1, no warmup prefix, no noise): linear warmup
    from warmup_lr_init over warmup_t steps, then cosine cycles of t_initial steps from base * cycle_decay**i down to lr_min, lr_min once
    cycle_limit cycles are done.  `step(t)` sets every group's lr for epoch (t_in_epochs) or update t; `step_update(t)` does so when the
    schedule counts updates."""

    def __init__(self, optimizer, t_initial, lr_min=0.0, cycle_decay=1.0, warmup_lr_init=0.0, warmup_t=0, cycle_limit=1, t_in_epochs=True):
        assert t_initial > 0 and lr_min >= 0
        self.optimizer = optimizer
        self.t_initial, self.lr_min, self.cycle_decay = t_initial, lr_min, cycle_decay
        self.warmup_lr_init, self.warmup_t, self.cycle_limit, self.t_in_epochs = warmup_lr_init, warmup_t, cycle_limit, t_in_epochs
        for group in optimizer.param_groups:
            group.setdefault('initial_lr', group['lr'])
        self.base_values = [group['initial_lr'] for group in optimizer.param_groups]
        if self.warmup_t:
            self.warmup_steps = [(v - warmup_lr_init) / self.warmup_t for v in self.base_values]
            self._set([self.warmup_lr_init for _ in self.base_values])
        else:
            self.warmup_steps = [1 for _ in self.base_values]

    def _set(self, values):
        for group, v in zip(self.optimizer.param_groups, values):
            group['lr'] = v

    def get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        i = t // self.t_initial
        if i >= self.cycle_limit:
            return [self.lr_min for _ in self.base_values]
        t_curr = t - self.t_initial * i
        gamma = self.cycle_decay ** i
        return [self.lr_min + 0.5 * (v * gamma - self.lr_min) * (1 + math.cos(math.pi * t_curr / self.t_initial)) for v in self.base_values]

    def step(self, epoch):
        if self.t_in_epochs:
            self._set(self.get_lr(epoch))

    def step_update(self, num_updates):
        if not self.t_in_epochs:
            self._set(self.get_lr(num_updates))


def _cfg(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def build_cosine_scheduler(cfg, optimizer):
    return CosineSchedule(optimizer, **{k: _cfg(cfg, k) for k in ('t_initial', 'lr_min', 'cycle_decay', 'warmup_lr_init', 'warmup_t', 'cycle_limit',
                                                                 't_in_epochs')})


def build_dataloader(dataset, batch_size=1, num_workers=1, training=True, dist=False, generator=None):
    """train.py:125-141: shuffled and drop_last for training, pinned host batches.  `generator` seeds the shuffle (and the workers)."""
    from torch.utils.data import DataLoader
    if dist:
        raise NotImplementedError("distributed training is not offered")
    return DataLoader(dataset, batch_size=batch_size, num_workers=num_workers, collate_fn=dataset.collate_fn, shuffle=training,
                      drop_last=training, pin_memory=torch.cuda.is_available(), generator=generator)
