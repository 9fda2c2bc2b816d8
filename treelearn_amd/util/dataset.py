"""Crops as training (or test) batches: the reference's `TreeDataset.__getitem__` and `collate_fn`
(tree_learn/dataset/dataset.py:34-226) over the files `util/crops.generate_random_crops` writes, DESIGN §12.

It runs on the host, as the reference's DataLoader workers do, and is a plain `torch.utils.data.Dataset`, so
`DataLoader(dataset, collate_fn=collate, num_workers=...)` works.  Differences from the reference:
  * files are taken in name order (the reference uses os.listdir order, which the file system decides);
  * augmentations draw from the dataset's own `np.random.RandomState(seed)` -- with the reference's methods, arguments
    and order, so the items equal the reference's after `np.random.seed(seed)` -- instead of numpy's global state.  In a
    DataLoader worker the stream is re-seeded from (seed, worker id, torch's seed of that worker), once per worker process:
    workers do not repeat each other, and non-persistent workers (a new process per epoch, with a new torch seed) draw new
    augmentations every epoch.  A DataLoader given a seeded `generator` makes the whole run reproducible.
"""
import math
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .tiles import _offset_labels_host

INSTANCE_LABEL_IGNORE_IN_RAW_DATA = -1                 # dataset.py:7-10
NON_TREE_CLASS_IN_RAW_DATA = 0
NON_TREE_CLASS_IN_PYTORCH_DATASET = 1
TREE_CLASS_IN_PYTORCH_DATASET = 0
ALL_AUGMENTATIONS = dict(jitter=True, flip=True, rot=True, scaled=True, point_jitter=True)      # configs/_modular/dataset_train.yaml


class CropDataset(Dataset):
    def __init__(self, data_root, inner_square_edge_length, training, data_augmentations=None, seed=0):
        self.data_paths = [os.path.join(data_root, p) for p in sorted(os.listdir(data_root))]
        self.inner_square_edge_length = inner_square_edge_length
        self.training = training
        self.data_augmentations = data_augmentations
        if training and data_augmentations is None:
            raise ValueError("training=True needs data_augmentations (the reference indexes them unconditionally)")
        self.seed = seed
        self.rs = np.random.RandomState(seed)
        self._worker = None

    def __len__(self):
        return len(self.data_paths)

    def _stream(self):
        info = torch.utils.data.get_worker_info()
        if info is not None and self._worker != (info.id, info.seed):
            self.rs = np.random.RandomState(np.random.SeedSequence([self.seed, info.id, info.seed]).generate_state(4))
            self._worker = (info.id, info.seed)
        return self.rs

    def __getitem__(self, index):
        rs = self._stream()
        data = np.load(self.data_paths[index])
        xyz = data["points"]
        input_feat = data["feat"]
        instance_label = data["instance_label"]
        semantic_label = np.empty(len(instance_label))
        semantic_label[instance_label == NON_TREE_CLASS_IN_RAW_DATA] = NON_TREE_CLASS_IN_PYTORCH_DATASET
        semantic_label[instance_label != NON_TREE_CLASS_IN_RAW_DATA] = TREE_CLASS_IN_PYTORCH_DATASET
        center = np.ones_like(xyz) if self.training else np.ones_like(xyz) * data["center"]
        xyz = self.transform_train(xyz, rs) if self.training else xyz
        pt_offset_label, mask_valid_offset = _offset_labels_host(xyz, instance_label, semantic_label)
        inf_norm = np.linalg.norm(xyz[:, :-1], ord=np.inf, axis=1)
        mask_inner = inf_norm <= (self.inner_square_edge_length / 2)
        mask_not_ignore = np.logical_not(instance_label == INSTANCE_LABEL_IGNORE_IN_RAW_DATA)
        mask_off = mask_inner & mask_not_ignore & (semantic_label != NON_TREE_CLASS_IN_PYTORCH_DATASET) & mask_valid_offset
        mask_sem = mask_inner & mask_not_ignore
        T = torch.from_numpy
        return (T(xyz), T(input_feat), T(instance_label), T(semantic_label), T(pt_offset_label), T(center), T(mask_inner), T(mask_off),
                T(mask_sem))

    def transform_train(self, xyz, rs, aug_prob=0.5, aug_prob_point_jitter=0.25):
        """dataset.py:92-103,143-164: point jitter in place on the float32 array, then one float64 matrix."""
        if self.point_jitter_coin(rs, aug_prob_point_jitter):
            xyz += np.clip(0.1 * rs.randn(xyz.shape[0], 3), -1 * 0.2, 0.2)
        return np.matmul(xyz, self.augmentation_matrix(rs, aug_prob))

    def point_jitter_coin(self, rs, aug_prob_point_jitter=0.25):
        """dataset.py:92-93: whether this item is jittered (one draw, only when the augmentation is on)."""
        return self.data_augmentations["point_jitter"] == True and rs.random() <= aug_prob_point_jitter      # noqa: E712  (the reference's test)

    def augmentation_matrix(self, rs, aug_prob=0.5):
        """dataset.py:143-164: the float64 3 x 3 matrix of one item, drawn in the reference's order.  Shared with the device path
        (util/device_dataset.DeviceCropLoader), which hands it to tl_train_item instead of multiplying on the host."""
        aug = self.data_augmentations
        m = np.eye(3)
        if aug["scaled"] and rs.rand() < aug_prob:
            scale_xy = rs.uniform(0.8, 1.2, 2)
            scale_z = rs.uniform(0.95, 1.05, 1)
            m = m * np.concatenate([scale_xy, scale_z])
        if aug["jitter"] and rs.rand() < aug_prob:
            m += rs.randn(3, 3) * 0.1
        if aug["flip"] and rs.rand() < aug_prob:
            m[0][0] *= rs.randint(0, 2) * 2 - 1
        if aug["rot"] and rs.rand() < aug_prob:
            theta = rs.rand() * 2 * math.pi
            m = np.matmul(m, [[math.cos(theta), math.sin(theta), 0], [-math.sin(theta), math.cos(theta), 0], [0, 0, 1]])
        return m

    def collate_fn(self, batch):
        return collate(batch)


def collate(batch):
    """dataset.py:167-226: the batch dict TreeLearn.forward takes."""
    assert len(batch) > 0, "empty batch"
    cols = list(zip(*batch))
    xyz, feat, inst, sem, off, center, m_inner, m_off, m_sem = cols
    batch_ids = [torch.ones(len(x)) * b for b, x in enumerate(xyz)]
    return {
        "coords": torch.cat(xyz, 0).to(torch.float32),
        "input_feats": torch.cat(feat, 0).to(torch.float32),
        "batch_ids": torch.cat(batch_ids, 0).long(),
        "semantic_labels": torch.cat(sem, 0).long(),
        "instance_labels": torch.cat(inst, 0).long(),
        "masks_inner": torch.cat(m_inner, 0).bool(),
        "masks_off": torch.cat(m_off, 0).bool(),
        "masks_sem": torch.cat(m_sem, 0).bool(),
        "offset_labels": torch.cat(off, 0).float(),
        "batch_size": len(batch),
        "centers": torch.cat(center, 0).float(),
    }
