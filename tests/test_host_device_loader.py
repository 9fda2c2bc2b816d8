"""CPU tests of the device batch path's host side: the factored augmentation draws against golden G15, the loader's refusal
to run without a GPU, and the new entry points' declarations."""
import json
import os
import re

import numpy as np
import pytest
import torch

from treelearn_amd.util.dataset import CropDataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("xyz", "input_feat", "instance_label", "semantic_label", "pt_offset_label", "center", "mask_inner", "mask_off", "mask_sem")


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_crops.npz"))


def _write_full(g, d):
    names = sorted({str(k).split("/")[1] for k in g.files if str(k).startswith("full/")})
    for n in names:
        np.savez(os.path.join(d, n + ".npz"), **{k: g[f"full/{n}/{k}"] for k in g[f"keys/{n}"]})
    return names


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_factored_draws_consume_the_stream_as_transform_train_did(g15, tmp_path):
    """The coin and the matrix, drawn through the two factored methods and applied by hand, give golden G15's items bit for bit (the items
    of the reference's TreeDataset(training=True)): same draws, same order, same arithmetic -- and the stream ends where __getitem__'s does."""
    names = _write_full(g15, str(tmp_path))
    aug, inner, seed = json.loads(str(g15["ds/aug"])), int(g15["ds/inner"]), int(g15["ds/seed"])
    whole = CropDataset(str(tmp_path), inner, True, aug, seed=seed)
    parts = CropDataset(str(tmp_path), inner, True, aug, seed=seed)
    jittered = 0
    for i, n in enumerate(names):
        item = whole[i]
        for k, v in zip(FIELDS, item):
            assert _same(v.numpy(), g15[f"item/{i}/{k}"]), (i, k)
        xyz = np.load(os.path.join(str(tmp_path), n + ".npz"))["points"]
        if parts.point_jitter_coin(parts.rs):
            xyz += np.clip(0.1 * parts.rs.randn(xyz.shape[0], 3), -1 * 0.2, 0.2)
            jittered += 1
        m = parts.augmentation_matrix(parts.rs)
        assert m.dtype == np.float64 and m.shape == (3, 3)
        assert _same(np.matmul(xyz, m), g15[f"item/{i}/xyz"]), i
        assert np.array_equal(whole.rs.get_state()[1], parts.rs.get_state()[1]) and whole.rs.get_state()[2] == parts.rs.get_state()[2], i
    print("jittered items:", jittered)


def test_disabled_augmentations_draw_nothing_through_the_factored_methods(tmp_path, g15):
    _write_full(g15, str(tmp_path))
    off = dict(jitter=False, flip=False, rot=False, scaled=False, point_jitter=False)
    ds = CropDataset(str(tmp_path), 4, True, off, seed=3)
    state = ds.rs.get_state()[1].copy()
    assert not ds.point_jitter_coin(ds.rs) and np.array_equal(ds.augmentation_matrix(ds.rs), np.eye(3))
    assert np.array_equal(ds.rs.get_state()[1], state)


def test_device_loader_without_a_gpu_raises(tmp_path, g15, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from treelearn_amd.util.device_dataset import DeviceCropLoader
    _write_full(g15, str(tmp_path))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceCropLoader(str(tmp_path), 4, False)


def test_new_entry_points_are_declared_with_matching_arity():
    from treelearn_amd import _hip
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    for name in ("tl_point_jitter", "tl_train_item_ws_bytes", "tl_train_item"):
        m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/treelearn_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _hip.PROTOTYPES, name
        assert len(_hip.PROTOTYPES[name][1]) == n_args, (name, n_args, len(_hip.PROTOTYPES[name][1]))
        assert hasattr(_hip.lib(), name)
    L = _hip.lib()
    assert L.tl_train_item_ws_bytes(0) == 0 and L.tl_train_item_ws_bytes(1000) > 1000 * 140
    assert L.tl_train_item(None, None, 5, None, 4.0, None, 0, 0, None, None, None, None, None, None, None, None, None, None, None) == _hip.TL_ERR_ARG
    assert L.tl_point_jitter(None, 5, 1, None) == _hip.TL_ERR_ARG
