"""DeviceCropLoader, PlotTiler.tiles(offset_labels="device") and fit(device_batches=True) on the GPU, against
CropDataset + collate, the tiler's host mode and the host-fed training run.  The bounds are those of tests/test_gpu_train_batch.py
(check_test_mode / check_train_mode); an instance is left out of the offset comparison only where numpy's np.partition(z, 10)[3] is not
the value of rank 3 on the host data, at most 3 per item.

Each step runs in a child process of its own under a time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

MAX_LEFT_OUT = 3


def _step(name, *args, limit=300):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), name, *[str(a) for a in args]],
                       cwd=REPO, capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"step {name} exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


# ------------------------------------------------------------------------------------------------ helpers (child process)
def _g15():
    return np.load(os.path.join(HERE, "golden", "g15_crops.npz"))


def _write_crops(g, d):
    os.makedirs(d, exist_ok=True)
    names = sorted({str(k).split("/")[1] for k in g.files if str(k).startswith("full/")})
    for n in names:
        np.savez(os.path.join(d, n + ".npz"), **{k: g[f"full/{n}/{k}"] for k in g[f"keys/{n}"]})
    return names


def _host(batch):
    import torch
    torch.cuda.current_stream().wait_event(batch["_ready_event"])
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in batch.items() if k != "_ready_event"}


def _rows(dev, lo, hi):
    return {k: v[lo:hi] for k, v in dev.items() if isinstance(v, np.ndarray)}


def _kept_rows(it):
    left_out = [lab for lab, d in it["info"].items() if not d["numpy_pick_is_rank3"]]
    assert len(left_out) <= MAX_LEFT_OUT, left_out
    return ~np.isin(it["instance_label"], left_out)


def _same_as_collate(it_list, host_batch):
    """The restated items (numpy's pick) ARE what CropDataset + collate give: same matrices, same everything."""
    import torch
    import train_batch_restatement as R
    want = R.collate(it_list)
    for k, v in host_batch.items():
        if k == "input_feats":
            continue
        w = v.numpy() if torch.is_tensor(v) else v
        assert np.array_equal(np.asarray(w), np.asarray(want[k])), k


# ------------------------------------------------------------------------------------------------ 7. the loader
def step_loader(base):
    import torch
    import train_batch_restatement as R
    import test_gpu_train_batch as T
    from treelearn_amd.util.dataset import CropDataset, collate
    from treelearn_amd.util.device_dataset import DeviceCropLoader
    g = _g15()
    names = _write_crops(g, base)
    assert len(names) == 3
    inner = int(g["ds/inner"])
    aug = dict(json.loads(str(g["ds/aug"])), point_jitter=False)
    assert any(aug.values())
    files = [np.load(os.path.join(base, n + ".npz")) for n in names]

    def restated(ds_draws, i, training):
        f = files[i]
        if training:
            assert not ds_draws.point_jitter_coin(ds_draws.rs)
            return R.item(f["points"], f["instance_label"], inner, m=ds_draws.augmentation_matrix(ds_draws.rs), rank3=False)
        return R.item(f["points"], f["instance_label"], inner, center=f["center"], rank3=False)

    # training, batch size 1, file order: the matrices of CropDataset(seed 5)
    loader = DeviceCropLoader(base, inner, True, aug, seed=5, batch_size=1)
    ds, draws = CropDataset(base, inner, True, aug, seed=5), CropDataset(base, inner, True, aug, seed=5)
    assert len(loader) == 3
    seen = 0
    for i, batch in enumerate(loader):
        dev = _host(batch)
        it = restated(draws, i, True)
        hb = collate([ds[i]])
        _same_as_collate([it], hb)
        assert sorted(dev) == sorted(hb) and dev["batch_size"] == 1
        for k, v in hb.items():
            if torch.is_tensor(v):
                assert str(dev[k].dtype) == str(v.numpy().dtype) and dev[k].shape == tuple(v.shape), k
        assert np.array_equal(dev["input_feats"], hb["input_feats"].numpy()) and np.array_equal(dev["batch_ids"], hb["batch_ids"].numpy())
        T.check_train_mode(dev, it, f"loader training item {i}", rows=_kept_rows(it), inner=inner)
        seen += 1
    assert seen == 3
    # test mode
    loader = DeviceCropLoader(base, inner, False, batch_size=1)
    ds = CropDataset(base, inner, False)
    seen = 0
    for i, batch in enumerate(loader):
        dev = _host(batch)
        it = restated(None, i, False)
        hb = collate([ds[i]])
        _same_as_collate([it], hb)
        assert np.array_equal(dev["centers"], hb["centers"].numpy()) and np.array_equal(dev["input_feats"], hb["input_feats"].numpy())
        assert np.array_equal(dev["batch_ids"], hb["batch_ids"].numpy())
        T.check_test_mode(dev, it, f"loader test item {i}", rows=_kept_rows(it))
        seen += 1
    assert seen == 3
    # batch size 2: concatenation, batch ids, the odd item dropped in training mode and kept otherwise
    loader = DeviceCropLoader(base, inner, True, aug, seed=5, batch_size=2)
    draws = CropDataset(base, inner, True, aug, seed=5)
    batches = [_host(b) for b in loader]
    assert len(loader) == 1 and len(batches) == 1 and batches[0]["batch_size"] == 2
    its = [restated(draws, 0, True), restated(draws, 1, True)]
    n0, n1 = len(its[0]["xyz"]), len(its[1]["xyz"])
    dev = batches[0]
    assert len(dev["coords"]) == n0 + n1 and np.array_equal(dev["batch_ids"], np.repeat([0, 1], [n0, n1]))
    assert np.array_equal(dev["input_feats"], np.concatenate([files[0]["feat"], files[1]["feat"]]).reshape(n0 + n1, -1))
    T.check_train_mode(_rows(dev, 0, n0), its[0], "batch of two, item 0", rows=_kept_rows(its[0]), inner=inner)
    T.check_train_mode(_rows(dev, n0, n0 + n1), its[1], "batch of two, item 1", rows=_kept_rows(its[1]), inner=inner)
    loader = DeviceCropLoader(base, inner, False, batch_size=2)
    batches = [_host(b) for b in loader]
    assert len(loader) == 2 and [b["batch_size"] for b in batches] == [2, 1]
    assert len(batches[1]["coords"]) == len(files[2]["points"]) and (batches[1]["batch_ids"] == 0).all()
    T.check_test_mode(batches[1], restated(None, 2, False), "the last odd item", rows=None)
    # a seeded generator repeats the order; a new epoch is augmented anew (here with every augmentation, point jitter included)
    every = dict(jitter=True, flip=True, rot=True, scaled=True, point_jitter=True)

    def epochs(loader, k):
        return [[_host(b) for b in loader] for _ in range(k)]
    a = epochs(DeviceCropLoader(base, inner, True, every, seed=5, batch_size=1, generator=torch.Generator().manual_seed(11)), 2)
    b = epochs(DeviceCropLoader(base, inner, True, every, seed=5, batch_size=1, generator=torch.Generator().manual_seed(11)), 2)
    for ea, eb in zip(a, b):
        assert len(ea) == 3
        for x, y in zip(ea, eb):
            assert x["coords"].tobytes() == y["coords"].tobytes() and x["offset_labels"].tobytes() == y["offset_labels"].tobytes()
    orders = {tuple(len(x["coords"]) for x in e) for e in a}
    print("row counts per epoch (shuffled):", [tuple(len(x["coords"]) for x in e) for e in a])
    assert all(sorted(o) == sorted(len(f["points"]) for f in files) for o in orders)
    c = epochs(DeviceCropLoader(base, inner, True, every, seed=5, batch_size=1), 2)           # file order: epoch 1 against epoch 2, item by item
    assert all(np.isfinite(x["coords"]).all() and np.isfinite(x["offset_labels"]).all() for e in c for x in e)
    assert not any(np.array_equal(x["coords"], y["coords"]) for x, y in zip(c[0], c[1]))
    print("loader step OK")


def test_loader_against_cropdataset_and_collate(tmp_path):
    _step("loader", tmp_path)


# ------------------------------------------------------------------------------------------------ 8. the tiler's device mode
def step_tiler(base):
    import torch
    import train_batch_restatement as R
    import test_gpu_train_batch as T
    import test_gpu_train_loop as TL
    from treelearn_amd.util.tiles import PlotTiler, write_tiles
    from treelearn_amd.util.trainer import validate
    forest = TL._write_forest(base)                                                  # the 26 m synthetic plot
    n_tiles = write_tiles(forest, dict(voxel_size=0.1, inner_edge=8, outer_edge=4.0, stride=1))
    d = np.load(os.path.join(base, "forest_voxelized0.1", "plot.npz"))
    feats = np.load(os.path.join(base, "features", "plot.npz"))["features"]
    tiler = PlotTiler(d["points"], d["labels"], feats)
    host_tiles = [_host(b) for b in tiler.tiles(8, 4.0, 1, 8, offset_labels="host")]
    dev_tiles = [_host(b) for b in tiler.tiles(8, 4.0, 1, 8, offset_labels="device")]
    assert len(host_tiles) == len(dev_tiles) == n_tiles >= 4
    bound_sum, n_off = 0.0, 0
    for h, v in zip(host_tiles, dev_tiles):
        assert h["tile_index"] == v["tile_index"] and sorted(h) == sorted(v)
        for k in h:
            if k not in ("offset_labels", "masks_off"):
                assert np.array_equal(np.asarray(h[k]), np.asarray(v[k])), (h["tile_index"], k)
                assert np.asarray(h[k]).dtype == np.asarray(v[k]).dtype, (h["tile_index"], k)
        it = R.item(h["coords"], h["instance_labels"].astype(np.int32), 8, center=h["centers"][0], rank3=False)
        assert np.array_equal(it["pt_offset_label"], h["offset_labels"]) and np.array_equal(it["mask_off"], h["masks_off"])
        rows = _kept_rows(it)
        T.check_test_mode({k: v[k] for k in T.KEYS}, it, f"tile {h['tile_index']}", rows=rows)
        # what validate sums: |offset - label| over the rows with masks_sem and the tree class; a label that moves by e moves a term by <= |e|
        counted = h["masks_sem"] & (h["semantic_labels"] == 0)
        a, b = v["offset_labels"].astype(np.float64), h["offset_labels"].astype(np.float64)
        tol = R.position_tolerance(it)[:, None] + R.ulp32(it["position"]) + R.ulp32(np.maximum(np.abs(a), np.abs(b)))
        tol[~rows] = np.abs(a - b)[~rows]                                          # instances left out: what they actually differ by
        bound_sum += float(np.linalg.norm(tol[counted], axis=1).sum()); n_off += int(counted.sum())
    model = TL._model()
    wa, wb = TL._Writer(), TL._Writer()
    a = validate(dict(epochs=1), 1, model, tiler.tiles(8, 4.0, 1, 8, offset_labels="host"), None, wa)
    b = validate(dict(epochs=1), 1, model, tiler.tiles(8, 4.0, 1, 8, offset_labels="device"), None, wb)
    print("validate host labels  :", a)
    print("validate device labels:", b)
    for k in ("tp", "fp", "tn", "fn", "n_off"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["n_off"] == n_off > 0
    print(f"|MAE difference| {abs(a['offset_mae'] - b['offset_mae']):.3e}, bound {bound_sum / n_off:.3e}")
    assert abs(a["offset_mae"] - b["offset_mae"]) < bound_sum / n_off
    print("tiler step OK")


def test_tiler_device_offset_labels_against_host(tmp_path):
    _step("tiler", tmp_path)


# ------------------------------------------------------------------------------------------------ 9. fit
def step_fit(base):
    import math
    import torch
    import test_gpu_train_loop as TL
    from treelearn_amd.util import trainer
    TL._write_training_data(base)
    cfg = TL._config(base, "run", epochs=4)
    cfg.device_batches = True
    finite = []                                                                      # one flag per training step
    make = trainer._grad_scaler

    class Checked:
        """The grad scaler fit builds, looking at every parameter gradient of EVERY step just before the optimizer gets it."""

        def __init__(self, scaler):
            self.scaler = scaler

        def step(self, optimizer):
            grads = [p.grad for g in optimizer.param_groups for p in g["params"] if p.requires_grad]
            assert grads and all(gr is not None for gr in grads), "a parameter without a gradient"
            finite.append(all(bool(torch.isfinite(gr).all()) for gr in grads))
            return self.scaler.step(optimizer)

        def __getattr__(self, name):
            return getattr(self.scaler, name)
    seen = []
    from treelearn_amd.util import device_dataset
    made = device_dataset.DeviceCropLoader.__init__

    def counting(self, *a, **k):
        seen.append(1)
        return made(self, *a, **k)
    trainer._grad_scaler = lambda enabled: Checked(make(enabled))
    device_dataset.DeviceCropLoader.__init__ = counting
    try:
        trainer.fit(cfg)
    finally:
        trainer._grad_scaler = make
        device_dataset.DeviceCropLoader.__init__ = made
    assert len(seen) == 2, "fit did not build the two device loaders"
    sc = TL._scalars(cfg.work_dir)
    epochs = [1, 2, 3, 4]
    for tag in ("train/semantic_loss", "train/offset_loss", "val/acc", "val/Offset_MAE"):
        assert sorted(sc[tag]) == epochs and all(math.isfinite(v) for v in sc[tag].values()), (tag, sc.get(tag))
    total = {e: sc["train/semantic_loss"][e] + sc["train/offset_loss"][e] for e in epochs}
    print("mean total loss per epoch:", total)
    print("val/acc:", sc["val/acc"], "val/Offset_MAE:", sc["val/Offset_MAE"], "grad scale:", sc["train/grad_scale"])
    # The run is fp16 with loss scaling, as test_gpu_train_loop's: a step whose SCALED gradients overflow is the scaler's to skip (it halves the
    # scale, growth needs 2000 good steps) and the host-fed run allows TL.MAX_SKIPPED of them.  Every other step's gradients must be finite:
    # the non-finite steps are exactly the skipped ones, so no non-finite gradient ever reaches the optimizer.
    skipped = math.log2(65536.0 / sc["train/grad_scale"][4])
    print(f"{len(finite)} steps, {finite.count(False)} with a non-finite scaled gradient, {skipped} skipped by the scaler")
    assert len(finite) >= 4 and finite.count(False) == skipped <= TL.MAX_SKIPPED, (finite, skipped)
    assert total[4] < total[1]
    assert sc["val/acc"][4] > sc["val/acc"][1]
    print("fit step OK")


def test_fit_with_device_batches(tmp_path):
    _step("fit", tmp_path)


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    globals()["step_" + sys.argv[1]](*sys.argv[2:])
