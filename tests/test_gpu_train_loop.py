"""The training program on the GPU: tl_pointwise_eval against the CPU restatement of the reference's pointwise_eval, `validate`
over device tiles and over tile files, `fit` for a few epochs, resume.

Each step runs in a child process of its own under a time limit (`timeout -k 10 <s> python tests/test_gpu_train_loop.py <step> ...`): a fault
or a hang ends that step and names it, and the next test starts from a fresh process."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

MODEL = dict(channels=32, num_blocks=4, use_feats=False, use_coords=False, spatial_shape=[256, 256, 512], voxel_size=0.1)   # tests/test_gpu_train_fused.py, 20-step test
MAX_SKIPPED = 8                                                                                                           # ... and its bound on skipped steps


def _step(name, *args, limit=300):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), name, *[str(a) for a in args]],
                       cwd=REPO, capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"step {name} exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


# ============================================================================================ 1. the kernel
def _inputs(n, dtype, seed):
    """Logits whose difference is exactly 0 or at least 1e-3 AFTER rounding to `dtype`: any faithful fp32 softmax decides them alike."""
    import torch
    g = torch.Generator().manual_seed(seed)
    l1 = torch.randn(n, generator=g).to(dtype)
    d = (torch.rand(n, generator=g) * 3 + 1e-3) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    d[torch.rand(n, generator=g) < 0.1] = 0.0                                        # ties: count as tree
    l0 = (l1.float() + d).to(dtype)
    diff = (l0.float() - l1.float()).abs()
    l0 = torch.where((diff > 0) & (diff < 1e-3), l1, l0)
    diff = (l0.float() - l1.float()).abs()
    assert bool(((diff == 0) | (diff >= 1e-3)).all()) and int((diff == 0).sum()) > 0.05 * n
    logits = torch.stack([l0, l1], 1).contiguous()
    offsets = (torch.randn(n, 3, generator=g) * 2).to(dtype)
    lab = torch.randn(n, 3, generator=g)
    sem = torch.randint(0, 2, (n,), generator=g)
    mask = torch.rand(n, generator=g) < 0.7
    return logits, offsets, sem, lab, mask


def _run_kernel(logits, offsets, sem, lab, mask):
    import torch
    from treelearn_amd.util.trainer import EvalState
    st = EvalState()
    st.add(logits, offsets, sem, lab, mask)
    torch.cuda.synchronize()
    return st


def _check(got, logits, offsets, sem, lab, mask, what):
    import train_restatement as R
    m = slice(None) if mask is None else mask.cpu()
    want = R.pointwise_eval(logits.cpu()[m], offsets.cpu()[m], sem.cpu()[m], lab.cpu()[m])
    mae = got["sum_off"] / got["n_off"] if got["n_off"] else 0.0
    print(f"{what}: counts {[got[k] for k in ('tp', 'fp', 'tn', 'fn', 'n_off')]} mae {mae!r} restatement {want['offset_mae']!r}")
    for k in ("tp", "fp", "tn", "fn", "n_off"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    n = len(logits) if mask is None else int(mask.sum())
    assert got["tp"] + got["fp"] + got["tn"] + got["fn"] == n                     # nothing left out
    assert mae == pytest.approx(want["offset_mae"], rel=1e-5), what
    if got["n_off"] == 0:
        assert mae == 0.0 and got["sum_off"] == 0.0


def step_kernel(dtype_name):
    import torch
    from treelearn_amd.util.trainer import EvalState, pointwise_eval
    dtype = dict(f32=torch.float32, f16=torch.float16, bf16=torch.bfloat16)[dtype_name]
    n = 1_000_003                                                                   # not a multiple of the workgroup size or of a lane's 4 rows
    host = _inputs(n, dtype, seed=11)
    logits, offsets, sem, lab, mask = (t.cuda() for t in host)
    whole = _run_kernel(logits, offsets, sem, lab, mask)
    _check(whole.read(), logits, offsets, sem, lab, mask, f"{dtype_name} 1M masked")
    again = _run_kernel(logits, offsets, sem, lab, mask)
    assert torch.equal(whole.state, again.state), "two identical runs differ"        # bit-identical state
    _check(_run_kernel(logits, offsets, sem, lab, None).read(), logits, offsets, sem, lab, None, f"{dtype_name} NULL mask")
    none = torch.zeros_like(mask)
    st = _run_kernel(logits, offsets, sem, lab, none)
    assert not bool(st.state.any()), "an all-false mask must leave the state at zero"
    _check(st.read(), logits, offsets, sem, lab, none, f"{dtype_name} all-false mask")
    # two calls on halves == one call on the whole (the second half starts at an odd row: the row-by-row form)
    h = n // 2
    halves = EvalState()
    halves.add(logits[:h], offsets[:h], sem[:h], lab[:h], mask[:h])
    halves.add(logits[h:], offsets[h:], sem[h:], lab[h:], mask[h:])
    a, b = whole.read(), halves.read()
    for k in ("tp", "fp", "tn", "fn", "n_off"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert b["sum_off"] == pytest.approx(a["sum_off"], rel=1e-12)
    # slices that break the 16-byte alignment one array at a time agree with the aligned run
    for lo in (1, 2, 3, 4):
        sl = slice(lo, n - 5)
        _check(_run_kernel(logits[sl], offsets[sl], sem[sl], lab[sl], mask[sl]).read(), logits[sl], offsets[sl], sem[sl], lab[sl], mask[sl],
               f"{dtype_name} rows {lo}..")
    # n = 0, small n, no tree rows
    st = EvalState()
    st.add(logits[:0], offsets[:0], sem[:0], lab[:0], mask[:0])
    assert not bool(st.state.any())
    for m in (1, 3, 255, 1001):
        _check(_run_kernel(logits[:m], offsets[:m], sem[:m], lab[:m], None).read(), logits[:m], offsets[:m], sem[:m], lab[:m], None, f"{dtype_name} n={m}")
    ones = torch.ones_like(sem)
    got = _run_kernel(logits, offsets, ones, lab, mask).read()
    _check(got, logits, offsets, ones, lab, mask, f"{dtype_name} no tree rows")
    assert got["n_off"] == 0 and got["tp"] == 0 and got["fn"] == 0

    class W:
        def __init__(self): self.rows = []
        def add_scalar(self, tag, value, step): self.rows.append((tag, float(value), step))
    w = W()
    r = pointwise_eval(logits, offsets, ones, lab, dict(epochs=3), 2, w, None)      # the Python side: 0 * sum -> 0
    assert r["offset_mae"] == 0.0 and w.rows[1] == ("val/Offset_MAE", 0.0, 2) and w.rows[0][0] == "val/acc"
    r = pointwise_eval(logits, offsets, sem, lab, dict(epochs=3), 1, w, None)
    _check(r, logits, offsets, sem, lab, None, f"{dtype_name} pointwise_eval()")
    assert w.rows[2] == ("val/acc", r["acc"], 1)
    # NaN accuracy (no counted row) is written as 0
    r = pointwise_eval(logits[:0], offsets[:0], sem[:0], lab[:0], dict(epochs=3), 1, w, None)
    assert math.isnan(r["acc"]) and w.rows[4] == ("val/acc", 0.0, 1)
    print("kernel step OK")


@pytest.mark.parametrize("dtype_name", ["f32", "f16", "bf16"])
def test_pointwise_eval_kernel_against_the_restatement(dtype_name):
    _step("kernel", dtype_name)


# ============================================================================================ 2. validate, two routes
def _write_forest(base, extent=26.0, seed=5, name="plot"):
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=extent, voxel=0.2, n_trees=int(extent * extent / 60), seed=seed)
    p = t["points"].astype(np.float64) + np.array([250.0, -140.0, 3.0])
    lab = t["instance_label"].astype(np.float64)
    lab[np.random.default_rng(seed).uniform(size=len(lab)) < 0.05] = -1
    os.makedirs(os.path.join(base, "forest"), exist_ok=True)
    path = os.path.join(base, "forest", f"{name}.npy")
    np.save(path, np.hstack([p, lab[:, None]]))
    return path


def _model(seed=5):
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import random_state_dict
    model = TreeLearn(**MODEL)
    model.load_state_dict(random_state_dict(seed, channels=MODEL["channels"], num_blocks=MODEL["num_blocks"]), strict=True)
    return model.cuda()


class _Writer:
    def __init__(self): self.rows = []
    def add_scalar(self, tag, value, step): self.rows.append((tag, float(value), step))
    def flush(self): pass


def step_validate(base):
    import torch
    from torch.utils.data import DataLoader
    import train_restatement as R
    from treelearn_amd.util.dataset import CropDataset
    from treelearn_amd.util.tiles import PlotTiler, write_tiles
    from treelearn_amd.util.trainer import validate
    forest = _write_forest(base)
    sample = dict(voxel_size=0.1, inner_edge=8, outer_edge=4.0, stride=1)
    n_tiles = write_tiles(forest, sample)
    names = sorted(os.listdir(os.path.join(base, "tiles", "npz")))
    assert n_tiles >= 4 and sorted(names) == sorted(f"plot_{i}.npz" for i in range(n_tiles))
    assert sorted(os.listdir(os.path.join(base, "tiles", "json"))) == sorted(f"plot_{i}.json" for i in range(n_tiles))
    assert os.listdir(os.path.join(base, "forest_voxelized0.1")) == ["plot.npz"] and os.listdir(os.path.join(base, "features")) == ["plot.npz"]
    meta = json.load(open(os.path.join(base, "tiles", "json", "plot_0.json")))
    assert list(meta) == ["plot_name", "n_neigh_sor", "multiplier_sor", "rad", "npoints_rad", "inner_edge", "outer_edge"]
    assert meta["plot_name"] == "plot" and meta["inner_edge"] == 8 and meta["outer_edge"] == 4.0 and meta["rad"] is None
    f0 = np.load(os.path.join(base, "tiles", "npz", "plot_0.npz"))
    assert (f0["points"].dtype, f0["feat"].dtype, f0["instance_label"].dtype, f0["center"].dtype) == (np.float32, np.float32, np.int32, np.float64)
    assert f0["center"].shape == (3,) and f0["points"].shape[1] == 3 and len(f0["feat"]) == len(f0["points"]) == len(f0["instance_label"])
    assert write_tiles(forest, sample) == n_tiles                                   # the caches are reused

    d = np.load(os.path.join(base, "forest_voxelized0.1", "plot.npz"))
    feats = np.load(os.path.join(base, "features", "plot.npz"))["features"]
    tiler = PlotTiler(d["points"], d["labels"], feats)
    device_tiles = lambda: tiler.tiles(8, 4.0, 1, 8, offset_labels="host")          # noqa: E731
    ds = CropDataset(os.path.join(base, "tiles", "npz"), 8, training=False)
    order = [int(os.path.basename(p)[:-4].split("_")[-1]) for p in ds.data_paths]    # name order is not tile order
    loader = DataLoader(ds, batch_size=1, collate_fn=ds.collate_fn, shuffle=False, num_workers=0)

    # the batches of the two routes, key by key
    by_index = {i: b for i, b in zip(order, loader)}
    n_seen = 0
    for i, tb in enumerate(device_tiles()):
        fb = by_index[i]
        torch.cuda.current_stream().wait_event(tb["_ready_event"])
        for k, v in fb.items():
            if torch.is_tensor(v):
                assert v.dtype == tb[k].dtype and torch.equal(v, tb[k].cpu()), (i, k)
            else:
                assert v == tb[k], (i, k)
        n_seen += 1
    assert n_seen == n_tiles

    model = _model()
    cfg = dict(epochs=1)
    wa, wb = _Writer(), _Writer()
    a = validate(cfg, 1, model, device_tiles(), None, wa)
    b = validate(cfg, 1, model, loader, None, wb)
    print("validate device tiles:", a)
    print("validate tile files  :", b)
    for k in ("tp", "fp", "tn", "fn", "n_off"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["offset_mae"] == pytest.approx(b["offset_mae"], rel=1e-6)
    assert [r[0] for r in wa.rows] == ["val/acc", "val/Offset_MAE"] and wa.rows[0][1] == a["acc"] and wa.rows[1][1] == a["offset_mae"]
    # ... and the restatement on what the reference's validate would concatenate
    model.eval()
    pairs = []
    with torch.no_grad():
        for tb in device_tiles():
            torch.cuda.current_stream().wait_event(tb["_ready_event"])
            out = model(tb, return_loss=False)
            pairs.append(({k: v.cpu() for k, v in out.items()}, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in tb.items() if k != "_ready_event"}))
    want = R.pointwise_eval(*R.gather_for_validate(pairs))
    print("restatement          :", want)
    assert want["n_off"] > 0 and want["tp"] + want["fp"] + want["tn"] + want["fn"] > 10000
    for k in ("tp", "fp", "tn", "fn", "n_off"):
        assert a[k] == want[k], (k, a[k], want[k])
    assert a["acc"] == pytest.approx(want["acc"], rel=1e-12)
    assert a["offset_mae"] == pytest.approx(want["offset_mae"], rel=1e-5)
    print("validate step OK")


def test_validate_over_device_tiles_and_over_tile_files(tmp_path):
    _step("validate", tmp_path)


# ============================================================================================ 3. fit and resume
def _write_training_data(base, n_train=6, n_val=2):
    """Synthetic crops / tiles in the crop file format (points, feat, instance_label, center), and the start weights as a checkpoint."""
    import torch
    from treelearn_amd.synth import make_tile, random_state_dict
    for sub, n, seed0 in (("train", n_train, 1), ("val", n_val, 101)):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
        for k in range(n):
            t = make_tile(extent=12.0, voxel=0.1, n_trees=6, fill=0.10, seed=seed0 + k)
            np.savez(os.path.join(base, sub, f"synth_{k}.npz"), points=t["points"].astype(np.float32), feat=t["feat"].astype(np.float32),
                     instance_label=t["instance_label"].astype(np.int32), center=np.asarray(t["center"], np.float64))
    torch.save(dict(net=random_state_dict(5, channels=MODEL["channels"], num_blocks=MODEL["num_blocks"])), os.path.join(base, "start.pth"))


def _config(base, work, epochs):
    from treelearn_amd.util.config import Config
    none = dict(jitter=False, flip=False, rot=False, scaled=False, point_jitter=False)
    return Config.from_dict(dict(
        model=MODEL, seed=3, work_dir=os.path.join(base, work),
        dataset_train=dict(training=True, data_root=os.path.join(base, "train"), data_augmentations=none, inner_square_edge_length=8),
        dataset_test=dict(training=False, data_root=os.path.join(base, "val"), inner_square_edge_length=8),
        dataloader=dict(train=dict(batch_size=2, num_workers=0), test=dict(batch_size=1, num_workers=0)),
        optimizer=dict(type="AdamW", lr=1e-3, weight_decay=1e-3),
        scheduler=dict(t_initial=100, lr_min=5e-5, cycle_decay=1, warmup_lr_init=1e-4, warmup_t=2, cycle_limit=1, t_in_epochs=True),
        epochs=epochs, examples_per_epoch=6, fp16=True, pretrain=os.path.join(base, "start.pth"), grad_norm_clip=True,
        save_frequency=2, validation_frequency=1))


def _scalars(work):
    from treelearn_amd.util.trainer import ScalarLog
    out = {}
    for r in ScalarLog.read(os.path.join(work, "scalars.jsonl")):
        out.setdefault(r["tag"], {})[r["step"]] = r["value"]
    return out


def _schedule_lr(cfg, epoch):
    s = cfg.scheduler
    base = cfg.optimizer.lr
    if epoch < s.warmup_t:
        return s.warmup_lr_init + epoch * (base - s.warmup_lr_init) / s.warmup_t
    return s.lr_min + 0.5 * (base - s.lr_min) * (1 + math.cos(math.pi * epoch / s.t_initial))


def step_fit(base):
    from treelearn_amd.util.trainer import fit
    _write_training_data(base)
    cfg = _config(base, "run", epochs=4)
    fit(cfg)
    sc = _scalars(cfg.work_dir)
    epochs = [1, 2, 3, 4]
    for tag in ("train/learning_rate", "train/semantic_loss", "train/offset_loss", "val/acc", "val/Offset_MAE"):
        assert sorted(sc[tag]) == epochs, (tag, sc.get(tag))
        assert all(math.isfinite(v) for v in sc[tag].values()), (tag, sc[tag])
    total = {e: sc["train/semantic_loss"][e] + sc["train/offset_loss"][e] for e in epochs}
    print("mean total loss per epoch:", total)
    print("val/acc:", sc["val/acc"], "val/Offset_MAE:", sc["val/Offset_MAE"], "grad scale:", sc["train/grad_scale"])
    assert total[4] < total[1]
    skipped = math.log2(65536.0 / sc["train/grad_scale"][4])                          # every skipped step halves the scale (growth needs 2000 good steps)
    print("skipped steps:", skipped)
    assert 0 <= skipped <= MAX_SKIPPED
    for e in epochs:
        assert sc["train/learning_rate"][e] == pytest.approx(_schedule_lr(cfg, e), rel=1e-12)
    assert 0.0 <= sc["val/acc"][4] <= 1.0 and sc["val/Offset_MAE"][4] > 0
    assert sorted(f for f in os.listdir(cfg.work_dir) if f.endswith(".pth")) == ["epoch_2.pth", "epoch_4.pth"]     # retention, save_frequency 2
    print("fit step OK")


def step_resume(base):
    import torch
    from treelearn_amd.util import trainer
    _write_training_data(base)
    cfg = _config(base, "run", epochs=2)
    trainer.fit(cfg)
    ckpt = os.path.join(cfg.work_dir, "epoch_2.pth")
    saved = torch.load(ckpt, map_location="cpu")
    seen = {}
    inner = trainer.train_epoch

    def spy(config, epoch, model, optimizer, *rest):
        if not seen:                                                                 # before the first step of the resumed run
            seen["epoch"] = epoch
            seen["net"] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            seen["opt"] = optimizer.state_dict()
            seen["opt"] = dict(param_groups=[dict(g) for g in seen["opt"]["param_groups"]],
                               state={k: {n: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for n, v in s.items()} for k, s in seen["opt"]["state"].items()})
        return inner(config, epoch, model, optimizer, *rest)

    trainer.train_epoch = spy
    try:
        trainer.fit(_config(base, "run", epochs=4), resume=ckpt)
    finally:
        trainer.train_epoch = inner
    assert seen["epoch"] == 3
    assert list(seen["net"]) == list(saved["net"])
    for k, v in saved["net"].items():
        assert torch.equal(v, seen["net"][k]), k
    assert seen["opt"]["param_groups"] == saved["optimizer"]["param_groups"]
    assert list(seen["opt"]["state"]) == list(saved["optimizer"]["state"]) and len(saved["optimizer"]["state"]) > 0
    for k, s in saved["optimizer"]["state"].items():
        for n, v in s.items():
            assert torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(seen["opt"]["state"][k][n]).cpu()), (k, n)
    sc = _scalars(cfg.work_dir)
    assert sorted(sc["train/learning_rate"]) == [1, 2, 3, 4] and sorted(sc["val/acc"]) == [1, 2, 3, 4]
    assert sc["train/learning_rate"][3] == pytest.approx(_schedule_lr(cfg, 3), rel=1e-12)
    assert all(math.isfinite(sc[t][e]) for t in ("train/semantic_loss", "train/offset_loss") for e in (3, 4))
    assert sorted(f for f in os.listdir(cfg.work_dir) if f.endswith(".pth")) == ["epoch_2.pth", "epoch_4.pth"]
    print("resume step OK")


def test_fit_trains_validates_logs_and_keeps_the_right_checkpoints(tmp_path):
    _step("fit", tmp_path)


def test_resume_continues_from_the_saved_state(tmp_path):
    _step("resume", tmp_path)


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    globals()["step_" + sys.argv[1]](*sys.argv[2:])
