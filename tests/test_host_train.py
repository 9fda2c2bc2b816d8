"""Host side of the training program (no GPU): LR schedule, checkpoints, config merge, the two new C entries, ScalarLog, both CLIs,
and the CPU restatement the GPU tests lean on."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt(lr=3e-3):
    return torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=lr, weight_decay=1e-3)


def test_cosine_schedule_closed_forms():
    """timm 0.6.12's CosineLRScheduler for the reference's arguments, against closed forms in float64 (1e-12 relative)."""
    from treelearn_amd.util.train import build_cosine_scheduler
    base, lr_min, w0 = 3e-3, 5e-5, 1e-5
    cfg = dict(t_initial=1000, lr_min=lr_min, cycle_decay=1, warmup_lr_init=w0, warmup_t=50, cycle_limit=1, t_in_epochs=True)   # configs/training/train.yaml
    opt = _opt(base)
    sch = build_cosine_scheduler(cfg, opt)
    lr = lambda: opt.param_groups[0]["lr"]                                               # noqa: E731
    assert lr() == w0                                                                    # set at construction
    sch.step(0); assert lr() == pytest.approx(w0, rel=1e-12)
    sch.step(1); assert lr() == pytest.approx(w0 + (base - w0) / 50, rel=1e-12)
    sch.step(49); assert lr() == pytest.approx(w0 + 49 * (base - w0) / 50, rel=1e-12)
    sch.step(50); assert lr() == pytest.approx(lr_min + 0.5 * (base - lr_min) * (1 + math.cos(0.05 * math.pi)), rel=1e-12)
    sch.step(500); assert lr() == pytest.approx((base + lr_min) / 2, rel=1e-12)
    for t in (1000, 1001, 2500):
        sch.step(t); assert lr() == pytest.approx(lr_min, rel=1e-12)
    # attribute-style config, two cycles with decay
    from treelearn_amd.util.config import Config
    cfg2 = Config(t_initial=100, lr_min=lr_min, cycle_decay=0.5, warmup_lr_init=w0, warmup_t=0, cycle_limit=2, t_in_epochs=True)
    opt = _opt(base)
    sch = build_cosine_scheduler(cfg2, opt)
    assert lr() == base                                                                  # no warmup: untouched at construction
    sch.step(0); assert lr() == pytest.approx(base, rel=1e-12)
    sch.step(100); assert lr() == pytest.approx(base * 0.5, rel=1e-12)                    # the second cycle's peak
    sch.step(150); assert lr() == pytest.approx(lr_min + 0.5 * (base * 0.5 - lr_min), rel=1e-12)
    for t in (200, 201, 1000):
        sch.step(t); assert lr() == pytest.approx(lr_min, rel=1e-12)
    # a schedule that counts updates ignores step(epoch)
    opt = _opt(base)
    sch = build_cosine_scheduler(dict(cfg, t_in_epochs=False), opt)
    sch.step(500); assert lr() == w0
    sch.step_update(500); assert lr() == pytest.approx((base + lr_min) / 2, rel=1e-12)


def test_checkpoint_save_retention_and_round_trip(tmp_path):
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.util.train import build_optimizer, checkpoint_save, is_multiple, load_checkpoint, weights_to_cpu
    assert is_multiple(4, 2) and not is_multiple(0, 2) and not is_multiple(5, 2)
    cfg = dict(channels=16, num_blocks=2, use_feats=False, use_coords=False, spatial_shape=[64, 64, 64])
    torch.manual_seed(0)
    model = TreeLearn(**cfg)
    opt = build_optimizer(model, dict(type="AdamW", lr=1e-3, weight_decay=1e-3))
    assert isinstance(opt, torch.optim.AdamW) and opt.param_groups[0]["weight_decay"] == 1e-3
    for p in model.parameters():
        p.grad = torch.randn_like(p)
    opt.step()
    work = str(tmp_path)
    for epoch in range(1, 6):
        checkpoint_save(epoch, model, opt, work, save_freq=2)
    assert sorted(os.listdir(work)) == ["epoch_2.pth", "epoch_4.pth", "epoch_5.pth"]
    state = torch.load(os.path.join(work, "epoch_4.pth"), map_location="cpu")
    assert set(state) == {"net", "optimizer", "epoch"} and state["epoch"] == 4
    assert all(v.device.type == "cpu" for v in state["net"].values())
    assert all(v.device.type == "cpu" for v in weights_to_cpu(model.state_dict()).values())
    torch.manual_seed(1)
    fresh = TreeLearn(**cfg)
    opt2 = build_optimizer(fresh, dict(type="AdamW", lr=1e-3, weight_decay=1e-3))
    assert load_checkpoint(os.path.join(work, "epoch_4.pth"), None, fresh, optimizer=opt2) == 5
    a, b = model.state_dict(), fresh.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    sa, sb = opt.state_dict(), opt2.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and list(sa["state"]) == list(sb["state"])
    for k in sa["state"]:
        for name, v in sa["state"][k].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb["state"][k][name])), (k, name)


def test_config_merge_and_path_resolution(tmp_path, monkeypatch):
    from treelearn_amd.util.config import Config, get_config, to_dict
    root = tmp_path / "proj"
    (root / "configs" / "_modular").mkdir(parents=True)
    (root / "configs" / "training").mkdir(parents=True)
    (root / "configs" / "_modular" / "model.yaml").write_text("model:\n  channels: 32\n  num_blocks: 7\n  spatial_shape: ~\n  nested:\n    a: 1\n    b: 2\n")
    (root / "configs" / "_modular" / "data.yaml").write_text("dataset_train:\n  training: True\n  data_root: 'x/y'\n  data_augmentations:\n    jitter: True\n    flip: True\n")
    main = root / "configs" / "training" / "train.yaml"
    main.write_text('default_args: ["configs/_modular/model.yaml", "configs/_modular/data.yaml"]\n'
                    "model:\n  spatial_shape: [500, 500, 1000]\n  nested:\n    b: 3\n"
                    "dataset_train:\n  data_augmentations:\n    flip: False\n"
                    "optimizer:\n  type: 'AdamW'\n  lr: 0.003\nepochs: 5\npretrain: ~\n")
    monkeypatch.chdir(tmp_path)                                   # the default_args paths do not exist relative to here: ancestor fallback
    cfg = get_config(str(main))
    assert "default_args" not in cfg
    assert cfg.model.spatial_shape == [500, 500, 1000] and cfg.model.channels == 32 and cfg.model.num_blocks == 7
    assert cfg.model.nested == {"a": 1, "b": 3}
    assert cfg.dataset_train.data_augmentations.flip is False and cfg.dataset_train.data_augmentations.jitter is True
    assert cfg.dataset_train.data_root == "x/y" and cfg.optimizer.lr == 0.003 and cfg.epochs == 5 and cfg.pretrain is None
    assert isinstance(cfg, Config) and isinstance(cfg.model, Config) and cfg["model"]["channels"] == 32
    cfg.work_dir = "w"
    assert cfg["work_dir"] == "w"
    with pytest.raises(AttributeError):
        cfg.no_such_key
    plain = to_dict(cfg)
    assert type(plain) is dict and type(plain["model"]) is dict
    monkeypatch.chdir(root)                                       # as given, the reference's way
    assert to_dict(get_config(str(main))) == {k: v for k, v in plain.items() if k != "work_dir"}
    (root / "configs" / "training" / "bad.yaml").write_text('default_args: ["configs/_modular/none.yaml"]\n')
    with pytest.raises(FileNotFoundError):
        get_config(str(root / "configs" / "training" / "bad.yaml"))


def test_new_entry_points_are_declared_prototyped_and_exported():
    from treelearn_amd import _hip, build as b
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    names = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(b.build(verbose=False))
    for n in ("tl_pointwise_eval", "tl_pointwise_eval_ws_bytes"):
        assert n in names and n in _hip.PROTOTYPES and hasattr(L, n)
    assert "train.py:89-102" in hdr
    lib = _hip.lib()
    assert lib.tl_pointwise_eval_ws_bytes(0) >= 64 and lib.tl_pointwise_eval_ws_bytes(1 << 22) >= lib.tl_pointwise_eval_ws_bytes(1000)
    assert lib.tl_pointwise_eval_ws_bytes(1 << 40) == lib.tl_pointwise_eval_ws_bytes(1 << 30)      # bounded: the grid is capped
    # null pointers, a negative count, an unknown dtype: refused before anything is launched (no GPU here)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    assert lib.tl_pointwise_eval(None, None, 0, None, None, None, 0, None, None, None) < 0
    assert lib.tl_pointwise_eval(p, p, 0, p, p, None, -1, p, p, None) < 0
    assert lib.tl_pointwise_eval(p, p, 7, p, p, None, 4, p, p, None) < 0
    assert lib.tl_pointwise_eval(p, p, 0, p, p, None, 4, p + 4, p, None) < 0                        # misaligned state
    assert lib.tl_pointwise_eval(p, p, 0, p, p, None, 0, p, p, None) == 0                           # n == 0: a no-op


def test_scalar_log_round_trips(tmp_path):
    from treelearn_amd.util.trainer import ScalarLog
    w = ScalarLog(str(tmp_path / "run"))
    w.add_scalar("train/learning_rate", 3e-3, 1)
    w.add_scalar("val/acc", torch.tensor(0.75), 1)
    w.add_scalar("val/Offset_MAE", 1.25, 2)
    w.flush()
    lines = [json.loads(s) for s in open(tmp_path / "run" / "scalars.jsonl").read().splitlines()]
    assert lines == [dict(tag="train/learning_rate", value=3e-3, step=1), dict(tag="val/acc", value=0.75, step=1),
                     dict(tag="val/Offset_MAE", value=1.25, step=2)]
    w.close()
    w2 = ScalarLog(str(tmp_path / "run"))                        # a resumed run appends
    w2.add_scalar("val/acc", 0.5, 3); w2.close()
    assert [r["step"] for r in ScalarLog.read(w2.path)] == [1, 1, 2, 3]


def test_command_lines_accept_the_documented_flags():
    from treelearn_amd.util import tiles, trainer
    a = trainer.parse_args(["--config", "configs/training/train.yaml", "--resume", "work_dirs/x/epoch_40.pth", "--work_dir", "run7"])
    assert (a.config, a.resume, a.work_dir) == ("configs/training/train.yaml", "work_dirs/x/epoch_40.pth", "run7")
    assert trainer.work_dir_of(a) == os.path.join("./work_dirs", "run7")
    b = trainer.parse_args(["--config", "a/b/train_small.yaml"])
    assert b.resume is None and trainer.work_dir_of(b) == os.path.join("./work_dirs", "train_small")
    with pytest.raises(SystemExit):
        trainer.parse_args([])
    t = tiles.parse_args(["--forest", "data/val/forest/L1W.npy"])
    assert t.forest == "data/val/forest/L1W.npy" and (t.voxel_size, t.inner_edge, t.outer_edge, t.stride) == (0.1, 8, 13.5, 1)
    t = tiles.parse_args(["--forest", "f.npz", "--voxel-size", "0.2", "--inner-edge", "6", "--outer-edge", "9", "--stride", "0.5"])
    assert (t.voxel_size, t.inner_edge, t.outer_edge, t.stride) == (0.2, 6.0, 9.0, 0.5)
    with pytest.raises(SystemExit):
        tiles.parse_args(["--forest", "f.npz", "--stride", "0"])


def test_write_tiles_refuses_the_denoising_keys(tmp_path):
    from treelearn_amd.util.tiles import write_tiles
    for k in ("n_neigh_sor", "multiplier_sor", "rad", "npoints_rad"):
        with pytest.raises(NotImplementedError, match=k):
            write_tiles(str(tmp_path / "forest" / "p.npy"), dict(sample_generator={k: 2.0}))


def test_restatement_on_a_hand_worked_example():
    import train_restatement as R
    logits = torch.tensor([[2.0, 0.0], [0.0, 2.0], [1.0, 1.0], [0.0, 3.0], [5.0, 1.0]])        # tree, non-tree, tie (tree), non-tree, tree
    sem = torch.tensor([0, 0, 1, 1, 0])
    off = torch.tensor([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0], [9.0, 9.0, 9.0], [1.0, 1.0, 1.0], [1.0, 2.0, 2.0]])
    lab = torch.zeros(5, 3)
    r = R.pointwise_eval(logits, off, sem, lab)
    assert (r["tp"], r["fp"], r["tn"], r["fn"], r["n_off"]) == (2, 1, 1, 1, 3)
    assert r["acc"] == pytest.approx(0.6) and r["offset_mae"] == pytest.approx((5.0 + 0.0 + 3.0) / 3)
    r = R.pointwise_eval(logits, off, torch.ones(5, dtype=torch.long), lab)
    assert r["n_off"] == 0 and r["offset_mae"] == 0.0


def test_batchnorm_entry_points_refuse_bad_views_before_any_launch():
    """Contracts checked on the host, so no GPU is needed: the wrappers refuse an operand with a column stride (a transposed view would be
    read as if its columns were adjacent), and the C entry points refuse ld % 4, C % 4 and C > 1024 before they launch anything."""
    from treelearn_amd import _hip, ops
    x = torch.zeros((40, 32)); xt = torch.zeros((32, 40)).t(); wide = torch.zeros((40, 64))[:, ::2]
    gamma = torch.ones(32); st = torch.zeros((4, 32)); parts = torch.zeros((4, 2, 32), dtype=torch.float64)
    for bad in (xt, wide):
        with pytest.raises(ValueError):
            ops.bn_train_stats(bad, gamma, gamma, 1e-4, 0.1)
        with pytest.raises(ValueError):
            ops.bn_train_bwd(bad, x, st, True)
        with pytest.raises(ValueError):
            ops.bn_train_bwd(x, bad, st, True)
        with pytest.raises(ValueError):
            ops.bn_train_bwd(x, x, st, True, dx_add=bad)
        with pytest.raises(ValueError):
            ops.bn_train_bwd_from_parts(bad, x, st, parts, 4)
        with pytest.raises(ValueError):
            ops.bn_train_bwd_from_parts(x, bad, st, parts, 4)
        with pytest.raises(ValueError):
            ops.bn_train_bwd_from_parts(x, x, st, parts, 4, dx_add=bad)
        with pytest.raises(ValueError):
            ops.bn_train_bwd_from_parts(x, x, st, parts, 4, dx=bad)
        with pytest.raises(ValueError):
            ops.column_sum(bad)
    lib = _hip.lib()
    buf = (ctypes.c_double * 8192)()
    p = ctypes.addressof(buf)
    stats = lambda ld, n, C: lib.tl_bn_train_stats(p, ld, n, C, _hip.TL_F32, p, p, 1e-4, 0.1, p, p, p, p, p, None, None, None, None)      # noqa: E731
    bwd = lambda ld, dld, xld, ald, C: lib.tl_bn_train_bwd(p, ld, _hip.TL_F32, p, dld, _hip.TL_F32, 16, C, p, p, p, p, 1, p, p, p, p, xld,       # noqa: E731
                                                           p if ald else None, ald, None)
    assert stats(10, 16, 8) == _hip.TL_ERR_ARG and stats(8, 16, 6) == _hip.TL_ERR_ARG and stats(1028, 16, 1028) == _hip.TL_ERR_ARG
    assert stats(8, 0, 8) == _hip.TL_ERR_ARG
    assert bwd(10, 8, 8, 0, 8) == _hip.TL_ERR_ARG and bwd(8, 10, 8, 0, 8) == _hip.TL_ERR_ARG and bwd(8, 8, 10, 0, 8) == _hip.TL_ERR_ARG
    assert bwd(8, 8, 8, 10, 8) == _hip.TL_ERR_ARG and bwd(8, 8, 8, 0, 6) == _hip.TL_ERR_ARG and bwd(1028, 1028, 1028, 0, 1028) == _hip.TL_ERR_ARG
    assert lib.tl_bn_ws_doubles(16, 6) == 0 and lib.tl_bn_ws_doubles(16, 1028) == 0 and lib.tl_bn_ws_doubles(16, 8) == 16
    # mixed 16-bit types: one 16-bit type per call
    assert lib.tl_bn_train_bwd(p, 8, _hip.TL_BF16, p, 8, _hip.TL_F16, 16, 8, p, p, p, p, 1, p, p, p, p, 8, None, 0, None) == _hip.TL_ERR_ARG
    assert lib.tl_bn_train_bwd(p, 8, _hip.TL_F16, p, 8, _hip.TL_BF16, 16, 8, p, p, p, p, 1, p, p, p, p, 8, None, 0, None) == _hip.TL_ERR_ARG


def test_weight_gradient_cases_have_an_exact_fp32_answer():
    """tests/wgrad_cases.py, every generator at its smallest size: present pairs per tap stay under the cap, the float64 reference of Set A is a
    multiple of 1/64, survives the round trip through fp32 and equals an integer recomputation; the special and one-pair tables hold what they
    say; Set B's values are representable in their 16-bit type and one product of them is exact in fp32."""
    import numpy as np
    import wgrad_cases as C
    for name, x, g, t, K in C.smallest_cases():
        if t is not None:
            assert t.dtype == np.int32 and t.shape == (K, g.shape[0]) and int((t >= 0).sum(1).max()) <= C.PAIR_CAP, name
            assert t.min() >= -1 and t.max() < x.shape[0], name
        ref = C.reference(x, g, t, K)
        assert np.array_equal(ref * 64, np.rint(ref * 64)), name
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), name
        assert np.array_equal(ref * 64, C.reference_int64(x, g, t, K).astype(np.float64)), name
        assert np.abs(ref).max() > 0, name
    rng = np.random.default_rng(3)
    t = C.special_table(rng, 27, 300, 350)
    cnt = (t >= 0).sum(1)
    assert cnt[0] == 0 and cnt[1] == 300 and np.array_equal(t[1], np.arange(300))
    assert cnt[2] == 1 and t[2, 299] == 349 and cnt[3] == 1 and t[3, 0] == 0
    assert cnt[4] == 300 and len(np.unique(t[4])) == 1
    assert [int(c) for c in cnt[5:8]] == [15, 16, 17] and (t[5:8, 64:] == -1).all()
    assert [int(c) for c in cnt[24:27]] == [1, 1, 1] and t[25, 299] == 0 and t[26, 0] == 349
    assert 0 < cnt[8] < 300
    assert (C.special_table(rng, 8, 1, 51) >= 0).sum(1).tolist() == [0, 1, 1, 1, 1, 1, 1, 1]           # one output row: what K and n_out allow
    for n_out, tiles in ((1, (64,)), (20, (16, 64)), (5000, (64, 128, 256, 4096))):
        t = C.one_pair_table(rng, 27, n_out, n_out + 50, tiles)
        assert ((t >= 0).sum(1) == 1).all()
        rows = [int(np.flatnonzero(t[k] >= 0)[0]) for k in range(27)]
        assert rows[0] == 0 and rows[1] == n_out - 1 and t[0, 0] == 0 and t[1, n_out - 1] == n_out + 49
        if n_out >= 27:
            assert len(set(rows)) == 27
    assert {63, 64, 127, 128, 255, 256, 4095, 4096} <= set(rows)
    for dt, bits in (("bf16", 8), ("f16", 11)):
        v = C.mantissa(rng, (64, 8), dt)
        assert np.array_equal(C.round_to(v, dt), v) and np.abs(v).min() >= 2.0 ** -4 and np.abs(v).max() <= 2.0 ** 4
        m, _ = np.frexp(v.astype(np.float64))
        assert np.array_equal(m * 2 ** bits, np.rint(m * 2 ** bits))                                    # `bits` significant bits
        p = v[:32].astype(np.float64) * v[32:].astype(np.float64)
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    assert np.array_equal(C.round_to(np.array([1.00390625, 1.01171875], np.float32), "bf16"), np.array([1.0, 1.015625], np.float32))   # ties to even, both ways
    a = np.concatenate([rng.normal(size=4096) * 10.0 ** rng.integers(-30, 30, size=4096), [-3.0e38, 1e-40, 0.0]]).astype(np.float32)
    assert np.array_equal(C.round_to(a, "bf16"), torch.from_numpy(a).bfloat16().float().numpy())
    # the case lists hold every value the kernels' constants ask for
    tiles = lambda c: 1 if c <= 32 else (3 if 64 < c <= 96 else 2)                                       # noqa: E731
    seen = {}
    for ci, co, K, n, _ in C.GENERIC:
        seen.setdefault((tiles(co), tiles(ci)), set()).add(n)
    assert len(seen) == 9 and all(len(v) >= 2 for v in seen.values())
    assert {c[3] for c in C.GENERIC} == {1, 2, 63, 64, 65, 4095, 4096, 4097, 16384, 16385} and {c[2] for c in C.GENERIC} == {1, 8, 27}
    assert C.dense_rows(64, 64) == [1, 63, 64, 65, 511, 513, 88 * 64 + 1, 136 * 64 + 1] and C.dense_rows(96, 96)[-1] == 48 * 128 + 1


def test_weight_gradient_tuning_keys_reach_the_f16_compilation():
    """The weight-gradient units are compiled twice (bf16 and IEEE half).  tl_set_tuning and tl_conv_wgrad_ws_floats belong to the first compilation;
    the half launchers must see the same keys, or a workspace sized under wgrad_dense = 0 / wgrad_rows = 0 / wgrad_dma = 2 / wgrad_dense_min_rows is
    too small for what the half kernels write (96 -> 96, 100 001 rows, wgrad_dense = 0: 28 partial sets allocated, 40 written)."""
    import wgrad_cases as C
    from treelearn_amd import _hip
    L = _hip.lib()
    f16 = L.tl_conv_wgrad_ws_floats_f16
    f16.restype, f16.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    shapes = [(100001, 27, 96, 96), (100000, 27, 192, 96), (70000, 27, 64, 64), (61000, 27, 128, 64), (30000, 1, 32, 32), (50001, 27, 4, 32), (500, 27, 64, 64)]
    sizes = set()
    try:
        for keys in ({}, dict(wgrad_dense=0), dict(wgrad_rows=0), dict(wgrad_dma=0), dict(wgrad_dma=2), dict(wgrad_dense_min_rows=1)):
            for k, v in {**C.KNOB_DEFAULTS, **keys}.items():
                assert L.tl_set_tuning(k.encode(), v) == 0
            got = tuple(int(L.tl_conv_wgrad_ws_floats(*s)) for s in shapes)
            assert got == tuple(int(f16(*s)) for s in shapes), keys
            sizes.add(got)
    finally:
        for k, v in C.KNOB_DEFAULTS.items():
            L.tl_set_tuning(k.encode(), v)
    assert len(sizes) == 5                                          # every key moves some size (wgrad_dma = 0 keeps the slot counts)
    per = 27 * 96 * 96
    assert L.tl_conv_wgrad_ws_floats(100001, 27, 96, 96) == 40 * per and f16(100001, 27, 96, 96) == 40 * per
