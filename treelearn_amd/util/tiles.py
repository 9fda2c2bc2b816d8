"""Device-resident inference tiling -- SURVEY.md 8f #3.

Mirrors, for the pipeline's configuration (plot_corners=None; tile denoising by util/outlier.py when its config keys are set), the chain
  SampleGenerator.tile_generate_and_save  (reference tree_learn/util/data_preparation.py:333-494)
  -> <plot>_<i>.npz -> TreeDataset.__getitem__ (test mode) -> collate_fn, batch size 1
     (tree_learn/dataset/dataset.py:34-76,167-226)
without the npz round trip: the voxelised plot stays in HBM, every tile is one `tl_tile_crop` call (box test,
stable compaction, centring, labels and masks fused), and the batch dict handed to the tile loop
(`util/pipeline.get_pointwise_preds`) holds device tensors.  Tile order, tile skipping (no point inside the inner
square) and every dtype decision are the reference's (golden G11).

Offset labels (dataset.py:111-140) depend on numpy's `np.partition(z, 10)[3]` -- an implementation-defined element
among the ten lowest points -- and on float32 summation order, so for bit-identical labels they are derived on the
host from the cropped tile exactly as the reference's DataLoader worker does (`offset_labels="host"`, the default).
`offset_labels="device"` derives them on the device instead (tl_train_item in test mode): the tree base starts at the 4th
smallest z by definition and is an exact sum, so the labels agree with the host's to float32 rounding wherever numpy's pick is that
element, and nothing is copied to the host.
Pure inference does not use them (`get_instances` reads coordinates, logits, offsets and the verticality
feature only): `offset_labels="none"` skips the D2H copy and returns zeros / an all-false `masks_off`.

`write_tiles` is the file form of the same chain, the reference's `generate_tiles` as tools/data_gen/gen_val_data.py calls it for
the validation forest of a training run:

    python -m treelearn_amd.util.tiles --forest PATH [--voxel-size V] [--inner-edge I] [--outer-edge O] [--stride S]
"""
import argparse
import ctypes
import json
import os
import os.path as osp
import sys

import numpy as np
import torch

from .. import _hip

IGNORE_LABEL, NON_TREE_LABEL = -1, 0            # raw-data conventions, dataset.py:7-8
NON_TREE_CLASS, TREE_CLASS = 1, 0               # dataset.py:9-10


def tile_grid(x_range, y_range, inner_edge, outer_edge, stride):
    """Inner and outer square extensions, float64 [T,4] = (x0, x1, y0, y1), tiles row-major from the top-left corner
    (data_preparation.py:362-389: the plot is padded by 1.5 outer edges, the inner edge is adapted so that an integer
    number of squares fits, then the squares are laid out every `stride` inner edges).  The plot ranges are float32
    (the voxelised plot is stored as float32) and numpy keeps the whole lay-out arithmetic in float32 -- Python
    floats are weak scalars -- before the result is widened and rounded to 5 decimals; restated the same way here."""
    f32 = np.float32
    lo = [np.round(f32(r[0]) - f32(1.5 * outer_edge), 2) for r in (x_range, y_range)]
    hi = [np.round(f32(r[1]) + f32(1.5 * outer_edge), 2) for r in (x_range, y_range)]
    span = [h - l - f32(2 * outer_edge) for l, h in zip(lo, hi)]
    n_fit = [int(np.round(sp / f32(inner_edge))) for sp in span]
    edge = [np.round(sp / f32(k), 5) for sp, k in zip(span, n_fit)]
    ncols, nrows = (int((k - 1) / stride + 1) for k in n_fit)
    sj = (stride * np.arange(ncols)).astype(f32); sj1 = (stride * np.arange(ncols) + 1).astype(f32)
    si = (stride * np.arange(nrows)).astype(f32); si1 = (stride * np.arange(nrows) + 1).astype(f32)
    left = lo[0] + f32(outer_edge); top = hi[1] - f32(outer_edge)
    x0 = left + sj * edge[0]; x1 = left + sj1 * edge[0]
    y0 = top - si1 * edge[1]; y1 = top - si * edge[1]
    inner = np.stack([np.tile(x0, nrows), np.tile(x1, nrows), np.repeat(y0, ncols), np.repeat(y1, ncols)], axis=1).astype(np.float64)
    inner = np.round(inner, 5)
    outer = inner + np.array([-outer_edge, outer_edge, -outer_edge, outer_edge])
    return inner, outer


def _offset_labels_host(xyz, inst, sem):
    """dataset.py:111-140 on the cropped tile (numpy, as in the reference's DataLoader worker)."""
    position = np.ones_like(xyz, dtype=np.float32)
    valid = np.zeros(len(xyz), dtype=bool)
    order = np.argsort(inst, kind="stable")
    bounds = np.flatnonzero(np.diff(inst[order])) + 1
    for sel in np.split(order, bounds):
        if sem[sel[0]] == NON_TREE_CLASS:
            continue
        pts = xyz[sel]; z = pts[:, 2]
        low = np.partition(z, 10)[3] if len(z) > 11 else z.min()
        base_pts = pts[z <= low + 0.5]
        if len(base_pts):
            position[sel] = np.mean(base_pts, axis=0); valid[sel] = True
        else:
            position[sel] = 0.0
    return position - xyz, valid


class PlotTiler:
    """Holds the voxelised plot (points f32[N,3], labels f32[N], features f32[N,F]) on the device and yields the
    reference's inference tiles as batch dicts."""

    def __init__(self, points, labels, feats, device="cuda"):
        as_t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        self.xyz = as_t(points); self.labels = as_t(labels).reshape(-1); self.feats = as_t(feats).reshape(len(self.xyz), -1)
        assert self.xyz.is_cuda, "PlotTiler needs the HIP library and a GPU"
        n = len(self.xyz)
        mn = self.xyz[:, :2].amin(0).cpu().numpy(); mx = self.xyz[:, :2].amax(0).cpu().numpy()      # get_ranges, data_preparation.py:497-508
        self.x_range, self.y_range = (mn[0], mx[0]), (mn[1], mx[1])
        F = self.feats.shape[1]; dev = self.xyz.device
        L = _hip.lib()
        self._ws = torch.empty(int(L.tl_tile_crop_ws_words(n)), dtype=torch.int32, device=dev)
        self._count = torch.empty(2, dtype=torch.int32, device=dev)
        self._stream = torch.cuda.Stream(device=dev)        # crops run beside the consumer's forward passes, not behind them
        self._buf = dict(coords=torch.empty((n, 3), dtype=torch.float32, device=dev), feats=torch.empty((n, max(F, 1)), dtype=torch.float32, device=dev),
                         inst=torch.empty(n, dtype=torch.int64, device=dev), sem=torch.empty(n, dtype=torch.int64, device=dev),
                         m_inner=torch.empty(n, dtype=torch.uint8, device=dev), m_sem=torch.empty(n, dtype=torch.uint8, device=dev))

    def crop(self, inner, outer, inner_square_edge_length, sample_generator=None):
        """One tile: (kept rows, rows in the inner square, centre f64[3]); the rows are in self._buf[...][:kept].
        `sample_generator` (the config section, or what outlier.active_filters returned): the outlier filters of
        data_preparation.py:446-454 on the cropped, centred f32 coordinates; every per-row buffer is compacted with the one mask.
        The inner-square count is the unfiltered one: the reference decides about an empty tile (:413-431) before it filters."""
        box = _hip.TileBox()
        i32 = inner.astype(np.float32)
        cx = np.round((i32[0] + i32[1]) / 2, 6); cy = np.round((i32[2] + i32[3]) / 2, 6)          # float32 arithmetic, data_preparation.py:431-434
        box.outer[:] = [float(v) for v in outer.astype(np.float32)]
        box.inner[:] = [float(v) for v in inner]
        box.center[:] = [float(cx), float(cy)]
        box.half_inner = float(inner_square_edge_length) / 2
        b = self._buf; F = self.feats.shape[1]
        _hip.check(_hip.lib().tl_tile_crop(_hip.ptr(self.xyz), _hip.ptr(self.labels), _hip.ptr(self.feats), len(self.xyz), F, ctypes.byref(box),
                                           _hip.ptr(b["coords"]), _hip.ptr(b["feats"]), _hip.ptr(b["inst"]), _hip.ptr(b["sem"]),
                                           _hip.ptr(b["m_inner"]), _hip.ptr(b["m_sem"]), _hip.ptr(self._count), _hip.ptr(self._ws), _hip.stream()),
                   "tl_tile_crop")
        kept, n_inner = (int(v) for v in self._count.cpu())
        if sample_generator is not None and kept > 0:
            from . import outlier
            filters = outlier.active_filters(sample_generator)
            if filters["sor"] is not None or filters["rad"] is not None:
                rows = outlier.denoise(b["coords"][:kept], filters).nonzero().squeeze(1)
                for buf in b.values():
                    buf[:len(rows)] = buf[:kept].index_select(0, rows)
                kept = len(rows)
        return kept, n_inner, np.array([float(cx), float(cy), 0.0])

    def tiles(self, inner_edge, outer_edge, stride, inner_square_edge_length, offset_labels="host", sample_generator=None):
        """Generator of batch dicts (collate_fn's keys, batch size 1), in the reference's tile numbering.  `sample_generator`: the config
        section whose complete pairs switch the outlier filters on (util/outlier.py); the numbering and the skipping of tiles do not change."""
        assert offset_labels in ("host", "none", "device")
        if sample_generator is not None:
            from .outlier import active_filters
            sample_generator = active_filters(sample_generator)
        inner, outer = tile_grid(self.x_range, self.y_range, inner_edge, outer_edge, stride)
        F = self.feats.shape[1]
        main = torch.cuda.current_stream()
        self._stream.wait_stream(main)                         # the plot arrays may have just been produced on the caller's stream
        for t in range(len(inner)):                            # (one wait for the whole generator: a per-tile wait would put every crop behind the consumer's previous forward)
            batch = self.tile_batch(inner[t], outer[t], inner_square_edge_length, offset_labels, tile_index=t, sync_with_caller=False,
                                    sample_generator=sample_generator)
            if batch is not None:
                yield batch

    def tile_batch(self, inner, outer, inner_square_edge_length, offset_labels="host", tile_index=0, sync_with_caller=True,
                   sample_generator=None):
        """ONE tile as a batch dict (collate_fn's keys, batch size 1) from its inner / outer square (x0, x1, y0, y1), or None when the inner
        square holds no point (data_preparation.py:412-427).  Random access for callers that own only some tiles of a plot (a rank of the
        sharded tile loop) or lay the squares out themselves.  `sync_with_caller=False`: the caller has already made the tiler's stream wait
        for whatever produced the plot arrays (`tiles()` does so once) -- the crop then does not queue behind the caller's stream."""
        assert offset_labels in ("host", "none", "device")
        F = self.feats.shape[1]
        main = torch.cuda.current_stream()
        if sync_with_caller:
            self._stream.wait_stream(main)                     # the plot arrays may have just been produced on the caller's stream
        t = tile_index
        # The crop (and its one host sync for the row count) goes on the tiler's own stream: a consumer that pulls the next
        # tile before launching the current forward (util/pipeline.get_pointwise_preds) then never waits for its own convs.
        with torch.cuda.stream(self._stream):
            kept, n_inner, center = self.crop(np.asarray(inner, np.float64), np.asarray(outer, np.float64), inner_square_edge_length, sample_generator)
            if n_inner == 0:                               # data_preparation.py:412-427: tiles whose inner square is empty are dropped
                return None
            b = self._buf
            if offset_labels == "device":
                batch = self._device_batch(kept, center, inner_square_edge_length, t)
                ready = torch.cuda.Event(); ready.record(self._stream)
        if offset_labels == "device":
            for v in batch.values():
                if torch.is_tensor(v):
                    v.record_stream(main)
            batch["_ready_event"] = ready
            return batch
        with torch.cuda.stream(self._stream):
            coords = b["coords"][:kept].clone(); inst = b["inst"][:kept].clone(); sem = b["sem"][:kept].clone()
            m_inner = b["m_inner"][:kept].bool(); m_sem = b["m_sem"][:kept].bool()
            if offset_labels == "host":
                off, valid = _offset_labels_host(coords.cpu().numpy(), inst.cpu().numpy(), sem.cpu().numpy())
                off_t = torch.from_numpy(off.astype(np.float32)).to(coords.device)
                m_off = m_sem & (sem != NON_TREE_CLASS) & torch.from_numpy(valid).to(coords.device)
            else:
                off_t = torch.zeros_like(coords); m_off = torch.zeros_like(m_sem)
            c32 = torch.from_numpy(center.astype(np.float32)).to(coords.device)
            batch = dict(coords=coords, input_feats=b["feats"][:kept, :F].clone(), batch_ids=torch.zeros(kept, dtype=torch.int64, device=coords.device),
                         semantic_labels=sem, instance_labels=inst, masks_inner=m_inner, masks_off=m_off, masks_sem=m_sem,
                         offset_labels=off_t, batch_size=1, centers=c32.expand(kept, 3).contiguous(), tile_index=t)
            ready = torch.cuda.Event(); ready.record(self._stream)
        for v in batch.values():
            if torch.is_tensor(v):
                v.record_stream(main)                      # allocated on the tiler's stream, consumed on the caller's
        batch["_ready_event"] = ready                      # consumers on another stream wait for this before reading the tile
        return batch


    def _device_batch(self, kept, center, inner_square_edge_length, tile_index):
        """`offset_labels="device"`: the batch of the cropped rows from one tl_train_item call in test mode (labels, masks and offset labels by
        the device rule of include/treelearn_hip.h: rank 3 for the tree base, an exact sum), nothing copied to the host."""
        from .device_dataset import ItemWorkspace, alloc_batch, train_item
        b = self._buf; F = self.feats.shape[1]; dev = self.xyz.device
        if getattr(self, "_item_ws", None) is None:
            self._item_ws = ItemWorkspace(dev)
        out = alloc_batch(kept, F, dev)
        out["input_feats"].copy_(b["feats"][:kept, :F])
        train_item(b["coords"][:kept], b["inst"][:kept].to(torch.int32), out, 0, float(inner_square_edge_length) / 2, self._item_ws,
                   center=center.astype(np.float32))
        out["batch_size"] = 1
        out["tile_index"] = tile_index
        return out


# ------------------------------------------------------------------------------------------------ validation tiles on disk
# configs/data_gen/gen_val_data.yaml over configs/_modular/sample_generation.yaml of the reference (stride 1: tiles do not overlap)
VAL_CFG = dict(voxel_size=0.1, search_radius_features=0.6, inner_edge=8, outer_edge=13.5, stride=1, feature_names=["verticality"],
               sample_generator=dict(n_neigh_sor=None, multiplier_sor=None, rad=None, npoints_rad=None))
_FILTER_KEYS = ("n_neigh_sor", "multiplier_sor", "rad", "npoints_rad")


def write_tiles(forest_path, sample_cfg=None, logger=None):
    """`generate_tiles` (tree_learn/util/pipeline.py:24-75) + `tile_generate_and_save` (data_preparation.py:333-494, plot_corners=None) for
    a labelled forest <base>/<dir>/<plot>.<ext>: writes <base>/forest_voxelized<v>/<plot>.npz (points, labels) and
    <base>/features/<plot>.npz (features) unless they exist -- the cache files util/crops.py writes for training forests -- then one
    <base>/tiles/npz/<plot>_<i>.npz (points f32 centred on the tile, feat f32, instance_label i32, center f64[3]) and
    <base>/tiles/json/<plot>_<i>.json per tile whose inner square holds a point, i counting those tiles.  `CropDataset(<base>/tiles/npz,
    inner_square_edge_length, training=False)` reads them.  Returns the number of tiles written."""
    from .features import check_feature_names, load_feature_cache, save_feature_cache
    from .prepare import compute_features, voxelize
    from .segment import load_forest
    cfg = dict(VAL_CFG, **{k: v for k, v in dict(sample_cfg or {}).items()})
    names = check_feature_names(cfg["feature_names"], for_model=True)         # before anything is written
    gen = dict(VAL_CFG["sample_generator"], **dict(cfg.get("sample_generator") or {}))
    from .outlier import active_filters
    filters = active_filters({k: gen.get(k) for k in _FILTER_KEYS})          # a half-set pair is refused here, before anything is written
    say = (lambda m: logger.info(m)) if logger is not None else (lambda m: None)
    plot_name = osp.basename(forest_path)[:-4]
    base_dir = osp.dirname(osp.dirname(osp.abspath(forest_path)))
    voxelized_dir = osp.join(base_dir, f"forest_voxelized{cfg['voxel_size']}")
    features_dir = osp.join(base_dir, "features")
    save_dir = osp.join(base_dir, "tiles")
    for d in (voxelized_dir, features_dir, osp.join(save_dir, "npz"), osp.join(save_dir, "json")):
        os.makedirs(d, exist_ok=True)

    say("voxelizing forest...")
    path_vox = osp.join(voxelized_dir, f"{plot_name}.npz")
    if not osp.exists(path_vox):
        data = load_forest(forest_path)
        if data.shape[1] == 3:                                                    # load_data: unlabelled clouds get -1
            data = np.hstack([data, IGNORE_LABEL * np.ones(len(data))[:, np.newaxis]])
        vox, _ = voxelize(data, cfg["voxel_size"])
        vox = np.round(vox.cpu().numpy().astype(np.float32), 2)
        np.savez_compressed(path_vox, points=vox[:, :3], labels=vox[:, 3])
    say("calculating features...")
    path_feat = osp.join(features_dir, f"{plot_name}.npz")
    if not osp.exists(path_feat):
        pts = np.load(path_vox)["points"]
        feats = compute_features(pts.astype(np.float64), search_radius=cfg["search_radius_features"], feature_names=names)
        save_feature_cache(path_feat, feats.cpu().numpy(), names)

    say("getting tiles...")
    d = np.load(path_vox)
    feats = load_feature_cache(path_feat, names)                              # ValueError: a cache written for another list
    tiler = PlotTiler(d["points"], d["labels"], feats)
    inner, outer = tile_grid(tiler.x_range, tiler.y_range, cfg["inner_edge"], cfg["outer_edge"], cfg["stride"])
    F = tiler.feats.shape[1]
    meta = {"plot_name": plot_name, "n_neigh_sor": gen["n_neigh_sor"], "multiplier_sor": gen["multiplier_sor"], "rad": gen["rad"],
            "npoints_rad": gen["npoints_rad"], "inner_edge": cfg["inner_edge"], "outer_edge": cfg["outer_edge"]}
    i = 0
    for t in range(len(inner)):
        # the masks the crop also fills are not stored (the dataset derives them from the points), so their edge length does not matter here
        kept, n_inner, center = tiler.crop(inner[t], outer[t], cfg["inner_edge"], filters)
        if n_inner == 0:
            continue
        b = tiler._buf
        data = dict(points=b["coords"][:kept].cpu().numpy(), feat=b["feats"][:kept, :F].cpu().numpy(),
                    instance_label=b["inst"][:kept].cpu().numpy().astype(np.int32), center=center)
        np.savez(osp.join(save_dir, "npz", f"{plot_name}_{i}.npz"), **data)
        with open(osp.join(save_dir, "json", f"{plot_name}_{i}.json"), "w") as f:
            json.dump(meta, f)
        i += 1
    return i


def parse_args(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.tiles", description="write the validation tiles of a labelled forest")
    ap.add_argument("--forest", required=True, help="labelled cloud <base>/<dir>/<plot>.npy|npz|txt|las, N x 4; tiles go to <base>/tiles")
    ap.add_argument("--voxel-size", type=float, default=VAL_CFG["voxel_size"])
    ap.add_argument("--search-radius-features", type=float, default=VAL_CFG["search_radius_features"])
    ap.add_argument("--inner-edge", type=float, default=VAL_CFG["inner_edge"])
    ap.add_argument("--outer-edge", type=float, default=VAL_CFG["outer_edge"])
    ap.add_argument("--stride", type=float, default=VAL_CFG["stride"])
    ap.add_argument("--n-neigh-sor", type=int, default=None, help="statistical outlier filter on every tile: neighbours (with --multiplier-sor)")
    ap.add_argument("--multiplier-sor", type=float, default=None, help="statistical outlier filter: standard-deviation ratio")
    ap.add_argument("--rad", type=float, default=None, help="radius outlier filter on every tile: radius in metres (with --npoints-rad)")
    ap.add_argument("--npoints-rad", type=int, default=None, help="radius outlier filter: a point is kept with more than this many points in the ball")
    ap.add_argument("--feature-names", nargs="+", default=list(VAL_CFG["feature_names"]),
                    help="point features of the tiles (util/features.py), at most 5, verticality last")
    a = ap.parse_args(argv)
    for k in ("voxel_size", "search_radius_features", "inner_edge", "outer_edge", "stride"):
        if not getattr(a, k) > 0:
            ap.error(f"--{k.replace('_', '-')} must be > 0")
    try:
        from .features import check_feature_names
        check_feature_names(a.feature_names, for_model=True)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    import logging
    a = parse_args(argv)
    if not osp.exists(a.forest):
        print(f"--forest {a.forest}: no such file", file=sys.stderr)
        return 2
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    cfg = dict(voxel_size=a.voxel_size, search_radius_features=a.search_radius_features, inner_edge=a.inner_edge, outer_edge=a.outer_edge,
               stride=a.stride, feature_names=a.feature_names, sample_generator=dict(n_neigh_sor=a.n_neigh_sor, multiplier_sor=a.multiplier_sor, rad=a.rad, npoints_rad=a.npoints_rad))
    try:
        n = write_tiles(a.forest, cfg, logger=logging.getLogger("treelearn_amd.tiles"))
    except NotImplementedError as e:                            # a half-set filter pair
        print(str(e), file=sys.stderr)
        return 2
    print(f"{n} tiles -> {osp.join(osp.dirname(osp.dirname(osp.abspath(a.forest))), 'tiles')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
