"""Segment a whole forest: the reference's `run_treelearn_pipeline` (tools/pipeline/pipeline.py:21-199) on the device, from one cloud
to a segmented forest and one file per tree.

    python -m treelearn_amd.util.segment --forest F.npy|npz|txt|las --weights model.pth --out DIR [...]

  segment_forest         <- pipeline.py:40-187 (centre, plot preparation, tile loop, ensemble, grouping, k-NN fill, then below)
  segment_from_pointwise <- pipeline.py:78-81,133-187 (outer-buffer removal, edge-tree categories, predictions back to the input cloud)
  save_results           <- pipeline.py:96-131,189-199 and util/pipeline.py:339-420 (save_data, save_treewise)

Everything between the stages stays on the device; the results cross PCIe once at the end."""
import argparse
import os
import sys

import numpy as np
import torch

from . import hull as _hull
from .pipeline import get_instances_device, get_pointwise_preds
from .postprocess import assign_remaining_points_nearest_neighbor_device, ensemble, knn_vote
from .prepare import compute_features, voxelize
from .tiles import PlotTiler

TREE_CLASS_IN_PYTORCH_DATASET = 0
NON_TREES_LABEL_IN_GROUPING = 0
NOT_ASSIGNED_LABEL_IN_GROUPING = -1
START_NUM_PREDS = 1
RETURN_TYPES = ("original", "voxelized", "voxelized_and_filtered")
SAVE_FORMATS = ("npz", "npy", "txt", "las", "laz")
CATEGORIES = ("completely_inside", "trunk_base_inside", "trunk_base_outside")

# configs/pipeline/pipeline.yaml + configs/_modular/{sample_generation,grouping,model}.yaml of the reference
SAMPLE_CFG = dict(voxel_size=0.1, search_radius_features=0.6, inner_edge=8.0, outer_edge=13.5, stride=0.5, feature_names=["verticality"])
GROUPING_CFG = dict(tree_conf_thresh=0.5, tau_vert=0.6, tau_off=4.0, tau_group=0.15, tau_min=50, use_hdbscan=True)
SHAPE_CFG = dict(outer_remove=None, alpha=0.6, buffer_size_to_determine_edge_trees=0.3)
MODEL_CFG = dict(channels=32, num_blocks=7, kernel_size=3, use_feats=False, use_coords=False, dim_coord=3, dim_feat=1,
                 max_num_points_per_voxel=3, spatial_shape=[500, 500, 1000], voxel_size=0.1)


def _get(cfg, k, default=None):
    if isinstance(cfg, dict):
        return cfg.get(k, default)
    return getattr(cfg, k, default)


def _log(logger, msg):
    if logger is not None:
        logger.info(msg)


def _consecutive(labels, start_num):
    """make_labels_consecutive on the device: rank among the distinct labels + start_num."""
    palette = torch.unique(labels)
    return torch.searchsorted(palette, labels) + start_num


def _keys(a, b):
    """Integer keys rint(x * 100) of two float32 [n, 3] arrays (as `ensemble` builds them), packed into one i64 per row on a shared base."""
    qa, qb = torch.round(a.float() * 100.0).to(torch.int64), torch.round(b.float() * 100.0).to(torch.int64)
    lo = torch.minimum(qa.min(0).values if len(qa) else qb.min(0).values, qb.min(0).values if len(qb) else qa.min(0).values)
    ra, rb = qa - lo, qb - lo
    span = torch.maximum(ra.max(0).values if len(ra) else rb.max(0).values, rb.max(0).values if len(rb) else ra.max(0).values) + 1
    if float(span.double().prod()) >= 2.0 ** 62:
        raise ValueError("coordinate span too large for packed 0.01 m keys")
    pack = lambda r: (r[:, 0] * span[1] + r[:, 1]) * span[2] + r[:, 2]          # noqa: E731
    return pack(ra), pack(rb)


def match_rows(coords, preds, targets, last_target_only):
    """Predictions of `coords` rows carried to `targets` rows whose 2-decimal float32 coordinates are equal (device; -1 / unmatched
    elsewhere).  A later `coords` row overrides an earlier one of the same key.  last_target_only=True: among targets of equal key only
    the last takes the prediction -- propagate_preds_hash_full's dictionary voxel -> original points (util/pipeline.py:423-452);
    False: every target of the key does -- propagate_preds_hash_vox (:455-465)."""
    dev = targets.device
    out = torch.full((len(targets),), -1, dtype=torch.int64, device=dev)
    if len(coords) == 0 or len(targets) == 0:
        return out, torch.ones(len(targets), dtype=torch.bool, device=dev)
    ks, kt = _keys(coords, targets)
    sk, sp = torch.sort(ks, stable=True)
    last = torch.ones_like(sk, dtype=torch.bool)
    last[:-1] = sk[:-1] != sk[1:]
    uk, up = sk[last], preds.index_select(0, sp[last])          # the last row of every key
    pos = torch.searchsorted(uk, kt).clamp_max(len(uk) - 1)
    hit = uk[pos] == kt
    if last_target_only:
        st, tp = torch.sort(kt, stable=True)
        tlast = torch.ones_like(st, dtype=torch.bool)
        tlast[:-1] = st[:-1] != st[1:]
        is_last = torch.zeros_like(hit)
        is_last[tp] = tlast
        hit = hit & is_last
    out[hit] = up[pos[hit]]
    return out, ~hit


def segment_from_pointwise(coords, offset_predictions, instance_preds, shape_cfg, return_type="original", trace=None, voxels=None,
                           points=None, logger=None):
    """Steps after grouping (pipeline.py:78-81,133-187) on device tensors: ensembled coords f32 [M, 3] (centred), offsets f32 [M, 3],
    instance ids i64 [M] (0 = non-tree, trees from 1, after the k-NN fill).  return_type "original" needs `trace` (prepare.voxelize),
    `voxels` (its f32 [V, 3] coordinates) and `points` (the centred input f64 [N, 3]); "voxelized" needs `voxels`.
    Returns a dict of device tensors: coords (f64, still centred), labels, categories (per tree 1..T: index into CATEGORIES),
    mask_inner (of the ensembled rows), instance_preds (after the removal), and the three shapes."""
    if return_type not in RETURN_TYPES:
        raise ValueError(f"return_type must be one of {RETURN_TYPES}, got {return_type!r}")
    alpha = float(_get(shape_cfg, "alpha", 0.6))
    outer_remove = _get(shape_cfg, "outer_remove", None)
    edge = float(_get(shape_cfg, "buffer_size_to_determine_edge_trees", 0.3))
    coords, off, inst = coords.float(), offset_predictions.float(), instance_preds.to(torch.int64).clone()
    out = {}
    mask_inner = None
    if outer_remove:
        _log(logger, "removing outer points")
        hbl = _hull.get_hull_buffer(coords[:, :2], alpha, float(outer_remove))
        mask_inner = ~_hull.get_coords_within_shape(coords, hbl)
        coords, off, inst = coords[mask_inner], off[mask_inner], inst[mask_inner]
        tree = inst != NON_TREES_LABEL_IN_GROUPING
        inst[tree] = _consecutive(inst[tree], START_NUM_PREDS)
        out["hull_buffer_large"] = hbl
    out["mask_inner"] = mask_inner
    out["instance_preds"] = inst
    out["ensemble_coords"] = coords

    # edge-tree categories (pipeline.py:133-156)
    tree = inst != NON_TREES_LABEL_IN_GROUPING
    n_trees = int(inst.max()) if bool(tree.any()) else 0
    means = _hull.get_cluster_means(coords[tree] + off[tree], inst[tree])
    hull = _hull.get_hull(coords[:, :2], alpha)
    within = _hull.get_coords_within_shape(means, hull) if len(means) else torch.zeros(0, dtype=torch.bool, device=coords.device)
    hbs = _hull.get_hull_buffer(coords[:, :2], alpha, edge)
    at_edge = _hull.get_coords_within_shape(coords, hbs)
    edge_ids = torch.unique(inst[at_edge])
    edge_ids = edge_ids[edge_ids != NON_TREES_LABEL_IN_GROUPING]
    not_at_edge = torch.ones(len(means), dtype=torch.bool, device=coords.device)
    not_at_edge[edge_ids - 1] = False
    cat = torch.where(within, torch.where(not_at_edge, 0, 1), 2)
    if len(cat) != n_trees:
        raise RuntimeError(f"tree labels are not consecutive: {len(cat)} means for max label {n_trees}")
    out.update(categories=cat, hull=hull, hull_buffer_small=hbs, cluster_means=means)

    # predictions back to the input cloud (pipeline.py:158-187)
    if return_type == "original":
        vox_pred, vox_miss = match_rows(coords, inst, voxels, last_target_only=True)
        p2v = trace["point2vox"]
        target, pred, miss = points, vox_pred.index_select(0, p2v), vox_miss.index_select(0, p2v)
    elif return_type == "voxelized":
        pred, miss = match_rows(coords, inst, voxels, last_target_only=False)
        target = voxels
    else:
        target, pred, miss = coords, inst.clone(), torch.zeros(len(coords), dtype=torch.bool, device=coords.device)
    if outer_remove:
        keep = ~_hull.get_coords_within_shape(target, out["hull_buffer_large"])
        target, pred, miss = target[keep], pred[keep], miss[keep]
    if bool(miss.any()):
        qi = torch.nonzero(miss).squeeze(1)
        pred[qi] = knn_vote(coords.contiguous(), inst.contiguous(), target.index_select(0, qi).float().contiguous(), 5)
    out.update(coords=target.double(), labels=pred)
    return out


def segment_forest(points, model, sample_cfg=None, grouping_cfg=None, shape_cfg=None, return_type="original", logger=None,
                   return_pointwise=False, inventory=False, inventory_cfg=None, terrain=False, terrain_cfg=None, stem=False, stem_cfg=None,
                   crown=False, crown_cfg=None, canopy=False, canopy_cfg=None, branches=False, branch_cfg=None, wood=False,
                   wood_cfg=None, leafwood=False, leafwood_cfg=None, leafwood_scales=None, leafwood_scales_min=None, preview=False,
                   preview_cfg=None, light=False, light_cfg=None):
    """points: N x 3 or N x 4 (x y z [label]) f64, host or device.  Returns numpy arrays: coords (f64, input frame), labels (i64),
    categories (per tree 1..T, index into CATEGORIES), and with return_pointwise the arrays of pipeline.py:100-111 (ensembled rows).
    inventory=True adds result["inventory"]: util.inventory.tree_inventory of the returned coords / labels, computed on the device in
    the centred frame and un-centred like the coords; inventory_cfg holds any of its five parameters.
    terrain=True adds result["terrain"] (util.terrain: the DTM of the label-0 rows of the returned cloud, computed on the device in the
    centred frame; the un-centred Terrain.to_host()) and result["height_above_ground"] (f64 [N], row-aligned with coords); terrain_cfg
    holds any of its five parameters.  With inventory=True as well, the inventory gets the ground columns.
    stem=True implies inventory=True and adds util.stem's columns and result["inventory"]["stem_profile"] (the circle of every slab along
    every stem); stem_cfg holds any of util.stem's parameters.
    crown=True implies inventory=True and adds util.crown's columns and result["inventory"]["crown_profile"] (rows and cells per layer,
    crown radii per sector); crown_cfg holds any of util.crown's parameters.
    canopy=True implies terrain=True and adds result["canopy"] (util.canopy: the canopy height model, tree tops and grid metrics of the
    returned cloud, from the same height_above_ground; the un-centred Canopy.to_host()) and result["stand"] (util.canopy.stand_summary,
    with the inventory when one is computed); canopy_cfg holds any of util.canopy's parameters.
    branches=True implies inventory=True and adds util.branches' columns and result["inventory"]["skeleton"] (the node table of every
    tree's skeleton; heights from the ground with a terrain, as for the crown); branch_cfg holds any of util.branches' parameters.
    wood=True implies branches=True and adds util.wood's columns and result["inventory"]["cylinders"] (the fitted circle, radius and
    frustum of every skeleton node); wood_cfg holds any of util.wood's parameters.
    leafwood=True implies inventory=True and adds util.leafwood's columns and result["inventory"]["leafwood"] (wood u8 [N], the wood flag
    of every row, row-aligned with coords, and the parameters); leafwood_cfg holds any of util.leafwood's parameters, leafwood_scales and
    leafwood_scales_min the scales of its seed.
    preview=True adds result["preview"]: util.render.render_forest's pictures (name -> u8 [H, W, 3]) of the returned cloud and of
    whatever else was computed, rendered from the arrays still on the device; preview_cfg holds any of util.render's parameters.
    light=True implies terrain=True and adds result["light"] (util.light: the voxel grid and the sensor-grid rasters of openness,
    effective LAI and gap fractions of the returned cloud; the un-centred Light.to_host()) and, with an inventory, util.light's
    LIGHT_COLUMNS after every other column; light_cfg holds any of util.light's parameters.  With preview=True there is one more
    picture, `light`: the openness raster."""
    extra = {}
    if preview:
        from .render import check_params as check_preview, render_forest
        preview_cfg = check_preview(preview_cfg)                                      # before any GPU work
    if branches or wood:
        from .branches import check_params as check_branches
        extra = dict(branches=True, branch_cfg=check_branches(branch_cfg))            # before any GPU work
        inventory = True
    if wood:
        from .wood import check_params as check_wood
        extra.update(wood=True, wood_cfg=check_wood(wood_cfg))                        # before any GPU work
    if leafwood:
        from .leafwood import check_params as check_leafwood, check_scales
        check_scales(scales=leafwood_scales, scales_min=leafwood_scales_min)          # before any GPU work
        extra.update(leafwood=True, leafwood_cfg=check_leafwood(leafwood_cfg), leafwood_scales=leafwood_scales, leafwood_scales_min=leafwood_scales_min)
        inventory = True
    if light:
        from .light import check_params as check_light, light_model
        light_cfg = check_light(light_cfg)                                            # before any GPU work
        terrain = True
    if canopy:
        from .canopy import canopy_model, check_params as check_canopy, stand_summary
        canopy_cfg = check_canopy(canopy_cfg)                                         # before any GPU work
        terrain = True
    if crown:
        from .crown import check_params as check_crown
        crown_cfg = check_crown(crown_cfg)                                            # before any GPU work
        inventory = True
    if stem:
        from .stem import check_params as check_stem
        stem_cfg = check_stem(stem_cfg)                                               # before any GPU work
        inventory = True
    if inventory:
        from .inventory import check_params, tree_inventory
        inventory_cfg = check_params(inventory_cfg)                                   # before any GPU work
    if terrain:
        from .terrain import check_params as check_terrain, terrain_model
        terrain_cfg = check_terrain(terrain_cfg)
    sample_cfg = dict(SAMPLE_CFG, **(sample_cfg or {})) if isinstance(sample_cfg, (dict, type(None))) else sample_cfg
    grouping_cfg = dict(GROUPING_CFG, **(grouping_cfg or {})) if isinstance(grouping_cfg, (dict, type(None))) else grouping_cfg
    shape_cfg = dict(SHAPE_CFG, **(shape_cfg or {})) if isinstance(shape_cfg, (dict, type(None))) else shape_cfg
    if return_type not in RETURN_TYPES:
        raise ValueError(f"return_type must be one of {RETURN_TYPES}, got {return_type!r}")
    from .features import check_feature_names
    feature_names = check_feature_names(_get(sample_cfg, "feature_names", None) or ["verticality"], for_model=True)
    if bool(getattr(model, "use_feats", False)) and int(getattr(model, "dim_feat", len(feature_names))) != len(feature_names):
        raise ValueError(f"the model was built with use_feats=True and dim_feat={model.dim_feat}, but feature_names holds "
                         f"{len(feature_names)} features: {feature_names}")                   # before the tile loop, not the executor's TypeError inside it
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if pts.ndim != 2 or pts.shape[1] not in (3, 4):
        raise ValueError(f"points must be N x 3 or N x 4, got {tuple(pts.shape)}")
    xyz = pts[:, :3].to("cuda", torch.float64)
    mean = xyz.mean(0)
    centred = xyz - mean
    vs = float(_get(sample_cfg, "voxel_size"))
    _log(logger, "voxelizing and computing features")
    down, trace = voxelize(centred, vs)
    vox = down[:, :3].float().contiguous()
    feats = compute_features(vox, float(_get(sample_cfg, "search_radius_features", 0.6)), feature_names)
    tiler = PlotTiler(vox, torch.full((len(vox),), -1.0, device=vox.device), feats)
    inner = float(_get(sample_cfg, "inner_edge"))
    tiles = tiler.tiles(inner, float(_get(sample_cfg, "outer_edge")), float(_get(sample_cfg, "stride")), inner, offset_labels="none",
                        sample_generator=_get(sample_cfg, "sample_generator"))
    _log(logger, "getting pointwise predictions")
    res = get_pointwise_preds(model, tiles, dict(voxel_size=vs), logger, keep_on_device=True)
    if len(res[4]) == 0 or not torch.is_tensor(res[4]):
        raise ValueError("no tile of the plot holds a point")
    _log(logger, "ensembling predictions")
    coords, sem, seml, off, offl, instl, bb, infeat = ensemble(res[4], res[0], res[1], res[2], res[3], res[5], res[6], res[7], return_device=True)
    _log(logger, "getting predicted instances")
    inst = get_instances_device(coords, off, sem, grouping_cfg, infeat[:, -1], TREE_CLASS_IN_PYTORCH_DATASET, NON_TREES_LABEL_IN_GROUPING,
                                NOT_ASSIGNED_LABEL_IN_GROUPING, START_NUM_PREDS)
    initial = inst.clone()
    tree = inst != NON_TREES_LABEL_IN_GROUPING
    if bool((inst[tree] != NOT_ASSIGNED_LABEL_IN_GROUPING).any()):
        inst[tree] = assign_remaining_points_nearest_neighbor_device(coords[tree] + off[tree], inst[tree], NOT_ASSIGNED_LABEL_IN_GROUPING)
    elif bool(tree.any()):            # no cluster survived grouping (the reference's k-NN fit fails on zero samples): no trees
        _log(logger, "no tree cluster found; every point is returned as non-tree")
        inst[tree] = NON_TREES_LABEL_IN_GROUPING
    r = segment_from_pointwise(coords, off, inst, shape_cfg, return_type, trace=trace, voxels=vox, points=centred, logger=logger)
    host = lambda t: t.cpu().numpy()                                                  # noqa: E731
    result = dict(coords=host(r["coords"] + mean), labels=host(r["labels"]), categories=host(r["categories"]))
    dtm = None
    if terrain:
        _log(logger, "computing the terrain model")
        dtm = terrain_model(r["coords"], r["labels"], offset=mean, **terrain_cfg)
        result["terrain"] = dtm.to_host()
        hag = dtm.height_above_ground(r["coords"])
        result["height_above_ground"] = host(hag)
    if inventory:
        _log(logger, "computing the tree inventory")
        result["inventory"] = tree_inventory(r["coords"], r["labels"], offset=mean, terrain=dtm, stem=stem, stem_cfg=stem_cfg if stem else None,
                                             crown=crown, crown_cfg=crown_cfg if crown else None, **extra, **inventory_cfg)
    if canopy:
        _log(logger, "computing the canopy height model")
        result["canopy"] = canopy_model(r["coords"], labels=r["labels"], height_above_ground=hag, offset=mean, **canopy_cfg).to_host()
        result["stand"] = stand_summary(result["canopy"], result.get("inventory"))
    if light:
        _log(logger, "computing the light model")
        lm = light_model(r["coords"], dtm, r["labels"], offset=mean, **light_cfg)
        result["light"] = lm.to_host()
        if inventory:                                                                 # the tree columns from the model's own grid, last
            result["inventory"].update(lm.tree_light(T=len(result["inventory"]["tree_id"])))
    if preview:
        _log(logger, "rendering the previews")
        shown = dict(result, coords=r["coords"], labels=r["labels"])
        if terrain:
            shown["height_above_ground"] = hag
        result["preview"] = {k: host(v) for k, v in render_forest(shown, **preview_cfg).items()}
    if return_pointwise:
        pw = dict(coords=coords, offset_predictions=off, offset_labels=offl, semantic_prediction_logits=sem, semantic_labels=seml,
                  instance_labels=instl, backbone_feats=bb, input_feats=infeat, instance_preds=inst, instance_preds_after_initial_clustering=initial)
        if r["mask_inner"] is not None:
            pw["masks_inner_coords"] = r["mask_inner"]
        result["pointwise"] = {k: host(v) for k, v in pw.items()}
        result["tau_vert"] = float(_get(grouping_cfg, "tau_vert")); result["tau_off"] = float(_get(grouping_cfg, "tau_off"))
    return result


# ------------------------------------------------------------------------------------------------ files
def check_formats(save_formats):
    """Raise before any GPU work if a format is unknown or needs a module that is not installed (laz: laspy; las is written natively)."""
    for f in save_formats:
        if f not in SAVE_FORMATS:
            raise ValueError(f"unknown save format {f!r}; expected one of {SAVE_FORMATS}")
        if f == "laz":
            try:
                import laspy  # noqa: F401
            except ImportError as e:
                raise ImportError(f"save format {f!r} needs the 'laspy' module, which is not installed (use las, npz, npy or txt)") from e


def save_data(data, save_format, save_name, save_folder, use_offset=True):
    """data N x 4 (x y z label) -> save_folder/save_name.<format> (util/pipeline.py:339-392's file contents for npy / npz / txt; las
    through util.las.write_las, encoded on the device, and laz through laspy: point format 3, scale 1 mm, treeID extra dimension,
    classification 2 for label 0 and 4 otherwise)."""
    path = os.path.join(save_folder, f"{save_name}.{save_format}")
    if save_format == "npy":
        np.save(path, data)
    elif save_format == "npz":
        np.savez_compressed(path, points=data[:, :3], labels=data[:, 3])
    elif save_format == "txt":
        np.savetxt(path, data)
    elif save_format == "las":
        from .las import write_las
        write_las(path, data[:, :3], data[:, 3], use_offset=use_offset)
    elif save_format == "laz":
        import laspy
        header = laspy.LasHeader(version="1.2", point_format=3)
        header.offsets = data[:, :3].mean(0) if (use_offset and len(data)) else np.zeros(3)
        header.scales = np.array([0.001, 0.001, 0.001])
        las = laspy.LasData(header)
        las.x, las.y, las.z = data[:, 0], data[:, 1], data[:, 2]
        las.add_extra_dim(laspy.ExtraBytesParams(name="treeID", type=np.uint32))
        las.treeID = data[:, 3].astype(np.uint32)
        las.classification = np.where(data[:, 3] == 0, 2, 4).astype(np.uint8)
        las.write(path)
    else:
        raise ValueError(f"unknown save format {save_format!r}")
    return path


def save_results(result, out_dir, plot_name, save_formats=("npz",), save_treewise=True, save_pointwise=False):
    """The reference's results layout under out_dir: full_forest/<plot_name>.<fmt> for every format; individual_trees/<category>/<id>.<fmt>
    and individual_trees/non_trees.<fmt> (first format; coordinates shifted by the mean of the returned cloud, as save_treewise does);
    pointwise_results/pointwise_results.npz + cluster_coords_initial / cluster_coords (first format) when the result holds them;
    tree_inventory.csv (util.inventory.write_inventory, with the category names) when the result holds an inventory; terrain.npz
    (util.terrain.write_terrain) and height_above_ground.npy when it holds a terrain; stem_profiles.npz (util.stem.write_stem_profiles) when
    the inventory holds stem profiles; crown_profiles.npz (util.crown.write_crown_profiles) when it holds crown profiles; skeletons.npz
    (util.branches.write_skeletons) when it holds "skeleton"; cylinders.npz (util.wood.write_cylinders) when it holds "cylinders"; leafwood.npy
    (util.leafwood.write_leafwood) when it holds "leafwood"; canopy.npz and stand.json
    (util.canopy.write_canopy, write_stand) when the result holds a canopy; light.npz (util.light.write_light) when it holds a light
    model; preview/<name>.png (util.render.write_png) when it holds
    previews."""
    save_formats = list(save_formats)
    check_formats(save_formats)
    coords, labels = np.asarray(result["coords"], np.float64), np.asarray(result["labels"], np.int64)
    full_dir = os.path.join(out_dir, "full_forest")
    os.makedirs(full_dir, exist_ok=True)
    for f in save_formats:
        save_data(np.hstack([coords, labels.reshape(-1, 1)]), f, plot_name, full_dir)
    if save_treewise:
        trees_dir = os.path.join(out_dir, "individual_trees")
        for c in CATEGORIES:
            os.makedirs(os.path.join(trees_dir, c), exist_ok=True)
        c0 = coords - np.mean(coords, axis=0)
        lab = torch.from_numpy(labels)
        if torch.cuda.is_available():
            lab = lab.cuda()
        sl, order = torch.sort(lab, stable=True)                          # one sort instead of a mask per tree
        ids, counts = torch.unique_consecutive(sl, return_counts=True)
        cats = np.asarray(result["categories"])
        ids, counts = ids.cpu().numpy(), counts.cpu().numpy()

        def tree_dir(i):
            """Where label i's file goes, or None for a label without a category."""
            if i == NON_TREES_LABEL_IN_GROUPING:
                return trees_dir
            return os.path.join(trees_dir, CATEGORIES[int(cats[i - 1])]) if 1 <= i <= len(cats) else None

        if save_formats[0] == "las":                                     # one encode in label order: every tree's file body is a byte range of it
            from .las import write_las_segments
            names = [("non_trees" if i == NON_TREES_LABEL_IN_GROUPING else str(int(i)), tree_dir(i)) for i in ids.tolist()]
            write_las_segments([None if d is None else os.path.join(d, f"{n}.las") for n, d in names], c0, lab, order,
                               np.concatenate([[0], np.cumsum(counts)]))
        else:
            order = order.cpu().numpy()
            at = 0
            for i, n in zip(ids.tolist(), counts.tolist()):
                rows = order[at:at + n]; at += n
                d = np.hstack([c0[rows], np.full((n, 1), float(i))])
                if tree_dir(i) is not None:
                    save_data(d, save_formats[0], "non_trees" if i == NON_TREES_LABEL_IN_GROUPING else str(int(i)), tree_dir(i), use_offset=False)
    if "inventory" in result:
        from .inventory import write_inventory
        os.makedirs(out_dir, exist_ok=True)
        write_inventory(os.path.join(out_dir, "tree_inventory.csv"), result["inventory"], categories=result["categories"])
        if "stem_profile" in result["inventory"]:
            from .stem import write_stem_profiles
            write_stem_profiles(os.path.join(out_dir, "stem_profiles.npz"), result["inventory"])
        if "crown_profile" in result["inventory"]:
            from .crown import write_crown_profiles
            write_crown_profiles(os.path.join(out_dir, "crown_profiles.npz"), result["inventory"])
        if "skeleton" in result["inventory"]:
            from .branches import write_skeletons
            write_skeletons(os.path.join(out_dir, "skeletons.npz"), result["inventory"])
        if "cylinders" in result["inventory"]:
            from .wood import write_cylinders
            write_cylinders(os.path.join(out_dir, "cylinders.npz"), result["inventory"])
        if "leafwood" in result["inventory"]:
            from .leafwood import write_leafwood
            write_leafwood(os.path.join(out_dir, "leafwood.npy"), result["inventory"])
    if "terrain" in result:
        from .terrain import write_terrain
        os.makedirs(out_dir, exist_ok=True)
        write_terrain(os.path.join(out_dir, "terrain.npz"), result["terrain"])
        np.save(os.path.join(out_dir, "height_above_ground.npy"), np.asarray(result["height_above_ground"], np.float64))
    if "canopy" in result:
        from .canopy import write_canopy, write_stand
        os.makedirs(out_dir, exist_ok=True)
        write_canopy(os.path.join(out_dir, "canopy.npz"), result["canopy"])
        write_stand(os.path.join(out_dir, "stand.json"), result["stand"])
    if "light" in result:
        from .light import write_light
        os.makedirs(out_dir, exist_ok=True)
        write_light(os.path.join(out_dir, "light.npz"), result["light"])
    if "preview" in result:
        from .render import write_previews
        write_previews(os.path.join(out_dir, "preview"), result["preview"])
    if save_pointwise and "pointwise" in result:
        pw = result["pointwise"]
        pdir = os.path.join(out_dir, "pointwise_results")
        os.makedirs(pdir, exist_ok=True)
        np.savez_compressed(os.path.join(pdir, "pointwise_results.npz"), **pw)
        c, off, ip, vert = pw["coords"], pw["offset_predictions"], pw["instance_preds"], pw["input_feats"][:, -1]
        m = (vert >= result["tau_vert"]) & (np.abs(off[:, 2]) <= result["tau_off"]) & (ip != NON_TREES_LABEL_IN_GROUPING)
        save_data(np.hstack([c[m] + off[m], ip[m].reshape(-1, 1)]), save_formats[0], "cluster_coords_initial", pdir)
        t = ip != NON_TREES_LABEL_IN_GROUPING
        save_data(np.hstack([c[t] + off[t], ip[t].reshape(-1, 1)]), save_formats[0], "cluster_coords", pdir)


# ------------------------------------------------------------------------------------------------ command line
def load_forest(path):
    """N x 3 or N x 4 float64 from .npy, .npz ('points' [+ 'labels']), whitespace-separated .txt, or .las / .laz (util.las.read_las:
    x y z, and the label column when the file has a treeID dimension)."""
    if path.lower().endswith((".las", ".laz")):
        from .las import read_las
        return read_las(path)
    from .eval import _read_points
    data = _read_points(path)
    if data.ndim != 2 or data.shape[1] not in (3, 4):
        raise ValueError(f"{path}: expected N x 3 or N x 4 (x y z [label]), got {data.shape}")
    return data


def sample_generator_of(a):
    """The `sample_generator` section of the parsed command line."""
    return dict(n_neigh_sor=a.n_neigh_sor, multiplier_sor=a.multiplier_sor, rad=a.rad, npoints_rad=a.npoints_rad)


def parse_args(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.segment", description="segment a forest point cloud into trees")
    ap.add_argument("--forest", required=True, help="input cloud: .npy / .npz / .txt / .las, N x 3 or N x 4")
    ap.add_argument("--weights", required=True, help="model checkpoint (.pth with a 'net' state dict)")
    ap.add_argument("--out", required=True, help="results directory")
    ap.add_argument("--voxel-size", type=float, default=SAMPLE_CFG["voxel_size"])
    ap.add_argument("--inner-edge", type=float, default=SAMPLE_CFG["inner_edge"])
    ap.add_argument("--outer-edge", type=float, default=SAMPLE_CFG["outer_edge"])
    ap.add_argument("--stride", type=float, default=SAMPLE_CFG["stride"])
    ap.add_argument("--n-neigh-sor", type=int, default=None, help="statistical outlier filter on every tile: neighbours (with --multiplier-sor)")
    ap.add_argument("--multiplier-sor", type=float, default=None, help="statistical outlier filter: standard-deviation ratio")
    ap.add_argument("--rad", type=float, default=None, help="radius outlier filter on every tile: radius in metres (with --npoints-rad)")
    ap.add_argument("--npoints-rad", type=int, default=None, help="radius outlier filter: a point is kept with more than this many points in the ball")
    ap.add_argument("--alpha", type=float, default=SHAPE_CFG["alpha"])
    ap.add_argument("--edge-buffer", type=float, default=SHAPE_CFG["buffer_size_to_determine_edge_trees"])
    ap.add_argument("--outer-remove", type=float, default=None, help="remove this many metres at the plot's xy outline (default: off)")
    ap.add_argument("--grouping", choices=("hdbscan", "dbscan"), default="hdbscan")
    ap.add_argument("--tau-min", type=int, default=GROUPING_CFG["tau_min"])
    ap.add_argument("--tau-group", type=float, default=GROUPING_CFG["tau_group"])
    ap.add_argument("--tau-vert", type=float, default=GROUPING_CFG["tau_vert"])
    ap.add_argument("--tau-off", type=float, default=GROUPING_CFG["tau_off"])
    ap.add_argument("--return-type", choices=RETURN_TYPES, default="original")
    ap.add_argument("--formats", nargs="+", default=["npz"], help=f"any of {SAVE_FORMATS}")
    ap.add_argument("--no-treewise", action="store_true", help="do not write individual_trees/")
    ap.add_argument("--save-pointwise", action="store_true", help="write pointwise_results/")
    ap.add_argument("--dtype", choices=("fp32", "bf16", "fp16"), default="fp32", help="network compute dtype")
    ap.add_argument("--inventory", action="store_true", help="write tree_inventory.csv: position, height, DBH and crown cover of every tree")
    from .inventory import add_arguments, check_params, params_of
    add_arguments(ap)
    ap.add_argument("--terrain", action="store_true", help="write terrain.npz and height_above_ground.npy; with --inventory, add the ground columns")
    from . import terrain as _terrain
    _terrain.add_arguments(ap)
    ap.add_argument("--stem", action="store_true", help="write stem_profiles.npz and add the stem columns to tree_inventory.csv (implies --inventory)")
    from . import stem as _stem
    _stem.add_arguments(ap)
    ap.add_argument("--crown", action="store_true", help="write crown_profiles.npz and add the crown columns to tree_inventory.csv (implies --inventory)")
    from . import crown as _crown
    _crown.add_arguments(ap)
    ap.add_argument("--branches", action="store_true", help="write skeletons.npz and add the branch columns to tree_inventory.csv (implies --inventory)")
    from . import branches as _branches
    _branches.add_arguments(ap)
    ap.add_argument("--wood", action="store_true", help="write cylinders.npz and add the wood columns to tree_inventory.csv (implies --branches)")
    from . import wood as _wood
    _wood.add_arguments(ap)
    ap.add_argument("--leafwood", action="store_true", help="write leafwood.npy (the wood flag of every row) and add the leafwood columns to tree_inventory.csv (implies --inventory); --branches and --wood then read the wood rows only")
    from . import leafwood as _leafwood
    _leafwood.add_arguments(ap)
    ap.add_argument("--canopy", action="store_true", help="write canopy.npz (canopy height model, tree tops, grid metrics) and stand.json (implies --terrain)")
    from . import canopy as _canopy
    _canopy.add_arguments(ap)
    ap.add_argument("--light", action="store_true", help="write light.npz (voxel grid, openness, effective LAI and gap fractions on a sensor grid) and add the light columns to tree_inventory.csv when it is written (implies --terrain)")
    from . import light as _light
    _light.add_arguments(ap)
    ap.add_argument("--preview", action="store_true", help="write preview/<name>.png: the segmented cloud from the top and the south, heights, the contact sheet of the trees, and the DTM, CHM and wood flags where they are computed")
    from . import render as _render
    _render.add_arguments(ap, "preview-")
    a = ap.parse_args(argv)
    try:
        check_params(params_of(a))
        _terrain.check_params(_terrain.params_of(a))
        _stem.check_params(_stem.params_of(a))
        _crown.check_params(_crown.params_of(a))
        _canopy.check_params(_canopy.params_of(a))
        _light.check_params(_light.params_of(a))
        _branches.check_params(_branches.params_of(a))
        _wood.check_params(_wood.params_of(a))
        _leafwood.check_params(_leafwood.params_of(a))
        _leafwood.check_scales(_leafwood.scales_of(a))
        _render.check_params(_render.params_of(a, "preview-"))
    except ValueError as e:
        ap.error(str(e))
    check_formats(a.formats)
    for k in ("voxel_size", "inner_edge", "outer_edge", "stride"):
        if not getattr(a, k) > 0:
            ap.error(f"--{k.replace('_', '-')} must be > 0")
    if a.outer_edge < a.inner_edge:
        ap.error("--outer-edge must be >= --inner-edge")
    if a.edge_buffer < 0 or (a.outer_remove is not None and a.outer_remove < 0):
        ap.error("buffer sizes must be >= 0")
    try:
        from .outlier import active_filters
        active_filters(sample_generator_of(a))
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))
    if not os.path.exists(a.forest):
        ap.error(f"--forest {a.forest}: no such file")
    if not os.path.exists(a.weights):
        ap.error(f"--weights {a.weights}: no such file")
    return a


def main(argv=None):
    import logging
    a = parse_args(argv)
    from ..model import TreeLearn
    from .train import load_checkpoint
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    logger = logging.getLogger("treelearn_amd.segment")
    points = load_forest(a.forest)
    dt = dict(fp32=torch.float32, bf16=torch.bfloat16, fp16=torch.float16)[a.dtype]
    model = TreeLearn(**dict(MODEL_CFG, voxel_size=a.voxel_size), compute_dtype=dt)
    load_checkpoint(a.weights, logger, model)
    model = model.cuda().eval()
    sample = dict(SAMPLE_CFG, voxel_size=a.voxel_size, inner_edge=a.inner_edge, outer_edge=a.outer_edge, stride=a.stride,
                  sample_generator=sample_generator_of(a))
    grouping = dict(GROUPING_CFG, use_hdbscan=a.grouping == "hdbscan", tau_min=a.tau_min, tau_group=a.tau_group,
                    tau_vert=a.tau_vert, tau_off=a.tau_off)
    shape = dict(SHAPE_CFG, alpha=a.alpha, buffer_size_to_determine_edge_trees=a.edge_buffer, outer_remove=a.outer_remove)
    with torch.no_grad():
        from . import branches as _branches, canopy as _canopy, crown as _crown, leafwood as _leafwood, light as _light, render as _render, stem as _stem, terrain as _terrain, wood as _wood
        from .inventory import params_of
        res = segment_forest(points, model, sample, grouping, shape, a.return_type, logger, return_pointwise=a.save_pointwise,
                             inventory=a.inventory, inventory_cfg=params_of(a) if a.inventory or a.stem or a.crown or a.branches or a.wood or a.leafwood else None,
                             terrain=a.terrain, terrain_cfg=_terrain.params_of(a) if a.terrain or a.canopy or a.light else None,
                             stem=a.stem, stem_cfg=_stem.params_of(a) if a.stem else None,
                             crown=a.crown, crown_cfg=_crown.params_of(a) if a.crown else None,
                             canopy=a.canopy, canopy_cfg=_canopy.params_of(a) if a.canopy else None,
                             branches=a.branches or a.wood, branch_cfg=_branches.params_of(a) if a.branches or a.wood else None,
                             wood=a.wood, wood_cfg=_wood.params_of(a) if a.wood else None,
                             leafwood=a.leafwood, leafwood_cfg=_leafwood.params_of(a) if a.leafwood else None,
                             leafwood_scales=a.leafwood_scales, leafwood_scales_min=a.leafwood_scales_min,
                             preview=a.preview, preview_cfg=_render.params_of(a, "preview-") if a.preview else None,
                             light=a.light, light_cfg=_light.params_of(a) if a.light else None)
    plot_name = os.path.splitext(os.path.basename(a.forest))[0]
    save_results(res, a.out, plot_name, a.formats, save_treewise=not a.no_treewise, save_pointwise=a.save_pointwise)
    cats = np.bincount(res["categories"], minlength=3)
    print(f"{plot_name}: {len(res['coords'])} points, {len(res['categories'])} trees "
          f"({', '.join(f'{n} {c}' for n, c in zip(cats, CATEGORIES))}) -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
