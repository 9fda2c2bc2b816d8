"""Scoring a segmented forest against labelled ground truth (reference tree_learn/util/eval.py, tools/evaluation/evaluate.py).

Same names, signatures and results as the reference, so that importing them from `treelearn_amd.util` instead of `tree_learn.util`
is the whole integration.  The point passes run on the GPU as two sparse kernels (csrc/tl_eval.hip):
  * tl_eval_contingency: the pred x gt point-count table.  Every iou / precision / recall matrix entry and every unpartitioned score
    follows from it exactly (tp = C, fp = row sum - C, fn = column sum - C, the same int64 -> float64 division as the reference);
  * tl_eval_partition: the radial (xy) and vertical (z) band counts of each (gt, pred) pair, reading only their points.
The host keeps what is small: the Hungarian assignment on the P x G matrix (scipy), the failure analysis and the aggregates.

    python -m treelearn_amd.util.eval --gt gt.npy --pred pred.npy [--out results.npz]
"""
import argparse
import sys

import numpy as np
import torch

from .. import _hip

DEFAULT_PARTITION = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1]     # configs/evaluation/evaluate.yaml of the reference
NON_TREE_LABEL = 0
MAX_INTERVALS = 256                                                         # tl_eval_partition: at most 257 edges

__all__ = ["get_detections", "get_detection_failures", "evaluate_instance_segmentation", "evaluate_no_partition", "evaluate_xy_partition",
           "evaluate_z_partition", "evaluate_no_partition_arrays", "evaluate_xy_partition_arrays", "evaluate_z_partition_arrays",
           "get_eval_components", "get_segmentation_metrics", "evaluate_forest", "load_points"]


# ------------------------------------------------------------------------------------------------ inputs
def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("treelearn_amd.util.eval runs its point passes on the GPU (tl_eval_*); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _labels(a, name):
    """int64 device tensor of a label array (numpy, list or tensor; float labels truncate like numpy's astype)."""
    dev = _device()
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)).astype(np.int64, copy=False))
    t = t.reshape(-1).to(dev, torch.int64).contiguous()
    if t.numel() == 0:
        raise ValueError(f"{name} is empty")
    return t


def _coords(a, n):
    """float64 device tensor [n, 3] (the reference's load_data yields float64)."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    t = t.to(_device(), torch.float64)
    if t.ndim != 2 or t.shape[1] < 3:
        raise ValueError(f"coords must have shape [N, 3], got {tuple(t.shape)}")
    if t.shape[0] != n:
        raise ValueError(f"mismatched lengths: {t.shape[0]} coordinates for {n} labels")
    return t[:, :3].contiguous()


def _same_length(pred, gt):
    if pred.numel() != gt.numel():
        raise ValueError(f"mismatched lengths: {pred.numel()} predictions for {gt.numel()} ground-truth labels")
    if pred.numel() >= 1 << 31:
        raise ValueError(f"{pred.numel()} points: the evaluation kernels take fewer than 2^31")


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


# ------------------------------------------------------------------------------------------------ the two kernels
def _contingency(pred, gt, n_pred, n_gt, non_tree):
    """i64 [(n_pred + 1), (n_gt + 1)]: row 0 = negative preds, column 0 = non-tree (and any negative) gt (tl_eval_contingency)."""
    L = _hip.lib()
    table = torch.empty((n_pred + 1) * (n_gt + 1), dtype=torch.int64, device=pred.device)
    _hip.check(L.tl_eval_contingency(_hip.ptr(pred), _hip.ptr(gt), pred.numel(), n_pred, n_gt, int(non_tree), _hip.ptr(table), _hip.stream()),
               "tl_eval_contingency")
    return table.view(n_pred + 1, n_gt + 1).cpu().numpy()


def _segments(labels, nseg):
    """Stable CSR of the points by label: the points of label s are order[start[s]:start[s + 1]] in ascending point order."""
    vals, order = torch.sort(labels, stable=True)
    start = torch.searchsorted(vals, torch.arange(nseg + 1, dtype=torch.int64, device=labels.device))
    return order.contiguous(), start.contiguous()


def _partition_counts(pred, gt, coords, pairs, edges, mode):
    """tp, fp, fn i64 [m, len(edges) - 1] and the normaliser f64 [m, 3] of every (gt, pred) pair (tl_eval_partition)."""
    L = _hip.lib()
    dev = pred.device
    m, nint = len(pairs), len(edges) - 1
    n_gt, n_pred = int(gt.max()) + 1, int(pred.max()) + 1
    n_gt = max(n_gt, 0); n_pred = max(n_pred, 0)
    g_order, g_start = _segments(gt, n_gt)
    p_order, p_start = _segments(pred, n_pred)
    sizes = (g_start[1:] - g_start[:-1]).cpu().numpy()
    for g, _ in pairs:
        k = int(sizes[g]) if 0 <= g < n_gt else 0
        if k < 5:
            raise ValueError(f"ground-truth tree {g} has {k} points: the partitions normalise by the 5th-largest value, which needs at least 5")
    pr = torch.from_numpy(np.asarray(pairs, np.int64).reshape(-1, 2)).to(dev).contiguous()
    ed = torch.from_numpy(np.asarray(edges, np.float64)).to(dev).contiguous()
    tp, fp, fn = (torch.zeros((m, nint), dtype=torch.int64, device=dev) for _ in range(3))
    norm = torch.zeros((m, 3), dtype=torch.float64, device=dev)
    if m:
        _hip.check(L.tl_eval_partition(_hip.ptr(coords), _hip.ptr(gt), _hip.ptr(pred), gt.numel(), _hip.ptr(g_order), _hip.ptr(g_start), n_gt,
                                       _hip.ptr(p_order), _hip.ptr(p_start), n_pred, _hip.ptr(pr), m, _hip.ptr(ed), nint + 1, mode,
                                       _hip.ptr(tp), _hip.ptr(fp), _hip.ptr(fn), _hip.ptr(norm), _hip.stream()), "tl_eval_partition")
    return tp.cpu().numpy(), fp.cpu().numpy(), fn.cpu().numpy(), norm.cpu().numpy()


# ------------------------------------------------------------------------------------------------ metrics
def get_eval_components(preds_mask, labels_mask):
    """tp, fp, tn, fn of two boolean masks (reference eval.py:230-239)."""
    p, t = np.asarray(_host(preds_mask), bool), np.asarray(_host(labels_mask), bool)
    assert len(p) == len(t)
    return (p & t).sum(), (p & ~t).sum(), (~p & ~t).sum(), (~p & t).sum()


def get_segmentation_metrics(tp, fp, fn):
    """precision, recall, iou; NaN where the denominator is 0 (reference eval.py:242-260)."""
    assert not (np.isnan(tp) or np.isnan(fp) or np.isnan(fn)), 'one of the inputs is nan'
    iou = np.nan if tp + fp + fn == 0 else tp / (tp + fp + fn)
    rec = np.nan if tp + fn == 0 else tp / (tp + fn)
    prec = np.nan if tp + fp == 0 else tp / (tp + fp)
    return prec, rec, iou


def _metrics(tp, fp, fn):
    """get_segmentation_metrics over int64 arrays (the same int64 -> float64 divisions)."""
    tp, fp, fn = (np.asarray(a, np.int64) for a in (tp, fp, fn))
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(tp + fp == 0, np.nan, tp / (tp + fp))
        rec = np.where(tp + fn == 0, np.nan, tp / (tp + fn))
        iou = np.where(tp + fp + fn == 0, np.nan, tp / (tp + fp + fn))
    return prec, rec, iou


def _nanmean(x):
    """DataFrame.mean's NaN-skipping mean: NaNs zeroed, summed, divided by the count of the others."""
    x = np.array(x, np.float64)
    nan = np.isnan(x)
    x[nan] = 0.0
    c = int((~nan).sum())
    return x.sum() / c if c else np.nan


# ------------------------------------------------------------------------------------------------ detection
def get_detections(instance_labels, instance_preds, min_iou_match, non_tree_label):
    """Hungarian matching of predicted and ground-truth trees on point IoU (reference eval.py:7-31).

    Returns matched_gts, matched_preds and the iou, precision and recall matrices, float64 [max pred + 1, max label + 1] with 0 where a
    prediction holds no point of a tree; all three come from one GPU contingency table."""
    from scipy.optimize import linear_sum_assignment
    gt, pred = _labels(instance_labels, "instance_labels"), _labels(instance_preds, "instance_preds")
    _same_length(pred, gt)
    bad = gt[(gt < 0) & (gt != int(non_tree_label))]
    if bad.numel():
        raise ValueError(f"ground-truth label {int(bad.min())} is negative and not the non-tree label {non_tree_label}: "
                         "the reference would write its scores into a wrapped column")
    iou, prec, rec = _matrices(_contingency(pred, gt, int(pred.max()) + 1, int(gt.max()) + 1, non_tree_label))
    rows, cols = linear_sum_assignment(iou, maximize=True)
    keep = iou[rows, cols] > min_iou_match
    return cols[keep], rows[keep], iou, prec, rec


def _matrices(table):
    """iou, precision, recall [P, G] from the contingency table (row / column 0 = none)."""
    C = table[1:, 1:]
    R = table[1:, :].sum(1)[:, None]           # points of each pred
    S = table[:, 1:].sum(0)[None, :]           # points of each gt tree
    hit = C > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(hit, C / (R + S - C), 0.0)
        prec = np.where(hit, C / R, 0.0)
        rec = np.where(hit, C / S, 0.0)
    return iou, prec, rec


def get_detection_failures(matched_gts, matched_preds, unique_instance_labels, unique_instance_preds, iou_matrix,
                           precision_matrix, recall_matrix, min_precision_for_pred, min_recall_for_gt):
    """Unmatched predictions and trees, and what they correspond to (reference eval.py:35-76).  Host-only: works on the matrices.

    Unmatched predictions whose precision summed over all trees reaches min_precision_for_pred map to the tree of highest precision
    (commission errors), else NaN.  Unmatched trees with a prediction of recall >= min_recall_for_gt map to that prediction and to the
    other tree of highest recall in it, if that recall reaches min_recall_for_gt (undersegmentation), else NaN."""
    assert (iou_matrix[matched_preds, matched_gts] > 0).sum() == len(matched_preds), 'a zero iou correspondence has been matched'
    # set differences in the reference's set order (it is what fixes the order of the outputs)
    non_matched_preds = np.array(list(set(unique_instance_preds) - set(matched_preds))).astype(np.int64)
    non_matched_gts = np.array(list(set(unique_instance_labels) - set(matched_gts))).astype(np.int64)

    pred_gt = [np.nan if precision_matrix[p].sum() < min_precision_for_pred else precision_matrix[p].argmax() for p in non_matched_preds]

    gt_pred, gt_other = [], []
    all_gts = np.arange(recall_matrix.shape[1])
    for g in non_matched_gts:
        col = recall_matrix[:, g]
        if col.max() < min_recall_for_gt:
            gt_pred.append(np.nan); gt_other.append(np.nan)
            continue
        p = np.argmax(col)
        gt_pred.append(p)
        others = np.delete(all_gts, g)
        r = recall_matrix[p, others]
        j = r.argmax()
        gt_other.append(np.nan if r[j] < min_recall_for_gt else others[j])
    return non_matched_gts, non_matched_preds, np.array(pred_gt), np.array(gt_pred), np.array(gt_other)


# ------------------------------------------------------------------------------------------------ segmentation
def _frame(cols):
    try:
        import pandas as pd
    except ImportError as e:
        raise ImportError("the evaluate_*_partition functions return a pandas.DataFrame and pandas is not installed; "
                          "use the *_arrays forms for a dict of numpy arrays") from e
    return pd.DataFrame.from_dict(cols)


def _pairs(unique_gts, unique_preds):
    g, p = np.asarray(_host(unique_gts), np.int64).reshape(-1), np.asarray(_host(unique_preds), np.int64).reshape(-1)
    m = min(len(g), len(p))                                    # zip()
    g, p = g[:m], p[:m]
    if (g < 0).any() or (p < 0).any():
        raise ValueError("unique_gts / unique_preds must be tree ids >= 0")
    return g, p


def _id_columns(g, p, mapping_to_original_gt_nums, mapping_to_original_pred_nums):
    return {"instance_pred": np.array([mapping_to_original_pred_nums[x] for x in p]),
            "instance_label": np.array([mapping_to_original_gt_nums[x] for x in g])}


def evaluate_no_partition_arrays(instance_preds, instance_labels, unique_gts, unique_preds, mapping_to_original_gt_nums,
                                 mapping_to_original_pred_nums):
    """evaluate_no_partition as a dict of numpy arrays (same columns)."""
    gt, pred = _labels(instance_labels, "instance_labels"), _labels(instance_preds, "instance_preds")
    _same_length(pred, gt)
    g, p = _pairs(unique_gts, unique_preds)
    n_gt = max(int(gt.max()) + 1, int(g.max()) + 1 if len(g) else 0)
    n_pred = max(int(pred.max()) + 1, int(p.max()) + 1 if len(p) else 0)
    T = _contingency(pred, gt, n_pred, n_gt, -1)
    C = T[p + 1, g + 1]
    tp, fp, fn = C, T[p + 1, :].sum(1) - C, T[:, g + 1].sum(0) - C
    out = _id_columns(g, p, mapping_to_original_gt_nums, mapping_to_original_pred_nums)
    out["prec"], out["rec"], out["iou"] = _metrics(tp, fp, fn)
    return out


def evaluate_no_partition(instance_preds, instance_labels, unique_gts, unique_preds, mapping_to_original_gt_nums, mapping_to_original_pred_nums):
    """Precision, recall and iou of each (gt, pred) pair over whole trees (reference eval.py:100-123), as a DataFrame."""
    return _frame(evaluate_no_partition_arrays(instance_preds, instance_labels, unique_gts, unique_preds, mapping_to_original_gt_nums,
                                               mapping_to_original_pred_nums))


def _partition_arrays(mode, instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls, mapping_to_original_gt_nums,
                      mapping_to_original_pred_nums):
    gt, pred = _labels(instance_labels, "instance_labels"), _labels(instance_preds, "instance_preds")
    _same_length(pred, gt)
    xyz = _coords(coords, gt.numel())
    g, p = _pairs(unique_gts, unique_preds)
    edges = list(intvls)
    if len(edges) - 1 > MAX_INTERVALS:
        raise ValueError(f"{len(edges) - 1} intervals: at most {MAX_INTERVALS}")
    # (fewer than two edges: no band, but the per-tree checks still run, as the reference still computes each tree's normaliser)
    tp, fp, fn, _ = _partition_counts(pred, gt, xyz, list(zip(g.tolist(), p.tolist())), edges if len(edges) >= 2 else [0.0, 0.0], mode)
    k = max(len(edges) - 1, 0)
    prec, rec, iou = _metrics(tp[:, :k], fp[:, :k], fn[:, :k])
    out = _id_columns(g, p, mapping_to_original_gt_nums, mapping_to_original_pred_nums)
    names = [f"{edges[i]}_{edges[i + 1]}" for i in range(k)]
    for name, v in (("prec", prec), ("rec", rec), ("iou", iou)):
        for i, s in enumerate(names):
            out[f"{name}_intvl{s}"] = v[:, i]
    return out


def evaluate_xy_partition_arrays(instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls, mapping_to_original_gt_nums,
                                 mapping_to_original_pred_nums):
    """evaluate_xy_partition as a dict of numpy arrays (same columns)."""
    return _partition_arrays(_hip.TL_EVAL_XY, instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls,
                             mapping_to_original_gt_nums, mapping_to_original_pred_nums)


def evaluate_z_partition_arrays(instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls, mapping_to_original_gt_nums,
                                mapping_to_original_pred_nums):
    """evaluate_z_partition as a dict of numpy arrays (same columns)."""
    return _partition_arrays(_hip.TL_EVAL_Z, instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls,
                             mapping_to_original_gt_nums, mapping_to_original_pred_nums)


def evaluate_xy_partition(instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls, mapping_to_original_gt_nums,
                          mapping_to_original_pred_nums):
    """Scores in radial bands around each tree's position, distances normalised by the tree's 5th-largest (reference eval.py:127-178)."""
    return _frame(evaluate_xy_partition_arrays(instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls,
                                               mapping_to_original_gt_nums, mapping_to_original_pred_nums))


def evaluate_z_partition(instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls, mapping_to_original_gt_nums,
                         mapping_to_original_pred_nums):
    """Scores in vertical bands from each tree's lowest point to its 5th-highest (reference eval.py:182-226)."""
    return _frame(evaluate_z_partition_arrays(instance_preds, instance_labels, unique_gts, unique_preds, coords, intvls,
                                              mapping_to_original_gt_nums, mapping_to_original_pred_nums))


def evaluate_instance_segmentation(instance_preds, instance_labels, unique_gts, unique_preds, coords, mapping_to_original_gt_nums,
                                   mapping_to_original_pred_nums, xy_partition, z_partition, frames=True):
    """(no_partition, xy, z) (reference eval.py:80-96); a partition that is None or empty gives None.  frames=False: dicts of arrays."""
    f = _frame if frames else (lambda d: d)
    args = (instance_preds, instance_labels, unique_gts, unique_preds)
    maps = (mapping_to_original_gt_nums, mapping_to_original_pred_nums)
    no = f(evaluate_no_partition_arrays(*args, *maps))
    xy = f(evaluate_xy_partition_arrays(*args, coords, xy_partition, *maps)) if xy_partition is not None and len(xy_partition) else None
    z = f(evaluate_z_partition_arrays(*args, coords, z_partition, *maps)) if z_partition is not None and len(z_partition) else None
    return no, xy, z


# ------------------------------------------------------------------------------------------------ the whole protocol
def _consecutive(labels, non_tree_label):
    """non-tree -> -1, trees -> 0, 1, ... in ascending order of the original ids; the new -> original map (-1 -> non_tree_label)."""
    labels = labels.clone()
    labels[labels == non_tree_label] = -1
    tree = labels != -1
    palette = torch.unique(labels[tree])
    labels[tree] = torch.searchsorted(palette, labels[tree])
    pal = palette.cpu().numpy()
    mapping = {i: v for i, v in enumerate(pal)}
    mapping[-1] = non_tree_label
    return labels, mapping, pal


def _aggregate(matched_gts, matched_preds, failures, no_partition, gmap, pmap):
    """Detection results in original ids and the aggregated scores (reference tools/evaluation/evaluate.py:78-102, 124-146): host-only.
    failures = get_detection_failures(...); no_partition = the evaluate_no_partition columns; gmap / pmap = new -> original ids."""
    non_matched_gts, non_matched_preds, nmp_gt, nmg_pred, nmg_other = failures
    no = no_partition
    og = lambda v: np.nan if np.isnan(v) else gmap[v]                          # noqa: E731
    op = lambda v: np.nan if np.isnan(v) else pmap[v]                          # noqa: E731
    matched_gts = np.array([gmap[v] for v in matched_gts])
    matched_preds = np.array([pmap[v] for v in matched_preds])
    non_matched_preds = np.array([pmap[v] for v in non_matched_preds])
    nmp_gt = np.array([og(v) for v in nmp_gt])
    keep = [not np.isnan(v) for v in nmp_gt]
    nmp_filtered = np.array([v for v, k in zip(non_matched_preds, keep) if k])
    nmp_gt_filtered = np.array([v for v, k in zip(nmp_gt, keep) if k])
    non_matched_gts = np.array([gmap[v] for v in non_matched_gts])
    nmg_other = np.array([og(v) for v in nmg_other])
    nmg_pred = np.array([op(v) for v in nmg_pred])

    completeness = len(matched_gts) / (len(matched_gts) + len(non_matched_gts))
    omission = 1 - completeness
    commission = len(nmp_filtered) / (len(matched_preds) + len(nmp_filtered))
    f1 = 2 * ((1 - commission) * (1 - omission)) / (2 - (commission + omission))
    det = {"completeness": np.round(completeness * 100, 1), "omission_error_rate": np.round(omission * 100, 1),
           "commission_error_rate": np.round(commission * 100, 1), "f1_score": np.round(f1 * 100, 1),
           "matched_gts": matched_gts, "matched_preds": matched_preds,
           "non_matched_preds": non_matched_preds, "non_matched_preds_corresponding_gt": nmp_gt,
           "non_matched_preds_filtered": nmp_filtered, "non_matched_preds_corresponding_gt_filtered": nmp_gt_filtered,
           "non_matched_gts": non_matched_gts, "non_matched_gts_corresponding_other_tree": nmg_other,
           "non_matched_gts_corresponding_pred": nmg_pred}
    seg = {k: np.round(_nanmean(no[c]) * 100, 1) for k, c in (("precision", "prec"), ("recall", "rec"), ("iou", "iou"))}
    return det, seg


def evaluate_forest(gt_coords, gt_labels, pred_coords, pred_labels, min_iou_for_match=0.5, min_precision_for_pred=0.5, min_recall_for_gt=0.5,
                    xy_partition=DEFAULT_PARTITION, z_partition=DEFAULT_PARTITION, non_tree_label=NON_TREE_LABEL, frames=True, timings=None):
    """The compute body of the reference's tools/evaluation/evaluate.py:evaluate(), without file I/O or logging.

    Propagates the predictions onto the ground-truth points (5-NN vote on the GPU), relabels both sides (non-tree -> -1, trees ->
    0, 1, ...), matches, analyses the failures, scores the segmentation and aggregates.  Returns (results_dict, propagated_preds):
    the reference's results dict (same keys and values; frames=False puts dicts of arrays where it has DataFrames) and the
    predictions on the ground-truth points in their original ids.  `timings`: a dict that receives per-stage milliseconds."""
    from .postprocess import knn_vote
    import time
    clock = [time.perf_counter()]
    gl = _labels(gt_labels, "gt_labels")
    gc = _coords(gt_coords, gl.numel())
    pl = _labels(pred_labels, "pred_labels")
    pc = _coords(pred_coords, pl.numel())

    def lap(name):
        if timings is not None:
            torch.cuda.synchronize()
            t = time.perf_counter()
            timings[name] = (t - clock[0]) * 1e3
            clock[0] = t
    lap("inputs")
    prop = knn_vote(pc.float().contiguous(), pl, gc.float().contiguous(), 5)          # propagate_preds(..., 5): float32 coordinates
    lap("propagation")

    gt, gmap, _ = _consecutive(gl, non_tree_label)
    pred, pmap, ppal = _consecutive(prop, non_tree_label)
    if pred.max() < 0:
        raise ValueError("no predicted tree: every propagated prediction is the non-tree label")

    n_pred, n_gt = int(pred.max()) + 1, int(gt.max()) + 1
    table = _contingency(pred, gt, n_pred, n_gt, -1)
    lap("contingency")
    from scipy.optimize import linear_sum_assignment
    iou, prec_m, rec_m = _matrices(table)
    rows, cols = linear_sum_assignment(iou, maximize=True)
    keep = iou[rows, cols] > min_iou_for_match
    matched_gts, matched_preds = cols[keep], rows[keep]
    failures = get_detection_failures(matched_gts, matched_preds, np.arange(n_gt), np.arange(n_pred), iou, prec_m, rec_m,
                                      min_precision_for_pred, min_recall_for_gt)
    non_matched_gts, non_matched_preds, nmp_gt, nmg_pred, nmg_other = failures
    lap("hungarian")

    unique_gts, unique_preds = np.arange(iou.shape[1]), iou.argmax(axis=0)
    f = _frame if frames else (lambda d: d)
    C = table[unique_preds + 1, unique_gts + 1]
    no = _id_columns(unique_gts, unique_preds, gmap, pmap)
    no["prec"], no["rec"], no["iou"] = _metrics(C, table[unique_preds + 1, :].sum(1) - C, table[:, unique_gts + 1].sum(0) - C)
    xy = z = None
    if xy_partition is not None and len(xy_partition):
        xy = evaluate_xy_partition_arrays(pred, gt, unique_gts, unique_preds, gc, xy_partition, gmap, pmap)
    lap("xy")
    if z_partition is not None and len(z_partition):
        z = evaluate_z_partition_arrays(pred, gt, unique_gts, unique_preds, gc, z_partition, gmap, pmap)
    lap("z")

    det, seg = _aggregate(matched_gts, matched_preds, failures, no, gmap, pmap)
    seg.update(no_partition=f(no), xy_partition=None if xy is None else f(xy), z_partition=None if z is None else f(z))
    pn = pred.cpu().numpy()
    propagated = np.where(pn < 0, non_tree_label, ppal[np.maximum(pn, 0)] if len(ppal) else non_tree_label).astype(np.int64)
    lap("aggregate")
    return {"detection_results": det, "segmentation_results": seg}, propagated


# ------------------------------------------------------------------------------------------------ command line
def _read_points(path):
    """A float64 array from .npy, .npz ('points' [+ 'labels'] as a last column, as the reference's load_data) or whitespace-separated .txt."""
    if path.endswith(".npy"):
        data = np.load(path)
    elif path.endswith(".npz"):
        with np.load(path) as z:
            if "points" not in z:
                raise ValueError(f"{path}: an .npz needs a 'points' array")
            data = z["points"] if "labels" not in z else np.hstack((z["points"], z["labels"][:, None]))
    elif path.endswith(".txt"):
        data = np.loadtxt(path, ndmin=2)
    else:
        raise ValueError(f"{path}: expected .npy, .npz or .txt")
    return np.asarray(data, np.float64)


def load_points(path):
    """N x 4 (x y z label) float64 from .npy, .npz ('points' [+ 'labels'], as the reference's load_data) or whitespace-separated .txt."""
    data = _read_points(path)
    if data.ndim != 2 or data.shape[1] != 4:
        raise ValueError(f"{path}: expected N x 4 (x y z label), got {data.shape}")
    return data


def _load_labelled(path):
    """load_points, and .las / .laz through util.las.read_las (a file without a treeID dimension has no label column and is refused)."""
    if not path.lower().endswith((".las", ".laz")):
        return load_points(path)
    from .las import read_las
    data = read_las(path)
    if data.shape[1] != 4:
        raise ValueError(f"{path}: expected N x 4 (x y z label), got {data.shape}: the file has no treeID dimension")
    return data


HEADLINE = (("Completeness", "detection_results", "completeness"), ("Omission Error Rate", "detection_results", "omission_error_rate"),
            ("Commission Error Rate", "detection_results", "commission_error_rate"), ("F1 Score", "detection_results", "f1_score"),
            ("Precision", "segmentation_results", "precision"), ("Recall", "segmentation_results", "recall"),
            ("Coverage", "segmentation_results", "iou"))


def flatten_results(results, propagated=None):
    """The results dict as flat npz entries: 'detection_results/completeness', 'segmentation_results/xy_partition/prec_intvl0_0.1', ..."""
    out = {}

    def walk(prefix, v):
        if isinstance(v, dict):
            for k, x in v.items():
                walk(f"{prefix}/{k}" if prefix else k, x)
        elif hasattr(v, "to_dict") and hasattr(v, "columns"):           # a DataFrame
            for c in v.columns:
                out[f"{prefix}/{c}"] = v[c].to_numpy()
        elif v is not None:
            out[prefix] = np.asarray(v)
    walk("", results)
    if propagated is not None:
        out["pred_forest_propagated_to_gt_pointcloud"] = np.asarray(propagated)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.eval", description="score a segmented forest against ground truth")
    ap.add_argument("--gt", required=True, help="ground truth: .npy / .npz / .txt / .las, N x 4 (x y z label)")
    ap.add_argument("--pred", required=True, help="prediction: .npy / .npz / .txt / .las, M x 4 (x y z label)")
    ap.add_argument("--out", default=None, help="write the results dict (flattened) to this .npz")
    a = ap.parse_args(argv)
    gt, pr = _load_labelled(a.gt), _load_labelled(a.pred)
    res, prop = evaluate_forest(gt[:, :3], gt[:, 3], pr[:, :3], pr[:, 3], frames=False)
    for title, sec, key in HEADLINE:
        print(f"{title}: {res[sec][key]}%")
    if a.out:
        np.savez_compressed(a.out, **flatten_results(res, prop))
    return 0


if __name__ == "__main__":
    sys.exit(main())
