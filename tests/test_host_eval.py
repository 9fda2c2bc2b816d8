"""Forest scoring, host side (no GPU): the numpy restatement (tests/eval_restatement.py) against the reference's outputs in G13, the
host-only helpers of treelearn_amd.util.eval (failure analysis, aggregates, metrics, file loading) and the public exports."""
import os

import numpy as np
import pytest

import eval_restatement as R

PART = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1]


@pytest.fixture(scope="module")
def g13(golden_dir):
    return R.load_g13(os.path.join(golden_dir, "g13_eval.npz"))        # (b) and (c)'s point clouds rebuilt, checked by digest


def case_keys(g13):
    return [f"a/{c}" for c in g13["a/cases"]] + ["b"]


def frame(g13, prefix):
    p = prefix + "/"
    return {k[len(p):]: v for k, v in g13.items() if k.startswith(p)}


def test_restatement_reproduces_the_reference_detection_and_segmentation(g13):
    for key in case_keys(g13):
        gt, pred, xyz = g13[f"{key}/gt"].astype(np.int64), g13[f"{key}/pred"].astype(np.int64), g13[f"{key}/coords"].astype(np.float64)
        mg, mp, iou, prec, rec = R.get_detections(gt, pred, float(g13[f"{key}/min_iou"]), -1)
        for name, v in dict(matched_gts=mg, matched_preds=mp, iou=iou, prec=prec, rec=rec).items():
            np.testing.assert_array_equal(v, g13[f"{key}/{name}"], err_msg=f"{key} {name}")
        ug, up = np.arange(iou.shape[1]), iou.argmax(axis=0)
        ref = frame(g13, f"{key}/no_partition")
        for name, v in zip(("prec", "rec", "iou"), R.no_partition(pred, gt, ug, up)):
            np.testing.assert_array_equal(v, ref[name], err_msg=f"{key} no_partition {name}")
        for part, mode in (("xy_partition", "xy"), ("z_partition", "z")):
            ref = frame(g13, f"{key}/{part}")
            got = R.partition(pred, gt, xyz, ug, up, PART, mode)
            assert set(got) | {"instance_pred", "instance_label"} == set(ref), key
            for name, v in got.items():
                np.testing.assert_array_equal(v, ref[name], err_msg=f"{key} {part} {name}")


def test_detection_failures_from_the_matrices(g13):
    from treelearn_amd.util.eval import get_detection_failures
    names = ("non_matched_gts", "non_matched_preds", "nmp_corresponding_gt", "nmg_corresponding_pred", "nmg_corresponding_other_tree")
    for key in case_keys(g13):
        gt, pred = g13[f"{key}/gt"], g13[f"{key}/pred"]
        got = get_detection_failures(g13[f"{key}/matched_gts"], g13[f"{key}/matched_preds"], np.arange(gt.max() + 1), np.arange(pred.max() + 1),
                                     g13[f"{key}/iou"], g13[f"{key}/prec"], g13[f"{key}/rec"], 0.5, 0.5)
        for name, v in zip(names, got):
            ref = g13[f"{key}/{name}"]
            assert v.dtype == ref.dtype, (key, name, v.dtype, ref.dtype)
            np.testing.assert_array_equal(v, ref, err_msg=f"{key} {name}")


def test_aggregates_of_evaluate(g13):
    """The reference evaluate()'s detection results and mean scores from the intermediates it worked from."""
    from treelearn_amd.util.eval import _aggregate
    gpal, ppal = g13["c/mid/gt_palette"], g13["c/mid/pred_palette"]
    gmap = {i: v for i, v in enumerate(gpal)}; gmap[-1] = 0
    pmap = {i: v for i, v in enumerate(ppal)}; pmap[-1] = 0
    fails = tuple(g13[f"c/mid/failures{i}"] for i in range(5))
    det, seg = _aggregate(g13["c/mid/matched_gts"], g13["c/mid/matched_preds"], fails, frame(g13, "c/mid/no_partition"), gmap, pmap)
    for k, v in det.items():
        ref = g13[f"c/detection_results/{k}"]
        np.testing.assert_array_equal(np.asarray(v), ref, err_msg=k)
        assert np.asarray(v).dtype == ref.dtype or ref.size == 0, (k, np.asarray(v).dtype, ref.dtype)
    for k in ("precision", "recall", "iou"):
        assert seg[k] == g13[f"c/segmentation_results/{k}"], k


def test_segmentation_metrics_and_components(g13):
    from treelearn_amd.util.eval import _metrics, get_eval_components, get_segmentation_metrics
    for key in case_keys(g13):
        gt, pred, iou = g13[f"{key}/gt"], g13[f"{key}/pred"], g13[f"{key}/iou"]
        c = get_eval_components(pred == iou.argmax(axis=0)[0], gt == 0)
        np.testing.assert_array_equal(np.array(c, np.int64), g13[f"{key}/components0"])
        np.testing.assert_array_equal(np.array(get_segmentation_metrics(c[0], c[1], c[3])), g13[f"{key}/metrics0"])
    assert all(np.isnan(v) for v in get_segmentation_metrics(0, 0, 0))
    tp, fp, fn = np.array([0, 3, 0, 2]), np.array([0, 1, 2, 0]), np.array([0, 0, 5, 0])
    got = _metrics(tp, fp, fn)
    for i in range(4):
        ref = get_segmentation_metrics(tp[i], fp[i], fn[i])
        np.testing.assert_array_equal(np.array([g[i] for g in got]), np.array(ref))


def test_nanmean_is_the_dataframe_mean():
    pd = pytest.importorskip("pandas")
    from treelearn_amd.util.eval import _nanmean
    rng = np.random.default_rng(0)
    for n in (1, 7, 20, 185, 1000):
        x = rng.random(n); x[rng.random(n) < 0.2] = np.nan
        assert _nanmean(x) == pd.DataFrame({"a": x})[["a"]].mean(0)["a"] or np.isnan(_nanmean(x))


def test_cli_file_loading(tmp_path, g13):
    from treelearn_amd.util.eval import flatten_results, load_points
    pts = g13["c/gt"].astype(np.float64)
    np.save(tmp_path / "a.npy", pts)
    np.savez(tmp_path / "b.npz", points=pts[:, :3], labels=pts[:, 3])
    np.savetxt(tmp_path / "c.txt", pts)
    for name in ("a.npy", "b.npz", "c.txt"):
        np.testing.assert_array_equal(load_points(str(tmp_path / name)), pts, err_msg=name)
    np.save(tmp_path / "bad.npy", pts[:, :3])
    with pytest.raises(ValueError):
        load_points(str(tmp_path / "bad.npy"))
    with pytest.raises(ValueError):
        load_points(str(tmp_path / "x.las"))
    flat = flatten_results({"detection_results": {"completeness": np.float64(50.0)}, "segmentation_results": {"xy_partition": {"prec_intvl0_0.1": np.ones(2)}, "z_partition": None}}, np.zeros(3))
    assert set(flat) == {"detection_results/completeness", "segmentation_results/xy_partition/prec_intvl0_0.1", "pred_forest_propagated_to_gt_pointcloud"}


def test_eval_entry_points_are_exported():
    import treelearn_amd.util as U
    from treelearn_amd import _hip
    for n in ("get_detections", "get_detection_failures", "evaluate_instance_segmentation", "evaluate_no_partition", "evaluate_xy_partition",
              "evaluate_z_partition", "get_eval_components", "get_segmentation_metrics", "evaluate_forest", "evaluate_xy_partition_arrays",
              "evaluate_z_partition_arrays", "evaluate_no_partition_arrays", "propagate_preds", "make_labels_consecutive"):
        assert callable(getattr(U, n)), n
    assert {"tl_eval_contingency", "tl_eval_partition"} <= set(_hip.PROTOTYPES)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "treelearn_hip.h")).read()
    assert "tl_eval_contingency(" in hdr and "tl_eval_partition(" in hdr


def test_eval_needs_the_gpu(monkeypatch):
    """No quiet CPU path: without a GPU the point passes refuse to run."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from treelearn_amd.util.eval import get_detections
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_detections(np.array([0, 1]), np.array([0, 1]), 0.5, -1)
