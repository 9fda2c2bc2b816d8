"""Forest scoring on the MI355X (treelearn_amd.util.eval, csrc/tl_eval.hip): exact against the reference's outputs in G13 (hand cases, a
150 k-point tile, the whole evaluate()), exact against the numpy restatement on the 68 m plot, device inputs = host inputs, and the
edge cases the reference crashes on or silently corrupts raise ValueError."""
import os

import numpy as np
import pytest
import torch

import eval_restatement as R

pytestmark = pytest.mark.gpu

PART = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1]


@pytest.fixture(scope="module")
def g13(golden_dir):
    return R.load_g13(os.path.join(golden_dir, "g13_eval.npz"))        # (b) and (c)'s point clouds rebuilt, checked by digest


def frame(g13, prefix):
    p = prefix + "/"
    return {k[len(p):]: v for k, v in g13.items() if k.startswith(p)}


def maps(gt, pred):
    gm = {i: i + 1 for i in range(int(gt.max()) + 1)}; gm[-1] = 0
    pm = {i: i + 1 for i in range(int(pred.max()) + 1)}; pm[-1] = 0
    return gm, pm


def check_frame(got, ref, what):
    assert set(got) == set(ref), (what, set(got) ^ set(ref))
    for k, v in ref.items():
        np.testing.assert_array_equal(np.asarray(got[k]), v, err_msg=f"{what} {k}")


def test_g13_every_output_exact(g13):
    from treelearn_amd.util import eval as E
    names = ("non_matched_gts", "non_matched_preds", "nmp_corresponding_gt", "nmg_corresponding_pred", "nmg_corresponding_other_tree")
    for key in [f"a/{c}" for c in g13["a/cases"]] + ["b"]:
        gt, pred, xyz = g13[f"{key}/gt"].astype(np.int64), g13[f"{key}/pred"].astype(np.int64), g13[f"{key}/coords"].astype(np.float64)
        mg, mp, iou, prec, rec = E.get_detections(gt, pred, float(g13[f"{key}/min_iou"]), -1)
        for name, v in dict(matched_gts=mg, matched_preds=mp, iou=iou, prec=prec, rec=rec).items():
            ref = g13[f"{key}/{name}"]
            assert v.dtype == ref.dtype and v.shape == ref.shape, (key, name)
            np.testing.assert_array_equal(v, ref, err_msg=f"{key} {name}")
        fails = E.get_detection_failures(mg, mp, np.arange(gt.max() + 1), np.arange(pred.max() + 1), iou, prec, rec, 0.5, 0.5)
        for name, v in zip(names, fails):
            np.testing.assert_array_equal(v, g13[f"{key}/{name}"], err_msg=f"{key} {name}")
        ug, up = np.arange(iou.shape[1]), iou.argmax(axis=0)
        gm, pm = maps(gt, pred)
        no, xy, z = E.evaluate_instance_segmentation(pred, gt, ug, up, xyz, gm, pm, PART, PART, frames=False)
        check_frame(no, frame(g13, f"{key}/no_partition"), f"{key} no_partition")
        check_frame(xy, frame(g13, f"{key}/xy_partition"), f"{key} xy_partition")
        check_frame(z, frame(g13, f"{key}/z_partition"), f"{key} z_partition")


def test_evaluate_forest_matches_the_reference_evaluate(g13):
    from treelearn_amd.util.eval import evaluate_forest
    gt, pr = g13["c/gt"].astype(np.float64), g13["c/pred"].astype(np.float64)
    res, prop = evaluate_forest(gt[:, :3], gt[:, 3], pr[:, :3], pr[:, 3], frames=False)
    np.testing.assert_array_equal(prop, g13["c/propagated"])
    for k, v in res["detection_results"].items():
        np.testing.assert_array_equal(np.asarray(v), g13[f"c/detection_results/{k}"], err_msg=k)
    seg = res["segmentation_results"]
    for k in ("precision", "recall", "iou"):
        assert seg[k] == g13[f"c/segmentation_results/{k}"], k
    for part in ("no_partition", "xy_partition", "z_partition"):
        check_frame(seg[part], frame(g13, f"c/segmentation_results/{part}"), part)


@pytest.fixture(scope="module")
def plot():
    """The 68 m synthetic plot (about 5 M points) with a perturbed segmentation, consecutive labels (-1 = non-tree)."""
    from treelearn_amd.synth import make_plot
    t = make_plot()
    xyz = t["points"].astype(np.float64)
    gt0 = t["instance_label"].astype(np.int64)
    pred0 = R.perturb(gt0, xyz, seed=21)
    return xyz, R.consecutive(gt0), R.consecutive(pred0)


def test_plot_counts_equal_the_restatement(plot):
    from treelearn_amd import _hip
    from treelearn_amd.util import eval as E
    xyz, gt, pred = plot
    dev = torch.device("cuda")
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    T = E._contingency(p, g, int(pred.max()) + 1, int(gt.max()) + 1, -1)
    np.testing.assert_array_equal(T, R.contingency(pred, gt, int(pred.max()) + 1, int(gt.max()) + 1, -1))
    iou, _, _ = E._matrices(T)
    ug, up = np.arange(iou.shape[1]), iou.argmax(axis=0)
    x = torch.from_numpy(xyz).to(dev)
    for mode, name in ((_hip.TL_EVAL_XY, "xy"), (_hip.TL_EVAL_Z, "z")):
        got = E._partition_counts(p, g, x, list(zip(ug.tolist(), up.tolist())), PART, mode)
        ref = R.partition_counts(pred, gt, xyz, ug, up, PART, name)
        for a, b, what in zip(got, ref, ("tp", "fp", "fn", "norm")):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} {what}")
        assert got[0].sum() > 0.5 * (gt >= 0).sum()                                  # most tree points land in a band as tp


def test_device_inputs_equal_host_inputs(g13):
    from treelearn_amd.util import eval as E
    gt, pred, xyz = g13["b/gt"].astype(np.int64), g13["b/pred"].astype(np.int64), g13["b/coords"].astype(np.float64)
    dev = torch.device("cuda")
    host = E.get_detections(gt, pred, 0.5, -1)
    devr = E.get_detections(torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev), 0.5, -1)
    for a, b in zip(host, devr):
        np.testing.assert_array_equal(a, b)
    ug, up = np.arange(host[2].shape[1]), host[2].argmax(axis=0)
    gm, pm = maps(gt, pred)
    a = E.evaluate_xy_partition_arrays(pred, gt, ug, up, xyz, PART, gm, pm)
    b = E.evaluate_xy_partition_arrays(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(ug).to(dev),
                                       torch.from_numpy(up).to(dev), torch.from_numpy(xyz.astype(np.float32)).to(dev), PART, gm, pm)
    check_frame(b, a, "device xy")
    gt4 = g13["c/gt"].astype(np.float64); pr4 = g13["c/pred"].astype(np.float64)
    r1, p1 = E.evaluate_forest(gt4[:, :3], gt4[:, 3], pr4[:, :3], pr4[:, 3], frames=False)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
    r2, p2 = E.evaluate_forest(T(gt4[:, :3]), T(gt4[:, 3]), T(pr4[:, :3].astype(np.float32)), T(pr4[:, 3].astype(np.int64)), frames=False)
    np.testing.assert_array_equal(p1, p2)
    for k, v in r1["detection_results"].items():
        np.testing.assert_array_equal(np.asarray(v), np.asarray(r2["detection_results"][k]), err_msg=k)
    check_frame(r2["segmentation_results"]["z_partition"], r1["segmentation_results"]["z_partition"], "device z")


def test_edge_cases_raise_value_error():
    from treelearn_amd.util import eval as E
    rng = np.random.default_rng(1)
    gt = np.repeat([-1, 0, 1], [20, 30, 4])
    pred = gt.copy()
    xyz = rng.random((len(gt), 3))
    with pytest.raises(ValueError, match="has 4 points"):
        E.evaluate_z_partition_arrays(pred, gt, np.array([0, 1]), np.array([0, 1]), xyz, PART, {0: 1, 1: 2}, {0: 1, 1: 2})
    with pytest.raises(ValueError, match="not the non-tree label"):
        E.get_detections(np.where(gt == 1, -2, gt), pred, 0.5, -1)
    with pytest.raises(ValueError, match="mismatched lengths"):
        E.get_detections(gt, pred[:-1], 0.5, -1)
    with pytest.raises(ValueError, match="mismatched lengths"):
        E.evaluate_xy_partition_arrays(pred, gt, np.array([0]), np.array([0]), xyz[:-1], PART, {0: 1}, {0: 1})
    with pytest.raises(ValueError, match="no predicted tree"):
        E.evaluate_forest(xyz, gt + 1, xyz, np.zeros(len(gt)))


def test_dataframe_round_trip(g13):
    pd = pytest.importorskip("pandas")
    from treelearn_amd.util import eval as E
    gt, pred, xyz = g13["a/merge/gt"].astype(np.int64), g13["a/merge/pred"].astype(np.int64), g13["a/merge/coords"].astype(np.float64)
    _, _, iou, _, _ = E.get_detections(gt, pred, 0.5, -1)
    ug, up = np.arange(iou.shape[1]), iou.argmax(axis=0)
    gm, pm = maps(gt, pred)
    df = E.evaluate_xy_partition(pred, gt, ug, up, xyz, PART, gm, pm)
    assert isinstance(df, pd.DataFrame) and "prec_intvl0_0.1" in df.columns and "iou_intvl0.9_1" in df.columns
    check_frame({c: df[c].to_numpy() for c in df.columns}, frame(g13, "a/merge/xy_partition"), "frame")
    no = E.evaluate_no_partition(pred, gt, ug, up, gm, pm)
    check_frame({c: no[c].to_numpy() for c in no.columns}, frame(g13, "a/merge/no_partition"), "frame no")
