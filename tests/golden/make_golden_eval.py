#!/usr/bin/env python3
"""Generate tests/golden/g13_eval.npz (forest scoring) by IMPORTING the reference: tree_learn/util/eval.py and
tools/evaluation/evaluate.py.  Run in the build container only (needs the reference checkout; only the .npz travels):

    python tests/golden/make_golden_eval.py

Reuses make_golden.py's inert mocks for the third-party imports the reference's util package pulls in (laspy, open3d, ...).

(a) hand cases: perfect match, merge, split, a prediction over non-tree points only, a gap in pred ids, a tree predicted entirely
    -1, a tree of exactly 5 points, an IoU tie for the Hungarian step -- every output of the reference's eval functions;
(b) a synthetic tile (~150 k points, ~20 trees) with label noise, a merge and a split -- the same outputs;
The point clouds of (b) and (c) are not stored: tests/eval_restatement.py rebuilds them from treelearn_amd.synth (tile_case_inputs,
evaluate_case_inputs) and checks them against the sha256 digests stored here; (c) stores only the bit mask of the kept points.
(c) the reference's whole evaluate(): load_data / save_data / torch.save / the logger patched, a prediction cloud that is a jittered
    subsample of the ground truth (propagate_preds runs for real, sklearn), and every ground-truth point kept only where its 5th- and
    6th-nearest prediction points are at least 1e-4 apart (relative), so that any exact 5-NN picks the same five.
"""
import importlib.util
import os
import sys
import tempfile
import types
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402,F401  (mocks, reference and repository on sys.path)

from tree_learn.util import eval as ref_eval                                   # noqa: E402
from tree_learn.util.pipeline import make_labels_consecutive                     # noqa: E402
from treelearn_amd.synth import make_tile                                        # noqa: E402
from eval_restatement import digest, evaluate_case_inputs, tile_case_inputs      # noqa: E402

PART = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1]
OUT = {}


def put_frame(prefix, df):
    for c in df.columns:
        OUT[f"{prefix}/{c}"] = df[c].to_numpy()


def scene(sizes, seed, n_ground=60):
    """Trees as point clusters (gt 0, 1, ...; -1 = ground) in float32-exact float64 coordinates."""
    rng = np.random.default_rng(seed)
    pts, lab = [], []
    for t, n in enumerate(sizes):
        c = np.array([4.0 * t, 1.5 * (t % 2), 0.0])
        p = c + rng.normal(0, [0.8, 0.8, 0.0], (n, 3)); p[:, 2] = rng.uniform(0, 8, n)
        pts.append(p); lab.append(np.full(n, t))
    pts.append(np.column_stack([rng.uniform(-2, 4 * len(sizes), n_ground), rng.uniform(-2, 3, n_ground), rng.uniform(0, 0.3, n_ground)]))
    lab.append(np.full(n_ground, -1))
    return np.concatenate(pts).astype(np.float32).astype(np.float64), np.concatenate(lab).astype(np.int64)


def run_reference(key, coords, gt, pred, min_iou=0.5):
    """Every reference function on consecutive labels (-1 = non-tree), as evaluate() calls them."""
    OUT[f"{key}/coords"] = coords.astype(np.float32); OUT[f"{key}/gt"] = gt.astype(np.int32); OUT[f"{key}/pred"] = pred.astype(np.int32)
    OUT[f"{key}/min_iou"] = np.float64(min_iou)
    mg, mp, iou, prec, rec = ref_eval.get_detections(gt, pred, min_iou, -1)
    for k, v in dict(matched_gts=mg, matched_preds=mp, iou=iou, prec=prec, rec=rec).items():
        OUT[f"{key}/{k}"] = v
    fail = ref_eval.get_detection_failures(mg, mp, np.arange(gt.max() + 1), np.arange(pred.max() + 1), iou, prec, rec, 0.5, 0.5)
    for k, v in zip(("non_matched_gts", "non_matched_preds", "nmp_corresponding_gt", "nmg_corresponding_pred", "nmg_corresponding_other_tree"), fail):
        OUT[f"{key}/{k}"] = v
    ug, up = np.arange(iou.shape[1]), iou.argmax(axis=0)
    gmap = {i: i + 1 for i in range(gt.max() + 1)}; gmap[-1] = 0
    pmap = {i: i + 1 for i in range(pred.max() + 1)}; pmap[-1] = 0
    no, xy, z = ref_eval.evaluate_instance_segmentation(pred, gt, ug, up, coords, gmap, pmap, PART, PART)
    put_frame(f"{key}/no_partition", no); put_frame(f"{key}/xy_partition", xy); put_frame(f"{key}/z_partition", z)
    tp, fp, tn, fn = ref_eval.get_eval_components(pred == up[0], gt == 0)
    OUT[f"{key}/components0"] = np.array([tp, fp, tn, fn], np.int64)
    OUT[f"{key}/metrics0"] = np.array(ref_eval.get_segmentation_metrics(tp, fp, fn), np.float64)


def hand_cases():
    rng = np.random.default_rng(7)
    cases = []
    c, g = scene([40, 30, 25], 1); cases.append(("perfect", c, g, g.copy(), 0.5))
    c, g = scene([40, 30, 25], 2); p = g.copy(); p[g == 1] = 0; p[g == 2] = 1; cases.append(("merge", c, g, p, 0.5))
    c, g = scene([40, 30], 3); p = g.copy(); i0 = np.flatnonzero(g == 0); p[i0[len(i0) // 2:]] = 2; cases.append(("split", c, g, p, 0.5))
    c, g = scene([40, 30], 4); p = g.copy(); p[g == -1] = 2; cases.append(("pred_on_non_tree", c, g, p, 0.5))
    c, g = scene([40, 30, 25], 5); p = np.select([g == 0, g == 1, g == 2], [0, 2, 5], -1); cases.append(("pred_id_gap", c, g, p, 0.5))
    c, g = scene([40, 30, 25], 6); p = g.copy(); p[g == 1] = -1; cases.append(("tree_all_minus1", c, g, p, 0.5))
    c, g = scene([40, 5, 30], 7); p = g.copy(); f = rng.random(len(p)) < 0.1; p[f] = rng.integers(-1, 3, f.sum()); cases.append(("five_points", c, g, p, 0.5))
    c, g = scene([40, 30], 8); p = g.copy(); i0 = np.flatnonzero(g == 0); p[i0[:20]] = 0; p[i0[20:]] = 1; p[g == 1] = 2
    cases.append(("iou_tie", c, g, p, 0.3))
    for name, c, g, p, mi in cases:
        run_reference(f"a/{name}", c, g, p, mi)
    OUT["a/cases"] = np.array([x[0] for x in cases])


def relabel(orig):
    lab = orig.astype(np.int64).copy()
    lab[lab == 0] = -1
    m = lab != -1
    lab[m], _ = make_labels_consecutive(lab[m], start_num=0)
    return lab


def tile_case():
    coords, gt, pred = tile_case_inputs()
    t = make_tile(extent=24.0, voxel=0.2, n_trees=22, fill=0.15, seed=3)
    assert np.array_equal(gt, relabel(t["instance_label"]))                 # the restatement's relabelling is the reference's
    run_reference("b", coords, gt, pred)
    for k in ("coords", "gt", "pred"):                                       # rebuilt by the tests (eval_restatement.tile_case_inputs)
        del OUT[f"b/{k}"]
    OUT["b/inputs_sha256"] = np.array(digest(coords, gt, pred))


def evaluate_case():
    from sklearn.neighbors import NearestNeighbors
    gt, pr = evaluate_case_inputs()
    gxyz, pxyz = gt[:, :3].astype(np.float32), pr[:, :3].astype(np.float32)
    nn = NearestNeighbors(n_neighbors=6).fit(pxyz)
    d, _ = nn.kneighbors(gxyz, 6)
    d5, d6 = d[:, 4].astype(np.float64), d[:, 5].astype(np.float64)
    ok = (d6 - d5) >= 1e-4 * np.maximum(d6, 1e-12)
    gt, pr = evaluate_case_inputs(ok)
    d, _ = nn.kneighbors(gt[:, :3].astype(np.float32), 6)
    assert np.all((d[:, 5].astype(np.float64) - d[:, 4]) >= 1e-4 * np.maximum(d[:, 5].astype(np.float64), 1e-12)), "5-NN margin"
    OUT["c/margin_ok_bits"], OUT["c/n_points"] = np.packbits(ok), np.int64(len(ok))       # the clouds themselves are rebuilt by the tests
    OUT["c/inputs_sha256"] = np.array(digest(gt, pr))

    spec = importlib.util.spec_from_file_location("ref_evaluate", "/root/reference/tools/evaluation/evaluate.py")
    ev = importlib.util.module_from_spec(spec); spec.loader.exec_module(ev)
    cap = {}

    def spy(name):
        f = getattr(ev, name)

        def g(*a, **k):
            r = f(*a, **k); cap.setdefault(name, []).append(r); return r
        setattr(ev, name, g)
    for n in ("get_detections", "get_detection_failures", "evaluate_instance_segmentation", "make_labels_consecutive", "propagate_preds"):
        spy(n)
    with tempfile.TemporaryDirectory() as tmp:
        paths = {os.path.join(tmp, "gt.npy"): gt, os.path.join(tmp, "pred", "pred.npy"): pr}
        cfg = types.SimpleNamespace(paths=types.SimpleNamespace(gt_forest_path=os.path.join(tmp, "gt.npy"), pred_forest_path=os.path.join(tmp, "pred", "pred.npy")),
                                    thresholds=types.SimpleNamespace(min_iou_for_match=0.5, min_precision_for_pred=0.5, min_recall_for_gt=0.5),
                                    partitions=types.SimpleNamespace(xy_partition=PART, z_partition=PART))
        saved = {}
        with mock.patch.object(ev, "load_data", lambda p: paths[p].copy()), \
             mock.patch.object(ev, "save_data", lambda data, fmt, name, d: saved.__setitem__(name, data)), \
             mock.patch.object(ev, "get_root_logger", lambda p: mock.MagicMock()), \
             mock.patch.object(ev.torch, "save", lambda obj, p: saved.__setitem__("results", obj)):
            ev.evaluate(cfg)
    res = saved["results"]
    for k, v in res["detection_results"].items():
        OUT[f"c/detection_results/{k}"] = np.asarray(v)
    for k, v in res["segmentation_results"].items():
        if hasattr(v, "columns"):
            put_frame(f"c/segmentation_results/{k}", v)
        else:
            OUT[f"c/segmentation_results/{k}"] = np.asarray(v)
    OUT["c/propagated"] = saved["pred_forest_propagated_to_gt_pointcloud"][:, 3].astype(np.int64)
    # the intermediates evaluate() works from (consecutive ids), for the host-only aggregate test
    mg, mp = cap["get_detections"][0][:2]
    OUT["c/mid/matched_gts"], OUT["c/mid/matched_preds"] = mg, mp
    for i, v in enumerate(cap["get_detection_failures"][0]):
        OUT[f"c/mid/failures{i}"] = v
    put_frame("c/mid/no_partition", cap["evaluate_instance_segmentation"][0][0])
    OUT["c/mid/gt_palette"] = np.array([cap["make_labels_consecutive"][0][1][i] for i in range(len(cap["make_labels_consecutive"][0][1]) - 1)])
    OUT["c/mid/pred_palette"] = np.array([cap["make_labels_consecutive"][1][1][i] for i in range(len(cap["make_labels_consecutive"][1][1]) - 1)])


if __name__ == "__main__":
    hand_cases()
    tile_case()
    evaluate_case()
    path = os.path.join(HERE, "g13_eval.npz")
    np.savez_compressed(path, **OUT)
    print(path, os.path.getsize(path), "bytes,", len(OUT), "arrays")
