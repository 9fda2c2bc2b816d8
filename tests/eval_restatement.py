"""The forest-scoring protocol (reference tree_learn/util/eval.py) restated in vectorised numpy, as the tests' second opinion on
treelearn_amd.util.eval.  No GPU: the contingency table is one np.bincount, the bands are counted per (gt, pred) pair over the points
of that pair only (stable CSR by label), in the reference's summation order where the order matters (the tree position)."""
import numpy as np


def contingency(pred, gt, n_pred, n_gt, non_tree=-1):
    """[(n_pred + 1), (n_gt + 1)] counts: row 0 = negative preds, column 0 = non-tree or negative gt (tl_eval_contingency's layout)."""
    pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
    r = np.where(pred < 0, 0, pred + 1)
    c = np.where((gt < 0) | (gt == non_tree), 0, gt + 1)
    ok = (r <= n_pred) & (c <= n_gt)
    return np.bincount(r[ok] * (n_gt + 1) + c[ok], minlength=(n_pred + 1) * (n_gt + 1)).reshape(n_pred + 1, n_gt + 1)


def scores(tp, fp, fn):
    tp, fp, fn = (np.asarray(a, np.int64) for a in (tp, fp, fn))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.where(tp + fp == 0, np.nan, tp / (tp + fp)), np.where(tp + fn == 0, np.nan, tp / (tp + fn)),
                np.where(tp + fp + fn == 0, np.nan, tp / (tp + fp + fn)))


def detection_matrices(labels, preds, non_tree):
    """iou, precision, recall [max pred + 1, max label + 1]; 0 where a pred holds no point of the tree."""
    T = contingency(preds, labels, int(np.max(preds)) + 1, int(np.max(labels)) + 1, non_tree)
    C = T[1:, 1:]
    R, S = T[1:].sum(1, keepdims=True), T[:, 1:].sum(0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.where(C > 0, C / (R + S - C), 0.0), np.where(C > 0, C / R, 0.0), np.where(C > 0, C / S, 0.0))


def get_detections(labels, preds, min_iou, non_tree):
    from scipy.optimize import linear_sum_assignment
    iou, prec, rec = detection_matrices(labels, preds, non_tree)
    r, c = linear_sum_assignment(iou, maximize=True)
    ok = iou[r, c] > min_iou
    return c[ok], r[ok], iou, prec, rec


def no_partition(preds, labels, unique_gts, unique_preds):
    """prec, rec, iou of each pair over whole trees."""
    preds, labels = np.asarray(preds, np.int64), np.asarray(labels, np.int64)
    g, p = np.asarray(unique_gts, np.int64), np.asarray(unique_preds, np.int64)
    T = contingency(preds, labels, max(preds.max(), p.max()) + 1, max(labels.max(), g.max()) + 1, -1)
    C = T[p + 1, g + 1]
    return scores(C, T[p + 1].sum(1) - C, T[:, g + 1].sum(0) - C)


def _csr(labels):
    order = np.argsort(labels, kind="stable")
    n = int(labels.max()) + 1 if len(labels) else 0
    start = np.searchsorted(labels[order], np.arange(n + 1))
    return order, start


def partition_counts(preds, labels, coords, unique_gts, unique_preds, edges, mode):
    """tp, fp, fn [m, len(edges) - 1] and the normaliser [m, 3] per (gt, pred) pair; mode 'xy' or 'z'."""
    preds, labels = np.asarray(preds, np.int64), np.asarray(labels, np.int64)
    coords = np.ascontiguousarray(coords, np.float64)
    go, gs = _csr(labels)
    po, ps = _csr(preds)
    edges = list(edges)
    k = len(edges) - 1
    pairs = list(zip(np.asarray(unique_gts).tolist(), np.asarray(unique_preds).tolist()))
    tp, fp, fn = (np.zeros((len(pairs), k), np.int64) for _ in range(3))
    norm = np.zeros((len(pairs), 3))
    for j, (g, p) in enumerate(pairs):
        gi = go[gs[g]:gs[g + 1]]
        pi = po[ps[p]:ps[p + 1]] if p < len(ps) - 1 else np.zeros(0, np.int64)
        pi = pi[labels[pi] != g]
        tree = coords[gi]
        zmin = np.min(tree[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):                    # a zero normaliser divides as IEEE says, as in the reference
            if mode == "xy":
                pos = np.mean(tree[tree[:, 2] <= zmin + 0.30], axis=0)[:2]      # (n, 3) row after row, as the reference
                dist = lambda idx: np.linalg.norm(coords[idx, :2] - pos, axis=1)    # noqa: E731
                regmax = np.sort(dist(gi))[-5]
                vg, vp = dist(gi) / regmax, dist(pi) / regmax
                norm[j] = (pos[0], pos[1], regmax)
            else:
                regmax = np.sort(tree[:, 2])[-5]
                d = regmax - zmin
                vg, vp = (coords[gi, 2] - zmin) / d, (coords[pi, 2] - zmin) / d
                norm[j] = (zmin, regmax, 0.0)
        hit = preds[gi] == p
        for i in range(k):
            bg = (vg >= edges[i]) & (vg < edges[i + 1])
            tp[j, i] = (bg & hit).sum()
            fn[j, i] = (bg & ~hit).sum()
            fp[j, i] = ((vp >= edges[i]) & (vp < edges[i + 1])).sum()
    return tp, fp, fn, norm


def partition(preds, labels, coords, unique_gts, unique_preds, edges, mode):
    """{'prec_intvl{lo}_{hi}': ..., 'rec_...', 'iou_...'} float64 [m] columns."""
    tp, fp, fn, _ = partition_counts(preds, labels, coords, unique_gts, unique_preds, edges, mode)
    pr, rc, io = scores(tp, fp, fn)
    edges = list(edges)
    out = {}
    for name, v in (("prec", pr), ("rec", rc), ("iou", io)):
        for i in range(len(edges) - 1):
            out[f"{name}_intvl{edges[i]}_{edges[i + 1]}"] = v[:, i]
    return out


def perturb(labels, coords, seed, noise=0.05):
    """A segmentation to score: ground-truth ids (0 = non-tree, trees >= 1) with tree 2 merged into tree 1, tree 3 split in x at its
    median, and a fraction `noise` of the points relabelled at random."""
    rng = np.random.default_rng(seed)
    labels = np.asarray(labels, np.int64)
    pred = labels.copy()
    ids = np.unique(labels[labels > 0])
    pred[labels == ids[1]] = ids[0]
    t3 = labels == ids[2]
    pred[t3 & (coords[:, 0] > np.median(coords[t3, 0]))] = ids.max() + 1
    flip = rng.random(len(pred)) < noise
    pred[flip] = rng.choice(np.concatenate([[0], ids]), flip.sum())
    return pred


# ------------------------------------------------------------------------------------------------ the inputs of G13 (b) and (c)
# Their point clouds are rebuilt here from the repository's synthetic generator instead of being stored: the fixture keeps the reference's
# outputs and a digest of the inputs it was made from, and load_g13 refuses a rebuild whose digest differs.
def consecutive(orig):
    """Reference evaluate()'s relabelling: non-tree (0) -> -1, trees -> 0, 1, ... in ascending order of their ids."""
    lab = np.where(np.asarray(orig, np.int64) == 0, -1, np.asarray(orig, np.int64))
    m = lab != -1
    lab[m] = np.searchsorted(np.unique(lab[m]), lab[m])
    return lab


def tile_case_inputs():
    """G13 (b): a 24 m tile (about 154 k points, 22 trees) and a perturbed segmentation of it, consecutive labels."""
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=24.0, voxel=0.2, n_trees=22, fill=0.15, seed=3)
    coords = t["points"].astype(np.float64)
    gt0 = t["instance_label"].astype(np.int64)
    return coords, consecutive(gt0), consecutive(perturb(gt0, coords, seed=4))


def evaluate_case_inputs(margin_ok=None):
    """G13 (c): ground truth (x y z id, 0 = non-tree, ids with gaps) and a prediction cloud that is a jittered 70 % subsample with a merge,
    a split and label noise, both N x 4 float64 of float32 values.  margin_ok: the ground-truth points kept (5-NN margin, see the generator)."""
    from treelearn_amd.synth import make_tile
    rng = np.random.default_rng(11)
    t = make_tile(extent=12.0, voxel=0.2, n_trees=8, fill=0.12, seed=5)
    gxyz = t["points"].astype(np.float32)
    glab = t["instance_label"].astype(np.int64) * 10
    keep = rng.random(len(gxyz)) < 0.7
    pxyz = (gxyz[keep] + rng.normal(0, 0.005, (keep.sum(), 3))).astype(np.float32)
    plab = perturb(glab[keep], pxyz.astype(np.float64), seed=12) * 7
    if margin_ok is not None:
        gxyz, glab = gxyz[margin_ok], glab[margin_ok]
    return (np.column_stack([gxyz.astype(np.float64), glab.astype(np.float64)]),
            np.column_stack([pxyz.astype(np.float64), plab.astype(np.float64)]))


def digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def load_g13(path):
    """tests/golden/g13_eval.npz with the rebuilt inputs of (b) and (c) filled in under the keys the cases use."""
    with np.load(path) as z:
        g = {k: z[k] for k in z.files}
    coords, gt, pred = tile_case_inputs()
    assert digest(coords, gt, pred) == str(g["b/inputs_sha256"]), "G13 (b): the rebuilt tile differs from the one the fixture was made from"
    g["b/coords"], g["b/gt"], g["b/pred"] = coords, gt, pred
    ok = np.unpackbits(g["c/margin_ok_bits"])[:int(g["c/n_points"])].astype(bool)
    gt4, pr4 = evaluate_case_inputs(ok)
    assert digest(gt4, pr4) == str(g["c/inputs_sha256"]), "G13 (c): the rebuilt clouds differ from the ones the fixture was made from"
    g["c/gt"], g["c/pred"] = gt4, pr4
    return g
