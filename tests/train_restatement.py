"""CPU / torch restatement of the reference's `pointwise_eval` (tools/training/train.py:89-102) and of the lists its `validate` (:61-86)
concatenates for it: what treelearn_amd.util.trainer and tl_pointwise_eval are checked against.  The reference's own function is
`@cuda_cast` and needs its package; this one runs anywhere.

  masks_off = semantic_labels == TREE                      (:92)
  offset loss = mean over masks_off of sqrt(sum((offset_predictions.float() - offset_labels)^2, 1)), `0 * sum` = 0 without such a row
               (util/train.py:159-164) -- the per-row norms in fp32 as there, their mean in float64
  tree_pred   = softmax(logits.float(), -1)[:, TREE] >= 0.5 (:98)
  tp, fp, tn, fn as get_eval_components (util/eval.py:230-238); acc = (tp + tn) / (tp + fp + fn + tn)   (:101-102)
"""
import numpy as np
import torch

TREE_CLASS_IN_DATASET = 0
TREE_CONF_THRESHOLD = 0.5


def pointwise_eval(semantic_prediction_logits, offset_predictions, semantic_labels, offset_labels):
    """CPU tensors in, dict(tp, fp, tn, fn, n_off, offset_mae, acc) out."""
    logits = semantic_prediction_logits.detach().cpu().float()
    offsets = offset_predictions.detach().cpu().float()
    sem = semantic_labels.detach().cpu().long()
    lab = offset_labels.detach().cpu().float()
    masks_off = sem == TREE_CLASS_IN_DATASET
    n_off = int(masks_off.sum())
    if n_off == 0:
        offset_mae = 0.0
    else:
        per_row = (offsets[masks_off] - lab[masks_off]).pow(2).sum(1).sqrt()              # fp32, as the reference's loss
        offset_mae = float(per_row.double().mean())
    if len(logits):
        tree_pred = (logits.softmax(dim=-1)[:, TREE_CLASS_IN_DATASET] >= TREE_CONF_THRESHOLD).numpy()
    else:
        tree_pred = np.zeros(0, bool)
    tree = (sem == TREE_CLASS_IN_DATASET).numpy()
    tp = int((tree_pred & tree).sum()); fp = int((tree_pred & ~tree).sum())
    fn = int((~tree_pred & tree).sum()); tn = int((~tree_pred & ~tree).sum())
    total = tp + fp + fn + tn
    return dict(tp=tp, fp=fp, tn=tn, fn=fn, n_off=n_off, offset_mae=offset_mae, acc=(tp + tn) / total if total else float("nan"))


def gather_for_validate(outputs_and_batches):
    """validate's lists (:72-75): per tile the rows with masks_sem, concatenated in tile order."""
    cols = [[], [], [], []]
    for output, batch in outputs_and_batches:
        m = batch["masks_sem"].cpu()
        for c, t in zip(cols, (output["semantic_prediction_logits"], output["offset_predictions"], batch["semantic_labels"], batch["offset_labels"])):
            c.append(t.detach().cpu()[m])
    return [torch.cat(c, 0) for c in cols]
