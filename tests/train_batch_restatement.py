"""numpy restatement of one dataset item and of collate (reference tree_learn/dataset/dataset.py:34-140,167-226), the yardstick of
tests/test_gpu_train_batch.py and tests/test_gpu_device_loader.py.  It follows the reference statement by statement (float32 test items, float64
training items, numpy's own float32 mean) with ONE explicit switch: `rank3=True` takes the start of the tree base as np.sort(z)[3] -- the rule of
tl_train_item -- where the reference takes np.partition(z, 10)[3], an implementation-defined element among the ten lowest."""
import numpy as np

IGNORE, NON_TREE_RAW = -1, 0
NON_TREE, TREE = 1, 0


def low_of(z, rank3):
    if len(z) > 11:
        return np.sort(z)[3] if rank3 else np.partition(z, 10)[3]
    return z.min()


def offset_labels(xyz, inst, sem, rank3=True):
    """dataset.py:111-140.  Returns (offsets, valid, position f32[n,3], info) -- info: per tree instance label -> dict(rows, n_base,
    max_abs_base, numpy_pick_is_rank3)."""
    position = np.ones_like(xyz, dtype=np.float32)
    valid = np.zeros(len(xyz), dtype=bool)
    info = {}
    order = np.argsort(inst, kind="stable")                                  # one group of rows per label, rows in file order
    for sel in np.split(order, np.flatnonzero(np.diff(inst[order])) + 1) if len(inst) else []:
        label = inst[sel[0]]
        if sem[sel[0]] == NON_TREE:
            continue
        pts = xyz[sel]
        z = pts[:, 2]
        low = low_of(z, rank3)
        base = pts[z <= low + 0.5]
        if len(base):
            position[sel] = np.mean(base, axis=0)
            valid[sel] = True
        else:
            position[sel] = 0.0
        info[int(label)] = dict(rows=sel, n_base=len(base), max_abs_base=float(np.abs(base).max()) if len(base) else 0.0,
                                numpy_pick_is_rank3=bool(len(z) <= 11 or np.partition(z, 10)[3] == np.sort(z)[3]))
    return position - xyz, valid, position, info


def item(points, instance_label, inner_square_edge_length, m=None, center=None, rank3=True):
    """dataset.py:34-76 for one crop: `m` = the float64 matrix of a training item (dataset.py:85-89), None = test mode.  numpy arrays with the
    item's own dtypes, plus `position` and `info` of offset_labels."""
    xyz = np.asarray(points, np.float32)
    inst = np.asarray(instance_label)
    sem = np.empty(len(inst))
    sem[inst == NON_TREE_RAW] = NON_TREE
    sem[inst != NON_TREE_RAW] = TREE
    cen = np.ones_like(xyz) if m is not None else np.ones_like(xyz) * np.asarray(center)
    if m is not None:
        xyz = np.matmul(xyz, np.asarray(m, np.float64))
    off, valid, position, info = offset_labels(xyz, inst, sem, rank3)
    inf_norm = np.linalg.norm(xyz[:, :-1], ord=np.inf, axis=1)
    m_inner = inf_norm <= (inner_square_edge_length / 2)
    not_ignore = np.logical_not(inst == IGNORE)
    m_off = m_inner & not_ignore & (sem != NON_TREE) & valid
    m_sem = m_inner & not_ignore
    return dict(xyz=xyz, instance_label=inst, semantic_label=sem, pt_offset_label=off, center=cen, mask_inner=m_inner, mask_off=m_off,
                mask_sem=m_sem, position=position, info=info, inf_norm=inf_norm)


def collate(items):
    """dataset.py:167-226 on restated items: the batch dict as numpy arrays with the tensors' dtypes."""
    cat = lambda k, dt: np.concatenate([np.asarray(it[k]) for it in items], 0).astype(dt)                 # noqa: E731
    return {
        "coords": cat("xyz", np.float32),
        "batch_ids": np.concatenate([np.full(len(it["xyz"]), b, np.int64) for b, it in enumerate(items)]),
        "semantic_labels": cat("semantic_label", np.int64),
        "instance_labels": cat("instance_label", np.int64),
        "masks_inner": cat("mask_inner", bool),
        "masks_off": cat("mask_off", bool),
        "masks_sem": cat("mask_sem", bool),
        "offset_labels": cat("pt_offset_label", np.float32),
        "centers": cat("center", np.float32),
        "batch_size": len(items),
    }


def ulp32(v):
    """One float32 unit in the last place at the magnitude of v."""
    return np.spacing(np.abs(np.asarray(v)).astype(np.float32)).astype(np.float64)


def position_tolerance(it):
    """Per row: n_base * 2^-24 * max|coordinate among the instance's base rows| -- the textbook bound of a sequential float32 sum of n_base
    terms against the exact sum, divided by n_base -- computed from the host data.  Zero for non-tree rows."""
    tol = np.zeros(len(it["xyz"]))
    for d in it["info"].values():
        tol[d["rows"]] = d["n_base"] * 2.0 ** -24 * d["max_abs_base"]
    return tol
