"""Plain numpy float64 form of the three stages every segmented forest passes through after the network (DESIGN §"Post-network
stages"): the k-NN majority vote (csrc/tl_knn.hip, util/postprocess.knn_vote), the ensemble's group mean (csrc/tl_prepare.hip
k_group_mean, util/postprocess.ensemble) and the eps-grouping (csrc/tl_cluster.hip, cluster.dbscan_min2).  This file is the
specification the kernels are compared with: no cell grids, no early exits, nothing imported from the package.

All distances are float64 on the float32 inputs, d = (dx*dx + dy*dy) + dz*dz with numpy's separate multiplies and adds (no fma)."""
import numpy as np

BLOCK = 256


# ============================================================================================ k-NN vote
def _vote(labels):
    """Most frequent label; ties go to the smallest label (np.unique sorts ascending, argmax takes the first maximum)."""
    vals, cnt = np.unique(labels, return_counts=True)
    return vals[np.argmax(cnt)]


def knn_order(ref_f32, qry_f32, k):
    """int64 [nq, min(k, nr)]: reference indices of every query's nearest rows, ordered by (d, reference index); and their d."""
    ref = np.asarray(ref_f32, dtype=np.float32).astype(np.float64)
    qry = np.asarray(qry_f32, dtype=np.float32).astype(np.float64)
    nr, nq = len(ref), len(qry)
    kk = min(int(k), nr)
    idx = np.empty((nq, kk), dtype=np.int64)
    dist = np.empty((nq, kk), dtype=np.float64)
    for a in range(0, nq, BLOCK):
        e = min(a + BLOCK, nq)
        dx = ref[None, :, 0] - qry[a:e, None, 0]
        dy = ref[None, :, 1] - qry[a:e, None, 1]
        dz = ref[None, :, 2] - qry[a:e, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        o = np.argsort(d, axis=1, kind="stable")[:, :kk]              # stable: equal d keep ascending reference index
        idx[a:e] = o
        dist[a:e] = np.take_along_axis(d, o, axis=1)
    return idx, dist


def knn_vote(ref_f32, lab, qry_f32, k):
    if k < 1:
        raise ValueError(f"Expected n_neighbors > 0. Got {k}")
    if k > len(ref_f32):
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {len(ref_f32)}")
    lab = np.asarray(lab, dtype=np.int64)
    idx, _ = knn_order(ref_f32, qry_f32, k)
    return np.array([_vote(lab[row]) for row in idx], dtype=np.int64).reshape(len(idx))


def knn_has_tie_at_k(ref_f32, qry_f32, k):
    """True where the k-th and (k+1)-th smallest distances of a query are equal: the k nearest are then a matter of index order."""
    if k >= len(ref_f32):
        return np.zeros(len(qry_f32), dtype=bool)
    _, dist = knn_order(ref_f32, qry_f32, k + 1)
    return dist[:, k - 1] == dist[:, k]


# ============================================================================================ group mean / ensemble
def group_mean(src_f32, sorted_keys, perm):
    """(mean f64 [G, C], first_idx i64 [G]): groups are the runs of equal sorted keys; per column the float64 sum of the members in
    perm order, one after the other, then / count."""
    src = np.asarray(src_f32, dtype=np.float32).astype(np.float64)
    keys = np.asarray(sorted_keys, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    n = len(keys)
    start = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    count = np.diff(np.concatenate([start, [n]]))
    rows = src[perm]                                                   # members in perm order
    acc = np.zeros((len(start), src.shape[1]), dtype=np.float64)
    for t in range(int(count.max())):                                  # t-th member of every group that has one: left-to-right sums
        live = np.flatnonzero(count > t)
        acc[live] = acc[live] + rows[start[live] + t]
    return acc / count[:, None].astype(np.float64), perm[start]


def ensemble_keys(coords):
    """(q f32 [n, 3], sorted int64 keys, perm): float32 rint(x * 100), lexicographic (x, y, z), stable."""
    c = np.asarray(coords).astype(np.float32)
    q = np.rint(c * np.float32(100.0)).astype(np.float32)
    qi = q.astype(np.int64)
    perm = np.lexsort((qi[:, 2], qi[:, 1], qi[:, 0]))                  # stable; the last key is the primary one
    s = qi[perm]
    new = np.concatenate([[True], (s[1:] != s[:-1]).any(1)])
    return q, np.cumsum(new).astype(np.int64) - 1, perm.astype(np.int64)


def ensemble(coords, semantic_scores, semantic_labels, offset_predictions, offset_labels, instance_labels, feats, input_feats):
    n = len(coords)
    q, keys, perm = ensemble_keys(coords)
    cols = [semantic_scores, semantic_labels, offset_predictions, offset_labels, instance_labels, feats, input_feats]
    mats = [np.asarray(a).reshape(n, -1).astype(np.float32) for a in cols]
    widths = np.cumsum([m.shape[1] for m in mats])[:-1]
    mean, first = group_mean(np.concatenate(mats, 1), keys, perm)
    p = np.split(mean, widths, axis=1)
    f32 = lambda t, a: (t[:, 0] if np.asarray(a).ndim == 1 else t).astype(np.float32)          # noqa: E731
    i64 = lambda t: t[:, 0].astype(np.int64)                                                    # noqa: E731  (truncation)
    return ((q[first] / np.float32(100.0)).astype(np.float32), f32(p[0], semantic_scores), i64(p[1]), f32(p[2], offset_predictions),
            f32(p[3], offset_labels), i64(p[4]), f32(p[5], feats), f32(p[6], input_feats))


# ============================================================================================ DBSCAN(eps, min_samples = 2)
def dbscan_min2(xy_f32, eps):
    """Connected components of the graph dx*dx + dy*dy <= eps*eps (full n x n float64 matrix); isolated points -1; clusters numbered
    by their smallest member index."""
    xy = np.asarray(xy_f32, dtype=np.float32).astype(np.float64)
    n = len(xy)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    dx = xy[None, :, 0] - xy[:, None, 0]
    dy = xy[None, :, 1] - xy[:, None, 1]
    adj = dx * dx + dy * dy <= np.float64(eps) * np.float64(eps)
    np.fill_diagonal(adj, False)
    comp = np.full(n, -1, dtype=np.int64)                              # smallest member index of the component, by flooding
    for s in range(n):
        if comp[s] >= 0 or not adj[s].any():
            continue
        comp[s] = s
        front = np.array([s])
        while len(front):
            nxt = np.flatnonzero(adj[front].any(0) & (comp < 0))
            comp[nxt] = s
            front = nxt
    roots = np.unique(comp[comp >= 0])                                 # ascending smallest member = the numbering
    out = np.full(n, -1, dtype=np.int64)
    live = comp >= 0
    out[live] = np.searchsorted(roots, comp[live])
    return out
