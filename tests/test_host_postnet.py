"""The post-network stages without a GPU: the restatement (tests/postnet_restatement.py, the specification of csrc/tl_knn.hip,
k_group_mean of csrc/tl_prepare.hip and csrc/tl_cluster.hip) against the libraries the reference calls on every case of
tests/postnet_cases.py, hand-worked cases, and the preconditions of the ring-bound generator."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postnet_cases as PC  # noqa: E402
import postnet_restatement as R  # noqa: E402

KNN_IDS = [c["id"] for c in PC.knn_cases()]
DB_IDS = [c["id"] for c in PC.dbscan_cases()]
ENS_PANDAS = [c for c in PC.ensemble_cases() if c["pandas"]]            # the mixed-magnitude case is for the GPU alone


# ============================================================================================ 1. against the libraries
@pytest.mark.parametrize("case", PC.knn_cases(), ids=KNN_IDS)
def test_knn_vote_restatement_against_sklearn(case):
    from sklearn.neighbors import KNeighborsClassifier
    ref, lab, qry, k = case["ref"], case["lab"], case["qry"], case["k"]
    want = R.knn_vote(ref, lab, qry, k)
    assert want.shape == (len(qry),) and want.dtype == np.int64
    tie = R.knn_has_tie_at_k(ref, qry, k)
    if case["tie_free"]:
        assert not tie.any(), int(tie.sum())
    else:
        assert tie.any()                                               # the case is there for its ties
    if not case["sklearn"]:
        return
    # sklearn's brute force expands |r - q|^2 = |r|^2 - 2 r.q + |q|^2: centred on the first reference point (exact in float64 for float32
    # inputs, and it leaves every difference unchanged) its error is a few ulp of the largest |x|^2.  Queries whose k-th and (k+1)-th
    # distances are closer than that are left out along with the exact ties.
    c = ref[0].astype(np.float64)
    rc, qc = ref.astype(np.float64) - c, qry.astype(np.float64) - c
    assert np.array_equal(rc + c, ref.astype(np.float64)) and np.array_equal(qc + c, qry.astype(np.float64))
    if k < len(ref):
        _, d = R.knn_order(ref, qry, k + 1)
        band = 64 * np.finfo(np.float64).eps * max(float((rc * rc).sum(1).max()), float((qc * qc).sum(1).max()), 1e-300)
        clear = (d[:, k] - d[:, k - 1]) > band
    else:
        clear = np.ones(len(qry), dtype=bool)
    assert not (clear & tie).any()
    if case["tie_free"]:
        assert clear.mean() > 0.95                                     # nearly every query of a tie-free case is compared
    if clear.any():
        got = KNeighborsClassifier(n_neighbors=k, algorithm="brute").fit(rc, lab).predict(qc[clear])
        assert np.array_equal(got, want[clear]), int((got != want[clear]).sum())


@pytest.mark.parametrize("case", PC.dbscan_cases(), ids=DB_IDS)
def test_dbscan_restatement_against_sklearn(case):
    from sklearn.cluster import DBSCAN
    want = R.dbscan_min2(case["xy"], case["eps"])
    got = DBSCAN(eps=case["eps"], min_samples=2).fit(case["xy"].astype(np.float64)).labels_
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", ENS_PANDAS, ids=[c["id"] for c in ENS_PANDAS])
def test_ensemble_restatement_against_pandas(case):
    """The reference function's arithmetic (util/pipeline.py ensemble: concat, round x, y, z to 2 decimals, groupby, mean, casts)."""
    pd = pytest.importorskip("pandas")
    a = {k: case[k] for k in PC.ENSEMBLE_KEYS}
    n = len(a["coords"])
    names, frames = {}, []
    for key in PC.ENSEMBLE_KEYS:
        m = a[key].reshape(n, -1)
        names[key] = [f"{key}{i}" for i in range(m.shape[1])] if key != "coords" else ["x", "y", "z"]
        frames.append(pd.DataFrame(m, columns=names[key]))
    df = pd.concat(frames, axis=1).round({"x": 2, "y": 2, "z": 2})
    grouped = df.groupby(["x", "y", "z"]).mean().reset_index()
    want = R.ensemble(*[a[k] for k in PC.ENSEMBLE_KEYS])
    assert len(grouped) == case["n_groups"] == len(want[0])
    for key, w in zip(PC.ENSEMBLE_KEYS, want):
        g = grouped[names[key]].to_numpy()
        if key in ("semantic_labels", "instance_labels"):
            assert w.dtype == np.int64 and np.array_equal(g.astype("int64").flatten(), w), key          # exact
        else:
            g = g.astype("float32")
            assert w.dtype == np.float32 and g.shape == w.shape, key
            ulp = np.spacing(np.abs(w))                                                                   # pandas may sum differently
            assert (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= ulp).all(), key


# ============================================================================================ 2. by hand
def test_knn_vote_by_hand():
    # five points on the x axis; the query at 0.9 sees, in order, 1 (d 0.1), 0 (0.9), 2 (1.1), 3 (2.1), 10 (9.1)
    ref = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], dtype=np.float32)
    lab = np.array([4, 9, 4, -2, -2])
    q = np.array([[0.9, 0, 0]], dtype=np.float32)
    idx, d = R.knn_order(ref, q, 5)
    assert idx.tolist() == [[1, 0, 2, 3, 4]] and (np.diff(d[0]) > 0).all()
    assert [int(R.knn_vote(ref, lab, q, k)[0]) for k in (1, 2, 3, 4, 5)] == [9, 4, 4, 4, -2]
    #   k = 1: {9}; k = 2: {9, 4} tie -> 4; k = 3: {9, 4, 4}; k = 4: {9, 4, 4, -2}; k = 5: two 4s and two -2s -> the smaller, -2
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        R.knn_vote(ref, lab, q, 6)
    with pytest.raises(ValueError, match="n_neighbors > 0"):
        R.knn_vote(ref, lab, q, 0)


def test_knn_distance_ties_go_to_the_earlier_reference_row():
    # the query is the centre of a square: four distances of exactly 0.5; k = 1 takes row 0, k = 3 rows 0, 1, 2
    ref = np.array([[0.5, 0.5, 0], [-0.5, 0.5, 0], [0.5, -0.5, 0], [-0.5, -0.5, 0]], dtype=np.float32)
    q = np.zeros((1, 3), dtype=np.float32)
    assert R.knn_has_tie_at_k(ref, q, 1)[0] and R.knn_has_tie_at_k(ref, q, 3)[0] and not R.knn_has_tie_at_k(ref, q, 4)[0]
    assert int(R.knn_vote(ref, [8, 1, 1, 1], q, 1)[0]) == 8
    assert int(R.knn_vote(ref, [8, 8, 1, 1], q, 3)[0]) == 8
    assert int(R.knn_vote(ref[::-1], [8, 8, 1, 1][::-1], q, 3)[0]) == 1


def test_group_mean_by_hand_and_the_49_row_group():
    src = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]], dtype=np.float32)
    keys = np.array([3, 3, 3, 9]); perm = np.array([2, 0, 3, 1])      # group 3 = rows 2, 0, 3; group 9 = row 1
    mean, first = R.group_mean(src, keys, perm)
    assert mean.tolist() == [[13.0 / 3.0, 130.0 / 3.0], [2.0, 20.0]] and first.tolist() == [2, 1]
    # 49 rows that all carry L: sum / count is L exactly; the product with the reciprocal falls below L for 1401 of the labels 0..2999
    L = np.arange(3000)
    below = np.array([int(np.float64(v * 49) * (1.0 / 49.0)) != v for v in L])
    assert below.sum() == 1401 and np.flatnonzero(below)[:8].tolist() == [1, 2, 3, 4, 6, 7, 8, 12]
    differ = [c for c in range(1, 101) if any(int(np.float64(v * c) * (1.0 / c)) != v for v in L)]
    assert differ == [49, 98]                                          # 49 alone among the group sizes 1..64
    for v in (1, 7, 12, 2999):
        mean, _ = R.group_mean(np.full((49, 1), v, dtype=np.float32), np.zeros(49, dtype=np.int64), np.arange(49))
        assert mean[0, 0] == v and int(mean[0, 0]) == v


def test_group_mean_adds_in_perm_order():
    # 1e8 + 1 - 1e8 in float64 is exact either way, so use magnitudes where the order shows: (2^60 + 1) - 2^60 = 0, 2^60 - 2^60 + 1 = 1
    big = np.float32(2.0 ** 60)
    src = np.array([[big], [1.0], [-big]], dtype=np.float32)
    keys = np.zeros(3, dtype=np.int64)
    assert R.group_mean(src, keys, np.array([0, 1, 2]))[0][0, 0] == 0.0
    assert R.group_mean(src, keys, np.array([0, 2, 1]))[0][0, 0] == 1.0 / 3.0


def test_ensemble_by_hand():
    coords = np.array([[1.004, 2.0, -0.004], [0.996, 2.0, 0.004], [1.006, 2.0, 0.0], [-1.0, 0.0, 0.0]], dtype=np.float32)
    one = lambda w: np.arange(4 * w, dtype=np.float32).reshape(4, w)                                  # noqa: E731
    out = R.ensemble(coords, one(2), np.array([1, 1, 0, 1]), one(3), one(3), np.array([5, 5, 6, 2]), one(32), one(1))
    # rows 0 and 1 round to (1.00, 2.00, 0.00) from both sides, row 2 to 1.01; the output is ordered by (x, y, z)
    assert np.array_equal(out[0], np.array([[-1, 0, 0], [1.0, 2, 0], [1.01, 2, 0]], dtype=np.float32))
    assert out[2].tolist() == [1, 1, 0] and out[5].tolist() == [2, 5, 6]
    assert out[1].tolist() == [[6, 7], [1, 2], [4, 5]] and out[7].tolist() == [[3], [0.5], [2]]
    assert [o.dtype for o in out] == [np.float32, np.float32, np.int64, np.float32, np.float32, np.int64, np.float32, np.float32]
    # a mean label of 0.5 truncates to 0 (and -0.5 would, too: astype truncates toward zero)
    out = R.ensemble(coords[:2], one(2)[:2], np.array([1, 0]), one(3)[:2], one(3)[:2], np.array([3, 4]), one(32)[:2], one(1)[:2])
    assert out[2].tolist() == [0] and out[5].tolist() == [3]


def test_dbscan_by_hand():
    # 0 - 1 - 2 chained by 0.1 steps, 3 alone, 4 - 5 a pair whose distance is exactly eps
    xy = np.array([[0, 0], [0.1, 0], [0.2, 0], [5, 5], [1.0, 1.0], [1.0, 1.25]], dtype=np.float32)
    assert R.dbscan_min2(xy, 0.25).tolist() == [0, 0, 0, -1, 1, 1]
    assert R.dbscan_min2(xy, 0.05).tolist() == [-1] * 6
    # numbering by the smallest member: the pair comes first when it holds row 0
    assert R.dbscan_min2(xy[[4, 0, 5, 1, 3, 2]], 0.25).tolist() == [0, 1, 0, 1, -1, 1]
    assert R.dbscan_min2(xy[:1], 0.25).tolist() == [-1] and R.dbscan_min2(xy[:0], 0.25).tolist() == []
    one_ulp = np.array([[0, 0], [np.nextafter(np.float32(0.25), np.float32(1)), 0]], dtype=np.float32)
    assert R.dbscan_min2(one_ulp, 0.25).tolist() == [-1, -1]


def test_dbscan_cases_hold_what_they_are_there_for():
    cases = {c["id"]: c for c in PC.dbscan_cases()}
    lab = R.dbscan_min2(cases["lattice-pitch-equals-eps"]["xy"], 0.25)
    assert (lab == 0).all()                                           # d == eps joins: the whole lattice is one component
    assert (R.dbscan_min2(cases["lattice-pitch-one-ulp-above-eps"]["xy"], 0.25) == -1).all()
    assert (R.dbscan_min2(cases["chain-3000"]["xy"], 0.15) == 0).all()
    sc = cases["scattered-4000"]
    cells = np.unique(np.floor(sc["xy"].astype(np.float64) / sc["eps"]).astype(np.int64), axis=0)
    assert len(cells) > 3900
    lab = R.dbscan_min2(cases["eps015-clumps"]["xy"], 0.15)
    assert lab.max() > 50 and (lab == -1).sum() > 100


# ============================================================================================ 3. the ring-bound generator
@pytest.mark.parametrize("lo", [-5000.0, -50000.0])
def test_ring_bound_preconditions_hold(lo):
    q, p, p2, c, h = PC.ring_bound_points(lo)                          # asserts the cells and the two inequalities itself
    inv_h = np.float32(1.0) / h
    cell = lambda x: int(np.floor((np.float32(x) - np.float32(lo)) * inv_h))                          # noqa: E731
    assert (cell(q), cell(p)) == (c, c + 2) and cell(p2) in (c - 1, c)
    gap, d = float(p) - float(q), float(q) - float(p2)
    assert gap < d < PC.RING_MARGIN * float(h)
    # binned in float64 the same points are where the bound assumes them: p, less than one cell edge from q, is at most one ring out
    cell64 = lambda x: int(np.floor((float(x) - float(lo)) * float(inv_h)))                           # noqa: E731
    assert cell64(p) - cell64(q) <= 1


def test_ring_bound_cases_want_the_label_of_the_nearer_point():
    for case in PC.ring_bound_cases():
        assert R.knn_vote(case["ref"], case["lab"], case["qry"], 1).tolist() == [3]                   # p, not p2 (5) or the anchor (7)
