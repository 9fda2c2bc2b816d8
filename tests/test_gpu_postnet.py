"""The post-network stages on the GPU -- tl_knn_vote / tl_knn_vote_grid (csrc/tl_knn.hip), tl_group_mean (csrc/tl_prepare.hip) behind
util/postprocess.ensemble, tl_cluster_grid (csrc/tl_cluster.hip) behind cluster.dbscan_min2 and group_dbscan -- against the float64
restatement of tests/postnet_restatement.py on the cases of tests/postnet_cases.py.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postnet_cases as PC  # noqa: E402
import postnet_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(kind, case, fn):
    """The restatement's result of a case, computed once and shared (read-only)."""
    key = (kind, case["id"])
    if key not in _WANT:
        res = fn()
        for a in (res if isinstance(res, tuple) else (res,)):
            a.setflags(write=False)
        _WANT[key] = res
    return _WANT[key]


def _knn_want(case):
    return _want("knn", case, lambda: R.knn_vote(case["ref"], case["lab"], case["qry"], case["k"]))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                       # a copy: the cases are read-only


# ============================================================================================ k-NN vote
@pytest.mark.parametrize("form", ("brute", "grid"))
@pytest.mark.parametrize("case", PC.knn_cases(), ids=[c["id"] for c in PC.knn_cases()])
def test_knn_vote_equals_the_restatement(case, form):
    import torch
    from treelearn_amd.util.postprocess import knn_vote
    got = knn_vote(_dev(case["ref"]), _dev(case["lab"]), _dev(case["qry"]), case["k"], force=form)
    want = torch.from_numpy(np.array(_knn_want(case))).cuda()
    assert got.dtype == torch.int64 and torch.equal(got, want), (int((got != want).sum()), len(want))


def test_knn_vote_refuses_k_outside_1_to_nr():
    from treelearn_amd.util.postprocess import knn_vote
    case = PC.knn_cases()[4]                                           # nr = 5
    ref, lab, qry = _dev(case["ref"]), _dev(case["lab"]), _dev(case["qry"])
    assert len(ref) == 5
    for form in ("brute", "grid", None):
        with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
            knn_vote(ref, lab, qry, 6, force=form)
        with pytest.raises(ValueError, match="n_neighbors > 0"):
            knn_vote(ref, lab, qry, 0, force=form)


def test_knn_vote_grid_refuses_dims_beyond_its_limit():
    import ctypes
    import torch
    from treelearn_amd import _hip
    L = _hip.lib()
    ref = torch.zeros((1, 3), device="cuda"); lab = torch.zeros(1, dtype=torch.int64, device="cuda"); out = torch.empty(1, dtype=torch.int64, device="cuda")
    keys = torch.zeros(1, dtype=torch.int64, device="cuda"); starts = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    lo = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    def call(dims):
        return L.tl_knn_vote_grid(_hip.ptr(ref), _hip.ptr(lab), _hip.ptr(keys), 1, _hip.ptr(keys), _hip.ptr(starts), 1, lo, 0.05,
                                  _hip.dims3(np.asarray(dims, dtype=np.int64)), _hip.ptr(ref), 1, 1, _hip.ptr(out), _hip.stream())
    assert call((1 << 20, 1, 1)) == 0 and int(out.item()) == 0
    for dims in (((1 << 20) + 1, 1, 1), (1, (1 << 20) + 1, 1), (1, 1, (1 << 20) + 1), (0, 1, 1)):
        assert call(dims) != 0, dims


# ============================================================================================ group mean
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("case", PC.group_mean_cases(), ids=[c["id"] for c in PC.group_mean_cases()])
def test_group_mean_is_bit_equal_to_the_restatement(case):
    import torch
    from treelearn_amd import _hip
    L = _hip.lib()
    src, keys, perm = _dev(case["src"]), _dev(case["keys"]), _dev(case["perm"])
    n, C = src.shape
    mean = torch.full((n, C), float("nan"), dtype=torch.float64, device="cuda")
    first = torch.full((n,), -7, dtype=torch.int64, device="cuda"); m = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(L.tl_downsample_ws_words(n)), dtype=torch.int32, device="cuda")
    _hip.check(L.tl_group_mean(_hip.ptr(src), n, C, _hip.ptr(keys), _hip.ptr(perm), _hip.ptr(mean), _hip.ptr(first), _hip.ptr(m), _hip.ptr(ws),
                               _hip.stream()), "tl_group_mean")
    want_mean, want_first = _want("gm", case, lambda: R.group_mean(case["src"], case["keys"], case["perm"]))
    G = len(want_first)
    assert int(m.item()) == G
    got = mean[:G].cpu().numpy()
    bad = _bits(got) != _bits(want_mean)
    assert not bad.any(), (int(bad.sum()), got[bad][:4].tolist(), want_mean[bad][:4].tolist())
    assert np.array_equal(first[:G].cpu().numpy(), want_first)
    assert bool(torch.isnan(mean[G:]).all()) and bool((first[G:] == -7).all())                       # nothing written past the groups


# ============================================================================================ ensemble
@pytest.mark.parametrize("case", PC.ensemble_cases(), ids=[c["id"] for c in PC.ensemble_cases()])
def test_ensemble_equals_the_restatement(case):
    import torch
    from treelearn_amd.util.postprocess import ensemble
    args = [case[k] for k in PC.ENSEMBLE_KEYS]
    want = _want("ens", case, lambda: R.ensemble(*args))
    host = ensemble(*args)
    dev = ensemble(*[_dev(a) for a in args], return_device=True)
    assert len(host) == len(dev) == 8
    for i, (w, h, d) in enumerate(zip(want, host, dev)):
        assert isinstance(h, np.ndarray) and torch.is_tensor(d) and d.is_cuda, i
        d = d.cpu().numpy()
        for got in (h, d):
            assert got.dtype == w.dtype and got.shape == w.shape, (i, got.dtype, got.shape)
            if w.dtype == np.int64:
                assert np.array_equal(got, w), (PC.ENSEMBLE_KEYS[i], int((got != w).sum()), got[got != w][:4].tolist(), w[got != w][:4].tolist())
            elif i == 0:
                assert np.array_equal(got, w), "coords"                                              # by value: -0.0 is 0.0
            else:
                assert np.array_equal(got.view(np.int32), w.view(np.int32)), PC.ENSEMBLE_KEYS[i]


# ============================================================================================ eps-grouping
@pytest.mark.parametrize("case", PC.dbscan_cases(), ids=[c["id"] for c in PC.dbscan_cases()])
def test_dbscan_min2_and_group_dbscan_equal_the_restatement(case):
    from treelearn_amd.cluster import dbscan_min2
    from treelearn_amd.util.pipeline import group_dbscan
    xy, eps = case["xy"], case["eps"]
    want = _want("db", case, lambda: R.dbscan_min2(xy, eps))
    got = dbscan_min2(xy, eps)
    assert got.dtype == np.int64 and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(dbscan_min2(_dev(xy), eps), want)
    # group_dbscan: clusters of at least thr points, renumbered from `start` in ascending order of their number; the rest not assigned
    for thr, start in ((1, 1), (3, 10)):
        ids, cnt = np.unique(want[want >= 0], return_counts=True)
        keep = ids[cnt >= thr]
        exp = np.full(len(want), -5, dtype=np.int64)
        ok = np.isin(want, keep)
        exp[ok] = np.searchsorted(keep, want[ok]) + start
        assert np.array_equal(group_dbscan(xy, eps, thr, -5, start), exp), (thr, start)
