"""GPU tests of the shared stream-compaction passes (csrc/tl_scan.h, csrc/tl_scan.hip) through every entry point that uses them, at the
edges of the 2048-item tile and of the one-workgroup pass over the partials: 2048 items are one tile, and 524 289 = 256 * 2048 + 1 items
give 257 partials, the smallest size at which that pass takes a second trip and its carry matters.  Every expectation is an exact
integer or an exact row copy computed with numpy / torch on the same data.

tl_hdbscan_mst_grid scans grid-cell counts, not points: a second trip would need more than 524 288 cells, which no input of a few
seconds reaches, so its tile-edge coverage stays with test_hdbscan_grid_form_equals_prim_form (tests/test_gpu_parity.py)."""
import numpy as np
import pytest
import torch

import crops_restatement as R
from treelearn_amd import _hip, ops
from treelearn_amd.cluster import dbscan_min2
from treelearn_amd.util import crops as C
from treelearn_amd.util.prepare import voxelize

pytestmark = pytest.mark.gpu
SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 4097, 524289)


# ============================================================================================ tl_compact_rows
@pytest.mark.parametrize("n", SIZES)
def test_compact_rows(n):
    x = torch.arange(n, dtype=torch.float32, device="cuda").reshape(n, 1).repeat(1, 3)          # row index in every column (exact in f32)
    masks = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool), "last": torch.zeros(n, dtype=torch.bool),
             "first": torch.zeros(n, dtype=torch.bool), "half": torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5}
    masks["last"][-1] = True; masks["first"][0] = True
    for name, m in masks.items():
        m = m.cuda()
        out, count = ops.compact_rows(x, m)
        k = int(count.item())
        assert k == int(m.sum()), name
        assert torch.equal(out[:k], x[m]), name


# ============================================================================================ tl_bitmap_scan
@pytest.mark.parametrize("n", SIZES)
def test_bitmap_scan(n):
    L = _hip.lib()
    rng = np.random.default_rng(n)
    for name, words in (("random", rng.integers(-2 ** 63, 2 ** 63, n, dtype=np.int64)), ("zeros", np.zeros(n, np.int64)),
                        ("ones", np.full(n, -1, np.int64))):
        pop = np.unpackbits(words.view(np.uint8)).reshape(n, 64).sum(1, dtype=np.uint64)
        want = (np.cumsum(pop) - pop).astype(np.uint32)
        bm = torch.from_numpy(words).cuda()
        pf = torch.empty(n, dtype=torch.int32, device="cuda"); total = torch.empty(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(L.tl_scan_ws_words(n)), dtype=torch.int32, device="cuda")
        _hip.check(L.tl_bitmap_scan(_hip.ptr(bm), n, _hip.ptr(pf), _hip.ptr(total), _hip.ptr(ws), _hip.stream()), "tl_bitmap_scan")
        assert np.array_equal(pf.cpu().numpy().view(np.uint32), want), name
        assert int(total.cpu().numpy().view(np.uint32)[0]) == int(pop.sum()), name


# ============================================================================================ tl_downsample_reduce (int64 count)
@pytest.mark.parametrize("n", SIZES)
def test_downsample_groups(n):
    """voxelize on points whose voxel keys form runs of 1..5 equal keys once sorted: voxel g holds the points with gid == g."""
    rng = np.random.default_rng(n)
    gid = np.repeat(np.arange(n), rng.integers(1, 6, n))[:n]
    gid = gid[rng.permutation(n)]                                       # input order != key order: first_idx is the first ORIGINAL row of a voxel
    data = np.zeros((n, 3)); data[:, 0] = gid                           # voxel size 1: one voxel per integer x
    groups, first = np.unique(gid, return_index=True)
    pts, trace = voxelize(data, 1.0)
    assert len(pts) == len(groups) == len(trace["first_idx"])
    assert np.array_equal(trace["first_idx"].cpu().numpy(), first)
    assert np.array_equal(trace["point2vox"].cpu().numpy(), gid)


# ============================================================================================ tl_cluster_grid
@pytest.mark.parametrize("n", (2049, 524289 + 2))
def test_dbscan_min2_pairs(n):
    """Point i is member i % 3 of group i // 3; groups sit on a 1024-wide lattice of pitch 4.  Members 0 and 1 are 0.5 apart, member 2 is
    2.0 away from both, eps = 1: every complete pair is a cluster, numbered in index order; member 2 and an unpaired last point are noise."""
    i = np.arange(n); g = i // 3; m = i % 3
    xy = np.stack([4.0 * (g % 1024) + np.choose(m, [0.0, 0.5, 0.25]), 4.0 * (g // 1024) + np.choose(m, [0.0, 0.0, np.sqrt(4.0 - 0.0625)])], 1)
    xy = xy.astype(np.float32)
    want = np.where((m == 2) | ((m == 0) & (i + 1 >= n)), -1, g)
    pairs = (n + 1) // 3
    assert np.array_equal(dbscan_min2(xy, 1.0), want)
    L = _hip.lib()
    t = torch.from_numpy(xy).cuda()
    labels = torch.empty(n, dtype=torch.int32, device="cuda"); ncl = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.tl_cluster_ws_bytes(n)), dtype=torch.uint8, device="cuda")
    _hip.check(L.tl_cluster_grid(_hip.ptr(t), n, 1.0, _hip.ptr(labels), _hip.ptr(ncl), _hip.ptr(ws), _hip.stream()), "tl_cluster_grid")
    assert int(ncl.item()) == pairs == int(want.max()) + 1
    assert np.array_equal(labels.cpu().numpy(), want)


# ============================================================================================ tl_crops_count / tl_crops_extract, two crops
@pytest.mark.parametrize("n", (2049, 524289))
def test_extract_two_crops(n):
    """The only caller with more than one group of partials: crop 0 keeps a sparse subset, crop 1 nearly everything."""
    rng = np.random.default_rng(n)
    xyz = np.round(np.stack([rng.uniform(0, 80, n), rng.uniform(0, 80, n), rng.uniform(0, 30, n)], 1), 2).astype(np.float32)
    labels = rng.integers(-1, 40, n).astype(np.float32)
    feats = np.stack([np.arange(n, dtype=np.float32), rng.uniform(0, 1, n).astype(np.float32)], 1)      # column 0 = source row
    centres = np.array([[-40.0, 40.0], [40.0, 40.0]], np.float32)
    rinv = C.inverse_rotations(np.array([1.1, 0.3]))
    chunk = 90
    out = list(C.extract_crops(xyz, labels, feats, centres, rinv, chunk))
    assert len(out) == 2
    for c, (pts, lab, ft) in enumerate(out):
        member, u, v, d = R.crop(xyz, centres[c], rinv[c], chunk)
        band = np.abs(d - chunk / 2) < 1e-9                                 # rows on the edge to within rounding (none expected)
        rows = ft[:, 0].astype(np.int64)
        assert int(member[~band].sum()) <= len(rows) <= int(member[~band].sum()) + int(band.sum()), c
        assert np.all(np.diff(rows) > 0), c                                 # plot row order
        got = np.zeros(n, bool); got[rows] = True
        assert np.array_equal(got[~band], member[~band]), c
        assert np.array_equal(pts[:, 0], u[rows].astype(np.float32)) and np.array_equal(pts[:, 1], v[rows].astype(np.float32)), c
        assert np.array_equal(pts[:, 2], xyz[rows, 2]) and np.array_equal(ft, feats[rows]), c
        assert lab.dtype == np.int32 and np.array_equal(lab, labels[rows].astype(np.int32)), c
    assert 0 < len(out[0][0]) < 0.2 * n and 0.9 * n < len(out[1][0]) < n
