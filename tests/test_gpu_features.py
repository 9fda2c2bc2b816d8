"""GPU tests of the geometric point features (csrc/tl_features.hip, util/prepare.compute_features, util/features.py): the hand-derived
cases of tests/features_cases.py, all 27 columns against the float64 restatement of tests/features_restatement.py on a synthetic tile,
column subsets, run-to-run bits, the plumbing through segment_forest, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import features_cases as cases
import features_restatement as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(ref.NAMES)
_refs = {}


def _raw(points, radius, names=ALL):
    """The kernel's columns in input order with the NaNs of the definition left in."""
    from treelearn_amd.util import prepare
    from treelearn_amd.util.features import feature_ids
    return prepare._eigen_features(points, radius, feature_ids(names), replace_nan=False).cpu().numpy()


def _tile_cloud():
    from treelearn_amd.synth import make_tile
    pts = make_tile(extent=8.0, voxel=0.1, n_trees=3, fill=0.10, seed=8)["points"].astype(np.float64)
    assert len(pts) == 34005
    return np.vstack([pts, np.array([[40.0, 40.0, 3.0], [40.2, 40.0, 3.0], [-50.0, 7.0, 1.0]])])       # isolated points: < 3 neighbours


def _tile_ref(radius):
    """The restatement of the tile cloud: computed once per radius and left unchanged."""
    if radius not in _refs:
        r = ref.restate(_tile_cloud(), radius)
        r["features"].setflags(write=False)
        _refs[radius] = r
    return _refs[radius]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_hand_derived_cases(name):
    from treelearn_amd.util.prepare import compute_features
    c = cases.CASES[name]()
    raw = _raw(c["points"], c["radius"])
    assert raw.dtype == np.float32 and raw.shape == (len(c["points"]), 27)
    c["check"](raw)
    r = ref.restate(c["points"], c["radius"])
    assert r["margin"] > 1e-10
    cases.compare(raw, r, min_inside=0.0)
    # through the public function: the same values, NaNs replaced by the column mean (f64 sum of the finite values / count, as f32)
    out = compute_features(c["points"], c["radius"], ALL).cpu().numpy()
    assert out.dtype == np.float32 and out.shape == raw.shape
    nan = np.isnan(raw)
    assert np.array_equal(out[~nan], raw[~nan])
    for col in np.flatnonzero(nan.any(0)):
        fin = raw[~nan[:, col], col]
        if len(fin) == 0:
            assert np.isnan(out[:, col]).all()
        else:
            want = np.float32(fin.astype(np.float64).sum() / len(fin))
            assert np.abs(out[nan[:, col], col].astype(np.float64) - want).max() <= 2.0 ** -22 * max(1.0, abs(float(want))), ref.NAMES[col]


@pytest.mark.parametrize("radius", [0.6, 0.65])
def test_all_columns_against_the_restatement(radius):
    r = _tile_ref(radius)
    ok = ~np.isnan(r["g3"])
    # conditions on the input, on the restatement first: no pair within 1e-10 of the radius, no point with close eigenvalues
    assert r["margin"] > 1e-10, r["margin"]
    assert (~ok).sum() == 3
    for k in ("g3", "gap23", "gap12"):
        assert r[k][ok].min() > 1e-5, (k, float(r[k][ok].min()))
    raw = _raw(_tile_cloud(), radius)
    cases.compare(raw, r, min_inside=1.0, report=lambda fig: print(f"radius {radius}: worst figures {fig}"))


def test_verticality_column_against_the_one_column_path():
    from treelearn_amd.util.prepare import compute_features
    pts = _tile_cloud()
    old = compute_features(pts, 0.6, ["verticality"]).cpu().numpy()[:, 0]
    new = compute_features(pts, 0.6, ["nz", "verticality"]).cpu().numpy()[:, 1]
    d = float(np.abs(old.astype(np.float64) - new.astype(np.float64)).max())
    print(f"verticality, new path against tl_verticality: {d:.3e}")
    assert d <= 2e-5


def test_column_subsets_orders_and_repeat_runs_give_the_same_bits():
    pts = _tile_cloud()
    full = _raw(pts, 0.6)
    sub = ["nz", "linearity", "verticality"]
    got = _raw(pts, 0.6, sub)
    assert got.shape == (len(pts), 3)
    assert np.array_equal(got.view(np.uint32), full[:, [ref.COL[n] for n in sub]].view(np.uint32))
    assert np.array_equal(_raw(pts, 0.6).view(np.uint32), full.view(np.uint32))
    # the bits do not depend on the order of the work table either
    from treelearn_amd.util import prepare
    from treelearn_amd.util.features import feature_ids
    xyz = prepare._dev_f64(pts)
    sx, skeys, perm, ext = prepare.sorted_cells(xyz, 0.6)
    pieces = prepare.feature_pieces(skeys)
    a = prepare.eigen_features_sorted(sx, skeys, ext, pieces, 0.6, feature_ids(ALL))
    b = prepare.eigen_features_sorted(sx, skeys, ext, pieces.flip(0).contiguous(), 0.6, feature_ids(ALL))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # ... nor on how the points fall into pieces: with every cell's first point as one more piece start, the waves that begin there
    # see other z-ranges and write the same rows once more
    head = torch.ones(len(skeys), dtype=torch.bool, device=skeys.device)
    head[1:] = skeys[1:] != skeys[:-1]
    finer = torch.unique(torch.cat([pieces, torch.nonzero(head).squeeze(1)]))
    assert len(finer) > len(pieces)
    c = prepare.eigen_features_sorted(sx, skeys, ext, finer.contiguous(), 0.6, feature_ids(ALL))
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_piece_table():
    from treelearn_amd.util.prepare import feature_pieces
    z = lambda col, cell, count: [(col << 21) | cell] * count                           # noqa: E731
    keys = torch.tensor(z(5, 0, 40) + z(5, 1, 50) + z(5, 7, 40) + z(6, 0, 1) + z(9, 3, 64) + z(9, 4, 5), dtype=torch.int64, device="cuda")
    assert feature_pieces(keys).tolist() == [0, 64, 128, 130, 131, 192]              # a column's first point, and every multiple of 64
    assert feature_pieces(keys[:1]).tolist() == [0]


def _small_plot():
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=24, voxel=0.1, n_trees=20, fill=0.10, seed=5)
    return t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])


def test_segment_forest_carries_three_feature_columns():
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.util.prepare import compute_features, voxelize
    from treelearn_amd.util.segment import segment_forest
    names = ["linearity", "planarity", "verticality"]
    pts = _small_plot()
    torch.manual_seed(3)
    kw = dict(channels=16, num_blocks=3, use_feats=True, spatial_shape=[500, 500, 1000], voxel_size=0.1)
    wrong = TreeLearn(dim_feat=1, **kw).cuda().eval()
    with pytest.raises(ValueError, match="dim_feat=1"):
        segment_forest(pts, wrong, sample_cfg=dict(feature_names=names))
    model = TreeLearn(dim_feat=3, **kw)
    # random backbone; heads pinned so that every point is a tree point with a zero offset: grouping then looks at every point
    sd = model.state_dict()
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    model.load_state_dict(sd)
    model = model.cuda().eval()
    # grouping reads the LAST feature column (tau_vert); no cluster can reach tau_min, so every point comes back as non-tree and the
    # stages after grouping, which this test is not about, have no tree to work on
    cfg = dict(use_hdbscan=False, tau_vert=0.6, tau_off=1e9, tau_group=0.15, tau_min=10 ** 9)
    with torch.no_grad():
        res = segment_forest(pts, model, sample_cfg=dict(feature_names=names, stride=1.0), grouping_cfg=cfg, return_type="original", return_pointwise=True)
    assert len(res["coords"]) == len(pts) and not res["labels"].any() and len(res["categories"]) == 0
    pw = res["pointwise"]
    assert pw["input_feats"].shape == (len(pw["coords"]), 3) and pw["input_feats"].dtype == np.float32
    # its rows are compute_features of the voxelised cloud at the ensembled coordinates
    centred = torch.from_numpy(pts).cuda() - torch.from_numpy(pts).cuda().mean(0)
    vox = voxelize(centred, 0.1)[0][:, :3].float().contiguous()
    feats = compute_features(vox, 0.6, names).cpu().numpy()

    def key(a):                                                                        # one i64 per row of 2-decimal coordinates
        q = np.round(np.asarray(a, np.float64) * 100).astype(np.int64) + (1 << 19)
        assert q.min() >= 0 and q.max() < (1 << 20)
        return (q[:, 0] << 40) | (q[:, 1] << 20) | q[:, 2]

    kv, kp = key(vox.cpu().numpy()), key(pw["coords"])
    order = np.argsort(kv)
    assert len(np.unique(kv)) == len(kv)
    idx = order[np.minimum(np.searchsorted(kv[order], kp), len(kv) - 1)]
    assert np.array_equal(kv[idx], kp)
    assert np.array_equal(pw["input_feats"], feats[idx])


def test_command_line(tmp_path):
    from treelearn_amd.util.prepare import compute_features
    c = cases.CASES["blob_3000"]()
    forest = tmp_path / "cloud.npy"
    np.save(forest, c["points"])
    out = tmp_path / "features.npz"
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "treelearn_amd.util.features", "--forest", str(forest), "--out", str(out),
                        "--features", "linearity", "planarity", "verticality", "--voxel-size", "0"],
                       capture_output=True, text=True, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO))
    assert p.returncode == 0, p.stderr[-2000:]
    with np.load(out) as f:
        assert sorted(f.files) == ["feature_names", "features", "points"]
        assert [str(s) for s in f["feature_names"]] == ["linearity", "planarity", "verticality"]
        assert np.array_equal(f["points"], c["points"]) and f["features"].dtype == np.float32
        want = compute_features(c["points"], 0.6, ["linearity", "planarity", "verticality"]).cpu().numpy()
        assert np.array_equal(f["features"], want)
