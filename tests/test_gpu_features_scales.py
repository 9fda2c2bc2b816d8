"""GPU tests of the multi-scale geometric features (csrc/tl_features.hip: tl_eigen_features_scales,
util/prepare.eigen_features_scales_sorted / compute_features_scales, util/features.py --radii).

The first yardstick is exact: every scale of one multi-scale launch is, bit for bit and NaN for NaN, what tl_eigen_features writes on the
SAME sorted arrays (cells of the largest radius) with radius = r_k -- that kernel only reads r^2, so a radius below the cell edge is valid
for it.  The second is the float64 restatement of tests/features_restatement.py, per scale, with the tolerances of features_cases.compare."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import features_cases as one
import features_restatement as ref
import features_scales_cases as cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(ref.NAMES)
TILE_RADII = (0.3, 0.45, 0.6)          # admissible on the tile (asserted below); 0.2 is not: its radius margin there is 1.4e-14
_refs = {}


def _sorted(points, radii):
    """The arrays of one launch: points sorted by the cells of the largest radius, keys, permutation, extent, piece table."""
    from treelearn_amd.util import prepare
    sx, skeys, perm, ext = prepare.sorted_cells(prepare._dev_f64(points), float(max(radii)))
    return sx, skeys, perm, ext, prepare.feature_pieces(skeys)


def _assert_every_scale_is_the_one_radius_kernel(points, radii, names=ALL):
    """The exact yardstick; returns the multi-scale output in sorted order and the permutation."""
    from treelearn_amd.util import prepare
    from treelearn_amd.util.features import feature_ids
    ids = feature_ids(names)
    sx, skeys, perm, ext, pieces = _sorted(points, radii)
    got = prepare.eigen_features_scales_sorted(sx, skeys, ext, pieces, radii, ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(points), len(radii), len(ids)) and got.is_contiguous()
    for k, r in enumerate(radii):
        want = prepare.eigen_features_sorted(sx, skeys, ext, pieces, r, ids)
        a, b = got[:, k, :].contiguous().view(torch.int32), want.view(torch.int32)
        assert torch.equal(torch.isnan(got[:, k, :]), torch.isnan(want)), (k, r)
        assert torch.equal(a, b), (k, r, int((a != b).any(1).sum()))
    # the reversed piece table: the same bits
    again = prepare.eigen_features_scales_sorted(sx, skeys, ext, pieces.flip(0).contiguous(), radii, ids)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    return got, perm


def _input_order(got, perm):
    out = torch.empty_like(got)
    out[perm] = got
    return out.cpu().numpy()


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
def test_hand_made_cases(name):
    c = cases.CASES[name]()
    got, perm = _assert_every_scale_is_the_one_radius_kernel(c["points"], c["radii"])
    raw = _input_order(got, perm)
    c["check"](raw)
    cases.compare_scales(raw, cases.restate_scales(c["points"], c["radii"]), on_the_radius=c.get("on_the_radius", False))
    # the public function with the NaNs left in is the same array
    from treelearn_amd.util.prepare import compute_features_scales
    pub = compute_features_scales(c["points"], c["radii"], ALL, replace_nan=False).cpu().numpy()
    assert pub.dtype == np.float32 and np.array_equal(pub.view(np.uint32), raw.view(np.uint32))


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_tile_every_scale_is_the_one_radius_kernel(S):
    radii = (TILE_RADII + (0.65,))[:S]
    _assert_every_scale_is_the_one_radius_kernel(_tile_cloud(), radii)


def test_tile_against_the_restatement():
    refs = [_tile_ref(r) for r in TILE_RADII]
    for r, res in zip(TILE_RADII, refs):                                            # the conditions on the input, on the restatement first
        ok = ~np.isnan(res["g3"])
        print(f"radius {r}: margin {res['margin']:.3e}, min gap23 {res['gap23'][ok].min():.3e}, min gap12 {res['gap12'][ok].min():.3e}")
        assert res["margin"] > 1e-10 and not ok[-3:].any() and ok.mean() > 0.99        # (at 0.3 m a few hundred sparse rows have < 3 neighbours too)
        assert res["gap23"][ok].min() > 1e-5 and res["gap12"][ok].min() > 1e-5
    from treelearn_amd.util.prepare import compute_features_scales
    raw = compute_features_scales(_tile_cloud(), TILE_RADII, ALL, replace_nan=False).cpu().numpy()
    for k, (r, res) in enumerate(zip(TILE_RADII, refs)):
        one.compare(raw[:, k, :], res, min_inside=1.0, report=lambda fig: print(f"radius {r}: worst figures {fig}"))


def test_repeat_runs_column_subsets_and_orders_give_the_same_bits():
    from treelearn_amd.util.prepare import compute_features_scales
    pts = _tile_cloud()
    full = compute_features_scales(pts, TILE_RADII, ALL, replace_nan=False).cpu().numpy()
    assert np.array_equal(compute_features_scales(pts, TILE_RADII, ALL, replace_nan=False).cpu().numpy().view(np.uint32), full.view(np.uint32))
    for sub in (["nz", "linearity", "verticality"], ["number_of_neighbors"], ["linearity", "planarity", "verticality", "number_of_neighbors"], ALL[::-1]):
        got = compute_features_scales(pts, TILE_RADII, sub, replace_nan=False).cpu().numpy()
        assert got.shape == (len(pts), 3, len(sub))
        assert np.array_equal(got.view(np.uint32), full[:, :, [ref.COL[n] for n in sub]].view(np.uint32)), sub
    # a subset of the scales is a subset of the rows, as long as the largest radius (the cell edge, so the order of the sums) stays
    got = compute_features_scales(pts, (0.45, 0.6), ALL, replace_nan=False).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), full[:, 1:, :].view(np.uint32))


def test_nan_replacement_is_per_scale_and_column():
    from treelearn_amd.util.prepare import compute_features_scales
    c = cases.CASES["between_radii"]()
    pts = np.vstack([c["points"], one.plane(0)["points"]])                          # finite rows to take the means from
    radii = (0.25, 0.45)                                                            # (0.289 .. 0.344 from row 0 to its neighbours)
    raw = compute_features_scales(pts, radii, ALL, replace_nan=False).cpu().numpy()
    out = compute_features_scales(pts, radii, ALL).cpu().numpy()
    assert out.dtype == np.float32 and out.shape == raw.shape == (len(pts), 2, 27)
    nan = np.isnan(raw)
    assert nan[0, 0].sum() == 26 and not nan[0, 1].any()                          # the row between the radii: NaN at scale 1 only
    assert np.array_equal(out[~nan], raw[~nan]) and not np.isnan(out).any()
    for k in range(2):
        for col in np.flatnonzero(nan[:, k, :].any(0)):
            fin = raw[~nan[:, k, col], k, col]
            want = np.float32(fin.astype(np.float64).sum() / len(fin))
            assert np.abs(out[nan[:, k, col], k, col].astype(np.float64) - want).max() <= 2.0 ** -22 * max(1.0, abs(float(want))), (k, ref.NAMES[col])
    # a (scale, column) without a finite value stays NaN
    alone = compute_features_scales(one.pair_and_single()["points"], (0.3, 0.65), ["linearity", "number_of_neighbors"]).cpu().numpy()
    assert np.isnan(alone[:, :, 0]).all() and alone[:, :, 1].tolist() == [[2.0, 2.0], [2.0, 2.0], [1.0, 1.0]]


def test_command_line(tmp_path):
    from treelearn_amd.util.prepare import compute_features_scales
    c = one.CASES["blob_3000"]()
    forest = tmp_path / "cloud.npy"
    np.save(forest, c["points"])
    out = tmp_path / "features.npz"
    names = ["linearity", "planarity", "verticality"]
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "treelearn_amd.util.features", "--forest", str(forest), "--out", str(out),
                        "--features"] + names + ["--voxel-size", "0", "--radii", "0.2", "0.4", "0.6"],
                       capture_output=True, text=True, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO))
    assert p.returncode == 0, p.stderr[-2000:]
    with np.load(out) as f:
        assert sorted(f.files) == ["feature_names", "features", "points", "radii"]
        assert [str(s) for s in f["feature_names"]] == names and f["radii"].tolist() == [0.2, 0.4, 0.6] and f["radii"].dtype == np.float64
        assert np.array_equal(f["points"], c["points"]) and f["features"].dtype == np.float32 and f["features"].shape == (3000, 3, 3)
        assert np.array_equal(f["features"], compute_features_scales(c["points"], (0.2, 0.4, 0.6), names).cpu().numpy())
