"""Host-side tests of the geometric point features (util/features.py, util/prepare.compute_features, csrc/tl_features.hip): no GPU.
The restatement against the hand-derived cases, the name rules, the cache-file rules, the C entry point's declaration, and the command
line's argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import features_cases as cases
import features_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_gives_the_hand_derived_answers(name):
    c = cases.CASES[name]()
    r = ref.restate(c["points"], c["radius"])
    assert r["margin"] > 1e-10
    c["check"](r["features"])
    cases.compare(r["features"].astype(np.float32), r, min_inside=0.0)             # the comparison accepts the yardstick's own f32 rounding


def test_restatement_replaces_nans_by_the_column_mean():
    c = cases.CASES["plane_with_strays"]()
    raw = ref.restate(c["points"], c["radius"])["features"]
    out = ref.replace_nan(raw)
    assert out.dtype == np.float32 and not np.isnan(out).any()
    v = ref.COL["verticality"]
    assert np.all(out[-3:, v] == np.float32(raw[:-3, v].astype(np.float32).astype(np.float64).mean()))
    assert out[-3:, ref.COL["number_of_neighbors"]].tolist() == [2.0, 2.0, 1.0]
    alone = ref.replace_nan(ref.restate(cases.CASES["pair_and_single"]()["points"], 0.65)["features"])
    assert np.isnan(alone[:, v]).all()                                              # no finite value in the column: nothing to fill with


def test_feature_names_are_the_table_of_the_restatement():
    from treelearn_amd.util.features import FEATURE_NAMES
    assert tuple(FEATURE_NAMES) == tuple(ref.NAMES) and len(FEATURE_NAMES) == 27
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    assert "TL_FEAT_COUNT = 27" in hdr
    for i in (0, 5, 10, 14):                                                       # the header's id table names the same ids
        assert re.search(r"\b%d %s\b" % (i, FEATURE_NAMES[i]), hdr), (i, FEATURE_NAMES[i])


def test_name_validation():
    from treelearn_amd.util.features import check_feature_names, feature_ids
    assert check_feature_names(("verticality",)) == ["verticality"]
    assert feature_ids(["nz", "linearity", "verticality"]) == [13, 5, 10]
    assert check_feature_names(list(ref.NAMES)) == list(ref.NAMES)
    for bad in (["verticalty"], ["linearity", "linearity"], [], "verticality", ["Linearity"]):
        with pytest.raises(ValueError):
            check_feature_names(bad)
    # a list that feeds a model: verticality is there and is last, at most five names
    assert check_feature_names(["linearity", "planarity", "verticality"], for_model=True) == ["linearity", "planarity", "verticality"]
    for bad in (["linearity"], ["verticality", "linearity"], ["PCA1", "PCA2", "linearity", "planarity", "sphericity", "verticality"]):
        with pytest.raises(ValueError):
            check_feature_names(bad, for_model=True)


def test_compute_features_refuses_names_before_any_gpu_work(monkeypatch):
    from treelearn_amd import _hip
    from treelearn_amd.util import prepare
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was touched"))
    for bad in (["verticality", "verticality"], ["curvature"], []):
        with pytest.raises(ValueError):
            prepare.compute_features(np.zeros((4, 3)), 0.6, bad)


def test_configurations_carry_the_default_list():
    from treelearn_amd.util import crops, segment, tiles
    for cfg in (segment.SAMPLE_CFG, tiles.VAL_CFG, crops.TRAIN_CFG):
        assert cfg["feature_names"] == ["verticality"]
    forest = os.path.join(REPO, "README.md")                                       # (only its existence is looked at)
    a = tiles.parse_args(["--forest", forest, "--feature-names", "linearity", "planarity", "verticality"])
    assert a.feature_names == ["linearity", "planarity", "verticality"] and tiles.parse_args(["--forest", forest]).feature_names == ["verticality"]
    for bad in (["verticality", "linearity"], ["linearity"], ["nope", "verticality"]):
        with pytest.raises(SystemExit):
            tiles.parse_args(["--forest", forest, "--feature-names"] + bad)


def test_crops_command_line_takes_feature_names(tmp_path):
    from treelearn_amd.util import crops
    (tmp_path / "forests").mkdir()
    a = crops.parse_args(["--base-dir", str(tmp_path), "--feature-names", "sphericity", "verticality"])
    assert a.feature_names == ["sphericity", "verticality"]
    assert crops.parse_args(["--base-dir", str(tmp_path)]).feature_names == ["verticality"]
    with pytest.raises(SystemExit):
        crops.parse_args(["--base-dir", str(tmp_path), "--feature-names", "verticality", "sphericity"])
    with pytest.raises(ValueError, match="verticality"):
        crops.generate_random_crops(str(tmp_path), dict(feature_names=["linearity"]))
    assert sorted(os.listdir(tmp_path)) == ["forests"]                             # refused before anything is written


def test_segment_forest_checks_names_and_model_before_any_gpu_work():
    from treelearn_amd.util.segment import segment_forest

    class Model:
        use_feats, dim_feat = True, 1

    pts = np.zeros((10, 3))
    with pytest.raises(ValueError, match="dim_feat=1"):
        segment_forest(pts, Model(), sample_cfg=dict(feature_names=["linearity", "planarity", "verticality"]))
    with pytest.raises(ValueError, match="verticality"):
        segment_forest(pts, Model(), sample_cfg=dict(feature_names=["verticality", "linearity"]))
    with pytest.raises(ValueError, match="at most 5"):
        segment_forest(pts, Model(), sample_cfg=dict(feature_names=["PCA1", "PCA2", "linearity", "planarity", "sphericity", "verticality"]))


class _Stop(Exception):
    pass


def test_cache_file_rules(tmp_path, monkeypatch):
    """features/<plot>.npz: `features` only with the default list, `feature_names` beside it with another list; a cache whose names differ
    from the configured ones is refused with both lists named; a cache without names counts as ["verticality"]."""
    from treelearn_amd.util import features as F, prepare, tiles
    n = 50
    pts = np.random.default_rng(0).uniform(0, 5, (n, 3)).astype(np.float32)
    calls = []

    def stub(points, search_radius=0.6, feature_names=("verticality",)):
        calls.append(list(feature_names))
        return torch.arange(n * len(feature_names), dtype=torch.float32).reshape(n, len(feature_names))

    def stop(*a, **k):
        raise _Stop()

    monkeypatch.setattr(prepare, "compute_features", stub)
    monkeypatch.setattr(tiles, "PlotTiler", stop)                                  # the tiler needs the GPU: the cache is settled before it
    three = ["linearity", "planarity", "verticality"]

    def plot(name):
        base = tmp_path / name
        (base / "forests").mkdir(parents=True)
        (base / "forest_voxelized0.1").mkdir()
        np.savez_compressed(base / "forest_voxelized0.1" / "plot.npz", points=pts, labels=np.zeros(n, np.float32))
        forest = base / "forests" / "plot.npy"
        np.save(forest, np.zeros((1, 4)))
        return str(forest), base / "features" / "plot.npz"

    forest, cache = plot("default")
    with pytest.raises(_Stop):
        tiles.write_tiles(forest)
    with np.load(cache) as f:
        assert f.files == ["features"] and f["features"].shape == (n, 1) and f["features"].dtype == np.float32
    with pytest.raises(ValueError) as e:
        tiles.write_tiles(forest, dict(feature_names=three))
    assert "['verticality']" in str(e.value) and str(three) in str(e.value)

    forest, cache = plot("three")
    with pytest.raises(_Stop):
        tiles.write_tiles(forest, dict(feature_names=three))
    with np.load(cache) as f:
        assert sorted(f.files) == ["feature_names", "features"] and [str(s) for s in f["feature_names"]] == three and f["features"].shape == (n, 3)
    with pytest.raises(_Stop):
        tiles.write_tiles(forest, dict(feature_names=three))                       # the cache is reused
    assert calls == [["verticality"], three]
    with pytest.raises(ValueError) as e:
        tiles.write_tiles(forest)
    assert "['verticality']" in str(e.value) and str(three) in str(e.value)
    with pytest.raises(ValueError):
        tiles.write_tiles(forest, dict(feature_names=["planarity", "linearity", "verticality"]))      # the order is part of the list
    assert np.array_equal(F.load_feature_cache(cache, three), np.arange(n * 3, dtype=np.float32).reshape(n, 3))
    # the crop generator reads the same files by the same rule
    from treelearn_amd.util import crops
    with pytest.raises(ValueError):
        crops._load_plot(str(tmp_path / "three" / "forest_voxelized0.1" / "plot.npz"), str(cache))
    assert crops._load_plot(str(tmp_path / "three" / "forest_voxelized0.1" / "plot.npz"), str(cache), three)[2].shape == (n, 3)


def test_entry_point_is_declared_bound_and_refuses_nulls():
    from treelearn_amd import _hip, build as b
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    m = re.search(r"\bint\s+tl_eigen_features\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, "tl_eigen_features is not declared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _hip.PROTOTYPES["tl_eigen_features"]
    assert res is ctypes.c_int32 and len(args) == len(params) == 11
    for p, a in zip(params, args):
        want = ctypes.c_void_p if ("*" in p or p.startswith("tl_stream_t")) else ctypes.c_int64 if p.startswith("int64_t") else \
            ctypes.c_double if p.startswith("double") else ctypes.c_int32
        assert a is want, (p, a)
    assert hasattr(ctypes.CDLL(b.build(verbose=False)), "tl_eigen_features")
    lib = _hip.lib()
    buf = (ctypes.c_int64 * 64)()                                                  # host memory: only looked at where the argument is a host array
    p = ctypes.c_void_p(ctypes.addressof(buf))
    cols = (ctypes.c_int32 * 27)(*range(27))
    c = ctypes.cast(cols, ctypes.c_void_p)
    call = lambda *a: lib.tl_eigen_features(*a, None)                              # noqa: E731
    E = _hip.TL_ERR_ARG
    assert call(None, None, 0, 0.0, None, None, 0, None, 0, None) == E
    for k in (0, 1, 4, 5, 7, 9):                                                   # every pointer in turn
        a = [p, p, 10, 0.6, p, p, 1, c, 3, p]
        a[k] = None
        assert call(*a) == E, k
    assert call(p, p, 0, 0.6, p, p, 1, c, 3, p) == E and call(p, p, 10, 0.6, p, p, 0, c, 3, p) == E       # n, n_pieces
    assert call(p, p, 10, 0.0, p, p, 1, c, 3, p) == E and call(p, p, 10, 0.6, p, p, 11, c, 3, p) == E      # radius, more pieces than points
    assert call(p, p, 10, 0.6, p, p, 1, c, 0, p) == E and call(p, p, 10, 0.6, p, p, 1, c, 28, p) == E      # F
    bad = (ctypes.c_int32 * 3)(0, 27, 1)
    assert call(p, p, 10, 0.6, p, p, 1, ctypes.cast(bad, ctypes.c_void_p), 3, p) == E                       # an id out of range
    bad = (ctypes.c_int32 * 3)(0, -1, 1)
    assert call(p, p, 10, 0.6, p, p, 1, ctypes.cast(bad, ctypes.c_void_p), 3, p) == E


def test_command_line_argument_errors(tmp_path):
    from treelearn_amd.util import features
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 3)))
    out = str(tmp_path / "o.npz")
    ok = ["--forest", str(forest), "--out", out, "--features", "linearity", "planarity", "verticality"]
    a = features.parse_args(ok)
    assert a.features == ["linearity", "planarity", "verticality"] and a.radius == 0.6 and a.voxel_size == 0.1
    assert features.parse_args(ok + ["--voxel-size", "0", "--radius", "0.4"]).voxel_size == 0
    assert features.parse_args(["--forest", str(forest), "--out", out, "--features", "nz"]).features == ["nz"]      # no verticality-last rule here
    for bad in (["--forest", str(forest), "--out", out],                                                            # no features
                ["--forest", str(forest), "--out", out, "--features", "curvature"],
                ["--forest", str(forest), "--out", out, "--features", "nz", "nz"],
                ok + ["--radius", "0"], ok + ["--voxel-size", "-1"],
                ["--forest", str(forest), "--out", str(tmp_path / "o.txt"), "--features", "nz"],
                ["--forest", str(tmp_path / "missing.npy"), "--out", out, "--features", "nz"]):
        with pytest.raises(SystemExit):
            features.main(bad)
    assert not os.path.exists(out)
