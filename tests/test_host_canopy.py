"""Host tests of the canopy height model: the numpy restatement against the cases worked by hand, the parameter and
command-line checks (no GPU is touched), the stand table on hand-built dicts, the writers, and the C declarations."""
import json
import os
import re

import numpy as np
import pytest

import canopy_cases as cases
import canopy_restatement as ref
import terrain_restatement as terrain_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"tl_chm_max": 14, "tl_chm_owner": 15, "tl_chm_pits": 9, "tl_chm_tops": 7, "tl_canopy_keys": 13, "tl_grid_metrics": 14}


def heights_of(case):
    if case["terrain_cfg"] is None:
        return case["h"]
    t = terrain_ref.terrain_model(case["xyz"], case["labels"], **case["terrain_cfg"])
    return terrain_ref.height_above_ground(t, case["xyz"])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_meets_the_hand_cases(name):
    case = cases.CASES[name]()
    h = heights_of(case)
    case["check"](ref.canopy_model(case["xyz"], h, case["labels"], **case["params"]))
    # float32 coordinates of the same cells, a fourth column and another row order change nothing that the case states
    wide = np.column_stack([case["xyz"], np.full(len(h), 7.0)]).astype(np.float32)
    p = np.random.default_rng(1).permutation(len(h))
    lab = None if case["labels"] is None else case["labels"][p]
    case["check"](ref.canopy_model(wide[p], h[p], lab, **case["params"]))


def test_restatement_empty_cloud_and_errors():
    c = ref.canopy_model(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int64))
    assert (c["nx"], c["ny"], c["metric_nx"], c["metric_ny"]) == (0, 0, 0, 0) and c["chm"].shape == (0, 0) and c["layers"].shape == (0, 0, 1)
    assert len(c["tops"]["h"]) == 0 and c["tops_per_tree"].shape == (0,) and c["n_no_ground"] == 0 and c["n_clipped"] == 0
    for xyz, h in (([[np.nan, 0.0, 0.0]], [1.0]), ([[0.0, np.inf, 0.0]], [1.0]), ([[0.0, 0.0, 0.0]], [np.inf]), ([[0.0, 0.0, 0.0]], [-np.inf])):
        with pytest.raises(ValueError):
            ref.canopy_model(np.array(xyz), np.array(h))
    with pytest.raises(ValueError):
        ref.canopy_model(np.zeros((1, 3)), np.zeros(1), cells=2)
    only_nan = ref.canopy_model(np.zeros((2, 3)), np.array([np.nan, np.nan]))
    assert only_nan["n_no_ground"] == 2 and only_nan["n"].tolist() == [[0]] and only_nan["layers"].tolist() == [[[0]]]
    assert np.isnan(only_nan["cover"][0, 0]) and np.isnan(only_nan["h_max"][0, 0])


def test_check_params():
    from treelearn_amd.util.canopy import DEFAULTS, check_params
    assert DEFAULTS == ref.DEFAULTS
    assert tuple(DEFAULTS) == ("cell", "pit_depth", "pit_min_neighbours", "top_window", "top_min_height", "metric_cell", "cutoff", "percentiles",
                               "layer", "max_layers")
    got = check_params()
    assert got == dict(DEFAULTS, percentiles=(25.0, 50.0, 75.0, 95.0, 99.0))
    assert check_params(dict(cell=1), top_window=2.0, layer=None) == dict(got, cell=1.0, top_window=2)
    assert isinstance(check_params(max_layers=3.0)["max_layers"], int)
    edges = dict(pit_depth=0, pit_min_neighbours=1, top_window=1, top_min_height=-3.0, cutoff=-1.0, percentiles=(0, 100), max_layers=1)
    assert check_params(edges)["percentiles"] == (0.0, 100.0)
    assert check_params(pit_min_neighbours=9, max_layers=256, percentiles=list(range(16)))["pit_min_neighbours"] == 9
    assert check_params(percentiles=50)["percentiles"] == (50.0,)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(cell=0), dict(cell=-1.0), dict(cell=inf), dict(cell=nan), dict(metric_cell=0), dict(metric_cell=inf), dict(layer=0),
                dict(layer=-1), dict(layer=nan), dict(pit_depth=-1e-9), dict(pit_depth=inf), dict(pit_depth=nan), dict(pit_min_neighbours=0),
                dict(pit_min_neighbours=10), dict(pit_min_neighbours=2.5), dict(top_window=0), dict(top_window=1.5), dict(top_window=nan),
                dict(top_min_height=inf), dict(top_min_height=nan), dict(cutoff=nan), dict(cutoff=-inf), dict(percentiles=()),
                dict(percentiles=list(range(17))), dict(percentiles=(50, 101)), dict(percentiles=(-1,)), dict(percentiles=(nan,)),
                dict(percentiles="median"), dict(max_layers=0), dict(max_layers=257), dict(max_layers=1.5), dict(window=2), dict(fill_radius=3)):
        with pytest.raises(ValueError):
            check_params(**bad)
    with pytest.raises(ValueError, match="unknown canopy parameter"):
        check_params(dict(cells=0.5))


def test_module_surface():
    from treelearn_amd.util import canopy
    assert set(canopy.__all__) == {"canopy_model", "cloud_canopy", "stand_summary", "write_canopy", "write_stand", "check_params", "Canopy", "DEFAULTS"}
    assert all(hasattr(canopy, k) for k in canopy.__all__) and callable(canopy.add_arguments) and callable(canopy.params_of)
    for k in ("Inputs.", "Parameters", "Grids.", "Step A", "Step B", "Step C", "Step D", "stand_summary", "no CPU fallback"):
        assert k in canopy.__doc__, k
    import argparse
    ap = argparse.ArgumentParser()
    canopy.add_arguments(ap)
    assert canopy.check_params(canopy.params_of(ap.parse_args([]))) == canopy.check_params()
    a = ap.parse_args(["--canopy-percentiles", "10", "90", "--canopy-top-window", "2"])
    assert canopy.params_of(a)["percentiles"] == [10.0, 90.0] and canopy.params_of(a)["top_window"] == 2


@pytest.mark.parametrize("argv", [
    ["--forest", "missing.npy", "--out", "o.npz"],
    ["--forest", __file__, "--out", "o.npz", "--canopy-cell", "0"],
    ["--forest", __file__, "--out", "o.npz", "--canopy-pit-min-neighbours", "10"],
    ["--forest", __file__, "--out", "o.npz", "--canopy-percentiles", "50", "101"],
    ["--forest", __file__, "--out", "o.npz", "--canopy-max-layers", "0"],
    ["--forest", __file__, "--out", "o.npz", "--fill-radius", "-1"],
    ["--forest", __file__, "--out", "o.npz"],                                        # a .py file: an unknown format
    ["--forest", __file__],
    ["--out", "o.npz"],
])
def test_canopy_command_line_errors(argv, capsys):
    from treelearn_amd.util.canopy import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--canopy", "--canopy-cell", "-1"], ["--canopy-top-window", "0"], ["--canopy-layer", "0"]])
def test_segment_command_line_canopy_errors(argv, capsys, tmp_path):
    from treelearn_amd.util.segment import parse_args
    (tmp_path / "w.pth").write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        parse_args(["--forest", __file__, "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)] + argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err


def test_segment_forest_checks_canopy_parameters_first():
    from treelearn_amd.util.segment import segment_forest
    with pytest.raises(ValueError, match="metric_cell"):
        segment_forest(None, None, canopy=True, canopy_cfg=dict(metric_cell=0.0))
    with pytest.raises(ValueError, match="unknown canopy parameter"):
        segment_forest(None, None, canopy=True, canopy_cfg=dict(window=3))


def _host_canopy():
    """A hand-built to_host() dict: 2 x 2 cells of 10 m, three with rows; chm 12, 1, NaN, 20."""
    return dict(cell=np.float64(10.0), cutoff=np.float64(2.0), n=np.array([[3, 1], [0, 2]], np.int32),
                chm=np.array([[12.0, 1.0], [np.nan, 20.0]]), tops_h=np.array([12.0, 20.0]), tops_per_tree=np.array([1, 0, 2, 1], np.int32))


def test_stand_summary_without_and_with_an_inventory():
    from treelearn_amd.util.canopy import stand_summary
    s = stand_summary(_host_canopy())
    assert set(s) == {"area_ha", "canopy_cover", "chm_mean", "chm_max", "n_tops"}
    assert s["area_ha"] == 3 * 100.0 / 1e4 and s["canopy_cover"] == 2.0 / 3.0 and s["chm_mean"] == 11.0 and s["chm_max"] == 20.0 and s["n_tops"] == 2
    nan = np.nan
    inv = dict(n_points=np.array([50, 0, 70, 9]), dbh=np.array([0.2, nan, 0.4, nan]), height=np.array([10.0, nan, 20.0, 5.0]))
    s = stand_summary(_host_canopy(), inv)
    assert s["n_trees"] == 3 and s["stems_per_ha"] == 3 / 0.03 and s["n_dbh"] == 2
    g = np.pi / 4.0 * np.array([0.04, 0.16])
    assert abs(s["basal_area_m2_per_ha"] - g.sum() / 0.03) <= 1e-12 and abs(s["qmd"] - np.sqrt(0.1)) <= 1e-12
    assert abs(s["lorey_height"] - (0.04 * 10.0 + 0.16 * 20.0) / 0.2) <= 1e-12                         # the NaN DBHs are skipped
    assert (s["trees_with_one_top"], s["trees_without_top"], s["trees_with_several_tops"]) == (2, 1, 1)
    # dbh_ag and height_ag are preferred where the inventory has them
    ag = dict(inv, dbh_ag=np.array([0.3, nan, nan, nan]), height_ag=np.array([11.0, nan, 21.0, 6.0]))
    s = stand_summary(_host_canopy(), ag)
    assert s["n_dbh"] == 1 and abs(s["qmd"] - 0.3) <= 1e-15 and abs(s["lorey_height"] - 11.0) <= 1e-12
    no_tops = {k: v for k, v in _host_canopy().items() if k != "tops_per_tree"}
    assert "trees_with_one_top" not in stand_summary(no_tops, inv)


def test_stand_summary_of_an_empty_plot_is_all_nan():
    from treelearn_amd.util.canopy import stand_summary
    empty = dict(cell=np.float64(0.5), cutoff=np.float64(2.0), n=np.zeros((0, 0), np.int32), chm=np.zeros((0, 0)), tops_h=np.zeros(0),
                 tops_per_tree=np.zeros(0, np.int32))
    inv = dict(n_points=np.zeros(0, np.int64), dbh=np.zeros(0), height=np.zeros(0))
    s = stand_summary(empty, inv)
    assert s["area_ha"] == 0.0 and s["n_tops"] == 0 and s["n_trees"] == 0 and s["n_dbh"] == 0
    for k in ("canopy_cover", "chm_mean", "chm_max", "stems_per_ha", "basal_area_m2_per_ha", "qmd", "lorey_height"):
        assert np.isnan(s[k]), k


def test_writers_round_trip(tmp_path):
    from treelearn_amd.util.canopy import stand_summary, write_canopy, write_stand
    d = _host_canopy()
    write_canopy(str(tmp_path / "c.npz"), d)
    with np.load(tmp_path / "c.npz") as f:
        assert set(f.files) == set(d) and all(np.array_equal(f[k], d[k], equal_nan=True) and f[k].dtype == d[k].dtype for k in d)
    s = stand_summary(d, dict(n_points=np.array([5]), dbh=np.array([np.nan]), height=np.array([3.0])))
    write_stand(str(tmp_path / "s.json"), s)
    back = json.load(open(tmp_path / "s.json"))
    assert list(back) == list(s) and back["qmd"] is None and back["lorey_height"] is None
    assert all(back[k] == s[k] for k in s if back[k] is not None)


def test_c_declarations_and_prototypes():
    from treelearn_amd import _hip
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    for name, n_args in KERNELS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/treelearn_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _hip.PROTOTYPES and len(_hip.PROTOTYPES[name][1]) == n_args, name
        assert m.group(1).strip().endswith("tl_stream_t stream")
    assert "csrc/tl_canopy.hip, DESIGN §22" in hdr
    src = open(os.path.join(REPO, "treelearn_amd", "csrc", "tl_canopy.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "__fma" not in src and "_rn(" not in src
