"""Host tests of the per-tree inventory: the numpy restatement against cases worked by hand (tests/inventory_cases.py),
the CSV writer, and the argument checks that come before any GPU work.  The kernel is held to the restatement in tests/test_gpu_inventory.py."""
import csv
import os

import numpy as np
import pytest

import inventory_cases as cases
import inventory_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_hand_cases(name):
    xyz, lab, check = cases.CASES[name]()
    inv = ref.tree_inventory(xyz, lab)
    assert tuple(inv) == ref.COLUMNS
    check(inv)
    # float32 input with a row stride of 4 is the same cloud once widened
    x4 = np.zeros((len(xyz), 4), np.float32)
    x4[:, :3] = xyz
    a, b = ref.tree_inventory(x4[:, :3], lab), ref.tree_inventory(x4[:, :3].astype(np.float64), lab)
    for k in ref.COLUMNS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_restatement_offset_and_parameters():
    xyz, lab, off, check = cases.offset_case()
    plain = ref.tree_inventory(xyz, lab)
    check(ref.tree_inventory(xyz, lab, offset=off), plain)
    # a thicker slice at another height takes other rows; a higher minimum turns the fit off; a coarser cell counts fewer cells
    assert ref.tree_inventory(xyz, lab, slice_height=1.25, slice_thickness=0.05)["dbh_n"].tolist() == [32]
    assert np.isnan(ref.tree_inventory(xyz, lab, dbh_min_points=65)["dbh"][0])
    assert ref.tree_inventory(xyz, lab, dbh_max_radius=0.1)["dbh_n"].tolist() == [0]
    assert ref.tree_inventory(xyz, lab, crown_cell=10.0)["crown_cells"].tolist() == [1]          # x in (0, 10), y in (-10, 0): one cell


def test_solve3_pivots_and_singular():
    # needs a row swap in the first column; solution (1, 2, 3)
    A = [[0.0, 2.0, 1.0], [4.0, 1.0, 0.0], [1.0, 1.0, 1.0]]
    x = np.array([1.0, 2.0, 3.0])
    sol = ref.solve3(A, list(np.asarray(A) @ x))
    assert np.allclose(sol, x, rtol=0, atol=1e-14)
    assert ref.solve3([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 1.0]], [1.0, 2.0, 3.0]) is None
    assert ref.solve3([[1.0, 0.0, 0.0], [0.0, 1e-13, 0.0], [0.0, 0.0, 1.0]], [1.0, 1.0, 1.0]) is None


def test_write_inventory_round_trips(tmp_path):
    from treelearn_amd.util.inventory import COLUMNS, INT_COLUMNS, write_inventory
    from treelearn_amd.util.segment import CATEGORIES
    assert COLUMNS == ref.COLUMNS and INT_COLUMNS == ref.INT_COLUMNS
    xyz, lab, _ = cases.case_degenerate()
    inv = ref.tree_inventory(xyz, lab, offset=[0.1, 1e6 / 3, -7e-5])
    for with_cat in (False, True):
        path = write_inventory(str(tmp_path / f"t{int(with_cat)}.csv"), inv, categories=[2, 0, 1] if with_cat else None)
        rows = list(csv.reader(open(path, newline="")))
        assert rows[0] == list(COLUMNS) + (["category"] if with_cat else [])
        assert len(rows) == 1 + 3
        for i, row in enumerate(rows[1:]):
            for k, cell in zip(COLUMNS, row):
                if k in INT_COLUMNS:
                    assert int(cell) == inv[k][i] and cell == str(int(inv[k][i]))
                elif np.isnan(inv[k][i]):
                    assert cell == "nan"
                else:
                    assert float(cell) == inv[k][i]                 # repr: the same bits come back
            if with_cat:
                assert row[-1] == CATEGORIES[[2, 0, 1][i]]
    with pytest.raises(ValueError):
        write_inventory(str(tmp_path / "bad.csv"), inv, categories=[0, 1])
    # no trees: the header alone
    e = ref.tree_inventory(np.zeros((2, 3)), np.zeros(2, np.int64))
    assert list(csv.reader(open(write_inventory(str(tmp_path / "e.csv"), e), newline=""))) == [list(COLUMNS)]


def test_argument_validation_before_any_gpu_work():
    from treelearn_amd.util.inventory import DEFAULTS, check_params, cloud_inventory, tree_inventory
    from treelearn_amd.util.segment import segment_forest
    assert DEFAULTS == dict(slice_height=1.3, slice_thickness=0.2, dbh_max_radius=1.0, dbh_min_points=8, crown_cell=0.25)
    assert check_params() == DEFAULTS and check_params(dict(crown_cell=0.5), slice_height=None)["crown_cell"] == 0.5
    xyz, lab = np.zeros((4, 3)), np.ones(4, np.int64)
    for bad in (dict(slice_thickness=0.0), dict(slice_thickness=-0.2), dict(crown_cell=0.0), dict(crown_cell=float("nan")),
                dict(dbh_max_radius=0.0), dict(dbh_max_radius=-1.0), dict(dbh_min_points=-1), dict(dbh_min_points=2.5),
                dict(slice_height=float("inf"))):
        with pytest.raises(ValueError):
            tree_inventory(xyz, lab, **bad)
        with pytest.raises(ValueError):
            check_params(bad)
        with pytest.raises(ValueError):
            cloud_inventory(np.zeros((4, 4)), **bad)
        with pytest.raises(ValueError):                              # before the model or the points are looked at
            segment_forest(None, None, inventory=True, inventory_cfg=bad)
    with pytest.raises(ValueError):
        check_params(dict(slice_hight=1.3))
    with pytest.raises(ValueError):
        tree_inventory(xyz, lab, offset=[1.0, 2.0])
    with pytest.raises(ValueError):
        cloud_inventory(np.zeros((4, 3)))


def test_command_lines_refuse_bad_parameters(tmp_path):
    from treelearn_amd.util import inventory, segment
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 4)))
    with pytest.raises(SystemExit):
        inventory.main(["--forest", str(forest), "--out", str(tmp_path / "o.csv"), "--crown-cell", "0"])
    with pytest.raises(SystemExit):
        inventory.main(["--forest", str(tmp_path / "missing.npy"), "--out", str(tmp_path / "o.csv")])
    (tmp_path / "w.pth").write_bytes(b"")
    with pytest.raises(SystemExit):
        segment.parse_args(["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path), "--inventory",
                            "--slice-thickness", "-1"])
    a = segment.parse_args(["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path), "--inventory", "--crown-cell", "0.5"])
    assert a.inventory and inventory.params_of(a) == dict(inventory.DEFAULTS, crown_cell=0.5)
    assert not segment.parse_args(["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]).inventory
