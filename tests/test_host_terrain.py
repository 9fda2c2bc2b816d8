"""Host tests of the terrain model: the numpy restatement against the cases worked by hand, the parameter and command-line
checks (no GPU is touched), and write_inventory with and without the ground columns."""
import csv
import io

import numpy as np
import pytest

import inventory_restatement as inv_ref
import terrain_cases as cases
import terrain_restatement as ref


def _view(t):
    return t, lambda xy: ref.ground_at(t, xy[:, 0], xy[:, 1])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_meets_the_hand_cases(name):
    xyz, lab, params, check = cases.CASES[name]()
    check(*_view(ref.terrain_model(xyz, lab, **params)))
    # float32 input widened exactly and a fourth column change nothing that the case states
    wide = np.column_stack([xyz, np.full(len(xyz), 7.0)])
    t = ref.terrain_model(wide, lab, **params)
    check(*_view(t))


def test_restatement_empty_cloud_and_height_above_ground():
    t = ref.terrain_model(np.zeros((0, 3)))
    assert (t["nx"], t["ny"]) == (0, 0) and t["z"].shape == (0, 0)
    assert np.isnan(ref.ground_at(t, [1.0], [2.0])).all()
    xyz, lab, params, _ = cases.CASES["plane"]()
    t = ref.terrain_model(xyz, lab, **params)
    up = xyz + np.array([0.0, 0.0, 2.5])
    assert np.abs(ref.height_above_ground(t, up) - 2.5).max() <= 1e-12
    assert np.isnan(ref.ground_at(t, [np.nan, 1.0], [1.0, np.inf])).all()
    with pytest.raises(ValueError):
        ref.terrain_model(np.array([[0.0, 0.0, np.nan]]))


def test_restatement_tree_columns_on_flat_ground():
    xyz, lab, check = cases.tree_on_flat_ground()
    t = ref.terrain_model(xyz, lab)
    got = ref.tree_inventory(xyz, lab, t)
    assert tuple(got) == inv_ref.COLUMNS + ref.GROUND_COLUMNS
    check(got)
    plain = inv_ref.tree_inventory(xyz, lab)
    for k in inv_ref.COLUMNS:
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    off = np.array([100.0, 200.0, 30.0])
    moved = ref.tree_inventory(xyz, lab, t, offset=off)
    assert moved["z_ground"][0] == 30.0 and moved["height_ag"][0] == got["height_ag"][0] and moved["base_gap"][0] == got["base_gap"][0]
    assert moved["dbh_ag_x"][0] == got["dbh_ag_x"][0] + 100.0 and moved["dbh_ag_y"][0] == got["dbh_ag_y"][0] + 200.0
    assert moved["x"][0] == got["x"][0] + 100.0
    # no terrain under the tree: NaN columns, dbh_ag_n = 0
    none = ref.tree_inventory(xyz, lab, ref.terrain_model(xyz, np.where(lab == 0, -1, lab)))
    assert none["dbh_ag_n"].tolist() == [0] and all(np.isnan(none[k][0]) for k in ref.GROUND_COLUMNS if k != "dbh_ag_n")


def test_check_params():
    from treelearn_amd.util.terrain import DEFAULTS, check_params
    assert DEFAULTS == dict(cell=0.5, max_slope=1.0, step_tol=0.2, window=2, fill_radius=20)
    assert check_params() == DEFAULTS and check_params(dict(cell=1), window=0.0, fill_radius=None) == dict(DEFAULTS, cell=1.0, window=0)
    assert isinstance(check_params(window=3.0)["window"], int)
    for bad in (dict(cell=0), dict(cell=-1.0), dict(cell=float("inf")), dict(cell=float("nan")), dict(max_slope=-0.1),
                dict(max_slope=float("nan")), dict(step_tol=-1e-9), dict(window=-1), dict(window=1.5), dict(fill_radius=-2),
                dict(fill_radius=0.5), dict(fill_radius=float("nan")), dict(radius=3), dict(crown_cell=0.25)):
        with pytest.raises(ValueError):
            check_params(**bad)
    with pytest.raises(ValueError, match="unknown terrain parameter"):
        check_params(dict(cells=0.5))


def test_columns_and_module_surface():
    from treelearn_amd.util import inventory, terrain
    assert terrain.GROUND_COLUMNS == ref.GROUND_COLUMNS == inventory.GROUND_COLUMNS
    assert inventory.COLUMNS == inv_ref.COLUMNS
    for k in ("Inputs.", "Grid.", "Step A", "Step B", "Step C", "Sampling", "Per-tree columns"):
        assert k in terrain.__doc__, k


@pytest.mark.parametrize("argv", [
    ["--forest", "missing.npy", "--out", "o.npz"],
    ["--forest", __file__, "--out", "o.npz", "--cell", "0"],
    ["--forest", __file__, "--out", "o.npz", "--max-slope", "-1"],
    ["--forest", __file__, "--out", "o.npz", "--window", "-1"],
    ["--forest", __file__, "--out", "o.npz", "--fill-radius", "1.5"],
    ["--forest", __file__],
    ["--out", "o.npz"],
])
def test_terrain_command_line_errors(argv, capsys):
    from treelearn_amd.util.terrain import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [
    ["--forest", __file__, "--out", "o.csv", "--terrain", "--cell", "-2"],
    ["--forest", __file__, "--out", "o.csv", "--step-tol", "-1"],
    ["--forest", "missing.npy", "--out", "o.csv", "--terrain"],
])
def test_inventory_command_line_terrain_errors(argv, capsys):
    from treelearn_amd.util.inventory import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err


def _csv_as_before(inv, names=None):
    """The CSV as write_inventory wrote it before the ground columns existed: COLUMNS, ints as str(int), floats as repr."""
    ints = ("tree_id", "n_points", "dbh_n", "crown_cells")
    f = io.StringIO(newline="")
    w = csv.writer(f)
    w.writerow(list(inv_ref.COLUMNS) + (["category"] if names else []))
    for i in range(len(inv["tree_id"])):
        row = [str(int(inv[k][i])) if k in ints else repr(float(inv[k][i])) for k in inv_ref.COLUMNS]
        w.writerow(row + ([names[i]] if names else []))
    return f.getvalue().encode()


def test_write_inventory_with_and_without_ground_columns(tmp_path):
    from treelearn_amd.util.inventory import write_inventory
    from treelearn_amd.util.segment import CATEGORIES
    xyz, lab, _ = cases.tree_on_flat_ground()
    lab = lab.copy()
    lab[-64:] = 3                                                      # a second tree and a gap: NaN rows in the CSV
    full = ref.tree_inventory(xyz, lab, ref.terrain_model(xyz, lab))
    plain = {k: full[k] for k in inv_ref.COLUMNS}
    write_inventory(str(tmp_path / "plain.csv"), plain)
    assert (tmp_path / "plain.csv").read_bytes() == _csv_as_before(plain)
    write_inventory(str(tmp_path / "plain_cat.csv"), plain, categories=[0, 1, 2])
    assert (tmp_path / "plain_cat.csv").read_bytes() == _csv_as_before(plain, [CATEGORIES[0], CATEGORIES[1], CATEGORIES[2]])
    write_inventory(str(tmp_path / "full.csv"), full, categories=[0, 1, 2])
    rows = list(csv.reader(open(tmp_path / "full.csv", newline="")))
    assert rows[0] == list(inv_ref.COLUMNS + ref.GROUND_COLUMNS) + ["category"] and len(rows) == 4
    before = list(csv.reader(io.StringIO(_csv_as_before(plain).decode(), newline="")))
    for r, b in zip(rows, before):
        assert r[:16] == b                                             # the sixteen columns keep their text
    j = rows[0].index("dbh_ag_n")
    assert [r[j] for r in rows[1:]] == [str(int(v)) for v in full["dbh_ag_n"]]
    j = rows[0].index("z_ground")
    assert [float(r[j]) for r in rows[1:2]] == [full["z_ground"][0]] and rows[2][j] == "nan"
