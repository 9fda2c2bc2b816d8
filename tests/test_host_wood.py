"""Host tests of the cylinder model, no GPU: the restatement against the closed forms of the hand cases and against an analytic
tree, the host-side rules of util.wood against the restatement's, check_params on every constraint, the argument parsers of the six
command lines, the files, and the entry points' declarations, exports and argument guards."""
import argparse
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import wood_cases as cases
import wood_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tl_wood_row_nodes": 10, "tl_wood_fit": 17}
# The analytic tree (wood_cases.surface_tree: a tapered trunk of 8 m and two limbs of 1.5 m, surface points, default parameters), measured
# on the restatement: wood_volume 0.524218 against the analytic 0.546323 (-4.05 %: the axis runs from the first node's centroid to the
# last one's, 7.68 of the 8 m, and a limb's first segment starts on the trunk's axis), axis_dbh 0.360459 against 0.361 (-0.15 %).
ANALYTIC_VOLUME_REL = 0.06              # measured 0.0405
ANALYTIC_DBH_ABS = 0.002                # measured 0.00054 m


def restated(case, offset=None):
    return ref.wood_structure(case["xyz"], case["lab"], case["tree"][:, 0], case["tree"][:, 1], case["tree"][:, 2], offset=offset,
                              branch_cfg=case["branch_cfg"], wood_cfg=case["wood_cfg"])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_on_the_hand_cases(name):
    """Every case's closed forms hold on the restatement, and its float decisions are farther than the margin from their thresholds."""
    case = cases.CASES[name]()
    want = restated(case)
    assert set(ref.MARGIN_KINDS) <= set(want["margins"]) and min(want["margins"].values()) > ref.MIN_MARGIN, want["margins"]
    case["check"](want)
    cyl, sk = want["cylinders"], want["skeleton"]
    assert tuple(cyl) == ref.CYLINDER_KEYS and cyl["n"].dtype == np.int64 and cyl["state"].dtype == np.int32 and want["row_node"].dtype == np.int32
    assert all(len(cyl[k]) == len(sk["parent"]) for k in ref.CYLINDER_KEYS[1:]) and cyl["centre"].shape == cyl["axis"].shape == (len(sk["parent"]), 3)
    # every row of a node is counted once, and only rows of reached voxels of trees with a skeleton belong to one
    assert np.array_equal(np.bincount(want["row_node"][want["row_node"] >= 0], minlength=len(cyl["n"])), cyl["n"])
    assert np.isnan(cyl["radius_fit"][cyl["state"] != 1]).all() and np.isfinite(cyl["radius_fit"][cyl["state"] == 1]).all()
    assert np.allclose(np.linalg.norm(cyl["axis"], axis=1), 1.0, rtol=0, atol=1e-15)


def test_analytic_tree_on_the_restatement():
    """Surface points on a tapered trunk and two limbs: the restatement's wood_volume and axis_dbh against the analytic values.  This
    judges the restatement (the GPU is only ever compared with the restatement)."""
    xyz, lab, an = cases.surface_tree()
    w = ref.tree_wood(xyz, lab)
    volume = an["trunk_volume"] + 2 * an["limb_volume"]
    dbh = 2 * an["r_at"](1.3)
    print(f"wood_volume {w['wood_volume'][0]:.6f} analytic {volume:.6f} rel {w['wood_volume'][0] / volume - 1:+.4f}; "
          f"axis_dbh {w['axis_dbh'][0]:.6f} analytic {dbh:.6f}")
    assert w["branch_count"][0] == 2 and w["skel_reached"][0] == w["skel_voxels"][0]
    assert abs(w["wood_volume"][0] / volume - 1) <= ANALYTIC_VOLUME_REL
    assert abs(w["axis_dbh"][0] - dbh) <= ANALYTIC_DBH_ABS
    assert abs(w["branch_volume_1"][0] / (2 * an["limb_volume"]) - 1) < 1.0       # the limbs' share is of the right order


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_host_rules_against_the_restatement(name):
    """util.wood.to_columns (steps 5-8, on the host) from the restatement's node table and fits: integers and states equal, floats to 1e-9."""
    from treelearn_amd.util.branches import check_params as check_branches
    from treelearn_amd.util.wood import CYLINDER_KEYS, FIT_KEYS, WOOD_COLUMNS, WOOD_INT_COLUMNS, check_params, to_columns
    case = cases.CASES[name]()
    off = np.array([10.5, -3.25, 100.0])
    want, plain = restated(case, offset=off), restated(case)
    fits = {k: plain["cylinders"][k] for k in FIT_KEYS}
    got = to_columns(plain["skeleton"], fits, case["tree"][:, 2], check_params(case["wood_cfg"]), check_branches(case["branch_cfg"]), off)
    assert tuple(got) == WOOD_COLUMNS + ("cylinders",) and WOOD_COLUMNS == ref.WOOD_COLUMNS and WOOD_INT_COLUMNS == ref.WOOD_INT
    assert tuple(got["cylinders"]) == CYLINDER_KEYS == ref.CYLINDER_KEYS
    for k in WOOD_COLUMNS:
        assert got[k].dtype == want[k].dtype and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        if k in WOOD_INT_COLUMNS:
            assert np.array_equal(got[k], want[k]), k
        else:
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-9, equal_nan=True), k
    for k in CYLINDER_KEYS:
        a, b = got["cylinders"][k], want["cylinders"][k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "i":
            assert np.array_equal(a, b), k
        else:
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a, b, rtol=0, atol=1e-9, equal_nan=True), k
    case["check"](dict(plain, **{k: got[k] for k in WOOD_COLUMNS}, cylinders=dict(got["cylinders"], centre=plain["cylinders"]["centre"])))


def test_check_params_on_every_constraint():
    from treelearn_amd.util.wood import WOOD_DEFAULTS, check_params
    assert WOOD_DEFAULTS == ref.WOOD_DEFAULTS == dict(min_points=8, max_rmse=0.03, min_radius=0.005, max_radius=1.0, max_growth=1.0, dbh_height=1.3)
    p = check_params()
    assert p == WOOD_DEFAULTS and type(p["min_points"]) is int and all(type(p[k]) is float for k in p if k != "min_points")
    assert check_params(dict(max_rmse=0.05, min_radius=None), min_points=3.0) == dict(WOOD_DEFAULTS, max_rmse=0.05, min_points=3)
    for ok in (dict(min_points=3), dict(max_rmse=0.0), dict(min_radius=0.0), dict(min_radius=0.5, max_radius=0.6), dict(max_growth=1.0), dict(dbh_height=0.0)):
        check_params(ok)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(min_points=2), dict(min_points=8.5), dict(min_points=True), dict(min_points=nan), dict(max_rmse=-0.01), dict(max_rmse=nan),
                dict(max_rmse=inf), dict(min_radius=-0.1), dict(min_radius=nan), dict(min_radius=1.0), dict(min_radius=2.0), dict(max_radius=inf),
                dict(max_radius=nan), dict(max_radius=0.005), dict(max_radius=-1.0), dict(max_growth=0.99), dict(max_growth=nan), dict(max_growth=inf),
                dict(dbh_height=-0.1), dict(dbh_height=nan), dict(dbh_height=inf), dict(radius=1.0)):
        with pytest.raises(ValueError):
            check_params(bad)


def test_argument_parsers(tmp_path):
    from treelearn_amd.util import branches, crown, inventory, segment, stem, wood
    ap = argparse.ArgumentParser()
    wood.add_arguments(ap)
    wood.add_arguments(ap)                                                # a second call adds nothing
    assert wood.params_of(ap.parse_args([])) == wood.WOOD_DEFAULTS
    a = ap.parse_args(["--wood-min-points", "5", "--wood-max-rmse", "0.05", "--wood-min-radius", "0.01", "--wood-max-radius", "0.8", "--wood-max-growth", "1.2",
                       "--wood-dbh-height", "1.0"])
    assert wood.params_of(a) == dict(min_points=5, max_rmse=0.05, min_radius=0.01, max_radius=0.8, max_growth=1.2, dbh_height=1.0)
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 4)))
    # a parameter outside its constraint ends every command line before any GPU work, and nothing is written
    with pytest.raises(SystemExit):
        wood.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--wood-min-points", "2"])
    with pytest.raises(SystemExit):
        wood.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--branch-reach", "3"])
    with pytest.raises(SystemExit):
        wood.main(["--forest", str(forest)])
    with pytest.raises(SystemExit):
        branches.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--wood", "--wood-max-growth", "0.5"])
    with pytest.raises(SystemExit):
        inventory.main(["--forest", str(forest), "--out", str(tmp_path / "o.csv"), "--wood", "--wood-max-rmse", "-1"])
    with pytest.raises(SystemExit):
        stem.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--wood", "--wood-min-radius", "2"])
    with pytest.raises(SystemExit):
        crown.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--wood", "--wood-dbh-height", "-1"])
    (tmp_path / "w.pth").write_bytes(b"")
    common = ["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    with pytest.raises(SystemExit):
        segment.parse_args(common + ["--wood", "--wood-max-radius", "0"])
    a = segment.parse_args(common + ["--wood", "--wood-min-points", "12", "--wood-max-growth", "1.1"])
    assert a.wood and not a.branches and wood.params_of(a) == dict(wood.WOOD_DEFAULTS, min_points=12, max_growth=1.1)
    assert not segment.parse_args(common).wood and wood.params_of(segment.parse_args(common)) == wood.WOOD_DEFAULTS
    assert not (tmp_path / "o.npz").exists() and not (tmp_path / "o.csv").exists()
    with pytest.raises(ValueError):                                       # the API checks before any GPU work too
        segment.segment_forest(None, None, wood=True, wood_cfg=dict(min_points=1))
    with pytest.raises(ValueError):
        segment.segment_forest(None, None, wood=True, branch_cfg=dict(voxel=0.0))
    with pytest.raises(ValueError):
        inventory.tree_inventory(None, None, wood=True, wood_cfg=dict(max_growth=0.5))
    with pytest.raises(ValueError):
        inventory.tree_inventory(None, None, wood=True, branch_cfg=dict(reach=5))     # wood implies branches
    with pytest.raises(ValueError):
        inventory.cloud_inventory(np.zeros((1, 4)), wood=True, wood_cfg=dict(nothing=1))


def _inventory_of(case):
    """An inventory dict as tree_inventory(..., wood=True) returns it, from the restatements (no GPU)."""
    import inventory_restatement as inv_ref
    import branches_restatement as br_ref
    res = dict(inv_ref.tree_inventory(case["xyz"], case["lab"]))
    want = restated(case)
    res.update({k: want[k] for k in br_ref.BRANCH_COLUMNS + ("skeleton",) + ref.WOOD_COLUMNS + ("cylinders",)})
    return res


def test_write_inventory_column_order(tmp_path):
    from treelearn_amd.util.branches import BRANCH_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, write_inventory
    from treelearn_amd.util.wood import WOOD_COLUMNS, WOOD_INT_COLUMNS
    inv = _inventory_of(cases.CASES["empty_slots"]())
    rows = list(csv.reader(open(write_inventory(str(tmp_path / "w.csv"), inv), newline="")))
    assert rows[0] == list(COLUMNS + BRANCH_COLUMNS + WOOD_COLUMNS) and len(rows) == 5
    at = len(COLUMNS + BRANCH_COLUMNS)
    for i, row in enumerate(rows[1:]):
        for k, cell in zip(WOOD_COLUMNS, row[at:]):
            if k in WOOD_INT_COLUMNS:
                assert cell == str(int(inv[k][i])), k
            else:
                assert cell == "nan" if np.isnan(inv[k][i]) else float(cell) == inv[k][i], k
    assert [r[at] for r in rows[1:]] == ["4", "0", "0", "3"]
    # without all nine: the columns of before, the same bytes
    plain = {k: inv[k] for k in COLUMNS + BRANCH_COLUMNS}
    partial = dict(plain, wood_volume=inv["wood_volume"], cylinders=inv["cylinders"])
    assert open(write_inventory(str(tmp_path / "p.csv"), partial), "rb").read() == open(write_inventory(str(tmp_path / "q.csv"), plain), "rb").read()
    assert list(csv.reader(open(tmp_path / "q.csv", newline="")))[0] == list(COLUMNS + BRANCH_COLUMNS)


def test_write_cylinders_round_trip(tmp_path):
    from treelearn_amd.util.wood import CYLINDER_KEYS, write_cylinders
    inv = _inventory_of(cases.CASES["two_trees"]())
    with np.load(write_cylinders(str(tmp_path / "c.npz"), inv)) as f:
        assert set(f.files) == {"tree_id"} | set(CYLINDER_KEYS) and f["tree_id"].tolist() == [1, 2] and f["tree_id"].dtype == np.int64
        for k in CYLINDER_KEYS:
            assert f[k].dtype == inv["cylinders"][k].dtype and f[k].tobytes() == inv["cylinders"][k].tobytes(), k
        assert f["node_start"].dtype == np.int64 and f["n"].dtype == np.int64 and f["state"].dtype == np.int32 and f["centre"].shape == (11, 3)
    with pytest.raises(ValueError):
        write_cylinders(str(tmp_path / "none.npz"), {k: v for k, v in inv.items() if k != "cylinders"})


def test_header_declares_and_library_exports_the_entry_points():
    """The two symbols are declared in a section of their own, bound with matching arity and exported; they refuse nulls, misaligned
    pointers, sizes and bad parameters before anything else, and return TL_OK without a launch for nothing to do (host memory: no GPU)."""
    from treelearn_amd import _hip, build as b
    from treelearn_amd.util.wood import check_params
    header = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    assert "csrc/tl_wood.hip, DESIGN §24" in header and "typedef struct tl_wood_params" in header
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES[name][1]), name
    L = ctypes.CDLL(b.build(verbose=False))
    assert all(hasattr(L, name) for name in ENTRY_POINTS)
    assert [f[0] for f in _hip.WoodParams._fields_] == ["max_rmse", "min_radius", "max_radius", "max_growth", "dbh_height", "min_points"]
    assert ctypes.sizeof(_hip.WoodParams) == 48
    lib = _hip.lib()
    good = _hip.WoodParams(**check_params())
    buf = (ctypes.c_double * 64)()                                       # host memory: only its address and alignment are looked at
    p, odd, odd2 = (ctypes.c_void_p(ctypes.addressof(buf) + k) for k in (0, 4, 2))
    rows = lambda *a: lib.tl_wood_row_nodes(*a, None)                     # noqa: E731
    fit = lambda *a: lib.tl_wood_fit(*a, None)                            # noqa: E731
    ok, bad = _hip.TL_OK, _hip.TL_ERR_ARG
    # nothing to do, found out after the argument checks and without a launch
    assert rows(p, 0, p, 5, p, p, p, 3, p) == ok and rows(p, 5, p, 5, p, p, p, 0, p) == ok and rows(p, 5, p, 0, p, p, p, 0, p) == ok
    assert fit(p, 0, p, p, p, p, p, 2, 3, good, p, p, p, p, p, p) == ok and fit(p, 5, p, p, p, p, p, 2, 0, good, p, p, p, p, p, p) == ok
    assert fit(p, 5, p, p, p, p, p, 0, 3, good, p, p, p, p, p, p) == ok
    # nulls, misaligned pointers, sizes
    assert rows(None, 0, p, 5, p, p, p, 3, p) == bad and rows(p, 0, p, 5, p, p, p, 3, None) == bad and rows(odd, 0, p, 5, p, p, p, 3, p) == bad
    assert rows(p, 0, odd, 5, p, p, p, 3, p) == bad and rows(p, 0, p, 5, odd2, p, p, 3, p) == bad and rows(p, 0, p, 5, odd, odd, odd, 3, odd) == ok
    assert rows(p, -1, p, 5, p, p, p, 3, p) == bad and rows(p, 0, p, -1, p, p, p, 0, p) == bad and rows(p, 0, p, 1 << 31, p, p, p, 3, p) == bad
    assert rows(p, 0, p, 5, p, p, p, 6, p) == bad and rows(p, 0, p, 5, p, p, p, -1, p) == bad
    assert fit(None, 0, p, p, p, p, p, 2, 3, good, p, p, p, p, p, p) == bad and fit(p, 0, p, p, p, p, p, 2, 3, None, p, p, p, p, p, p) == bad
    assert fit(p, 0, odd, p, p, p, p, 2, 3, good, p, p, p, p, p, p) == bad and fit(p, 0, p, p, p, odd2, p, 2, 3, good, p, p, p, p, p, p) == bad
    assert fit(p, 0, p, p, p, odd, p, 2, 3, good, p, p, p, odd, p, p) == ok and fit(p, 0, p, p, p, p, p, 2, 3, good, p, odd, p, p, p, p) == bad
    assert fit(p, 0, p, p, p, p, p, 2, 3, good, p, p, p, p, p, None) == bad and fit(p, 0, p, p, p, p, p, 2, 3, good, p, p, p, p, odd, p) == bad
    assert fit(p, -1, p, p, p, p, p, 2, 3, good, p, p, p, p, p, p) == bad and fit(p, 0, p, p, p, p, p, -1, 3, good, p, p, p, p, p, p) == bad
    assert fit(p, 0, p, p, p, p, p, 2, -1, good, p, p, p, p, p, p) == bad and fit(p, 0, p, p, p, p, p, 2, 1 << 31, good, p, p, p, p, p, p) == bad
    nan, inf = float("nan"), float("inf")
    for wrong in (dict(min_points=2), dict(max_rmse=-0.01), dict(max_rmse=nan), dict(max_rmse=inf), dict(min_radius=-0.1), dict(min_radius=nan),
                  dict(min_radius=1.0), dict(max_radius=inf), dict(max_radius=nan), dict(max_radius=0.001), dict(max_growth=0.5), dict(max_growth=nan),
                  dict(max_growth=inf), dict(dbh_height=-1.0), dict(dbh_height=nan), dict(dbh_height=inf)):
        with pytest.raises(ValueError):
            check_params(wrong)                                           # the host check and the library's agree
        wp = _hip.WoodParams(**dict(check_params(), **wrong))
        assert fit(p, 0, p, p, p, p, p, 2, 3, wp, p, p, p, p, p, p) == bad, wrong
