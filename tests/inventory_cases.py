"""Inventory cases worked by hand, shared by tests/test_host_inventory.py (through the numpy restatement) and tests/test_gpu_inventory.py
(through tl_tree_inventory).  Each case is (coords f64 [N, 3], labels i64 [N], check): check(inv) asserts on the returned columns."""
import numpy as np

NAN = np.isnan


def _stem(cx, cy, r, zs, n_ang, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n_ang) / n_ang
    return np.concatenate([np.column_stack([cx + r * np.cos(a), cy + r * np.sin(a), np.full(n_ang, z)]) for z in zs])


def _base(cx, cy, z=0.0):
    """Four base rows at height z whose mean is (cx, cy) up to rounding: they fix z_low = z (rank 3 of more than 11 rows) and the position."""
    return np.array([[cx + 0.125, cy, z], [cx - 0.125, cy, z], [cx, cy + 0.125, z], [cx, cy - 0.125, z]])


def _shuffled(xyz, labels, seed):
    p = np.random.default_rng(seed).permutation(len(xyz))
    return np.ascontiguousarray(xyz[p]), np.ascontiguousarray(labels[p])


def case_rank3():
    """Trees of 11, 12 and 13 rows with duplicated z: more than 11 rows take rank 3 from either end, 11 rows the extremes."""
    z11 = [0, 0, 0, 0.5, 1, 2, 3, 4, 4, 4, 5]                     # min 0, max 5
    z12 = [0, 0, 0, 0.5, 0.5, 1, 2, 3, 4, 4, 4, 5]                # sorted[3] = 0.5, sorted[-4] = 4
    z13 = [1, 1, 1, 1, 1, 2, 3, 7, 8, 9, 9, 9, 9]                 # sorted[3] = 1,   sorted[-4] = 9
    rows, lab = [], []
    for t, zs in enumerate((z11, z12, z13), start=1):
        k = np.arange(len(zs), dtype=np.float64)
        rows.append(np.column_stack([10.0 * t + 0.01 * k, -5.0 + 0.02 * k, np.asarray(zs, np.float64)]))
        lab.append(np.full(len(zs), t))
    xyz, lab = _shuffled(np.concatenate(rows), np.concatenate(lab).astype(np.int64), 1)

    def check(inv):
        assert inv["n_points"].tolist() == [11, 12, 13]
        assert inv["z_low"].tolist() == [0.0, 0.5, 1.0]
        assert inv["z_top"].tolist() == [5.0, 4.0, 9.0]
        assert inv["height"].tolist() == [5.0, 3.5, 8.0]
        # base rows: z <= z_low + 0.5 -> the rows of z in {0, 0.5}: k = 0..3; {0, 0.5, 0.5, 1}: k = 0..5; z = 1: k = 0..4
        assert abs(inv["x"][0] - (10.0 + 0.01 * 1.5)) < 1e-12 and abs(inv["y"][1] - (-5.0 + 0.02 * 2.5)) < 1e-12
        assert abs(inv["x"][2] - (30.0 + 0.01 * 2.0)) < 1e-12 and abs(inv["z"][1] - (0.0 * 3 + 0.5 * 2 + 1) / 6) < 1e-12
        assert inv["dbh_n"].tolist() == [0, 0, 0] and NAN(inv["dbh"]).all()
    return xyz, lab, check


def case_circle():
    """32 angles x two z layers exactly on a circle of radius 0.15 around (3, -2): dbh 0.30, centre and rmse to 1e-12."""
    xyz = np.concatenate([_base(3.0, -2.0), _stem(3.0, -2.0, 0.15, (1.25, 1.35), 32), [[3.0, -2.0, 6.0]] * 4])
    xyz, lab = _shuffled(xyz, np.ones(len(xyz), np.int64), 2)

    def check(inv):
        assert inv["n_points"].tolist() == [72] and inv["z_low"][0] == 0.0 and inv["z_top"][0] == 6.0
        assert abs(inv["x"][0] - 3.0) < 1e-12 and abs(inv["y"][0] + 2.0) < 1e-12 and inv["z"][0] == 0.0
        assert inv["dbh_n"].tolist() == [64]
        assert abs(inv["dbh"][0] - 0.30) <= 1e-12
        assert abs(inv["dbh_x"][0] - 3.0) <= 1e-12 and abs(inv["dbh_y"][0] + 2.0) <= 1e-12
        assert 0 <= inv["dbh_rmse"][0] <= 1e-12
    return xyz, lab, check


def case_degenerate():
    """Tree 1: ten collinear slice rows; tree 2: seven rows on a circle; tree 3: ten coincident rows.  No DBH, dbh_n still reported."""
    k = np.arange(10, dtype=np.float64)
    line = np.column_stack([3.0 + 0.01 * k, -2.0 + 0.02 * k, np.full(10, 1.3)])
    xyz = np.concatenate([_base(3.0, -2.0), line, _base(13.0, -2.0), _stem(13.0, -2.0, 0.15, (1.3,), 7), _base(23.0, -2.0),
                          np.tile([[23.05, -2.0, 1.3]], (10, 1))])
    lab = np.concatenate([np.full(14, 1), np.full(11, 2), np.full(14, 3)]).astype(np.int64)
    xyz, lab = _shuffled(xyz, lab, 3)

    def check(inv):
        assert inv["dbh_n"].tolist() == [10, 7, 10]
        for c in ("dbh", "dbh_x", "dbh_y", "dbh_rmse"):
            assert NAN(inv[c]).all(), c
        assert not NAN(inv["x"]).any() and inv["height"].tolist() == [1.3, 1.3, 1.3]
    return xyz, lab, check


def case_slice_bounds():
    """z exactly at the slice's lower bound is in, exactly at the upper bound is out; a row at dbh_max_radius or beyond is out."""
    lo, hi = (0.0 + 1.3) - 0.2 / 2, (0.0 + 1.3) + 0.2 / 2          # the bounds as every implementation computes them
    ring = _stem(3.0, -2.0, 0.15, (1.3,), 8)
    extra = np.array([[3.15, -2.0, lo], [3.0, -1.85, np.nextafter(lo, -np.inf)], [2.85, -2.0, hi], [3.0, -2.15, np.nextafter(hi, -np.inf)],
                      [3.0 + 1.5, -2.0, 1.3], [3.0, -2.0 + 0.99, 1.3], [4.0, -2.0, 1.3]])      # the last: u = 1.0 exactly
    xyz = np.concatenate([_base(3.0, -2.0), ring, extra])
    xyz, lab = _shuffled(xyz, np.ones(len(xyz), np.int64), 4)

    def check(inv):
        assert inv["n_points"].tolist() == [19] and inv["z_low"][0] == 0.0 and inv["x"][0] == 3.0
        assert inv["dbh_n"].tolist() == [8 + 3]                    # lo, just under hi, and the row 0.99 m away
    return xyz, lab, check


def case_crown():
    """Crown cells of 0.25 m over negative coordinates and rows exactly on cell borders (floor, not truncation)."""
    x = np.array([-0.25, -0.2500001, -1e-9, -0.0, 0.0, 0.2499999, 0.25, 0.25, -0.5, 0.1])
    y = np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.0, -0.25, -0.5, -1e-12])
    # cells: (-1,0) (-2,0) (-1,0) (0,0) (0,0) (0,0) (1,0) (1,-1) (-2,-2) (0,-1)  ->  7 distinct
    xyz = np.column_stack([x, y, np.linspace(0, 1, len(x))])
    lab = np.ones(len(x), np.int64)

    def check(inv):
        assert inv["crown_cells"].tolist() == [7]
        assert inv["crown_area"][0] == 7 * 0.0625
        assert abs(inv["crown_diameter"][0] - 2 * np.sqrt(7 * 0.0625 / np.pi)) < 1e-15
    return xyz, lab, check


def case_gap():
    """Labels {1, 3} (and 0, -1, which are ignored): tree 2 has no rows and NaN in every float column."""
    xyz = np.array([[0.0, 0, 0], [1.0, 1, 1], [5.0, 5, 0], [9.0, 9, 9], [9.0, 9, 9]])
    lab = np.array([1, 1, 3, 0, -1], np.int64)

    def check(inv):
        assert inv["tree_id"].tolist() == [1, 2, 3] and inv["n_points"].tolist() == [2, 0, 1]
        assert inv["dbh_n"].tolist() == [0, 0, 0] and inv["crown_cells"].tolist() == [2, 0, 1]
        for c in ("x", "y", "z", "z_low", "z_top", "height", "dbh", "dbh_x", "dbh_y", "dbh_rmse", "crown_area", "crown_diameter"):
            assert NAN(inv[c][1]), c
        assert inv["z_low"][0] == 0.0 and inv["z_top"][0] == 1.0 and inv["height"][2] == 0.0
        assert inv["x"][0] == 0.0 and inv["x"][2] == 5.0          # base rows: z <= z_low + 0.5
    return xyz, lab, check


def case_empty():
    """No label >= 1: no trees, every column of length 0."""
    xyz = np.zeros((3, 3))
    lab = np.array([0, -1, 0], np.int64)

    def check(inv):
        assert all(len(v) == 0 for v in inv.values()) and inv["n_points"].dtype == np.int64
    return xyz, lab, check


CASES = dict(rank3=case_rank3, circle=case_circle, degenerate=case_degenerate, slice_bounds=case_slice_bounds, crown=case_crown,
             gap=case_gap, empty=case_empty)


def offset_case():
    """The circle case with an offset: the shifted columns move by it, the others do not."""
    xyz, lab, _ = case_circle()
    off = np.array([1000.0, 2000.0, 50.0])

    def check(inv, plain):
        for k, a in (("x", 0), ("y", 1), ("z", 2), ("z_low", 2), ("z_top", 2), ("dbh_x", 0), ("dbh_y", 1)):
            assert np.array_equal(inv[k], plain[k] + off[a]), k
        for k in ("height", "dbh", "dbh_rmse", "dbh_n", "n_points", "crown_cells", "crown_area", "crown_diameter"):
            assert np.array_equal(inv[k], plain[k], equal_nan=True), k
    return xyz, lab, off, check
