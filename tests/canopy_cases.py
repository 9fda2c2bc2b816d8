"""Canopy cases worked by hand, shared by tests/test_host_canopy.py (the numpy restatement) and tests/test_gpu_canopy.py
(the kernels).  CASES: name -> function returning a dict: xyz f64[N, 3], h f64[N] (the height above ground handed in; None when
terrain_cfg is given: the test then takes it from the terrain of the label-0 rows), labels i64[N] or None, params, check; check(c)
asserts the hand values on c, a dict with the keys of canopy_restatement.canopy_model (numpy arrays / ints).  CHM cells are 0.5 m; all
clouds fit one 10 m metrics cell unless the case says otherwise."""
import numpy as np

NAN = float("nan")


def _cloud(H, c=0.5):
    """One row at the centre of every cell of H [ny, nx] that holds a number, with that height (z = h)."""
    H = np.asarray(H, np.float64)
    j, i = np.nonzero(~np.isnan(H))
    return np.column_stack([(i + 0.5) * c, (j + 0.5) * c, H[j, i]]), H[j, i].copy()


def _shape(c, nx, ny, ix0=0, iy0=0):
    assert (c["ix0"], c["iy0"], c["nx"], c["ny"]) == (ix0, iy0, nx, ny), (c["ix0"], c["iy0"], c["nx"], c["ny"])
    for k, dt in (("n", np.int32), ("top", np.float64), ("owner", np.int32), ("chm", np.float64), ("state", np.uint8), ("tops_mask", np.uint8)):
        assert c[k].shape == (ny, nx) and c[k].dtype == dt, (k, c[k].shape, c[k].dtype)
    for k, dt in (("metric_n", np.int32), ("metric_n_veg", np.int32), ("cover", np.float64), ("h_max", np.float64), ("h_mean", np.float64),
                  ("h_sd", np.float64)):
        assert c[k].shape == (c["metric_ny"], c["metric_nx"]) and c[k].dtype == dt, (k, c[k].shape, c[k].dtype)
    assert c["percentiles"].dtype == np.float64 and c["layers"].dtype == np.int32
    assert c["tops"]["i"].dtype == c["tops"]["j"].dtype == np.int64 and c["tops"]["owner"].dtype == np.int32


def _tops(c, want):
    """want: a list of (i, j, h) in row-major order."""
    t = c["tops"]
    assert list(zip(t["i"].tolist(), t["j"].tolist(), t["h"].tolist())) == want, (t["i"], t["j"], t["h"])
    assert int(c["tops_mask"].sum()) == len(want)
    assert np.array_equal(t["x"], (c["ix0"] + t["i"] + 0.5) * 0.5) and np.array_equal(t["y"], (c["iy0"] + t["j"] + 0.5) * 0.5)


def _same(a, b):
    assert np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True), (a, b)


def _case(H, check, labels=None, **params):
    xyz, h = _cloud(H)
    return dict(xyz=xyz, h=h, labels=labels, params=params, check=check, terrain_cfg=None)


def _rows(h, check, labels=None, x=None, **params):
    """Rows of the given heights in the cell [0, 0.5)^2 (or at the given x, y = 0.25)."""
    h = np.asarray(h, np.float64)
    x = np.full(len(h), 0.25) if x is None else np.asarray(x, np.float64)
    xyz = np.column_stack([x, np.full(len(h), 0.25), h])
    return dict(xyz=xyz, h=h, labels=None if labels is None else np.asarray(labels, np.int64), params=params, check=check, terrain_cfg=None)


def flat():
    """5 x 5 cells at 10 m: nothing is a pit, the plateau gives one top at cell (0, 0), whose window of 4 cells spans the grid.  One
    metrics cell: 25 rows, all vegetation, cover 1, mean 10, sd 0, every percentile 10; L = floor(10 / 1) + 1 = 11, all rows in layer 10."""
    def check(c):
        _shape(c, 5, 5)
        assert (c["n"] == 1).all() and (c["top"] == 10.0).all() and (c["chm"] == 10.0).all() and (c["state"] == 1).all() and (c["owner"] == -1).all()
        _tops(c, [(0, 0, 10.0)])
        assert (c["tops"]["x"][0], c["tops"]["y"][0]) == (0.25, 0.25) and c["tops"]["owner"][0] == -1 and "tops_per_tree" not in c
        assert (c["metric_nx"], c["metric_ny"], c["metric_ix0"], c["metric_iy0"]) == (1, 1, 0, 0)
        assert c["metric_n"][0, 0] == 25 and c["metric_n_veg"][0, 0] == 25 and c["cover"][0, 0] == 1.0 and c["h_max"][0, 0] == 10.0
        assert c["h_mean"][0, 0] == 10.0 and c["h_sd"][0, 0] == 0.0 and (c["percentiles"][0, 0] == 10.0).all() and c["percentiles"].shape == (1, 1, 5)
        assert c["layers"].shape == (1, 1, 11) and c["layers"][0, 0].tolist() == [0] * 10 + [25]
        assert c["n_no_ground"] == 0 and c["n_clipped"] == 0
    return _case(np.full((5, 5), 10.0), check)


def _pit(centre):
    H = np.full((3, 3), 12.0)
    H[1, 1] = centre
    return H


def pit_exactly_on_the_bound():
    """3 x 3 cells at 12 m, the centre at 10 m: the median of its 8 neighbours is 12, 12 - 10 = 2.0 is not > pit_depth = 2.0: kept.  An
    edge cell has 5 neighbours, 10 12 12 12 12, median 12, no pit; a corner has 3 < 5."""
    def check(c):
        _shape(c, 3, 3)
        assert (c["state"] == 1).all()
        _same(c["chm"], _pit(10.0)); _same(c["top"], _pit(10.0))
        _tops(c, [(0, 0, 12.0)])
    return _case(_pit(10.0), check)


def pit_one_ulp_deeper():
    """The same with the centre one ulp below 10: 12 - h = 2 + 4 ulp(2) > 2.0: filled with the median 12, state 2; top keeps the raw value."""
    low = np.nextafter(10.0, 0.0)

    def check(c):
        _shape(c, 3, 3)
        want = np.ones((3, 3), np.uint8); want[1, 1] = 2
        assert np.array_equal(c["state"], want) and (c["chm"] == 12.0).all() and c["top"][1, 1] == low and c["n"][1, 1] == 1
        _tops(c, [(0, 0, 12.0)])
    return _case(_pit(low), check)


def pits_off():
    """pit_min_neighbours = 9 can never be met: the pit one ulp too deep stays, and so would any hole."""
    low = np.nextafter(10.0, 0.0)

    def check(c):
        assert (c["state"] == 1).all()
        _same(c["chm"], _pit(low))
    return _case(_pit(low), check, pit_min_neighbours=9)


def even_neighbours_at_a_corner():
    """pit_min_neighbours = 2.  rows j = 0: 1 10 10; j = 1: 13 - 10; j = 2: 10 10 10.  The corner (0, 0) has two neighbours with a value,
    10 and 13: median (10 + 13) / 2 = 11.5, 11.5 - 1 > 2: filled, state 2.  The empty centre has 8: 1 10 10 10 10 10 10 13, median (10 +
    10) / 2 = 10, state 3.  (0, 1): 1 10 10 13 -> 10; (1, 0): 1 10 10 10 -> 10, the cell is higher; (2, 0): 10 13 -> 11.5, 1.5 is not > 2.
    The only top is the 13 at i = 0, j = 1."""
    H = [[1.0, 10.0, 10.0], [13.0, NAN, 10.0], [10.0, 10.0, 10.0]]

    def check(c):
        _shape(c, 3, 3)
        _same(c["chm"], [[11.5, 10.0, 10.0], [13.0, 10.0, 10.0], [10.0, 10.0, 10.0]])
        assert c["state"].tolist() == [[2, 1, 1], [1, 3, 1], [1, 1, 1]] and c["n"][1, 1] == 0 and np.isnan(c["top"][1, 1]) and c["top"][0, 0] == 1.0
        _tops(c, [(0, 1, 13.0)])
    return _case(H, check, pit_min_neighbours=2)


def holes():
    """rows j = 0: 10 10 10 -; j = 1: 10 - 10 -; j = 2: 10 10 10 8.  The hole (1, 1) has 8 neighbours at 10: filled with 10, state 3.  The
    hole (0, 3) has 2 and the hole (1, 3) has 4 (10 10 10 8), fewer than 5: NaN, state 0.  (1, 2) has 5: 8 10 10 10 10, median 10: no pit."""
    H = [[10.0, 10.0, 10.0, NAN], [10.0, NAN, 10.0, NAN], [10.0, 10.0, 10.0, 8.0]]

    def check(c):
        _shape(c, 4, 3)
        _same(c["chm"], [[10.0, 10.0, 10.0, NAN], [10.0, 10.0, 10.0, NAN], [10.0, 10.0, 10.0, 8.0]])
        assert c["state"].tolist() == [[1, 1, 1, 0], [1, 3, 1, 0], [1, 1, 1, 1]]
        assert c["n"].tolist() == [[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 1, 1]] and (c["owner"] == -1).all()
        _tops(c, [(0, 0, 10.0)])
        assert c["metric_n"][0, 0] == 9
    return _case(H, check)


def plateau_of_two_cells():
    """top_window = 1.  rows j = 0: 6 9 9; j = 1: 6 6 6.  The two 9s tie: the one with the lower row-major index, i = 1, j = 0, is the
    top.  Every 6 has a 9 or an equal cell of lower index next to it."""
    def check(c):
        _shape(c, 3, 2)
        assert (c["state"] == 1).all()
        _tops(c, [(1, 0, 9.0)])
        assert (c["tops"]["x"][0], c["tops"]["y"][0]) == (0.75, 0.25)
    return _case([[6.0, 9.0, 9.0], [6.0, 6.0, 6.0]], check, top_window=1)


def tops_on_the_border():
    """top_window = 1.  20 m in the corner (0, 0), 15 m in the corner (2, 2), 6 m elsewhere: both corners are tops with their windows
    clipped to 2 x 2 cells; the median of the centre's neighbours is 6, nothing is a pit."""
    H = np.full((3, 3), 6.0); H[0, 0] = 20.0; H[2, 2] = 15.0

    def check(c):
        _shape(c, 3, 3)
        assert (c["state"] == 1).all()
        _tops(c, [(0, 0, 20.0), (2, 2, 15.0)])
    return _case(H, check, top_window=1)


def maximum_below_top_min_height():
    """The highest cell is at 4 m < top_min_height = 5 m: no top; with labels tops_per_tree is all 0."""
    def check(c):
        _shape(c, 2, 2)
        _tops(c, [])
        assert c["tops"]["x"].shape == (0,) and c["tops_per_tree"].tolist() == [0, 0] and c["tops_per_tree"].dtype == np.int32
        assert c["owner"].tolist() == [[1, 1], [2, 2]]
    return _case([[1.0, 2.0], [3.0, 4.0]], check, labels=np.array([1, 1, 2, 2], np.int64))


def owner_tie():
    """Cell 0 holds rows of 7 m (label 2), 7 m (label 5) and 3 m (label 9); cell 1 one row of 4 m (label 1).  Labels 2 and 5 tie for the
    maximum of cell 0: the larger, 5, owns it; label 9 is lower down.  The one top (7 m) belongs to tree 5 of T = 9."""
    def check(c):
        _shape(c, 2, 1)
        assert c["owner"].tolist() == [[5, 1]] and c["n"].tolist() == [[3, 1]] and c["top"].tolist() == [[7.0, 4.0]]
        _tops(c, [(0, 0, 7.0)])
        assert c["tops"]["owner"].tolist() == [5] and c["tops_per_tree"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    return _rows([7.0, 7.0, 3.0, 4.0], check, labels=[2, 5, 9, 1], x=[0.1, 0.2, 0.3, 0.75])


def owner_label_0():
    """Cell 0: 9 m with label 0 over 2 m with label 3; cell 1: 6 m with label 3.  Label 0 owns cell 0 and its top, which counts for no
    tree; a cell whose highest row has label -1 has owner -1."""
    def check(c):
        _shape(c, 3, 1)
        assert c["owner"].tolist() == [[0, 3, -1]]
        _tops(c, [(0, 0, 9.0)])
        assert c["tops"]["owner"].tolist() == [0] and c["tops_per_tree"].tolist() == [0, 0, 0]
    return _rows([9.0, 2.0, 6.0, 5.5], check, labels=[0, 3, 3, -1], x=[0.1, 0.2, 0.75, 1.25])


def height_equal_to_the_cutoff():
    """Rows at 2.0, 2.0, 3.0 and 1.0 m with cutoff 2.0: only the 3.0 is vegetation (strict).  cover = 1 / 4; one vegetation row: mean 3, sd
    0 and every percentile 3."""
    def check(c):
        assert c["metric_n"][0, 0] == 4 and c["metric_n_veg"][0, 0] == 1 and c["cover"][0, 0] == 0.25 and c["h_max"][0, 0] == 3.0
        assert c["h_mean"][0, 0] == 3.0 and c["h_sd"][0, 0] == 0.0 and (c["percentiles"][0, 0] == 3.0).all()
        assert c["layers"][0, 0].tolist() == [0, 1, 2, 1]
    return _rows([2.0, 2.0, 3.0, 1.0], check)


def percentiles_0_and_100():
    """Vegetation rows 3 4 5 6 10 (and 1 m below the cutoff), percentiles 0, 50, 100, 25, 90: m - 1 = 4; 0 -> v[0] = 3; 50 -> pos 2 -> 5; 100
    -> pos 4 -> 10; 25 -> pos 1 -> 4; 90 -> pos 3.6 -> 6 + (10 - 6) * 0.6 = 8.4.  mean 28 / 5 = 5.6, sd = sqrt(29.2 / 5)."""
    def check(c):
        assert c["metric_n"][0, 0] == 6 and c["metric_n_veg"][0, 0] == 5 and c["percentiles"].shape == (1, 1, 5)
        got = c["percentiles"][0, 0]
        assert got[:4].tolist() == [3.0, 5.0, 10.0, 4.0] and abs(got[4] - 8.4) <= 1e-12
        assert abs(c["h_mean"][0, 0] - 5.6) <= 1e-12 and abs(c["h_sd"][0, 0] - np.sqrt(29.2 / 5.0)) <= 1e-12 and c["cover"][0, 0] == 5.0 / 6.0
    return _rows([10.0, 1.0, 4.0, 3.0, 6.0, 5.0], check, percentiles=(0, 50, 100, 25, 90))


def negative_heights():
    """Rows at -0.5, -3.0, 0.2 and 1.5 m: L = floor(1.5 / 1) + 1 = 2; the negative rows count in layer 0 with the 0.2: layers 3, 1.  No
    vegetation: cover 0, h_max 1.5, mean, sd and percentiles NaN."""
    def check(c):
        assert c["layers"].shape == (1, 1, 2) and c["layers"][0, 0].tolist() == [3, 1] and c["n_clipped"] == 0
        assert c["metric_n"][0, 0] == 4 and c["metric_n_veg"][0, 0] == 0 and c["cover"][0, 0] == 0.0 and c["h_max"][0, 0] == 1.5
        assert np.isnan(c["h_mean"][0, 0]) and np.isnan(c["h_sd"][0, 0]) and np.isnan(c["percentiles"][0, 0]).all()
        assert c["top"][0, 0] == 1.5
    return _rows([-0.5, -3.0, 0.2, 1.5], check)


def rows_above_the_last_layer():
    """max_layers = 3: L = min(3, floor(9.9) + 1) = 3.  Rows 0.5 1.5 2.5 7.0 9.9: layers 1, 1, 3; the rows at 7.0 and 9.9 lie at or above
    L * layer = 3 m: n_clipped = 2."""
    def check(c):
        assert c["layers"].shape == (1, 1, 3) and c["layers"][0, 0].tolist() == [1, 1, 3] and c["n_clipped"] == 2
    return _rows([0.5, 1.5, 2.5, 7.0, 9.9], check, max_layers=3)


def rows_over_missing_ground():
    """Three cells in a row, terrain fill_radius = 0.  Ground rows (label 0, z = 0) at the centres of cells 0 and 1, a tree row 8 m up over
    cell 1, two tree rows over cell 2, which has no ground and is not filled: their height is NaN, they are skipped and counted.  The
    row over cell 1 sits between a ground cell and a NaN cell, so it takes the value of its own cell: h = 8."""
    xyz = np.array([[0.25, 0.25, 0.0], [0.75, 0.25, 0.0], [0.75, 0.25, 8.0], [1.25, 0.25, 9.0], [1.3, 0.2, 7.0]])
    lab = np.array([0, 0, 1, 1, 1], np.int64)

    def check(c):
        _shape(c, 3, 1)
        assert c["n"].tolist() == [[1, 2, 0]] and c["n_no_ground"] == 2 and c["owner"].tolist() == [[0, 1, -1]]
        _same(c["top"], [[0.0, 8.0, NAN]]); _same(c["chm"], [[0.0, 8.0, NAN]])
        assert c["state"].tolist() == [[1, 1, 0]] and c["metric_n"][0, 0] == 3 and c["metric_n_veg"][0, 0] == 1
        _tops(c, [(1, 0, 8.0)])
        assert c["tops_per_tree"].tolist() == [1]
    return dict(xyz=xyz, h=None, labels=lab, params={}, check=check, terrain_cfg=dict(fill_radius=0))


CASES = {f.__name__: f for f in (flat, pit_exactly_on_the_bound, pit_one_ulp_deeper, pits_off, even_neighbours_at_a_corner, holes,
                                 plateau_of_two_cells, tops_on_the_border, maximum_below_top_min_height, owner_tie, owner_label_0,
                                 height_equal_to_the_cutoff, percentiles_0_and_100, negative_heights, rows_above_the_last_layer,
                                 rows_over_missing_ground)}
