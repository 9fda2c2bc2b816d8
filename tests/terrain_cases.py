"""Terrain cases worked by hand, shared by tests/test_host_terrain.py (the numpy restatement) and tests/test_gpu_terrain.py
(the kernels).  CASES: name -> function returning (xyz f64[N, 3], labels i64[N] or None, params, check); check(t, sample) asserts the
hand values on t (a dict: ix0, iy0, nx, ny, z, state, n_candidates as numpy arrays / ints) and on sample(xy f64[M, 2]) -> f64[M]."""
import numpy as np

NAN = float("nan")


def _centres(nx, ny, c=0.5):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    return (i.reshape(-1) + 0.5) * c, (j.reshape(-1) + 0.5) * c


def _shape(t, ix0, iy0, nx, ny):
    assert (t["ix0"], t["iy0"], t["nx"], t["ny"]) == (ix0, iy0, nx, ny), (t["ix0"], t["iy0"], t["nx"], t["ny"])
    assert t["z"].shape == t["state"].shape == t["n_candidates"].shape == (ny, nx)
    assert t["z"].dtype == np.float64 and t["state"].dtype == np.uint8 and t["n_candidates"].dtype == np.int32


def plane():
    """z = 0.1 x + 0.05 y, one candidate at every cell centre of an 8 x 8 grid of 0.5 m cells.  The slope is far below max_slope: every
    cell is ground and equals the plane at its centre (the candidate's own z).  Bilinear interpolation reproduces a plane between the
    centres; in the outer half cell both corners clamp to the border cell, so the sample is the plane at the border centre."""
    x, y = _centres(8, 8)
    f = lambda x, y: 0.1 * x + 0.05 * y                                # noqa: E731
    xyz = np.column_stack([x, y, f(x, y)])

    def check(t, sample):
        _shape(t, 0, 0, 8, 8)
        assert (t["state"] == 1).all() and (t["n_candidates"] == 1).all()
        assert np.array_equal(t["z"], f(x, y).reshape(8, 8))
        rng = np.random.default_rng(0)
        q = rng.uniform(0.25, 3.75, (200, 2))
        assert np.abs(sample(q) - f(q[:, 0], q[:, 1])).max() <= 1e-12
        edge = np.array([[0.1, 1.3], [3.9, 1.3], [1.3, 0.05], [1.3, 3.99], [0.0, 0.0], [-5.0, 2.0], [9.0, 9.0]])
        want = f(np.clip(edge[:, 0], 0.25, 3.75), np.clip(edge[:, 1], 0.25, 3.75))
        assert np.abs(sample(edge) - want).max() <= 1e-12
    return xyz, None, {}, check


def _stump_cloud():
    x, y = _centres(3, 3)
    z = 0.1 * np.arange(3)[None, :].repeat(3, 0).reshape(-1)           # 0, 0.1, 0.2 by column
    z[4] = 2.0                                                         # the centre cell's only candidate
    return np.column_stack([x, y, z])


def stump():
    """3 x 3 cells, z = 0, 0.1, 0.2 by column, the centre's only candidate 2 m up: 2.0 - 0.0 > 1.0 * 0.5 + 0.2, rejected; its neighbours
    look up at it and are kept.  Fill at rho = 1, row-major: weights 1/2, 1, 1/2, 1, 1, 1/2, 1, 1/2 (sum 6) on z = 0, .1, .2, 0, .2, 0,
    .1, .2: sum(w z) = 0.1 + 0.1 + 0.2 + 0.1 + 0.1 = 0.6, value 0.1, state 4."""
    def check(t, sample):
        _shape(t, 0, 0, 3, 3)
        want = np.ones((3, 3), np.uint8)
        want[1, 1] = 4
        assert np.array_equal(t["state"], want) and (t["n_candidates"] == 1).all()
        assert abs(t["z"][1, 1] - 0.1) <= 1e-12
        assert np.array_equal(t["z"][[0, 2]], [[0.0, 0.1, 0.2]] * 2)
        assert abs(sample(np.array([[0.75, 0.75]]))[0] - 0.1) <= 1e-12
    return _stump_cloud(), None, {}, check


def stump_window_0():
    """window = 0: no neighbour is looked at, nothing is rejected, the stump stays."""
    def check(t, sample):
        _shape(t, 0, 0, 3, 3)
        assert (t["state"] == 1).all() and t["z"][1, 1] == 2.0
    return _stump_cloud(), None, dict(window=0), check


def step_on_the_bound():
    """c = 0.5, max_slope = 1, step_tol = 0.25, neighbour at d = 0.5: the bound is 0.75 exactly.  A difference of 0.75 is kept."""
    xyz = np.array([[0.25, 0.25, 0.0], [0.75, 0.25, 0.75]])

    def check(t, sample):
        _shape(t, 0, 0, 2, 1)
        assert t["state"].tolist() == [[1, 1]] and t["z"].tolist() == [[0.0, 0.75]]
    return xyz, None, dict(cell=0.5, max_slope=1.0, step_tol=0.25, window=1), check


def step_one_ulp_over():
    """The same with the upper cell one ulp higher: rejected, then filled from its only ground neighbour (value 0.0, state 4)."""
    xyz = np.array([[0.25, 0.25, 0.0], [0.75, 0.25, np.nextafter(0.75, 1.0)]])

    def check(t, sample):
        _shape(t, 0, 0, 2, 1)
        assert t["state"].tolist() == [[1, 4]] and t["z"].tolist() == [[0.0, 0.0]]
    return xyz, None, dict(cell=0.5, max_slope=1.0, step_tol=0.25, window=1), check


def _hole_cloud():
    x, y = _centres(5, 5)
    ring = (np.abs(x - 1.25) > 0.75) | (np.abs(y - 1.25) > 0.75)      # the outer ring of the 5 x 5 grid
    x, y = x[ring], y[ring]
    return np.column_stack([x, y, 0.2 * x])


def hole_3x3():
    """5 x 5 cells, z = 0.2 x at the 16 outer centres, the inner 3 x 3 empty.  The ring of the hole fills at rho = 1, the centre at
    rho = 2, by symmetry to the plane's value there, 0.25.  The hole's corner (1, 1) sees (0,0) (1,0) (2,0) (0,1) (0,2) with weights
    .5, 1, .5, 1, .5 (sum 3.5) on z = .05, .15, .25, .05, .05: sum(w z) = .025 + .15 + .125 + .05 + .025 = 0.375."""
    def check(t, sample):
        _shape(t, 0, 0, 5, 5)
        want = np.ones((5, 5), np.uint8)
        want[1:4, 1:4] = 3
        assert np.array_equal(t["state"], want)
        n = np.ones((5, 5), np.int32)
        n[1:4, 1:4] = 0
        assert np.array_equal(t["n_candidates"], n)
        assert abs(t["z"][2, 2] - 0.25) <= 1e-12
        assert abs(t["z"][1, 1] - 0.375 / 3.5) <= 1e-12
        # (2, 1): the column i = 0 at distance 1: (0,1) (0,2) (0,3) with weights .5, 1, .5 on z = .05 -> .05
        assert abs(t["z"][2, 1] - 0.05) <= 1e-12
    return _hole_cloud(), None, {}, check


def hole_fill_radius_0():
    """fill_radius = 0: nothing is filled, the hole stays NaN in state 0."""
    def check(t, sample):
        _shape(t, 0, 0, 5, 5)
        assert (t["state"][1:4, 1:4] == 0).all() and np.isnan(t["z"][1:4, 1:4]).all() and np.isfinite(t["z"]).sum() == 16
        # a sample whose four corners include the hole falls back to its own cell: finite on the ring, NaN in the hole
        assert sample(np.array([[0.4, 0.4]]))[0] == 0.2 * 0.25 and np.isnan(sample(np.array([[1.25, 1.25]]))[0])
    return _hole_cloud(), None, dict(fill_radius=0), check


def wide_hole():
    """7 x 1 cells, candidates in cells 0 (z = 1) and 6 (z = 3), fill_radius = 1: cells 1 and 5 fill (state 3), cells 2 .. 4 stay NaN in
    state 0.  x = 0.6: corners 0 and 1, both 1.0.  x = 0.9: corners 1 and 2, one NaN: the own cell 1, 1.0.  x = 1.75: own cell 3: NaN."""
    xyz = np.array([[0.25, 0.25, 1.0], [3.25, 0.25, 3.0]])

    def check(t, sample):
        _shape(t, 0, 0, 7, 1)
        assert t["state"].tolist() == [[1, 3, 0, 0, 0, 3, 1]]
        assert np.array_equal(t["z"], [[1.0, 1.0, NAN, NAN, NAN, 3.0, 3.0]], equal_nan=True)
        assert np.array_equal(sample(np.array([[0.6, 0.25], [0.9, 0.1], [1.75, 0.3], [3.4, 7.0]])), [1.0, 1.0, NAN, 3.0], equal_nan=True)
    return xyz, None, dict(fill_radius=1), check


def borders():
    """Negative coordinates and rows exactly on cell borders (c = 0.5): x = -0.75 -> cell -2; -0.5 and -0.25 -> cell -1 (floor, not
    truncation); 0.0 -> cell 0; 1.0, the maximum, -> cell 2, the grid's last column.  y = -0.5 for all: iy0 = -1."""
    xyz = np.array([[-0.75, -0.5, 0.3], [-0.5, -0.5, 0.2], [-0.25, -0.5, 0.1], [0.0, -0.5, 0.0], [1.0, -0.5, 0.05]])

    def check(t, sample):
        _shape(t, -2, -1, 5, 1)
        assert t["n_candidates"].tolist() == [[1, 2, 1, 0, 1]]
        assert t["state"].tolist() == [[1, 1, 1, 3, 1]]
        assert t["z"][0, :3].tolist() == [0.3, 0.1, 0.0] and t["z"][0, 4] == 0.05
        assert abs(t["z"][0, 3] - 0.025) <= 1e-12                      # (0.0 + 0.05) / 2 at rho = 1
    return xyz, None, {}, check


def other_labels():
    """Tree rows (label 3) and unassigned rows (label -1) extend the grid but never feed a minimum, however low they lie."""
    xyz = np.array([[0.25, 0.25, 1.0], [0.75, 0.25, 1.1], [2.25, 0.25, -5.0], [-0.75, 0.25, -9.0], [0.3, 0.3, -7.0]])
    lab = np.array([0, 0, 3, -1, 3])

    def check(t, sample):
        _shape(t, -2, 0, 7, 1)
        assert t["n_candidates"].tolist() == [[0, 0, 1, 1, 0, 0, 0]]
        assert t["state"].tolist() == [[3, 3, 1, 1, 3, 3, 3]]
        assert t["z"][0, 2:4].tolist() == [1.0, 1.1] and t["z"].min() >= 1.0 and t["z"].max() <= 1.1
    return xyz, lab, {}, check


def no_candidates():
    """No row is labelled 0: the whole grid is NaN in state 0, and so is every sample."""
    xyz = np.array([[0.25, 0.25, 1.0], [1.75, 1.25, 2.0]])

    def check(t, sample):
        _shape(t, 0, 0, 4, 3)
        assert (t["state"] == 0).all() and (t["n_candidates"] == 0).all() and np.isnan(t["z"]).all()
        assert np.isnan(sample(np.array([[0.3, 0.3], [1.0, 1.0]]))).all()
    return xyz, np.array([1, 2]), {}, check


def one_cell():
    """A 1 x 1 grid: every sample, inside or far outside, is the cell's value."""
    xyz = np.array([[0.1, 0.2, 4.0], [0.4, 0.3, 3.5]])

    def check(t, sample):
        _shape(t, 0, 0, 1, 1)
        assert t["z"].tolist() == [[3.5]] and t["state"].tolist() == [[1]] and t["n_candidates"].tolist() == [[2]]
        assert sample(np.array([[0.25, 0.25], [0.0, 0.49], [-100.0, 50.0]])).tolist() == [3.5, 3.5, 3.5]
    return xyz, None, {}, check


CASES = dict(plane=plane, stump=stump, stump_window_0=stump_window_0, step_on_the_bound=step_on_the_bound, step_one_ulp_over=step_one_ulp_over,
             hole_3x3=hole_3x3, hole_fill_radius_0=hole_fill_radius_0, wide_hole=wide_hole, borders=borders, other_labels=other_labels,
             no_candidates=no_candidates, one_cell=one_cell)


def tree_on_flat_ground():
    """One tree (label 1) on flat ground z = 0 (label 0, every cell centre of 6 x 6 cells): a stem of 64 rows per layer on a circle of
    radius 0.15 about (1.5, 1.5), layers every 0.05 m from 0.07 to 3.02 m; the rows below 0.42 m -- the foot -- are labelled 0 and lie
    above the ground rows.  z_ground = 0 exactly, so height_ag = z_top = 3.02, base_gap = z_low = 0.42 (rank 3 of 64 tied rows) and
    the slice 1.2 <= z < 1.4 holds the layers 1.22, 1.27, 1.32, 1.37: dbh_ag = 0.30 from 256 rows, while the §16 slice about z_low +
    1.3 = 1.72 gives the same circle from rows half a metre higher."""
    gx, gy = _centres(6, 6)
    rows, lab = [np.column_stack([gx, gy, np.zeros(36)])], [np.zeros(36, np.int64)]
    a = 2 * np.pi * np.arange(64) / 64
    for k in range(1, 61):
        zl = 0.05 * k + 0.02
        rows.append(np.column_stack([1.5 + 0.15 * np.cos(a), 1.5 + 0.15 * np.sin(a), np.full(64, zl)]))
        lab.append(np.full(64, 1 if k >= 8 else 0, np.int64))
    xyz, lab = np.concatenate(rows), np.concatenate(lab)

    def check(inv):
        assert inv["n_points"].tolist() == [53 * 64]
        assert inv["z_ground"][0] == 0.0 and inv["base_gap"][0] == inv["z_low"][0] and inv["height_ag"][0] == inv["z_top"][0]
        assert abs(inv["z_low"][0] - 0.42) <= 1e-12 and abs(inv["z_top"][0] - 3.02) <= 1e-12
        assert inv["dbh_ag_n"].tolist() == [256] and abs(inv["dbh"][0] - 0.30) <= 1e-9
        assert abs(inv["dbh_ag"][0] - 0.30) <= 1e-9 and abs(inv["dbh_ag_x"][0] - 1.5) <= 1e-9 and abs(inv["dbh_ag_y"][0] - 1.5) <= 1e-9
        assert inv["dbh_ag_rmse"][0] <= 1e-9
    return xyz, lab, check
