"""Hand-derived cases for the geometric point features and the one comparison both test files use.

A case is dict(points f64 [N, 3], radius, check): `check(f)` takes the RAW feature matrix f [N, 27] (columns in the order of
features_restatement.NAMES, NaN where the definition says NaN) of any implementation and asserts answers that need no implementation.
Radius 0.65 wherever points sit on a 0.1 or 0.2 m lattice: no lattice distance is within 1e-3 of it.

compare(got, ref, ...) holds the tolerances of the comparison against the restatement."""
import numpy as np

from features_restatement import COL, EIGENVALUE_SCALED, NAMES, RATIOS

R_LATTICE = 0.65
EPS = 2.0 ** -21           # eigenvalue features: the two f64 solvers differ by O(2^-50) of the trace, the rest is the f32 rounding of the output
VEC_TOL = 1e-5             # eigenvector components and verticality (the bound of the existing verticality test)
GAP = 1e-5                 # an eigenvector is compared where its eigenvalue is this far (relative to l1) from its neighbours


def _col(f, name):
    return np.asarray(f, np.float64)[:, COL[name]]


def _vec(f, k):
    a = COL[f"eigenvector{k}x"]
    return np.asarray(f, np.float64)[:, a:a + 3]


def _oriented(d):
    d = np.asarray(d, np.float64) / np.linalg.norm(d)
    x, y, z = d
    return -d if (z < 0 or (z == 0 and (y < 0 or (y == 0 and x < 0)))) else d


def _assert_dir(got, want, what):
    """Rows of got [N, 3] equal the unit vector `want`; up to the sign of the whole vector where |want_z| < 1e-3 (the orientation rule then
    rests on rounding)."""
    err = np.abs(got - want).max(1)
    if abs(want[2]) < 1e-3:
        err = np.minimum(err, np.abs(got + want).max(1))
    assert err.max() < VEC_TOL, (what, float(err.max()))


# ------------------------------------------------------------------------------------------------ planes
def plane(theta_deg, half=8, spacing=0.1):
    """A (2 half + 1)^2 lattice in the plane through the origin whose normal is theta off the vertical (rotated about the y axis)."""
    t = np.deg2rad(theta_deg)
    u, v = np.meshgrid(np.arange(-half, half + 1) * spacing, np.arange(-half, half + 1) * spacing, indexing="ij")
    u, v = u.ravel(), v.ravel()
    pts = np.column_stack([u * np.cos(t), v, -u * np.sin(t)]) + np.array([3.0, -2.0, 1.5])
    normal = np.array([np.sin(t), 0.0, np.cos(t)])

    def check(f):
        assert not np.isnan(f).any()
        _assert_dir(np.asarray(f, np.float64)[:, COL["nx"]:COL["nz"] + 1], normal, f"normal of the {theta_deg} deg plane")
        _assert_dir(_vec(f, 3), normal, f"e3 of the {theta_deg} deg plane")
        assert np.abs(_col(f, "verticality") - (1.0 - np.cos(t))).max() < VEC_TOL
        assert np.abs(_col(f, "sphericity")).max() <= EPS and np.abs(_col(f, "surface_variation")).max() <= EPS
        assert np.abs(_col(f, "anisotropy") - 1.0).max() <= EPS
        assert np.abs(_col(f, "planarity") - _col(f, "eigenvalue2") / _col(f, "eigenvalue1")).max() <= EPS
        l1 = _col(f, "eigenvalue1")
        om = _col(f, "omnivariance")
        assert (om >= 0).all() and (om <= 1.01e-2 * l1).all()
    return dict(points=pts, radius=R_LATTICE, check=check)


# ------------------------------------------------------------------------------------------------ a straight line
def line(direction, n=20, spacing=0.1):
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    pts = np.arange(n)[:, None] * spacing * d[None, :] + np.array([-1.0, 0.5, 2.0])
    want = _oriented(d)

    def check(f):
        assert not np.isnan(f).any()
        assert np.abs(_col(f, "linearity") - 1.0).max() <= EPS and np.abs(_col(f, "PCA1") - 1.0).max() <= EPS
        _assert_dir(_vec(f, 1), want, f"e1 of the line along {direction}")
    return dict(points=pts, radius=R_LATTICE, check=check)


# ------------------------------------------------------------------------------------------------ the centre of a cubic lattice
def lattice_centre():
    g = np.arange(-3, 4) * 0.2
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    pts = np.column_stack([x.ravel(), y.ravel(), z.ravel()]) + np.array([10.0, 10.0, 10.0])
    centre = int(np.flatnonzero((np.abs(pts - 10.0) < 1e-9).all(1))[0])

    def check(f):
        c = np.asarray(f, np.float64)[centre]
        assert abs(c[COL["linearity"]]) <= EPS and abs(c[COL["planarity"]]) <= EPS
        assert abs(c[COL["sphericity"]] - 1.0) <= EPS and abs(c[COL["PCA1"]] - 1.0 / 3.0) <= EPS
        # the ball of radius 0.65 on a 0.2 m lattice: offsets with i^2 + j^2 + k^2 <= 10
        i = np.arange(-3, 4)
        assert c[COL["number_of_neighbors"]] == ((i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2) <= 10).sum()
    return dict(points=pts, radius=R_LATTICE, check=check)


# ------------------------------------------------------------------------------------------------ fewer than three neighbours
def pair_and_single():
    pts = np.array([[40.0, 40.0, 3.0], [40.2, 40.0, 3.0], [-50.0, 7.0, 1.0]])

    def check(f):
        f = np.asarray(f, np.float64)
        assert f[:, COL["number_of_neighbors"]].tolist() == [2.0, 2.0, 1.0]
        assert np.isnan(np.delete(f, COL["number_of_neighbors"], axis=1)).all()
    return dict(points=pts, radius=R_LATTICE, check=check)


def plane_with_strays():
    """The flat plane plus the pair and the single point: the rows the column-mean replacement fills."""
    p = plane(0)["points"]
    pts = np.vstack([p, pair_and_single()["points"]])

    def check(f):
        f = np.asarray(f, np.float64)
        assert np.isnan(np.delete(f[-3:], COL["number_of_neighbors"], axis=1)).all() and not np.isnan(f[:-3]).any()
        assert f[-3:, COL["number_of_neighbors"]].tolist() == [2.0, 2.0, 1.0]
        assert np.abs(f[:-3, COL["verticality"]]).max() < VEC_TOL
    return dict(points=pts, radius=R_LATTICE, check=check)


# ------------------------------------------------------------------------------------------------ small clouds
def single_point():
    def check(f):
        f = np.asarray(f, np.float64)
        assert f.shape == (1, len(NAMES)) and f[0, COL["number_of_neighbors"]] == 1.0
        assert np.isnan(np.delete(f, COL["number_of_neighbors"], axis=1)).all()
    return dict(points=np.array([[1.0, -2.0, 3.0]]), radius=0.6, check=check)


def two_points():
    def check(f):
        f = np.asarray(f, np.float64)
        assert f[:, COL["number_of_neighbors"]].tolist() == [2.0, 2.0]
        assert np.isnan(np.delete(f, COL["number_of_neighbors"], axis=1)).all()
    return dict(points=np.array([[0.0, 0.0, 0.0], [0.3, 0.1, -0.2]]), radius=0.6, check=check)


def within_one_cell():
    """Five points inside a 0.2 m box: a cloud smaller than one cell, every point a neighbour of every other."""
    pts = np.array([[0.00, 0.00, 0.00], [0.20, 0.05, 0.10], [0.10, 0.20, 0.05], [0.05, 0.10, 0.20], [0.15, 0.15, 0.15]]) + np.array([-7.0, 2.0, 0.5])

    def check(f):
        f = np.asarray(f, np.float64)
        assert (f[:, COL["number_of_neighbors"]] == 5.0).all() and not np.isnan(f).any()
        for c in (c for c in range(f.shape[1]) if c != COL["verticality"] and NAMES[c] not in ("nx", "ny", "nz") and not NAMES[c].startswith("eigenvector")):
            assert np.ptp(f[:, c]) <= EPS * max(1.0, np.abs(f[:, c]).max()), NAMES[c]        # one neighbourhood: one covariance
    return dict(points=pts, radius=0.6, check=check)


def on_cell_boundaries(radius=0.6, n=400, seed=3):
    """Negative coordinates, and points exactly on the boundaries of the radius-sized cells (the grid starts at min - radius)."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-2.0, 1.0, size=(n, 3))
    lo = pts.min()
    k = 0
    for axis in range(3):
        for step in (1, 2, 3, 4):
            pts[10 + k, axis] = lo + step * radius                  # (lo stays the minimum: step >= 1)
            k += 1
    pts[40] = lo + np.array([1, 2, 3]) * radius                       # a cell corner
    assert pts.min() == lo

    def check(f):
        f = np.asarray(f, np.float64)
        assert f.shape == (n, len(NAMES)) and (f[:, COL["number_of_neighbors"]] >= 1).all()
    return dict(points=pts, radius=radius, check=check)


def blob(n, seed=11, radius=0.6):
    """Random points in a 1.0 m cube: several hundred points per cell (more than one 64-point piece) and neighbour ranges far longer than
    any chunk."""
    pts = np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 3)) + np.array([-0.3, 5.0, 2.0])

    def check(f):
        f = np.asarray(f, np.float64)
        assert not np.isnan(f).any() and f[:, COL["number_of_neighbors"]].min() > 200
    return dict(points=pts, radius=radius, check=check)


CASES = {
    "plane_0": lambda: plane(0), "plane_30": lambda: plane(30), "plane_75": lambda: plane(75),
    "line_x": lambda: line([1, 0, 0]), "line_y_neg": lambda: line([0, -1, 0]), "line_skew": lambda: line([1, 2, -2]),
    "line_diag": lambda: line([1, -1, 0]), "line_z": lambda: line([0, 0, 1]),
    "lattice_centre": lattice_centre,
    "pair_and_single": pair_and_single, "plane_with_strays": plane_with_strays,
    "single_point": single_point, "two_points": two_points, "within_one_cell": within_one_cell,
    "on_cell_boundaries": on_cell_boundaries,
    "blob_3008": lambda: blob(3008), "blob_3000": lambda: blob(3000),           # a multiple of 64, and not
}


# ------------------------------------------------------------------------------------------------ against the restatement
def compare(got, ref, min_inside=1.0, report=None):
    """got: RAW features [N, 27] of the implementation under test; ref: features_restatement.restate of the same cloud.
    number_of_neighbors and the NaN pattern: equal.  Eigenvalue features: |delta| <= 2^-21 x scale, scale 1 for the ratios, s for
    eigenvalue_sum / eigenvalue1..3 / omnivariance, max(1, |value|) for eigenentropy; where g3 < 1e-6, omnivariance is checked as
    0 <= value <= 1.01e-2 l1.  Eigenvector components and verticality: 1e-5 absolute -- e3 (and nx ny nz, verticality) where gap23 > 1e-5,
    e1 where gap12 > 1e-5, e2 where both; up to the sign of the whole vector where the restatement's |z| < 1e-3.
    min_inside: the fraction of the >= 3-neighbour rows that must meet the gap conditions, per column group."""
    got = np.asarray(got, np.float64)
    want = ref["features"]
    assert got.shape == want.shape
    assert np.array_equal(got[:, COL["number_of_neighbors"]], want[:, COL["number_of_neighbors"]])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want[:, COL["eigenvalue1"]])
    if not ok.any():
        return
    g, w = got[ok], want[ok]
    s, l1, g3, gap23, gap12 = (ref[k][ok] for k in ("s", "l1", "g3", "gap23", "gap12"))
    figures = {}

    def bound(name, delta, scale, rows=None):
        rows = np.ones(len(delta), bool) if rows is None else rows
        if rows.any():
            worst = float((np.abs(delta[rows]) / scale[rows] if np.ndim(scale) else np.abs(delta[rows]) / scale).max())
            figures[name] = worst
            return worst
        return 0.0

    one = np.ones(len(g))
    fails = []
    for n in RATIOS:
        finite = ~np.isnan(w[:, COL[n]])                              # (a zero denominator: NaN on both sides, checked above)
        if bound(n, g[:, COL[n]] - w[:, COL[n]], one, finite) > EPS:
            fails.append(n)
    for n in EIGENVALUE_SCALED:
        rows = g3 >= 1e-6 if n == "omnivariance" else None
        if bound(n, g[:, COL[n]] - w[:, COL[n]], s, rows) > EPS:
            fails.append(n)
    flat = g3 < 1e-6
    if flat.any():
        om = g[flat, COL["omnivariance"]]
        if not ((om >= 0).all() and (om <= 1.01e-2 * l1[flat]).all()):
            fails.append("omnivariance (flat)")
    ee = COL["eigenentropy"]
    if bound("eigenentropy", g[:, ee] - w[:, ee], np.maximum(1.0, np.abs(w[:, ee]))) > EPS:
        fails.append("eigenentropy")

    def vec_err(a, b):
        err = np.abs(a - b).max(1)
        either = np.abs(b[:, 2]) < 1e-3
        err[either] = np.minimum(err[either], np.abs(a[either] + b[either]).max(1))
        return err

    in3, in1 = gap23 > GAP, gap12 > GAP
    for name, rows in (("e3", in3), ("e1", in1), ("e2", in3 & in1)):
        assert rows.mean() >= min_inside, (name, float(rows.mean()))
        if not rows.any():
            continue
        a = COL[f"eigenvector{name[1]}x"]
        figures[name] = float(vec_err(g[rows, a:a + 3], w[rows, a:a + 3]).max())
        if figures[name] > VEC_TOL:
            fails.append(name)
    if in3.any():
        a = COL["nx"]
        figures["normal"] = float(vec_err(g[in3, a:a + 3], w[in3, a:a + 3]).max())
        figures["verticality"] = float(np.abs(g[in3, COL["verticality"]] - w[in3, COL["verticality"]]).max())
        fails += [k for k in ("normal", "verticality") if figures[k] > VEC_TOL]
    if report is not None:
        report(figures)
    assert not fails, (fails, figures)
