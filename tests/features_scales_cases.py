"""Hand-made cases for the multi-scale geometric features: the smallest clouds at which k_eigen_features_scales can go wrong.

A case is dict(points f64 [N, 3], radii (1..4 ascending), check): `check(f)` takes the RAW feature array f [N, S, 27] (columns in the order
of features_restatement.NAMES, NaN where the definition says NaN, rows in the input's order) of any implementation and asserts answers
that need no implementation.  Every scale of every case is also compared with features_restatement.restate at that radius
(features_cases.compare), and on the device with tl_eigen_features on the same sorted arrays, bit for bit."""
import numpy as np

import features_cases as one
from features_restatement import COL, NAMES

NN = COL["number_of_neighbors"]


def _counts(f):
    return np.asarray(f, np.float64)[:, :, NN]


def _nan_rows(f):
    """bool [N, S]: every column but number_of_neighbors is NaN."""
    return np.isnan(np.delete(np.asarray(f, np.float64), NN, axis=2)).all(2)


def _finite_rows(f):
    return ~np.isnan(np.asarray(f, np.float64)).any(2)


def _pairs(points):
    d = points[:, None, :] - points[None, :, :]
    return np.sqrt((d * d).sum(2))


def _by_distance(points, radii):
    """Neighbour counts [N, S] by brute force; asserts that no distance is within 1e-6 of a radius."""
    d = _pairs(points)
    for r in radii:
        assert np.abs(d - r).min() > 1e-6
    return np.stack([(d <= r).sum(1) for r in radii], 1).astype(np.float64)


# ------------------------------------------------------------------------------------------------ neighbours between two radii
def between_radii():
    """Point 0's only neighbours (but itself) lie between r1 = 0.2 and r2 = 0.5: scale 1 is a NaN row with count 1, scale 2 is finite.
    The four others sit within 0.2 of each other."""
    pts = np.array([[0.0, 0.0, 0.0], [0.30, 0.05, 0.02], [0.33, -0.02, 0.06], [0.28, 0.06, -0.04], [0.34, 0.03, 0.04]]) + np.array([-3.0, 4.0, 1.0])
    radii = (0.2, 0.5)

    def check(f):
        want = _by_distance(pts, radii)
        assert want[0].tolist() == [1.0, 5.0] and (want[1:, 0] == 4.0).all() and (want[:, 1] == 5.0).all()
        assert np.array_equal(_counts(f), want)
        assert _nan_rows(f)[0, 0] and _finite_rows(f)[0, 1] and _finite_rows(f)[1:].all()
    return dict(points=pts, radii=radii, check=check)


def two_and_three():
    """Three points on a bent line: at r1 the ends have exactly 2 neighbours (NaN) and the middle exactly 3 (finite); at r2 all have 3;
    at r0 = 0.05 every point is alone."""
    pts = np.array([[0.0, 0.0, 0.0], [0.2, 0.02, 0.0], [0.4, 0.0, 0.03]]) + np.array([7.0, -7.0, 0.0])
    radii = (0.05, 0.25, 0.45)

    def check(f):
        assert np.array_equal(_counts(f), np.array([[1, 2, 3], [1, 3, 3], [1, 2, 3]], np.float64))
        assert np.array_equal(_counts(f), _by_distance(pts, radii))
        assert np.array_equal(_nan_rows(f), np.array([[True, True, False], [True, False, False], [True, True, False]]))
        f = np.asarray(f, np.float64)
        assert np.abs(f[:, 2, COL["sphericity"]]).max() <= one.EPS            # three points span a plane: l3 = 0
    return dict(points=pts, radii=radii, check=check)


def one_ulp_apart():
    """Two radii one ulp apart with a pair of points at exactly the larger one: d^2 = r2^2 in f64 (a distance along one axis, so d^2
    is the one product), so the pair counts at scale 2 and not at scale 1."""
    r2 = 0.25                                                              # a power of two: r2 * r2 is exact, and so is the coordinate difference
    r1 = np.nextafter(r2, 0.0)
    pts = np.array([[1.0, 1.0, 1.0], [1.0 + r2, 1.0, 1.0], [1.0, 1.0 + r2, 1.0], [1.0, 1.0, 1.0 - r2]])
    assert (pts[1, 0] - pts[0, 0]) ** 2 == r2 * r2 and r1 * r1 < r2 * r2

    def check(f):
        assert np.array_equal(_counts(f), np.array([[1, 4], [1, 2], [1, 2], [1, 2]], np.float64))
        assert _nan_rows(f)[:, 0].all() and _finite_rows(f)[0, 1] and _nan_rows(f)[1:, 1].all()
    return dict(points=pts, radii=(float(r1), r2), check=check, on_the_radius=True)


# ------------------------------------------------------------------------------------------------ piece lengths
def column(n, radii=(0.15, 0.3), seed=5):
    """n random points in one (x, y) column of cells, a thin vertical stick: pieces of 64 and a tail."""
    rng = np.random.default_rng(seed + n)
    pts = np.column_stack([rng.uniform(0.0, 0.1, n), rng.uniform(0.0, 0.1, n), rng.uniform(0.0, 0.012 * n, n)]) + np.array([2.0, -1.0, 0.5])

    def check(f):
        assert np.asarray(f).shape == (n, len(radii), len(NAMES))
        c = _counts(f)
        assert (np.diff(c, axis=1) >= 0).all() and (c[:, 0] >= 1).all() and c[:, -1].max() > c[:, 0].max()
    return dict(points=pts, radii=radii, check=check)


def single_column_of_cells():
    """A cloud whose every point lies in one (x, y) column of cells of the largest radius, four scales."""
    c = column(200, radii=(0.1, 0.2, 0.3, 0.4), seed=9)
    assert np.ptp(c["points"][:, 0]) < 0.4 and np.ptp(c["points"][:, 1]) < 0.4
    return c


def blob(n):
    """features_cases.blob at radii (0.25, 0.5): ranges longer than two chunks of 128 candidates."""
    pts = one.blob(n)["points"]
    radii = (0.25, 0.5)

    def check(f):
        c = _counts(f)
        assert _finite_rows(f).all() and c[:, 1].min() > 150 and (c[:, 0] < c[:, 1]).all() and c[:, 0].min() >= 3
    return dict(points=pts, radii=radii, check=check)


def negative_on_boundaries():
    """features_cases.on_cell_boundaries with the cells of the largest radius 0.6: negative coordinates, points on cell faces and a corner."""
    pts = one.on_cell_boundaries(radius=0.6)["points"]
    radii = (0.3, 0.45, 0.6)

    def check(f):
        c = _counts(f)
        assert (c >= 1).all() and (np.diff(c, axis=1) >= 0).all()
    return dict(points=pts, radii=radii, check=check)


def plane_scales(S):
    """The 30 degree plane of features_cases at S radii: the same normal at every scale."""
    p = one.plane(30)
    radii = (0.25, 0.35, 0.45, 0.65)[4 - S:]

    def check(f):
        for k in range(S):
            p["check"](np.asarray(f)[:, k, :])
    return dict(points=p["points"], radii=radii, check=check)


CASES = {
    "between_radii": between_radii, "two_and_three": two_and_three, "one_ulp_apart": one_ulp_apart,
    "column_63": lambda: column(63), "column_64": lambda: column(64), "column_65": lambda: column(65), "column_129": lambda: column(129),
    "single_column_of_cells": single_column_of_cells,
    "blob_3000": lambda: blob(3000), "blob_3008": lambda: blob(3008),
    "negative_on_boundaries": negative_on_boundaries,
    "plane_S1": lambda: plane_scales(1), "plane_S2": lambda: plane_scales(2), "plane_S3": lambda: plane_scales(3), "plane_S4": lambda: plane_scales(4),
}


def restate_scales(points, radii):
    """features_restatement.restate per radius -> list of its dicts (features f64 [N, 27], margin, ...)."""
    import features_restatement as ref
    return [ref.restate(points, r) for r in radii]


def compare_scales(got, refs, min_inside=0.0, on_the_radius=False):
    """got [N, S, 27] against restate_scales: features_cases.compare per scale, after the restatement's own radius margin.  A case that
    puts a pair ON a radius on purpose has no such margin: the restatement's kd-tree does not promise the device's expression there, so
    that case rests on its hand-derived check and on the exact comparison with tl_eigen_features alone."""
    got = np.asarray(got)
    assert got.shape[1] == len(refs)
    if on_the_radius:
        return
    for k, r in enumerate(refs):
        assert r["margin"] > 1e-10, (k, r["margin"])
        one.compare(got[:, k, :], r, min_inside=min_inside)
