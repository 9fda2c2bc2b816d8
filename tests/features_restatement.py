"""A numpy float64 yardstick for the geometric point features that imports nothing from the package:
scipy's cKDTree.query_ball_point for the neighbourhoods, a two-pass covariance about the neighbourhood's mean, np.linalg.eigh, and then
the definitions of the feature table, written out once more.

restate(points, radius) -> dict:
    features  f64 [N, 27]  columns in the order of NAMES, NaN where the definition says NaN (nothing replaced)
    g3, gap23, gap12  f64 [N]  l3 / l1, (l2 - l3) / l1, (l1 - l2) / l1  (NaN with fewer than 3 neighbours): how well the eigenvalues and
                               eigenvectors of a point are conditioned
    l1, s     f64 [N]      the scales the tolerances refer to
    margin    float        min | |d| - r | / r over all pairs with |d| < 1.02 r: how far the cloud is from a neighbour set that depends
                           on the last bit of a distance
replace_nan(features) -> f32 [N, F]: NaNs of a column replaced by the mean of its finite values (f64 sum / count, cast to f32)."""
import numpy as np
from scipy.spatial import cKDTree

NAMES = ("eigenvalue_sum", "omnivariance", "eigenentropy", "anisotropy", "planarity", "linearity", "PCA1", "PCA2",
         "surface_variation", "sphericity", "verticality", "nx", "ny", "nz", "number_of_neighbors",
         "eigenvalue1", "eigenvalue2", "eigenvalue3",
         "eigenvector1x", "eigenvector1y", "eigenvector1z", "eigenvector2x", "eigenvector2y", "eigenvector2z",
         "eigenvector3x", "eigenvector3y", "eigenvector3z")
COL = {n: i for i, n in enumerate(NAMES)}
EIGENVALUE_SCALED = ("eigenvalue_sum", "omnivariance", "eigenvalue1", "eigenvalue2", "eigenvalue3")     # compared relative to s
RATIOS = ("anisotropy", "planarity", "linearity", "PCA1", "PCA2", "surface_variation", "sphericity")


def orient(v):
    """[N, 3] unit vectors -> the same lines with z >= 0; z == 0: y >= 0; that 0 too: x >= 0."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    flip = (z < 0) | ((z == 0) & ((y < 0) | ((y == 0) & (x < 0))))
    return np.where(flip[:, None], -v, v)


def _covariances(points, radius, block=2048):
    """Neighbour counts i64 [N] and sample covariances f64 [N, 3, 3] (NaN rows with fewer than 2 neighbours)."""
    n = len(points)
    tree = cKDTree(points)
    cnt = np.zeros(n, np.int64)
    cov = np.full((n, 3, 3), np.nan)
    for a in range(0, n, block):
        e = min(n, a + block)
        lists = tree.query_ball_point(points[a:e], radius)
        c = np.array([len(l) for l in lists], np.int64)
        cnt[a:e] = c
        flat = np.concatenate([np.asarray(l, np.int64) for l in lists]) if c.sum() else np.zeros(0, np.int64)
        start = np.concatenate([[0], np.cumsum(c)[:-1]])
        nb = points[flat]
        mean = np.add.reduceat(nb, start, axis=0) / c[:, None]
        d = nb - np.repeat(mean, c, axis=0)
        outer = d[:, :, None] * d[:, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            cov[a:e] = np.add.reduceat(outer.reshape(-1, 9), start, axis=0).reshape(-1, 3, 3) / (c - 1)[:, None, None]
    return cnt, cov


def radius_margin(points, radius):
    pairs = cKDTree(points).query_pairs(1.02 * radius, output_type="ndarray")
    if len(pairs) == 0:
        return 1.0                                               # only the pairs (i, i): | 0 - r | / r
    d = np.linalg.norm(points[pairs[:, 0]] - points[pairs[:, 1]], axis=1)
    return float(min(1.0, np.abs(d - radius).min() / radius))


def restate(points, radius):
    points = np.ascontiguousarray(points, np.float64)
    n = len(points)
    cnt, cov = _covariances(points, radius)
    ok = cnt >= 3
    w = np.full((n, 3), np.nan)
    v = np.full((n, 3, 3), np.nan)
    if ok.any():
        w[ok], v[ok] = np.linalg.eigh(cov[ok])                    # ascending
    l1, l2, l3 = (np.maximum(w[:, k], 0.0) for k in (2, 1, 0))    # clamped at 0 (NaN stays NaN)
    l1, l2, l3 = (np.where(ok, l, np.nan) for l in (l1, l2, l3))
    e1, e2, e3 = (orient(v[:, :, k]) for k in (2, 1, 0))
    s = l1 + l2 + l3
    f = np.full((n, len(NAMES)), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        xlnx = lambda l: np.where(l > 0, l * np.log(np.where(l > 0, l, 1.0)), np.where(np.isnan(l), np.nan, 0.0))      # noqa: E731
        f[:, COL["eigenvalue_sum"]] = s
        f[:, COL["omnivariance"]] = np.cbrt(l1 * l2 * l3)
        f[:, COL["eigenentropy"]] = -(xlnx(l1) + xlnx(l2) + xlnx(l3))
        f[:, COL["anisotropy"]] = (l1 - l3) / l1
        f[:, COL["planarity"]] = (l2 - l3) / l1
        f[:, COL["linearity"]] = (l1 - l2) / l1
        f[:, COL["PCA1"]] = l1 / s
        f[:, COL["PCA2"]] = l2 / s
        f[:, COL["surface_variation"]] = l3 / s
        f[:, COL["sphericity"]] = l3 / l1
        g3, gap23, gap12 = l3 / l1, (l2 - l3) / l1, (l1 - l2) / l1
    f[:, COL["verticality"]] = 1.0 - np.abs(e3[:, 2])
    f[:, COL["nx"]:COL["nz"] + 1] = e3
    f[:, COL["number_of_neighbors"]] = cnt
    f[:, COL["eigenvalue1"]], f[:, COL["eigenvalue2"]], f[:, COL["eigenvalue3"]] = l1, l2, l3
    f[:, COL["eigenvector1x"]:COL["eigenvector1x"] + 3] = e1
    f[:, COL["eigenvector2x"]:COL["eigenvector2x"] + 3] = e2
    f[:, COL["eigenvector3x"]:COL["eigenvector3x"] + 3] = e3
    return dict(features=f, g3=g3, gap23=gap23, gap12=gap12, l1=l1, s=s, margin=radius_margin(points, radius))


def replace_nan(features):
    f = np.asarray(features)
    out = f.astype(np.float32)
    for c in range(f.shape[1]):
        col = out[:, c]
        bad = np.isnan(col)
        if bad.any():
            col[bad] = np.float32(col[~bad].astype(np.float64).sum() / (~bad).sum()) if (~bad).any() else np.float32("nan")
    return out
