"""Geometric point features: the full eigen-feature set of the radius neighbourhood.

    python -m treelearn_amd.util.features --forest cloud.npy --out features.npz --features linearity planarity verticality [--radius 0.6] [--voxel-size 0.1]
    python -m treelearn_amd.util.features --forest cloud.npy --out features.npz --features linearity planarity --radii 0.2 0.4 0.6

With --radii (1 to 4 ascending radii) the file holds features f32 [M, S, F] of all radii, from one cell sort and one launch of
tl_eigen_features_scales (util.prepare.compute_features_scales), and `radii` beside `feature_names` and `points`.

The reference's `compute_features(points, search_radius, feature_names=[...])` (tree_learn/util/data_preparation.py:82-88) forwards any
list of jakteristics feature names; `util.prepare.compute_features` does the same through `tl_eigen_features` (csrc/tl_features.hip).
With l1 >= l2 >= l3 the eigenvalues of the sample covariance (n - 1) of all points within the radius (inclusive, the point itself
included), e1, e2, e3 their unit eigenvectors and s = l1 + l2 + l3:

    eigenvalue_sum s            omnivariance cbrt(l1 l2 l3)     eigenentropy -sum l ln l
    anisotropy (l1 - l3) / l1   planarity (l2 - l3) / l1        linearity (l1 - l2) / l1
    PCA1 l1 / s                 PCA2 l2 / s                     surface_variation l3 / s
    sphericity l3 / l1          verticality 1 - |e3z|           nx ny nz = e3
    number_of_neighbors         eigenvalue1..3 = l1 l2 l3       eigenvector1x .. eigenvector3z = e1, e2, e3

jakteristics is not installed here, so parity with it is unpinned; these are the project's deliberate deviations from it:
  - eigenvalues are clamped at 0 (a covariance that is singular up to rounding gives a tiny negative one otherwise);
  - 0 ln 0 = 0 in the eigenentropy (not NaN);
  - every eigenvector is oriented by z >= 0; when z == 0 by y >= 0; when that is 0 too by x >= 0 (jakteristics keeps its solver's sign);
  - fewer than 3 neighbours give NaN in every column except number_of_neighbors (jakteristics diagonalises a rank-deficient
    covariance there); ratios with a zero denominator are NaN.  `compute_features` replaces the NaNs of a column by the mean of its
    finite values, like the reference's replace_nanfeatures.
"""
import argparse
import os
import sys

import numpy as np

FEATURE_NAMES = ("eigenvalue_sum", "omnivariance", "eigenentropy", "anisotropy", "planarity", "linearity", "PCA1", "PCA2",
                 "surface_variation", "sphericity", "verticality", "nx", "ny", "nz", "number_of_neighbors",
                 "eigenvalue1", "eigenvalue2", "eigenvalue3",
                 "eigenvector1x", "eigenvector1y", "eigenvector1z", "eigenvector2x", "eigenvector2y", "eigenvector2z",
                 "eigenvector3x", "eigenvector3y", "eigenvector3z")        # position = the id tl_eigen_features takes
DEFAULT_FEATURE_NAMES = ("verticality",)
MAX_MODEL_FEATS = 5                                                          # tl_voxel_feats takes F <= 5


def check_feature_names(feature_names, for_model=False):
    """The list of names as a list of str, or ValueError: a name that is not one of FEATURE_NAMES, a duplicate, an empty list.
    `for_model`: the rules of a list that feeds the pipeline -- `verticality` is there and is last (grouping reads input_feats[:, -1],
    as the reference does), and at most MAX_MODEL_FEATS names."""
    if isinstance(feature_names, str):
        raise ValueError(f"feature_names must be a list of names, got the string {feature_names!r}")
    names = [str(n) for n in feature_names]
    if not names:
        raise ValueError("feature_names is empty")
    unknown = [n for n in names if n not in FEATURE_NAMES]
    if unknown:
        raise ValueError(f"unknown feature name(s) {unknown}; expected any of {list(FEATURE_NAMES)}")
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"duplicate feature name(s) {dup}")
    if for_model:
        if names[-1] != "verticality":
            raise ValueError(f"feature_names must end with 'verticality' (grouping reads the last feature column), got {names}")
        if len(names) > MAX_MODEL_FEATS:
            raise ValueError(f"at most {MAX_MODEL_FEATS} features can feed the model, got {len(names)}: {names}")
    return names


def feature_ids(feature_names):
    return [FEATURE_NAMES.index(n) for n in check_feature_names(feature_names)]


MAX_SCALES = 4                                                                         # TL_FEAT_MAX_SCALES


def check_radii(radii):
    """1 .. MAX_SCALES finite radii > 0 in strictly ascending order as a list of float, or ValueError.  Touches no GPU."""
    if isinstance(radii, (str, bytes)) or not hasattr(radii, "__iter__"):
        raise ValueError(f"radii must be a sequence of numbers, got {radii!r}")
    vals = list(radii)
    if not 1 <= len(vals) <= MAX_SCALES:
        raise ValueError(f"radii must hold 1 to {MAX_SCALES} values, got {len(vals)}")
    for v in vals:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not v > 0:
            raise ValueError(f"every radius must be a finite number > 0, got {v!r}")
    vals = [float(v) for v in vals]
    if any(b <= a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"radii must be strictly ascending, got {vals}")
    return vals


# ------------------------------------------------------------------------------------------------ the cache file features/<plot>.npz
def save_feature_cache(path, feats, feature_names):
    """With the default list the file holds `features` only (the bytes it always had); with another list also `feature_names`."""
    names = check_feature_names(feature_names)
    if names == list(DEFAULT_FEATURE_NAMES):
        np.savez_compressed(path, features=feats)
    else:
        np.savez_compressed(path, features=feats, feature_names=np.array(names))


def load_feature_cache(path, feature_names):
    """`features` of a cache file written for `feature_names`; ValueError when it was written for another list (a file without names
    counts as ["verticality"])."""
    names = check_feature_names(feature_names)
    with np.load(path) as f:
        have = [str(n) for n in f["feature_names"]] if "feature_names" in f.files else list(DEFAULT_FEATURE_NAMES)
        feats = f["features"]
    if have != names:
        raise ValueError(f"{path} holds the features {have}, the configuration asks for {names}: remove the file or change feature_names")
    return feats


# ------------------------------------------------------------------------------------------------ command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.features", description="geometric features of every point of a cloud")
    ap.add_argument("--forest", required=True, help="input cloud: .npy / .npz / .txt / .las, N x 3 or N x 4")
    ap.add_argument("--out", required=True, help="output .npz: features f32 [M, F], feature_names, points f64 [M, 3]")
    ap.add_argument("--features", nargs="+", required=True, help="any of: " + " ".join(FEATURE_NAMES))
    rad = ap.add_mutually_exclusive_group()
    rad.add_argument("--radius", type=float, default=0.6, help="search radius in metres")
    rad.add_argument("--radii", type=float, nargs="+", default=None, metavar="R",
                     help="1 to 4 ascending search radii: features [M, S, F] of all of them from one launch, and `radii` in the output")
    ap.add_argument("--voxel-size", type=float, default=0.1, help="down-sample to this voxel size first; 0 takes the cloud as it is")
    a = ap.parse_args(argv)
    try:
        a.features = check_feature_names(a.features)
        if a.radii is not None:
            a.radii = check_radii(a.radii)
    except ValueError as e:
        ap.error(str(e))
    if not a.radius > 0:
        ap.error("--radius must be > 0")
    if not a.voxel_size >= 0:
        ap.error("--voxel-size must be >= 0")
    if not a.out.endswith(".npz"):
        ap.error("--out must end with .npz")
    if not os.path.exists(a.forest):
        ap.error(f"--forest {a.forest}: no such file")
    return a


def main(argv=None):
    a = parse_args(argv)
    from .prepare import compute_features, compute_features_scales, voxelize
    from .segment import load_forest
    pts = np.ascontiguousarray(load_forest(a.forest)[:, :3], dtype=np.float64)
    if a.voxel_size > 0:
        vox, _ = voxelize(pts, a.voxel_size)
        pts = vox[:, :3].cpu().numpy().astype(np.float64)
    if a.radii is not None:
        feats = compute_features_scales(pts, a.radii, a.features)
        np.savez_compressed(a.out, features=feats.cpu().numpy(), radii=np.array(a.radii, np.float64), feature_names=np.array(a.features), points=pts)
        print(f"{len(pts)} points x {len(a.radii)} radii x {len(a.features)} features -> {a.out}")
        return 0
    feats = compute_features(pts, search_radius=a.radius, feature_names=a.features)
    np.savez_compressed(a.out, features=feats.cpu().numpy(), feature_names=np.array(a.features), points=pts)
    print(f"{len(pts)} points x {len(a.features)} features -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
