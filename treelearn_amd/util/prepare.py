"""Plot preparation on the device -- SURVEY.md 8f #4: what `generate_tiles` does before tiling
(reference tree_learn/util/pipeline.py:24-65) and what the pipeline does after grouping to carry the
predictions back to the original cloud (util/pipeline.py:423-452).

  voxelize           <- data_preparation.py:60-79 (open3d 0.17.0 VoxelDownSampleAndTrace)
  compute_features   <- data_preparation.py:82-100 (jakteristics 0.5.1, search radius 0.6 m: verticality, or any list of its feature names)
  propagate_to_original <- util/pipeline.py:441-452 (`propagate_preds_hash_full`: hash dictionary voxel -> original indices)

open3d and jakteristics are not part of the reference tree and not installable here: their published algorithms are
restated (csrc/tl_prepare.hip, csrc/tl_features.hip) and checked against an independent numpy/scipy oracle; parity with the two libraries
themselves is unpinned.  Deliberate differences, all on quantities the path does not depend on: voxels come out in
ascending (x, y, z) order (open3d: unordered_map order), and points with fewer than three neighbours inside the search
radius get NaN -> column mean (jakteristics diagonalises a rank-deficient covariance there)."""
import ctypes

import numpy as np
import torch

from .. import _hip

_I64x3 = ctypes.c_int64 * 3
_I64x2 = ctypes.c_int64 * 2


def _dev_f64(a):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device="cuda", dtype=torch.float64).contiguous()


def _keys(xyz, cell, origin, round_input):
    """Packed cell keys (device i64[n]) of f64 points relative to `origin` (host float), plus the largest cell index per axis."""
    L = _hip.lib()
    n = len(xyz)
    src = torch.round(xyz * 100.0) / 100.0 if round_input else xyz
    base = [int(np.floor((float(v) - origin) / cell)) for v in src.amin(0).cpu()]
    top = [int(np.floor((float(v) - origin) / cell)) for v in src.amax(0).cpu()]
    keys = torch.empty(n, dtype=torch.int64, device=xyz.device); err = torch.empty(1, dtype=torch.int32, device=xyz.device)
    _hip.check(L.tl_cell_keys(_hip.ptr(xyz), n, float(cell), float(origin), _I64x3(*base), int(round_input), _hip.ptr(keys), _hip.ptr(err), _hip.stream()),
               "tl_cell_keys")
    if int(err.item()):
        raise ValueError("plot extent exceeds 2^21 cells along one axis")
    return keys, [t - b for t, b in zip(top, base)]


def voxelize(data, voxel_size, round_first=False):
    """data [N, 3 (+ other columns)] -> (down-sampled [M, 3 (+ other)] float64 like the reference's np.hstack, trace).
    Coordinates: mean of the 2-decimal-rounded points of each voxel (in input order, double), then float32 and rounded to
    2 decimals as `generate_tiles` does (util/pipeline.py:44-45); with `round_first`, rounded to 2 decimals in double and
    then float32, as the training-data generator does (tools/data_gen/gen_train_data.py:40-42).  Other columns: those of
    the first point of the voxel.
    `trace` = dict(first_idx i64[M], point2vox i64[N]) on the device (the reference returns open3d's per-voxel index lists)."""
    L = _hip.lib()
    arr = data if torch.is_tensor(data) else torch.from_numpy(np.ascontiguousarray(data))
    xyz = _dev_f64(arr[:, :3])
    n = len(xyz)
    bound = float((torch.round(xyz * 100.0) / 100.0).abs().max()) + 100.0             # data_preparation.py:68-69
    origin = -bound - 0.5 * voxel_size                                                # open3d shifts the grid by half a voxel
    keys, _ = _keys(xyz, voxel_size, origin, True)
    skeys, perm = torch.sort(keys, stable=True)
    out = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
    first = torch.empty(n, dtype=torch.int64, device=xyz.device); p2v = torch.empty(n, dtype=torch.int64, device=xyz.device)
    m = torch.empty(1, dtype=torch.int64, device=xyz.device)
    ws = torch.empty(int(L.tl_downsample_ws_words(n)), dtype=torch.int32, device=xyz.device)
    fn = L.tl_downsample_reduce_r64 if round_first else L.tl_downsample_reduce
    _hip.check(fn(_hip.ptr(xyz), _hip.ptr(skeys), _hip.ptr(perm), n, _hip.ptr(out), _hip.ptr(first), _hip.ptr(p2v), _hip.ptr(m),
                  _hip.ptr(ws), _hip.stream()), "tl_downsample_reduce")
    M = int(m.item())
    pts = out[:M]; first = first[:M]
    if arr.shape[1] > 3:
        other = arr[:, 3:].to(xyz.device).index_select(0, first)
        pts = torch.cat([pts.double(), other.double()], 1)
    return pts, dict(first_idx=first, point2vox=p2v)


def compute_features(points, search_radius=0.6, feature_names=("verticality",)):
    """points [N,3] -> float32 [N,F] in the order of `feature_names` (any of util.features.FEATURE_NAMES, no duplicates), NaNs replaced
    per column by the mean of the column's finite values (replace_nanfeatures).  ["verticality"] alone is the path of the pipeline
    (util/pipeline.py:64) through tl_verticality; every other list goes through tl_eigen_features."""
    from .features import feature_ids
    ids = feature_ids(feature_names)                                                  # ValueError before any GPU work
    if list(feature_names) != ["verticality"]:
        return _eigen_features(points, search_radius, ids)
    L = _hip.lib()
    xyz = _dev_f64(points)
    n = len(xyz)
    origin = float(xyz.min()) - search_radius
    keys, ext = _keys(xyz, search_radius, origin, False)
    skeys, perm = torch.sort(keys)
    sx = xyz.index_select(0, perm).contiguous()
    v = torch.empty(n, dtype=torch.float32, device=xyz.device)
    _hip.check(L.tl_verticality(_hip.ptr(sx), _hip.ptr(skeys), n, float(search_radius), _I64x2(ext[0], ext[1]), _hip.ptr(v), _hip.stream()), "tl_verticality")
    out = torch.empty_like(v); out[perm] = v
    nan = torch.isnan(out)
    if bool(nan.any()):
        out[nan] = out[~nan].double().mean().float() if bool((~nan).any()) else float("nan")
    return out.reshape(-1, 1)


PIECE = 64                                                                             # points per wave of tl_eigen_features
_COLUMN_SHIFT = 21                                                                     # tl_cell_keys: z-cell in the low 21 bits


def feature_pieces(sorted_keys):
    """The work table of tl_eigen_features (device i64[n_pieces]): the sorted index of every point that starts an (x, y) column of cells
    or whose index is a multiple of PIECE.  Its length is the one value read back to the host."""
    n = len(sorted_keys)
    col = sorted_keys >> _COLUMN_SHIFT
    start = (torch.arange(n, dtype=torch.int64, device=sorted_keys.device) % PIECE) == 0
    start[1:] |= col[1:] != col[:-1]
    return torch.nonzero(start).squeeze(1).contiguous()


def sorted_cells(xyz, search_radius):
    """f64 device points -> (points sorted by their `search_radius`-sized cell with z fastest, sorted keys, stable permutation, extent)."""
    origin = float(xyz.min()) - search_radius
    keys, ext = _keys(xyz, search_radius, origin, False)
    skeys, perm = torch.sort(keys, stable=True)
    return xyz.index_select(0, perm).contiguous(), skeys, perm, ext


def eigen_features_sorted(sx, skeys, ext, pieces, search_radius, ids):
    """tl_eigen_features on sorted points: f32 [n, len(ids)] in sorted order, NaNs left in."""
    L = _hip.lib()
    n, F = len(sx), len(ids)
    out = torch.empty((n, F), dtype=torch.float32, device=sx.device)
    cols = (ctypes.c_int32 * F)(*ids)
    _hip.check(L.tl_eigen_features(_hip.ptr(sx), _hip.ptr(skeys), n, float(search_radius), _I64x2(ext[0], ext[1]), _hip.ptr(pieces), len(pieces),
                                   ctypes.cast(cols, ctypes.c_void_p), F, _hip.ptr(out), _hip.stream()), "tl_eigen_features")
    return out


def _eigen_features(points, search_radius, ids, replace_nan=True):
    """compute_features through tl_eigen_features; replace_nan=False leaves the NaNs of the definition in (what the tests compare)."""
    xyz = _dev_f64(points)
    sx, skeys, perm, ext = sorted_cells(xyz, search_radius)
    v = eigen_features_sorted(sx, skeys, ext, feature_pieces(skeys), search_radius, ids)
    out = torch.empty_like(v); out[perm] = v
    if not replace_nan:
        return out
    finite = ~torch.isnan(out)
    # per column: f64 sum of the finite values / their count, cast to f32 (a column without a finite value stays NaN)
    mean = (torch.where(finite, out.double(), torch.zeros((), dtype=torch.float64, device=out.device)).sum(0) / finite.sum(0).double()).float()
    return torch.where(finite, out, mean.expand_as(out)).contiguous()


def eigen_features_scales_sorted(sx, skeys, ext, pieces, radii, ids):
    """tl_eigen_features_scales on points sorted by cells of max(radii): f32 [n, len(radii), len(ids)] in sorted order, NaNs left in.
    Every scale is, bit for bit, eigen_features_sorted on the same arrays at that radius."""
    from .features import check_radii
    radii = check_radii(radii)
    L = _hip.lib()
    n, S, F = len(sx), len(radii), len(ids)
    out = torch.empty((n, S, F), dtype=torch.float32, device=sx.device)
    cols, rad = (ctypes.c_int32 * F)(*ids), (ctypes.c_double * S)(*radii)
    _hip.check(L.tl_eigen_features_scales(_hip.ptr(sx), _hip.ptr(skeys), n, ctypes.cast(rad, ctypes.c_void_p), S, _I64x2(ext[0], ext[1]), _hip.ptr(pieces),
                                          len(pieces), ctypes.cast(cols, ctypes.c_void_p), F, _hip.ptr(out), _hip.stream()), "tl_eigen_features_scales")
    return out


def compute_features_scales(points, radii, feature_names, replace_nan=True):
    """points [N, 3] -> float32 [N, S, F]: the features of `feature_names` (any of util.features.FEATURE_NAMES, no duplicates) at every
    radius of `radii` (1 .. 4, strictly ascending), in input order, from one cell sort at max(radii), one work table and one launch of
    tl_eigen_features_scales.  NaNs are replaced per (scale, column) by the mean of that column's finite values at that scale, the rule
    of compute_features; replace_nan=False leaves them in."""
    from .features import check_radii, feature_ids
    ids, radii = feature_ids(feature_names), check_radii(radii)                       # ValueError before any GPU work
    xyz = _dev_f64(points)
    sx, skeys, perm, ext = sorted_cells(xyz, radii[-1])
    v = eigen_features_scales_sorted(sx, skeys, ext, feature_pieces(skeys), radii, ids)
    out = torch.empty_like(v); out[perm] = v
    if not replace_nan:
        return out
    finite = ~torch.isnan(out)
    mean = (torch.where(finite, out.double(), torch.zeros((), dtype=torch.float64, device=out.device)).sum(0) / finite.sum(0).double()).float()
    return torch.where(finite, out, mean.expand_as(out)).contiguous()


def propagate_to_original(preds_voxelized, trace):
    """Every original point takes the prediction of its voxel (util/pipeline.py:441-452 without the hash dictionary)."""
    p = preds_voxelized if torch.is_tensor(preds_voxelized) else torch.from_numpy(np.asarray(preds_voxelized))
    return p.to(trace["point2vox"].device).index_select(0, trace["point2vox"])
