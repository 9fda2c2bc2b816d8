"""Statistical and radius outlier removal on the device -- the reference's `sor_filter` and `rad_filter`
(tree_learn/util/data_preparation.py:589-614), which `SampleGenerator` applies to every training crop (:281-287) and every
inference or validation tile (:446-454) when the `sample_generator` keys n_neigh_sor / multiplier_sor and rad / npoints_rad are set.

The reference delegates both to open3d (`remove_statistical_outlier`, `remove_radius_outlier`).  open3d is not part of the reference
tree and not installable here, so -- as with util/prepare.py -- the published algorithm is restated (recalled from open3d 0.17 and
nanoflann) and THAT RESTATEMENT IS THE SPECIFICATION; parity with open3d itself is unpinned.  All arithmetic is float64,
d2(i, j) = (dx*dx + dy*dy) + dz*dz in that order without fma contraction, d = sqrt(d2) correctly rounded.

  statistical (nb_neighbors = k, std_ratio = s):
    avg[i]  = (sum of the min(k, n) smallest d(i, .), point i itself included at distance 0, added in ascending order) / min(k, n)
    mean    = (sum of avg[i] over avg[i] > 0) / n                      (the divisor is n)
    std     = sqrt((sum of (avg[i] - mean)^2 over avg[i] > 0) / (n - 1))
    keep[i] = avg[i] > 0 and avg[i] < mean + s * std                   (n <= 1 and k = 1 keep nothing)
  radius (radius = r, nb_points = m):
    count[i] = number of j, i included, with d2(i, j) < r * r          (strict)
    keep[i]  = count[i] > m

A filter is active only when both keys of its pair are set.  A pair with one key set is refused: the reference silently ignores it, here
it is taken for a config mistake.  With both filters active the statistical one runs first and the radius filter sees only its survivors.

Kernels: csrc/tl_outlier.hip (tl_outlier_keys, tl_knn_mean_dist, tl_sor_keep, tl_radius_count); torch sorts the cell keys."""
import ctypes

import numpy as np
import torch

from .. import _hip

PAIRS = (("n_neigh_sor", "multiplier_sor"), ("rad", "npoints_rad"))
MAX_NEIGHBOURS = 64                                  # tl_knn_mean_dist keeps the k best one per lane of a wavefront
_MAX_CELLS = 1 << 21                                 # cells per axis of the Morton key
_D3 = ctypes.c_double * 3


def _get(cfg, k):
    if cfg is None:
        return None
    return cfg.get(k) if isinstance(cfg, dict) else getattr(cfg, k, None)


def active_filters(cfg):
    """The parsed pairs of a `sample_generator` section (dict or namespace): dict(sor=(k, s) or None, rad=(r, m) or None).
    NotImplementedError names a key that is set without its partner; ValueError for k outside 1..64, s <= 0, r <= 0 or m < 0."""
    if isinstance(cfg, dict) and set(cfg) == {"sor", "rad"}:
        return cfg
    for a, b in PAIRS:
        for one, other in ((a, b), (b, a)):
            if _get(cfg, one) is not None and _get(cfg, other) is None:
                raise NotImplementedError(f"{one} is set but {other} is not: an outlier filter needs both keys of its pair "
                                          "(the reference ignores a half-set pair; here it is refused as a config mistake)")
    sor = rad = None
    if _get(cfg, "n_neigh_sor") is not None:
        k, s = _get(cfg, "n_neigh_sor"), float(_get(cfg, "multiplier_sor"))
        if int(k) != k or not 1 <= int(k) <= MAX_NEIGHBOURS:
            raise ValueError(f"n_neigh_sor must be an integer in 1..{MAX_NEIGHBOURS}, got {k!r}")
        if not s > 0:
            raise ValueError(f"multiplier_sor must be > 0, got {s!r}")
        sor = (int(k), s)
    if _get(cfg, "rad") is not None:
        r, m = float(_get(cfg, "rad")), _get(cfg, "npoints_rad")
        if not (r > 0 and np.isfinite(r)):
            raise ValueError(f"rad must be > 0, got {r!r}")
        if int(m) != m or int(m) < 0:
            raise ValueError(f"npoints_rad must be an integer >= 0, got {m!r}")
        rad = (r, int(m))
    return dict(sor=sor, rad=rad)


def _xyz64(points):
    """(f64 [n,3] contiguous device tensor, whether the input was a host array)."""
    host = not torch.is_tensor(points)
    t = torch.from_numpy(np.array(np.asarray(points)[:, :3])) if host else points[:, :3]          # a copy: contiguous and writable
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points must be float32 or float64, got {t.dtype}")
    return t.to(device="cuda", dtype=torch.float64).contiguous(), host


def knn_cell(k):
    """Cell edge of the k-NN grid, metres.  Chosen from the clouds this project filters: voxelised at 0.1 m, so a surface holds about
    100 points per m^2 and the k-th neighbour lies near 0.056 sqrt(k) m; the walk ends at its first level when that is below the
    edge.  Any value gives the same results (a poor one costs coarser levels or longer candidate lists)."""
    return 0.1 + 0.08 * float(np.sqrt(k))


class _Grid:
    """Points sorted by the Morton key of a uniform grid of edge >= `cell` (grown until 2^21 cells per axis hold the cloud)."""

    def __init__(self, xyz, cell):
        n = len(xyz)
        lo = xyz.amin(0).cpu().numpy(); hi = xyz.amax(0).cpu().numpy()
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("points hold a non-finite coordinate")
        ext = float((hi - lo).max())
        h = max(float(cell), ext / (_MAX_CELLS - 2))                                  # never more than 2^21 cells: grow the cell instead
        dims = [int(np.floor((hi[a] - lo[a]) / h)) + 2 for a in range(3)]             # + 1 for the top cell, + 1 for the quotient's rounding
        self.lo, self.h, self.dims = _D3(*[float(v) for v in lo]), h, _hip.dims3(dims)
        L = _hip.lib()
        keys = torch.empty(n, dtype=torch.int64, device=xyz.device); err = torch.empty(1, dtype=torch.int32, device=xyz.device)
        _hip.check(L.tl_outlier_keys(_hip.ptr(xyz), n, self.lo, h, self.dims, _hip.ptr(keys), _hip.ptr(err), _hip.stream()), "tl_outlier_keys")
        self.keys, self.perm = torch.sort(keys)
        self.xyz = xyz.index_select(0, self.perm).contiguous()
        self._err = err

    def check(self):
        if int(self._err.item()):
            raise ValueError("a point fell outside the cell grid")


def knn_mean_dist(points, k, cell=None):
    """avg f64[n] (device): mean distance of every point to its min(k, n) nearest, itself included.  k in 1..64."""
    xyz, _ = _xyz64(points)
    n = len(xyz)
    avg = torch.empty(n, dtype=torch.float64, device=xyz.device)
    if n == 0:
        return avg
    g = _Grid(xyz, knn_cell(k) if cell is None else cell)
    _hip.check(_hip.lib().tl_knn_mean_dist(_hip.ptr(g.xyz), _hip.ptr(g.keys), _hip.ptr(g.perm), n, g.lo, g.h, g.dims, int(k), _hip.ptr(avg),
                                           _hip.stream()), "tl_knn_mean_dist")
    g.check()
    return avg


def sor_keep(avg, std_ratio):
    """(keep bool[n], thr f64[1]) on the device from the mean distances."""
    n = len(avg)
    keep = torch.empty(n, dtype=torch.uint8, device=avg.device); thr = torch.zeros(1, dtype=torch.float64, device=avg.device)
    if n == 0:
        return keep.bool(), thr
    L = _hip.lib()
    ws = torch.empty(int(L.tl_sor_ws_doubles(n)), dtype=torch.float64, device=avg.device)
    _hip.check(L.tl_sor_keep(_hip.ptr(avg), n, float(std_ratio), _hip.ptr(keep), _hip.ptr(thr), _hip.ptr(ws), _hip.stream()), "tl_sor_keep")
    return keep.bool(), thr


def radius_count(points, radius, cell=None):
    """count i32[n] (device): points strictly inside the ball of `radius` around every point, itself included."""
    xyz, _ = _xyz64(points)
    n = len(xyz)
    count = torch.empty(n, dtype=torch.int32, device=xyz.device)
    if n == 0:
        return count
    g = _Grid(xyz, 1.001 * float(radius) if cell is None else cell)                    # the ball lies inside the 27 cells around a point's own
    _hip.check(_hip.lib().tl_radius_count(_hip.ptr(g.xyz), _hip.ptr(g.keys), _hip.ptr(g.perm), n, g.lo, g.h, g.dims, float(radius), _hip.ptr(count),
                                          _hip.stream()), "tl_radius_count")
    g.check()
    return count


def _sor(xyz, k, s):
    if k < 1 or int(k) != k:
        raise ValueError(f"n_neigh_sor must be an integer >= 1, got {k!r}")
    if not s > 0:
        raise ValueError(f"multiplier_sor must be > 0, got {s!r}")
    return sor_keep(knn_mean_dist(xyz, int(k)), s)[0]


def _rad(xyz, r, m):
    if not r > 0:
        raise ValueError(f"rad must be > 0, got {r!r}")
    return radius_count(xyz, r) > int(m)


def _like(mask, host):
    return mask.cpu().numpy() if host else mask


def sor_filter(points, n_neigh_sor, multiplier_sor):
    """data_preparation.py:589-600: keep mask of open3d's remove_statistical_outlier as restated above.  points [n, >= 3] f32 / f64,
    device tensor or numpy array; the mask comes back as the same kind."""
    xyz, host = _xyz64(points)
    return _like(_sor(xyz, n_neigh_sor, multiplier_sor), host)


def rad_filter(points, rad, npoints_rad):
    """data_preparation.py:603-614: keep mask of open3d's remove_radius_outlier as restated above."""
    xyz, host = _xyz64(points)
    return _like(_rad(xyz, rad, npoints_rad), host)


def denoise(points, cfg):
    """The combined keep mask of the filters `cfg` activates (a `sample_generator` section or what active_filters returned): the
    statistical filter first, the radius filter on its survivors (data_preparation.py:281-287,446-454).  No filter: all True."""
    f = active_filters(cfg)
    xyz, host = _xyz64(points)
    keep = torch.ones(len(xyz), dtype=torch.bool, device=xyz.device)
    if f["sor"] is not None:
        keep = _sor(xyz, *f["sor"])
    if f["rad"] is not None:
        if f["sor"] is None:
            keep = _rad(xyz, *f["rad"])
        else:
            rows = keep.nonzero().squeeze(1)
            keep = torch.zeros_like(keep)
            keep[rows[_rad(xyz.index_select(0, rows), *f["rad"])]] = True
    return _like(keep, host)
