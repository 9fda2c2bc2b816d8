"""The plot outline -- mirrors reference tree_learn/util/pipeline.py `grid_points` (:226-238), `get_hull_buffer` (:240-253), `get_hull`
(:256-265), `shift_hull` (:268-273), `get_coords_within_shape` (:211-223) and `get_cluster_means` (:277-284).

The alpha shape (alphashape.alphashape -> polygonize + unary_union -> shift_hull's exterior ring) is restated on the host from the
Delaunay triangulation of the 0.25 m grid reduction; the per-point tests against it run on the device
(csrc/tl_hull.hip, `tl_ring_classify`).  A shape is a closed f64 ring plus, for the buffer of `get_hull_buffer`, a radius: the
reference's buffer of the ring LINE, i.e. every point closer to the ring than the radius, on either side."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from .. import _hip

HULL_ERROR = "failed to calculate concave hull. Set alpha=0 to use convex hull or set outer_remove=~"
_MAX_CELLS = 1 << 22


@dataclass
class Shape:
    """ring f64[V, 2], closed (ring[0] == ring[-1]); radius None for the hull polygon, the buffer distance otherwise."""
    ring: np.ndarray
    radius: float = None
    _index: dict = field(default_factory=dict, repr=False)


def _dev(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device="cuda", dtype=dtype or t.dtype)


def grid_points(coords, grid_size):
    """First point of every (floor(x / g), floor(y / g)) cell in first-occurrence order (pandas drop_duplicates), on the device in f64.
    floor(x / g) equals numpy's x // g for a power-of-two g such as the pipeline's 0.25 (the quotient is exact)."""
    xy = _dev(coords[:, :2], torch.float64).contiguous()
    if len(xy) == 0:
        return xy
    cell = torch.floor(xy / grid_size).to(torch.int64)
    c = cell - cell.min(0).values
    key = c[:, 0] * (int(c[:, 1].max()) + 1) + c[:, 1]
    skey, perm = torch.sort(key, stable=True)
    head = torch.ones_like(skey, dtype=torch.bool)
    head[1:] = skey[1:] != skey[:-1]
    first = torch.sort(perm[head]).values                       # the first member of each cell, in input order
    return xy.index_select(0, first)


def _convex_ring(p):
    from scipy.spatial import ConvexHull, QhullError
    try:
        v = ConvexHull(p).vertices                              # counter-clockwise in 2-D
    except (QhullError, ValueError) as e:
        raise ValueError(HULL_ERROR) from e
    return p[np.r_[v, v[:1]]]


def filled_triangles(tri, alpha):
    """Boolean per Delaunay simplex: circumradius < 1 / alpha (zero-area triangles never), plus every other triangle that cannot reach the
    convex-hull boundary through shared edges of other non-kept triangles (the holes that polygonize + unary_union fill)."""
    p = tri.points[tri.simplices]                               # [T, 3, 2]
    a = np.linalg.norm(p[:, 1] - p[:, 2], axis=1)
    b = np.linalg.norm(p[:, 0] - p[:, 2], axis=1)
    c = np.linalg.norm(p[:, 0] - p[:, 1], axis=1)
    area2 = np.abs((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        circ = a * b * c / (2.0 * area2)                        # abc / (4 * area)
    kept = (area2 > 0) & (circ < 1.0 / alpha)
    nb = tri.neighbors
    reach = ~kept & (nb == -1).any(1)
    front = np.flatnonzero(reach)
    while len(front):
        n = nb[front].reshape(-1)
        n = n[n >= 0]
        n = n[~kept[n] & ~reach[n]]
        n = np.unique(n)
        reach[n] = True
        front = n
    return ~reach


def _edge_connected(tri, filled):
    idx = np.flatnonzero(filled)
    seen = np.zeros(len(filled), bool)
    seen[idx[0]] = True
    front = idx[:1]
    while len(front):
        n = tri.neighbors[front].reshape(-1)
        n = np.unique(n[n >= 0])
        n = n[filled[n] & ~seen[n]]
        seen[n] = True
        front = n
    return bool(seen[filled].all())


def _trace_ring(tri, filled):
    s = tri.simplices[filled]
    p = tri.points
    orient = ((p[s[:, 1], 0] - p[s[:, 0], 0]) * (p[s[:, 2], 1] - p[s[:, 0], 1])
              - (p[s[:, 1], 1] - p[s[:, 0], 1]) * (p[s[:, 2], 0] - p[s[:, 0], 0]))
    s = np.where((orient < 0)[:, None], s[:, ::-1], s)          # counter-clockwise triangles
    nb = tri.neighbors[filled]
    nb = np.where((orient < 0)[:, None], nb[:, ::-1], nb)      # neighbour j is opposite vertex j
    src, dst = [], []
    for j in range(3):                                          # edge opposite vertex j: s[(j+1)%3] -> s[(j+2)%3]
        out = (nb[:, j] < 0) | ~filled[np.maximum(nb[:, j], 0)]
        src.append(s[out, (j + 1) % 3]); dst.append(s[out, (j + 2) % 3])
    src, dst = np.concatenate(src), np.concatenate(dst)
    if len(np.unique(src)) != len(src):
        raise ValueError(HULL_ERROR)                            # a vertex the boundary passes twice: not one simple ring
    nxt = dict(zip(src.tolist(), dst.tolist()))
    start = int(src.min())
    ring = [start]
    v = nxt[start]
    while v != start:
        ring.append(v)
        v = nxt[v]
        if len(ring) > len(src):
            raise ValueError(HULL_ERROR)
    if len(ring) != len(src):
        raise ValueError(HULL_ERROR)                            # more than one boundary ring
    ring.append(start)
    return p[np.asarray(ring)]


def alpha_ring(points, alpha):
    """Exterior ring (closed, counter-clockwise, f64) of the alpha shape of 2-D points (host)."""
    from scipy.spatial import Delaunay, QhullError
    p = np.asarray(points, np.float64)
    if alpha <= 0 or len(p) < 4:
        return _convex_ring(p)
    try:
        tri = Delaunay(p)
    except (QhullError, ValueError) as e:
        raise ValueError(HULL_ERROR) from e
    filled = filled_triangles(tri, alpha)
    if not filled.any() or not _edge_connected(tri, filled):
        raise ValueError(HULL_ERROR)                            # empty, or a MultiPolygon: shift_hull's assertion
    return _trace_ring(tri, filled)


def _ring_of(coords, alpha):
    xy = _dev(coords[:, :2], torch.float64)
    mean = xy.mean(0).cpu().numpy()
    grid = grid_points(xy - torch.from_numpy(mean).to(xy.device), 0.25).cpu().numpy()
    return alpha_ring(grid, alpha) + mean                         # shift_hull


def get_hull(coords, alpha):
    return Shape(_ring_of(coords, alpha))


def get_hull_buffer(coords, alpha, buffersize):
    return Shape(_ring_of(coords, alpha), float(buffersize))


def _ring_index(ring, r, device):
    """Slab and cell lists of a ring on the device (include/treelearn_hip.h tl_ring_lists / tl_ring_covered)."""
    L = _hip.lib()
    ring = np.ascontiguousarray(ring, np.float64)
    V = len(ring)
    if V < 4 or not np.array_equal(ring[0], ring[-1]) or not np.isfinite(ring).all():
        raise ValueError("a ring needs at least 3 distinct vertices, closed (first vertex repeated last), all finite")
    g = _hip.RingGrid()
    lo, hi = ring.min(0), ring.max(0)
    pad = 1e-9 * (float(np.abs(ring).max()) + r + 1.0) + 1e-7 * (1.0 + r)     # far above the rounding of the per-point formulas
    g.r, g.pad = float(r), pad
    g.nslab = int(min(max((V - 1) // 2, 1), 1 << 20))
    g.slab_lo = float(lo[1] - pad)
    g.slab_h = float((hi[1] - lo[1] + 2 * pad) / g.nslab)
    if r > 0:
        glo = lo - r - pad
        ext = hi + r + pad - glo
        h = max(r / 2, float(ext.max()) / 1024, float(np.sqrt(ext[0] * ext[1] / _MAX_CELLS)))
        g.lo[:] = [float(v) for v in glo]
        g.h = h
        g.nx, g.ny = int(ext[0] // h) + 1, int(ext[1] // h) + 1
        g.cover_r2 = (r - 2 * pad) ** 2 if r > 2 * pad else 0.0
    ncells = g.nx * g.ny
    d_ring = torch.from_numpy(ring).to(device)
    cell_cnt = torch.zeros(max(ncells, 1), dtype=torch.int64, device=device)
    slab_cnt = torch.zeros(g.nslab, dtype=torch.int64, device=device)
    _hip.check(L.tl_ring_lists(_hip.ptr(d_ring), V, ctypes.byref(g), _hip.ptr(cell_cnt), _hip.ptr(slab_cnt), None, None, _hip.stream()),
               "tl_ring_lists")
    cell_start = torch.zeros(ncells + 1, dtype=torch.int64, device=device); cell_start[1:] = torch.cumsum(cell_cnt[:ncells], 0)
    slab_start = torch.zeros(g.nslab + 1, dtype=torch.int64, device=device); slab_start[1:] = torch.cumsum(slab_cnt, 0)
    n_slab, n_cell = (int(v) for v in torch.stack([slab_start[-1], cell_start[-1]]).cpu())
    if max(n_slab, n_cell) >= (1 << 31):
        raise ValueError("ring lists exceed 2^31 entries")
    slab_seg = torch.empty(max(n_slab, 1), dtype=torch.int32, device=device)
    cell_seg = torch.empty(max(n_cell, 1), dtype=torch.int32, device=device)
    cell_cur = cell_start[:-1].clone() if ncells else cell_cnt
    slab_cur = slab_start[:-1].clone()
    _hip.check(L.tl_ring_lists(_hip.ptr(d_ring), V, ctypes.byref(g), _hip.ptr(cell_cur), _hip.ptr(slab_cur), _hip.ptr(cell_seg), _hip.ptr(slab_seg),
                               _hip.stream()), "tl_ring_lists")
    covered = torch.zeros(max(ncells, 1), dtype=torch.uint8, device=device)
    _hip.check(L.tl_ring_covered(_hip.ptr(d_ring), ctypes.byref(g), _hip.ptr(cell_start), _hip.ptr(cell_seg), _hip.ptr(covered), _hip.stream()),
               "tl_ring_covered")
    return dict(grid=g, ring=d_ring, slab_start=slab_start, slab_seg=slab_seg, cell_start=cell_start, cell_seg=cell_seg, covered=covered,
                entries=n_slab + n_cell)


def ring_classify(points, ring, r=0.0, index=None):
    """u8 device tensor per point: bit 0 = strictly inside the closed ring, bit 1 = distance to the ring < r (include/treelearn_hip.h
    tl_ring_classify).  points: [n, >= 2] f32 / f64 rows (device or host); only x and y are read."""
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if pts.dtype not in (torch.float32, torch.float64):
        pts = pts.double()
    pts = pts.to("cuda")
    if pts.ndim != 2 or pts.shape[1] < 2:
        raise ValueError(f"points must be [n, >= 2], got {tuple(pts.shape)}")
    if pts.stride(1) != 1 or (len(pts) > 1 and pts.stride(0) < pts.shape[1]):
        pts = pts.contiguous()
    idx = index if index is not None else _ring_index(ring, float(r), pts.device)
    out = torch.empty(len(pts), dtype=torch.uint8, device=pts.device)
    ld = pts.stride(0) if len(pts) > 1 else pts.shape[1]
    _hip.check(_hip.lib().tl_ring_classify(_hip.ptr(pts), int(pts.dtype == torch.float64), ld, len(pts), _hip.ptr(idx["ring"]),
                                           ctypes.byref(idx["grid"]), _hip.ptr(idx["slab_start"]), _hip.ptr(idx["slab_seg"]),
                                           _hip.ptr(idx["cell_start"]), _hip.ptr(idx["cell_seg"]), _hip.ptr(idx["covered"]),
                                           _hip.ptr(out), _hip.stream()), "tl_ring_classify")
    return out


def get_coords_within_shape(coords, shape):
    """Device bool mask: inside the hull polygon (radius None), or within `radius` of its ring on either side (a hull buffer)."""
    r = 0.0 if shape.radius is None else float(shape.radius)
    key = (r, torch.cuda.current_device())
    if key not in shape._index:
        shape._index[key] = _ring_index(shape.ring, r, torch.device("cuda"))
    bits = ring_classify(coords, shape.ring, r, shape._index[key])
    return (bits & (1 if shape.radius is None else 2)) != 0


def get_cluster_means(coords, labels):
    """Per-label mean of the coordinate rows in ascending label order, as pandas groupby('label').mean() computes it: per group and
    column a compensated (Kahan) sum in the rows' own dtype, in row order, then divided by the count in that dtype (golden G14: float32
    rows give float32 means, bit for bit).  Device in, device out; one vectorised step per row rank over all groups at once (the
    step count is the largest group's size)."""
    c = _dev(coords)
    if c.dtype not in (torch.float32, torch.float64):
        c = c.double()
    lab = _dev(labels, torch.int64).reshape(-1)
    uniq, inv, cnt = torch.unique(lab, return_inverse=True, return_counts=True)
    G, C = len(uniq), c.shape[1]
    s = torch.zeros((G, C), dtype=c.dtype, device=c.device)
    if G == 0:
        return s
    comp = torch.zeros_like(s)
    _, perm = torch.sort(inv, stable=True)
    rows = c.index_select(0, perm)                               # rows grouped by label, row order kept within a group
    start = torch.cumsum(cnt, 0) - cnt
    by_size = torch.argsort(cnt, descending=True, stable=True)
    cnt_desc = cnt[by_size].cpu().numpy()
    start_desc = start[by_size]
    n_active = len(cnt_desc)
    for k in range(int(cnt_desc[0])):
        while n_active and cnt_desc[n_active - 1] <= k:
            n_active -= 1
        g = by_size[:n_active]
        v = rows.index_select(0, start_desc[:n_active] + k)
        y = v - comp[g]
        t = s[g] + y
        comp[g] = (t - s[g]) - y
        s[g] = t
    return s / cnt.to(c.dtype)[:, None]
