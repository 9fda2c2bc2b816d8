"""Hand cases of tl_cross_nn.  A case is a dict: ref f64[nr, 3], q f32 / f64 [nq, 3 or 4], T (3 x 4 or None), max_dist, cell
(None: 1.001 * max_dist) and check(nn, d2), which holds the case's own expected values -- written down by hand, not computed by any
search.  The grid of a case starts at the reference's minimum corner (util.outlier._Grid), which is what places the borders below."""
import numpy as np

INF = np.inf


def _d2(p, r):
    """(dx*dx + dy*dy) + dz*dz in Python floats (IEEE double, one rounding per operation)."""
    dx, dy, dz = float(r[0]) - float(p[0]), float(r[1]) - float(p[1]), float(r[2]) - float(p[2])
    return (dx * dx + dy * dy) + dz * dz


def _case(ref, q, nn, d2, T=None, max_dist=1.0, cell=None, dtype=np.float64):
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype)
    q = q.reshape(-1, q.shape[-1] if q.ndim == 2 else 3)
    want_nn, want_d2 = np.asarray(nn, np.int64).reshape(-1), np.asarray(d2, np.float64).reshape(-1)

    def check(got_nn, got_d2):
        got_nn, got_d2 = np.asarray(got_nn), np.asarray(got_d2)
        assert got_nn.dtype == np.int64 and got_d2.dtype == np.float64, (got_nn.dtype, got_d2.dtype)
        assert got_nn.shape == want_nn.shape and got_d2.shape == want_d2.shape
        assert np.array_equal(got_nn, want_nn), (got_nn, want_nn)
        assert got_d2.tobytes() == want_d2.tobytes(), (got_d2, want_d2)

    return dict(ref=ref, q=q, T=None if T is None else np.asarray(T, np.float64), max_dist=float(max_dist), cell=cell, check=check)


def cell_border():
    """h = 1.001: the query stands exactly on the border of cells 0 and 1; its neighbour lies in cell 0, a farther point in cell 1."""
    ref = [(0, 0, 0), (0.5, 0, 0), (1.9, 0, 0), (3.5, 0, 0)]
    q = [(1.001, 0, 0)]
    return _case(ref, q, [1], [_d2(q[0], ref[1])])


def outside_the_grid():
    """Queries one cell below and above the grid: within max_dist of a border point, beyond it, and two cells out."""
    ref = [(0, 0, 0), (2, 2, 2)]
    q = [(-0.9, 0, 0), (-1.0005, 0, 0), (-1.05, 0, 0), (2.9, 2, 2), (2, 2, 3.0005), (2, 4.5, 2), (0, -0.6, -0.6)]
    return _case(ref, q, [0, -1, -1, 1, -1, -1, 0], [_d2(q[0], ref[0]), INF, INF, _d2(q[3], ref[1]), INF, INF, _d2(q[6], ref[0])])


def far_and_not_finite():
    ref = [(0, 0, 0), (2, 2, 2)]
    q = [(1e12, 0, 0), (0, -1e12, 0), (1e300, 1e300, 1e300), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0.25, 0, 0)]
    return _case(ref, q, [-1] * 6 + [0], [INF] * 6 + [0.0625])


def far_after_the_transform():
    """A translation of 1e12 m, and one that overflows: the moved query is far away or not finite, the input is ordinary."""
    ref = [(0, 0, 0), (2, 2, 2)]
    T = [[1, 0, 0, 1e12], [0, 1, 0, 0], [0, 0, 1, 0]]
    return _case(ref, [(0.5, 0, 0), (-1e12, 0.5, 0)], [-1, 0], [INF, 0.25], T=T)


def overflow_after_the_transform():
    ref = [(0, 0, 0), (2, 2, 2)]
    T = [[1e308, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    return _case(ref, [(100.0, 0, 0), (0.0, 0.5, 0)], [-1, 0], [INF, 0.25], T=T)


def tie_first_order():
    return _case([(-0.5, 0, 0), (0.5, 0, 0), (3, 3, 3)], [(0, 0, 0)], [0], [0.25])


def tie_second_order():
    """The same two points in the other row order: the smaller ORIGINAL row wins, which is now the other point."""
    return _case([(0.5, 0, 0), (-0.5, 0, 0), (3, 3, 3)], [(0, 0, 0)], [0], [0.25])


def duplicates():
    ref = [(3, 3, 3), (0.25, 0.5, 0), (0, 0, 0), (0.25, 0.5, 0), (0.25, 0.5, 0)]
    q = [(0.25, 0.5, 0), (0.25, 0.75, 0)]
    return _case(ref, q, [1, 1], [0.0, 0.0625])


def exactly_max_dist():
    """d2 == max_dist * max_dist is not a neighbour (strict); the next smaller double is."""
    ref = [(0, 0, 0), (4, 0, 0)]
    below = float(np.nextafter(1.0, 0.0))
    q = [(1.0, 0, 0), (below, 0, 0), (0, -1.0, 0), (5.0, 0, 0)]
    return _case(ref, q, [-1, 0, -1, -1], [INF, below * below, INF, INF])


def exactly_max_dist_half():
    return _case([(0, 0, 0), (4, 0, 0)], [(0.5, 0, 0), (0.4375, 0, 0)], [-1, 0], [INF, 0.4375 * 0.4375], max_dist=0.5)


def rotation_to_negative_cells():
    """Half a turn about z sends the queries to negative coordinates, below the grid's corner."""
    T = [[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0]]
    ref = [(0, 0, 0.5), (3, 3, 1)]
    q = [(0.5, 0.5, 0.5), (2, 2, 0.5), (-3, -2.5, 1)]
    return _case(ref, q, [0, -1, 1], [0.5, INF, 0.25], T=T)


def no_reference():
    return _case(np.zeros((0, 3)), [(0, 0, 0), (1, 2, 3)], [-1, -1], [INF, INF])


def one_reference():
    return _case([(1, 2, 3)], [(1, 2, 3.5), (1, 2, 4.5), (1.5, 2.5, 3.5)], [0, -1, 0], [0.25, INF, 0.75])


def no_query():
    return _case([(0, 0, 0), (1, 1, 1)], np.zeros((0, 3)), [], [])


def one_query():
    return _case([(0, 0, 0), (1, 1, 1)], [(1, 1, 0.5)], [1], [0.25])


def _one_cell(n):
    """n reference points in one cell, 1 mm apart along x; the nearest is the LAST row, and the first of a second wave pass for n = 65, 129."""
    ref = [(0.001 * k, 0.125, 0.25) for k in range(n)] + [(5, 5, 5)]
    q = [(0.001 * (n - 1) + 0.0002, 0.125, 0.25), (-0.0002, 0.125, 0.25), (0.001 * 63 + 0.0004, 0.125, 0.25)]
    near = min(n - 1, 63)
    return _case(ref, q, [n - 1, 0, near], [_d2(q[0], ref[n - 1]), _d2(q[1], ref[0]), _d2(q[2], ref[near])])


def _formats(dtype, ld):
    """f32 queries are widened before anything else: 0.1f is 0.100000001490116..., and the distance is that of the widened value."""
    ref = [(0, 0, 0), (2, 2, 2)]
    rows = [(0.1, 0.2, 0.3), (1.7, 1.9, 2.1)]
    q = np.full((2, ld), 99.0, dtype)
    q[:, :3] = rows
    wide = q[:, :3].astype(np.float64)
    return _case(ref, q, [0, 1], [_d2(wide[0], ref[0]), _d2(wide[1], ref[1])], dtype=dtype)


def coarse_cell():
    """Any cell >= 1.0001 * max_dist gives the same answer."""
    c = cell_border()
    c["cell"] = 2.5
    return c


CASES = dict(cell_border=cell_border, outside_the_grid=outside_the_grid, far_and_not_finite=far_and_not_finite,
             far_after_the_transform=far_after_the_transform, overflow_after_the_transform=overflow_after_the_transform,
             tie_first_order=tie_first_order, tie_second_order=tie_second_order, duplicates=duplicates, exactly_max_dist=exactly_max_dist,
             exactly_max_dist_half=exactly_max_dist_half, rotation_to_negative_cells=rotation_to_negative_cells, no_reference=no_reference,
             one_reference=one_reference, no_query=no_query, one_query=one_query, coarse_cell=coarse_cell,
             one_cell_63=lambda: _one_cell(63), one_cell_64=lambda: _one_cell(64), one_cell_65=lambda: _one_cell(65),
             one_cell_129=lambda: _one_cell(129),
             f32_ld3=lambda: _formats(np.float32, 3), f32_ld4=lambda: _formats(np.float32, 4), f64_ld3=lambda: _formats(np.float64, 3),
             f64_ld4=lambda: _formats(np.float64, 4))


# ------------------------------------------------------------------------------------------------ the scene of the registration tests
def scene(seed=0):
    """1 000 rows of gently sloped ground and six vertical cylinders of 333 rows each inside 12 x 12 x 6 m: (xyz f64[2998, 3], labels)."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.0, 12.0, (1000, 2))
    ground = np.column_stack([g, 0.05 * g[:, 0] + 0.03 * g[:, 1] + rng.normal(0.0, 0.01, 1000)])
    parts, labels = [ground], [np.zeros(1000, np.int64)]
    centres = [(2.0, 2.5), (6.0, 1.5), (10.0, 3.0), (3.0, 8.0), (7.0, 9.5), (10.5, 8.5)]
    for t, (cx, cy) in enumerate(centres):
        ang = rng.uniform(0.0, 2 * np.pi, 333); r = 0.12 + 0.02 * t
        z0 = 0.05 * cx + 0.03 * cy
        parts.append(np.column_stack([cx + r * np.cos(ang), cy + r * np.sin(ang), z0 + rng.uniform(0.0, 4.5, 333)]))
        labels.append(np.full(333, t + 1, np.int64))
    return np.concatenate(parts), np.concatenate(labels)


def true_transform(dof):
    """yaw 2 deg, pitch 0.3 deg (0 for dof 4), t = (0.15, -0.10, 0.05): moving -> reference."""
    yaw, pitch = np.deg2rad(2.0), np.deg2rad(0.3 if dof == 6 else 0.0)
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = (0.15, -0.10, 0.05)
    return T


def moved_copy(xyz, dof, seed=1):
    """(moving cloud, permutation): the rows of xyz permuted and moved by the inverse of true_transform(dof)."""
    T = true_transform(dof)
    perm = np.random.default_rng(seed).permutation(len(xyz))
    R, t = T[:3, :3], T[:3, 3]
    return (xyz[perm] - t) @ R, perm                                     # R^T (p - t), row-wise


def second_epoch(xyz, labels, seed=2):
    """The scene's second epoch: tree 3 gone, a new tree elsewhere, tree 5 one metre taller, the trees numbered in another order.
    Returns (xyz, labels, {reference id: second-epoch id})."""
    rng = np.random.default_rng(seed)
    renumber = {1: 4, 2: 6, 4: 1, 5: 2, 6: 5}                           # 3 is dropped; the new tree is 3 in the second epoch
    keep = labels != 3
    x2, l2 = xyz[keep].copy(), labels[keep].copy()
    ang = rng.uniform(0.0, 2 * np.pi, 80)
    cx, cy = 7.0, 9.5
    top = np.column_stack([cx + 0.2 * np.cos(ang), cy + 0.2 * np.sin(ang), 0.05 * cx + 0.03 * cy + rng.uniform(4.5, 5.5, 80)])
    ang = rng.uniform(0.0, 2 * np.pi, 300)
    cx, cy = 5.5, 5.0
    new = np.column_stack([cx + 0.15 * np.cos(ang), cy + 0.15 * np.sin(ang), 0.05 * cx + 0.03 * cy + rng.uniform(0.0, 4.0, 300)])
    x2 = np.concatenate([x2, top, new]); l2 = np.concatenate([l2, np.full(80, 5, np.int64), np.full(300, 7, np.int64)])
    out = np.zeros_like(l2)
    for a, b in renumber.items():
        out[l2 == a] = b
    out[l2 == 7] = 3
    return x2, out, renumber
