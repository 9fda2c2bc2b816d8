"""Scenes of the light stage worked by hand: voxels of 1 m in a 9 x 9 x 9 grid spanned by two corner rows, a few obstacle
rows, a few origins and directions, and what the walk must give for them.  Every case is a dict of xyz, labels (or None), voxel, origins,
skip (or None), dirs, ring, n_rings, max_range, min_hits and check(result), result = dict(counts, status, code, first) as numpy arrays."""
import numpy as np

CORNERS = [[0.5, 0.5, 0.5], [8.5, 8.5, 8.5]]
MID = [4.5, 4.5, 4.5]
UP = [0.0, 0.0, 1.0]
BLOCKED, TOP, RANGE, SIDE = 0, 1, 2, 3


def _scene(obstacles, origins, dirs, check, labels=None, skip=None, ring=None, n_rings=1, max_range=60.0, min_hits=1):
    xyz = np.array(CORNERS + [[i + 0.5, j + 0.5, k + 0.5] for i, j, k in obstacles], np.float64)
    lab = None if labels is None else np.array([0, 0] + list(labels), np.int64)
    dirs = np.array(dirs, np.float64).reshape(-1, 3)
    return dict(xyz=xyz, labels=lab, voxel=1.0, origins=np.array(origins, np.float64).reshape(-1, 3), skip=skip, dirs=dirs,
                ring=np.zeros(len(dirs), np.int32) if ring is None else np.array(ring, np.int32), n_rings=n_rings, max_range=max_range,
                min_hits=min_hits, check=check)


def empty_space():
    """Nothing but the two corner voxels: up leaves through the top, east and down through a side and the bottom."""
    def check(r):
        assert r["status"].tolist() == [0] and r["code"].tolist() == [[TOP, SIDE, SIDE]] and np.isnan(r["first"]).all()
        assert r["counts"].tolist() == [[[0, 1, 0, 0], [0, 0, 0, 2]]]
    return _scene([], [MID], [UP, [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]], check, ring=[0, 1, 1], n_rings=2)


def slab():
    """A closed slab at iz = 6, two voxels above the origin's: blocked overhead at t = 1.5 and at (0.8, 0, 0.6) at t = 2.5 = 1.5 / 0.6,
    while (0.96, 0, 0.28) leaves through the east side at t = 4.5 / 0.96 before it reaches the slab at 1.5 / 0.28."""
    def check(r):
        assert r["code"].tolist() == [[BLOCKED, BLOCKED, SIDE]]
        assert r["first"][0, 0] == 1.5 and r["first"][0, 1] == 1.5 / 0.6 and np.isnan(r["first"][0, 2])
        assert r["counts"].tolist() == [[[1, 0, 0, 0], [1, 0, 0, 1]]]
    return _scene([(i, j, 6) for i in range(9) for j in range(9)], [MID], [UP, [0.8, 0.0, 0.6], [0.96, 0.0, 0.28]], check, ring=[0, 1, 1], n_rings=2)


def one_voxel_on_the_vertical():
    """One voxel at (4, 4, 7): blocked straight up at t = 2.5; (0.6, 0, 0.8) passes it in voxel (6, 4, 7) and leaves through the top."""
    def check(r):
        assert r["code"].tolist() == [[BLOCKED, TOP]] and r["first"][0, 0] == 2.5 and r["counts"].tolist() == [[[1, 1, 0, 0]]]
    return _scene([(4, 4, 7)], [MID], [UP, [0.6, 0.0, 0.8]], check)


def space_diagonal_from_a_corner():
    """From the corner (4, 4, 4) along (1, 1, 1) / sqrt 3 the three times tie at every step: x, then y, then z, so the ray visits (5, 4, 4),
    (5, 5, 4), (5, 5, 5) and none of (4, 5, 4), (4, 4, 5), (4, 5, 5), which are occupied: it is blocked at (5, 5, 5) at the tied time."""
    d = 1.0 / np.sqrt(3.0)

    def check(r):
        assert r["code"].tolist() == [[BLOCKED]] and r["first"][0, 0] == (5.0 * 1.0 - 4.0) / d
    return _scene([(4, 5, 4), (4, 4, 5), (4, 5, 5), (5, 5, 5)], [[4.0, 4.0, 4.0]], [[d, d, d]], check)


def diagonal_takes_x_first():
    """The same ray with (5, 4, 4) occupied: the first step of the three-way tie is x."""
    d = 1.0 / np.sqrt(3.0)

    def check(r):
        assert r["code"].tolist() == [[BLOCKED]] and r["first"][0, 0] == 1.0 / d
    return _scene([(5, 4, 4), (5, 5, 5)], [[4.0, 4.0, 4.0]], [[d, d, d]], check)


def origin_on_a_face():
    """An origin on the face x = 4 belongs to voxel 4; westwards it enters voxel 3 at t = 0 and is blocked there; (0, -0.6, -0.8) does not
    move in x and leaves through the bottom."""
    def check(r):
        assert r["status"].tolist() == [0] and r["code"].tolist() == [[BLOCKED, BLOCKED, SIDE]]
        assert r["first"][0, 0] == 0.0 and r["first"][0, 1] == 0.0 and np.isnan(r["first"][0, 2])
    return _scene([(3, 4, 4)], [[4.0, 4.5, 4.5]], [[-1.0, 0.0, 0.0], [-0.6, -0.8, 0.0], [0.0, -0.6, -0.8]], check)


def two_hits():
    """min_hits = 2: voxels at (4, 4, 6) and (4, 4, 8) block the vertical at the second, t = 3.5; (0.6, 0, 0.8) meets only (6, 4, 7)
    and leaves through the top."""
    def check(r):
        assert r["code"].tolist() == [[BLOCKED, TOP]] and r["first"][0, 0] == 3.5
    return _scene([(4, 4, 6), (4, 4, 8), (6, 4, 7)], [MID], [UP, [0.6, 0.0, 0.8]], check, min_hits=2)


def range_ends_before_the_obstacle():
    """max_range = 2: the planes above the origin are at 0.5, 1.5 and 2.5, the obstacle (4, 4, 7) would be entered at 2.5."""
    def check(r):
        assert r["code"].tolist() == [[RANGE]] and np.isnan(r["first"]).all() and r["counts"].tolist() == [[[0, 0, 1, 0]]]
    return _scene([(4, 4, 7)], [MID], [UP], check, max_range=2.0)


def skip_the_owner():
    """The only obstacle belongs to tree 5: an origin that skips 5 sees the sky, one that skips 3 or nothing is blocked."""
    def check(r):
        assert r["code"].tolist() == [[TOP], [BLOCKED], [BLOCKED]] and r["first"][1, 0] == 2.5
    return _scene([(4, 4, 7)], [MID, MID, MID], [UP], check, labels=[5], skip=np.array([5, 3, -1], np.int32))


def origin_outside():
    """An origin beyond the grid: status 1, no counts, code 255; the one inside is counted."""
    def check(r):
        assert r["status"].tolist() == [1, 0, 1] and r["counts"].tolist() == [[[0, 0, 0, 0]], [[0, 1, 0, 0]], [[0, 0, 0, 0]]]
        assert r["code"].tolist() == [[255], [TOP], [255]] and np.isnan(r["first"]).all()
    return _scene([], [[20.0, 4.5, 4.5], MID, [4.5, 4.5, -0.5]], [UP], check)


CASES = {f.__name__: f for f in (empty_space, slab, one_voxel_on_the_vertical, space_diagonal_from_a_corner, diagonal_takes_x_first, origin_on_a_face,
                                 two_hits, range_ends_before_the_obstacle, skip_the_owner, origin_outside)}
