"""Host side of the plot outline and of the segmentation command line (treelearn_amd/util/hull.py, util/segment.py): the alpha-shape ring
against the independent triangle-set statement of tests/edge_restatement.py, its error paths, and argument validation.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from edge_restatement import inside_alpha_shape, ring_bits
from treelearn_amd.util.hull import HULL_ERROR, alpha_ring, filled_triangles

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(mask_fn, extent, spacing=0.25, seed=0):
    """Jittered grid points inside a shape (one per 0.25 m cell, like grid_points leaves them)."""
    rng = np.random.default_rng(seed)
    g = np.arange(-extent, extent, spacing)
    xx, yy = np.meshgrid(g, g, indexing="ij")
    p = np.column_stack([xx.ravel(), yy.ravel()]) + rng.uniform(0, spacing * 0.9, size=(xx.size, 2))
    return p[mask_fn(p[:, 0], p[:, 1])]


SHAPES = {
    "convex": lambda x, y: (np.abs(x) < 8) & (np.abs(y) < 6),
    "concave_c": lambda x, y: (np.hypot(x, y) < 9) & ~((x > -2) & (np.abs(y) < 3)),
    "clearing": lambda x, y: (np.abs(x) < 9) & (np.abs(y) < 9) & (np.hypot(x - 1, y) > 3.5),
    # a C whose tips touch: an annulus cut by a slit narrower than the point spacing -> the hole is enclosed and filled
    "c_tips_touch": lambda x, y: (np.hypot(x, y) < 9) & (np.hypot(x, y) > 4) & ~((x > 0) & (np.abs(y) < 0.05)),
}


def _check_ring(points, alpha, seed=1):
    ring = alpha_ring(points, alpha)
    assert np.array_equal(ring[0], ring[-1]) and len(ring) >= 4
    rng = np.random.default_rng(seed)
    lo, hi = points.min(0) - 1, points.max(0) + 1
    q = rng.uniform(lo, hi, size=(20000, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        ours = (ring_bits(q[:, 0], q[:, 1], ring, 0.0) & 1).astype(bool)
    if alpha <= 0:
        from scipy.spatial import Delaunay
        ref = Delaunay(points).find_simplex(q) >= 0
    else:
        ref = inside_alpha_shape(points, alpha, q)
    assert (ours != ref).sum() == 0, f"{(ours != ref).sum()} of {len(q)} query points disagree"
    return ring, ours


@pytest.mark.parametrize("alpha", [0.0, 0.6, 2.0])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_alpha_ring_matches_triangle_set(shape, alpha):
    pts = _cloud(SHAPES[shape], 10)
    _check_ring(pts, alpha)


def test_clearing_and_touching_tips_are_filled():
    for shape, centre in (("clearing", (1.0, 0.0)), ("c_tips_touch", (0.0, 0.0))):
        ring = alpha_ring(_cloud(SHAPES[shape], 10), 0.6)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert ring_bits(np.array([centre[0]]), np.array([centre[1]]), ring, 0.0)[0] & 1, shape
    ring = alpha_ring(_cloud(SHAPES["concave_c"], 10), 0.6)                 # the C's opening stays outside
    with np.errstate(divide="ignore", invalid="ignore"):
        assert not ring_bits(np.array([5.0]), np.array([0.0]), ring, 0.0)[0] & 1


def test_lobes_joined_at_one_vertex_raise():
    p = np.array([[0.0, 0.0], [-1.0, 0.3], [-1.0, -0.3], [1.0, 0.3], [1.0, -0.3]])
    with pytest.raises(ValueError, match="failed to calculate concave hull"):
        alpha_ring(p, 1.0)
    assert len(alpha_ring(p, 0.0)) == 5                                      # the convex hull: 4 vertices, closed


def test_empty_alpha_shape_raises():
    pts = _cloud(SHAPES["convex"], 10, spacing=2.0)
    with pytest.raises(ValueError, match="failed to calculate concave hull"):
        alpha_ring(pts, 50.0)                                                # no triangle has circumradius < 2 cm


def test_few_points_and_degenerate_paths():
    tri3 = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 1.0]])
    ring = alpha_ring(tri3, 5.0)                                             # < 4 points: convex hull whatever alpha
    assert len(ring) == 4 and {tuple(v) for v in ring} == {tuple(v) for v in tri3}
    with pytest.raises(ValueError, match="failed to calculate concave hull"):
        alpha_ring(tri3[:2], 0.6)                                            # no polygon from 2 points
    with pytest.raises(ValueError, match="failed to calculate concave hull"):
        alpha_ring(np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]), 0.6)   # collinear: no triangulation

    class Tri:                                                               # a zero-area simplex is never kept, and not enclosed here
        points = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
        simplices = np.array([[0, 1, 2]])
        neighbors = np.array([[-1, -1, -1]])
    assert not filled_triangles(Tri, 0.6).any()
    assert HULL_ERROR.startswith("failed to calculate concave hull")


def _cli(*args, timeout=60):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, "-m", "treelearn_amd.util.segment", *args], capture_output=True, text=True, timeout=timeout, cwd=REPO, env=env)


def test_cli_argument_validation(tmp_path):
    forest = tmp_path / "plot.npy"
    np.save(forest, np.zeros((10, 3)))
    w = tmp_path / "w.pth"
    w.write_bytes(b"")
    base = ["--forest", str(forest), "--weights", str(w), "--out", str(tmp_path / "out")]
    p = _cli(*base, "--formats", "laz")
    try:
        import laspy  # noqa: F401
    except ImportError:
        assert p.returncode != 0 and "laspy" in p.stderr, p.stderr[-400:]     # fails before any model or GPU work
        assert not (tmp_path / "out").exists()
    p = _cli(*base, "--formats", "ply")
    assert p.returncode != 0 and "unknown save format" in p.stderr
    p = _cli(*base, "--return-type", "tiles")
    assert p.returncode == 2 and "invalid choice" in p.stderr
    p = _cli(*base, "--voxel-size", "0")
    assert p.returncode == 2 and "--voxel-size must be > 0" in p.stderr
    p = _cli(*base, "--inner-edge", "20")
    assert p.returncode == 2 and "--outer-edge must be >= --inner-edge" in p.stderr
    p = _cli("--forest", str(tmp_path / "missing.npy"), "--weights", str(w), "--out", str(tmp_path / "o"))
    assert p.returncode == 2 and "no such file" in p.stderr


def test_load_forest_accepts_three_and_four_columns(tmp_path):
    from treelearn_amd.util.eval import load_points
    from treelearn_amd.util.segment import load_forest
    a3, a4 = np.random.default_rng(0).normal(size=(7, 3)), np.random.default_rng(1).normal(size=(7, 4))
    np.save(tmp_path / "a3.npy", a3); np.savez(tmp_path / "a4.npz", points=a4[:, :3], labels=a4[:, 3]); np.savetxt(tmp_path / "a3.txt", a3)
    assert np.array_equal(load_forest(str(tmp_path / "a3.npy")), a3)
    assert np.array_equal(load_forest(str(tmp_path / "a4.npz")), a4)
    assert np.allclose(load_forest(str(tmp_path / "a3.txt")), a3)
    with pytest.raises(ValueError):
        load_points(str(tmp_path / "a3.npy"))                                # the scorer still wants N x 4
    np.save(tmp_path / "bad.npy", np.zeros((4, 5)))
    with pytest.raises(ValueError, match="N x 3 or N x 4"):
        load_forest(str(tmp_path / "bad.npy"))


def test_save_results_layout_without_gpu(tmp_path):
    """npz / npy / txt writers and the reference's directory layout (the tree sort runs on the host when no GPU is present)."""
    from treelearn_amd.util.segment import save_results
    rng = np.random.default_rng(0)
    coords = rng.normal(size=(50, 3)) + 1000.0
    labels = np.repeat([0, 1, 2, 3, 0], 10)
    res = dict(coords=coords, labels=labels, categories=np.array([0, 1, 2]))
    save_results(res, str(tmp_path), "plot", ["npz", "txt"])
    z = np.load(tmp_path / "full_forest" / "plot.npz")
    assert np.array_equal(z["points"], coords) and np.array_equal(z["labels"], labels)
    assert (tmp_path / "full_forest" / "plot.txt").exists()
    t = np.load(tmp_path / "individual_trees" / "trunk_base_inside" / "2.npz")
    assert np.allclose(t["points"], coords[20:30] - coords.mean(0)) and (t["labels"] == 2).all()
    nt = np.load(tmp_path / "individual_trees" / "non_trees.npz")
    assert np.array_equal(nt["points"], np.vstack([coords[:10], coords[40:]]) - coords.mean(0))
    assert sorted(os.listdir(tmp_path / "individual_trees" / "completely_inside")) == ["1.npz"]
    assert sorted(os.listdir(tmp_path / "individual_trees" / "trunk_base_outside")) == ["3.npz"]
