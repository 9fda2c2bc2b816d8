"""Terrain model of a segmented forest on the device: a raster of ground heights (DTM), the ground under any point, height above
ground per point, and -- through util.inventory -- tree height and DBH measured from the ground.

    python -m treelearn_amd.util.terrain --forest cloud.npy|npz|txt|las --out dtm.npz [--hag hag.npy] [--cell 0.5 ...]

The semantics are the project's own; tests/terrain_restatement.py states them in numpy float64.

Inputs.  coords [N, 3] in f32 or f64, with a row stride of 3 or 4 read in place, widened to f64 exactly.  Optional labels [N] in i64.
Ground candidates are the rows with label == 0 when labels are given, else all rows.  A non-finite coordinate sets a device flag and
the host raises ValueError, as tl_crown_keys does.  §10's exactness contract applies to every formula: f64, plain operators,
`#pragma clang fp contract(off)`, squared distances in predicates.

Parameters (DEFAULTS, checked by check_params, which touches no GPU): cell 0.5 m (> 0, finite), max_slope 1.0 (>= 0), step_tol 0.2 m
(>= 0), window 2 cells (integer >= 0), fill_radius 20 cells (integer >= 0).  An unknown name raises ValueError.

Grid.  The grid spans all rows, candidates or not, so that every row can be sampled.  ix0 = floor(xmin / c), nx = floor(xmax / c) -
ix0 + 1, and the same in y.  A row's cell is (floor(x / c) - ix0, floor(y / c) - iy0): floor, not truncation, the crown-cell rule of §16.
The cell centre is ((ix0 + i) + 0.5) * c.  The grid is row-major [ny, nx].  nx, ny <= 32768 and nx * ny <= 2^26, otherwise the host
raises ValueError naming the extent and the cell.  N = 0 gives an empty grid.

Step A, cell minima.  zmin[j, i] is the lowest candidate z of the cell, exactly.  A cell without a candidate is `empty`.

Step B, one-sided slope filter.  A single pass evaluated against the raw minima of step A; not iterative, so it does not depend on
order.  A cell p with a minimum is `rejected` when some other cell q with a minimum, within Chebyshev distance `window` of it, has
zmin[p] - zmin[q] > max_slope * d + step_tol, with d = c * sqrt(di^2 + dj^2) and di, dj the integer index differences.  The comparison
is strict: a difference exactly on the bound is kept.  The remaining cells with a minimum are `ground` and keep their minimum as value.
Known weakness: one return far below the ground rejects its neighbours instead of itself (the §15 filters are the remedy).

Step C, fill.  Every `empty` or `rejected` cell looks at the `ground` cells of steps A and B, never at filled ones, in windows of
Chebyshev radius rho = 1, 2, ..., fill_radius.  At the first rho whose window holds at least one `ground` cell its value is
sum(w z) / sum(w) over the `ground` cells of that window, taken in row-major order, with w = 1 / (di^2 + dj^2).  If no rho qualifies the
value is NaN and the cell keeps the state `empty` or `rejected`; otherwise its state becomes `filled`.

Outputs.  z f64[ny, nx]; state u8[ny, nx]: 0 empty-unfilled, 1 ground, 2 rejected-unfilled, 3 filled-from-empty, 4 filled-from-rejected;
n_candidates i32[ny, nx].

Sampling (ground_at(x, y)).  u = x / c - (ix0 + 0.5), i0 = floor(u), fx = u - i0; then i0 and i0 + 1 are clamped to [0, nx - 1]; the
same in y.  With all four corners finite: (g00 (1 - fx) + g10 fx) (1 - fy) + (g01 (1 - fx) + g11 fx) fy.  Otherwise the result is the
value of the cell that contains the point (indices clamped), NaN included.  height_above_ground = z - ground_at(x, y), in f64.

Per-tree columns (GROUND_COLUMNS), added to the inventory only when a terrain is handed in, after the existing 16 columns, which keep
their bits.  z_ground is ground_at the tree's x, y, the §16 position in the same frame; height_ag = z_top - z_ground; base_gap = z_low -
z_ground; dbh_ag, dbh_ag_x, dbh_ag_y, dbh_ag_n, dbh_ag_rmse follow exactly §16's slice, fit and NaN rules with z_ground in place of
z_low.  All of these are NaN when z_ground is NaN; dbh_ag_n is then 0.  The offset shift applies to z_ground, dbh_ag_x, dbh_ag_y.

csrc/tl_terrain.hip holds tl_dtm_min, tl_dtm_filter, tl_dtm_fill and tl_dtm_sample; the extent of the cloud is one torch aminmax.
Coordinates handed to Terrain.sample / height_above_ground are in the frame the terrain was built in; `offset` only un-centres what
to_host() returns.  There is no CPU fallback."""
import argparse
import sys
import time

import numpy as np

DEFAULTS = dict(cell=0.5, max_slope=1.0, step_tol=0.2, window=2, fill_radius=20)
GROUND_COLUMNS = ("z_ground", "height_ag", "base_gap", "dbh_ag", "dbh_ag_x", "dbh_ag_y", "dbh_ag_n", "dbh_ag_rmse")
STATES = ("empty", "ground", "rejected", "filled_from_empty", "filled_from_rejected")
MAX_SIDE, MAX_CELLS = 32768, 1 << 26
_NO_GPU = "treelearn_amd.util.terrain runs on the GPU (tl_dtm_min); there is no CPU fallback"

__all__ = ["terrain_model", "cloud_terrain", "write_terrain", "check_params", "Terrain", "DEFAULTS", "GROUND_COLUMNS"]


def check_params(cfg=None, **kw):
    """The five parameters as a dict of plain numbers (defaults filled in); ValueError for an unknown name, a cell that is not positive
    and finite, a negative or NaN slope or tolerance, a window or fill radius that is not an integer >= 0.  Touches no GPU."""
    p = dict(DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in DEFAULTS:
                raise ValueError(f"unknown terrain parameter {k!r}; expected one of {tuple(DEFAULTS)}")
            if v is not None:
                p[k] = v
    p["cell"] = float(p["cell"])
    if not (p["cell"] > 0 and np.isfinite(p["cell"])):
        raise ValueError(f"cell must be > 0 and finite, got {p['cell']!r}")
    for k in ("max_slope", "step_tol"):
        p[k] = float(p[k])
        if not (p[k] >= 0 and np.isfinite(p[k])):
            raise ValueError(f"{k} must be >= 0 and finite, got {p[k]!r}")
    for k in ("window", "fill_radius"):
        if isinstance(p[k], float) and not np.isfinite(p[k]) or int(p[k]) != p[k] or int(p[k]) < 0 or int(p[k]) > MAX_SIDE:
            raise ValueError(f"{k} must be an integer in 0 .. {MAX_SIDE}, got {p[k]!r}")
        p[k] = int(p[k])
    return p


def _device_coords(a, min_cols=3):
    """A host or device array as a device tensor the kernels read in place: f32 / f64 [N, min_cols..4], unit column stride."""
    import torch
    c = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
    if c.ndim != 2 or not (min_cols <= c.shape[1] <= 4):
        raise ValueError(f"coordinates must have shape [N, {min_cols}] .. [N, 4], got {tuple(c.shape)}")
    if c.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"coordinates must be float32 or float64, got {c.dtype}")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    c = c.to("cuda")
    if len(c) and (c.stride(1) != 1 or c.stride(0) < c.shape[1]):
        c = c.contiguous()
    return c


class Terrain:
    """The raster on the device: z f64[ny, nx], state u8[ny, nx], n_candidates i32[ny, nx]; cell (ix0 + i, iy0 + j) of edge `cell`."""

    def __init__(self, z, state, n_candidates, ix0, iy0, nx, ny, cell, offset=None):
        self.z, self.state, self.n_candidates = z, state, n_candidates
        self.ix0, self.iy0, self.nx, self.ny, self.cell, self.offset = int(ix0), int(iy0), int(nx), int(ny), float(cell), offset

    def _sample(self, pts, want_ground, want_hag):
        import torch
        from .. import _hip
        c = _device_coords(pts, 3 if want_hag else 2)
        n = len(c)
        ground = torch.empty(n, dtype=torch.float64, device=c.device) if want_ground else None
        hag = torch.empty(n, dtype=torch.float64, device=c.device) if want_hag else None
        if n:
            _hip.check(_hip.lib().tl_dtm_sample(_hip.ptr(c), int(c.dtype == torch.float64), c.stride(0), n, _hip.ptr(self.z), self.cell, self.ix0,
                                                self.iy0, self.nx, self.ny, _hip.ptr(ground), _hip.ptr(hag), _hip.stream()), "tl_dtm_sample")
        return ground, hag

    def sample(self, xy_or_coords):
        """Ground height f64[N] (device) under the rows of an [N, 2], [N, 3] or [N, 4] array (x, y first), in the terrain's frame."""
        return self._sample(xy_or_coords, True, False)[0]

    def height_above_ground(self, coords):
        """z - ground f64[N] (device) per row of an [N, 3] or [N, 4] array, in the terrain's frame."""
        return self._sample(coords, False, True)[1]

    def to_host(self):
        """dict of numpy arrays: x0, y0 (the lower corner of cell [0, 0]), cell, z, state, n_candidates -- un-centred by `offset`."""
        off = np.zeros(3) if self.offset is None else self.offset
        c = np.float64(self.cell)
        return dict(x0=np.float64(self.ix0) * c + off[0], y0=np.float64(self.iy0) * c + off[1], cell=c, z=self.z.cpu().numpy() + off[2],
                    state=self.state.cpu().numpy(), n_candidates=self.n_candidates.cpu().numpy())


def terrain_model(coords, labels=None, *, cell=0.5, max_slope=1.0, step_tol=0.2, window=2, fill_radius=20, offset=None, stages=None):
    """coords [N, 3] float32 or float64 (a row stride of 3 or 4 elements is read in place), labels [N] integers or None; numpy arrays or
    tensors, on the host or the device.  Returns a Terrain.  `offset` (3 values) is kept for to_host(), the un-centring of
    segment_forest.  `stages`: a list that receives (name, seconds) per stage, each closed by a device synchronise (tools/dev_terrain.py)."""
    p = check_params(cell=cell, max_slope=max_slope, step_tol=step_tol, window=window, fill_radius=fill_radius)
    from .inventory import _offset
    off = _offset(offset)
    import torch
    from .. import _hip
    c = _device_coords(coords)
    n, dev = len(c), c.device
    lab = None
    if labels is not None:
        lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)).astype(np.int64, copy=False))
        lab = lab.reshape(-1)
        if lab.shape[0] != n:
            raise ValueError(f"mismatched lengths: {n} coordinates for {lab.shape[0]} labels")
        lab = lab.to(dev, torch.int64).contiguous()
    L = _hip.lib()
    t0 = [time.perf_counter()]

    def mark(name):
        if stages is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            stages.append((name, now - t0[0]))
            t0[0] = now

    cw = np.float64(p["cell"])
    if n:
        lo, hi = torch.aminmax(c[:, :2], dim=0)                                      # exact in the input's own format; NaN propagates
        ext = torch.stack([lo, hi]).to(torch.float64).cpu().numpy()
        if not np.isfinite(ext).all():
            raise ValueError("a coordinate is not finite")
        ix0, iy0 = (int(v) for v in np.floor(ext[0] / cw))
        nx, ny = (int(v) for v in np.floor(ext[1] / cw) - np.floor(ext[0] / cw) + 1)
        if nx > MAX_SIDE or ny > MAX_SIDE or nx * ny > MAX_CELLS:
            raise ValueError(f"the cloud spans {ext[1][0] - ext[0][0]:.6g} x {ext[1][1] - ext[0][1]:.6g} m: {nx} x {ny} cells of {p['cell']} m, "
                             f"beyond {MAX_SIDE} cells a side or {MAX_CELLS} cells in all; use a larger cell")
    else:
        ix0 = iy0 = nx = ny = 0
    mark("extent")

    keys = torch.empty((ny, nx), dtype=torch.int64, device=dev)
    count = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    zmin = torch.empty((ny, nx), dtype=torch.float64, device=dev)
    state0 = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
    z = torch.empty((ny, nx), dtype=torch.float64, device=dev)
    state = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
    if n:
        _hip.check(L.tl_dtm_min(_hip.ptr(c), int(c.dtype == torch.float64), c.stride(0), n, _hip.ptr(lab), p["cell"], ix0, iy0, nx, ny,
                                _hip.ptr(keys), _hip.ptr(count), _hip.ptr(err), _hip.stream()), "tl_dtm_min")
    mark("min")
    if n:
        _hip.check(L.tl_dtm_filter(_hip.ptr(keys), nx, ny, p["cell"], p["max_slope"], p["step_tol"], p["window"], _hip.ptr(zmin), _hip.ptr(state0),
                                   _hip.stream()), "tl_dtm_filter")
    mark("filter")
    if n:
        _hip.check(L.tl_dtm_fill(_hip.ptr(zmin), _hip.ptr(state0), nx, ny, p["fill_radius"], _hip.ptr(z), _hip.ptr(state), _hip.stream()),
                   "tl_dtm_fill")
    mark("fill")
    if n and int(err.item()):
        raise ValueError("a coordinate is not finite")
    return Terrain(z, state, count, ix0, iy0, nx, ny, p["cell"], off)


def cloud_terrain(points, **params):
    """The terrain of an N x 3 or N x 4 cloud (x y z [label]), as the command line computes it: the coordinates are centred on their
    float64 mean on the device, as cloud_inventory does, and the mean is kept as the terrain's `offset`.  Returns (terrain, centred
    coordinates on the device), so that the caller can sample its rows in the terrain's frame."""
    import torch
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if pts.ndim != 2 or pts.shape[1] not in (3, 4):
        raise ValueError(f"expected an N x 3 or N x 4 cloud (x y z [label]), got {tuple(pts.shape)}")
    check_params(**params)
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    pts = pts.to("cuda")
    xyz = pts[:, :3].to(torch.float64)
    lab = pts[:, 3].to(torch.int64) if pts.shape[1] == 4 else None
    if len(xyz) == 0:
        return terrain_model(xyz, lab, **params), xyz
    mean = xyz.mean(0)
    centred = xyz - mean
    return terrain_model(centred, lab, offset=mean, **params), centred


def write_terrain(path, terrain):
    """.npz with the keys of Terrain.to_host() (a dict of those arrays is taken as it is)."""
    d = terrain if isinstance(terrain, dict) else terrain.to_host()
    with open(path, "wb") as f:
        np.savez(f, **d)
    return path


def add_arguments(ap):
    """The five parameters as command-line options (shared with util.segment and util.inventory)."""
    ap.add_argument("--cell", type=float, default=DEFAULTS["cell"], help="edge of the terrain cells, metres")
    ap.add_argument("--max-slope", type=float, default=DEFAULTS["max_slope"], help="steepest ground the slope filter keeps, rise over run")
    ap.add_argument("--step-tol", type=float, default=DEFAULTS["step_tol"], help="height difference the slope filter always allows, metres")
    ap.add_argument("--window", type=int, default=DEFAULTS["window"], help="reach of the slope filter, cells")
    ap.add_argument("--fill-radius", type=int, default=DEFAULTS["fill_radius"], help="farthest ground cell a cell without ground is filled from, cells")


def params_of(a):
    return {k: getattr(a, k) for k in DEFAULTS}


def main(argv=None):
    import os
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.terrain", description="terrain model (DTM) and height above ground of a cloud")
    ap.add_argument("--forest", required=True, help="cloud: .npy / .npz / .txt / .las, N x 3 (x y z) or N x 4 (x y z label; label 0 = ground candidates)")
    ap.add_argument("--out", required=True, help=".npz to write: x0, y0, cell, z, state, n_candidates")
    ap.add_argument("--hag", default=None, help=".npy to write: N x 4, x y z height_above_ground in the input's frame")
    add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        params = check_params(params_of(a))
    except ValueError as e:
        ap.error(str(e))
    if not os.path.exists(a.forest):
        ap.error(f"--forest {a.forest}: no such file")
    from .segment import load_forest
    data = load_forest(a.forest)
    if data.ndim != 2 or data.shape[1] not in (3, 4):
        ap.error(f"--forest {a.forest}: expected N x 3 or N x 4 (x y z [label]), got {data.shape}")
    terrain, centred = cloud_terrain(data, **params)
    host = terrain.to_host()
    write_terrain(a.out, host)
    if a.hag:
        hag = terrain.height_above_ground(centred).cpu().numpy()
        np.save(a.hag, np.column_stack([np.asarray(data[:, :3], np.float64), hag]))
    counts = np.bincount(host["state"].reshape(-1), minlength=5)
    print(f"{a.forest}: {len(data)} points, {terrain.nx} x {terrain.ny} cells of {terrain.cell} m: {counts[1]} ground, {counts[3] + counts[4]} filled, "
          f"{counts[0] + counts[2]} without a value -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
