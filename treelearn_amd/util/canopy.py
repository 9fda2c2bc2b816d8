"""Canopy height model of a cloud on the device: the per-area side of the measurements.  A raster of the highest height
above ground per cell (CHM) with pits and holes mended, tree tops on it -- a tree count that does not depend on the segmentation --,
height percentiles, canopy cover and a vertical profile per cell of a coarser metrics grid, and a stand table.

    python -m treelearn_amd.util.canopy --forest cloud.npy|npz|txt|las --out canopy.npz [--stand stand.json] [--canopy-cell 0.5 ...]

The semantics are the project's own; tests/canopy_restatement.py states them in numpy float64.

Inputs.  coords [N, 3] in f32 or f64, with a row stride of 3 or 4 read in place, widened to f64 exactly.  h f64[N]: the height above
ground of every row, from Terrain.height_above_ground(coords) or handed in ready.  Optional labels [N] in i64.  A row whose h is NaN
(the terrain has no value under it) takes part in nothing and is counted in n_no_ground.  A non-finite x or y, or an infinite h, raises
ValueError("... not finite").  -0.0 counts as 0.0.  §10's exactness contract applies to every formula: f64, plain operators,
`#pragma clang fp contract(off)`.

Parameters (DEFAULTS, checked by check_params, which touches no GPU): cell 0.5 m (> 0, finite), pit_depth 2.0 m (>= 0, finite),
pit_min_neighbours 5 (integer 1..9; 9 can never be met and turns step B off), top_window 4 cells (integer >= 1), top_min_height 5.0 m
(finite), metric_cell 10.0 m (> 0, finite), cutoff 2.0 m (finite), percentiles (25, 50, 75, 95, 99) (1..16 values in [0, 100]), layer
1.0 m (> 0, finite), max_layers 64 (integer 1..256).  An unknown name raises ValueError.

Grids.  Two grids, each by the terrain's rule over all rows: ix0 = floor(xmin / c), nx = floor(xmax / c) - ix0 + 1, the same in y; a
row's cell is (floor(x / c) - ix0, floor(y / c) - iy0); the cell centre is ((ix0 + i) + 0.5) * c; arrays are row-major [ny, nx]; nx, ny <=
32768 and nx * ny <= 2^26, otherwise ValueError naming the extent and the cell before anything is allocated.  The CHM grid has c = cell,
the metrics grid c = metric_cell.  N = 0 gives empty grids.

Step A, tl_chm_max.  top[j, i] is the highest h of the cell, exactly; n[j, i] i32 its rows with a finite h; a cell without one is empty,
top NaN.  With labels, tl_chm_owner writes owner[j, i] i32: the largest label among the rows whose h equals the cell's maximum (label 0
can own a cell; labels below 0 never do).  Without labels, or in an empty cell, owner is -1.

Step B, tl_chm_pits.  One pass against the raw top.  v = the non-empty values among the cell's 8 neighbours inside the grid, k their
number, m their median: sorted ascending, the middle value for odd k, (v[k/2 - 1] + v[k/2]) / 2 for even k.  A non-empty cell with k >=
pit_min_neighbours and m - top > pit_depth (strict): chm = m, state 2.  Any other non-empty cell: chm = top, state 1.  An empty cell with
k >= pit_min_neighbours: chm = m, state 3.  Any other empty cell: chm NaN, state 0.  owner is not changed.

Step C, tl_chm_tops.  A cell is a top when chm is finite and >= top_min_height, no cell within Chebyshev distance top_window (clipped to
the grid) has a greater chm, and none of them with an equal chm has a smaller row-major index: a plateau gives one top.  tops_mask u8;
the tops in row-major order with i, j, x, y (cell centre), h, owner.  With labels, tops_per_tree i32[T] (T = max label): tops per owner
in 1..T.

Step D, tl_canopy_keys, two sorts, tl_grid_metrics.  Rows sorted by h, then stably by metrics cell: every cell is a contiguous range of
ascending heights.  Per cell: metric_n i32 rows; metric_n_veg i32 rows with h > cutoff (strict); cover = n_veg / n (NaN for n = 0);
h_max; h_mean and h_sd of the vegetation rows (population sd, two passes; NaN for n_veg = 0); per percentile q of the m vegetation
rows v: pos = (q / 100.0) * (m - 1), lo = floor(pos), t = pos - lo, v[lo] + (v[min(lo + 1, m - 1)] - v[lo]) * t; layers i32[ny, nx, L], L =
min(max_layers, floor(max finite h / layer) + 1), at least 1: a row with h < 0 counts in layer 0, any other in layer min(floor(h / layer),
L - 1); n_clipped: rows at or above L * layer.  Sums run in a fixed order over the sorted values, so every output has the same bits for
any row order.

stand_summary: area_ha (CHM cells with rows), canopy_cover (cells with chm > cutoff over cells with a finite chm), chm_mean, chm_max,
n_tops; with an inventory n_trees, stems_per_ha, n_dbh, basal_area_m2_per_ha, qmd, lorey_height and the trees with one, no, several tops.

csrc/tl_canopy.hip holds the six kernels; the extents are torch aminmax, the sorts torch.sort.  Coordinates are in the frame the terrain
was built in; `offset` only un-centres what to_host() returns (x0, y0, metric_x0, metric_y0, tops_x, tops_y; heights are relative and
stay).  There is no CPU fallback."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

DEFAULTS = dict(cell=0.5, pit_depth=2.0, pit_min_neighbours=5, top_window=4, top_min_height=5.0, metric_cell=10.0, cutoff=2.0,
                percentiles=(25, 50, 75, 95, 99), layer=1.0, max_layers=64)
STATES = ("empty", "top", "pit_filled", "hole_filled")
MAX_SIDE, MAX_CELLS = 32768, 1 << 26
_NO_GPU = "treelearn_amd.util.canopy runs on the GPU (tl_chm_max); there is no CPU fallback"
_HELP = dict(cell="edge of the CHM cells, metres", pit_depth="a cell this far below the median of its neighbours is a pit, metres",
             pit_min_neighbours="neighbours with a value a cell needs to be mended (1..9; 9 turns the step off)",
             top_window="reach of the tree-top window, cells", top_min_height="lowest CHM value that can be a tree top, metres",
             metric_cell="edge of the metrics cells, metres", cutoff="rows above this height are vegetation, metres",
             percentiles="height percentiles of the vegetation rows per metrics cell (1..16 values in 0..100)",
             layer="thickness of the layers of the vertical profile, metres", max_layers="most layers of the vertical profile (1..256)")

__all__ = ["canopy_model", "cloud_canopy", "stand_summary", "write_canopy", "write_stand", "check_params", "Canopy", "DEFAULTS"]


def _integer(name, v, lo, hi):
    if isinstance(v, bool) or isinstance(v, float) and not np.isfinite(v) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def check_params(cfg=None, **kw):
    """The ten parameters as a dict of plain numbers (defaults filled in, percentiles a tuple of floats); ValueError for an unknown name
    or a value outside its range (the table of DESIGN §22).  Touches no GPU."""
    p = dict(DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in DEFAULTS:
                raise ValueError(f"unknown canopy parameter {k!r}; expected one of {tuple(DEFAULTS)}")
            if v is not None:
                p[k] = v
    for k in ("cell", "metric_cell", "layer"):
        p[k] = float(p[k])
        if not (p[k] > 0 and np.isfinite(p[k])):
            raise ValueError(f"{k} must be > 0 and finite, got {p[k]!r}")
    p["pit_depth"] = float(p["pit_depth"])
    if not (p["pit_depth"] >= 0 and np.isfinite(p["pit_depth"])):
        raise ValueError(f"pit_depth must be >= 0 and finite, got {p['pit_depth']!r}")
    for k in ("top_min_height", "cutoff"):
        p[k] = float(p[k])
        if not np.isfinite(p[k]):
            raise ValueError(f"{k} must be finite, got {p[k]!r}")
    p["pit_min_neighbours"] = _integer("pit_min_neighbours", p["pit_min_neighbours"], 1, 9)
    p["top_window"] = _integer("top_window", p["top_window"], 1, MAX_SIDE)
    p["max_layers"] = _integer("max_layers", p["max_layers"], 1, 256)
    try:
        q = tuple(float(v) for v in (p["percentiles"] if np.ndim(p["percentiles"]) else (p["percentiles"],)))
    except (TypeError, ValueError):
        raise ValueError(f"percentiles must be 1 .. 16 numbers in [0, 100], got {p['percentiles']!r}") from None
    if not 1 <= len(q) <= 16 or not all(0.0 <= v <= 100.0 for v in q):
        raise ValueError(f"percentiles must be 1 .. 16 numbers in [0, 100], got {p['percentiles']!r}")
    p["percentiles"] = q
    return p


def _grid(ext, c, what):
    """ix0, iy0, nx, ny of the grid of edge c over the extent [[xmin, ymin], [xmax, ymax]] (f64), or ValueError beyond the limits."""
    cw = np.float64(c)
    ix0, iy0 = (int(v) for v in np.floor(ext[0] / cw))
    nx, ny = (int(v) for v in np.floor(ext[1] / cw) - np.floor(ext[0] / cw) + 1)
    if nx > MAX_SIDE or ny > MAX_SIDE or nx * ny > MAX_CELLS:
        raise ValueError(f"the cloud spans {ext[1][0] - ext[0][0]:.6g} x {ext[1][1] - ext[0][1]:.6g} m: {nx} x {ny} {what} cells of {c} m, "
                         f"beyond {MAX_SIDE} cells a side or {MAX_CELLS} cells in all; use a larger cell")
    return ix0, iy0, nx, ny


class Canopy:
    """The rasters on the device.  CHM grid [ny, nx] of edge `cell` at (ix0, iy0): n i32, top f64, owner i32, chm f64, state u8 (index
    into STATES), tops_mask u8; tops: dict of i, j (i64), x, y, h (f64), owner (i32) per top in row-major order; tops_per_tree i32[T] or
    None.  Metrics grid [metric_ny, metric_nx] of edge `metric_cell` at (metric_ix0, metric_iy0): metric_n, metric_n_veg i32, cover,
    h_max, h_mean, h_sd f64, percentiles f64[.., .., P], layers i32[.., .., L].  n_no_ground, n_clipped: ints.  params: the checked
    parameters."""
    GRID_KEYS = ("n", "top", "owner", "chm", "state", "tops_mask")
    METRIC_KEYS = ("metric_n", "metric_n_veg", "cover", "h_max", "h_mean", "h_sd", "percentiles", "layers")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to_host(self):
        """dict of numpy arrays: x0, y0 (the lower corner of cell [0, 0]), cell, GRID_KEYS, tops_i, tops_j, tops_x, tops_y, tops_h,
        tops_owner, tops_per_tree (with labels), metric_x0, metric_y0, metric_cell, METRIC_KEYS, percentile_q, layer, cutoff,
        n_no_ground, n_clipped -- x and y un-centred by `offset`."""
        off = np.zeros(3) if self.offset is None else self.offset
        c, mc = np.float64(self.cell), np.float64(self.metric_cell)
        d = dict(x0=np.float64(self.ix0) * c + off[0], y0=np.float64(self.iy0) * c + off[1], cell=c)
        d.update({k: getattr(self, k).cpu().numpy() for k in self.GRID_KEYS})
        d.update({"tops_" + k: v.cpu().numpy() for k, v in self.tops.items()})
        d["tops_x"], d["tops_y"] = d["tops_x"] + off[0], d["tops_y"] + off[1]
        if self.tops_per_tree is not None:
            d["tops_per_tree"] = self.tops_per_tree.cpu().numpy()
        d.update(metric_x0=np.float64(self.metric_ix0) * mc + off[0], metric_y0=np.float64(self.metric_iy0) * mc + off[1], metric_cell=mc)
        d.update({k: getattr(self, k).cpu().numpy() for k in self.METRIC_KEYS})
        d.update(percentile_q=np.asarray(self.params["percentiles"], np.float64), layer=np.float64(self.params["layer"]),
                 cutoff=np.float64(self.params["cutoff"]), n_no_ground=np.int64(self.n_no_ground), n_clipped=np.int64(self.n_clipped))
        return d


def canopy_model(coords, terrain=None, labels=None, *, height_above_ground=None, offset=None, stages=None, **params):
    """coords [N, 3] float32 or float64 (a row stride of 3 or 4 elements is read in place), labels [N] integers or None; numpy arrays or
    tensors, on the host or the device.  The heights come from `terrain` (a util.terrain.Terrain in the frame of coords) or from
    `height_above_ground` (f64 [N], as Terrain.height_above_ground gives it); one of the two is required.  Returns a Canopy.  `offset` (3
    values) is kept for to_host().  `stages`: a list that receives (name, seconds) per stage, each closed by a device synchronise
    (tools/dev_canopy.py)."""
    p = check_params(**params)
    if (terrain is None) == (height_above_ground is None):
        raise ValueError("canopy_model takes a terrain or a height_above_ground, one of the two")
    from .inventory import _offset
    from .terrain import _device_coords
    off = _offset(offset)
    import torch
    from .. import _hip
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    c = _device_coords(coords)
    n, dev = len(c), c.device
    lab = None
    if labels is not None:
        lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)).astype(np.int64, copy=False))
        lab = lab.reshape(-1)
        if lab.shape[0] != n:
            raise ValueError(f"mismatched lengths: {n} coordinates for {lab.shape[0]} labels")
        lab = lab.to(dev, torch.int64).contiguous()
    lib = _hip.lib()
    t0 = [time.perf_counter()]

    def mark(name):
        if stages is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            stages.append((name, now - t0[0]))
            t0[0] = now

    if height_above_ground is None:
        h = terrain.height_above_ground(c)
    else:
        h = height_above_ground if torch.is_tensor(height_above_ground) else torch.from_numpy(np.asarray(height_above_ground, np.float64))
        h = h.reshape(-1)
        if h.shape[0] != n:
            raise ValueError(f"mismatched lengths: {n} coordinates for {h.shape[0]} heights")
        h = h.to(dev, torch.float64).contiguous()
    mark("hag")

    L = 1
    if n:
        lo, hi = torch.aminmax(c[:, :2], dim=0)                                      # exact in the input's own format; NaN propagates
        known = h[~torch.isnan(h)]
        hlo, hhi = (float(v) for v in torch.aminmax(known)) if len(known) else (0.0, 0.0)
        ext = torch.stack([lo, hi]).to(torch.float64).cpu().numpy()
        if not np.isfinite(ext).all():
            raise ValueError("a coordinate is not finite")
        if not (np.isfinite(hlo) and np.isfinite(hhi)):
            raise ValueError("a height above ground is not finite")
        ix0, iy0, nx, ny = _grid(ext, p["cell"], "CHM")
        mx0, my0, mnx, mny = _grid(ext, p["metric_cell"], "metrics")
        if len(known):
            L = int(max(1.0, min(float(p["max_layers"]), float(np.floor(np.float64(hhi) / np.float64(p["layer"])) + 1.0))))
    else:
        ix0 = iy0 = nx = ny = mx0 = my0 = mnx = mny = 0
    mark("extent")

    f64 = int(c.dtype == torch.float64)
    ld = c.stride(0) if n else 3
    cells, mcells, P = nx * ny, mnx * mny, len(p["percentiles"])
    keys = torch.empty((ny, nx), dtype=torch.int64, device=dev)
    count = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    owner = torch.full((ny, nx), -1, dtype=torch.int32, device=dev)
    top = torch.empty((ny, nx), dtype=torch.float64, device=dev)
    chm = torch.empty((ny, nx), dtype=torch.float64, device=dev)
    state = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
    mask = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
    if n:
        _hip.check(lib.tl_chm_max(_hip.ptr(c), f64, ld, n, _hip.ptr(h), p["cell"], ix0, iy0, nx, ny, _hip.ptr(keys), _hip.ptr(count), _hip.ptr(flags),
                                  _hip.stream()), "tl_chm_max")
    mark("maxima")
    if n and lab is not None:
        _hip.check(lib.tl_chm_owner(_hip.ptr(c), f64, ld, n, _hip.ptr(h), _hip.ptr(lab), p["cell"], ix0, iy0, nx, ny, _hip.ptr(keys), _hip.ptr(owner),
                                    _hip.ptr(flags), _hip.stream()), "tl_chm_owner")
    mark("owners")
    if cells:
        _hip.check(lib.tl_chm_pits(_hip.ptr(keys), nx, ny, p["pit_depth"], p["pit_min_neighbours"], _hip.ptr(top), _hip.ptr(chm), _hip.ptr(state),
                                   _hip.stream()), "tl_chm_pits")
    mark("pits")
    if cells:
        _hip.check(lib.tl_chm_tops(_hip.ptr(chm), nx, ny, p["top_window"], p["top_min_height"], _hip.ptr(mask), _hip.stream()), "tl_chm_tops")
    at = torch.nonzero(mask)                                                         # row-major order
    tj, ti = at[:, 0], at[:, 1]
    cw = np.float64(p["cell"])
    tops = dict(i=ti, j=tj, x=((ix0 + ti).to(torch.float64) + 0.5) * cw, y=((iy0 + tj).to(torch.float64) + 0.5) * cw, h=chm[tj, ti], owner=owner[tj, ti])
    per_tree = None
    if lab is not None:
        T = max(int(lab.max()), 0) if n else 0
        own = tops["owner"].to(torch.int64)
        own = own[(own >= 1) & (own <= T)]
        per_tree = torch.bincount(own, minlength=T + 1)[1:].to(torch.int32)
    mark("tops")

    mkeys = torch.empty(n, dtype=torch.int64, device=dev)
    if n:
        _hip.check(lib.tl_canopy_keys(_hip.ptr(c), f64, ld, n, _hip.ptr(h), p["metric_cell"], mx0, my0, mnx, mny, _hip.ptr(mkeys), _hip.ptr(flags),
                                      _hip.stream()), "tl_canopy_keys")
    mark("keys")
    hs, order = torch.sort(h)                                                        # NaN last; their key -1 puts them first below
    skeys, order2 = torch.sort(mkeys.index_select(0, order), stable=True)
    hs = hs.index_select(0, order2).contiguous()
    start = torch.searchsorted(skeys, torch.arange(mcells + 1, dtype=torch.int64, device=dev)).contiguous()
    if not n:
        hs = torch.zeros(1, dtype=torch.float64, device=dev)                         # (a pointer to pass; no height is read)
    mark("sorts")
    metrics = torch.empty((mny, mnx, 4 + P), dtype=torch.float64, device=dev)
    counts = torch.empty((mny, mnx, 2), dtype=torch.int32, device=dev)
    layers = torch.empty((mny, mnx, L), dtype=torch.int32, device=dev)
    n_clipped = torch.zeros(1, dtype=torch.int32, device=dev)
    if mcells:
        q = (ctypes.c_double * P)(*p["percentiles"])
        _hip.check(lib.tl_grid_metrics(_hip.ptr(hs), n, _hip.ptr(start), mcells, p["cutoff"], q, P, p["layer"], L, _hip.ptr(metrics), _hip.ptr(counts),
                                       _hip.ptr(layers), _hip.ptr(n_clipped), _hip.stream()), "tl_grid_metrics")
    mark("metrics")
    fl = flags.cpu().numpy()
    if n and int(fl[0]):
        raise ValueError("a coordinate or a height above ground is not finite, or a label is beyond 32 bits")
    return Canopy(n=count, top=top, owner=owner, chm=chm, state=state, tops_mask=mask, tops=tops, tops_per_tree=per_tree,
                  metric_n=counts[:, :, 0].contiguous(), metric_n_veg=counts[:, :, 1].contiguous(), cover=metrics[:, :, 0].contiguous(),
                  h_max=metrics[:, :, 1].contiguous(), h_mean=metrics[:, :, 2].contiguous(), h_sd=metrics[:, :, 3].contiguous(),
                  percentiles=metrics[:, :, 4:].contiguous(), layers=layers, n_no_ground=int(fl[1]), n_clipped=int(n_clipped.item()),
                  ix0=ix0, iy0=iy0, nx=nx, ny=ny, cell=p["cell"], metric_ix0=mx0, metric_iy0=my0, metric_nx=mnx, metric_ny=mny,
                  metric_cell=p["metric_cell"], params=p, offset=off)


def cloud_canopy(points, terrain_cfg=None, **params):
    """The canopy of an N x 3 or N x 4 cloud (x y z [label]), as the command line computes it: util.terrain.cloud_terrain centres the
    coordinates on their float64 mean and builds the terrain (of the label-0 rows when there are labels; parameters in terrain_cfg), the
    canopy is taken in that frame with the mean as `offset`.  Returns (canopy, terrain)."""
    import torch
    from .terrain import check_params as check_terrain, cloud_terrain
    p = check_params(**params)
    terrain_cfg = check_terrain(terrain_cfg)
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if pts.ndim != 2 or pts.shape[1] not in (3, 4):
        raise ValueError(f"expected an N x 3 or N x 4 cloud (x y z [label]), got {tuple(pts.shape)}")
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    pts = pts.to("cuda")
    terrain, centred = cloud_terrain(pts, **terrain_cfg)
    lab = pts[:, 3].to(torch.int64) if pts.shape[1] == 4 else None
    return canopy_model(centred, terrain, lab, offset=terrain.offset, **p), terrain


def _nan_div(a, b):
    return float(a) / float(b) if b else float("nan")


def stand_summary(canopy, inventory=None):
    """The stand table as a dict of plain numbers, computed on the host from the small arrays.  canopy: a Canopy or its to_host() dict;
    inventory: the dict of util.inventory.tree_inventory, or None.  Empty denominators give NaN."""
    d = canopy if isinstance(canopy, dict) else canopy.to_host()
    cell, chm = float(d["cell"]), np.asarray(d["chm"], np.float64)
    area_ha = float(int((np.asarray(d["n"]) > 0).sum()) * (cell * cell) / 1e4)
    known = chm[np.isfinite(chm)]
    out = dict(area_ha=area_ha, canopy_cover=_nan_div(int((known > float(d["cutoff"])).sum()), len(known)),
               chm_mean=float(known.mean()) if len(known) else float("nan"), chm_max=float(known.max()) if len(known) else float("nan"),
               n_tops=int(len(d["tops_h"])))
    if inventory is None:
        return out
    dbh = np.asarray(inventory["dbh_ag" if "dbh_ag" in inventory else "dbh"], np.float64)
    height = np.asarray(inventory["height_ag" if "height_ag" in inventory else "height"], np.float64)
    n_trees = int((np.asarray(inventory["n_points"]) > 0).sum())
    ok = np.isfinite(dbh)
    g = (np.pi / 4.0) * dbh[ok] * dbh[ok]                                             # basal area per tree, m^2
    both = ok & np.isfinite(height)
    gh = (np.pi / 4.0) * dbh[both] * dbh[both]
    out.update(n_trees=n_trees, stems_per_ha=_nan_div(n_trees, area_ha), n_dbh=int(ok.sum()), basal_area_m2_per_ha=_nan_div(g.sum(), area_ha),
               qmd=float(np.sqrt((dbh[ok] * dbh[ok]).mean())) if ok.any() else float("nan"),
               lorey_height=_nan_div((gh * height[both]).sum(), gh.sum()))
    if d.get("tops_per_tree") is not None:
        per = np.asarray(d["tops_per_tree"])
        out.update(trees_with_one_top=int((per == 1).sum()), trees_without_top=int((per == 0).sum()), trees_with_several_tops=int((per > 1).sum()))
    return out


def write_canopy(path, canopy):
    """.npz with the keys of Canopy.to_host() (a dict of those arrays is taken as it is)."""
    d = canopy if isinstance(canopy, dict) else canopy.to_host()
    with open(path, "wb") as f:
        np.savez(f, **d)
    return path


def write_stand(path, summary):
    """.json of a stand_summary (NaN is written as null)."""
    clean = {k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in summary.items()}
    with open(path, "w") as f:
        json.dump(clean, f, indent=1)
        f.write("\n")
    return path


def add_arguments(ap):
    """One --canopy-... option per parameter (shared with util.segment)."""
    for k, v in DEFAULTS.items():
        opt = "--canopy-" + k.replace("_", "-")
        if k == "percentiles":
            ap.add_argument(opt, type=float, nargs="+", default=list(v), help=_HELP[k])
        else:
            ap.add_argument(opt, type=int if isinstance(v, int) else float, default=v, help=_HELP[k])


def params_of(a):
    return {k: getattr(a, "canopy_" + k) for k in DEFAULTS}


def main(argv=None):
    import os
    from . import terrain as _terrain
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.canopy", description="canopy height model, tree tops, grid metrics and stand table of a cloud")
    ap.add_argument("--forest", required=True, help="cloud: .npy / .npz / .txt / .las, N x 3 (x y z) or N x 4 (x y z label; label 0 = ground candidates)")
    ap.add_argument("--out", required=True, help=".npz to write: the arrays of Canopy.to_host()")
    ap.add_argument("--stand", default=None, help=".json to write: the stand table (with the inventory's columns when the cloud is labelled)")
    add_arguments(ap)
    _terrain.add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        params = check_params(params_of(a))
        terrain_cfg = _terrain.check_params(_terrain.params_of(a))
    except ValueError as e:
        ap.error(str(e))
    if not os.path.exists(a.forest):
        ap.error(f"--forest {a.forest}: no such file")
    from .segment import load_forest
    try:
        data = load_forest(a.forest)
    except ValueError as e:
        ap.error(f"--forest {a.forest}: {e}")
    if data.ndim != 2 or data.shape[1] not in (3, 4):
        ap.error(f"--forest {a.forest}: expected N x 3 or N x 4 (x y z [label]), got {data.shape}")
    canopy, _ = cloud_canopy(data, terrain_cfg=terrain_cfg, **params)
    host = canopy.to_host()
    write_canopy(a.out, host)
    inv = None
    if a.stand:
        if data.shape[1] == 4:
            from .inventory import cloud_inventory
            inv = cloud_inventory(data, terrain=True, terrain_cfg=terrain_cfg)
        write_stand(a.stand, stand_summary(host, inv))
    print(f"{a.forest}: {len(data)} points, {canopy.nx} x {canopy.ny} cells of {canopy.cell} m, {len(host['tops_h'])} tree tops, "
          f"{canopy.metric_nx} x {canopy.metric_ny} metrics cells of {canopy.metric_cell} m, {canopy.n_no_ground} rows without ground -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
