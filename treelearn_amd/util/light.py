"""Light under the canopy on the device: how much sky a place in the stand still sees.  A bit grid of the occupied voxels
of the cloud, rays marched through it from sensors above the ground, from the top of every tree and from any position, and from their
exit counts the gap fraction per zenith ring, canopy openness, the effective leaf area index and the zenith gap -- the synthetic
counterpart of a hemispherical photograph.

    python -m treelearn_amd.util.light --forest cloud.npy|npz|txt|las --out light.npz [--light-voxel 0.25] [--sensor-cell 2]
                                       [--sensor-height 1.3] [--rings 9] [--azimuths 36] [--max-range 60] [--hemi x,y --hemi-out sky.png]

The semantics are the project's own; tests/light_restatement.py states them in numpy float64.  §10's exactness contract applies to every
formula of the kernels: f64, plain operators, `#pragma clang fp contract(off)`; the walk keeps no accumulated floating-point state.

Parameters (DEFAULTS, checked by check_params, which touches no GPU): voxel 0.25 m (> 0, finite), sensor_cell 2.0 m (> 0, finite),
sensor_height 1.3 m (finite), n_rings 9 (integer 1..256), n_azimuth 36 (integer 1..4096), max_zenith 90.0 degrees (in (0, 90]), max_range
60.0 m (> 0, finite), min_hits 1 (integer >= 1), lai_max_zenith 75.0 degrees (in (0, 90]), zenith_cone 30.0 degrees (in (0, 90]).  An
unknown name raises ValueError.

Voxel grid.  The terrain's rule in all three axes over all rows: ix0 = floor(xmin / v), nx = floor(xmax / v) - ix0 + 1, the same in y and
z; a row's voxel is (floor(x / v) - ix0, ...).  occ: one bit per voxel, u32 words along x, [nz, ny, ceil(nx / 32)]; with labels owner
i32[nz, ny, nx]: the largest label >= 0 among the voxel's rows, -1 when there is none.  Integer atomics: the same bits for any row order.
nx * ny * nz <= 2^31 without owner and <= 2^28 with it, each side <= 8192, otherwise ValueError naming the extent and the voxel before
anything is allocated.  A non-finite coordinate raises ValueError.

Direction table.  sky_directions(n_rings, n_azimuth, max_zenith): ray r * n_azimuth + a is the unit vector (sin t cos p, sin t sin p,
cos t) at zenith t = (r + 0.5) * max_zenith / n_rings and azimuth p = (a + 0.5) * 360 / n_azimuth -- the half steps keep the rays off the
axes --, in ring r, whose bounds are theta_lo = r * max_zenith / n_rings and theta_hi = (r + 1) * max_zenith / n_rings.  march takes any
table whose vectors are finite and of unit length to 1e-12 and whose rings lie in 0 .. R - 1; the host checks that.

The walk of origin o and direction d.  i_a = floor(o_a / v) - i0_a; an origin outside the grid has status 1, no counts and NaN results
(n_outside counts them).  s_a = sign of d_a; t_a = ((i0_a + i_a + (s_a > 0 ? 1 : 0)) * v - o_a) / d_a for s_a != 0 and +inf otherwise,
always from the integer index.  Repeat: the axis of the smallest t (ties to x, then y, then z), t_enter = t_a; t_enter > max_range: code
2; i_a += s_a; outside the grid: code 1 through the top, code 3 through a side or the bottom; recompute t_a; the voxel entered is a hit
when its bit is set and (skip < 0 or owner != skip); at min_hits hits: code 0, first = t_enter.  The origin's own voxel is never tested.
counts i32[P, R, 4] hold the rays of origin p and ring r per code (integer atomics); on request code u8[P, D] and first f64[P, D].

Derived on the host in f64 (derive): gap[r] = (n1 + n2) / (D_r - n3), NaN when every ray left through a side; edge_share = sum n3 / D;
openness = sum gap[r] w_r / sum w_r over the rings with a gap, w_r = cos theta_lo - cos theta_hi; lai_e = 2 * sum -ln(max(gap[r], 1 /
(2 D_r))) * cos theta_r * u_r over the rings with a gap and theta_r <= lai_max_zenith, theta_r the middle of the ring and u_r = sin
theta_r normalised to sum 1 over those rings; gap_zenith: the gap of the pooled counts of the rings with theta_hi <= zenith_cone.

Users.  The sensor grid: sensors at the centres ((sx0 + i) + 0.5) * sensor_cell of the cells over the xy extent, z = terrain.sample(x,
y) + sensor_height, skip -1; a sensor without ground or outside the grid is NaN.  Per tree (tree_light, LIGHT_COLUMNS): one origin per
(tree, x, y column) of the grid at the centre of the tree's highest voxel of the column, skip = the tree's label; the tree's counts are
the integer sum over its columns.  point_light: openness per row from the centres of the occupied voxels.  hemi_picture: size^2
directions in equidistant polar projection (zenith = max_zenith * radius, east to the right, north up), sky light, blocked pixels shaded
by `first`, rays lost through a side grey, outside the circle black.

csrc/tl_light.hip holds tl_light_voxels and tl_light_march; the extent is one torch aminmax and the tree columns' tops torch integer
plumbing (a key per (label, iy, ix), amax of iz).  Coordinates are in the frame the terrain was built in; `offset` only un-centres what
to_host() returns (x0, y0, z0, sensor_x0, sensor_y0).  There is no CPU fallback."""
import argparse
import sys
import time

import numpy as np

DEFAULTS = dict(voxel=0.25, sensor_cell=2.0, sensor_height=1.3, n_rings=9, n_azimuth=36, max_zenith=90.0, max_range=60.0, min_hits=1,
                lai_max_zenith=75.0, zenith_cone=30.0)
LIGHT_COLUMNS = ("light_columns", "light_openness", "light_gap_zenith", "light_lai_above", "light_edge_share")
LIGHT_INT_COLUMNS = ("light_columns",)
RASTER_KEYS = ("openness", "lai_e", "gap_zenith", "edge_share", "gap")
CODES = ("blocked", "open_top", "open_range", "side")
MAX_SIDE, MAX_VOXELS, MAX_OWNED = 8192, 1 << 31, 1 << 28
SKY_RGB, SIDE_RGB, OUTSIDE_RGB = (200, 225, 255), (110, 110, 110), (0, 0, 0)
_OPTIONS = dict(voxel="--light-voxel", sensor_cell="--sensor-cell", sensor_height="--sensor-height", n_rings="--rings", n_azimuth="--azimuths",
                max_zenith="--max-zenith", max_range="--max-range", min_hits="--light-min-hits", lai_max_zenith="--lai-max-zenith",
                zenith_cone="--zenith-cone")
_HELP = dict(voxel="edge of the light voxels, metres", sensor_cell="edge of the sensor cells, metres", sensor_height="height of the sensors above the ground, metres",
             n_rings="zenith rings of the sky table (1..256)", n_azimuth="azimuth steps of the sky table (1..4096)",
             max_zenith="largest zenith angle of the sky table, degrees", max_range="a ray that reaches this length is open, metres",
             min_hits="occupied voxels that block a ray", lai_max_zenith="rings up to this zenith angle enter lai_e, degrees",
             zenith_cone="rings up to this zenith angle enter gap_zenith, degrees")
_NO_GPU = "treelearn_amd.util.light runs on the GPU (tl_light_march); there is no CPU fallback"

__all__ = ["light_model", "cloud_light", "light_voxels", "march", "sky_directions", "hemi_directions", "derive", "tree_columns", "write_light", "check_params", "Light",
           "Voxels", "DEFAULTS", "LIGHT_COLUMNS"]


def _integer(name, v, lo, hi):
    if isinstance(v, bool) or isinstance(v, float) and not np.isfinite(v) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def check_params(cfg=None, **kw):
    """The ten parameters as a dict of plain numbers (defaults filled in); ValueError for an unknown name or a value outside its range.
    Touches no GPU."""
    p = dict(DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in DEFAULTS:
                raise ValueError(f"unknown light parameter {k!r}; expected one of {tuple(DEFAULTS)}")
            if v is not None:
                p[k] = v
    for k in ("voxel", "sensor_cell", "max_range"):
        p[k] = float(p[k])
        if not (p[k] > 0 and np.isfinite(p[k])):
            raise ValueError(f"{k} must be > 0 and finite, got {p[k]!r}")
    p["sensor_height"] = float(p["sensor_height"])
    if not np.isfinite(p["sensor_height"]):
        raise ValueError(f"sensor_height must be finite, got {p['sensor_height']!r}")
    for k in ("max_zenith", "lai_max_zenith", "zenith_cone"):
        p[k] = float(p[k])
        if not 0.0 < p[k] <= 90.0:
            raise ValueError(f"{k} must lie in (0, 90] degrees, got {p[k]!r}")
    p["n_rings"] = _integer("n_rings", p["n_rings"], 1, 256)
    p["n_azimuth"] = _integer("n_azimuth", p["n_azimuth"], 1, 4096)
    p["min_hits"] = _integer("min_hits", p["min_hits"], 1, 1 << 20)
    return p


def sky_directions(n_rings=9, n_azimuth=36, max_zenith=90.0):
    """(dirs f64[D, 3], ring i32[D], theta_lo f64[R], theta_hi f64[R]): D = n_rings * n_azimuth unit vectors, ring-major, at zenith (r +
    0.5) * max_zenith / n_rings and azimuth (a + 0.5) * 360 / n_azimuth; the ring of each; the rings' bounds in degrees."""
    n_rings, n_azimuth = _integer("n_rings", n_rings, 1, 256), _integer("n_azimuth", n_azimuth, 1, 4096)
    max_zenith = float(max_zenith)
    if not 0.0 < max_zenith <= 90.0:
        raise ValueError(f"max_zenith must lie in (0, 90] degrees, got {max_zenith!r}")
    r = np.arange(n_rings, dtype=np.float64)
    th = np.deg2rad((r + 0.5) * max_zenith / n_rings)
    ph = np.deg2rad((np.arange(n_azimuth, dtype=np.float64) + 0.5) * 360.0 / n_azimuth)
    dirs = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :],
                     np.broadcast_to(np.cos(th)[:, None], (n_rings, n_azimuth))], axis=2).reshape(-1, 3)
    ring = np.repeat(np.arange(n_rings, dtype=np.int32), n_azimuth)
    return np.ascontiguousarray(dirs), ring, r * max_zenith / n_rings, (r + 1.0) * max_zenith / n_rings


def hemi_directions(size, max_zenith=90.0):
    """The table of a hemispherical picture of size x size pixels in equidistant polar projection: (dirs f64[D, 3], inside bool[size,
    size]).  Pixel (row, col) sits at u = (col + 0.5) - size / 2 to the east and w = size / 2 - (row + 0.5) to the north; rho = sqrt(u^2 +
    w^2) / (size / 2); the pixels with rho < 1 are inside the circle and look at zenith max_zenith * rho and azimuth atan2(w, u), in
    row-major order."""
    size = _integer("size", size, 2, 2048)
    half = size / 2.0
    u = (np.arange(size, dtype=np.float64) + 0.5) - half
    uu, ww = np.meshgrid(u, -u)                                                       # image row 0 at the top
    rho = np.sqrt(uu * uu + ww * ww) / half
    inside = rho < 1.0
    th = np.deg2rad(float(max_zenith)) * rho[inside]
    ph = np.arctan2(ww[inside], uu[inside])
    dirs = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
    return np.ascontiguousarray(dirs / np.sqrt((dirs * dirs).sum(1))[:, None]), inside


def derive(counts, rays, theta_lo, theta_hi, lai_max_zenith=75.0, zenith_cone=30.0):
    """The derived quantities of counts [..., R, 4] (integers) with rays [..., R] or [R] rays per ring and the rings' bounds in degrees:
    dict of gap f64[..., R], openness, lai_e, gap_zenith, edge_share f64[...].  One fixed expression each, rings in ascending order."""
    c = np.asarray(counts).astype(np.int64)
    R = c.shape[-2]
    lead = c.shape[:-2]
    rays = np.broadcast_to(np.asarray(rays).astype(np.int64), lead + (R,))
    lo_deg, hi_deg = np.asarray(theta_lo, np.float64), np.asarray(theta_hi, np.float64)
    nan = np.float64("nan")
    known = rays - c[..., 3]
    is_open = c[..., 1] + c[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(known > 0, is_open.astype(np.float64) / known.astype(np.float64), nan)
        total = rays.sum(-1)
        edge = np.where(total > 0, c[..., 3].sum(-1).astype(np.float64) / total.astype(np.float64), nan)
        w = np.cos(np.deg2rad(lo_deg)) - np.cos(np.deg2rad(hi_deg))
        has = ~np.isnan(gap)
        num, den = np.zeros(lead), np.zeros(lead)
        for r in range(R):
            num = num + np.where(has[..., r], gap[..., r] * w[r], 0.0)
            den = den + np.where(has[..., r], w[r], 0.0)
        openness = np.where(den > 0, num / den, nan)
        mid = np.deg2rad((lo_deg + hi_deg) / 2.0)
        use = has & ((lo_deg + hi_deg) / 2.0 <= lai_max_zenith)
        usum = np.zeros(lead)
        for r in range(R):
            usum = usum + np.where(use[..., r], np.sin(mid[r]), 0.0)
        acc = np.zeros(lead)
        for r in range(R):
            g = np.maximum(np.where(use[..., r], gap[..., r], 1.0), 1.0 / (2.0 * rays[..., r].astype(np.float64)))
            acc = acc + np.where(use[..., r], -np.log(g) * np.cos(mid[r]) * (np.sin(mid[r]) / usum), 0.0)
        lai = np.where(usum > 0, 2.0 * acc, nan)
        cone = hi_deg <= zenith_cone
        known_c = known[..., cone].sum(-1)
        gz = np.where(known_c > 0, is_open[..., cone].sum(-1).astype(np.float64) / known_c.astype(np.float64), nan)
    return dict(gap=gap, openness=openness, lai_e=lai, gap_zenith=gz, edge_share=edge)


class Voxels:
    """The voxel grid on the device: occ u32[nz, ny, ceil(nx / 32)], owner i32[nz, ny, nx] or None; voxel (ix0 + i, iy0 + j, iz0 + k) of
    edge `voxel`."""

    def __init__(self, occ, owner, ix0, iy0, iz0, nx, ny, nz, voxel):
        self.occ, self.owner, self.voxel = occ, owner, float(voxel)
        self.ix0, self.iy0, self.iz0, self.nx, self.ny, self.nz = int(ix0), int(iy0), int(iz0), int(nx), int(ny), int(nz)

    def index(self, coords):
        """The voxel of every row of device coordinates, i64[N, 3] (ix, iy, iz): the kernels' rule in torch's f64."""
        import torch
        f = torch.floor(coords[:, :3].to(torch.float64) / self.voxel).to(torch.int64)
        return f - torch.tensor([self.ix0, self.iy0, self.iz0], dtype=torch.int64, device=coords.device)

    def centres(self, idx):
        """The centres f64[K, 3] of the voxels idx i64[K, 3]: ((i0 + i) + 0.5) * voxel."""
        import torch
        i0 = torch.tensor([self.ix0, self.iy0, self.iz0], dtype=torch.int64, device=idx.device)
        return (((i0 + idx).to(torch.float64) + 0.5) * self.voxel).contiguous()


def _labels(labels, n, dev):
    import torch
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)).astype(np.int64, copy=False))
    lab = lab.reshape(-1)
    if lab.shape[0] != n:
        raise ValueError(f"mismatched lengths: {n} coordinates for {lab.shape[0]} labels")
    return lab.to(dev, torch.int64).contiguous()


def light_voxels(coords, labels=None, voxel=0.25):
    """coords [N, 3] float32 or float64 (a row stride of 3 or 4 elements is read in place), labels [N] integers or None; numpy arrays or
    tensors, on the host or the device.  Returns the Voxels of the cloud (tl_light_voxels)."""
    voxel = check_params(voxel=voxel)["voxel"]
    import torch
    from .. import _hip
    from .terrain import _device_coords
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    c = _device_coords(coords)
    n, dev = len(c), c.device
    lab = None if labels is None else _labels(labels, n, dev)
    if n:
        lo, hi = torch.aminmax(c[:, :3], dim=0)                                      # exact in the input's own format; NaN propagates
        ext = torch.stack([lo, hi]).to(torch.float64).cpu().numpy()
        if not np.isfinite(ext).all():
            raise ValueError("a coordinate is not finite")
        v = np.float64(voxel)
        i0 = [int(k) for k in np.floor(ext[0] / v)]
        nn = [int(k) for k in np.floor(ext[1] / v) - np.floor(ext[0] / v) + 1]
        limit = MAX_VOXELS if lab is None else MAX_OWNED
        if max(nn) > MAX_SIDE or nn[0] * nn[1] * nn[2] > limit:
            span = ext[1] - ext[0]
            raise ValueError(f"the cloud spans {span[0]:.6g} x {span[1]:.6g} x {span[2]:.6g} m: {nn[0]} x {nn[1]} x {nn[2]} light voxels of {voxel} m, "
                             f"beyond {MAX_SIDE} voxels a side or {limit} voxels in all; use a larger voxel")
    else:
        i0, nn = [0, 0, 0], [0, 0, 0]
    nx, ny, nz = nn
    occ = torch.empty((nz, ny, (nx + 31) // 32), dtype=torch.int32, device=dev)
    owner = None if lab is None else torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if n:
        _hip.check(_hip.lib().tl_light_voxels(_hip.ptr(c), int(c.dtype == torch.float64), c.stride(0), n, _hip.ptr(lab), voxel, i0[0], i0[1], i0[2],
                                              nx, ny, nz, _hip.ptr(occ), _hip.ptr(owner), _hip.ptr(err), _hip.stream()), "tl_light_voxels")
        if int(err.item()):
            raise ValueError("a coordinate is not finite, or a label is beyond 32 bits")
    return Voxels(occ, owner, i0[0], i0[1], i0[2], nx, ny, nz, voxel)


def check_table(dirs, ring, n_rings):
    """The direction table as host arrays (f64[D, 3], i32[D]); ValueError unless every vector is finite and of unit length to 1e-12 and
    every ring lies in 0 .. n_rings - 1."""
    d = np.ascontiguousarray(np.asarray(dirs.cpu() if hasattr(dirs, "cpu") else dirs, dtype=np.float64))
    r = np.ascontiguousarray(np.asarray(ring.cpu() if hasattr(ring, "cpu") else ring))
    if d.ndim != 2 or d.shape[1] != 3 or r.shape != (len(d),):
        raise ValueError(f"a direction table is f64[D, 3] with ring i32[D], got {d.shape} and {r.shape}")
    n_rings = _integer("n_rings", n_rings, 1, 1 << 16)
    if len(d):
        if not np.isfinite(d).all():
            raise ValueError("a direction is not finite")
        norm = np.sqrt((d * d).sum(1))
        if not (np.abs(norm - 1.0) <= 1e-12).all():
            raise ValueError("a direction is not of unit length (to 1e-12)")
        if r.min() < 0 or r.max() >= n_rings:
            raise ValueError(f"a ring lies outside 0 .. {n_rings - 1}")
    return d, r.astype(np.int32), n_rings


def march(vox, origins, dirs, ring, n_rings, *, skip=None, max_range=60.0, min_hits=1, rays=False):
    """The rays of `origins` f64[P, 3] (host or device, in the grid's frame) along the table (dirs, ring) through `vox` (tl_light_march).
    skip: i32[P] labels whose voxels do not block, or None.  Returns a dict of device tensors: counts i32[P, R, 4], status i32[P] (1 = the
    origin is outside the grid), and with rays=True code u8[P, D] (255 for such an origin) and first f64[P, D] (NaN unless blocked)."""
    p = check_params(max_range=max_range, min_hits=min_hits)
    d, r, R = check_table(dirs, ring, n_rings)
    import torch
    from .. import _hip
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    dev = vox.occ.device
    o = origins if torch.is_tensor(origins) else torch.from_numpy(np.ascontiguousarray(np.asarray(origins, np.float64)))
    o = o.reshape(-1, 3).to(dev, torch.float64).contiguous()
    P, D = len(o), len(d)
    sk = None
    if skip is not None:
        sk = skip if torch.is_tensor(skip) else torch.from_numpy(np.ascontiguousarray(np.asarray(skip)))
        sk = sk.reshape(-1)
        if sk.shape[0] != P:
            raise ValueError(f"mismatched lengths: {P} origins for {sk.shape[0]} skip labels")
        sk = sk.to(dev, torch.int32).contiguous()
    dd, rr = torch.from_numpy(d).to(dev), torch.from_numpy(r).to(dev)
    counts = torch.zeros((P, R, 4), dtype=torch.int32, device=dev)
    status = torch.ones(P, dtype=torch.int32, device=dev)
    code = torch.full((P, D), 255, dtype=torch.uint8, device=dev) if rays else None
    first = torch.full((P, D), float("nan"), dtype=torch.float64, device=dev) if rays else None
    if P and vox.nx * vox.ny * vox.nz:
        if D == 0:
            dd = torch.zeros((1, 3), dtype=torch.float64, device=dev)                 # (pointers to pass; the table is empty)
            rr = torch.zeros(1, dtype=torch.int32, device=dev)
        _hip.check(_hip.lib().tl_light_march(_hip.ptr(o), _hip.ptr(sk), P, _hip.ptr(dd), _hip.ptr(rr), D, R, _hip.ptr(vox.occ), _hip.ptr(vox.owner),
                                             vox.voxel, vox.ix0, vox.iy0, vox.iz0, vox.nx, vox.ny, vox.nz, p["max_range"], p["min_hits"],
                                             _hip.ptr(counts), _hip.ptr(status), _hip.ptr(code), _hip.ptr(first), _hip.stream()), "tl_light_march")
    out = dict(counts=counts, status=status)
    if rays:
        out.update(code=code, first=first)
    return out


def _derive_origins(m, rays, lo, hi, p):
    """derive() per origin of a march, NaN for the origins outside the grid."""
    d = derive(m["counts"].cpu().numpy(), rays, lo, hi, p["lai_max_zenith"], p["zenith_cone"])
    out = m["status"].cpu().numpy() != 0
    for k in d:
        d[k] = np.array(d[k], np.float64)
        d[k][out] = np.nan
    return d, out


def tree_columns(vox, coords, labels, T, sky, params, mark=None):
    """The LIGHT_COLUMNS of trees 1 .. T as numpy arrays [T]: vox a Voxels with owner, coords and labels the device rows it was built
    from, sky = sky_directions(...)."""
    import torch
    p = params
    dirs, ring, lo, hi = sky
    R = len(lo)
    dev = coords.device
    out = dict(light_columns=np.zeros(T, np.int64), **{k: np.full(T, np.nan) for k in LIGHT_COLUMNS[1:]})
    tree = (labels >= 1) & (labels <= T)
    if T == 0 or not bool(tree.any()):
        return out
    idx = vox.index(coords[tree])
    lab = labels[tree]
    key = (lab * vox.ny + idx[:, 1]) * vox.nx + idx[:, 0]                             # one key per (label, iy, ix)
    ukey, inv = torch.unique(key, return_inverse=True)
    top = torch.full((len(ukey),), -1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, idx[:, 2], "amax")
    ulab = ukey // (vox.ny * vox.nx)
    rem = ukey - ulab * (vox.ny * vox.nx)
    uiy = rem // vox.nx
    origins = vox.centres(torch.stack([rem - uiy * vox.nx, uiy, top], dim=1))
    if mark:
        mark("tree columns: tops")
    m = march(vox, origins, dirs, ring, R, skip=ulab.to(torch.int32), max_range=p["max_range"], min_hits=p["min_hits"])
    counts = torch.zeros((T + 1, R, 4), dtype=torch.int64, device=dev).index_add_(0, ulab, m["counts"].to(torch.int64))
    ncol = torch.bincount(ulab, minlength=T + 1)[1:].cpu().numpy()
    if mark:
        mark("tree columns: march")
    rays = np.bincount(ring, minlength=R).astype(np.int64)
    d = derive(counts[1:].cpu().numpy(), ncol[:, None] * rays[None, :], lo, hi, p["lai_max_zenith"], p["zenith_cone"])
    out["light_columns"] = ncol.astype(np.int64)
    for k, src in zip(LIGHT_COLUMNS[1:], ("openness", "gap_zenith", "lai_e", "edge_share")):
        out[k] = np.where(ncol > 0, d[src], np.nan)
    return out


def light_stage(coords, labels, T, params, mark=None):
    """The LIGHT_COLUMNS of a labelled cloud on the device, as util.inventory appends them."""
    p = check_params(params)
    vox = light_voxels(coords, labels, p["voxel"])
    if mark:
        mark("light voxels")
    return tree_columns(vox, coords, labels, T, sky_directions(p["n_rings"], p["n_azimuth"], p["max_zenith"]), p, mark)


class Light:
    """The light model of a cloud.  vox: the Voxels on the device; sky: (dirs, ring, theta_lo, theta_hi) on the host; the sensor grid
    [sensor_ny, sensor_nx] of edge sensor_cell at (sensor_ix0, sensor_iy0) as host arrays: openness, lai_e, gap_zenith, edge_share f64,
    gap f64[.., .., R], counts i32[.., .., R, 4], sensor_z f64; n_outside, n_no_ground: sensors outside the grid and without ground;
    params: the checked parameters."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to_host(self):
        """dict of numpy arrays: x0, y0, z0 (the lower corner of voxel [0, 0, 0]), voxel, occ, sensor_x0, sensor_y0,
        sensor_cell, sensor_z, RASTER_KEYS, counts, dirs, ring, theta_lo, theta_hi, n_outside, n_no_ground -- x, y and z un-centred by
        `offset`.  The dense owner grid (4 bytes per voxel) stays on the device, as vox.owner: neither copied nor written to light.npz."""
        off = np.zeros(3) if self.offset is None else self.offset
        v, sc, vox = np.float64(self.vox.voxel), np.float64(self.params["sensor_cell"]), self.vox
        d = dict(x0=np.float64(vox.ix0) * v + off[0], y0=np.float64(vox.iy0) * v + off[1], z0=np.float64(vox.iz0) * v + off[2], voxel=v,
                 occ=vox.occ.cpu().numpy().view(np.uint32))
        d.update(sensor_x0=np.float64(self.sensor_ix0) * sc + off[0], sensor_y0=np.float64(self.sensor_iy0) * sc + off[1], sensor_cell=sc,
                 sensor_z=self.sensor_z + off[2])
        d.update({k: getattr(self, k) for k in RASTER_KEYS})
        d.update(counts=self.counts, dirs=self.sky[0], ring=self.sky[1], theta_lo=self.sky[2], theta_hi=self.sky[3],
                 n_outside=np.int64(self.n_outside), n_no_ground=np.int64(self.n_no_ground))
        return d

    def tree_light(self, T=None):
        """The LIGHT_COLUMNS per tree 1 .. T (T = the largest label by default) as numpy arrays; needs labels."""
        if self.labels is None:
            raise ValueError("tree_light needs a light model built with labels")
        if T is None:
            T = max(int(self.labels.max()), 0) if len(self.labels) else 0
        return tree_columns(self.vox, self.coords, self.labels, int(T), self.sky, self.params)

    def point_light(self, coords=None, n_rings=2, n_azimuth=32, chunk=1 << 20):
        """Openness f64[N] (numpy) per row of `coords` (the model's own rows by default; rows outside the grid get NaN): one march per
        unique voxel from its centre along sky_directions(n_rings, n_azimuth, max_zenith), with max_range and min_hits as given, gathered
        back to the rows."""
        import torch
        from .terrain import _device_coords
        p, vox = self.params, self.vox
        dirs, ring, lo, hi = sky_directions(n_rings, n_azimuth, p["max_zenith"])
        c = self.coords if coords is None else _device_coords(coords)
        if len(c) == 0:
            return np.zeros(0, np.float64)
        idx = vox.index(c)
        size = torch.tensor([vox.nx, vox.ny, vox.nz], dtype=torch.int64, device=c.device)
        inside = ((idx >= 0) & (idx < size)).all(1)
        lin = torch.where(inside, (idx[:, 2] * vox.ny + idx[:, 1]) * vox.nx + idx[:, 0], torch.full_like(idx[:, 0], -1))
        ulin, inv = torch.unique(lin, return_inverse=True)
        uz = ulin // (vox.ny * vox.nx)
        rem = ulin - uz * (vox.ny * vox.nx)
        uy = rem // vox.nx
        origins = vox.centres(torch.stack([rem - uy * vox.nx, uy, uz], dim=1))
        origins[ulin < 0] = float("nan")                                             # rows outside the grid: an origin outside it
        rays = np.bincount(ring, minlength=len(lo)).astype(np.int64)
        per = np.empty(len(ulin), np.float64)
        for a in range(0, len(ulin), chunk):
            m = march(vox, origins[a:a + chunk], dirs, ring, len(lo), max_range=p["max_range"], min_hits=p["min_hits"])
            per[a:a + chunk] = _derive_origins(m, rays, lo, hi, p)[0]["openness"]
        return per[inv.cpu().numpy()]

    def hemi_rays(self, x, y, size=512, z=None):
        """The hemispherical view from (x, y) in the model's frame, z = ground + sensor_height unless given: (code u8[size, size], first
        f64[size, size]); pixels outside the circle have code 254.  Equidistant polar projection: a pixel at radius rho (1 = the edge of
        the circle) looks at zenith max_zenith * rho; east is to the right and north up."""
        import torch
        size = _integer("size", size, 2, 2048)
        if z is None:
            z = float(self.terrain.sample(torch.tensor([[float(x), float(y)]], dtype=torch.float64))[0]) + self.params["sensor_height"]
        dirs, inside = hemi_directions(size, self.params["max_zenith"])
        m = march(self.vox, np.array([[float(x), float(y), float(z)]]), dirs, np.zeros(len(dirs), np.int32), 1, max_range=self.params["max_range"],
                  min_hits=self.params["min_hits"], rays=True)
        code, first = np.full((size, size), 254, np.uint8), np.full((size, size), np.nan)
        code[inside], first[inside] = m["code"][0].cpu().numpy(), m["first"][0].cpu().numpy()
        return code, first

    def hemi_picture(self, x, y, size=512, z=None, out=None):
        """The hemispherical picture u8[size, size, 3] (numpy) of hemi_rays: sky SKY_RGB, blocked pixels a green that darkens with
        nearness (by `first` over max_range), rays lost through a side SIDE_RGB, an origin outside the grid and the pixels outside the
        circle OUTSIDE_RGB.  Written to `out` (.png, util.render.write_png) when given."""
        code, first = self.hemi_rays(x, y, size, z)
        img = np.zeros(code.shape + (3,), np.uint8)
        img[(code == 1) | (code == 2)] = SKY_RGB
        img[code == 3] = SIDE_RGB
        img[code >= 254] = OUTSIDE_RGB
        near = np.clip(np.nan_to_num(first, nan=0.0) / self.params["max_range"], 0.0, 1.0)
        shade = np.floor(30.0 + 130.0 * np.sqrt(near) + 0.5)
        blocked = code == 0
        img[blocked] = np.stack([shade * 0.45, shade, shade * 0.35], axis=-1)[blocked].astype(np.uint8)
        if out is not None:
            from .render import write_png
            write_png(out, img)
        return img


def light_model(coords, terrain, labels=None, offset=None, stages=None, **params):
    """coords [N, 3] float32 or float64 (a row stride of 3 or 4 elements is read in place), labels [N] integers or None; numpy arrays or
    tensors, on the host or the device.  terrain: a util.terrain.Terrain in the frame of coords (the sensors stand on it).  Returns a
    Light.  `offset` (3 values) is kept for to_host().  `stages`: a list that receives (name, seconds) per stage, each closed by a device
    synchronise (tools/dev_light.py)."""
    p = check_params(**params)
    from .inventory import _offset
    from .terrain import _device_coords
    off = _offset(offset)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    c = _device_coords(coords)
    n, dev = len(c), c.device
    lab = None if labels is None else _labels(labels, n, dev)
    t0 = [time.perf_counter()]

    def mark(name):
        if stages is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            stages.append((name, now - t0[0]))
            t0[0] = now

    vox = light_voxels(c, lab, p["voxel"])
    mark("voxels")
    sky = sky_directions(p["n_rings"], p["n_azimuth"], p["max_zenith"])
    dirs, ring, lo, hi = sky
    R = len(lo)
    sc = np.float64(p["sensor_cell"])
    if n:
        xlo, xhi = torch.aminmax(c[:, :2], dim=0)
        ext = torch.stack([xlo, xhi]).to(torch.float64).cpu().numpy()
        sx0, sy0 = (int(k) for k in np.floor(ext[0] / sc))
        snx, sny = (int(k) for k in np.floor(ext[1] / sc) - np.floor(ext[0] / sc) + 1)
        if snx > MAX_SIDE or sny > MAX_SIDE:
            raise ValueError(f"the cloud spans {ext[1][0] - ext[0][0]:.6g} x {ext[1][1] - ext[0][1]:.6g} m: {snx} x {sny} sensor cells of "
                             f"{p['sensor_cell']} m, beyond {MAX_SIDE} cells a side; use a larger sensor_cell")
    else:
        sx0 = sy0 = snx = sny = 0
    sx = ((sx0 + np.arange(snx)).astype(np.float64) + 0.5) * sc
    sy = ((sy0 + np.arange(sny)).astype(np.float64) + 0.5) * sc
    gx, gy = np.meshgrid(sx, sy)                                                     # [sny, snx], row 0 the lowest y
    xy = torch.from_numpy(np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)).to(dev)
    ground = terrain.sample(xy) if len(xy) else torch.zeros(0, dtype=torch.float64, device=dev)
    sz = ground + p["sensor_height"]
    origins = torch.cat([xy, sz[:, None]], dim=1).contiguous()
    m = march(vox, origins, dirs, ring, R, max_range=p["max_range"], min_hits=p["min_hits"])
    mark("sensor grid")
    rays = np.bincount(ring, minlength=R).astype(np.int64)
    d, outside = _derive_origins(m, rays, lo, hi, p)
    no_ground = np.isnan(sz.cpu().numpy())
    counts = m["counts"].cpu().numpy().reshape(sny, snx, R, 4)
    mark("derive")
    return Light(vox=vox, sky=sky, terrain=terrain, coords=c, labels=lab, params=p, offset=off, sensor_ix0=sx0, sensor_iy0=sy0, sensor_nx=snx,
                 sensor_ny=sny, sensor_z=sz.cpu().numpy().reshape(sny, snx), counts=counts, openness=d["openness"].reshape(sny, snx),
                 lai_e=d["lai_e"].reshape(sny, snx), gap_zenith=d["gap_zenith"].reshape(sny, snx), edge_share=d["edge_share"].reshape(sny, snx),
                 gap=d["gap"].reshape(sny, snx, R), n_outside=int((outside & ~no_ground).sum()), n_no_ground=int(no_ground.sum()))


def cloud_light(points, terrain_cfg=None, **params):
    """The light model of an N x 3 or N x 4 cloud (x y z [label]), as the command line computes it: util.terrain.cloud_terrain centres the
    coordinates on their float64 mean and builds the terrain (of the label-0 rows when there are labels; parameters in terrain_cfg), the
    light model is taken in that frame with the mean as `offset`.  Returns (light, terrain)."""
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
    return light_model(centred, terrain, lab, offset=terrain.offset, **p), terrain


def write_light(path, light):
    """.npz with the keys of Light.to_host() (a dict of those arrays is taken as it is)."""
    d = light if isinstance(light, dict) else light.to_host()
    with open(path, "wb") as f:
        np.savez(f, **d)
    return path


def add_arguments(ap):
    """One option per parameter (shared with util.segment and util.inventory)."""
    for k, v in DEFAULTS.items():
        ap.add_argument(_OPTIONS[k], dest="light_" + k, type=int if isinstance(v, int) else float, default=v, help=_HELP[k])


def params_of(a):
    return {k: getattr(a, "light_" + k) for k in DEFAULTS}


def main(argv=None):
    import os
    from . import terrain as _terrain
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.light", description="light under the canopy: gap fraction, openness and effective LAI of a cloud")
    ap.add_argument("--forest", required=True, help="cloud: .npy / .npz / .txt / .las, N x 3 (x y z) or N x 4 (x y z label; label 0 = ground candidates)")
    ap.add_argument("--out", required=True, help=".npz to write: the arrays of Light.to_host()")
    ap.add_argument("--hemi", default=None, help="x,y in the input's frame: the position of a hemispherical picture (with --hemi-out)")
    ap.add_argument("--hemi-out", default=None, help=".png to write: the hemispherical picture at --hemi")
    ap.add_argument("--hemi-size", type=int, default=512, help="edge of the hemispherical picture, pixels (2..2048)")
    add_arguments(ap)
    _terrain.add_arguments(ap)
    a = ap.parse_args(argv)
    hemi = None
    try:
        params = check_params(params_of(a))
        terrain_cfg = _terrain.check_params(_terrain.params_of(a))
        if (a.hemi is None) != (a.hemi_out is None):
            raise ValueError("--hemi and --hemi-out go together")
        if a.hemi is not None:
            hemi = [float(v) for v in a.hemi.split(",")]
            if len(hemi) != 2 or not np.isfinite(hemi).all():
                raise ValueError(f"--hemi takes x,y, got {a.hemi!r}")
            _integer("--hemi-size", a.hemi_size, 2, 2048)
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
    light, _ = cloud_light(data, terrain_cfg=terrain_cfg, **params)
    write_light(a.out, light)
    if hemi is not None:
        off = np.zeros(3) if light.offset is None else light.offset
        light.hemi_picture(hemi[0] - off[0], hemi[1] - off[1], a.hemi_size, out=a.hemi_out)
    known = light.openness[np.isfinite(light.openness)]
    print(f"{a.forest}: {len(data)} points, {light.vox.nx} x {light.vox.ny} x {light.vox.nz} voxels of {light.vox.voxel} m, {light.sensor_nx} x "
          f"{light.sensor_ny} sensors of {light.params['sensor_cell']} m, mean openness {float(known.mean()) if len(known) else float('nan'):.3f}, "
          f"{light.n_outside} sensors outside the grid, {light.n_no_ground} without ground -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
