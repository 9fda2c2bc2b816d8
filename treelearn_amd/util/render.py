"""Pictures of clouds and rasters on the device, written as PNG: point splats with a depth test, rasters as depth-keyed pixels, a
shading pass that makes unlit points readable, and a contact sheet of the trees.  The batch counterpart of the reference's
interactive `tree_learn/util/plot.py: juxtapose`.

    python -m treelearn_amd.util.render --forest cloud.npy|npz|txt|las --out DIR [--views top south] [--color label] [--size 1024]
                                        [--splat 2] [--cards] [--terrain] [--canopy]

The semantics are the project's own; tests/render_restatement.py states them in numpy float64.

Canvas.  keys u64 [H, W], cleared to 0; 0 means empty; W and H are 1 .. 16384; image row 0 is the top.

View record.  views f64 [V, 18], V >= 1: u[3] screen right, v[3] screen up, w[3] towards the viewer, c[3] the centre, s pixels per metre
(> 0), x0, y0, vw, vh the viewport rectangle on the canvas in pixels (integers held in f64, inside the canvas), one reserved 0.  All
projection is orthographic.  Presets (u, v, w): top (1,0,0) (0,1,0) (0,0,1); south (1,0,0) (0,0,1) (0,-1,0); north (-1,0,0) (0,0,1)
(0,1,0); east (0,1,0) (0,0,1) (1,0,0); west (0,-1,0) (0,0,1) (-1,0,0).  view(az, el): azimuth in degrees clockwise from +y of where
the camera stands, elevation in degrees above the horizon; w = (sin az cos el, cos az cos el, sin el), u = (-cos az, sin az, 0), v = w x
u, built on the host with math.sin / math.cos; `oblique` is view(210, 35).  The device sees only the record.

A row p is f32 or f64, stride 3 or 4, widened exactly.  Its view is views[vid[row]], or views[0] without vid (i32); a negative vid skips
the row, a vid >= V skips it and sets the flag.  q = p - c; a = (u0 qx + u1 qy) + u2 qz, b and d likewise with v and w; fx = a s + (x0 +
vw / 2), fy = (y0 + vh / 2) - b s; px = floor(fx), py = floor(fy).

Depth and key.  The depth is float32(d + 0.0), round to nearest even (-0.0 counts as 0.0); its 32-bit order-preserving image is bits ^
0xFFFFFFFF when the sign bit is set, else bits | 0x80000000: a larger d is nearer the viewer and wins, and no finite or infinite depth
maps to 0.  key = image << 32 | rgb, rgb = r << 16 | g << 8 | b; equal depths after the rounding are settled by the larger rgb, which
keeps the picture independent of the row order.

Footprint.  size k in 1 .. 9 covers pixels px - (k - 1) // 2 .. px + k // 2 and the same for py; a pixel is kept only inside the row's
viewport (clipping is per pixel: a tree on a contact sheet never bleeds into its neighbour's card) and takes atomicMax(keys, key).

Skipped rows.  A row with a non-finite coordinate, or a depth that is not finite as f32, is skipped and sets the flag; the host's aminmax
check comes first and raises ValueError("... not finite").  A set flag raises ValueError when the image is taken.

Colour of a row.  mode 0 constant.  mode 1 label: i64 labels through lut u32 [P], P >= 3: label < 0 -> lut[0], 0 -> lut[1], else lut[2 +
(label - 1) mod (P - 2)]; the default palette has P = 258, lut[0] = (40,40,40), lut[1] = (150,150,150), entry 2 + i =
colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 0.65, 0.95), each channel floor(x * 255 + 0.5).  mode 2 scalar: f32 or f64 values
through lut u32 [256] with lo < hi: index floor((v - lo) / (hi - lo) * 255 + 0.5) clamped to 0 .. 255, NaN -> nan_rgb; the ramps
`height`, `terrain`, `grey`, `wood` are control colours interpolated in integer arithmetic.  mode 3 rgb: u8 [N, 3].

Raster to keys.  A grid f64 [ny, nx] with row 0 the lowest y, an integer zoom >= 1, placed at (x0, y0): pixel (py, px) of the ny zoom x
nx zoom block reads cell (ny - 1 - py // zoom, px // zoom); NaN -> key 0, else image of float32(value + 0.0) << 32 | the scalar colour.
Plain stores.  The value is the depth, so the shading gives a DTM or CHM its relief.

Shading.  out u8 [H, W, 3].  A pixel with key 0 is `background`.  Otherwise d_c is the decoded f32 depth widened to f64; the neighbours
are the 8 offsets (dy, dx) in {-r, 0, r}^2 without the centre in row-major order; one outside the image or with key 0 contributes 0, any
other max(0, d_n - d_c); o = the sum in that order / 8.0; shade = 1.0 / (1.0 + strength o); each channel floor(ch shade + 0.5).
strength 0 copies the colours.  The optional depth is f32 [H, W], NaN where empty.  r is 1 .. 16, strength >= 0 and finite.

Parameters (DEFAULTS, checked by check_params, which touches no GPU): size 1024 (integer 16 .. 16384), splat 2 (integer 1 .. 9), views
("top", "south") (preset names, "oblique", or (az, el) pairs), radius 1 (integer 1 .. 16), strength 1.0 (>= 0, finite), cols 8 (integer
1 .. 256), card (192, 320) (two integers 8 .. 4096), background (0, 0, 0).  An unknown name raises ValueError.

csrc/tl_render.hip holds the three kernels (tl_splat, tl_raster_keys, tl_render_shade).  There is no CPU fallback."""
import argparse
import colorsys
import math
import os
import struct
import sys
import zlib

import numpy as np

PRESETS = dict(top=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), south=((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0)),
               north=((-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)), east=((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),
               west=((0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 0.0)))
OBLIQUE = (210.0, 35.0)
RAMPS = dict(height=((0, 68, 27), (255, 237, 60), (255, 255, 255)), terrain=((44, 127, 144), (140, 100, 60), (255, 255, 255)),
             grey=((32, 32, 32), (255, 255, 255)), wood=((60, 160, 60), (139, 90, 43)))
COLORS = dict(black=(0, 0, 0), white=(255, 255, 255), red=(255, 0, 0), lime=(0, 255, 0), green=(0, 128, 0), blue=(0, 0, 255),
              yellow=(255, 255, 0), cyan=(0, 255, 255), magenta=(255, 0, 255), orange=(255, 165, 0), purple=(128, 0, 128),
              brown=(165, 42, 42), grey=(128, 128, 128), gray=(128, 128, 128), silver=(192, 192, 192), pink=(255, 192, 203),
              navy=(0, 0, 128), teal=(0, 128, 128), olive=(128, 128, 0), maroon=(128, 0, 0))
COLOR_BY = ("label", "height", "hag", "wood")
DEFAULTS = dict(size=1024, splat=2, views=("top", "south"), radius=1, strength=1.0, cols=8, card=(192, 320), background=(0, 0, 0))
MAX_SIDE = 16384
_NO_GPU = "treelearn_amd.util.render runs on the GPU (tl_splat); there is no CPU fallback"
_HELP = dict(size="edge of a cloud view, pixels (16..16384)", splat="footprint of a point, pixels (1..9)",
             views="views of the cloud: top south north east west oblique, or AZ,EL in degrees")

__all__ = ["Canvas", "fit_view", "view", "view_axes", "view_record", "render_cloud", "render_trees", "render_forest", "juxtapose", "tree_cards",
           "write_png", "default_palette", "ramp", "parse_color", "check_params", "DEFAULTS", "PRESETS", "RAMPS", "COLORS"]


# ------------------------------------------------------------------------------------------------ cameras, colours (host, no GPU)
def view(az, el):
    """(u, v, w) of a camera standing at azimuth `az` (degrees clockwise from +y) and elevation `el` (degrees above the horizon)."""
    a, e = math.radians(float(az)), math.radians(float(el))
    w = (math.sin(a) * math.cos(e), math.cos(a) * math.cos(e), math.sin(e))
    u = (-math.cos(a), math.sin(a), 0.0)
    v = (w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0])
    return u, v, w


def _view_spec(spec):
    """A preset name, "oblique", "AZ,EL" or a pair of numbers -> a name or a (az, el) tuple of floats; ValueError otherwise."""
    if isinstance(spec, str):
        if spec in PRESETS or spec == "oblique":
            return spec
        parts = spec.split(",")
    else:
        try:
            parts = list(spec)
        except TypeError:
            parts = []
    try:
        pair = tuple(float(v) for v in parts)
    except (TypeError, ValueError):
        pair = ()
    if len(pair) != 2 or not all(math.isfinite(v) for v in pair):
        raise ValueError(f"a view is one of {tuple(PRESETS) + ('oblique',)} or an (azimuth, elevation) pair in degrees, got {spec!r}")
    return pair


def view_axes(spec):
    """u, v, w as three tuples of a preset name, "oblique" or an (az, el) pair."""
    spec = _view_spec(spec)
    if isinstance(spec, str):
        return view(*OBLIQUE) if spec == "oblique" else PRESETS[spec]
    return view(*spec)


def view_name(spec):
    spec = _view_spec(spec)
    return spec if isinstance(spec, str) else f"az{spec[0]:g}_el{spec[1]:g}"


def view_record(spec, centre, s, viewport):
    """The f64 [18] record of a view: axes of `spec`, centre (3), s pixels per metre, viewport (x0, y0, vw, vh)."""
    u, v, w = view_axes(spec)
    return np.array([*u, *v, *w, *(float(x) for x in centre), float(s), *(float(x) for x in viewport), 0.0], np.float64)


def _box_extent(u, v, lo, hi):
    """The centre of the box and the largest |a|, |b| of its 8 corners about it."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = (lo + hi) / 2.0
    with np.errstate(invalid="ignore"):                                              # (a box that is not finite: the caller raises)
        corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]) - c
        return c, float(np.abs(corners @ np.asarray(u, np.float64)).max()), float(np.abs(corners @ np.asarray(v, np.float64)).max())


def _scale(extents, sides, margin):
    cand = [side / 2.0 * (1.0 - 2.0 * margin) / e for side, e in zip(sides, extents) if e > 0.0]
    return min(cand) if cand else 1.0


def fit_view(spec, lo_xyz, hi_xyz, viewport, margin=0.05):
    """The record that shows the box lo_xyz .. hi_xyz in `viewport` (x0, y0, vw, vh): the centre is the middle of the box, s the scale at
    which its 8 projected corners fill the viewport less `margin` of it on every side (1 for a box without width and height)."""
    if not 0.0 <= float(margin) < 0.5:
        raise ValueError(f"margin must be in [0, 0.5), got {margin!r}")
    u, v, _ = view_axes(spec)
    c, ea, eb = _box_extent(u, v, lo_xyz, hi_xyz)
    if not np.isfinite(c).all() or not math.isfinite(ea) or not math.isfinite(eb):
        raise ValueError("a coordinate is not finite")
    return view_record(spec, c, _scale((ea, eb), (viewport[2], viewport[3]), float(margin)), viewport)


def tree_cards(lo, hi, cols=8, card=(192, 320), spec="south", margin=0.05):
    """The views of a contact sheet from the per-tree boxes lo, hi f64 [T, 3] (a tree without rows: lo > hi or not finite): views f64
    [T, 18] and the canvas (W, H).  Card t - 1 of tree t sits at column (t - 1) % cols, row (t - 1) // cols; every card has the scale at
    which the widest and the tallest tree fit a card less the margin; a tree is centred on the middle of its own box."""
    lo, hi = np.asarray(lo, np.float64).reshape(-1, 3), np.asarray(hi, np.float64).reshape(-1, 3)
    T, (cw, ch) = len(lo), card
    u, v, _ = view_axes(spec)
    centres, ea, eb = [], 0.0, 0.0
    for t in range(T):
        if not (np.isfinite(lo[t]).all() and np.isfinite(hi[t]).all() and (lo[t] <= hi[t]).all()):
            centres.append(np.zeros(3))
            continue
        c, a, b = _box_extent(u, v, lo[t], hi[t])
        centres.append(c)
        ea, eb = max(ea, a), max(eb, b)
    s = _scale((ea, eb), (cw, ch), float(margin))
    views = np.array([view_record(spec, c, s, ((t % cols) * cw, (t // cols) * ch, cw, ch)) for t, c in enumerate(centres)], np.float64).reshape(-1, 18)
    return views, (cols * cw, max(1, -(-T // cols)) * ch)


def _rgb(c):
    """(r, g, b) integers 0 .. 255 -> the packed colour."""
    try:
        r, g, b = (int(v) for v in c)
        if not all(0 <= v <= 255 and v == w for v, w in zip((r, g, b), c)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"a colour is three integers in 0 .. 255, got {c!r}") from None
    return r << 16 | g << 8 | b


def parse_color(c):
    """A CSS colour name of COLORS, '#rrggbb' or an (r, g, b) triple -> (r, g, b)."""
    if isinstance(c, str):
        k = c.strip().lower()
        if k in COLORS:
            return COLORS[k]
        if len(k) == 7 and k[0] == "#":
            try:
                return tuple(int(k[i:i + 2], 16) for i in (1, 3, 5))
            except ValueError:
                pass
        raise ValueError(f"unknown colour {c!r}; expected '#rrggbb' or one of {tuple(COLORS)}")
    p = _rgb(c)
    return p >> 16, p >> 8 & 255, p & 255


def default_palette(P=258):
    """u32 [P] for the label mode: (40,40,40) for labels below 0, (150,150,150) for label 0, then golden-ratio hues."""
    if int(P) != P or P < 3:
        raise ValueError(f"a palette has at least 3 entries, got {P!r}")
    lut = [_rgb((40, 40, 40)), _rgb((150, 150, 150))]
    for i in range(int(P) - 2):
        lut.append(_rgb(tuple(int(math.floor(x * 255 + 0.5)) for x in colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 0.65, 0.95))))
    return np.array(lut, np.uint32)


def ramp(name):
    """u32 [256]: the control colours of RAMPS[name], interpolated in integer arithmetic."""
    if name not in RAMPS:
        raise ValueError(f"unknown ramp {name!r}; expected one of {tuple(RAMPS)}")
    stops = RAMPS[name]
    K = len(stops)
    out = []
    for i in range(256):
        seg = min(i * (K - 1) // 255, K - 2)
        rem = i * (K - 1) - seg * 255
        out.append(_rgb(tuple((stops[seg][ch] * (255 - rem) + stops[seg + 1][ch] * rem + 127) // 255 for ch in range(3))))
    return np.array(out, np.uint32)


_ramp_table = ramp                              # (Canvas.splat and Canvas.raster have a parameter of that name)


# ------------------------------------------------------------------------------------------------ parameters
def _integer(name, v, lo, hi):
    if isinstance(v, bool) or isinstance(v, float) and not np.isfinite(v) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def check_params(cfg=None, **kw):
    """The parameters as a dict of plain values (defaults filled in); ValueError for an unknown name or a value outside its range.
    Touches no GPU."""
    p = dict(DEFAULTS)
    for src in (cfg or {}), kw:
        for k, v in src.items():
            if k not in DEFAULTS:
                raise ValueError(f"unknown render parameter {k!r}; expected one of {tuple(DEFAULTS)}")
            if v is not None:
                p[k] = v
    p["size"] = _integer("size", p["size"], 16, MAX_SIDE)
    p["splat"] = _integer("splat", p["splat"], 1, 9)
    p["radius"] = _integer("radius", p["radius"], 1, 16)
    p["cols"] = _integer("cols", p["cols"], 1, 256)
    try:
        p["strength"] = float(p["strength"])
    except (TypeError, ValueError):
        raise ValueError(f"strength must be >= 0 and finite, got {p['strength']!r}") from None
    if not (p["strength"] >= 0 and np.isfinite(p["strength"])):
        raise ValueError(f"strength must be >= 0 and finite, got {p['strength']!r}")
    v = p["views"]
    try:
        v = [v] if isinstance(v, str) else list(v)
    except TypeError:
        raise ValueError(f"views must name at least one view, got {p['views']!r}") from None
    if len(v) == 2 and all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v):
        v = [tuple(v)]                                                               # one (az, el) pair
    if not v:
        raise ValueError("views must name at least one view")
    p["views"] = tuple(_view_spec(s) for s in v)
    try:
        cw, ch = p["card"]
    except (TypeError, ValueError):
        raise ValueError(f"card must be two integers in 8 .. 4096, got {p['card']!r}") from None
    p["card"] = (_integer("card width", cw, 8, 4096), _integer("card height", ch, 8, 4096))
    p["background"] = parse_color(p["background"])
    return p


# ------------------------------------------------------------------------------------------------ the canvas
def _check_views(views, W, H):
    v = np.asarray(views, np.float64).reshape(-1, 18) if np.size(views) and np.size(views) % 18 == 0 else None
    if v is None or not len(v):
        raise ValueError(f"a view is a record of 18 numbers or an array [V, 18] with V >= 1, got shape {np.shape(views)}")
    if not np.isfinite(v).all():
        raise ValueError("a view record is not finite")
    if not (v[:, 12] > 0).all():
        raise ValueError("the scale of a view must be > 0")
    r = v[:, 13:17]
    if not ((r == np.floor(r)).all() and (r[:, :2] >= 0).all() and (r[:, 2:] >= 1).all() and (r[:, 0] + r[:, 2] <= W).all() and (r[:, 1] + r[:, 3] <= H).all()):
        raise ValueError(f"a viewport (x0, y0, vw, vh) must be whole numbers inside the {W} x {H} canvas")
    return np.ascontiguousarray(v)


class Canvas:
    """A canvas of depth-and-colour keys on the device.  splat() and raster() draw into it and return it, layers accumulate; image()
    shades it into u8 [H, W, 3]."""

    def __init__(self, width, height, background=(0, 0, 0)):
        self.width, self.height = _integer("width", width, 1, MAX_SIDE), _integer("height", height, 1, MAX_SIDE)
        self.background = _rgb(parse_color(background))
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError(_NO_GPU)
        self.keys = torch.zeros((self.height, self.width), dtype=torch.int64, device="cuda")     # (the u64 keys, bit for bit)
        self.flags = torch.zeros(4, dtype=torch.int32, device="cuda")
        self._luts = {}

    def clear(self):
        self.keys.zero_(); self.flags.zero_()
        return self

    def _lut(self, name, values):
        import torch
        if name not in self._luts:
            self._luts[name] = torch.from_numpy(np.ascontiguousarray(values, np.uint32).view(np.int32)).to("cuda")
        return self._luts[name]

    def splat(self, coords, *, view, color=None, labels=None, values=None, rgb=None, ramp="height", lo=None, hi=None, size=2, vid=None,
              palette=None, nan_color=(0, 0, 0)):
        """Draws coords [N, 3 or 4] (f32 or f64, host or device) through `view`: one record of 18 numbers, or [V, 18] with vid i32 [N].
        The colour: one of color (a name, '#rrggbb' or a triple; the default is white), labels (i64 through `palette`, default_palette()
        by default), values (f32 / f64 through the ramp `ramp` -- a name of RAMPS or 256 packed colours -- between lo and hi, which default
        to the finite minimum and maximum; NaN gets nan_color), rgb (u8 [N, 3])."""
        import torch
        from .. import _hip
        from .terrain import _device_coords
        size = _integer("size", size, 1, 9)
        if sum(x is not None for x in (color, labels, values, rgb)) > 1:
            raise ValueError("splat takes one of color, labels, values, rgb")
        views = _check_views(view.detach().cpu().numpy() if torch.is_tensor(view) else view, self.width, self.height)
        c = _device_coords(coords)
        n, dev = len(c), c.device
        if vid is None and len(views) != 1:
            raise ValueError(f"{len(views)} views need a vid per row")

        def rows(a, dtype, what, cols=None):
            t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
            t = t.reshape(-1) if cols is None else t.reshape(-1, cols)
            if t.shape[0] != n:
                raise ValueError(f"mismatched lengths: {n} coordinates for {t.shape[0]} {what}")
            return t.to(dev, dtype).contiguous()

        mode, attr, lut, P, flo, fhi, c0, attr_f64 = 0, None, None, 0, 0.0, 1.0, 0xFFFFFF, 0
        if labels is not None:
            mode, attr = 1, rows(labels, torch.int64, "labels")
            pal = default_palette() if palette is None else np.ascontiguousarray(palette, np.uint32).reshape(-1)
            if len(pal) < 3:
                raise ValueError(f"a palette has at least 3 entries, got {len(pal)}")
            lut, P = self._lut(("palette", pal.tobytes()), pal), len(pal)
        elif values is not None:
            v = values if torch.is_tensor(values) else torch.from_numpy(np.ascontiguousarray(np.asarray(values)))
            mode, attr = 2, rows(v, torch.float64 if v.dtype == torch.float64 else torch.float32, "values")
            attr_f64 = int(attr.dtype == torch.float64)
            table = _ramp_table(ramp) if isinstance(ramp, str) else np.ascontiguousarray(ramp, np.uint32).reshape(-1)
            if len(table) != 256:
                raise ValueError(f"a ramp has 256 entries, got {len(table)}")
            lut, P = self._lut(("ramp", table.tobytes()), table), 256
            flo, fhi = _range_of(attr, lo, hi)
        elif rgb is not None:
            mode, attr = 3, rows(rgb, torch.uint8, "colours", cols=3)
        elif color is not None:
            c0 = _rgb(parse_color(color))
        vd = None
        if vid is not None:
            vd = rows(vid, torch.int32, "view indices")
        if n == 0:
            return self
        lo3, hi3 = torch.aminmax(c[:, :3])                                           # exact in the input's own format; NaN propagates
        if not (math.isfinite(float(lo3)) and math.isfinite(float(hi3))):
            raise ValueError("a coordinate is not finite")
        vdev = torch.from_numpy(views).to(dev)
        _hip.check(_hip.lib().tl_splat(_hip.ptr(c), int(c.dtype == torch.float64), c.stride(0), n, _hip.ptr(vd), _hip.ptr(vdev), len(views), mode, c0,
                                       _hip.ptr(attr), attr_f64, _hip.ptr(lut), P, flo, fhi, _rgb(parse_color(nan_color)), size, _hip.ptr(self.keys),
                                       self.width, self.height, _hip.ptr(self.flags), _hip.stream()), "tl_splat")
        return self

    def raster(self, grid, *, ramp, lo=None, hi=None, zoom=1, at=(0, 0)):
        """Writes a grid f64 [ny, nx] (row 0 the lowest y; NaN = empty) as a block of ny zoom x nx zoom pixels at `at` = (x0, y0): the
        cell's value is the depth of its pixels, its colour comes from the ramp between lo and hi (default: the finite extremes)."""
        import torch
        from .. import _hip
        g = grid if torch.is_tensor(grid) else torch.from_numpy(np.ascontiguousarray(np.asarray(grid, np.float64)))
        if g.ndim != 2:
            raise ValueError(f"a raster is a grid [ny, nx], got {tuple(g.shape)}")
        g = g.to("cuda", torch.float64).contiguous()
        ny, nx = g.shape
        zoom = _integer("zoom", zoom, 1, MAX_SIDE)
        x0, y0 = (_integer("at", v, 0, MAX_SIDE) for v in at)
        if x0 + nx * zoom > self.width or y0 + ny * zoom > self.height:
            raise ValueError(f"a {nx} x {ny} raster at zoom {zoom} placed at ({x0}, {y0}) leaves the {self.width} x {self.height} canvas")
        table = _ramp_table(ramp) if isinstance(ramp, str) else np.ascontiguousarray(ramp, np.uint32).reshape(-1)
        if len(table) != 256:
            raise ValueError(f"a ramp has 256 entries, got {len(table)}")
        flo, fhi = _range_of(g, lo, hi)
        if nx * ny == 0:
            return self
        _hip.check(_hip.lib().tl_raster_keys(_hip.ptr(g), nx, ny, zoom, x0, y0, _hip.ptr(self._lut(("ramp", table.tobytes()), table)), flo, fhi,
                                             _hip.ptr(self.keys), self.width, self.height, _hip.stream()), "tl_raster_keys")
        return self

    def image(self, radius=1, strength=1.0, return_depth=False):
        """u8 [H, W, 3] on the device (and the depth f32 [H, W], NaN where empty, with return_depth).  ValueError when a row was skipped
        by the kernel: a view index beyond the views, or a depth beyond float32."""
        import torch
        from .. import _hip
        radius = _integer("radius", radius, 1, 16)
        strength = float(strength)
        if not (strength >= 0 and math.isfinite(strength)):
            raise ValueError(f"strength must be >= 0 and finite, got {strength!r}")
        out = torch.empty((self.height, self.width, 3), dtype=torch.uint8, device="cuda")
        depth = torch.empty((self.height, self.width), dtype=torch.float32, device="cuda") if return_depth else None
        _hip.check(_hip.lib().tl_render_shade(_hip.ptr(self.keys), self.width, self.height, radius, strength, self.background, _hip.ptr(out),
                                              _hip.ptr(depth), _hip.stream()), "tl_render_shade")
        if int(self.flags[0]):
            raise ValueError("a row was skipped: its view index is beyond the views, or its depth is not finite as float32")
        return (out, depth) if return_depth else out


def _range_of(t, lo, hi):
    """lo, hi of a scalar layer: the given ones, else the finite minimum and maximum of t (0, 1 without a finite value; hi = lo + 1 for a
    single value)."""
    import torch
    if lo is None or hi is None:
        known = t[torch.isfinite(t)]
        a, b = (float(v) for v in torch.aminmax(known)) if known.numel() else (0.0, 1.0)
        lo, hi = (a if lo is None else float(lo)), (b if hi is None else float(hi))
        if hi <= lo:
            hi = lo + 1.0
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"lo < hi, both finite, is required; got {lo!r}, {hi!r}")
    return lo, hi


# ------------------------------------------------------------------------------------------------ whole pictures
def _cloud(coords, labels=None):
    import torch
    from .terrain import _device_coords
    c = _device_coords(coords)
    lab = None
    if labels is not None:
        lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)).astype(np.int64, copy=False))
        lab = lab.reshape(-1)
        if lab.shape[0] != len(c):
            raise ValueError(f"mismatched lengths: {len(c)} coordinates for {lab.shape[0]} labels")
        lab = lab.to(c.device, torch.int64).contiguous()
    return c, lab


def _box(c):
    """lo, hi f64 [3] of the cloud on the host (zeros for an empty cloud); ValueError for a non-finite coordinate."""
    import torch
    if not len(c):
        return np.zeros(3), np.zeros(3)
    lo, hi = torch.aminmax(c[:, :3], dim=0)
    box = torch.stack([lo, hi]).to(torch.float64).cpu().numpy()
    if not np.isfinite(box).all():
        raise ValueError("a coordinate is not finite")
    return box[0], box[1]


def render_cloud(coords, labels=None, *, views=("top", "south"), color="label", size=1024, splat=2, hag=None, wood=None, radius=1, strength=1.0,
                 background=(0, 0, 0)):
    """One size x size picture of the cloud per view: a dict view name -> u8 [size, size, 3] on the device.  color: "label" (needs
    labels), "height" (z through the height ramp), "hag" (needs hag, the height above ground per row) or "wood" (needs wood, the u8 flag
    per row)."""
    import torch
    p = check_params(views=views, size=size, splat=splat, radius=radius, strength=strength, background=background)
    if color not in COLOR_BY:
        raise ValueError(f"color must be one of {COLOR_BY}, got {color!r}")
    need = dict(label=labels, hag=hag, wood=wood)
    if color in need and need[color] is None:
        raise ValueError(f"color={color!r} needs the {'labels' if color == 'label' else color} of the rows")
    c, lab = _cloud(coords, labels)
    lo, hi = _box(c)
    out = {}
    for spec in p["views"]:
        cv = Canvas(p["size"], p["size"], p["background"])
        rec = fit_view(spec, lo, hi, (0, 0, p["size"], p["size"]))
        if color == "label":
            cv.splat(c, view=rec, labels=lab, size=p["splat"])
        elif color == "wood":
            w = wood if torch.is_tensor(wood) else torch.from_numpy(np.ascontiguousarray(np.asarray(wood)))
            cv.splat(c, view=rec, values=w.to(torch.float32), ramp="wood", lo=0.0, hi=1.0, size=p["splat"])
        else:
            cv.splat(c, view=rec, values=c[:, 2] if color == "height" else hag, ramp="height", nan_color=(90, 90, 90), size=p["splat"])
        out[view_name(spec)] = cv.image(p["radius"], p["strength"])
    return out


def render_trees(coords, labels, *, cols=8, card=(192, 320), view="south", splat=2, radius=1, strength=1.0, background=(0, 0, 0), palette=None):
    """The contact sheet: one card per tree 1 .. T in label order, `cols` cards a row, every card at the scale of the widest and the
    tallest tree, each tree centred on the middle of its own bounding box, all of them in one tl_splat launch (label <= 0: vid -1).
    Returns u8 [rows card_h, cols card_w, 3] on the device."""
    import torch
    p = check_params(cols=cols, card=card, splat=splat, radius=radius, strength=strength, background=background, views=(view,))
    c, lab = _cloud(coords, labels)
    _box(c)
    T = max(int(lab.max()), 0) if len(lab) else 0
    W, H = p["cols"] * p["card"][0], max(1, -(-T // p["cols"])) * p["card"][1]
    if W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError(f"{T} trees on cards of {p['card']} in {p['cols']} columns need a {W} x {H} sheet, beyond {MAX_SIDE} pixels a side")
    cv = Canvas(W, H, p["background"])
    if T == 0:
        return cv.image(p["radius"], p["strength"])
    tree = lab >= 1
    idx = (lab[tree] - 1).reshape(-1, 1).expand(-1, 3).contiguous()
    xyz = c[:, :3][tree]
    lo = torch.full((T, 3), float("inf"), dtype=c.dtype, device=c.device).scatter_reduce(0, idx, xyz, "amin")
    hi = torch.full((T, 3), float("-inf"), dtype=c.dtype, device=c.device).scatter_reduce(0, idx, xyz, "amax")
    views, _ = tree_cards(lo.to(torch.float64).cpu().numpy(), hi.to(torch.float64).cpu().numpy(), p["cols"], p["card"], p["views"][0])
    vid = torch.where(tree, lab - 1, torch.full_like(lab, -1)).to(torch.int32)
    return cv.splat(c, view=views, vid=vid, labels=lab, size=p["splat"], palette=palette).image(p["radius"], p["strength"])


def _raster_picture(grid, ramp_name, size, radius, strength, background, tops=None):
    """A grid zoomed to about `size` pixels and shaded; tops = (i, j) cell indices drawn on it as 5-pixel white marks."""
    import torch
    g = grid if torch.is_tensor(grid) else torch.from_numpy(np.ascontiguousarray(np.asarray(grid, np.float64)))
    ny, nx = g.shape
    if nx * ny == 0:
        return Canvas(1, 1, background).image(radius, strength)
    if max(nx, ny) > MAX_SIDE:
        raise ValueError(f"a {nx} x {ny} raster is beyond {MAX_SIDE} pixels a side")
    zoom = max(1, min(size // max(nx, ny), MAX_SIDE // max(nx, ny)))
    cv = Canvas(nx * zoom, ny * zoom, background).raster(g, ramp=ramp_name, zoom=zoom)
    if tops is not None and len(tops[0]):
        ti, tj = ((t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t))).to("cuda", torch.float64) for t in tops)
        known = g[torch.isfinite(g)]
        front = (float(known.max()) if known.numel() else 0.0) + 1.0                  # in front of every cell
        pts = torch.stack([ti + 0.5, tj + 0.5, torch.full_like(ti, front)], dim=1).contiguous()
        rec = view_record("top", (nx / 2.0, ny / 2.0, 0.0), float(zoom), (0, 0, nx * zoom, ny * zoom))
        cv.splat(pts, view=rec, color="white", size=5)
    return cv.image(radius, strength)


def render_forest(result, **cfg):
    """The pictures of a segment_forest result (arrays on the host or the device): top_labels, south_labels, top_height (by height above
    ground when the result holds one); dtm and chm when it holds a terrain and a canopy, zoomed to about the size of the cloud views, the
    tree tops on the chm as 5-pixel white marks; light, the openness raster, when it holds a light model; leafwood when the inventory
    holds the flags; trees, the contact sheet.  cfg: the parameters of check_params (views is not used: the views are fixed).  Returns a
    dict name -> u8 [H, W, 3] on the device."""
    p = check_params(cfg)
    c, lab = _cloud(result["coords"], result["labels"])
    kw = dict(size=p["size"], splat=p["splat"], radius=p["radius"], strength=p["strength"], background=p["background"])
    out = {}
    by_label = render_cloud(c, lab, views=("top", "south"), color="label", **kw)
    out["top_labels"], out["south_labels"] = by_label["top"], by_label["south"]
    hag = result.get("height_above_ground")
    out["top_height"] = render_cloud(c, views=("top",), color="height" if hag is None else "hag", hag=hag, **kw)["top"]
    relief = dict(size=p["size"], radius=p["radius"], strength=4.0 * p["strength"], background=p["background"])
    if result.get("terrain") is not None:
        out["dtm"] = _raster_picture(result["terrain"]["z"], "terrain", **relief)
    if result.get("canopy") is not None:
        can = result["canopy"]
        out["chm"] = _raster_picture(can["chm"], "height", tops=(can["tops_i"], can["tops_j"]), **relief)
    if result.get("light") is not None:
        out["light"] = _raster_picture(result["light"]["openness"], "height", **relief)
    wood = (result.get("inventory") or {}).get("leafwood")
    if wood is not None:
        out["leafwood"] = render_cloud(c, views=("south",), color="wood", wood=wood["wood"], **kw)["south"]
    out["trees"] = render_trees(c, lab, cols=p["cols"], card=p["card"], splat=p["splat"], radius=p["radius"], strength=p["strength"],
                                background=p["background"])
    return out


def juxtapose(cloud1, cloud2, label1, label2, color1="blue", color2="red", subset=10, renderer=None, size=1, opacity=1, out=None):
    """Two clouds side by side, the reference's tree_learn/util/plot.py: juxtapose as a picture: every `subset`-th row of each, cloud1 and
    cloud2 from the south in two viewports over one shared box, below them both from the top in one viewport, cloud1 in color1 and cloud2
    in color2 (names of COLORS or '#rrggbb'); `size` is the footprint of a point in pixels.  label1 and label2 name the clouds (a picture
    carries no legend: they are checked to be strings and otherwise unused); renderer and opacity are accepted and ignored.  Returns the
    image u8 [1024, 1024, 3] as a numpy array and writes it to `out` (.png) when given."""
    import torch
    from .terrain import _device_coords
    subset, size = _integer("subset", subset, 1, 1 << 30), _integer("size", size, 1, 9)
    c1, c2 = parse_color(color1), parse_color(color2)
    if not (isinstance(label1, str) and isinstance(label2, str)):
        raise ValueError("label1 and label2 are the names of the two clouds")
    a, b = _device_coords(cloud1)[::subset], _device_coords(cloud2)[::subset]
    boxes = [_box(t) for t in (a, b) if len(t)]
    lo = np.min([bx[0] for bx in boxes], axis=0) if boxes else np.zeros(3)
    hi = np.max([bx[1] for bx in boxes], axis=0) if boxes else np.zeros(3)
    S = 512
    cv = Canvas(2 * S, 2 * S)
    left, right, below = (fit_view(v, lo, hi, r) for v, r in (("south", (0, 0, S, S)), ("south", (S, 0, S, S)), ("top", (0, S, 2 * S, S))))
    a, b = (t.contiguous() if len(t) else t for t in (a, b))
    cv.splat(a, view=left, color=c1, size=size).splat(b, view=right, color=c2, size=size)
    cv.splat(a, view=below, color=c1, size=size).splat(b, view=below, color=c2, size=size)
    img = cv.image().cpu().numpy()
    if out is not None:
        write_png(out, img)
    return img


# ------------------------------------------------------------------------------------------------ files
def write_png(path, image):
    """An image u8 [H, W, 3] (numpy or a tensor) as an 8-bit RGB PNG: one IDAT chunk, filter 0 on every row."""
    img = image.detach().cpu().numpy() if hasattr(image, "detach") else np.asarray(image)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"an image is uint8 [H, W, 3] with H, W >= 1, got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), np.uint8)
    raw[:, 1:] = img.reshape(h, 3 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6))
                + chunk(b"IEND", b""))
    return path


def write_previews(out_dir, images):
    """out_dir/<name>.png for every image of the dict; returns the paths."""
    os.makedirs(out_dir, exist_ok=True)
    return [write_png(os.path.join(out_dir, f"{k}.png"), v) for k, v in images.items()]


# ------------------------------------------------------------------------------------------------ command line
def add_arguments(ap, prefix=""):
    """--<prefix>size, --<prefix>splat, --<prefix>views (util.segment shares them as --preview-...)."""
    ap.add_argument(f"--{prefix}size", type=int, default=DEFAULTS["size"], help=_HELP["size"])
    ap.add_argument(f"--{prefix}splat", type=int, default=DEFAULTS["splat"], help=_HELP["splat"])
    ap.add_argument(f"--{prefix}views", nargs="+", default=list(DEFAULTS["views"]), help=_HELP["views"])


def params_of(a, prefix=""):
    k = prefix.replace("-", "_")
    return dict(size=getattr(a, k + "size"), splat=getattr(a, k + "splat"), views=tuple(getattr(a, k + "views")))


def main(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.render", description="pictures of a point cloud as PNG files")
    ap.add_argument("--forest", required=True, help="cloud: .npy / .npz / .txt / .las, N x 3 (x y z) or N x 4 (x y z label)")
    ap.add_argument("--out", required=True, help="directory to write <view>_<color>.png (and trees.png, dtm.png, chm.png) into")
    ap.add_argument("--color", choices=COLOR_BY[:3], default=None, help="colour the rows by (default: label for a labelled cloud, else height; hag needs --terrain)")
    ap.add_argument("--cards", action="store_true", help="write trees.png, the contact sheet of a labelled cloud")
    ap.add_argument("--terrain", action="store_true", help="build the terrain model and write dtm.png")
    ap.add_argument("--canopy", action="store_true", help="build the canopy height model and write chm.png (implies --terrain)")
    add_arguments(ap)
    a = ap.parse_args(argv)
    try:
        p = check_params(params_of(a))
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
    labelled = data.shape[1] == 4
    color = a.color or ("label" if labelled else "height")
    if color == "label" and not labelled:
        ap.error("--color label needs an N x 4 cloud (x y z label)")
    if a.cards and not labelled:
        ap.error("--cards needs an N x 4 cloud (x y z label)")
    if color == "hag" and not (a.terrain or a.canopy):
        ap.error("--color hag needs --terrain")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    pts = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    lab = pts[:, 3].to(torch.int64) if labelled else None
    xyz = pts[:, :3] - pts[:, :3].mean(0)
    images, hag = {}, None
    if a.terrain or a.canopy:
        from .terrain import terrain_model
        dtm = terrain_model(xyz, lab)
        hag = dtm.height_above_ground(xyz)
        images["dtm"] = _raster_picture(dtm.z, "terrain", p["size"], p["radius"], 4.0 * p["strength"], p["background"])
        if a.canopy:
            from .canopy import canopy_model
            can = canopy_model(xyz, labels=lab, height_above_ground=hag)
            images["chm"] = _raster_picture(can.chm, "height", p["size"], p["radius"], 4.0 * p["strength"], p["background"],
                                            tops=(can.tops["i"], can.tops["j"]))
    for name, img in render_cloud(xyz, lab, views=p["views"], color=color, size=p["size"], splat=p["splat"], hag=hag).items():
        images[f"{name}_{color}"] = img
    if a.cards:
        images["trees"] = render_trees(xyz, lab, cols=p["cols"], card=p["card"], splat=p["splat"])
    paths = write_previews(a.out, images)
    print(f"{a.forest}: {len(data)} points -> {len(paths)} pictures in {a.out}: {', '.join(sorted(images))}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
