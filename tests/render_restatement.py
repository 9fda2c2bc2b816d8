"""The semantics of the renderer in numpy float64, written from the text alone: it imports nothing from the package.

Canvas: keys u64 [H, W], 0 = empty, image row 0 at the top.  A view record is 18 f64: u, v, w, c, s, x0, y0, vw, vh, 0.  A key is
image(float32 depth) << 32 | rgb; the larger key wins a pixel.  Every function below loops or vectorises as is convenient: all results are
maxima, selections and fixed-order sums, so the order of the rows cannot matter."""
import colorsys
import math

import numpy as np

PRESETS = {
    "top": ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    "south": ((1, 0, 0), (0, 0, 1), (0, -1, 0)),
    "north": ((-1, 0, 0), (0, 0, 1), (0, 1, 0)),
    "east": ((0, 1, 0), (0, 0, 1), (1, 0, 0)),
    "west": ((0, -1, 0), (0, 0, 1), (-1, 0, 0)),
}
RAMPS = {
    "height": ((0, 68, 27), (255, 237, 60), (255, 255, 255)),
    "terrain": ((44, 127, 144), (140, 100, 60), (255, 255, 255)),
    "grey": ((32, 32, 32), (255, 255, 255)),
    "wood": ((60, 160, 60), (139, 90, 43)),
}


def view(az, el):
    """u, v, w of a camera standing at azimuth az (degrees clockwise from +y) and elevation el (degrees above the horizon)."""
    a, e = math.radians(az), math.radians(el)
    w = np.array([math.sin(a) * math.cos(e), math.cos(a) * math.cos(e), math.sin(e)])
    u = np.array([-math.cos(a), math.sin(a), 0.0])
    return u, np.cross(w, u), w


def axes(spec):
    if isinstance(spec, str):
        if spec == "oblique":
            return view(210.0, 35.0)
        return tuple(np.array(r, np.float64) for r in PRESETS[spec])
    return view(float(spec[0]), float(spec[1]))


def record(spec, centre, s, viewport):
    u, v, w = axes(spec)
    return np.concatenate([u, v, w, np.asarray(centre, np.float64), [float(s)], np.asarray(viewport, np.float64), [0.0]])


def fit_view(spec, lo, hi, viewport, margin=0.05):
    """The record whose centre is the middle of the box lo .. hi and whose scale lets the 8 projected corners fill the viewport less the
    margin on every side; a box without width and height gets s = 1."""
    u, v, _ = axes(spec)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = (lo + hi) / 2.0
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]) - c
    ea, eb = np.abs(corners @ u).max(), np.abs(corners @ v).max()
    cand = [viewport[2 + i] / 2.0 * (1.0 - 2.0 * margin) / e for i, e in enumerate((ea, eb)) if e > 0.0]
    return record(spec, c, min(cand) if cand else 1.0, viewport)


def enc32(d):
    """The order-preserving u32 image of float32 depths."""
    b = np.asarray(d, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), b ^ np.uint32(0xFFFFFFFF), b | np.uint32(0x80000000)).astype(np.uint32)


def dec32(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(np.float32)


def pack(rgb):
    r = np.asarray(rgb, np.int64)
    return r[..., 0] << 16 | r[..., 1] << 8 | r[..., 2]


def default_palette(P=258):
    lut = [(40, 40, 40), (150, 150, 150)]
    for i in range(P - 2):
        lut.append(tuple(int(math.floor(x * 255 + 0.5)) for x in colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 0.65, 0.95)))
    return pack(np.array(lut)).astype(np.uint32)


def ramp(name):
    """256 entries between the control colours, in integer arithmetic."""
    stops = RAMPS[name]
    K = len(stops)
    out = []
    for i in range(256):
        seg = min(i * (K - 1) // 255, K - 2)
        rem = i * (K - 1) - seg * 255
        out.append(tuple((stops[seg][ch] * (255 - rem) + stops[seg + 1][ch] * rem + 127) // 255 for ch in range(3)))
    return pack(np.array(out)).astype(np.uint32)


def ramp_index(v, lo, hi):
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((np.asarray(v, np.float64) - lo) / (hi - lo) * 255.0 + 0.5)
    return np.where(t >= 0.0, np.minimum(t, 255.0), 0.0).astype(np.int64)


def colours(n, mode, rgb=0, attr=None, lut=None, lo=0.0, hi=1.0, nan_rgb=0):
    """u32 [n]: the colour of every row."""
    if mode == 0:
        return np.full(n, rgb, np.uint32)
    if mode == 1:
        lab, P = np.asarray(attr, np.int64), len(lut)
        idx = np.where(lab < 0, 0, np.where(lab == 0, 1, 2 + (np.maximum(lab, 1) - 1) % (P - 2)))
        return (np.asarray(lut, np.uint32)[idx] & np.uint32(0xFFFFFF)).astype(np.uint32)
    if mode == 2:
        v = np.asarray(attr).astype(np.float64)
        nan = np.isnan(v)
        c = np.asarray(lut, np.uint32)[ramp_index(np.where(nan, lo, v), lo, hi)] & np.uint32(0xFFFFFF)
        return np.where(nan, np.uint32(nan_rgb), c).astype(np.uint32)
    return pack(np.asarray(attr, np.uint8)).astype(np.uint32)


def project(coords, views, vid=None):
    """px, py (f64, whole numbers or not finite), the f32 depth, the view record of every row, `use` (rows that are drawn) and `flag`."""
    p = np.asarray(coords)[:, :3].astype(np.float64)
    n, views = len(p), np.asarray(views, np.float64).reshape(-1, 18)
    vid = np.zeros(n, np.int64) if vid is None else np.asarray(vid, np.int64)
    over = vid >= len(views)
    use = (vid >= 0) & ~over
    m = views[np.where(use, vid, 0)]
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(all="ignore"):
        q = p - m[:, 9:12]
        a = (m[:, 0] * q[:, 0] + m[:, 1] * q[:, 1]) + m[:, 2] * q[:, 2]
        b = (m[:, 3] * q[:, 0] + m[:, 4] * q[:, 1]) + m[:, 5] * q[:, 2]
        d = (m[:, 6] * q[:, 0] + m[:, 7] * q[:, 1]) + m[:, 8] * q[:, 2]
        df = (d + 0.0).astype(np.float32)
        px = np.floor(a * m[:, 12] + (m[:, 13] + m[:, 15] / 2.0))
        py = np.floor((m[:, 14] + m[:, 16] / 2.0) - b * m[:, 12])
    ok = finite & np.isfinite(df)
    flag = bool((over | (use & ~ok)).any())
    return px, py, df, m, use & ok, flag


def splat(keys, coords, views, vid=None, mode=0, rgb=0, attr=None, lut=None, lo=0.0, hi=1.0, nan_rgb=0, size=2):
    """Draws the rows into keys (u64 [H, W], in place) and returns the flag."""
    H, W = keys.shape
    px, py, df, m, use, flag = project(coords, views, vid)
    col = colours(len(px), mode, rgb, attr, lut, lo, hi, nan_rgb)
    key = enc32(df).astype(np.uint64) << np.uint64(32) | col.astype(np.uint64)
    for oy in range(-((size - 1) // 2), size // 2 + 1):
        for ox in range(-((size - 1) // 2), size // 2 + 1):
            X, Y = px + ox, py + oy
            with np.errstate(invalid="ignore"):
                keep = use & (X >= m[:, 13]) & (X <= m[:, 13] + m[:, 15] - 1.0) & (Y >= m[:, 14]) & (Y <= m[:, 14] + m[:, 16] - 1.0)
                keep &= (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
            np.maximum.at(keys, (Y[keep].astype(np.int64), X[keep].astype(np.int64)), key[keep])
    return flag


def raster_keys(keys, grid, lut, lo, hi, zoom=1, at=(0, 0)):
    grid = np.asarray(grid, np.float64)
    ny, nx = grid.shape
    for py in range(ny * zoom):
        for px in range(nx * zoom):
            v = grid[ny - 1 - py // zoom, px // zoom]
            k = np.uint64(0)
            if not np.isnan(v):
                k = np.uint64(int(enc32(np.float32(v + 0.0))) << 32 | int(lut[int(ramp_index(v, lo, hi))]) & 0xFFFFFF)
            keys[at[1] + py, at[0] + px] = k
    return keys


def shade(keys, radius=1, strength=1.0, background=(0, 0, 0)):
    """out u8 [H, W, 3] and depth f32 [H, W] (NaN where empty)."""
    H, W = keys.shape
    depth = np.where(keys != 0, dec32((keys >> np.uint64(32)).astype(np.uint32)), np.float32(np.nan)).astype(np.float32)
    dc = depth.astype(np.float64)
    o = np.zeros((H, W))
    for dy in (-radius, 0, radius):
        for dx in (-radius, 0, radius):
            if dy == 0 and dx == 0:
                continue
            dn = np.full((H, W), np.nan)
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            yn, xn = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            dn[ys, xs] = dc[yn, xn]
            with np.errstate(invalid="ignore"):
                diff = dn - dc
                o = o + np.where(diff > 0.0, diff, 0.0)
    o = o / 8.0
    with np.errstate(invalid="ignore", over="ignore"):
        sh = np.where(keys != 0, 1.0 / (1.0 + strength * o), 1.0)
    rgb = np.where(keys != 0, keys & np.uint64(0xFFFFFF), np.uint64(int(pack(background)))).astype(np.int64)
    out = np.empty((H, W, 3), np.uint8)
    for ch, shift in enumerate((16, 8, 0)):
        with np.errstate(invalid="ignore"):
            t = np.floor((rgb >> shift & 0xFF).astype(np.float64) * sh + 0.5)
        out[:, :, ch] = np.where(t >= 0.0, np.minimum(t, 255.0), 0.0).astype(np.uint8)
    return out, depth


def tree_cards(coords, labels, cols=8, card=(192, 320), spec="south", margin=0.05):
    """The contact sheet: views f64 [T, 18], vid i64 [N], (W, H).  Card t - 1 of tree t sits at column (t - 1) % cols, row (t - 1) // cols;
    every card has the scale at which the widest and the tallest tree fit a card less the margin; a tree is centred on its own box."""
    p, lab = np.asarray(coords)[:, :3].astype(np.float64), np.asarray(labels, np.int64)
    T = int(max(lab.max(), 0)) if len(lab) else 0
    u, v, _ = axes(spec)
    cw, ch = card
    boxes, ea, eb = [], 0.0, 0.0
    for t in range(1, T + 1):
        rows = p[lab == t]
        if not len(rows):
            boxes.append(np.zeros(3))
            continue
        lo, hi = rows.min(0), rows.max(0)
        c = (lo + hi) / 2.0
        corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]) - c
        ea, eb = max(ea, np.abs(corners @ u).max()), max(eb, np.abs(corners @ v).max())
        boxes.append(c)
    cand = [e2 / 2.0 * (1.0 - 2.0 * margin) / e for e2, e in ((cw, ea), (ch, eb)) if e > 0.0]
    s = min(cand) if cand else 1.0
    views = np.array([record(spec, c, s, (((t % cols) * cw), (t // cols) * ch, cw, ch)) for t, c in enumerate(boxes)]).reshape(-1, 18)
    n_rows = max(1, -(-T // cols))
    return views, np.where(lab >= 1, lab - 1, -1), (cols * cw, n_rows * ch)
