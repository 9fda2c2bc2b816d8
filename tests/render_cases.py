"""Cases of the renderer worked by hand.  A case is a dict: W, H (the canvas), ops (a list of ("splat", kwargs) and
("raster", kwargs) in the vocabulary of render_restatement.splat / raster_keys), keys {(py, px): (depth, rgb)} -- every pixel that is
not empty --, flag, and optionally shade (radius, strength, background) with image {(py, px): (r, g, b)} for the pixels worked out.
expected_keys() packs `keys` with struct, independently of the restatement's numpy.

Unless a case says otherwise the view is `top` (u = x, v = y, w = z) about the origin at 1 pixel per metre, so with a viewport (x0, y0,
vw, vh): fx = x + (x0 + vw / 2), fy = (y0 + vh / 2) - y, depth = z."""
import struct

import numpy as np

TOP = (1, 0, 0, 0, 1, 0, 0, 0, 1)
PRESETS = {"top": TOP, "south": (1, 0, 0, 0, 0, 1, 0, -1, 0), "north": (-1, 0, 0, 0, 0, 1, 0, 1, 0), "east": (0, 1, 0, 0, 0, 1, 1, 0, 0),
           "west": (0, -1, 0, 0, 0, 1, -1, 0, 0)}
IDENTITY_LUT = np.arange(256, dtype=np.uint32)                      # rgb = the ramp index itself


def rec(viewport, axes=TOP, centre=(0, 0, 0), s=1.0):
    return np.array([*axes, *centre, s, *viewport, 0], np.float64)


def image32(depth):
    """The order-preserving image of a float32 depth, through struct."""
    b = struct.unpack("<I", struct.pack("<f", depth))[0]
    return b ^ 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000


def expected_keys(case):
    k = np.zeros((case["H"], case["W"]), np.uint64)
    for (py, px), (d, rgb) in case["keys"].items():
        k[py, px] = np.uint64(image32(d) << 32 | rgb)
    return k


def rgb_rows(*colours):
    return np.array([[c >> 16, c >> 8 & 255, c & 255] for c in colours], np.uint8)


def integer_fx():
    """Viewport (0, 0, 8, 8): fx = x + 4, fy = 4 - y.  Row A (1, 0.5, 2): fx = 5.0 exactly -> px 5; fy = 3.5 -> py 3.  Row B (1 - 2^-50,
    -0.5, 1): 1 - 2^-50 is a double, and so is 5 - 2^-50 (the spacing of doubles in [4, 8) is 2^-50): fx is one ulp below 5 -> px 4; fy =
    4.5 -> py 4.  k = 1."""
    xyz = np.array([[1.0, 0.5, 2.0], [1.0 - 2.0 ** -50, -0.5, 1.0]])
    return dict(W=8, H=8, ops=[("splat", dict(coords=xyz, views=rec((0, 0, 8, 8)), mode=0, rgb=0x010203, size=1))],
                keys={(3, 5): (2.0, 0x010203), (4, 4): (1.0, 0x010203)}, flag=False)


def _borders(k, keys):
    """Viewport (2, 1, 4, 5) on an 8 x 8 canvas: columns 2 .. 5, rows 1 .. 5; fx = x + 4, fy = 3.5 - y.  Four rows, one in every corner
    pixel: (-1.5, 2) -> (py 1, px 2), (1.5, 2) -> (1, 5), (-1.5, -2) -> (5, 2), (1.5, -2) -> (5, 5), colours 1, 2, 3, 4, depth 1."""
    xyz = np.array([[-1.5, 2.0, 1.0], [1.5, 2.0, 1.0], [-1.5, -2.0, 1.0], [1.5, -2.0, 1.0]])
    return dict(W=8, H=8, ops=[("splat", dict(coords=xyz, views=rec((2, 1, 4, 5)), mode=3, attr=rgb_rows(1, 2, 3, 4), size=k))],
                keys={p: (1.0, c) for c, ps in keys.items() for p in ps}, flag=False)


def borders_k1():
    """k = 1: the footprint is the pixel itself."""
    return _borders(1, {1: [(1, 2)], 2: [(1, 5)], 3: [(5, 2)], 4: [(5, 5)]})


def borders_k2():
    """k = 2: px .. px + 1, py .. py + 1.  Top left: all four inside.  Top right: column 6 is outside.  Bottom left: row 6 is outside.
    Bottom right: only the pixel itself."""
    return _borders(2, {1: [(1, 2), (1, 3), (2, 2), (2, 3)], 2: [(1, 5), (2, 5)], 3: [(5, 2), (5, 3)], 4: [(5, 5)]})


def borders_k3():
    """k = 3: px - 1 .. px + 1, py - 1 .. py + 1.  Column 1 and row 0 (top left), column 6 and row 0 (top right), column 1 and row 6,
    column 6 and row 6 are outside: four pixels are left of each footprint of nine."""
    return _borders(3, {1: [(1, 2), (1, 3), (2, 2), (2, 3)], 2: [(1, 4), (1, 5), (2, 4), (2, 5)], 3: [(4, 2), (4, 3), (5, 2), (5, 3)],
                        4: [(4, 4), (4, 5), (5, 4), (5, 5)]})


def straddle():
    """An 8 x 4 canvas, view 0 in (0, 0, 4, 4), view 1 in (4, 0, 4, 4).  Row 0 in view 0 at (1.5, 0.5): fx = 3.5, fy = 1.5 -> (py 1, px
    3); k = 3 covers columns 2 .. 4, of which 4 belongs to the other viewport: columns 2, 3, rows 0 .. 2.  Row 1 in view 1 at (-1.5, 0.5):
    fx = -1.5 + 6 = 4.5 -> px 4; columns 3 .. 5, of which 3 is outside: columns 4, 5."""
    xyz = np.array([[1.5, 0.5, 1.0], [-1.5, 0.5, 2.0]])
    views = np.stack([rec((0, 0, 4, 4)), rec((4, 0, 4, 4))])
    keys = {(y, x): (1.0, 7) for y in (0, 1, 2) for x in (2, 3)}
    keys.update({(y, x): (2.0, 9) for y in (0, 1, 2) for x in (4, 5)})
    return dict(W=8, H=4, ops=[("splat", dict(coords=xyz, views=views, vid=np.array([0, 1], np.int32), mode=3, attr=rgb_rows(7, 9), size=3))],
                keys=keys, flag=False)


def equal_depth():
    """Two rows on one pixel at depth 1, colours 0x0000FF and 0x00FF00: the larger rgb, 0x00FF00, wins."""
    xyz = np.array([[0.5, 0.5, 1.0], [0.5, 0.5, 1.0]])
    return dict(W=4, H=4, ops=[("splat", dict(coords=xyz, views=rec((0, 0, 4, 4)), mode=3, attr=rgb_rows(0x0000FF, 0x00FF00), size=1))],
                keys={(1, 2): (1.0, 0x00FF00)}, flag=False)


def f32_tie():
    """Depths 1 and 1 + 2^-40 differ as doubles and are both 1.0f.  The nearer row is blue (0x0000FF), the other red (0xFF0000): after the
    rounding they tie, and red is the larger rgb."""
    xyz = np.array([[0.5, 0.5, 1.0 + 2.0 ** -40], [0.5, 0.5, 1.0]])
    return dict(W=4, H=4, ops=[("splat", dict(coords=xyz, views=rec((0, 0, 4, 4)), mode=3, attr=rgb_rows(0x0000FF, 0xFF0000), size=1))],
                keys={(1, 2): (1.0, 0xFF0000)}, flag=False)


def signed_zero():
    """Row 0 (-1, -1, -0.0): d = (0 * -1 + 0 * -1) + 1 * -0.0 = (-0.0 + -0.0) + -0.0 = -0.0, and -0.0 + 0.0 = +0.0.  Row 1 (-1, -1, 0.0): d
    = +0.0.  Both have the image 0x80000000 (that of -0.0 itself would be 0x7FFFFFFF, and lose); row 0 has the larger colour and wins.
    fx = -1 + 2 = 1, fy = 2 + 1 = 3."""
    xyz = np.array([[-1.0, -1.0, -0.0], [-1.0, -1.0, 0.0]])
    return dict(W=4, H=4, ops=[("splat", dict(coords=xyz, views=rec((0, 0, 4, 4)), mode=3, attr=rgb_rows(0x00FF00, 0x0000FF), size=1))],
                keys={(3, 1): (0.0, 0x00FF00)}, flag=False)


def negative_depth():
    """One row at depth -5 on an empty pixel: -5.0f is 0xC0A00000, its image 0x3F5FFFFF, which is above 0: the key 0x3F5FFFFF00000001
    is drawn."""
    assert image32(-5.0) == 0x3F5FFFFF
    return dict(W=4, H=4, ops=[("splat", dict(coords=np.array([[0.5, 0.5, -5.0]]), views=rec((0, 0, 4, 4)), mode=0, rgb=1, size=1))],
                keys={(1, 2): (-5.0, 1)}, flag=False)


def view_indices():
    """V = 2.  vid -1: skipped.  vid 2 = V: skipped, and the flag is set.  vid 1: drawn in viewport (4, 0, 4, 4): fx = 0.5 + 6 -> px 6."""
    xyz = np.array([[0.5, 0.5, 1.0], [0.5, 0.5, 1.0], [0.5, 0.5, 1.0]])
    views = np.stack([rec((0, 0, 4, 4)), rec((4, 0, 4, 4))])
    return dict(W=8, H=4, ops=[("splat", dict(coords=xyz, views=views, vid=np.array([-1, 2, 1], np.int32), mode=0, rgb=5, size=1))],
                keys={(1, 6): (1.0, 5)}, flag=True)


def _preset(name, py, px, depth):
    """The point (1, 2, 3) in a 16 x 16 viewport about the origin: fx = a + 8, fy = 8 - b.
      top    a =  1  b = 2  d =  3  -> px  9  py 6        south  a =  1  b = 3  d = -2  -> px  9  py 5
      north  a = -1  b = 3  d =  2  -> px  7  py 5        east   a =  2  b = 3  d =  1  -> px 10  py 5
      west   a = -2  b = 3  d = -1  -> px  6  py 5"""
    return dict(W=16, H=16, ops=[("splat", dict(coords=np.array([[1.0, 2.0, 3.0]]), views=rec((0, 0, 16, 16), PRESETS[name]), mode=0, rgb=3, size=1))],
                keys={(py, px): (depth, 3)}, flag=False)


def preset_top():
    return _preset("top", 6, 9, 3.0)


def preset_south():
    return _preset("south", 5, 9, -2.0)


def preset_north():
    return _preset("north", 5, 7, 2.0)


def preset_east():
    return _preset("east", 5, 10, 1.0)


def preset_west():
    return _preset("west", 5, 6, -1.0)


PALETTE_ENTRY_2 = (242, 85, 85)


def labels():
    """P = 258.  Label -1 -> lut[0] = (40, 40, 40); 0 -> lut[1] = (150, 150, 150); 1 -> lut[2]; 257 -> lut[2 + 256 mod 256] = lut[2].
    lut[2] of the default palette is hsv (0, 0.65, 0.95): r = v = 0.95 -> floor(242.25 + 0.5) = 242; g = b = v (1 - s) = 0.3325 ->
    floor(84.7875 + 0.5) = 85.  Entries 3 .. 257 of this case's table are the numbers 3 .. 257, which no row may get.  Rows at x = -1.5,
    -0.5, 0.5, 1.5 -> px 0, 1, 2, 3 in row 1."""
    lut = np.arange(258, dtype=np.uint32)
    lut[:3] = [40 << 16 | 40 << 8 | 40, 150 << 16 | 150 << 8 | 150, 242 << 16 | 85 << 8 | 85]
    xyz = np.array([[-1.5, 0.5, 1.0], [-0.5, 0.5, 1.0], [0.5, 0.5, 1.0], [1.5, 0.5, 1.0]])
    return dict(W=4, H=4, ops=[("splat", dict(coords=xyz, views=rec((0, 0, 4, 4)), mode=1, attr=np.array([-1, 0, 1, 257], np.int64), lut=lut, size=1))],
                keys={(1, 0): (1.0, int(lut[0])), (1, 1): (1.0, int(lut[1])), (1, 2): (1.0, int(lut[2])), (1, 3): (1.0, int(lut[2]))}, flag=False)


def scalars():
    """lo = 2, hi = 4, lut[i] = i.  2 -> floor(0 + 0.5) = 0; 4 -> floor(255.5) = 255; 1 -> floor(-127.5 + 0.5) = -127 -> 0; 9 ->
    floor(892.5 + 0.5) = 893 -> 255; 3 -> floor(127.5 + 0.5) = 128; NaN -> nan_rgb = 0xABCDEF.  Rows at x = -2.5 .. 2.5 -> px 0 .. 5."""
    xyz = np.array([[x, 0.5, 1.0] for x in (-2.5, -1.5, -0.5, 0.5, 1.5, 2.5)])
    v = np.array([2.0, 4.0, 1.0, 9.0, 3.0, np.nan])
    return dict(W=6, H=2, ops=[("splat", dict(coords=xyz, views=rec((0, 0, 6, 2)), mode=2, attr=v, lut=IDENTITY_LUT, lo=2.0, hi=4.0, nan_rgb=0xABCDEF,
                                               size=1))],
                keys={(0, 0): (1.0, 0), (0, 1): (1.0, 255), (0, 2): (1.0, 0), (0, 3): (1.0, 255), (0, 4): (1.0, 128), (0, 5): (1.0, 0xABCDEF)}, flag=False)


GRID = np.array([[1.0, np.nan], [3.0, 2.0]])                         # grid row 0 is the lowest y: it is the LOWER image row


def raster_zoom1():
    """lo = 1, hi = 3, lut[i] = i: 1 -> 0, 3 -> 255, 2 -> floor(127.5 + 0.5) = 128.  At (1, 1) on a 4 x 4 canvas: image row 1 shows grid
    row 1 (3, 2), image row 2 grid row 0 (1, NaN): the NaN cell stays empty."""
    return dict(W=4, H=4, ops=[("raster", dict(grid=GRID, lut=IDENTITY_LUT, lo=1.0, hi=3.0, zoom=1, at=(1, 1)))],
                keys={(1, 1): (3.0, 255), (1, 2): (2.0, 128), (2, 1): (1.0, 0)}, flag=False)


def raster_zoom3():
    """The same grid at zoom 3 at (0, 0) on a 6 x 6 canvas: every cell is a 3 x 3 block; rows 0 .. 2 show grid row 1."""
    keys = {}
    for y in range(3):
        for x in range(3):
            keys[(y, x)], keys[(y, x + 3)], keys[(y + 3, x)] = (3.0, 255), (2.0, 128), (1.0, 0)
    return dict(W=6, H=6, ops=[("raster", dict(grid=GRID, lut=IDENTITY_LUT, lo=1.0, hi=3.0, zoom=3, at=(0, 0)))], keys=keys, flag=False)


def _step(strength, grid, image):
    lut = np.full(256, 200 << 16 | 100 << 8 | 50, np.uint32)
    keys = {(2 - j, i): (float(grid[j, i]), 200 << 16 | 100 << 8 | 50) for j in range(3) for i in range(3) if not np.isnan(grid[j, i])}
    return dict(W=3, H=3, ops=[("raster", dict(grid=grid, lut=lut, lo=0.0, hi=2.0, zoom=1, at=(0, 0)))], keys=keys, flag=False,
                shade=dict(radius=1, strength=strength, background=(9, 8, 7)), image=image)


def shade_step():
    """A 3 x 3 image, every row depths (0, 2, 2), every pixel (200, 100, 50); r = 1, strength = 1.  The corner (0, 0) has 5 neighbours
    outside; inside are (0, 1) = 2 -> 2, (1, 0) = 0 -> 0, (1, 1) = 2 -> 2: o = 4 / 8, shade = 1 / 1.5: floor(133.33 + 0.5) = 133,
    floor(66.67 + 0.5) = 67, floor(33.33 + 0.5) = 33.  (1, 0): three neighbours at 2 -> o = 6 / 8, shade = 1 / 1.75: floor(114.29 + 0.5) =
    114, floor(57.14 + 0.5) = 57, floor(28.57 + 0.5) = 29.  Columns 1 and 2 have nothing in front of them: unchanged."""
    grid = np.array([[0.0, 2.0, 2.0]] * 3)
    image = {(0, 0): (133, 67, 33), (2, 0): (133, 67, 33), (1, 0): (114, 57, 29)}
    image.update({(y, x): (200, 100, 50) for y in range(3) for x in (1, 2)})
    return _step(1.0, grid, image)


def shade_strength0():
    """strength = 0: shade = 1 everywhere, the colours are copied; the NaN cell (grid row 0, column 2 = image pixel (2, 2)) shows the
    background (9, 8, 7)."""
    grid = np.array([[0.0, 2.0, np.nan], [0.0, 2.0, 2.0], [0.0, 2.0, 2.0]])
    image = {(y, x): (200, 100, 50) for y in range(3) for x in range(3)}
    image[(2, 2)] = (9, 8, 7)
    return _step(0.0, grid, image)


CASES = {f.__name__: f for f in (integer_fx, borders_k1, borders_k2, borders_k3, straddle, equal_depth, f32_tie, signed_zero, negative_depth,
                                 view_indices, preset_top, preset_south, preset_north, preset_east, preset_west, labels, scalars, raster_zoom1,
                                 raster_zoom3, shade_step, shade_strength0)}
