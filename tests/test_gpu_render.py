"""GPU tests of the renderer: tl_splat, tl_raster_keys and tl_render_shade against the numpy restatement, exact and dtype
included -- every output is a maximum, a selection or a fixed-order f64 formula, so there is no tolerance anywhere --, then the host
interface, segment_forest(preview=True), save_results and both command lines."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_cases as cases
import render_restatement as ref
from test_host_render import decode_png

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TL_ERR_ARG = -1


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def u64(keys):
    return keys.cpu().numpy().view(np.uint64)


def gpu_splat(keys, flags, coords, views, vid=None, mode=0, rgb=0, attr=None, lut=None, lo=0.0, hi=1.0, nan_rgb=0, size=2, n=None):
    """tl_splat called directly, past every host check.  coords: a numpy array or a device tensor [N, 3 or 4] read with its own stride."""
    from treelearn_amd import _hip
    c = coords if torch.is_tensor(coords) else dev(coords)
    v = dev(np.asarray(views, np.float64).reshape(-1, 18))
    a = None if attr is None else dev(attr)
    t = None if lut is None else dev(np.asarray(lut, np.uint32))
    i = None if vid is None else dev(np.asarray(vid, np.int32))
    H, W = keys.shape
    rc = _hip.lib().tl_splat(P(c), int(c.dtype == torch.float64), c.stride(0) if len(c) else 3, len(c) if n is None else n, P(i), P(v), len(v), mode, rgb,
                             P(a), int(a is not None and a.dtype == torch.float64), P(t), 0 if t is None else len(t), lo, hi, nan_rgb, size, P(keys), W,
                             H, P(flags), _hip.stream())
    torch.cuda.synchronize()
    return rc


def gpu_raster(keys, grid, lut, lo, hi, zoom=1, at=(0, 0)):
    from treelearn_amd import _hip
    g = dev(np.asarray(grid, np.float64))
    H, W = keys.shape
    return _hip.lib().tl_raster_keys(P(g), g.shape[1], g.shape[0], zoom, at[0], at[1], P(dev(np.asarray(lut, np.uint32))), lo, hi, P(keys), W, H,
                                     _hip.stream())


def gpu_shade(keys, radius=1, strength=1.0, background=(0, 0, 0)):
    from treelearn_amd import _hip
    H, W = keys.shape
    out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    depth = torch.empty((H, W), dtype=torch.float32, device="cuda")
    assert _hip.lib().tl_render_shade(P(keys), W, H, radius, strength, int(ref.pack(background)), P(out), P(depth), _hip.stream()) == 0
    return out.cpu().numpy(), depth.cpu().numpy()


def canvas(W, H):
    return torch.zeros((H, W), dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


# ------------------------------------------------------------------ the hand cases
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_kernels_meet_the_hand_cases(name):
    case = cases.CASES[name]()
    keys, flags = canvas(case["W"], case["H"])
    for op, kw in case["ops"]:
        assert (gpu_raster(keys, **kw) if op == "raster" else gpu_splat(keys, flags, **kw)) == 0
    assert same(u64(keys), cases.expected_keys(case))
    assert bool(flags[0].item()) == case["flag"] and flags[1:].tolist() == [0, 0, 0]
    if "shade" in case:
        out, depth = gpu_shade(keys, **case["shade"])
        want_out, want_depth = ref.shade(cases.expected_keys(case), **case["shade"])
        assert same(out, want_out) and same(depth, want_depth)
        for (py, px), rgb in case["image"].items():
            assert tuple(out[py, px]) == rgb, (py, px)


# ------------------------------------------------------------------ a random cloud, two viewports
W, H = 96, 64


@pytest.fixture(scope="module")
def cloud():
    """20 000 rows over 12 x 9 x 15 m, of which the last 3 000 repeat earlier rows (same coordinates and view, another label, value and
    colour): depth ties.  View 0 is the top view in the left half of the canvas, view 1 the south view in the right half."""
    rng = np.random.default_rng(11)
    xyz = rng.uniform((-6.0, -4.5, 0.0), (6.0, 4.5, 15.0), (17000, 3))
    vid = rng.integers(0, 2, 17000).astype(np.int32)
    again = rng.integers(0, 17000, 3000)
    xyz, vid = np.concatenate([xyz, xyz[again]]), np.concatenate([vid, vid[again]])
    n = len(xyz)
    labels = rng.integers(-1, 600, n).astype(np.int64)
    values = rng.uniform(-2.0, 17.0, n)
    values[rng.integers(0, n, 200)] = np.nan
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    lo, hi = (-6.0, -4.5, 0.0), (6.0, 4.5, 15.0)
    views = np.stack([ref.fit_view("top", lo, hi, (0, 0, 48, 64)), ref.fit_view("south", lo, hi, (48, 0, 48, 64), margin=0.0)])
    return dict(xyz=xyz, vid=vid, labels=labels, values=values, rgb=rgb, views=views)


def modes_of(c):
    return [dict(mode=0, rgb=0x30A0F0), dict(mode=1, attr=c["labels"], lut=ref.default_palette()),
            dict(mode=2, attr=c["values"], lut=ref.ramp("height"), lo=0.0, hi=15.0, nan_rgb=0x112233),
            dict(mode=2, attr=c["values"].astype(np.float32), lut=ref.ramp("terrain"), lo=0.0, hi=15.0, nan_rgb=0x112233), dict(mode=3, attr=c["rgb"])]


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_splat_matches_the_restatement(cloud, dtype, stride):
    xyz = cloud["xyz"].astype(dtype)
    rows = dev(xyz)
    if stride == 4:
        rows = dev(np.column_stack([xyz, np.full(len(xyz), np.nan, dtype)]))[:, :3]       # the fourth column is never read
    assert rows.stride(0) == stride
    for kw in modes_of(cloud):
        for k in (1, 2, 5):
            keys, flags = canvas(W, H)
            assert gpu_splat(keys, flags, rows, cloud["views"], vid=cloud["vid"], size=k, **kw) == 0
            want = np.zeros((H, W), np.uint64)
            assert ref.splat(want, xyz, cloud["views"], vid=cloud["vid"], size=k, **kw) is False
            assert same(u64(keys), want), (kw["mode"], k)
            assert flags.tolist() == [0, 0, 0, 0] and (want != 0).sum() > 1500
    out, depth = gpu_shade(keys, 2, 0.7, (10, 20, 30))
    want_out, want_depth = ref.shade(want, 2, 0.7, (10, 20, 30))
    assert same(out, want_out) and same(depth, want_depth)


def test_two_row_orders_give_the_same_bits(cloud):
    p = np.random.default_rng(2).permutation(len(cloud["xyz"]))
    for kw in modes_of(cloud):
        a, fa = canvas(W, H)
        b, fb = canvas(W, H)
        assert gpu_splat(a, fa, cloud["xyz"], cloud["views"], vid=cloud["vid"], size=3, **kw) == 0
        kw = dict(kw, attr=None if kw.get("attr") is None else kw["attr"][p])
        assert gpu_splat(b, fb, cloud["xyz"][p], cloud["views"], vid=cloud["vid"][p], size=3, **kw) == 0
        assert torch.equal(a, b)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(gpu_shade(a, 1, 2.0), gpu_shade(b, 1, 2.0)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_many_rows_on_one_pixel(n):
    rng = np.random.default_rng(n)
    xyz = np.column_stack([np.full(n, 0.25), np.full(n, -0.25), rng.integers(0, 40, n) * 0.5]).astype(np.float32)
    lab = rng.integers(1, 9, n).astype(np.int64)
    view = cases.rec((0, 0, 8, 8))
    keys, flags = canvas(8, 8)
    assert gpu_splat(keys, flags, xyz, view, mode=1, attr=lab, lut=ref.default_palette(), size=2) == 0
    want = np.zeros((8, 8), np.uint64)
    ref.splat(want, xyz, view, mode=1, attr=lab, lut=ref.default_palette(), size=2)
    assert same(u64(keys), want) and (want != 0).sum() == 4


# ------------------------------------------------------------------ the host interface
def forest_of_trees(T=300, per_tree=40, seed=4):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-60.0, 60.0, (T, 2))
    height = rng.uniform(4.0, 30.0, T)
    t = np.repeat(np.arange(T), per_tree)
    xyz = np.column_stack([base[t] + rng.normal(0.0, 1.0, (len(t), 2)) * (height[t] / 12.0)[:, None], rng.uniform(0.0, 1.0, len(t)) * height[t]])
    lab = (t + 1).astype(np.int64)
    other = np.column_stack([rng.uniform(-60.0, 60.0, (500, 2)), rng.uniform(0.0, 0.3, 500)])
    return np.concatenate([xyz, other]), np.concatenate([lab, rng.integers(-1, 1, 500)])


def test_contact_sheet_is_one_restatement_per_tree():
    from treelearn_amd.util.render import render_trees
    xyz, lab = forest_of_trees()
    p = np.random.default_rng(0).permutation(len(lab))
    xyz, lab = xyz[p], lab[p]
    got = render_trees(xyz, lab, cols=20, card=(24, 40), splat=2, strength=0.5, background=(5, 5, 5))
    views, vid, (w, h) = ref.tree_cards(xyz, lab, cols=20, card=(24, 40))
    assert (w, h) == (480, 600) and len(views) == 300 and tuple(got.shape) == (h, w, 3) and got.dtype == torch.uint8
    want = np.zeros((h, w), np.uint64)
    for t in range(300):
        rows = lab == t + 1
        card = np.zeros((h, w), np.uint64)
        assert ref.splat(card, xyz[rows], views[t], mode=1, attr=lab[rows], lut=ref.default_palette(), size=2) is False
        x0, y0 = int(views[t, 13]), int(views[t, 14])
        outside = card.copy()
        outside[y0:y0 + 40, x0:x0 + 24] = 0
        assert not outside.any() and card.any()                                       # a tree stays on its own card
        want = np.maximum(want, card)
    assert same(got.cpu().numpy(), ref.shade(want, 1, 0.5, (5, 5, 5))[0])
    assert same(render_trees(xyz[p], lab[p], cols=20, card=(24, 40), splat=2, strength=0.5, background=(5, 5, 5)).cpu().numpy(), got.cpu().numpy())


def test_two_layers_are_one_call_on_the_concatenation(cloud):
    from treelearn_amd.util.render import Canvas
    xyz, lab, views, vid = cloud["xyz"], cloud["labels"], cloud["views"], cloud["vid"]
    half = len(xyz) // 2
    two = Canvas(W, H).splat(xyz[:half], view=views, vid=vid[:half], labels=lab[:half], size=3).splat(xyz[half:], view=views, vid=vid[half:],
                                                                                                   labels=lab[half:], size=3)
    one = Canvas(W, H).splat(torch.from_numpy(xyz).cuda(), view=views, vid=torch.from_numpy(vid).cuda(), labels=torch.from_numpy(lab), size=3)
    assert torch.equal(one.keys, two.keys) and one.keys.dtype == torch.int64
    want = np.zeros((H, W), np.uint64)
    ref.splat(want, xyz, views, vid=vid, mode=1, attr=lab, lut=ref.default_palette(), size=3)
    assert same(u64(one.keys), want)
    img, depth = one.image(radius=2, strength=0.3, return_depth=True)
    want_img, want_depth = ref.shade(want, 2, 0.3)
    assert same(img.cpu().numpy(), want_img) and same(depth.cpu().numpy(), want_depth)
    # values through a named ramp with the default range (the finite extremes), constant colours by name, rgb rows
    v = cloud["values"]
    got = Canvas(W, H).splat(xyz, view=views, vid=vid, values=v, ramp="height", nan_color=(1, 2, 3), size=1).splat(
        xyz[:100], view=views[0], color="#ff8000", size=4).splat(xyz[100:300].astype(np.float32), view=views[1:], rgb=cloud["rgb"][100:300], size=1)
    ref.splat(want := np.zeros((H, W), np.uint64), xyz, views, vid=vid, mode=2, attr=v, lut=ref.ramp("height"), lo=np.nanmin(v), hi=np.nanmax(v),
              nan_rgb=0x010203, size=1)
    ref.splat(want, xyz[:100], views[0], mode=0, rgb=0xFF8000, size=4)
    ref.splat(want, xyz[100:300].astype(np.float32), views[1], mode=3, attr=cloud["rgb"][100:300], size=1)
    assert same(u64(got.keys), want)
    assert not Canvas(W, H).splat(xyz, view=views, vid=vid).clear().keys.any()


@pytest.mark.parametrize("shape,zoom,radius", [((7, 5), 2, 1), ((7, 5), 1, 3), ((80, 80), 1, 1), ((80, 80), 1, 16)])
def test_raster_and_shade(shape, zoom, radius):
    from treelearn_amd.util.render import Canvas
    rng = np.random.default_rng(shape[0] + radius)
    grid = rng.normal(0.0, 3.0, shape)
    grid[rng.uniform(size=shape) < 0.15] = np.nan
    grid[0, 0], grid[-1, -1] = np.nan, -0.0
    ny, nx = shape
    cv = Canvas(nx * zoom + 3, ny * zoom + 2, background=(7, 8, 9)).raster(grid, ramp="terrain", zoom=zoom, at=(3, 1))
    want = np.zeros((ny * zoom + 2, nx * zoom + 3), np.uint64)
    ref.raster_keys(want, grid, ref.ramp("terrain"), np.nanmin(grid), np.nanmax(grid), zoom, (3, 1))
    assert same(u64(cv.keys), want) and (want == 0).sum() > 5 * zoom
    img, depth = cv.image(radius=radius, strength=1.5, return_depth=True)
    want_img, want_depth = ref.shade(want, radius, 1.5, (7, 8, 9))
    assert same(img.cpu().numpy(), want_img) and same(depth.cpu().numpy(), want_depth)
    assert same(cv.image(radius=radius, strength=0.0).cpu().numpy(), ref.shade(want, radius, 0.0, (7, 8, 9))[0])
    with pytest.raises(ValueError, match="leaves the"):
        Canvas(nx * zoom, ny * zoom).raster(grid, ramp="grey", zoom=zoom, at=(1, 0))


def test_the_empty_cloud_and_host_checks():
    from treelearn_amd.util.render import Canvas, juxtapose, render_cloud, render_trees
    bg = np.broadcast_to(np.array([3, 4, 5], np.uint8), (16, 24, 3))
    img, depth = Canvas(24, 16, (3, 4, 5)).splat(np.zeros((0, 3)), view=cases.rec((0, 0, 24, 16)), labels=np.zeros(0, np.int64)).image(return_depth=True)
    assert same(img.cpu().numpy(), np.ascontiguousarray(bg)) and np.isnan(depth.cpu().numpy()).all() and depth.dtype == torch.float32
    got = render_cloud(np.zeros((0, 3), np.float32), np.zeros(0, np.int64), size=16, background=(3, 4, 5))
    assert set(got) == {"top", "south"} and all(same(v.cpu().numpy(), np.ascontiguousarray(bg[:, :16])) for v in got.values())
    assert tuple(render_trees(np.zeros((0, 3)), np.zeros(0, np.int64), cols=3, card=(8, 9)).shape) == (9, 24, 3)
    assert not juxtapose(np.zeros((0, 3)), np.zeros((0, 3)), "a", "b").any()
    cv, one = Canvas(8, 8), np.zeros((1, 3))
    view = cases.rec((0, 0, 8, 8))
    for xyz in ([[np.nan, 0, 0]], [[0, np.inf, 0]], [[0, 0, -np.inf]]):
        with pytest.raises(ValueError, match="not finite"):
            cv.splat(np.array(xyz, np.float64), view=view)
    for bad in (cases.rec((0, 0, 9, 8)), cases.rec((-1, 0, 4, 4)), cases.rec((0, 0, 4.5, 4)), cases.rec((0, 0, 0, 4)), cases.rec((0, 0, 8, 8), s=0.0),
                cases.rec((0, 0, 8, 8), s=np.nan), np.zeros(17), np.zeros((0, 18))):
        with pytest.raises(ValueError):
            cv.splat(one, view=bad)
    for kw in (dict(size=0), dict(size=10), dict(labels=[1, 2]), dict(values=[1.0], lo=2.0, hi=2.0), dict(values=[1.0], ramp="jet"),
               dict(values=[1.0], labels=[1]), dict(color="nocolour"), dict(vid=[0, 0]), dict(labels=[1], palette=[1, 2])):
        with pytest.raises(ValueError):
            cv.splat(one, view=view, **kw)
    with pytest.raises(ValueError, match="need a vid"):
        cv.splat(one, view=np.stack([view, view]))
    with pytest.raises(TypeError):
        cv.splat(np.zeros((1, 3), np.int32), view=view)
    assert not cv.keys.any()
    for kw in (dict(radius=0), dict(radius=17), dict(strength=-1.0), dict(strength=float("nan"))):
        with pytest.raises(ValueError):
            cv.image(**kw)
    # a view index beyond the views passes the host (vid lives on the device) and is reported when the image is taken
    cv.splat(np.zeros((2, 3)), view=view, vid=[0, 1])
    with pytest.raises(ValueError, match="skipped"):
        cv.image()


# ------------------------------------------------------------------ the C entries: refused arguments, zero sizes, skipped rows
def test_entries_refuse_bad_arguments_and_return_on_zero_sizes():
    from treelearn_amd import _hip
    L, s = _hip.lib(), _hip.stream()
    keys, flags = canvas(8, 8)
    pts, view = dev(np.zeros((4, 3))), dev(cases.rec((0, 0, 8, 8)))
    lab, val, lut, pal = dev(np.zeros(4, np.int64)), dev(np.zeros(4)), dev(cases.IDENTITY_LUT), dev(ref.default_palette())
    off = ctypes.c_void_p(pts.data_ptr() + 4)

    def splat(pts=P(pts), f64=1, ld=3, n=4, vid=None, views=P(view), V=1, mode=0, rgb=1, attr=None, af64=0, lut=None, P_=0, lo=0.0, hi=1.0, nan=0, k=1,
              keys=P(keys), W=8, H=8, flags=P(flags)):
        return L.tl_splat(pts, f64, ld, n, vid, views, V, mode, rgb, attr, af64, lut, P_, lo, hi, nan, k, keys, W, H, flags, s)

    assert splat() == 0
    for bad in (dict(pts=None), dict(views=None), dict(keys=None), dict(flags=None), dict(pts=off), dict(f64=2), dict(ld=2), dict(n=-1), dict(V=0),
                dict(mode=-1), dict(mode=4), dict(rgb=1 << 24), dict(nan=1 << 24), dict(k=0), dict(k=10), dict(W=0), dict(H=0), dict(W=16385),
                dict(H=16385), dict(mode=1), dict(mode=1, attr=P(lab)), dict(mode=1, attr=P(lab), lut=P(pal), P_=2), dict(mode=2, attr=P(val), af64=1),
                dict(mode=2, attr=P(val), af64=1, lut=P(lut), P_=255), dict(mode=2, attr=P(val), af64=1, lut=P(lut), P_=256, lo=1.0, hi=1.0),
                dict(mode=2, attr=P(val), af64=1, lut=P(lut), P_=256, lo=2.0, hi=1.0), dict(mode=2, attr=P(val), af64=1, lut=P(lut), P_=256, hi=float("inf")),
                dict(mode=2, attr=P(val), af64=1, lut=P(lut), P_=256, lo=float("nan")), dict(mode=2, attr=P(val), af64=2, lut=P(lut), P_=256),
                dict(mode=3), dict(vid=ctypes.c_void_p(lab.data_ptr() + 2))):
        assert splat(**bad) == TL_ERR_ARG, bad
    assert splat(mode=1, attr=P(lab), lut=P(pal), P_=258) == 0 and splat(mode=2, attr=P(val), af64=1, lut=P(lut), P_=256) == 0
    torch.cuda.synchronize()
    before = keys.clone()
    assert splat(n=0, rgb=0xFFFFFF) == 0                                              # zero rows: nothing is launched, nothing cleared
    assert torch.equal(keys, before) and keys.any() and flags.tolist() == [0, 0, 0, 0]

    grid = dev(np.ones((2, 3)))

    def raster(grid=P(grid), nx=3, ny=2, zoom=1, x0=0, y0=0, lut=P(lut), lo=0.0, hi=1.0, keys=P(keys), W=8, H=8):
        return L.tl_raster_keys(grid, nx, ny, zoom, x0, y0, lut, lo, hi, keys, W, H, s)

    assert raster() == 0 and raster(zoom=2, x0=2, y0=4) == 0
    for bad in (dict(grid=None), dict(lut=None), dict(keys=None), dict(nx=-1), dict(ny=-1), dict(zoom=0), dict(x0=-1), dict(y0=-1), dict(x0=6), dict(y0=7),
                dict(zoom=3), dict(lo=1.0), dict(lo=float("nan")), dict(hi=float("inf")), dict(W=0), dict(H=16385),
                dict(grid=ctypes.c_void_p(grid.data_ptr() + 4))):
        assert raster(**bad) == TL_ERR_ARG, bad
    torch.cuda.synchronize()
    before = keys.clone()
    assert raster(nx=0) == 0 and raster(ny=0) == 0 and torch.equal(keys, before)

    out, depth = torch.empty((8, 8, 3), dtype=torch.uint8, device="cuda"), torch.empty((8, 8), dtype=torch.float32, device="cuda")

    def shade(keys=P(keys), W=8, H=8, r=1, strength=1.0, bg=0, out=P(out), depth=P(depth)):
        return L.tl_render_shade(keys, W, H, r, strength, bg, out, depth, s)

    assert shade() == 0 and shade(depth=None) == 0 and shade(r=16, strength=0.0) == 0
    for bad in (dict(keys=None), dict(out=None), dict(W=0), dict(H=0), dict(W=16385), dict(r=0), dict(r=17), dict(strength=-1.0),
                dict(strength=float("inf")), dict(strength=float("nan")), dict(bg=1 << 24), dict(out=P(keys)), dict(depth=P(keys)), dict(depth=P(out)),
                dict(depth=ctypes.c_void_p(depth.data_ptr() + 2))):
        assert shade(**bad) == TL_ERR_ARG, bad
    torch.cuda.synchronize()


def test_kernel_skips_and_flags_rows_past_the_host_checks():
    view = np.stack([cases.rec((0, 0, 4, 4)), cases.rec((4, 0, 4, 4))])
    xyz = np.array([[0.5, 0.5, 1.0], [np.nan, 0.5, 9.0], [0.5, np.inf, 9.0], [0.5, 0.5, -np.inf], [0.5, 0.5, 1e39], [0.5, 0.5, 2.0], [1e30, 0.5, 9.0]])
    for bad_rows, vid in (([1], [0, 0, -1, -1, -1, 0, 0]), ([2], [0, -1, 1, -1, -1, 0, 0]), ([3, 4], [0, -1, -1, 1, 0, 0, 0]), ([5], [0, -1, -1, -1, -1, 2, 0]),
                          ([], [0, -1, -1, -1, -1, 0, 0])):
        keys, flags = canvas(8, 4)
        assert gpu_splat(keys, flags, xyz, view, vid=vid, mode=0, rgb=7, size=3) == 0
        want = np.zeros((4, 8), np.uint64)
        assert ref.splat(want, xyz, view, vid=vid, mode=0, rgb=7, size=3) is bool(bad_rows)
        assert same(u64(keys), want) and flags.tolist() == [int(bool(bad_rows)), 0, 0, 0], bad_rows
        drawn = ref.dec32((want[want != 0] >> np.uint64(32)).astype(np.uint32))
        assert len(drawn) == 9 and float(drawn.max()) == (1.0 if bad_rows == [5] else 2.0)
    keys, flags = canvas(8, 4)
    flags[0] = 1                                                                      # tl_splat leaves a set flag as it is
    assert gpu_splat(keys, flags, xyz[:1], view[:1]) == 0 and flags.tolist() == [1, 0, 0, 0]


# ------------------------------------------------------------------ pictures of a forest, segment_forest, save_results, the command lines
def _small_plot(labelled=False):
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)
    pts = t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])
    return np.column_stack([pts, t["instance_label"].astype(np.float64)]) if labelled else pts


def _state_dict():
    from treelearn_amd.synth import random_state_dict
    sd = random_state_dict(7, channels=32, num_blocks=7)
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    return sd


def test_render_forest_of_a_labelled_plot():
    """render_forest on a result put together by hand: the labelled 12 m plot, its terrain and canopy, and a wood flag per row."""
    from treelearn_amd.util.canopy import canopy_model
    from treelearn_amd.util.render import render_forest
    from treelearn_amd.util.terrain import terrain_model
    data = _small_plot(labelled=True)
    xyz = torch.from_numpy(data[:, :3] - data[:, :3].mean(0)).cuda()
    lab = torch.from_numpy(data[:, 3].astype(np.int64)).cuda()
    dtm = terrain_model(xyz, lab)
    hag = dtm.height_above_ground(xyz)
    can = canopy_model(xyz, labels=lab, height_above_ground=hag).to_host()
    wood = (data[:, 2] - data[:, 2].min() < 3.0).astype(np.uint8)
    res = dict(coords=xyz, labels=lab, height_above_ground=hag, terrain=dtm.to_host(), canopy=can, inventory=dict(leafwood=dict(wood=wood)))
    got = render_forest(res, size=160, cols=3, card=(48, 80))
    assert set(got) == {"top_labels", "south_labels", "top_height", "dtm", "chm", "leafwood", "trees"}
    assert all(v.dtype == torch.uint8 and v.is_cuda and v.shape[2] == 3 for v in got.values())
    for k in ("top_labels", "south_labels", "top_height", "leafwood"):
        assert tuple(got[k].shape) == (160, 160, 3), k
    assert tuple(got["trees"].shape) == (2 * 80, 3 * 48, 3)
    ny, nx = can["chm"].shape
    zoom = 160 // max(nx, ny)
    assert tuple(got["chm"].shape) == (ny * zoom, nx * zoom, 3) and tuple(got["dtm"].shape) == tuple(np.array(dtm.z.shape) * (160 // max(dtm.z.shape))) + (3,)
    assert len(can["tops_h"]) > 0
    for i, j in zip(can["tops_i"], can["tops_j"]):                                    # every tree top is a white mark on the chm
        assert got["chm"][(ny - 1 - j) * zoom + zoom // 2, i * zoom + zoom // 2].tolist() == [255, 255, 255]
    colours = {tuple(c) for c in got["leafwood"].reshape(-1, 3).unique(dim=0).tolist()}
    assert (0, 0, 0) in colours and len(colours) > 3
    # the top view by labels is the restatement's picture of the same cloud
    c = xyz.cpu().numpy()
    view = ref.fit_view("top", c.min(0), c.max(0), (0, 0, 160, 160))
    ref.splat(want := np.zeros((160, 160), np.uint64), c, view, mode=1, attr=lab.cpu().numpy(), lut=ref.default_palette(), size=2)
    assert same(got["top_labels"].cpu().numpy(), ref.shade(want, 1, 1.0)[0])
    plain = render_forest(dict(coords=c, labels=lab.cpu().numpy()), size=160, cols=3, card=(48, 80))
    assert set(plain) == {"top_labels", "south_labels", "top_height", "trees"} and torch.equal(plain["top_labels"], got["top_labels"])


def test_segment_forest_preview_files_and_command_lines(tmp_path):
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.util.segment import MODEL_CFG, save_results, segment_forest
    pts = _small_plot()
    sd = _state_dict()
    m = TreeLearn(**MODEL_CFG).cuda().eval()
    m.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)
    with torch.no_grad():
        res = segment_forest(pts, m, sample_cfg=dict(stride=1.0), grouping_cfg=cfg, return_type="original", canopy=True, preview=True,
                             preview_cfg=dict(size=128, card=(32, 48)))
    assert set(res) == {"coords", "labels", "categories", "terrain", "height_above_ground", "canopy", "stand", "preview"}
    pre = res["preview"]
    assert set(pre) == {"top_labels", "south_labels", "top_height", "dtm", "chm", "trees"}
    assert all(isinstance(v, np.ndarray) and v.dtype == np.uint8 and v.ndim == 3 and v.shape[2] == 3 for v in pre.values())
    assert pre["top_labels"].shape == (128, 128, 3) and pre["top_labels"].any() and pre["trees"].shape[1] == 8 * 32
    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    assert sorted(os.listdir(tmp_path / "api" / "preview")) == sorted(k + ".png" for k in pre)
    for k, v in pre.items():
        assert same(decode_png(open(tmp_path / "api" / "preview" / (k + ".png"), "rb").read()), v), k
    del res["preview"]
    save_results(res, str(tmp_path / "plain"), "plot", ["npy"], save_treewise=False)
    assert not (tmp_path / "plain" / "preview").exists()

    env = dict(os.environ, PYTHONPATH=REPO)
    forest = tmp_path / "plot.npy"
    np.save(forest, pts)
    torch.save({"net": sd}, tmp_path / "w.pth")
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "treelearn_amd.util.segment", "--forest", str(forest), "--weights",
                        str(tmp_path / "w.pth"), "--out", str(tmp_path / "cli"), "--grouping", "dbscan", "--tau-vert", "0", "--tau-off", "1e9",
                        "--tau-group", "0.3", "--tau-min", "20", "--stride", "1.0", "--no-treewise", "--formats", "npy", "--canopy", "--preview",
                        "--preview-size", "128"], capture_output=True, text=True, cwd=REPO, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "cli" / "preview")) == sorted(k + ".png" for k in pre)
    for k in ("top_labels", "south_labels", "top_height", "dtm", "chm"):              # (the sheet's cards differ in size; shapes, not bits:
        got = decode_png(open(tmp_path / "cli" / "preview" / (k + ".png"), "rb").read())   # another process may group other trees)
        assert got.shape == pre[k].shape and got.any() == pre[k].any(), k


def test_render_command_line(tmp_path):
    from treelearn_amd.util.render import render_cloud
    data = _small_plot(labelled=True)
    forest = tmp_path / "labelled.npy"
    np.save(forest, data)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "treelearn_amd.util.render", "--forest", str(forest), "--out",
                        str(tmp_path / "out"), "--views", "top", "210,35", "--size", "96", "--splat", "1", "--cards", "--canopy"],
                       capture_output=True, text=True, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO))
    assert p.returncode == 0 and "pictures" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    assert sorted(os.listdir(tmp_path / "out")) == ["az210_el35_label.png", "chm.png", "dtm.png", "top_label.png", "trees.png"]
    pts = torch.from_numpy(data).cuda()
    want = render_cloud(pts[:, :3] - pts[:, :3].mean(0), pts[:, 3].to(torch.int64), views=("top", (210, 35)), size=96, splat=1)
    for name, file in (("top", "top_label.png"), ("az210_el35", "az210_el35_label.png")):
        assert same(decode_png(open(tmp_path / "out" / file, "rb").read()), want[name].cpu().numpy()), name
    assert decode_png(open(tmp_path / "out" / "trees.png", "rb").read()).shape == (320, 8 * 192, 3)


def test_juxtapose(tmp_path):
    from treelearn_amd.util.render import juxtapose
    rng = np.random.default_rng(8)
    a = rng.uniform((-5.0, -5.0, 0.0), (0.0, 5.0, 20.0), (4000, 3))
    b = rng.uniform((0.0, -5.0, 0.0), (5.0, 5.0, 10.0), (3000, 3)).astype(np.float32)
    img = juxtapose(a, b, "prediction", "ground truth", out=str(tmp_path / "j.png"))
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (1024, 1024, 3)
    flat = {tuple(c) for c in np.unique(img.reshape(-1, 3), axis=0).tolist()}
    assert (0, 0, 0) in flat and any(c[2] > 0 and c[0] == 0 for c in flat) and any(c[0] > 0 and c[2] == 0 for c in flat)
    assert not img[:512, :512, 0].any() and not img[:512, 512:, 2].any()              # cloud1 (blue) on the left, cloud2 (red) on the right
    assert img[512:, :, 0].any() and img[512:, :, 2].any()                            # both in the overlay
    assert same(decode_png(open(tmp_path / "j.png", "rb").read()), img)
    # every `subset`-th row: the picture is that of the thinned clouds
    lo, hi = np.minimum(a[::10].min(0), b[::10].astype(np.float64).min(0)), np.maximum(a[::10].max(0), b[::10].astype(np.float64).max(0))
    want = np.zeros((1024, 1024), np.uint64)
    for cloud, rgb, spec, vp in ((a, 0x0000FF, "south", (0, 0, 512, 512)), (b, 0xFF0000, "south", (512, 0, 512, 512)), (a, 0x0000FF, "top", (0, 512, 1024, 512)),
                                 (b, 0xFF0000, "top", (0, 512, 1024, 512))):
        ref.splat(want, cloud[::10], ref.fit_view(spec, lo, hi, vp), mode=0, rgb=rgb, size=1)
    assert same(img, ref.shade(want, 1, 1.0)[0])
    two = juxtapose(a, b, "a", "b", color1="#00ff00", color2="orange", subset=1, renderer="notebook", size=3, opacity=0.5)
    assert two[:512, :512, 1].any() and (two != 0).sum() > (img != 0).sum()
    for kw in (dict(color1="bleu"), dict(subset=0), dict(size=0)):
        with pytest.raises(ValueError):
            juxtapose(a, b, "a", "b", **kw)
