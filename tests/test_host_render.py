"""Host tests of the renderer: the numpy restatement against the cases worked by hand, the parameter and command-line checks
(no GPU is touched), cameras, palette and ramps, the C declarations, and the PNG writer read back by a decoder written here."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import render_cases as cases
import render_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"tl_splat": 22, "tl_raster_keys": 13, "tl_render_shade": 9}


def run_restatement(case, order=None):
    keys, flag = np.zeros((case["H"], case["W"]), np.uint64), False
    for op, kw in case["ops"]:
        if op == "raster":
            ref.raster_keys(keys, **kw)
            continue
        kw = dict(kw)
        if order is not None:
            p = order(len(kw["coords"]))
            for k in ("coords", "vid", "attr"):
                if kw.get(k) is not None:
                    kw[k] = kw[k][p]
        flag |= ref.splat(keys, **kw)
    return keys, flag


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_meets_the_hand_cases(name):
    case = cases.CASES[name]()
    for order in (None, lambda n: np.arange(n)[::-1]):
        keys, flag = run_restatement(case, order)
        assert keys.dtype == np.uint64 and np.array_equal(keys, cases.expected_keys(case)), name
        assert flag == case["flag"]
    if "shade" in case:
        out, depth = ref.shade(keys, **case["shade"])
        assert out.dtype == np.uint8 and depth.dtype == np.float32
        for (py, px), rgb in case["image"].items():
            assert tuple(out[py, px]) == rgb, (py, px)
        want = np.full(keys.shape, np.nan, np.float32)
        for (py, px), (d, _) in case["keys"].items():
            want[py, px] = d
        assert np.array_equal(depth, want, equal_nan=True)


def test_restatement_skips_and_flags_what_is_not_finite():
    view = cases.rec((0, 0, 4, 4))
    for xyz in ([[np.nan, 0.0, 0.0]], [[0.0, np.inf, 0.0]], [[0.0, 0.0, 1e39]], [[0.0, 0.0, -1e300]]):
        keys = np.zeros((4, 4), np.uint64)
        assert ref.splat(keys, np.array(xyz), view, size=3) is True and not keys.any()
    keys = np.zeros((4, 4), np.uint64)
    assert ref.splat(keys, np.array([[1e30, 0.0, 0.0]]), view) is False and not keys.any()          # far outside: skipped, no flag
    assert ref.splat(keys, np.zeros((0, 3)), view) is False
    assert 0 not in ref.enc32(np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, -3.4e38], np.float32)).tolist()
    d = np.array([-np.inf, -2.0, -1e-45, 0.0, 1e-45, 2.0, np.inf], np.float32)
    assert (np.diff(ref.enc32(d).astype(np.int64)) > 0).all() and np.array_equal(ref.dec32(ref.enc32(d)), d)


def test_presets_and_view_are_orthonormal():
    from treelearn_amd.util import render
    specs = list(render.PRESETS) + ["oblique", (0, 0), (90, 0), (210, 35), (123.4, -56.7), (0, 90), (37, 89.5)]
    for spec in specs:
        m = np.array(render.view_axes(spec), np.float64)
        assert np.abs(m @ m.T - np.eye(3)).max() <= 1e-15, spec
        assert np.abs(np.cross(m[0], m[1]) - m[2]).max() <= 1e-15, spec             # right-handed: u x v = w
        want = np.array(ref.axes(spec), np.float64)
        assert np.array_equal(m, want), spec
    for name, axes in cases.PRESETS.items():
        assert np.array_equal(np.array(render.PRESETS[name]).reshape(-1), np.array(axes, np.float64)), name
    assert render.view_axes("oblique") == render.view(210, 35) and render.view_axes("210,35") == render.view(210, 35)
    u, v, w = render.view(180, 0)                                                     # a camera in the south looks north: the south preset
    assert np.abs(np.array([u, v, w]) - np.array(render.PRESETS["south"])).max() <= 2e-16
    for bad in ("up", "1,2,3", (1,), (1, float("nan")), None, 5):
        with pytest.raises(ValueError):
            render.view_axes(bad)


def test_fit_view_and_tree_cards():
    from treelearn_amd.util import render
    lo, hi = (-3.0, 1.0, 0.0), (5.0, 7.0, 20.0)
    for spec in ("top", "south", "east", "oblique", (30, 10)):
        got = render.fit_view(spec, lo, hi, (10, 20, 300, 200))
        assert got.shape == (18,) and got.dtype == np.float64 and np.array_equal(got, ref.fit_view(spec, lo, hi, (10, 20, 300, 200)))
        assert got[9:12].tolist() == [1.0, 4.0, 10.0] and got[13:].tolist() == [10.0, 20.0, 300.0, 200.0, 0.0]
    south = render.fit_view("south", lo, hi, (0, 0, 300, 200))
    assert south[12] == min(150 * 0.9 / 4.0, 100 * 0.9 / 10.0)                        # 8 m wide, 20 m tall: the height decides
    assert render.fit_view("top", (1, 1, 1), (1, 1, 1), (0, 0, 8, 8))[12] == 1.0      # a single point
    with pytest.raises(ValueError, match="not finite"):
        render.fit_view("top", (0, 0, 0), (np.inf, 1, 1), (0, 0, 8, 8))
    with pytest.raises(ValueError, match="margin"):
        render.fit_view("top", lo, hi, (0, 0, 8, 8), margin=0.5)
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-20, 20, (400, 3))
    lab = rng.integers(-1, 12, 400)
    lab[lab == 7] = 0                                                                 # tree 7 has no rows
    T = int(lab.max())
    blo = np.array([xyz[lab == t].min(0) if (lab == t).any() else np.full(3, np.inf) for t in range(1, T + 1)])
    bhi = np.array([xyz[lab == t].max(0) if (lab == t).any() else np.full(3, -np.inf) for t in range(1, T + 1)])
    views, (W, H) = render.tree_cards(blo, bhi, cols=4, card=(40, 60))
    want, vid, size = ref.tree_cards(xyz, lab, cols=4, card=(40, 60))
    assert np.array_equal(views, want) and (W, H) == size == (160, 180) and vid.min() == -1
    assert len(set(views[:, 12])) == 1 and views[5, 13:17].tolist() == [40.0, 60.0, 40.0, 60.0]
    assert render.tree_cards(np.zeros((0, 3)), np.zeros((0, 3)))[1] == (8 * 192, 320)


def test_palette_and_ramps():
    from treelearn_amd.util import render
    pal = render.default_palette()
    assert pal.dtype == np.uint32 and pal.shape == (258,) and np.array_equal(pal, ref.default_palette())
    unpack = lambda c: (int(c) >> 16, int(c) >> 8 & 255, int(c) & 255)                # noqa: E731
    assert unpack(pal[0]) == (40, 40, 40) and unpack(pal[1]) == (150, 150, 150) and unpack(pal[2]) == cases.PALETTE_ENTRY_2
    assert len(set(pal.tolist())) > 200 and int(pal.max()) <= 0xFFFFFF
    assert render.default_palette(3).tolist() == pal[:3].tolist()
    with pytest.raises(ValueError):
        render.default_palette(2)
    ends = dict(height=((0, 68, 27), (255, 255, 255)), terrain=((44, 127, 144), (255, 255, 255)), grey=((32, 32, 32), (255, 255, 255)),
                wood=((60, 160, 60), (139, 90, 43)))
    assert set(render.RAMPS) == set(ends) and render.RAMPS == ref.RAMPS
    for name, (first, last) in ends.items():
        r = render.ramp(name)
        assert r.dtype == np.uint32 and r.shape == (256,) and np.array_equal(r, ref.ramp(name)), name
        assert unpack(r[0]) == first and unpack(r[255]) == last, name
    assert unpack(render.ramp("grey")[128]) == ((32 * 127 + 255 * 128 + 127) // 255,) * 3
    mid = render.ramp("height")
    assert unpack(mid[127]) == ((0 * 1 + 255 * 254 + 127) // 255, (68 * 1 + 237 * 254 + 127) // 255, (27 * 1 + 60 * 254 + 127) // 255)
    with pytest.raises(ValueError, match="unknown ramp"):
        render.ramp("jet")
    assert render.parse_color("Blue") == (0, 0, 255) and render.parse_color("#0a10ff") == (10, 16, 255) and render.parse_color((1, 2, 3)) == (1, 2, 3)
    for bad in ("bleu", "#12345", "#12345g", (1, 2), (1, 2, 256), (1.5, 2, 3), None):
        with pytest.raises(ValueError):
            render.parse_color(bad)


def test_check_params():
    from treelearn_amd.util.render import DEFAULTS, check_params
    assert tuple(DEFAULTS) == ("size", "splat", "views", "radius", "strength", "cols", "card", "background")
    got = check_params()
    assert got == DEFAULTS
    assert check_params(dict(size=64.0), splat=9, strength=0, cols=None) == dict(got, size=64, splat=9, strength=0.0)
    assert check_params(views="oblique")["views"] == ("oblique",) and check_params(views=(210, 35))["views"] == ((210.0, 35.0),)
    assert check_params(views=["top", "10,20", (30, 40)])["views"] == ("top", (10.0, 20.0), (30.0, 40.0))
    assert check_params(background="navy", card=[8, 4096])["background"] == (0, 0, 128)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(size=15), dict(size=16385), dict(size=100.5), dict(size=nan), dict(size=True), dict(splat=0), dict(splat=10), dict(radius=0),
                dict(radius=17), dict(strength=-1e-9), dict(strength=inf), dict(strength=nan), dict(strength="dark"), dict(cols=0), dict(cols=257),
                dict(card=(7, 100)), dict(card=(100, 4097)), dict(card=100), dict(card=(1, 2, 3)), dict(views=()), dict(views=("top", "above")),
                dict(views=5), dict(background="nocolour"), dict(background=(0, 0, 300)), dict(colour="label"), dict(width=3)):
        with pytest.raises(ValueError):
            check_params(**bad)
    with pytest.raises(ValueError, match="unknown render parameter"):
        check_params(dict(sizes=1))


def test_module_surface():
    from treelearn_amd.util import render
    for k in ("Canvas", "fit_view", "view", "render_cloud", "render_trees", "render_forest", "juxtapose", "write_png", "check_params", "DEFAULTS"):
        assert k in render.__all__, k
    assert all(hasattr(render, k) for k in render.__all__) and callable(render.add_arguments) and callable(render.params_of) and callable(render.main)
    for k in ("Canvas.", "View record.", "Presets", "Depth and key.", "Footprint.", "Skipped rows.", "Colour of a row.", "Raster to keys.", "Shading.",
              "Parameters", "no CPU fallback"):
        assert k in render.__doc__, k
    import argparse
    import inspect
    ap = argparse.ArgumentParser()
    render.add_arguments(ap, "preview-")
    assert render.check_params(render.params_of(ap.parse_args([]), "preview-")) == render.check_params()
    a = ap.parse_args(["--preview-size", "256", "--preview-views", "top", "210,35", "--preview-splat", "3"])
    assert render.check_params(render.params_of(a, "preview-")) == dict(render.check_params(), size=256, splat=3, views=("top", (210.0, 35.0)))
    assert list(inspect.signature(render.juxtapose).parameters) == ["cloud1", "cloud2", "label1", "label2", "color1", "color2", "subset", "renderer",
                                                                    "size", "opacity", "out"]
    sig = inspect.signature(render.juxtapose).parameters
    assert (sig["color1"].default, sig["color2"].default, sig["subset"].default, sig["size"].default, sig["opacity"].default) == ("blue", "red", 10, 1, 1)


@pytest.mark.parametrize("argv", [
    ["--forest", "missing.npy", "--out", "o"],
    ["--forest", __file__, "--out", "o", "--size", "8"],
    ["--forest", __file__, "--out", "o", "--splat", "10"],
    ["--forest", __file__, "--out", "o", "--views", "above"],
    ["--forest", __file__, "--out", "o", "--color", "depth"],
    ["--forest", __file__, "--out", "o"],                                            # a .py file: an unknown format
    ["--forest", __file__],
    ["--out", "o"],
])
def test_render_command_line_errors(argv, capsys):
    from treelearn_amd.util.render import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err


def test_render_command_line_needs_labels_for_label_colours(tmp_path, capsys):
    from treelearn_amd.util.render import main
    np.save(tmp_path / "c.npy", np.zeros((5, 3)))
    for extra in (["--color", "label"], ["--cards"], ["--color", "hag"]):
        with pytest.raises(SystemExit) as e:
            main(["--forest", str(tmp_path / "c.npy"), "--out", str(tmp_path / "o")] + extra)
        assert e.value.code == 2 and "usage:" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--preview", "--preview-size", "8"], ["--preview-splat", "0"], ["--preview-views", "top", "below"]])
def test_segment_command_line_preview_errors(argv, capsys, tmp_path):
    from treelearn_amd.util.segment import parse_args
    (tmp_path / "w.pth").write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        parse_args(["--forest", __file__, "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)] + argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err


def test_segment_command_line_takes_the_preview_options(tmp_path):
    from treelearn_amd.util.render import params_of
    from treelearn_amd.util.segment import parse_args
    (tmp_path / "w.pth").write_bytes(b"")
    base = ["--forest", __file__, "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    assert parse_args(base).preview is False
    a = parse_args(base + ["--preview", "--preview-size", "300", "--preview-views", "east", "oblique"])
    assert a.preview is True and params_of(a, "preview-") == dict(size=300, splat=2, views=("east", "oblique"))


def test_segment_forest_checks_preview_parameters_first():
    from treelearn_amd.util.segment import segment_forest
    with pytest.raises(ValueError, match="splat"):
        segment_forest(None, None, preview=True, preview_cfg=dict(splat=0))
    with pytest.raises(ValueError, match="unknown render parameter"):
        segment_forest(None, None, preview=True, preview_cfg=dict(colour="label"))


def test_c_declarations_and_prototypes():
    from treelearn_amd import _hip
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    for name, n_args in KERNELS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/treelearn_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _hip.PROTOTYPES and len(_hip.PROTOTYPES[name][1]) == n_args, name
        assert m.group(1).strip().endswith("tl_stream_t stream")
    assert "csrc/tl_render.hip, DESIGN §27" in hdr
    src = open(os.path.join(REPO, "treelearn_amd", "csrc", "tl_render.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "__fma" not in src and "_rn(" not in src
    for call in ("exp", "exp2", "log", "log2", "sin", "cos", "tan", "pow", "sqrt", "rsqrt"):      # no transcendental function on the device
        assert not re.search(r"\b_*%sf?\s*\(" % call, src), call
    product = re.sub(r"#ifdef TL_RENDER_COUNT.*?#else", "", src, flags=re.S)            # (the counting build of tools/dev_render.py aside)
    assert set(re.findall(r"\batomic[A-Z]\w*", product)) == {"atomicMax"}                   # integer maxima only
    assert "tl_splat" in open(os.path.join(REPO, "treelearn_amd", "util", "render.py")).read()


def decode_png(data):
    """A decoder for what write_png writes: 8-bit RGB, no interlace, filter 0 on every row."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        at += 12 + n
    assert at == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, flt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()                                                        # filter byte 0 on every row
    return raw[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (64, 33)])
def test_write_png_round_trip(tmp_path, shape):
    from treelearn_amd.util.render import write_png
    img = np.random.default_rng(shape[0]).integers(0, 256, shape + (3,)).astype(np.uint8)
    path = write_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(decode_png(open(path, "rb").read()), img)
    for bad in (img[:, :, 0], img.astype(np.int32), np.zeros((0, 4, 3), np.uint8), np.zeros((2, 2, 4), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "b.png"), bad)


def test_write_png_is_read_by_pillow(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from treelearn_amd.util.render import write_png
    img = np.random.default_rng(5).integers(0, 256, (19, 23, 3)).astype(np.uint8)
    with Image.open(write_png(str(tmp_path / "a.png"), img)) as im:
        assert im.mode == "RGB" and im.size == (23, 19) and np.array_equal(np.asarray(im), img)
