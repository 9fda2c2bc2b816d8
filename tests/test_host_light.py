"""Host tests of the light stage: the parameter checks, the direction table, the derived formulas against hand numbers, the
numpy restatement against the cases worked by hand, the C declarations and the command-line parsers.  No GPU is touched."""
import os
import re

import numpy as np
import pytest

import light_cases as cases
import light_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"tl_light_voxels": 16, "tl_light_march": 23}


def test_check_params():
    from treelearn_amd.util.light import DEFAULTS, check_params
    assert DEFAULTS == ref.DEFAULTS
    assert tuple(DEFAULTS) == ("voxel", "sensor_cell", "sensor_height", "n_rings", "n_azimuth", "max_zenith", "max_range", "min_hits",
                               "lai_max_zenith", "zenith_cone")
    got = check_params()
    assert got == DEFAULTS and isinstance(got["n_rings"], int) and isinstance(got["voxel"], float)
    assert check_params(dict(voxel=1), n_rings=3.0, min_hits=None) == dict(got, voxel=1.0, n_rings=3)
    assert check_params(max_zenith=90, zenith_cone=1e-3, sensor_height=-2)["sensor_height"] == -2.0
    inf, nan = float("inf"), float("nan")
    for bad in (dict(voxel=0), dict(voxel=-1.0), dict(voxel=inf), dict(voxel=nan), dict(sensor_cell=0), dict(sensor_cell=nan),
                dict(sensor_height=inf), dict(sensor_height=nan), dict(n_rings=0), dict(n_rings=257), dict(n_rings=2.5), dict(n_rings=True),
                dict(n_azimuth=0), dict(n_azimuth=4097), dict(max_zenith=0), dict(max_zenith=90.5), dict(max_zenith=nan), dict(max_range=0),
                dict(max_range=inf), dict(min_hits=0), dict(min_hits=1.5), dict(lai_max_zenith=0), dict(lai_max_zenith=91), dict(zenith_cone=-1),
                dict(zenith_cone=nan), dict(cell=0.5), dict(rings=9)):
        with pytest.raises(ValueError):
            check_params(**bad)
    with pytest.raises(ValueError, match="unknown light parameter"):
        check_params(dict(voxels=0.25))


@pytest.mark.parametrize("shape", [(9, 36, 90.0), (1, 1, 90.0), (5, 7, 60.0), (18, 72, 80.0)])
def test_sky_directions(shape):
    from treelearn_amd.util.light import sky_directions
    R, A, zmax = shape
    dirs, ring, lo, hi = sky_directions(R, A, zmax)
    want = ref.sky_directions(R, A, zmax)
    assert dirs.shape == (R * A, 3) and dirs.dtype == np.float64 and ring.shape == (R * A,) and ring.dtype == np.int32
    assert lo.shape == hi.shape == (R,) and lo.dtype == hi.dtype == np.float64
    assert np.abs(np.sqrt((dirs * dirs).sum(1)) - 1.0).max() <= 1e-15 and (dirs != 0.0).all() and (dirs[:, 2] > 0).all()
    assert ring.tolist() == [r for r in range(R) for _ in range(A)]
    assert lo[0] == 0.0 and hi[-1] == zmax and np.array_equal(lo[1:], hi[:-1]) and (hi > lo).all()
    zen = np.rad2deg(np.arccos(dirs[:, 2]))
    assert (zen > lo[ring]).all() and (zen < hi[ring]).all()
    w = np.cos(np.deg2rad(lo)) - np.cos(np.deg2rad(hi))
    assert abs(w.sum() - (1.0 - np.cos(np.deg2rad(zmax)))) <= 1e-14              # a telescoping sum of R terms, each rounded once
    for g, x in zip((dirs, ring, lo, hi), want):
        assert g.dtype == x.dtype and np.abs(g - x).max() <= 1e-15
    az = np.rad2deg(np.arctan2(dirs[:A, 1], dirs[:A, 0])) % 360.0
    assert np.abs(az - (np.arange(A) + 0.5) * 360.0 / A).max() <= 1e-9


def test_sky_directions_refusals():
    from treelearn_amd.util.light import check_table, sky_directions
    for bad in ((0, 36, 90.0), (9, 0, 90.0), (9, 36, 0.0), (9, 36, 91.0), (2.5, 36, 90.0)):
        with pytest.raises(ValueError):
            sky_directions(*bad)
    dirs, ring, _, _ = sky_directions(2, 4)
    d, r, R = check_table(dirs, ring, 2)
    assert d.dtype == np.float64 and r.dtype == np.int32 and R == 2
    for bd, br, R in ((dirs * 1.001, ring, 2), (dirs * 0.0, ring, 2), (np.where(np.arange(8)[:, None] == 3, np.nan, dirs), ring, 2), (dirs, ring, 1),
                      (dirs, ring - 1, 2), (dirs[:, :2], ring, 2), (dirs, ring[:3], 2), (dirs * (1.0 + 1e-11), ring, 2)):
        with pytest.raises(ValueError):
            check_table(bd, br, R)
    check_table(dirs * (1.0 + 1e-13), ring, 2)                                       # unit to 1e-12


def _sky():
    from treelearn_amd.util.light import sky_directions
    dirs, ring, lo, hi = sky_directions()
    return np.bincount(ring), lo, hi


def test_derived_all_open_all_blocked_all_side():
    from treelearn_amd.util.light import derive
    rays, lo, hi = _sky()
    counts = np.zeros((9, 4), np.int32)
    counts[:, 1] = rays                                                               # every ray leaves through the top
    d = derive(counts, rays, lo, hi)
    assert d["gap"].tolist() == [1.0] * 9 and d["openness"] == 1.0 and d["lai_e"] == 0.0 and d["gap_zenith"] == 1.0 and d["edge_share"] == 0.0
    counts[:, 1], counts[:, 2] = 20, 16                                               # ... or reaches max_range: as open
    assert derive(counts, rays, lo, hi)["openness"] == 1.0
    blocked = np.zeros((9, 4), np.int32)
    blocked[:, 0] = rays
    d = derive(blocked, rays, lo, hi)
    assert d["gap"].tolist() == [0.0] * 9 and d["openness"] == 0.0 and d["gap_zenith"] == 0.0
    mid = np.deg2rad((lo + hi) / 2.0)[:8]                                             # rings up to 75 degrees: the first eight
    u = np.sin(mid) / np.sin(mid).sum()
    floor = 2.0 * (-np.log(1.0 / 72.0) * np.cos(mid) * u).sum()
    assert abs(d["lai_e"] - floor) <= 1e-12 * floor and 4.5 < floor < 5.5
    side = np.zeros((9, 4), np.int32)
    side[:, 3] = rays
    d = derive(side, rays, lo, hi)
    assert np.isnan(d["gap"]).all() and np.isnan(d["openness"]) and np.isnan(d["lai_e"]) and np.isnan(d["gap_zenith"]) and d["edge_share"] == 1.0


def test_derived_by_hand_and_against_the_restatement():
    from treelearn_amd.util.light import derive
    lo, hi = np.array([0.0, 30.0, 60.0]), np.array([30.0, 60.0, 90.0])
    rays = np.array([4, 4, 4])
    counts = np.array([[1, 2, 1, 0], [2, 0, 0, 2], [0, 0, 0, 4]], np.int32)            # gaps 3/4, 0/2, none
    d = derive(counts, rays, lo, hi, lai_max_zenith=75.0, zenith_cone=60.0)
    assert d["gap"][:2].tolist() == [0.75, 0.0] and np.isnan(d["gap"][2]) and d["edge_share"] == 0.5
    w = np.cos(np.deg2rad(lo)) - np.cos(np.deg2rad(hi))
    assert abs(d["openness"] - 0.75 * w[0] / (w[0] + w[1])) <= 1e-15
    assert d["gap_zenith"] == 3.0 / 6.0                                               # pooled: (2 + 1 + 0) open of (4 + 4 - 2) known
    s15, s45 = np.sin(np.deg2rad(15.0)), np.sin(np.deg2rad(45.0))
    lai = 2.0 * (-np.log(0.75) * np.cos(np.deg2rad(15.0)) * s15 / (s15 + s45) - np.log(1.0 / 8.0) * np.cos(np.deg2rad(45.0)) * s45 / (s15 + s45))
    assert abs(d["lai_e"] - lai) <= 1e-12 * lai
    assert derive(counts, rays, lo, hi, zenith_cone=20.0)["gap_zenith"] != derive(counts, rays, lo, hi, zenith_cone=20.0)["gap_zenith"]   # no ring: NaN
    # stacked counts, and every value against the restatement
    rng = np.random.default_rng(3)
    sky_rays, slo, shi = _sky()
    many = np.zeros((50, 9, 4), np.int64)
    for i in range(50):
        for r in range(9):
            many[i, r] = rng.multinomial(36, rng.dirichlet([0.5] * 4))
    many[0, :, :] = 0; many[0, :, 3] = 36                                              # all lost through a side
    many[1, :, 3] = 0; many[1, :, 0] = 36 - many[1, :, 1] - many[1, :, 2]
    got = derive(many, sky_rays, slo, shi)
    assert got["gap"].shape == (50, 9) and got["openness"].shape == (50,)
    for i in range(50):
        want = ref.derive(many[i], sky_rays, slo, shi)
        for k in ("gap", "openness", "lai_e", "gap_zenith", "edge_share"):
            a, b = np.asarray(got[k][i], np.float64), np.asarray(want[k], np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (i, k)
            ok = ~np.isnan(b)
            assert (np.abs(a[ok] - b[ok]) <= 1e-12 * np.abs(b[ok])).all(), (i, k)
    per_tree = derive(many[:2].sum(0), 2 * sky_rays, slo, shi)                         # pooled over two columns: twice the rays per ring
    assert per_tree["edge_share"] == many[:2, :, 3].sum() / (2.0 * 324.0)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_meets_the_hand_cases(name):
    from treelearn_amd.util import light
    assert (light.DEFAULTS, light.MAX_SIDE, light.MAX_VOXELS, light.MAX_OWNED) == (ref.DEFAULTS, ref.MAX_SIDE, ref.MAX_VOXELS, ref.MAX_OWNED)
    case = cases.CASES[name]()
    vox = ref.light_voxels(case["xyz"], case["labels"], case["voxel"])
    assert vox["n"] == [9, 9, 9] and vox["i0"] == [0, 0, 0] and vox["occ"].shape == (9, 9, 1) and vox["occ"].dtype == np.uint32
    assert (vox["owner"] is None) == (case["labels"] is None)
    res = ref.march(vox, case["origins"], case["dirs"], case["ring"], case["n_rings"], case["skip"], case["max_range"], case["min_hits"])
    assert res["counts"].dtype == np.int32 and res["code"].dtype == np.uint8 and res["first"].dtype == np.float64 and res["status"].dtype == np.int32
    case["check"](res)
    # float32 coordinates of the same voxels, a fourth column and another row order change nothing
    wide = np.column_stack([case["xyz"], np.full(len(case["xyz"]), 7.0)]).astype(np.float32)
    p = np.random.default_rng(1).permutation(len(wide))
    vox2 = ref.light_voxels(wide[p], None if case["labels"] is None else case["labels"][p], case["voxel"])
    assert np.array_equal(vox2["occ"], vox["occ"]) and (vox["owner"] is None or np.array_equal(vox2["owner"], vox["owner"]))


def test_restatement_grid_words_owner_and_refusals():
    from treelearn_amd.util import light
    assert (light.MAX_SIDE, light.MAX_VOXELS, light.MAX_OWNED) == (ref.MAX_SIDE, ref.MAX_VOXELS, ref.MAX_OWNED) and light.CODES[3] == "side"
    xyz = np.array([[-0.3, 0.1, 5.0], [8.2, 0.1, 5.0], [8.2, 0.3, 5.1], [7.5, 0.2, 5.2], [0.0, 0.6, 5.6]])
    vox = ref.light_voxels(xyz, np.array([4, 2, 7, -3, 0]), 0.25)
    assert vox["i0"] == [-2, 0, 20] and vox["n"] == [35, 3, 3] and vox["occ"].shape == (3, 3, 2)
    assert vox["occ"][0, 0].tolist() == [1, (1 << 2) | (1 << 0)] and vox["occ"][0, 1].tolist() == [0, 1 << 2] and vox["occ"][2, 2].tolist() == [1 << 2, 0]
    assert vox["owner"][0, 0, 0] == 4 and vox["owner"][0, 0, 34] == 2 and vox["owner"][0, 1, 34] == 7 and vox["owner"][0, 0, 32] == -1
    assert vox["owner"][2, 2, 2] == 0 and (vox["owner"] >= -1).all() and int(vox["full"].sum()) == 5
    empty = ref.light_voxels(np.zeros((0, 3)), None, 0.25)
    assert empty["n"] == [0, 0, 0] and empty["occ"].shape == (0, 0, 0)
    out = ref.march(empty, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [0], 1)
    assert out["status"].tolist() == [1] and out["counts"].tolist() == [[[0, 0, 0, 0]]]
    with pytest.raises(ValueError):
        ref.light_voxels(np.array([[0.0, np.nan, 0.0]]), None, 0.25)
    with pytest.raises(ValueError):
        ref.light_voxels(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), None, 1e-4)


def test_module_surface_and_argument_parsers(capsys):
    import argparse
    from treelearn_amd.util import inventory, light, segment
    assert all(hasattr(light, k) for k in light.__all__) and callable(light.add_arguments) and callable(light.params_of)
    assert light.LIGHT_COLUMNS == ("light_columns", "light_openness", "light_gap_zenith", "light_lai_above", "light_edge_share")
    for k in ("Parameters", "Voxel grid.", "Direction table.", "The walk", "Derived", "Users.", "no CPU fallback"):
        assert k in light.__doc__, k
    ap = argparse.ArgumentParser()
    light.add_arguments(ap)
    assert light.check_params(light.params_of(ap.parse_args([]))) == light.check_params()
    a = ap.parse_args(["--light-voxel", "0.5", "--sensor-cell", "4", "--sensor-height", "2", "--rings", "6", "--azimuths", "24", "--max-range", "40"])
    assert light.params_of(a) == dict(light.DEFAULTS, voxel=0.5, sensor_cell=4.0, sensor_height=2.0, n_rings=6, n_azimuth=24, max_range=40.0)
    for argv in (["--forest", "missing.npy", "--out", "o.npz"], ["--forest", __file__, "--out", "o.npz", "--light-voxel", "0"],
                 ["--forest", __file__, "--out", "o.npz", "--rings", "0"], ["--forest", __file__, "--out", "o.npz", "--hemi", "1,2"],
                 ["--forest", __file__, "--out", "o.npz", "--hemi", "1", "--hemi-out", "s.png"], ["--forest", __file__, "--out", "o.npz"],
                 ["--forest", __file__], ["--out", "o.npz"]):
        with pytest.raises(SystemExit) as e:
            light.main(argv)
        assert e.value.code == 2 and "usage:" in capsys.readouterr().err
    with pytest.raises(ValueError, match="unknown light parameter"):
        segment.segment_forest(None, None, light=True, light_cfg=dict(cell=3))
    with pytest.raises(ValueError, match="voxel"):
        inventory.tree_inventory(None, None, light=True, light_cfg=dict(voxel=0.0))
    with pytest.raises(ValueError, match="max_range"):
        inventory.cloud_inventory(np.zeros((1, 4)), light=True, light_cfg=dict(max_range=-1.0))


def test_segment_and_inventory_command_lines_take_the_flag(capsys, tmp_path):
    from treelearn_amd.util.segment import parse_args
    (tmp_path / "w.pth").write_bytes(b"")
    base = ["--forest", __file__, "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    a = parse_args(base + ["--light", "--rings", "5"])
    assert a.light and a.light_n_rings == 5 and not parse_args(base).light
    with pytest.raises(SystemExit) as e:
        parse_args(base + ["--light", "--light-voxel", "-1"])
    assert e.value.code == 2 and "usage:" in capsys.readouterr().err
    from treelearn_amd.util import inventory
    with pytest.raises(SystemExit) as e:
        inventory.main(["--forest", __file__, "--out", "o.csv", "--light", "--azimuths", "0"])
    assert e.value.code == 2 and "usage:" in capsys.readouterr().err


def test_write_inventory_puts_the_light_columns_last(tmp_path):
    from treelearn_amd.util.inventory import COLUMNS, INT_COLUMNS, write_inventory
    from treelearn_amd.util.light import LIGHT_COLUMNS
    inv = {k: (np.array([1, 2]) if k in INT_COLUMNS else np.array([0.5, np.nan])) for k in COLUMNS}
    inv.update(light_columns=np.array([12, 0]), light_openness=np.array([0.25, np.nan]), light_gap_zenith=np.array([1.0, np.nan]),
               light_lai_above=np.array([0.1, np.nan]), light_edge_share=np.array([0.0, np.nan]))
    write_inventory(str(tmp_path / "t.csv"), inv)
    rows = open(tmp_path / "t.csv").read().splitlines()
    assert rows[0].split(",") == list(COLUMNS + LIGHT_COLUMNS) and rows[1].split(",")[-5:] == ["12", "0.25", "1.0", "0.1", "0.0"]
    assert rows[2].split(",")[-5:] == ["0", "nan", "nan", "nan", "nan"]
    plain = {k: inv[k] for k in COLUMNS}
    write_inventory(str(tmp_path / "p.csv"), plain)
    assert open(tmp_path / "p.csv").read().splitlines()[0].split(",") == list(COLUMNS)


def test_write_light_round_trip(tmp_path):
    from treelearn_amd.util.light import write_light
    d = dict(voxel=np.float64(0.25), occ=np.array([[[5]]], np.uint32), openness=np.array([[0.5, np.nan]]), n_outside=np.int64(1))
    write_light(str(tmp_path / "l.npz"), d)
    with np.load(tmp_path / "l.npz") as f:
        assert set(f.files) == set(d) and all(np.array_equal(f[k], d[k], equal_nan=f[k].dtype.kind == "f") and f[k].dtype == d[k].dtype for k in d)


def test_c_declarations_and_prototypes():
    from treelearn_amd import _hip
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    for name, n_args in KERNELS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/treelearn_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _hip.PROTOTYPES and len(_hip.PROTOTYPES[name][1]) == n_args, name
        assert m.group(1).strip().endswith("tl_stream_t stream")
    assert "csrc/tl_light.hip, DESIGN §28" in hdr
    src = open(os.path.join(REPO, "treelearn_amd", "csrc", "tl_light.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "__fma" not in src and "_rn(" not in src
    assert "atomicOr" in src and "atomicMax" in src and "__ballot" in src and "__popcll" in src
    from treelearn_amd import build as b
    import ctypes
    L = ctypes.CDLL(b.build(verbose=False))
    assert all(hasattr(L, k) for k in KERNELS)
