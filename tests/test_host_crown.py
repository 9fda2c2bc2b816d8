"""Host tests of the crown structure: the numpy restatement against cases worked by hand (tests/crown_cases.py), the parameter
checks that come before any GPU work, the CSV and .npz writers and the two entry points of the built library.  The kernels are held to
the restatement in tests/test_gpu_crown.py."""
import csv
import ctypes
import os

import numpy as np
import pytest

import crown_cases as cases
import crown_restatement as ref
import inventory_restatement as inv_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(case, **kw):
    """A hand case through the restatement (with the case's z_ref in place of z_low where it sets one)."""
    if "z_ref" not in case:
        return ref.tree_crowns(case["xyz"], case["lab"], crown_cfg=case["cfg"], **kw)
    base = inv_ref.tree_inventory(case["xyz"], case["lab"])
    res = dict(base)
    res.update(ref.crown_structure(case["xyz"], case["lab"], base["x"], base["y"], case["z_ref"], base["z_top"], **case["cfg"]))
    return res


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_hand_cases(name):
    case = cases.CASES[name]()
    res = restated(case)
    assert tuple(res)[:16] == inv_ref.COLUMNS and tuple(res)[16:] == ref.CROWN_COLUMNS + ("crown_profile", "L_t", "margins")
    assert tuple(res["crown_profile"]) == ref.PROFILE_KEYS and tuple(res["margins"]) == ref.MARGIN_KINDS
    case["check"](res)
    T, L = len(res["tree_id"]), res["crown_profile"]["h"].shape[1]
    assert L == (int(res["L_t"].max()) if T else 0) and np.array_equal(res["L_t"], res["crown_layers"])
    layer = dict(ref.CROWN_DEFAULTS, **case["cfg"])["layer"]
    for t in range(T):                                               # h is a layer's bottom where the tree has the layer, NaN beyond
        Lt = int(res["L_t"][t])
        assert np.array_equal(res["crown_profile"]["h"][t, :Lt], np.arange(Lt) * layer) and np.isnan(res["crown_profile"]["h"][t, Lt:]).all()
        assert (res["crown_profile"]["n"][t, Lt:] == 0).all() and (res["crown_profile"]["cells"][t, Lt:] == 0).all()
        assert (res["crown_profile"]["cells"][t] <= res["crown_profile"]["n"][t]).all()
    # the positions are the anchor centres exactly: every implementation starts from the same bits (crown_cases.py)
    has = res["n_points"] > 0
    assert np.array_equal(res["x"][has] * 8 % 1, np.zeros(has.sum())) and np.array_equal(res["y"][has] * 8 % 1, np.zeros(has.sum()))
    # float32 input with a row stride of 4 is the same cloud once widened
    x4 = np.zeros((len(case["xyz"]), 4), np.float32)
    x4[:, :3] = case["xyz"]
    a, b = restated(dict(case, xyz=x4[:, :3])), restated(dict(case, xyz=x4[:, :3].astype(np.float64)))
    for k in ref.CROWN_COLUMNS:
        assert np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], res[k], equal_nan=True), k


def test_restatement_margins_and_sectors():
    """A lollipop moved off the lattice: the sector margin is the smallest distance of a projection cell from a sector border."""
    case = cases.CASES["lollipop"]()
    xyz = case["xyz"] + np.array([0.0625 + 0.001, 0.0625 - 0.002, 0.0])       # the cells stay, the position moves inside its cell
    res = ref.tree_crowns(xyz, case["lab"])
    assert res["crown_proj_cells"][0] == 16 and res["crown_voxels"][0] == 64 and res["margins"]["layer"] == np.inf and res["margins"]["anchor"] == np.inf
    u = (np.arange(10, 14) + 0.5) * 0.25 - res["x"][0]
    v = (np.arange(-10, -6) + 0.5) * 0.25 - res["y"][0]
    want = min(min(abs(a), abs(b), abs(abs(a) - abs(b))) for a in u for b in v)
    assert res["margins"]["sector"] == want and 0.0005 < want < 0.0635
    assert [ref.sector(*p) for p in ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1), (-1, 0), (-2, -1), (-1, -1), (-1, -2),
                                     (0, -1), (1, -2), (1, -1), (2, -1), (0, 0))] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 0]
    # with a reference height that is not a rank of the rows, the layer margin is reported
    base = inv_ref.tree_inventory(xyz, case["lab"])
    low = ref.crown_structure(xyz, case["lab"], base["x"], base["y"], base["z_low"] - 0.01, base["z_top"])
    assert abs(low["margins"]["layer"] - 0.02) < 1e-12 and low["crown_layers"][0] == 12


def test_restatement_offset_moves_the_centroid_only():
    case = cases.CASES["label_gap"]()
    off = np.array([1000.0, 2000.0, 50.0])
    plain, moved = restated(case), restated(case, offset=off)
    for k in ref.CROWN_COLUMNS:
        want = plain[k] + off[0] if k == "crown_x" else plain[k] + off[1] if k == "crown_y" else plain[k]
        assert np.array_equal(moved[k], want, equal_nan=True), k
    for k in ref.PROFILE_KEYS:
        assert np.array_equal(moved["crown_profile"][k], plain["crown_profile"][k], equal_nan=True), k
    assert np.array_equal(moved["x"], plain["x"] + off[0], equal_nan=True)      # the inventory's own columns still move as before


def test_restatement_errors():
    case = cases.CASES["lollipop"]()
    far = lambda ix: np.concatenate([case["xyz"], [[(ix + 0.5) / 4, -1.875, 4.25]]])          # noqa: E731  one more row in layer 8
    lab = np.concatenate([case["lab"], [1]])
    for ix in (12 - 4096, 12 + 4095):                                    # the last cells the key can hold
        res = ref.tree_crowns(far(ix), lab)
        assert res["crown_proj_cells"][0] == 17 and res["margins"]["anchor"] == 0.5
    for ix in (12 - 4097, 12 + 4096):
        with pytest.raises(ValueError):
            ref.tree_crowns(far(ix), lab)
    bad = case["xyz"].copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        ref.crown_structure(bad, case["lab"], [3.125], [-1.875], [0.0], [5.75])
    with pytest.raises(ValueError, match="unknown crown parameter"):
        ref.crown_structure(case["xyz"], case["lab"], [3.125], [-1.875], [0.0], [5.75], layers=3)


def test_check_params():
    from treelearn_amd.util.crown import CROWN_COLUMNS, CROWN_DEFAULTS, CROWN_INT_COLUMNS, PROFILE_KEYS, check_params
    assert CROWN_DEFAULTS == ref.CROWN_DEFAULTS and CROWN_COLUMNS == ref.CROWN_COLUMNS and CROWN_INT_COLUMNS == ref.CROWN_INT
    assert PROFILE_KEYS == ref.PROFILE_KEYS
    assert CROWN_DEFAULTS == dict(layer=0.5, cell=0.25, max_layers=256, min_height=1.0, base_percent=10, max_gap=1)
    assert CROWN_COLUMNS == ("crown_layers", "crown_base_h", "crown_length", "crown_ratio", "crown_widest_h", "crown_voxels", "crown_volume",
                             "crown_proj_cells", "crown_proj_area", "crown_x", "crown_y", "crown_offset", "crown_radius_max", "crown_radius_mean")
    assert check_params() == CROWN_DEFAULTS and check_params(dict(layer=1.0), cell=None)["layer"] == 1.0
    assert check_params(max_layers=256.0)["max_layers"] == 256 and check_params(min_height=0, max_gap=0, base_percent=100, max_layers=1)["max_gap"] == 0
    assert isinstance(check_params(layer=1)["layer"], float) and isinstance(check_params(base_percent=5.0)["base_percent"], int)
    bad = [dict(layer=0.0), dict(layer=-1.0), dict(cell=0.0), dict(max_layers=0), dict(max_layers=257), dict(max_layers=2.5), dict(min_height=-0.1),
           dict(base_percent=0), dict(base_percent=101), dict(base_percent=9.5), dict(max_gap=-1), dict(max_gap=0.5), dict(layer=float("nan")),
           dict(cell=float("inf")), dict(min_height=float("inf")), dict(max_layers=float("nan")), dict(max_gap=True)]
    for b in bad:
        with pytest.raises(ValueError):
            check_params(b)
        with pytest.raises(ValueError):
            check_params(**b)
    with pytest.raises(ValueError, match="unknown crown parameter"):
        check_params(dict(layers=0.5))


def test_argument_validation_before_any_gpu_work():
    from treelearn_amd.util.inventory import cloud_inventory, tree_inventory
    from treelearn_amd.util.segment import segment_forest
    xyz, lab = np.zeros((4, 3)), np.ones(4, np.int64)
    for b in (dict(layer=0.0), dict(base_percent=0), dict(nope=1)):
        with pytest.raises(ValueError):
            tree_inventory(xyz, lab, crown=True, crown_cfg=b)
        with pytest.raises(ValueError):
            cloud_inventory(np.zeros((4, 4)), crown=True, crown_cfg=b)
        with pytest.raises(ValueError):                              # before the model or the points are looked at
            segment_forest(None, None, crown=True, crown_cfg=b)


def test_command_lines_refuse_bad_parameters(tmp_path):
    from treelearn_amd.util import crown, inventory, segment, stem
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 4)))
    with pytest.raises(SystemExit):
        crown.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--crown-layer", "0"])
    with pytest.raises(SystemExit):
        crown.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--crown-base-percent", "101"])
    with pytest.raises(SystemExit):
        crown.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--crown-cell", "0"])
    with pytest.raises(SystemExit):
        crown.main(["--forest", str(tmp_path / "missing.npy"), "--out", str(tmp_path / "o.npz")])
    with pytest.raises(SystemExit):
        crown.main(["--forest", str(forest)])
    with pytest.raises(SystemExit):
        inventory.main(["--forest", str(forest), "--out", str(tmp_path / "o.csv"), "--crown", "--crown-max-layers", "300"])
    with pytest.raises(SystemExit):
        stem.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--crown", "--crown-max-gap", "-1"])
    (tmp_path / "w.pth").write_bytes(b"")
    common = ["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    with pytest.raises(SystemExit):
        segment.parse_args(common + ["--crown", "--crown-min-height", "-2"])
    a = segment.parse_args(common + ["--crown", "--crown-layer", "0.25", "--crown-max-gap", "2", "--crown-cell", "0.5"])
    assert a.crown and crown.params_of(a) == dict(crown.CROWN_DEFAULTS, layer=0.25, max_gap=2, cell=0.5)
    assert inventory.params_of(a)["crown_cell"] == 0.5                   # one --crown-cell: the crown cover of the inventory and this stage
    assert not segment.parse_args(common).crown and crown.params_of(segment.parse_args(common)) == crown.CROWN_DEFAULTS
    assert not (tmp_path / "o.npz").exists() and not (tmp_path / "o.csv").exists()


def _reference_csv(path, inv, columns, ints):
    """The CSV format of util.inventory.write_inventory, written independently: repr floats, str ints."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(list(columns))
        for i in range(len(inv["tree_id"])):
            w.writerow([str(int(inv[k][i])) if k in ints else repr(float(inv[k][i])) for k in columns])


def test_write_inventory_with_and_without_crown_columns(tmp_path):
    from treelearn_amd.util.crown import CROWN_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, INT_COLUMNS, write_inventory
    res = restated(cases.CASES["label_gap"]())
    plain = {k: res[k] for k in COLUMNS}
    # without the crown columns: the bytes of before (the format written out by hand here)
    _reference_csv(tmp_path / "want.csv", plain, COLUMNS, INT_COLUMNS)
    assert open(write_inventory(str(tmp_path / "plain.csv"), plain), "rb").read() == (tmp_path / "want.csv").read_bytes()
    partial = dict(plain, crown_layers=res["crown_layers"], crown_profile=res["crown_profile"])    # not all fourteen: none is written
    assert open(write_inventory(str(tmp_path / "partial.csv"), partial), "rb").read() == (tmp_path / "want.csv").read_bytes()
    # with them: appended after the sixteen, the three counts as integers, floats read back to the same bits
    rows = list(csv.reader(open(write_inventory(str(tmp_path / "crown.csv"), res), newline="")))
    assert rows[0] == list(COLUMNS + CROWN_COLUMNS) and len(rows) == 1 + 3
    old = list(csv.reader(open(tmp_path / "want.csv", newline="")))
    for i, row in enumerate(rows[1:]):
        assert row[:16] == old[1 + i]
        for k, cell in zip(CROWN_COLUMNS, row[16:]):
            if k in ref.CROWN_INT:
                assert cell == str(int(res[k][i])), k
            else:
                assert cell == "nan" if np.isnan(res[k][i]) else float(cell) == res[k][i], k
    assert [r[16] for r in rows[1:]] == ["12", "0", "10"] and [r[21] for r in rows[1:]] == ["64", "0", "32"] and [r[23] for r in rows[1:]] == ["16", "0", "16"]


def test_write_crown_profiles_round_trip(tmp_path):
    from treelearn_amd.util.crown import PROFILE_KEYS, write_crown_profiles
    res = restated(cases.CASES["label_gap"](), offset=[0.1, 1e6 / 3, -7e-5])
    path = write_crown_profiles(str(tmp_path / "crowns.npz"), res)
    with np.load(path) as f:
        assert set(f.files) == {"tree_id"} | set(PROFILE_KEYS)
        assert f["tree_id"].tolist() == [1, 2, 3] and f["tree_id"].dtype == np.int64
        for k in PROFILE_KEYS:
            assert f[k].shape == ((3, 8) if k == "radii" else (3, 12)) and f[k].dtype == res["crown_profile"][k].dtype
            assert f[k].tobytes() == res["crown_profile"][k].tobytes(), k
    with pytest.raises(ValueError):
        write_crown_profiles(str(tmp_path / "none.npz"), inv_ref.tree_inventory(np.zeros((2, 3)), np.ones(2, np.int64)))
    e = restated(cases.CASES["no_trees"]())
    with np.load(write_crown_profiles(str(tmp_path / "e.npz"), e)) as f:
        assert f["tree_id"].shape == (0,) and f["h"].shape == (0, 0) and f["radii"].shape == (0, 8)


def test_library_exports_the_crown_entry_points():
    """Both symbols are exported and bound, refuse nulls and bad parameters before anything else, and return TL_OK without a launch for
    nothing to do (no GPU is needed to find that out)."""
    from treelearn_amd import _hip, build as b
    from treelearn_amd.util.crown import check_params
    L = ctypes.CDLL(b.build(verbose=False))
    assert hasattr(L, "tl_crown_voxel_keys") and hasattr(L, "tl_crown_structure")
    assert len(_hip.PROTOTYPES["tl_crown_voxel_keys"][1]) == 9 and len(_hip.PROTOTYPES["tl_crown_structure"][1]) == 13
    assert [f[0] for f in _hip.CrownParams._fields_] == ["layer", "cell", "min_height", "max_layers", "base_percent", "max_gap"]
    assert ctypes.sizeof(_hip.CrownParams) == 48
    lib = _hip.lib()
    good = _hip.CrownParams(**check_params())
    buf = (ctypes.c_double * 64)()                                   # host memory: only its address and alignment are looked at
    p, odd = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(ctypes.addressof(buf) + 4)
    odd2 = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    keys = lambda *a: lib.tl_crown_voxel_keys(*a, None)              # noqa: E731
    struct = lambda *a: lib.tl_crown_structure(*a, None)             # noqa: E731
    # nothing to do, found out after the argument checks and without a launch
    assert struct(p, 0, p, p, 0, 2, good, p, p, p, p, p) == _hip.TL_OK and struct(p, 0, p, p, 3, 0, good, p, p, p, p, p) == _hip.TL_OK
    assert keys(p, p, 0, p, 3, good, p, p) == _hip.TL_OK and keys(p, p, 5, p, 0, good, p, p) == _hip.TL_OK
    assert struct(p, 5, p, p, 3, 256, good, p, p, p, p, None) == _hip.TL_ERR_ARG
    assert keys(None, p, 0, p, 3, good, p, p) == _hip.TL_ERR_ARG and keys(p, p, 0, p, 3, None, p, p) == _hip.TL_ERR_ARG
    assert keys(p, odd, 0, p, 3, good, p, p) == _hip.TL_ERR_ARG and keys(p, p, -1, p, 3, good, p, p) == _hip.TL_ERR_ARG
    assert keys(p, p, 0, p, 3, good, p, None) == _hip.TL_ERR_ARG and keys(p, p, 0, p, 3, good, p, odd2) == _hip.TL_ERR_ARG
    assert keys(p, p, 0, p, -1, good, p, p) == _hip.TL_ERR_ARG and keys(p, p, 0, p, 1 << 21, good, p, p) == _hip.TL_ERR_ARG
    assert struct(None, 0, p, p, 0, 2, good, p, p, p, p, p) == _hip.TL_ERR_ARG and struct(p, 0, p, odd, 0, 2, good, p, p, p, p, p) == _hip.TL_ERR_ARG
    assert struct(p, -1, p, p, 0, 2, good, p, p, p, p, p) == _hip.TL_ERR_ARG and struct(p, 0, p, p, -1, 2, good, p, p, p, p, p) == _hip.TL_ERR_ARG
    assert struct(p, 0, p, p, 0, -1, good, p, p, p, p, p) == _hip.TL_ERR_ARG and struct(p, 0, p, p, 0, 2, None, p, p, p, p, p) == _hip.TL_ERR_ARG
    assert struct(p, 0, p, p, 0, 257, good, p, p, p, p, p) == _hip.TL_ERR_ARG     # a profile wider than max_layers
    small = _hip.CrownParams(**check_params(max_layers=10))
    assert struct(p, 0, p, p, 0, 10, small, p, p, p, p, p) == _hip.TL_OK and struct(p, 0, p, p, 0, 11, small, p, p, p, p, p) == _hip.TL_ERR_ARG
    for bad in (dict(layer=0.0), dict(layer=float("nan")), dict(cell=-1.0), dict(cell=float("inf")), dict(min_height=-0.5), dict(min_height=float("nan")),
                dict(max_layers=0), dict(max_layers=257), dict(base_percent=0), dict(base_percent=101), dict(max_gap=-1)):
        with pytest.raises(ValueError):
            check_params(bad)                                        # the host check and the library's agree
        cp = _hip.CrownParams(**dict(check_params(), **bad))
        assert keys(p, p, 0, p, 3, cp, p, p) == _hip.TL_ERR_ARG and struct(p, 0, p, p, 0, 2, cp, p, p, p, p, p) == _hip.TL_ERR_ARG, bad
