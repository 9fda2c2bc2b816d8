"""Host tests of the stem profiles: the numpy restatement against cases worked by hand (tests/stem_cases.py), the parameter
checks that come before any GPU work, the CSV and .npz writers and the two entry points of the built library.  The kernels are held to
the restatement in tests/test_gpu_stem.py."""
import csv
import ctypes
import os

import numpy as np
import pytest

import inventory_restatement as inv_ref
import stem_cases as cases
import stem_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(case, **kw):
    """A hand case through the restatement (with the case's z_ref in place of z_low where it sets one)."""
    if "z_ref" not in case:
        return ref.tree_stems(case["xyz"], case["lab"], stem_cfg=case["cfg"], **kw)
    base = inv_ref.tree_inventory(case["xyz"], case["lab"])
    res = dict(base)
    res.update(ref.stem_profiles(case["xyz"], case["lab"], base["x"], base["y"], case["z_ref"], base["z_top"], **case["cfg"]))
    return res


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_hand_cases(name):
    case = cases.CASES[name]()
    res = restated(case)
    assert tuple(res)[:16] == inv_ref.COLUMNS and tuple(res)[16:] == ref.STEM_COLUMNS + ("stem_profile", "S_t", "margins")
    print(name, res["margins"])
    if not case.get("exact"):
        assert min(res["margins"].values()) > ref.MIN_MARGIN, res["margins"]
    case["check"](res)
    T, S = len(res["tree_id"]), res["stem_profile"]["h"].shape[1]
    assert S == (int(res["S_t"].max()) if T else 0)
    for t in range(T):                                               # h is a slab's height where the tree has the slab, NaN beyond
        St = int(res["S_t"][t])
        assert np.array_equal(res["stem_profile"]["h"][t, :St], ref.slab_heights(dict(ref.STEM_DEFAULTS, **case["cfg"]))[:St])
        assert np.isnan(res["stem_profile"]["h"][t, St:]).all() and (res["stem_profile"]["state"][t, St:] == 0).all()
    # float32 input with a row stride of 4 is the same cloud once widened
    x4 = np.zeros((len(case["xyz"]), 4), np.float32)
    x4[:, :3] = case["xyz"]
    a, b = restated(dict(case, xyz=x4[:, :3])), restated(dict(case, xyz=x4[:, :3].astype(np.float64)))
    for k in ref.STEM_COLUMNS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_restatement_offset_moves_the_centres_only():
    case = cases.CASES["lean"]()
    off = np.array([1000.0, 2000.0, 50.0])
    plain, moved = restated(case), restated(case, offset=off)
    for k in ref.STEM_COLUMNS:
        assert np.array_equal(plain[k], moved[k], equal_nan=True), k
    for k in ref.PROFILE_FLOAT + ref.PROFILE_INT:
        want = plain["stem_profile"][k] + off[0] if k == "x" else plain["stem_profile"][k] + off[1] if k == "y" else plain["stem_profile"][k]
        assert np.array_equal(moved["stem_profile"][k], want, equal_nan=True), k
    assert np.array_equal(moved["x"], plain["x"] + off[0])           # the inventory's own columns still move as before


def test_check_params():
    from treelearn_amd.util.stem import STEM_COLUMNS, STEM_DEFAULTS, check_params
    assert STEM_DEFAULTS == ref.STEM_DEFAULTS and STEM_COLUMNS == ref.STEM_COLUMNS
    assert STEM_COLUMNS == ("stem_slices", "stem_base_h", "stem_top_h", "stem_volume", "dbh_stem", "stem_lean", "stem_taper")
    assert check_params() == STEM_DEFAULTS and check_params(dict(step=1.0), thickness=None)["step"] == 1.0
    assert check_params(thickness=0.5)["thickness"] == 0.5 and check_params(max_slices=256.0)["max_slices"] == 256
    assert check_params(search_factor=1, max_growth=1, search_margin=0, min_radius=1.0, max_misses=1, min_points=3)["min_points"] == 3
    bad = [dict(first_height=0.0), dict(step=0.0), dict(step=-1.0), dict(thickness=0.0), dict(thickness=0.6), dict(max_slices=0),
           dict(max_slices=257), dict(max_slices=2.5), dict(corridor=0.0), dict(start_radius=0.0), dict(search_factor=0.99),
           dict(search_margin=-0.1), dict(min_points=2), dict(min_points=8.5), dict(max_rmse=0.0), dict(min_radius=0.0),
           dict(min_radius=1.5), dict(max_radius=0.01), dict(max_growth=0.9), dict(max_misses=0), dict(dbh_height=0.0),
           dict(step=float("nan")), dict(corridor=float("inf")), dict(max_rmse=float("nan")), dict(max_slices=float("nan"))]
    for b in bad:
        with pytest.raises(ValueError):
            check_params(b)
        with pytest.raises(ValueError):
            check_params(**b)
    with pytest.raises(ValueError, match="unknown stem parameter"):
        check_params(dict(stepp=0.5))


def test_argument_validation_before_any_gpu_work():
    from treelearn_amd.util.inventory import cloud_inventory, tree_inventory
    from treelearn_amd.util.segment import segment_forest
    xyz, lab = np.zeros((4, 3)), np.ones(4, np.int64)
    for b in (dict(step=0.0), dict(thickness=0.6), dict(nope=1)):
        with pytest.raises(ValueError):
            tree_inventory(xyz, lab, stem=True, stem_cfg=b)
        with pytest.raises(ValueError):
            cloud_inventory(np.zeros((4, 4)), stem=True, stem_cfg=b)
        with pytest.raises(ValueError):                              # before the model or the points are looked at
            segment_forest(None, None, stem=True, stem_cfg=b)


def test_command_lines_refuse_bad_parameters(tmp_path):
    from treelearn_amd.util import inventory, segment, stem
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 4)))
    with pytest.raises(SystemExit):
        stem.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--stem-step", "0"])
    with pytest.raises(SystemExit):
        stem.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--stem-thickness", "0.7"])
    with pytest.raises(SystemExit):
        stem.main(["--forest", str(tmp_path / "missing.npy"), "--out", str(tmp_path / "o.npz")])
    with pytest.raises(SystemExit):
        stem.main(["--forest", str(forest)])
    with pytest.raises(SystemExit):
        inventory.main(["--forest", str(forest), "--out", str(tmp_path / "o.csv"), "--stem", "--stem-max-slices", "300"])
    (tmp_path / "w.pth").write_bytes(b"")
    common = ["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    with pytest.raises(SystemExit):
        segment.parse_args(common + ["--stem", "--stem-min-points", "2"])
    a = segment.parse_args(common + ["--stem", "--stem-step", "0.25", "--stem-max-misses", "5"])
    assert a.stem and stem.params_of(a) == dict(stem.STEM_DEFAULTS, step=0.25, max_misses=5)
    assert not segment.parse_args(common).stem and stem.params_of(segment.parse_args(common)) == stem.STEM_DEFAULTS
    assert not (tmp_path / "o.npz").exists()


def _reference_csv(path, inv, columns, ints):
    """The CSV format of util.inventory.write_inventory, written independently: repr floats, str ints."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(list(columns))
        for i in range(len(inv["tree_id"])):
            w.writerow([str(int(inv[k][i])) if k in ints else repr(float(inv[k][i])) for k in columns])


def test_write_inventory_with_and_without_stem_columns(tmp_path):
    from treelearn_amd.util.inventory import COLUMNS, INT_COLUMNS, write_inventory
    from treelearn_amd.util.stem import STEM_COLUMNS
    res = restated(cases.CASES["label_gap"]())
    plain = {k: res[k] for k in COLUMNS}
    # without the stem columns: the bytes of before (the format written out by hand here)
    _reference_csv(tmp_path / "want.csv", plain, COLUMNS, INT_COLUMNS)
    assert open(write_inventory(str(tmp_path / "plain.csv"), plain), "rb").read() == (tmp_path / "want.csv").read_bytes()
    partial = dict(plain, stem_slices=res["stem_slices"], stem_profile=res["stem_profile"])      # not all seven: none is written
    assert open(write_inventory(str(tmp_path / "partial.csv"), partial), "rb").read() == (tmp_path / "want.csv").read_bytes()
    # with them: appended after the sixteen, stem_slices as an integer, floats read back to the same bits
    rows = list(csv.reader(open(write_inventory(str(tmp_path / "stem.csv"), res), newline="")))
    assert rows[0] == list(COLUMNS + STEM_COLUMNS) and len(rows) == 1 + 3
    for i, row in enumerate(rows[1:]):
        assert row[:16] == list(csv.reader(open(tmp_path / "want.csv", newline="")))[1 + i]
        assert row[16] == str(int(res["stem_slices"][i]))
        for k, cell in zip(STEM_COLUMNS[1:], row[17:]):
            assert cell == "nan" if np.isnan(res[k][i]) else float(cell) == res[k][i], k
    assert [r[16] for r in rows[1:]] == ["6", "0", "4"]


def test_write_stem_profiles_round_trip(tmp_path):
    from treelearn_amd.util.stem import PROFILE_KEYS, write_stem_profiles
    res = restated(cases.CASES["label_gap"](), offset=[0.1, 1e6 / 3, -7e-5])
    path = write_stem_profiles(str(tmp_path / "stems.npz"), res)
    with np.load(path) as f:
        assert set(f.files) == {"tree_id"} | set(PROFILE_KEYS) and PROFILE_KEYS == ref.PROFILE_FLOAT + ref.PROFILE_INT
        assert f["tree_id"].tolist() == [1, 2, 3] and f["tree_id"].dtype == np.int64
        for k in PROFILE_KEYS:
            assert f[k].shape == (3, 6) and f[k].dtype == res["stem_profile"][k].dtype
            assert f[k].tobytes() == res["stem_profile"][k].tobytes(), k
    with pytest.raises(ValueError):
        write_stem_profiles(str(tmp_path / "none.npz"), inv_ref.tree_inventory(np.zeros((2, 3)), np.ones(2, np.int64)))
    e = restated(cases.CASES["no_trees"]())
    with np.load(write_stem_profiles(str(tmp_path / "e.npz"), e)) as f:
        assert f["tree_id"].shape == (0,) and f["h"].shape == (0, 0)


def test_library_exports_the_stem_entry_points():
    """Both symbols are exported and bound, refuse nulls and bad parameters before anything else, and return TL_OK without a launch for
    nothing to do (no GPU is needed to find that out)."""
    from treelearn_amd import _hip, build as b
    from treelearn_amd.util.stem import STEM_DEFAULTS, check_params
    L = ctypes.CDLL(b.build(verbose=False))
    assert hasattr(L, "tl_stem_keys") and hasattr(L, "tl_stem_profile")
    assert len(_hip.PROTOTYPES["tl_stem_keys"][1]) == 9 and len(_hip.PROTOTYPES["tl_stem_profile"][1]) == 12
    assert [f[0] for f in _hip.StemParams._fields_] == [k for k in STEM_DEFAULTS if k not in ("max_slices", "min_points", "max_misses")] + \
        ["max_slices", "min_points", "max_misses"]
    lib = _hip.lib()
    good = _hip.StemParams(**check_params())
    buf = (ctypes.c_double * 64)()                                   # host memory: only its address and alignment are looked at
    p, odd = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(ctypes.addressof(buf) + 4)
    keys = lambda *a: lib.tl_stem_keys(*a, None)                     # noqa: E731
    prof = lambda *a: lib.tl_stem_profile(*a, None)                  # noqa: E731
    assert keys(p, p, 0, p, 3, 2, good, p) == _hip.TL_OK and prof(p, 0, p, p, 0, 2, good, p, p, p, p) == _hip.TL_OK
    assert prof(p, 0, p, p, 3, 0, good, p, p, p, p) == _hip.TL_OK
    assert keys(None, p, 0, p, 3, 2, good, p) == _hip.TL_ERR_ARG and keys(p, p, 0, p, 3, 2, None, p) == _hip.TL_ERR_ARG
    assert keys(p, odd, 0, p, 3, 2, good, p) == _hip.TL_ERR_ARG and keys(p, p, -1, p, 3, 2, good, p) == _hip.TL_ERR_ARG
    assert keys(p, p, 0, p, 3, 129, good, p) == _hip.TL_ERR_ARG      # a profile wider than max_slices
    assert prof(p, 0, p, p, 0, 2, good, p, p, p, None) == _hip.TL_ERR_ARG and prof(p, 0, p, odd, 0, 2, good, p, p, p, p) == _hip.TL_ERR_ARG
    assert prof(p, 0, p, p, -1, 2, good, p, p, p, p) == _hip.TL_ERR_ARG
    for bad in (dict(step=0.0), dict(thickness=0.6), dict(max_slices=257), dict(min_points=2), dict(search_factor=0.5), dict(min_radius=2.0),
                dict(max_misses=0), dict(max_rmse=float("nan")), dict(corridor=float("inf")), dict(dbh_height=-1.0), dict(max_growth=0.5),
                dict(search_margin=-1.0), dict(first_height=0.0), dict(start_radius=0.0), dict(max_radius=float("inf"))):
        with pytest.raises(ValueError):
            check_params(bad)                                        # the host check and the library's agree
        cp = _hip.StemParams(**dict(check_params(), **bad))
        assert keys(p, p, 0, p, 3, 2, cp, p) == _hip.TL_ERR_ARG and prof(p, 0, p, p, 0, 2, cp, p, p, p, p) == _hip.TL_ERR_ARG, bad
