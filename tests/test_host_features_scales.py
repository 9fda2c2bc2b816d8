"""Host-side tests of the multi-scale geometric features (util/features.py, util/prepare.compute_features_scales,
csrc/tl_features.hip: tl_eigen_features_scales): no GPU.  The hand-made cases through the restatement, the rules of a list of radii, the
command line's --radii, and the C entry point: its declaration, its binding and every argument it refuses."""
import ctypes
import os
import re

import numpy as np
import pytest

import features_scales_cases as cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_gives_the_hand_made_answers(name):
    c = cases.CASES[name]()
    assert 1 <= len(c["radii"]) <= 4 and all(b > a for a, b in zip(c["radii"], c["radii"][1:]))
    if c.get("on_the_radius"):
        return                                                                     # (the kd-tree promises nothing ON a radius; see compare_scales)
    refs = cases.restate_scales(c["points"], c["radii"])
    f = np.stack([r["features"] for r in refs], 1)
    assert f.shape == (len(c["points"]), len(c["radii"]), 27)
    c["check"](f)
    cases.compare_scales(f.astype(np.float32), refs)                              # the comparison accepts the yardstick's own f32 rounding


def test_the_cases_cover_every_number_of_scales():
    assert sorted({len(cases.CASES[k]()["radii"]) for k in cases.CASES}) == [1, 2, 3, 4]


def test_check_radii():
    from treelearn_amd.util.features import MAX_SCALES, check_radii
    assert MAX_SCALES == 4
    assert check_radii([0.2]) == [0.2] and check_radii((0.2, 0.4, 0.6)) == [0.2, 0.4, 0.6] and check_radii(np.array([1, 2, 3, 4])) == [1.0, 2.0, 3.0, 4.0]
    assert check_radii([0.25, np.nextafter(0.25, 1.0)])[1] > 0.25
    nan, inf = float("nan"), float("inf")
    for bad in ([], [0.1, 0.2, 0.3, 0.4, 0.5], [0.2, 0.2], [0.4, 0.2], [0.0, 0.2], [-0.1, 0.2], [0.2, nan], [nan], [0.2, inf], ["0.2"], [True, 2.0], "0.2", 0.2, None):
        with pytest.raises(ValueError):
            check_radii(bad)


def test_compute_features_scales_refuses_names_and_radii_before_any_gpu_work(monkeypatch):
    from treelearn_amd import _hip
    from treelearn_amd.util import prepare
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was touched"))
    monkeypatch.setattr(prepare, "_dev_f64", lambda a: pytest.fail("the device was touched"))
    pts = np.zeros((4, 3))
    for names, radii in ((["curvature"], [0.2, 0.4]), ([], [0.2]), (["nz", "nz"], [0.2]), (["nz"], []), (["nz"], [0.4, 0.2]), (["nz"], [0.1, 0.2, 0.3, 0.4, 0.5]),
                         (["nz"], [0.2, float("nan")])):
        with pytest.raises(ValueError):
            prepare.compute_features_scales(pts, radii, names)


def test_command_line_radii(tmp_path):
    from treelearn_amd.util import features
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 3)))
    out = str(tmp_path / "o.npz")
    ok = ["--forest", str(forest), "--out", out, "--features", "linearity", "planarity"]
    a = features.parse_args(ok)
    assert a.radii is None and a.radius == 0.6                                    # without --radii nothing changes
    a = features.parse_args(ok + ["--radii", "0.2", "0.4", "0.6"])
    assert a.radii == [0.2, 0.4, 0.6] and a.features == ["linearity", "planarity"]
    assert features.parse_args(ok + ["--radii", "0.5"]).radii == [0.5]
    for bad in (ok + ["--radii"], ok + ["--radii", "0.4", "0.2"], ok + ["--radii", "0.2", "0.2"], ok + ["--radii", "0", "0.2"], ok + ["--radii", "nan"],
                ok + ["--radii", "0.1", "0.2", "0.3", "0.4", "0.5"], ok + ["--radii", "0.2", "0.4", "--radius", "0.6"], ok + ["--radius", "0.6", "--radii", "0.2"]):
        with pytest.raises(SystemExit):
            features.main(bad)
    assert not os.path.exists(out)


def test_entry_point_is_declared_bound_and_refuses_bad_arguments():
    from treelearn_amd import _hip, build as b
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    assert re.search(r"#define\s+TL_FEAT_MAX_SCALES\s+4\b", hdr)
    m = re.search(r"\bint\s+tl_eigen_features_scales\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, "tl_eigen_features_scales is not declared"
    assert hdr.index("tl_eigen_features(") < m.start() < hdr.index("random training crops")       # next to tl_eigen_features
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _hip.PROTOTYPES["tl_eigen_features_scales"]
    assert res is ctypes.c_int32 and len(args) == len(params) == 12
    for p, a in zip(params, args):
        want = ctypes.c_void_p if ("*" in p or p.startswith("tl_stream_t")) else ctypes.c_int64 if p.startswith("int64_t") else \
            ctypes.c_double if p.startswith("double") else ctypes.c_int32
        assert a is want, (p, a)
    assert hasattr(ctypes.CDLL(b.build(verbose=False)), "tl_eigen_features_scales")
    lib = _hip.lib()
    buf = (ctypes.c_int64 * 64)()                                                  # host memory: only looked at where the argument is a host array
    p = ctypes.c_void_p(ctypes.addressof(buf))
    cols = (ctypes.c_int32 * 27)(*range(27))
    c = ctypes.cast(cols, ctypes.c_void_p)

    def radii(*v):
        return ctypes.cast((ctypes.c_double * max(1, len(v)))(*v), ctypes.c_void_p)

    call = lambda *a: lib.tl_eigen_features_scales(*a, None)                       # noqa: E731
    E = _hip.TL_ERR_ARG
    good = lambda: [p, p, 10, radii(0.2, 0.4), 2, p, p, 1, c, 3, p]              # noqa: E731  (nothing of it is ever launched: see below)
    assert call(None, None, 0, None, 0, None, None, 0, None, 0, None) == E
    for k in (0, 1, 3, 5, 6, 8, 10):                                               # every pointer in turn
        a = good()
        a[k] = None
        assert call(*a) == E, k
    for k, v in ((2, 0), (2, -1), (7, 0), (7, 11), (7, 1 << 31), (4, 0), (4, 5), (4, -1), (9, 0), (9, 28)):      # n, n_pieces, S, F
        a = good()
        a[k] = v
        if (k, v) == (7, 1 << 31):
            a[2] = 1 << 40
        assert call(*a) == E, (k, v)
    nan, inf = float("nan"), float("inf")
    for S, r in ((1, (0.0,)), (1, (-0.2,)), (1, (nan,)), (1, (inf,)), (2, (0.2, 0.2)), (2, (0.4, 0.2)), (2, (0.2, nan)), (2, (nan, 0.2)), (2, (0.2, inf)),
                 (3, (0.2, 0.4, 0.3)), (4, (0.1, 0.2, 0.3, 0.3)), (4, (0.0, 0.2, 0.3, 0.4))):
        a = good()
        a[3], a[4] = radii(*r), S
        assert call(*a) == E, (S, r)
    for ext in ((-1, 4), (3, 1 << 21)):
        a = good()
        a[5] = ctypes.cast((ctypes.c_int64 * 2)(*ext), ctypes.c_void_p)
        assert call(*a) == E, ext
    for ids in ((0, 27, 1), (0, -1, 1)):                                           # an id out of range
        a = good()
        a[8] = ctypes.cast((ctypes.c_int32 * 3)(*ids), ctypes.c_void_p)
        assert call(*a) == E, ids
