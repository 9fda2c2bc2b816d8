"""Host tests of the branch structure, no GPU: the restatement against the closed forms of the hand cases, the host-side
branch rules of util.branches against the restatement's, check_params on every constraint, the argument parsers, the files, and the
entry points' declarations, exports and argument guards."""
import argparse
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import branches_cases as cases
import branches_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tl_skel_voxel_keys": 9, "tl_skel_distance": 8, "tl_skel_nodes": 10, "tl_skel_links": 19}


def restated(case, offset=None):
    return ref.branch_structure(case["xyz"], case["lab"], case["tree"][:, 0], case["tree"][:, 1], case["tree"][:, 2], offset=offset, **case["cfg"])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_on_the_hand_cases(name):
    """Every case's closed forms (distances of named voxels, node counts, lengths) hold on the restatement, and its float decisions are
    farther than the margin from their thresholds."""
    case = cases.CASES[name]()
    want = restated(case)
    assert min(want["margins"].values()) > ref.MIN_MARGIN, want["margins"]
    case["check"](want, cases.d_lookup(case, want["keys"], want["d"]))
    assert (np.diff(want["keys"]) > 0).all() and want["d"].dtype == np.int32 and len(want["d"]) == len(want["keys"]) == want["skel_voxels"].sum()
    sk = want["skeleton"]
    assert sk["count"].sum() == want["skel_reached"].sum() and (sk["parent"] < np.arange(len(sk["parent"])) - sk["node_start"][:-1].repeat(
        np.diff(sk["node_start"]))).all()


def test_weights_and_pole_closed_forms():
    assert [ref.weight(*v) for v in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 0, 0), (2, 1, 0), (2, 1, 1), (2, 2, 0), (2, 2, 1), (2, 2, 2))] == \
        [100, 141, 173, 200, 223, 244, 282, 300, 346]
    assert len(ref.offsets(1)) == 26 and len(ref.offsets(2)) == 124
    for n, level in ((30, 3), (31, 3), (7, 1), (50, 7)):                  # a pole of n voxels of 0.1 m from one source voxel
        case = cases.build([cases.pole(n)], dict(voxel=0.1, base_reach=0, base_layers=1, level=level), None)
        w = restated(case)
        assert w["d"].tolist() == [100 * k for k in range(n)] and w["skel_nodes"][0] == -(-n // level)
        last = (n - 1) // level
        top = (level * last + n - 1) / 2                                  # the mean layer of the last node
        length = 0.1 * (top - (level - 1) / 2) if last else 0.0
        assert abs(w["axis_length"][0] - length) < 1e-9 and abs(w["axis_top_h"][0] - 0.1 * top) < 1e-9 and w["branch_count"][0] == 0


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_host_branch_rules_against_the_restatement(name):
    """util.branches.to_columns (step 7, on the host) from the restatement's node table: orders, branch ids and integer columns equal, the
    lengths and heights to 1e-9."""
    from treelearn_amd.util.branches import BRANCH_COLUMNS, BRANCH_INT_COLUMNS, check_params, to_columns
    case = cases.CASES[name]()
    off = np.array([10.5, -3.25, 100.0])
    want, sk = restated(case, offset=off), restated(case)["skeleton"]
    kstart = np.searchsorted(want["keys"], np.arange(len(case["tree"]) + 1, dtype=np.int64) << 35)
    host = dict(kstart=kstart, node_start=sk["node_start"], xyz=sk["xyz"], parent=sk["parent"], bin=sk["bin"], count=sk["count"])
    got = to_columns(host, case["tree"][:, 2], check_params(case["cfg"]), off)
    assert tuple(got) == BRANCH_COLUMNS + ("skeleton",) and BRANCH_INT_COLUMNS == ref.BRANCH_INT
    for k in ref.SKELETON_KEYS:
        assert got["skeleton"][k].dtype == want["skeleton"][k].dtype and np.array_equal(got["skeleton"][k], want["skeleton"][k]), k
    for k in BRANCH_COLUMNS:
        assert got[k].dtype == want[k].dtype and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        if k in BRANCH_INT_COLUMNS:
            assert np.array_equal(got[k], want[k]), k
        else:
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-9, equal_nan=True), k


def test_check_params_on_every_constraint():
    from treelearn_amd.util.branches import BRANCH_DEFAULTS, check_params
    assert BRANCH_DEFAULTS == ref.BRANCH_DEFAULTS == dict(voxel=0.1, reach=1, base_reach=10, base_layers=5, level=3, min_branch=0.5, min_height=1.0,
                                                          max_voxels=1 << 20)
    p = check_params()
    assert p == BRANCH_DEFAULTS and all(type(p[k]) is int for k in ("reach", "base_reach", "base_layers", "level", "max_voxels"))
    assert check_params(dict(voxel=0.05, reach=None), level=2.0) == dict(BRANCH_DEFAULTS, voxel=0.05, level=2)
    for ok in (dict(reach=2), dict(base_reach=0), dict(base_reach=2047), dict(base_layers=1), dict(level=1), dict(min_branch=0.0), dict(min_height=0.0),
               dict(max_voxels=1), dict(max_voxels=1 << 22)):
        check_params(ok)
    for bad in (dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(reach=0), dict(reach=3), dict(reach=1.5),
                dict(reach=True), dict(base_reach=-1), dict(base_reach=2048), dict(base_reach=0.5), dict(base_layers=0), dict(base_layers=1.5),
                dict(level=0), dict(level=2.5), dict(level=10 ** 6 + 1), dict(min_branch=-0.1), dict(min_branch=float("nan")), dict(min_height=-1.0),
                dict(min_height=float("inf")), dict(max_voxels=0), dict(max_voxels=(1 << 22) + 1), dict(max_voxels=float("nan")), dict(radius=1.0)):
        with pytest.raises(ValueError):
            check_params(bad)


def test_argument_parsers(tmp_path):
    from treelearn_amd.util import branches, crown, inventory, segment, stem
    ap = argparse.ArgumentParser()
    branches.add_arguments(ap)
    branches.add_arguments(ap)                                            # a second call adds nothing
    assert branches.params_of(ap.parse_args([])) == branches.BRANCH_DEFAULTS
    a = ap.parse_args(["--branch-voxel", "0.05", "--branch-reach", "2", "--branch-base-reach", "4", "--branch-base-layers", "2", "--branch-level", "5",
                       "--branch-min-branch", "0.25", "--branch-min-height", "2", "--branch-max-voxels", "1000"])
    assert branches.params_of(a) == dict(voxel=0.05, reach=2, base_reach=4, base_layers=2, level=5, min_branch=0.25, min_height=2.0, max_voxels=1000)
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 4)))
    # a parameter outside its constraint ends every command line before any GPU work, and nothing is written
    with pytest.raises(SystemExit):
        branches.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--branch-reach", "3"])
    with pytest.raises(SystemExit):
        branches.main(["--forest", str(forest)])
    with pytest.raises(SystemExit):
        inventory.main(["--forest", str(forest), "--out", str(tmp_path / "o.csv"), "--branches", "--branch-voxel", "0"])
    with pytest.raises(SystemExit):
        stem.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--branches", "--branch-level", "0"])
    with pytest.raises(SystemExit):
        crown.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--branches", "--branch-base-reach", "2048"])
    (tmp_path / "w.pth").write_bytes(b"")
    common = ["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    with pytest.raises(SystemExit):
        segment.parse_args(common + ["--branches", "--branch-min-branch", "-1"])
    a = segment.parse_args(common + ["--branches", "--branch-reach", "2", "--branch-level", "4"])
    assert a.branches and branches.params_of(a) == dict(branches.BRANCH_DEFAULTS, reach=2, level=4)
    assert not segment.parse_args(common).branches and branches.params_of(segment.parse_args(common)) == branches.BRANCH_DEFAULTS
    assert not (tmp_path / "o.npz").exists() and not (tmp_path / "o.csv").exists()
    with pytest.raises(ValueError):                                       # the API checks before any GPU work too
        segment.segment_forest(None, None, branches=True, branch_cfg=dict(voxel=0.0))
    with pytest.raises(ValueError):
        inventory.tree_inventory(None, None, branches=True, branch_cfg=dict(reach=5))
    with pytest.raises(ValueError):
        inventory.cloud_inventory(np.zeros((1, 4)), branches=True, branch_cfg=dict(nothing=1))


def _inventory_of(case):
    """An inventory dict as tree_inventory(..., branches=True) returns it, from the restatements (no GPU)."""
    import inventory_restatement as inv_ref
    res = dict(inv_ref.tree_inventory(case["xyz"], case["lab"]))
    want = restated(case)
    res.update({k: want[k] for k in ref.BRANCH_COLUMNS + ("skeleton",)})
    return res


def test_write_inventory_column_order(tmp_path):
    from treelearn_amd.util.branches import BRANCH_COLUMNS, BRANCH_INT_COLUMNS
    from treelearn_amd.util.inventory import COLUMNS, write_inventory
    inv = _inventory_of(cases.CASES["empty_slots"]())
    rows = list(csv.reader(open(write_inventory(str(tmp_path / "b.csv"), inv), newline="")))
    assert rows[0] == list(COLUMNS + BRANCH_COLUMNS) and len(rows) == 5
    for i, row in enumerate(rows[1:]):
        for k, cell in zip(BRANCH_COLUMNS, row[16:]):
            if k in BRANCH_INT_COLUMNS:
                assert cell == str(int(inv[k][i])), k
            else:
                assert cell == "nan" if np.isnan(inv[k][i]) else float(cell) == inv[k][i], k
    assert [r[16] for r in rows[1:]] == ["12", "0", "8", "30"]
    # without all thirteen: the columns of before, the same bytes
    plain = {k: inv[k] for k in COLUMNS}
    partial = dict(plain, skel_voxels=inv["skel_voxels"], skeleton=inv["skeleton"])
    assert open(write_inventory(str(tmp_path / "p.csv"), partial), "rb").read() == open(write_inventory(str(tmp_path / "q.csv"), plain), "rb").read()
    assert list(csv.reader(open(tmp_path / "q.csv", newline="")))[0] == list(COLUMNS)
    # after the crown group
    from treelearn_amd.util.crown import CROWN_COLUMNS
    crowned = dict(inv, **{k: np.zeros(4) for k in CROWN_COLUMNS})
    assert list(csv.reader(open(write_inventory(str(tmp_path / "c.csv"), crowned), newline="")))[0] == list(COLUMNS + CROWN_COLUMNS + BRANCH_COLUMNS)


def test_write_skeletons_round_trip(tmp_path):
    from treelearn_amd.util.branches import SKELETON_KEYS, write_skeletons
    inv = _inventory_of(cases.CASES["two_trees"]())
    with np.load(write_skeletons(str(tmp_path / "s.npz"), inv)) as f:
        assert set(f.files) == {"tree_id"} | set(SKELETON_KEYS) and f["tree_id"].tolist() == [1, 2] and f["tree_id"].dtype == np.int64
        for k in SKELETON_KEYS:
            assert f[k].dtype == inv["skeleton"][k].dtype and f[k].tobytes() == inv["skeleton"][k].tobytes(), k
        assert f["node_start"].dtype == np.int64 and f["xyz"].dtype == np.float64 and f["count"].dtype == np.int64
        assert all(f[k].dtype == np.int32 for k in ("parent", "bin", "order", "branch"))
    with pytest.raises(ValueError):
        write_skeletons(str(tmp_path / "none.npz"), {k: v for k, v in inv.items() if k != "skeleton"})


def test_header_declares_and_library_exports_the_entry_points():
    """The four symbols are declared in a section of their own, bound with matching arity and exported; they refuse nulls, misaligned
    pointers and bad parameters before anything else, and return TL_OK without a launch for nothing to do (no GPU is needed for that)."""
    from treelearn_amd import _hip, build as b
    from treelearn_amd.util.branches import check_params
    header = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    assert "csrc/tl_skeleton.hip, DESIGN §23" in header and "typedef struct tl_skel_params" in header
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES[name][1]), name
    L = ctypes.CDLL(b.build(verbose=False))
    assert all(hasattr(L, name) for name in ENTRY_POINTS)
    assert [f[0] for f in _hip.SkeletonParams._fields_] == ["voxel", "min_branch", "min_height", "reach", "base_reach", "base_layers", "level", "max_voxels"]
    assert ctypes.sizeof(_hip.SkeletonParams) == 64
    lib = _hip.lib()
    good = _hip.SkeletonParams(**check_params())
    buf = (ctypes.c_double * 64)()                                       # host memory: only its address and alignment are looked at
    p, odd, odd2 = (ctypes.c_void_p(ctypes.addressof(buf) + k) for k in (0, 4, 2))
    keys = lambda *a: lib.tl_skel_voxel_keys(*a, None)                    # noqa: E731
    dist = lambda *a: lib.tl_skel_distance(*a, None)                      # noqa: E731
    nodes = lambda *a: lib.tl_skel_nodes(*a, None)                        # noqa: E731
    links = lambda *a: lib.tl_skel_links(*a, None)                        # noqa: E731
    ok, bad = _hip.TL_OK, _hip.TL_ERR_ARG
    # nothing to do, found out after the argument checks and without a launch
    assert keys(p, p, 0, p, 3, good, p, p) == ok and keys(p, p, 5, p, 0, good, p, p) == ok
    assert dist(p, 0, p, 3, good, p, p) == ok and dist(p, 5, p, 0, good, p, p) == ok
    assert nodes(p, 0, p, 3, good, p, p, p, p) == ok and nodes(p, 5, p, 0, good, p, p, p, p) == ok
    assert links(p, 0, p, p, 3, good, p, p, p, p, p, 0, p, p, p, p, p, p) == ok and links(p, 5, p, p, 3, good, p, p, p, p, p, 0, p, p, p, p, p, p) == ok
    # nulls, misaligned pointers, sizes
    assert keys(None, p, 0, p, 3, good, p, p) == bad and keys(p, p, 0, p, 3, None, p, p) == bad and keys(p, odd, 0, p, 3, good, p, p) == bad
    assert keys(p, p, -1, p, 3, good, p, p) == bad and keys(p, p, 0, p, -1, good, p, p) == bad and keys(p, p, 0, p, 1 << 21, good, p, p) == bad
    assert keys(p, p, 0, p, 3, good, p, None) == bad and keys(p, p, 0, p, 3, good, p, odd2) == bad and keys(p, p, 0, p, 3, good, p, odd) == ok
    assert dist(None, 0, p, 3, good, p, p) == bad and dist(p, 0, odd, 3, good, p, p) == bad and dist(p, 0, p, 3, good, odd2, p) == bad
    assert dist(p, -1, p, 3, good, p, p) == bad and dist(p, 1 << 31, p, 3, good, p, p) == bad and dist(p, 0, p, 3, good, p, None) == bad
    assert nodes(p, 0, p, 3, good, None, p, p, p) == bad and nodes(p, 0, p, 3, good, p, p, odd, p) == bad and nodes(p, 0, p, 3, good, p, p, p, odd) == bad
    assert nodes(p, 0, p, 1 << 21, good, p, p, p, p) == bad and nodes(p, 0, p, 3, None, p, p, p, p) == bad
    assert links(p, 0, p, None, 3, good, p, p, p, p, p, 0, p, p, p, p, p, p) == bad and links(p, 0, p, p, 3, good, p, p, p, p, p, 1, p, p, p, p, p, p) == bad
    assert links(p, 0, p, p, 3, good, p, p, p, p, p, -1, p, p, p, p, p, p) == bad and links(p, 0, p, p, 3, good, p, p, p, p, p, 0, p, odd, p, p, p, p) == bad
    assert links(p, 0, p, p, 3, good, p, p, p, p, p, 0, p, p, odd, p, p, p) == bad and links(p, 0, p, p, 3, good, p, p, p, p, p, 0, p, p, p, p, p, None) == bad
    for wrong in (dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(min_branch=-0.5), dict(min_height=float("nan")), dict(reach=0),
                  dict(reach=3), dict(base_reach=-1), dict(base_reach=2048), dict(base_layers=0), dict(level=0), dict(level=10 ** 6 + 1), dict(max_voxels=0)):
        with pytest.raises(ValueError):
            check_params(wrong)                                           # the host check and the library's agree
        sp = _hip.SkeletonParams(**dict(check_params(), **wrong))
        assert keys(p, p, 0, p, 3, sp, p, p) == bad and dist(p, 0, p, 3, sp, p, p) == bad and nodes(p, 0, p, 3, sp, p, p, p, p) == bad, wrong
        assert links(p, 0, p, p, 3, sp, p, p, p, p, p, 0, p, p, p, p, p, p) == bad, wrong
