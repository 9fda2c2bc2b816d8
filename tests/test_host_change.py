"""Host tests of the two-epoch comparison, no GPU: the restatement against the hand cases' own expected values and against
its registration bound, the documented tree against math.fsum, the host solve of util.change on sums with a known answer, init parsing,
the change table and its file, the command line's argument errors, and the entry points' declarations, exports and argument guards."""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest

import change_cases as cases
import change_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"tl_cross_nn": 16, "tl_rigid_sums_ws_doubles": 1, "tl_rigid_sums": 14}


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_restatement_on_the_hand_cases(name):
    case = cases.CASES[name]()
    case["check"](*ref.cross_nn(case["ref"], case["q"], case["T"], case["max_dist"]))


@pytest.mark.parametrize("dof", [6, 4])
def test_restatement_registers_the_exact_copy(dof):
    """The restatement has to meet the 1e-9 m bound on the CPU before the GPU is asked to."""
    xyz, _ = cases.scene()
    mov, perm = cases.moved_copy(xyz, dof)
    r = ref.register(xyz, mov, dof=dof, tol_angle=1e-10, tol_shift=1e-10)
    err = np.abs(ref.move(r["T"][:3], mov) - xyz[perm]).max()
    print(f"dof {dof}: {len(r['iterations'])} iterations, max |T q - p| = {err:.3g} m")
    assert r["converged"] and err <= 1e-9
    assert np.abs(r["T"] - cases.true_transform(dof)).max() <= 1e-9
    assert r["iterations"][0]["reject"] == 1.0 and all(it["reject"] >= 0.1 for it in r["iterations"])


@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2048, 2049, 3 * 2048 + 5])
def test_tree_sum_against_fsum(n):
    """A pairwise tree of depth ceil(log2 n) is within (depth + 2) * 2^-53 * sum |term| of the exact sum; padding adds exact zeros."""
    rng = np.random.default_rng(n)
    v = rng.normal(0.0, 1.0, (n, 3)) * np.array([1.0, 1e6, 1e-6])
    got = ref.tree_sum(v)
    assert got.shape == (3,) and got.dtype == np.float64
    for k in range(3):
        bound = (math.ceil(math.log2(max(n, 1))) + 2) * 2.0 ** -53 * math.fsum(np.abs(v[:, k]))
        assert abs(got[k] - math.fsum(v[:, k])) <= bound
    if 0 < n <= 2048:                                                     # one chunk: the plain halving tree, written out
        s = np.zeros((2048, 3)); s[:n] = v
        for stride in (1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1):
            s[:stride] += s[stride:2 * stride]
        assert got.tobytes() == s[0].tobytes()


def _known_step(dof, rng):
    yaw, pitch = np.deg2rad(7.0), np.deg2rad(3.0 if dof == 6 else 0.0)
    Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
    R, t = Rz @ Ry, np.array([0.4, -0.3, 0.2])
    c = np.array([1234.5, 5432.25, 312.5])
    a = c + rng.uniform(-5, 5, (40, 3))
    b = a @ R.T + t
    return R, t, c, a, b


@pytest.mark.parametrize("dof", [6, 4])
def test_host_solve_on_sums_with_a_known_answer(dof):
    from treelearn_amd.util import change
    R, t, c, a, b = _known_step(dof, np.random.default_rng(5))
    nn = np.arange(len(a)); d2 = ((a - b) ** 2).sum(1)
    sums = ref.rigid_sums(b, a, None, nn, d2, c, np.inf)
    assert sums[0] == len(a)
    dT, angle, shift = change.solve(sums, c, dof)
    assert np.abs(dT[:3, :3] - R).max() < 1e-10 and np.abs(dT[:3, :3] @ a.T + dT[:3, 3:4] - b.T).max() < 1e-9 and tuple(dT[3]) == (0, 0, 0, 1)
    want_angle = np.arccos((np.trace(R) - 1) / 2)
    assert abs(angle - want_angle) < 1e-10 and abs(shift - np.linalg.norm(R @ c + t - c)) < 1e-8
    rT, rangle, rshift = ref.solve(sums, c, dof)                          # the same numpy calls in the same order: the same bits
    assert dT.tobytes() == rT.tobytes() and angle == rangle and shift == rshift
    # a reflection in the data does not come back as one
    mirrored = np.array(sums); mirrored[7:16] = (sums[7:16].reshape(3, 3) * np.array([1.0, 1.0, -1.0])).reshape(-1); mirrored[6] = -sums[6]
    assert np.linalg.det(change.solve(mirrored, c, 6)[0][:3, :3]) > 0.999
    assert change.invert(dT).tobytes() == ref.invert(dT).tobytes() and np.abs(change.invert(dT) @ dT - np.eye(4)).max() < 1e-9


def test_init_parsing():
    from treelearn_amd.util import change
    assert np.array_equal(change.parse_init(None), np.eye(4))
    T = change.parse_init((1.0, -2.0, 0.5, 90.0))
    assert np.allclose(T, [[0, -1, 0, 1], [1, 0, 0, -2], [0, 0, 1, 0.5], [0, 0, 0, 1]], atol=1e-16)
    assert change.parse_init(T).tobytes() == T.tobytes() and change.parse_init(T) is not T
    assert change.parse_init([1, 2, 3, 4]).tobytes() == ref.parse_init([1, 2, 3, 4]).tobytes()
    bad_last = np.eye(4); bad_last[3, 0] = 1
    for bad in ((1, 2, 3), np.eye(3), (1, 2, 3, float("nan")), bad_last, np.full((4, 4), np.inf)):
        with pytest.raises(ValueError):
            change.parse_init(bad)


def test_not_finite_input_is_refused_before_any_launch():
    from treelearn_amd.util import change
    good = np.zeros((8, 3)); bad = good.copy(); bad[3, 1] = np.nan
    for a, b in ((bad, good), (good, bad)):
        with pytest.raises(ValueError, match="not finite"):
            change.register(a, b)
        with pytest.raises(ValueError, match="not finite"):
            change.cloud_distance(a, b)
    with pytest.raises(ValueError, match="not finite"):
        ref.register(bad, good)
    with pytest.raises(ValueError):
        change.register(good, good, dof=5)
    with pytest.raises(ValueError):
        change.register(good, good, max_dist=0.0)
    with pytest.raises(TypeError):
        change.register(good.astype(np.int32), good)


def _hand_match():
    return dict(pairs=[(4, 1, 0.9), (1, 4, 0.8)], unmatched_ref=[3], unmatched_mov=[2], lost_points=np.array([5, 0, 40, 7]),
                gained_points=np.array([2, 30, 0, 9]))


def _hand_inventory(T, shift=0.0):
    return dict(x=np.arange(T) * 2.0 + shift, y=np.arange(T) * 1.0, z=np.zeros(T), height=10.0 + np.arange(T) + shift, dbh=0.2 + 0.01 * np.arange(T),
                crown_area=4.0 + np.arange(T))


def test_change_table_and_its_file(tmp_path):
    from treelearn_amd.util import change
    inv_r, inv_m = _hand_inventory(4), _hand_inventory(4, shift=0.5)
    T = change.parse_init((1.0, 0.0, 0.0, 0.0))
    tab = change.change_table(_hand_match(), inv_r, inv_m, T)
    assert tuple(tab) == change.table_columns() == ("status", "ref_id", "mov_id", "overlap", "d_position", "height_ref", "height_mov", "d_height",
                                                    "dbh_ref", "dbh_mov", "d_dbh", "crown_area_ref", "crown_area_mov", "d_crown_area",
                                                    "gained_points", "lost_points")
    assert tab["status"] == ["survivor", "survivor", "lost", "ingrowth"] and tab["ref_id"] == [1, 4, 3, -1] and tab["mov_id"] == [4, 1, -1, 2]
    assert tab["overlap"][:2] == [0.8, 0.9] and all(math.isnan(v) for v in tab["overlap"][2:])
    # ref tree 1 at (0, 0); moving tree 4 at (6.5, 3) carried to (7.5, 3)
    assert tab["d_position"][0] == float(np.hypot(7.5, 3.0)) and math.isnan(tab["d_position"][2]) and math.isnan(tab["d_position"][3])
    assert tab["height_ref"][0] == 10.0 and tab["height_mov"][0] == 13.5 and tab["d_height"][0] == 3.5
    assert math.isnan(tab["height_mov"][2]) and math.isnan(tab["d_height"][2]) and tab["height_ref"][2] == 12.0
    assert math.isnan(tab["dbh_ref"][3]) and tab["crown_area_mov"][3] == 5.0
    assert tab["gained_points"] == [9, 2, 0, 30] and tab["lost_points"] == [5, 7, 40, 0]
    ground = change.change_table(_hand_match(), dict(inv_r, height_ag=inv_r["height"], dbh_ag=inv_r["dbh"]),
                                 dict(inv_m, height_ag=inv_m["height"] + 1, dbh_ag=inv_m["dbh"]), T)
    assert tuple(ground) == change.table_columns(ground=True) and ground["d_height_ag"][0] == 4.5 and ground["d_dbh_ag"][1] == inv_m["dbh"][0] - inv_r["dbh"][3]
    rows = list(csv.reader(open(change.write_table(str(tmp_path / "change.csv"), tab), newline="")))
    assert rows[0] == list(change.table_columns()) and len(rows) == 5
    assert [r[0] for r in rows[1:]] == tab["status"] and rows[3][2] == "-1" and rows[3][3] == "nan" and float(rows[1][7]) == 3.5 and rows[4][-2] == "30"
    # the files of a result without a registration and without labels
    res = dict(T=T, T_inv=change.invert(T), registration=None, distance_moving=np.array([0.5, np.inf]), distance_ref=np.array([0.25]))
    paths = change.write_change(str(tmp_path / "out"), res, write_registered="npy", moving_points=np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]))
    assert [os.path.basename(p) for p in paths] == ["transform.json", "distance_moving.npy", "distance_ref.npy", "registered.npy"]
    import json
    meta = json.load(open(paths[0]))
    assert meta["T"] == T.tolist() and meta["T_inv"][0][3] == -1.0 and meta["registered"] is False and meta["iterations"] == []
    assert np.array_equal(np.load(paths[3]), [[2.0, 2.0, 3.0], [1.0, 0.0, 0.0]]) and np.load(paths[1])[1] == np.inf
    with pytest.raises(ValueError):
        change.write_change(str(tmp_path / "out"), res, write_registered="ply", moving_points=np.zeros((1, 3)))
    with pytest.raises(ValueError):
        change.write_change(str(tmp_path / "out"), res, write_registered="npy")


def test_command_line_argument_errors(tmp_path):
    from treelearn_amd.util import change
    a, b = str(tmp_path / "a.npy"), str(tmp_path / "b.npy")
    np.save(a, np.zeros((4, 4))); np.save(b, np.zeros((4, 4)))
    common = ["--ref", a, "--moving", b, "--out", str(tmp_path / "o")]
    _, ok = change.parse_args(common + ["--dof", "4", "--init", "1,2,3,45", "--stable-band", "0.5", "4", "--write-registered", "las", "--no-register"])
    assert ok.dof == 4 and ok.init == (1.0, 2.0, 3.0, 45.0) and ok.stable_band == [0.5, 4.0] and ok.no_register and ok.write_registered == "las"
    _, d = change.parse_args(common)
    assert (d.dof, d.max_dist, d.reject_min, d.match_dist, d.min_overlap, d.init, d.stable_band, d.terrain) == (6, 1.0, 0.1, 0.2, 0.3, None, None, False)
    for bad in (["--dof", "5"], ["--max-dist", "0"], ["--max-dist", "nan"], ["--reject-min", "-1"], ["--match-dist", "0"], ["--min-overlap", "1.5"],
                ["--init", "1,2,3"], ["--init", "a,b,c,d"], ["--stable-band", "4", "0.5"], ["--write-registered", "ply"], ["--max-iters", "0"]):
        with pytest.raises(SystemExit):
            change.main(common + bad)
    with pytest.raises(SystemExit):
        change.main(["--ref", a, "--moving", str(tmp_path / "none.npy"), "--out", str(tmp_path / "o")])
    with pytest.raises(SystemExit):
        change.main(["--ref", a, "--out", str(tmp_path / "o")])
    assert not (tmp_path / "o").exists()


def test_header_declares_and_library_exports_the_entry_points():
    """The symbols are declared in a section of their own, bound with matching arity and exported; they refuse nulls, misaligned pointers
    and bad sizes before anything else, and tl_cross_nn returns TL_OK without a launch for no query (host memory: no GPU)."""
    from treelearn_amd import _hip, build as b
    header = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    assert "two epochs of one plot (csrc/tl_change.hip, DESIGN §30)" in header
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint(?:64_t)? " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == arity == len(_hip.PROTOTYPES[name][1]), name
    L = ctypes.CDLL(b.build(verbose=False))
    assert all(hasattr(L, name) for name in ENTRY_POINTS)
    assert '#include "tl_morton.h"' in open(os.path.join(REPO, "treelearn_amd", "csrc", "tl_outlier.hip")).read()      # one copy of the search
    assert "spread3" not in open(os.path.join(REPO, "treelearn_amd", "csrc", "tl_outlier.hip")).read()
    lib = _hip.lib()
    buf = (ctypes.c_double * 64)()                                       # host memory: only its address and alignment are looked at
    p, odd, odd2 = (ctypes.c_void_p(ctypes.addressof(buf) + k) for k in (0, 4, 2))
    lo, dims, c3 = (ctypes.c_double * 3)(), _hip.dims3([4, 4, 4]), (ctypes.c_double * 3)()
    eye = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    ok, bad = _hip.TL_OK, _hip.TL_ERR_ARG

    def cross(xyz=p, keys=p, perm=p, nr=5, h=1.001, q=p, f64=1, ld=3, nq=0, T=eye, max_dist=1.0, nn=p, d2=p, dims=dims):
        return lib.tl_cross_nn(xyz, keys, perm, nr, lo, h, dims, q, f64, ld, nq, T, max_dist, nn, d2, None)

    assert cross() == ok and cross(T=None) == ok and cross(ld=4, f64=0) == ok and cross(q=odd, f64=0) == ok and cross(h=1.0001) == ok
    assert cross(nr=0, xyz=None, keys=None, perm=None, h=0.0) == ok                            # no reference: the grid is not looked at
    for kw in (dict(q=None), dict(nn=None), dict(d2=None), dict(xyz=None), dict(keys=None), dict(perm=None), dict(q=odd), dict(q=odd2, f64=0),
               dict(nn=odd), dict(d2=odd), dict(xyz=odd), dict(keys=odd), dict(perm=odd), dict(ld=2), dict(nq=-1), dict(nr=-1), dict(f64=2), dict(f64=-1),
               dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(h=1.0), dict(h=float("inf")),
               dict(T=ctypes.cast(odd, ctypes.POINTER(ctypes.c_double)))):
        assert cross(**kw) == bad, kw
    assert cross(h=0.0) == _hip.TL_ERR_UNSUPPORTED and cross(dims=_hip.dims3([0, 4, 4])) == _hip.TL_ERR_UNSUPPORTED

    def sums(q=p, f64=1, ld=3, nq=4, T=eye, nn=p, d2=p, r=p, nr=5, c=c3, reject2=1.0, out=p, ws=p):
        return lib.tl_rigid_sums(q, f64, ld, nq, T, nn, d2, r, nr, c, reject2, out, ws, None)

    for kw in (dict(q=None), dict(nn=None), dict(d2=None), dict(r=None), dict(out=None), dict(ws=None), dict(q=odd), dict(q=odd2, f64=0), dict(nn=odd),
               dict(d2=odd), dict(r=odd), dict(out=odd), dict(ws=odd), dict(ld=2), dict(nq=-1), dict(nr=-1), dict(f64=3), dict(reject2=-1.0),
               dict(reject2=float("nan")), dict(c=(ctypes.c_double * 3)(float("nan"), 0, 0)), dict(T=ctypes.cast(odd, ctypes.POINTER(ctypes.c_double)))):
        assert sums(**kw) == bad, kw
    ws = lib.tl_rigid_sums_ws_doubles
    assert [ws(n) for n in (0, 1, 2048, 2049, 2048 * 2048, 2048 * 2048 + 1)] == [17, 17, 17, 17 * 3, 17 * 2049, 17 * (2049 + 2 + 1)]
