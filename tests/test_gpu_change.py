"""GPU tests of the two-epoch comparison: tl_cross_nn and tl_rigid_sums against tests/change_restatement.py, bit for bit;
register, match_trees, compare_forests and the command line on a small scene with a known answer."""
import csv
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import change_cases as cases
import change_restatement as ref

pytestmark = pytest.mark.gpu


def _cross(refxyz, q, T=None, max_dist=1.0, cell=None):
    from treelearn_amd.util import change
    R = change._Reference(torch.from_numpy(np.ascontiguousarray(refxyz, np.float64)).reshape(-1, 3).cuda(), 1.001 * max_dist if cell is None else cell)
    nn, d2 = change._cross_nn(R, torch.from_numpy(np.ascontiguousarray(q)).cuda(), T, max_dist)
    torch.cuda.synchronize()
    return nn.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases(name):
    case = cases.CASES[name]()
    T = None if case["T"] is None else np.vstack([case["T"], [0, 0, 0, 1]])
    case["check"](*_cross(case["ref"], case["q"], T, case["max_dist"], case["cell"]))


def _rotation(rx, ry, rz):
    a, b, c = np.deg2rad([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


@functools.lru_cache(maxsize=None)
def _random_search():
    rng = np.random.default_rng(11)
    r = rng.uniform(0.0, 6.0, (3000, 3))
    T = np.eye(4)
    T[:3, :3] = _rotation(3.0, 2.0, 1.0); T[:3, 3] = (0.3, -0.2, 0.1)
    p = rng.uniform(-0.8, 6.8, (2000, 3))                                 # where the queries land: inside the cube and up to 0.8 m outside
    q = (p - T[:3, 3]) @ T[:3, :3]
    return r, q, T, ref.cross_nn(r, q, T[:3], 0.5)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_search_is_the_brute_force(dtype):
    r, q, T, _ = _random_search()
    q = q.astype(dtype)
    want_nn, want_d2 = ref.cross_nn(r, q, T[:3], 0.5) if dtype == np.float32 else _random_search()[3]
    assert 0.3 < (want_nn >= 0).mean() < 0.98                             # both outcomes are exercised
    nn, d2 = _cross(r, q, T, 0.5)
    assert np.array_equal(nn, want_nn) and d2.tobytes() == want_d2.tobytes()
    nn2, d22 = _cross(r, q, T, 0.5, cell=2.5 * 0.5)                        # another cell size: the same bits
    assert np.array_equal(nn2, nn) and d22.tobytes() == d2.tobytes()
    perm = np.random.default_rng(12).permutation(len(r))                   # another row order: the same distances and neighbour coordinates
    nn3, d23 = _cross(r[perm], q, T, 0.5)
    assert d23.tobytes() == d2.tobytes() and np.array_equal(nn3 >= 0, nn >= 0)
    assert np.array_equal(r[perm][nn3[nn3 >= 0]], r[nn[nn >= 0]])


OFFSET = np.array([512345.678, 5412345.25, 312.5])


@pytest.mark.parametrize("nq", [1, 2047, 2048, 2049, 3 * 2048 + 5])
@pytest.mark.parametrize("mode", ["mixed", "none", "f32_ld4"])
def test_rigid_sums_bit_equal_and_within_the_tree_bound(nq, mode):
    from treelearn_amd.util import change
    rng = np.random.default_rng(nq)
    nr = 500
    r = OFFSET + rng.uniform(-20, 20, (nr, 3))
    T = np.eye(4)
    T[:3, :3] = _rotation(0.2, -0.1, 0.5); T[:3, 3] = OFFSET - T[:3, :3] @ OFFSET + (0.05, 0.02, -0.01)
    q = OFFSET + rng.uniform(-20, 20, (nq, 3))
    if mode == "f32_ld4":
        q = np.column_stack([q, np.zeros(nq)]).astype(np.float32)
    nn = rng.integers(0, nr, nq); nn[rng.random(nq) < 0.2] = -1
    d2 = rng.uniform(0.0, 1.0, nq)
    reject2 = 0.0 if mode == "none" else 0.64
    want = ref.rigid_sums(r, q, T[:3], nn, d2, OFFSET, reject2)
    R = change._Reference(torch.from_numpy(r).cuda(), 1.0)
    R.centre = OFFSET
    qd, nnd, d2d = torch.from_numpy(q).cuda(), torch.from_numpy(nn).cuda(), torch.from_numpy(d2).cuda()
    got = change._rigid_sums(R, qd, T, nnd, d2d, reject2)
    again = change._rigid_sums(R, qd, T, nnd, d2d, reject2)
    assert got.dtype == np.float64 and got.shape == (17,)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert again.tobytes() == got.tobytes()
    terms = ref.rigid_terms(r, q, T[:3], nn, d2, OFFSET, reject2)
    if mode == "none":
        assert not got.any() and not np.signbit(got).any()
    else:
        assert got[0] == ((nn >= 0) & (d2 < reject2)).sum()
    for k in range(17):                                                   # the bound of a pairwise tree: derived, not measured
        bound = (math.ceil(math.log2(nq)) + 2) * 2.0 ** -53 * math.fsum(np.abs(terms[:, k]))
        assert abs(got[k] - math.fsum(terms[:, k])) <= bound, k


@functools.lru_cache(maxsize=None)
def _restated_registration(kind, dof):
    xyz, _ = cases.scene()
    mov, perm = cases.moved_copy(xyz, dof)
    if kind == "copy":
        r, q = xyz, mov
    else:
        r, q = xyz[0::2], mov[np.argsort(perm)][1::2]                     # even rows against the moved odd rows: no exact pairs
    return r, q, perm, ref.register(r, q, dof=dof, tol_angle=1e-10, tol_shift=1e-10)


def _same_log(reg, want):
    assert len(reg.iterations) == len(want["iterations"]) and reg.converged == want["converged"]
    for a, b in zip(reg.iterations, want["iterations"]):
        assert a["pairs"] == b["pairs"] and all(a[k] == b[k] for k in ("rms", "reject", "angle", "shift")), (a, b)
    assert reg.T.tobytes() == want["T"].tobytes() and reg.inlier_share == want["inlier_share"]


@pytest.mark.parametrize("dof", [6, 4])
def test_register_on_an_exact_copy(dof):
    from treelearn_amd.util import change
    r, q, perm, want = _restated_registration("copy", dof)
    reg = change.register(r, q, dof=dof, tol_angle=1e-10, tol_shift=1e-10)
    _same_log(reg, want)
    err = np.abs(ref.move(reg.T[:3], q) - r[perm]).max()
    print(f"dof {dof}: {len(reg.iterations)} iterations, max |T q - p| = {err:.3g} m")
    assert reg.converged and err <= 1e-9


@pytest.mark.parametrize("dof", [6, 4])
def test_register_on_an_even_odd_split(dof):
    from treelearn_amd.util import change
    r, q, _, want = _restated_registration("split", dof)
    reg = change.register(r, q, dof=dof, tol_angle=1e-10, tol_shift=1e-10)
    _same_log(reg, want)
    print(f"dof {dof}: {len(reg.iterations)} iterations, |T - true| = {np.abs(reg.T - cases.true_transform(dof)).max():.3g} (the sampling, not asserted)")


def test_register_masks_and_init():
    """The masks choose the rows that register; init is where the iteration starts."""
    from treelearn_amd.util import change
    xyz, lab = cases.scene()
    mov, perm = cases.moved_copy(xyz, 6)
    reg = change.register(xyz, mov, ref_mask=lab > 0, moving_mask=lab[perm] > 0, tol_angle=1e-10, tol_shift=1e-10)
    want = ref.register(xyz[lab > 0], mov[lab[perm] > 0], tol_angle=1e-10, tol_shift=1e-10)
    _same_log(reg, want)
    far = mov + (3.0, 0.0, 0.0)
    reg = change.register(xyz, far, init=(-3.0, 0.0, 0.0, 0.0), tol_angle=1e-10, tol_shift=1e-10)
    assert reg.converged and np.abs(ref.move(reg.T[:3], far) - xyz[perm]).max() <= 1e-9


def test_refusals():
    from treelearn_amd import _hip
    from treelearn_amd.util import change
    xyz, _ = cases.scene()
    bad = xyz.copy(); bad[5, 2] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        change.register(torch.from_numpy(bad).cuda(), xyz)
    with pytest.raises(ValueError, match="not finite"):
        change.register(xyz, bad)
    with pytest.raises(ValueError, match=r"^2 pairs within max_dist = 0\.5"):
        change.register(xyz, np.concatenate([xyz[:2], xyz[2:] + 100.0]), max_dist=0.5)
    with pytest.raises(ValueError, match=r"^0 pairs within max_dist = 1\.0"):
        change.register(xyz, xyz + 100.0, dof=4)
    # a cell below 1.0001 * max_dist, at the ABI
    R = change._Reference(torch.from_numpy(xyz).cuda(), 1.0)
    q = torch.from_numpy(xyz).cuda(); nn = torch.empty(len(xyz), dtype=torch.int64, device="cuda"); d2 = torch.empty(len(xyz), dtype=torch.float64, device="cuda")
    call = lambda max_dist: _hip.lib().tl_cross_nn(_hip.ptr(R.xyz), _hip.ptr(R.keys), _hip.ptr(R.perm), R.n, R.lo, R.h, R.dims, _hip.ptr(q), 1, 3, len(q),  # noqa: E731
                                                   None, max_dist, _hip.ptr(nn), _hip.ptr(d2), _hip.stream())
    assert call(1.0) == _hip.TL_ERR_ARG and call(0.99995) == _hip.TL_ERR_ARG and call(0.9999) == _hip.TL_OK
    torch.cuda.synchronize()
    assert (nn.cpu().numpy() == np.arange(len(xyz))).all() and not d2.cpu().numpy().any()


def _two_epochs():
    xyz, lab = cases.scene()
    x2, l2, renumber = cases.second_epoch(xyz, lab)
    T = cases.true_transform(6)
    perm = np.random.default_rng(3).permutation(len(x2))
    return xyz, lab, ((x2 - T[:3, 3]) @ T[:3, :3])[perm], l2[perm], renumber, T


def _same_match(got, want):
    assert got["pairs"] == want["pairs"] and got["unmatched_ref"] == want["unmatched_ref"] and got["unmatched_mov"] == want["unmatched_mov"]
    for k in ("lost_points", "gained_points", "n_ref", "n_mov"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k


def test_match_trees():
    from treelearn_amd.util import change
    xyz, lab, x2, l2, renumber, T = _two_epochs()
    want = ref.match_trees(xyz, lab, x2, l2, T)
    got = change.match_trees(xyz, lab, x2, l2, T)
    _same_match(got, want)
    assert [(r, m) for r, m, _ in got["pairs"]] == sorted(renumber.items()) and got["unmatched_ref"] == [3] and got["unmatched_mov"] == [3]
    assert got["lost_points"][2] > 300 and got["gained_points"][2] > 280 and got["gained_points"][1] >= 60        # (rows near the ground have neighbours; tree 5 -> 2 grew)
    # labels that are no trees, and a moving cloud without any tree
    _same_match(change.match_trees(xyz, -lab, x2, l2, T), ref.match_trees(xyz, -lab, x2, l2, T))
    none = change.match_trees(xyz, lab, x2, np.zeros_like(l2), T)
    assert none["pairs"] == [] and none["unmatched_ref"] == [1, 2, 3, 4, 5, 6] and none["unmatched_mov"] == []


def test_compare_forests_and_the_command_line(tmp_path):
    from treelearn_amd.util import change
    xyz, lab, x2, l2, renumber, T = _two_epochs()
    a, b = np.column_stack([xyz, lab.astype(np.float64)]), np.column_stack([x2, l2.astype(np.float64)])
    res = change.compare_forests(a, b)
    want_reg = ref.register(xyz, x2)
    _same_log(res["registration"], want_reg)
    assert np.abs(res["T"] - T).max() < 1e-3 and res["T_inv"].tobytes() == ref.invert(res["T"]).tobytes()
    _same_match(res["match"], ref.match_trees(xyz, lab, x2, l2, want_reg["T"]))
    nn, d2 = ref.cross_nn(xyz, x2, want_reg["T"][:3], 1.0)
    assert res["distance_moving"].cpu().numpy().tobytes() == np.sqrt(d2).tobytes() and np.array_equal(res["nn_moving"].cpu().numpy(), nn)
    assert res["distance_ref"].shape == (len(xyz),)
    tab = res["table"]
    by_ref = {r: i for i, r in enumerate(tab["ref_id"]) if r > 0}
    assert tab["status"] == ["survivor"] * 5 + ["lost", "ingrowth"] and tab["ref_id"] == [1, 2, 4, 5, 6, 3, -1] and tab["mov_id"] == [4, 6, 1, 2, 5, -1, 3]
    assert tab["status"][by_ref[3]] == "lost" and tab["lost_points"][by_ref[3]] > 300 and tab["gained_points"][-1] > 280
    assert 0.8 < tab["d_height"][by_ref[5]] < 1.2 and all(abs(tab["d_height"][by_ref[r]]) < 0.01 for r in (1, 2, 4, 6))
    assert all(tab["d_position"][by_ref[r]] < 0.02 for r in (1, 2, 4, 5, 6)) and all(tab["overlap"][by_ref[r]] > 0.8 for r in (1, 2, 4, 5, 6))
    unlabelled = change.compare_forests(xyz, x2, registration=False, init=T)
    assert unlabelled["registration"] is None and "table" not in unlabelled and unlabelled["T"].tobytes() == T.tobytes()
    # the command line on two .npy files
    fa, fb, out = str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), str(tmp_path / "change")
    np.save(fa, a); np.save(fb, b)
    change.main(["--ref", fa, "--moving", fb, "--out", out, "--write-registered", "npy"])
    assert sorted(os.listdir(out)) == ["change.csv", "distance_moving.npy", "distance_ref.npy", "registered.npy", "transform.json"]
    meta = json.load(open(os.path.join(out, "transform.json")))
    assert meta["T"] == res["T"].tolist() and meta["converged"] and len(meta["iterations"]) == len(want_reg["iterations"]) and meta["rms"] == res["registration"].rms
    rows = list(csv.reader(open(os.path.join(out, "change.csv"), newline="")))
    assert rows[0] == list(change.table_columns()) and [r[0] for r in rows[1:]] == tab["status"] and [int(r[1]) for r in rows[1:]] == tab["ref_id"]
    assert np.load(os.path.join(out, "distance_moving.npy")).tobytes() == res["distance_moving"].cpu().numpy().tobytes()
    assert np.load(os.path.join(out, "distance_ref.npy")).shape == (len(xyz),)
    moved = np.load(os.path.join(out, "registered.npy"))
    assert moved.shape == b.shape and moved[:, :3].tobytes() == ref.move(res["T"][:3], x2).tobytes() and np.array_equal(moved[:, 3], l2)


def test_stable_band_registers_on_the_stems():
    from treelearn_amd.util import change
    xyz, lab, x2, l2, _, T = _two_epochs()
    a, b = np.column_stack([xyz, lab.astype(np.float64)]), np.column_stack([x2, l2.astype(np.float64)])
    res = change.compare_forests(a, b, stable_band=(0.5, 4.0), dof=4, init=(0.1, -0.1, 0.0, 1.5), terrain=True)
    assert res["registration"].iterations[0]["pairs"] < 0.9 * (l2 > 0).sum() and "d_height_ag" in res["table"]
    assert tuple(res["table"]) == change.table_columns(ground=True)
