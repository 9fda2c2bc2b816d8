"""tl_train_item and tl_point_jitter on the GPU against tests/train_batch_restatement.py and against the unmodified host path
(util/tiles._offset_labels_host).

Bounds, none of them measured:
  * test mode: coords, labels, masks, batch ids and centres are bitwise equal.  The tree position is a mean of n_base float32 rows: the
    reference sums them one after another in float32, the kernel exactly, so |position - reference| <= n_base * 2^-24 * max|coordinate among
    the base rows| + one float32 ulp of the position (the textbook bound, computed per instance from the host data).  The position is seen
    through offset = fl32(position - x), which rounds once on either side: one float32 ulp of the offset is allowed on top.
  * training mode (float64 coordinates): coords within one float32 ulp (BLAS may fuse the three-term dot product); masks equal, and no row
    of these inputs lies within 2^-40 of the inner square's edge; position within one float32 ulp (seen through offset + x, half an ulp of
    the offset on top); offsets within two float32 ulps of max(|position|, |x|).

Each step runs in a child process of its own under a time limit: a fault or a hang ends that step and names it."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

INNER = 8.0
KEYS = ("coords", "semantic_labels", "instance_labels", "offset_labels", "masks_inner", "masks_off", "masks_sem", "batch_ids", "centers")


def _step(name, *args, limit=300):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), name, *[str(a) for a in args]],
                       cwd=REPO, capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"step {name} exited with {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return r.stdout


# ------------------------------------------------------------------------------------------------ helpers (child process)
def run_item(points, inst, m=None, center=None, row_offset=0, total=None, batch_id=0, inner=INNER, out=None, ws=None):
    """tl_train_item on one item -> (dict of the item's rows as numpy, the batch tensors)."""
    import torch
    from treelearn_amd.util.device_dataset import ItemWorkspace, alloc_batch, train_item
    n = len(points)
    xyz = torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(inst, np.int32)).cuda()
    if out is None:
        out = alloc_batch(total if total is not None else row_offset + n, 1, xyz.device)
    train_item(xyz, lab, out, row_offset, inner / 2, ws or ItemWorkspace(xyz.device), m=m, center=center, batch_id=batch_id)
    torch.cuda.synchronize()
    return {k: out[k][row_offset:row_offset + n].cpu().numpy() for k in KEYS}, out


def check_exact(dev, want, keys, what):
    for k in keys:
        assert dev[k].dtype == want[k].dtype, (what, k, dev[k].dtype, want[k].dtype)
        assert np.array_equal(dev[k], want[k]), (what, k, int((dev[k] != want[k]).sum()))


def check_test_mode(dev, it, what, rows=None):
    """The bounds of test 1.  `rows`: bool mask of the rows whose offsets (and masks_off) are compared -- all by default."""
    import train_batch_restatement as R
    want = R.collate([it])
    check_exact(dev, want, ("coords", "semantic_labels", "instance_labels", "masks_inner", "masks_sem", "centers"), what)
    assert dev["batch_ids"].dtype == np.int64
    rows = np.ones(len(dev["coords"]), bool) if rows is None else rows
    assert np.array_equal(dev["masks_off"][rows], want["masks_off"][rows]), (what, "masks_off")
    a, b = dev["offset_labels"].astype(np.float64), want["offset_labels"].astype(np.float64)
    tol = R.position_tolerance(it)[:, None] + R.ulp32(it["position"]) + R.ulp32(np.maximum(np.abs(a), np.abs(b)))
    err = np.abs(a - b)
    worst = float((err / tol)[rows].max(initial=0))
    print(f"{what}: {int(rows.sum())} rows, max |offset - restatement| {float(err[rows].max(initial=0)):.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= tol)[rows].all()), (what, worst)


def check_train_mode(dev, it, what, rows=None, inner=INNER):
    """The bounds of test 2."""
    import train_batch_restatement as R
    want = R.collate([it])
    rows = np.ones(len(dev["coords"]), bool) if rows is None else rows
    x64 = it["xyz"]
    assert x64.dtype == np.float64
    err_c = np.abs(dev["coords"].astype(np.float64) - want["coords"].astype(np.float64))
    assert bool((err_c <= R.ulp32(x64)).all()), (what, "coords", float((err_c / R.ulp32(x64)).max()))
    near = np.abs(it["inf_norm"] - inner / 2) <= 2.0 ** -40
    assert not near.any(), (what, "rows on the inner square's edge", int(near.sum()))
    check_exact(dev, want, ("semantic_labels", "instance_labels", "masks_inner", "masks_sem", "centers"), what)
    assert np.array_equal(dev["masks_off"][rows], want["masks_off"][rows]), (what, "masks_off")
    off = dev["offset_labels"].astype(np.float64)
    p = it["position"].astype(np.float64)
    pos_err = np.abs(off + x64 - p)                                                  # the device position seen through its offsets
    pos_tol = R.ulp32(p) + 0.5 * R.ulp32(off) + np.abs(x64) * 2.0 ** -49
    assert bool((pos_err <= pos_tol)[rows].all()), (what, "position", float((pos_err / pos_tol)[rows].max()))
    err = np.abs(off - want["offset_labels"].astype(np.float64))
    tol = 2 * R.ulp32(np.maximum(np.abs(p), np.abs(x64)))
    worst = float((err / tol)[rows].max(initial=0))
    print(f"{what}: {int(rows.sum())} rows, coords max err {float(err_c.max()):.3e}, offsets worst err / bound {worst:.3f}")
    assert bool((err <= tol)[rows].all()), (what, worst)


def tile2():
    from treelearn_amd.synth import CONFIGS, make_tile
    return make_tile(**CONFIGS["config2"], seed=0)


def tile12(seed=7, ignore=True):
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=12.0, voxel=0.1, n_trees=6, fill=0.10, seed=seed)
    lab = t["instance_label"].copy()
    if ignore:
        lab[lab == 2] = -1                                                           # a whole tree, and 3 % of all rows, unlabelled
        lab[np.random.default_rng(seed).uniform(size=len(lab)) < 0.03] = -1
    return dict(t, instance_label=lab)


def matrices():
    s, c = math.sin(0.7), math.cos(0.7)
    rot = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
    scale = np.eye(3) * np.array([1.13, 0.87, 1.02])
    flip = scale.copy(); flip[0][0] *= -1
    jit = scale + np.random.RandomState(11).randn(3, 3) * 0.1
    return dict(identity=np.eye(3), scale=scale, scale_flip_rot=np.matmul(flip, rot), jitter=np.matmul(jit, rot))


def matrix_rs3():
    """scale + jitter + rot drawn from RandomState(3), in the reference's order."""
    rs = np.random.RandomState(3)
    m = np.eye(3) * np.concatenate([rs.uniform(0.8, 1.2, 2), rs.uniform(0.95, 1.05, 1)])
    m += rs.randn(3, 3) * 0.1
    th = rs.rand() * 2 * math.pi
    return np.matmul(m, [[math.cos(th), math.sin(th), 0], [-math.sin(th), math.cos(th), 0], [0, 0, 1]])


# ------------------------------------------------------------------------------------------------ steps
def step_test_mode():
    import train_batch_restatement as R
    for name, t in (("config-2 seed-0 tile", tile2()), ("12 m tile with -1", tile12())):
        c = np.array([3.5, -2.25, 0.0])
        dev, _ = run_item(t["points"], t["instance_label"], center=c)
        it = R.item(t["points"], t["instance_label"], INNER, center=c, rank3=True)
        assert (dev["batch_ids"] == 0).all()
        check_test_mode(dev, it, name)
    print("test_mode step OK")


def step_train_mode():
    import train_batch_restatement as R
    t = tile2()
    t12 = tile12()
    for name, m in matrices().items():
        for tn, tt in (("config-2", t), ("12 m", t12)):
            dev, _ = run_item(tt["points"], tt["instance_label"], m=m, batch_id=3)
            it = R.item(tt["points"], tt["instance_label"], INNER, m=m, rank3=True)
            assert (dev["batch_ids"] == 3).all() and (dev["centers"] == 1).all()
            check_train_mode(dev, it, f"{tn} {name}")
    print("train_mode step OK")


def step_host_path():
    """Against numpy's own pick: util/tiles._offset_labels_host inside the restatement's item(rank3=False)."""
    import train_batch_restatement as R
    from treelearn_amd.util.tiles import _offset_labels_host
    t = tile2()
    for name, m in (("identity", None), ("RandomState(3) matrix", matrix_rs3())):
        it = R.item(t["points"], t["instance_label"], INNER, m=m, center=np.zeros(3), rank3=False)
        off, valid = _offset_labels_host(it["xyz"], it["instance_label"], it["semantic_label"])          # the unmodified host path
        assert np.array_equal(off, it["pt_offset_label"]) and valid[it["semantic_label"] == 0].all()
        left_out = [lab for lab, d in it["info"].items() if not d["numpy_pick_is_rank3"]]
        print(f"{name}: {len(it['info'])} tree instances, numpy's pick is not rank 3 for {len(left_out)}")
        assert len(it["info"]) == 64 and len(left_out) <= 3
        rows = ~np.isin(it["instance_label"], left_out)
        dev, _ = run_item(t["points"], t["instance_label"], m=m, center=None if m is not None else np.zeros(3))
        (check_train_mode if m is not None else check_test_mode)(dev, it, f"host path, {name}", rows=rows)
    print("host_path step OK")


def edge_item(seed=0):
    rng = np.random.default_rng(seed)
    pts, lab = [], []

    def add(label, p):
        pts.append(np.asarray(p, np.float64)); lab.append(np.full(len(p), label, np.int64))
    add(0, np.column_stack([rng.uniform(-6, 6, (50, 2)), rng.uniform(0, 0.3, 50)]))
    for label, k in ((5, 1), (6, 4), (7, 11), (-2147483648, 12), (2147483647, 13), (-7, 300)):
        c = rng.uniform(-5, 5, 2)
        add(label, np.column_stack([c + rng.uniform(-0.3, 0.3, (k, 2)), rng.uniform(0, 12, k)]))
    for label, zs in ((20, [0.3] * 4), (21, [0.1, 0.1, 0.2, 0.2, 0.2]), (22, [0.25] * 7), (23, [0.5, 0.5, 0.5, 0.75])):   # duplicates among the lowest
        k = 40
        z = np.concatenate([zs, rng.uniform(1.0, 9.0, k - len(zs))])
        add(label, np.column_stack([rng.uniform(-4, 4, 2) + rng.uniform(-0.2, 0.2, (k, 2)), z]))
    for label, k in ((30, 50), (31, 9)):                                            # the lowest point 3 m below the rest
        z = np.concatenate([[2.0], rng.uniform(5.0, 6.0, k - 1)])
        add(label, np.column_stack([rng.uniform(-4, 4, 2) + rng.uniform(-0.2, 0.2, (k, 2)), z]))
    add(-1, np.column_stack([rng.uniform(-6, 6, (30, 2)), rng.uniform(0, 5, 30)]))
    p = np.round(np.concatenate(pts), 2).astype(np.float32); l = np.concatenate(lab).astype(np.int32)
    order = rng.permutation(len(p))                                                 # labels interleaved: no wave holds one label
    return p[order], l[order]


def tiny_negative_item():
    """Base rows whose coordinates are tiny negatives, -0.0 and small negative fractions: the values at which a fixed-point conversion built
    on x - floor(x) would go wrong (that difference rounds to 1.0 for -2^-54 <= x < 0).  One instance of 10 rows (all of them base rows), one
    of 40 whose 13 lowest rows carry the values, between ground rows."""
    rng = np.random.default_rng(4)
    tiny = np.array([-1e-30, -2.0 ** -54, -0.0, 0.3 - 0.1 * 3, -2.0 ** -60, -1e-3, -0.3, -0.75, -1.0 - 2.0 ** -23, -2.0 ** -24], np.float32)
    assert (tiny <= 0).all() and np.signbit(tiny).all()
    pts = [np.column_stack([rng.uniform(-6, 6, (50, 2)), rng.uniform(0, 0.3, 50)])]
    lab = [np.zeros(50, np.int64)]
    pts.append(np.column_stack([tiny, tiny[::-1], rng.uniform(0, 0.3, 10)])); lab.append(np.full(10, 40, np.int64))
    low = np.column_stack([np.resize(tiny, 13), np.resize(tiny[3:], 13), rng.uniform(0, 0.3, 13)])
    low[:3, 2] = np.float32(-1e-30), -0.0, -(2.0 ** -54)                             # the heights as well
    high = np.column_stack([rng.uniform(-0.2, 0.2, (27, 2)), rng.uniform(3.0, 9.0, 27)])
    pts.append(np.concatenate([low, high])); lab.append(np.full(40, 41, np.int64))
    p = np.concatenate(pts).astype(np.float32); l = np.concatenate(lab).astype(np.int32)
    order = rng.permutation(len(p))
    return p[order], l[order]


def step_edges():
    import torch
    import train_batch_restatement as R
    from treelearn_amd import _hip
    m = matrices()["jitter"]
    rng = np.random.default_rng(1)
    cases = {"small instances, duplicates, outlier": edge_item()}
    g = np.column_stack([rng.uniform(-6, 6, (5000, 2)), rng.uniform(0, 1, 5000)]).astype(np.float32)
    cases["no tree"] = (g, np.zeros(5000, np.int32))
    cases["only label -1"] = (g, np.full(5000, -1, np.int32))
    distinct = np.unique(rng.integers(-(2 ** 31), 2 ** 31, 30000))
    distinct = rng.permutation(distinct[distinct != 0])[:20000]
    assert len(distinct) == 20000
    lab = rng.permutation(np.repeat(distinct, 10)).astype(np.int32)
    many = np.round(np.column_stack([rng.uniform(-20, 20, (200000, 2)), rng.uniform(0, 30, 200000)]), 2).astype(np.float32)
    cases["20 000 labels on 200 000 rows"] = (many, lab)
    cases["tiny negative base rows"] = tiny_negative_item()
    for name, (p, l) in cases.items():
        dev, _ = run_item(p, l, center=np.array([1.0, 2.0, 0.0]))
        check_test_mode(dev, R.item(p, l, INNER, center=np.array([1.0, 2.0, 0.0])), f"{name}, test mode")
        dev, _ = run_item(p, l, m=m)
        check_train_mode(dev, R.item(p, l, INNER, m=m), f"{name}, training mode")
    # tiny negatives once more, straight against the float64 mean: with the identity and a pure scale the values stay tiny and negative
    p, l = cases["tiny negative base rows"]
    for name, mm in (("test mode", None), ("identity", np.eye(3)), ("scale", matrices()["scale"])):
        dev, _ = run_item(p, l, m=mm, center=None if mm is not None else np.zeros(3))
        x = p.astype(np.float64) if mm is None else np.matmul(p, mm)
        if mm is not None:
            check_train_mode(dev, R.item(p, l, INNER, m=mm), f"tiny negative base rows, {name}")
        for label in (40, 41):
            sel = l == label
            z = x[sel, 2]
            base = x[sel][z <= (np.sort(z)[3] if sel.sum() > 11 else z.min()) + 0.5]
            assert len(base) == (10 if label == 40 else 13)
            mean = base.mean(axis=0)                                                  # float64: exact to 2^-53 relative per term
            seen = dev["offset_labels"][sel].astype(np.float64) + x[sel]             # the position through each row's offset
            tol = R.ulp32(mean) + R.ulp32(dev["offset_labels"][sel]) + np.abs(base).max() * 2.0 ** -49
            assert bool((np.abs(seen - mean) <= tol).all()), (name, label, float(np.abs(seen - mean).max()))
    p, l = cases["no tree"]
    dev, _ = run_item(p, l, center=np.zeros(3))
    assert not dev["masks_off"].any() and np.array_equal(dev["offset_labels"], (1 - p).astype(np.float32)) and (dev["semantic_labels"] == 1).all()
    p, l = cases["only label -1"]
    dev, _ = run_item(p, l, center=np.zeros(3))
    assert not dev["masks_off"].any() and not dev["masks_sem"].any() and dev["masks_inner"].any() and (dev["semantic_labels"] == 0).all()
    # n = 0: an error code, nothing launched
    L = _hip.lib()
    assert L.tl_train_item_ws_bytes(0) == 0 and L.tl_train_item_ws_bytes(-3) == 0
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    q = _hip.ptr(buf)
    rc = L.tl_train_item(q, q, 0, None, 4.0, None, 0, 0, q, q, q, q, q, q, q, q, q, q, _hip.stream())
    assert rc == _hip.TL_ERR_ARG, rc
    assert L.tl_point_jitter(q, 0, 1, _hip.stream()) == _hip.TL_ERR_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())
    print("edges step OK")


def step_determinism():
    a, b = tile12(seed=7), tile12(seed=8)
    pa, la = a["points"][:100001], a["instance_label"][:100001]                      # an odd row count: the second item starts at an odd row
    pb, lb = b["points"], b["instance_label"]
    for m in (None, matrices()["jitter"]):
        c = None if m is not None else np.array([0.5, 0.25, 0.0])
        one, _ = run_item(pb, lb, m=m, center=c)
        two, _ = run_item(pb, lb, m=m, center=c)
        for k in KEYS:
            assert one[k].tobytes() == two[k].tobytes(), ("two calls differ", k)
        total = len(pa) + len(pb)
        first, out = run_item(pa, la, m=m, center=c, row_offset=0, total=total, batch_id=0)
        second, out = run_item(pb, lb, m=m, center=c, row_offset=len(pa), total=total, batch_id=0, out=out)
        assert len(pa) % 2 == 1
        for k in KEYS:
            assert one[k].tobytes() == second[k].tobytes(), ("row offset changes the rows", k)
            assert out[k][:len(pa)].cpu().numpy().tobytes() == first[k].tobytes(), ("the second item touched the first one's rows", k)
    print("determinism step OK")


def _phi(x):
    return 0.5 * (1 + math.erf(x / math.sqrt(2)))


def step_jitter():
    import torch
    from treelearn_amd.util.device_dataset import point_jitter
    n = 1_000_000
    rng = np.random.default_rng(2)
    base = rng.uniform(-20, 20, (n, 3)).astype(np.float32)

    def run(x, key):
        t = torch.from_numpy(x.copy()).cuda()
        point_jitter(t, key)
        torch.cuda.synchronize()
        return t.cpu().numpy()
    a, b, c = run(base, 12345), run(base, 12345), run(base, 12346)
    assert a.tobytes() == b.tobytes(), "same key, different bits"
    assert (a != c).mean() > 0.9, "different keys give the same draws"
    d = a.astype(np.float64) - base.astype(np.float64)
    assert bool((np.abs(d) <= 0.2 + np.spacing(np.abs(a)).astype(np.float64)).all())
    assert (a != base).mean() > 0.99
    # a function of (key, row, component): any sub-range started at row 0 of its own array repeats the head of the stream
    head = run(base[:1000], 12345)
    assert head.tobytes() == a[:1000].tobytes()
    # statistics on zeros (delta = the rounded draw itself): X = clip(0.1 g, -0.2, 0.2)
    z = run(np.zeros((n, 3), np.float32), 2 ** 63 + 977).astype(np.float64).ravel()
    k = len(z)
    p_clip = 2 * _phi(-2.0)
    phi2 = math.exp(-2.0) / math.sqrt(2 * math.pi)
    inner2 = (2 * _phi(2.0) - 1) - 2 * 2 * phi2                                     # int_{-2}^{2} t^2 phi
    inner4 = 3 * (2 * _phi(2.0) - 1) - 2 * phi2 * (2 ** 3 + 3 * 2)                  # int_{-2}^{2} t^4 phi
    var = 0.01 * (inner2 + 4 * p_clip)
    mu4 = 1e-4 * (inner4 + 16 * p_clip)
    sd = math.sqrt(var)
    se_mean, se_sd, se_p = sd / math.sqrt(k), math.sqrt((mu4 - var * var) / (4 * k * var)), math.sqrt(p_clip * (1 - p_clip) / k)
    share = float((np.abs(z) == np.float64(np.float32(0.2))).mean())
    print(f"jitter: {k} draws, mean {z.mean():.3e} (se {se_mean:.1e}), sd {z.std():.6f} against {sd:.6f} (se {se_sd:.1e}), "
          f"share at the clip {share:.5f} against {p_clip:.5f} (se {se_p:.1e})")
    assert abs(z.mean()) <= 5 * se_mean
    assert abs(z.std() - sd) <= 5 * se_sd
    assert abs(share - p_clip) <= 5 * se_p
    for comp in range(3):                                                           # the three components are streams of their own
        assert abs(z[comp::3].mean()) <= 5 * sd / math.sqrt(n)
    print("jitter step OK")


# ------------------------------------------------------------------------------------------------ tests
def test_test_mode_matches_the_restatement_with_the_rank3_rule():
    _step("test_mode")


def test_training_mode_matches_the_restatement():
    _step("train_mode", limit=600)


def test_offset_labels_match_the_unmodified_host_path_where_numpy_picks_rank3():
    _step("host_path")


def test_edge_cases():
    _step("edges")


def test_bits_do_not_depend_on_the_call_or_on_the_row_offset():
    _step("determinism")


def test_point_jitter_is_keyed_clipped_and_normal():
    """The clipped normal X = clip(0.1 g, -0.2, 0.2) has standard deviation 0.1 * sqrt(int_{-2}^{2} t^2 phi + 4 * 2 Phi(-2)) = 0.09594 (the
    0.0880 sometimes quoted is the TRUNCATED normal's, which drops the mass at the clip); the test derives it, and its standard errors."""
    _step("jitter")


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    globals()["step_" + sys.argv[1]](*sys.argv[2:])
