"""GPU tests of the light stage (csrc/tl_light.hip, util/light.py) against the numpy restatement of
tests/light_restatement.py.

Bounds.  Grid shapes and origins, occ, owner, counts, status, code and first are compared exactly, dtype included: the voxel of a row
and every step of a walk are floors, comparisons and one fixed f64 expression (a multiply, a subtract, a divide) from integer indices,
and the counts are integer sums, so nothing depends on an order.  The derived floats (gap, openness, lai_e, gap_zenith, edge_share and
the tree columns) are compared to 1e-12 relative: the two sides evaluate the same formulas over at most a dozen f64 terms per value
(nine rings), where only the association of those few sums and products can differ, each by at most one rounding of 1.1e-16."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import light_cases as cases
import light_restatement as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12
DERIVED = ("gap", "openness", "lai_e", "gap_zenith", "edge_share")


def _exact(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), name


def _close(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"NaN pattern of {name}"
    ok = ~np.isnan(want)
    err = float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)).max()) if ok.any() else 0.0
    print(f"{name}: max relative difference {err:.3e}")
    assert (np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])).all(), (name, err)


def _occ(vox):
    return vox.occ.cpu().numpy().view(np.uint32)


def assert_voxels(vox, want):
    assert [vox.ix0, vox.iy0, vox.iz0] == want["i0"] and [vox.nx, vox.ny, vox.nz] == want["n"] and vox.voxel == want["voxel"]
    _exact("occ", _occ(vox), want["occ"])
    assert (vox.owner is None) == (want["owner"] is None)
    if want["owner"] is not None:
        _exact("owner", vox.owner.cpu().numpy(), want["owner"])


def gpu_march(vox, origins, dirs, ring, n_rings, skip=None, max_range=60.0, min_hits=1):
    from treelearn_amd.util.light import march
    m = march(vox, origins, dirs, ring, n_rings, skip=skip, max_range=max_range, min_hits=min_hits, rays=True)
    return {k: v.cpu().numpy() for k, v in m.items()}


def assert_march(got, want):
    for k in ("counts", "status", "code", "first"):
        _exact(k, got[k], want[k])


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_hand_cases_through_the_kernels(name):
    from treelearn_amd.util.light import light_voxels, march
    case = cases.CASES[name]()
    vox = light_voxels(case["xyz"], case["labels"], case["voxel"])
    want_vox = ref.light_voxels(case["xyz"], case["labels"], case["voxel"])
    assert_voxels(vox, want_vox)
    args = (case["origins"], case["dirs"], case["ring"], case["n_rings"])
    kw = dict(skip=case["skip"], max_range=case["max_range"], min_hits=case["min_hits"])
    got = gpu_march(vox, *args, **kw)
    case["check"](got)
    assert_march(got, ref.march(want_vox, *args, **kw))
    only = march(vox, *args, **kw)                                                    # without the per-ray outputs: the same counts
    assert set(only) == {"counts", "status"} and np.array_equal(only["counts"].cpu().numpy(), got["counts"])


def test_empty_cloud_and_refused_inputs():
    from treelearn_amd.util.light import light_voxels, march
    vox = light_voxels(np.zeros((0, 3)), np.zeros(0, np.int64))
    assert_voxels(vox, ref.light_voxels(np.zeros((0, 3)), np.zeros(0, np.int64)))
    got = gpu_march(vox, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [0], 1)
    assert_march(got, ref.march(ref.light_voxels(np.zeros((0, 3))), [[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], [0], 1))
    xyz = cases.CASES["slab"]()["xyz"]
    for col, bad in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        b = xyz.copy()
        b[5, col] = bad
        with pytest.raises(ValueError, match="not finite"):
            light_voxels(b)
    free = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=r"8 x 8 x 8 m: \d+ x \d+ x \d+ light voxels of 0.0001 m"):   # the extent and the voxel are named
        light_voxels(xyz, None, 1e-4)
    with pytest.raises(ValueError, match="light voxels of 0.01 m"):                  # 801^3 > 2^28 with an owner grid, < 2^31 without
        light_voxels(xyz, np.zeros(len(xyz), np.int64), 0.01)
    assert torch.cuda.memory_allocated() <= free + (1 << 20)                         # no grid of 5e14 voxels was allocated
    vox = light_voxels(xyz, None, 1.0)
    with pytest.raises(ValueError, match="unit length"):
        march(vox, [cases.MID], [[0.0, 0.0, 2.0]], [0], 1)
    with pytest.raises(ValueError, match="ring"):
        march(vox, [cases.MID], [[0.0, 0.0, 1.0]], [1], 1)
    with pytest.raises(ValueError, match="mismatched"):
        march(vox, [cases.MID], [[0.0, 0.0, 1.0]], [0], 1, skip=np.array([1, 2], np.int32))
    nan_origin = gpu_march(vox, [[np.nan, 4.5, 4.5], cases.MID], [[0.0, 0.0, 1.0]], [0], 1)
    assert nan_origin["status"].tolist() == [1, 0] and nan_origin["code"].tolist() == [[255], [0]]


# ------------------------------------------------------------------ word and lane edges
def _edge_table(D):
    """D directions whose rings straddle the waves: the 9 x 36 sky table for 324, else the first D rows of an 11 x 7 table."""
    from treelearn_amd.util.light import sky_directions
    if D == 324:
        dirs, ring, _, _ = sky_directions()
        return dirs, ring, 9
    dirs, ring, _, _ = sky_directions(11, 7, 88.0)
    down = dirs[:D] * np.where(np.arange(D) % 5 == 4, -1.0, 1.0)[:, None]            # every fifth ray looks down and away
    return np.ascontiguousarray(down), ring[:D].copy(), 11


@pytest.mark.parametrize("D,P", [(1, 1), (63, 65), (64, 1), (65, 65), (324, 0), (324, 65)])
@pytest.mark.parametrize("nx", [31, 32, 33, 64, 65])
def test_word_and_lane_edges(nx, D, P):
    """Grids whose x rows end one bit before, on and after a word; tables that fill a wave less one lane, exactly, and one lane more, and
    the sky table, whose rings of 36 straddle the waves of 64; no origin, one, and one more than a wave's worth."""
    from treelearn_amd.util.light import light_voxels
    rng = np.random.default_rng(1000 * nx + D + P)
    n = 6 * nx
    xyz = np.column_stack([rng.uniform(0, nx, n), rng.uniform(0, 5, n), rng.uniform(0, 6, n)])
    xyz[:2] = [[0.5, 0.5, 0.5], [nx - 0.5, 4.5, 5.5]]
    xyz[2:6, 0] = [nx - 0.25, nx - 1.5, 31.5 if nx > 32 else 0.25, 32.5 if nx > 33 else 1.25]        # the last bits of the words
    lab = rng.integers(-1, 5, n).astype(np.int64)
    vox = light_voxels(xyz, lab, 1.0)
    want_vox = ref.light_voxels(xyz, lab, 1.0)
    assert want_vox["n"] == [nx, 5, 6] and want_vox["occ"].shape == (6, 5, (nx + 31) // 32) and want_vox["full"][:, :, nx - 1].any()
    assert_voxels(vox, want_vox)
    dirs, ring, R = _edge_table(D)
    origins = np.column_stack([rng.uniform(0, nx, P), rng.uniform(0, 5, P), rng.uniform(0, 3, P)])
    skip = rng.integers(-1, 5, P).astype(np.int32)
    got = gpu_march(vox, origins, dirs, ring, R, skip=skip, max_range=20.0)
    want = ref.march(want_vox, origins, dirs, ring, R, skip=skip, max_range=20.0)
    assert got["counts"].shape == (P, R, 4) and got["code"].shape == (P, D) and int(want["counts"].sum()) == P * D
    assert_march(got, want)


# ------------------------------------------------------------------ a random cloud of about 20 000 rows over 12 x 9 x 10 m
VOXEL = 0.25
MARCH = dict(max_range=9.0, min_hits=1)


def _random_cloud():
    rng = np.random.default_rng(28)
    n = 20_000
    x, y = rng.uniform(0.0, 12.0, n), rng.uniform(0.0, 9.0, n)
    tree = 1 + (np.floor(x / 4.0) + 3 * np.floor(y / 4.5)).astype(np.int64)           # six crowns on a 3 x 2 lattice
    r2 = (x % 4.0 - 2.0) ** 2 + (y % 4.5 - 2.25) ** 2
    kind = rng.uniform(size=n)
    z = np.where(kind < 0.25, rng.uniform(0.0, 0.2, n), 0.0)                          # ground
    stem = (kind >= 0.25) & (kind < 0.32)
    x[stem], y[stem] = np.floor(x[stem] / 4.0) * 4.0 + 2.0 + rng.normal(0, 0.05, stem.sum()), np.floor(y[stem] / 4.5) * 4.5 + 2.25 + rng.normal(0, 0.05, stem.sum())
    z[stem] = rng.uniform(0.2, 6.0, stem.sum())
    crown = kind >= 0.32
    top = 5.0 + 4.5 * np.exp(-r2 / 2.0)
    z[crown] = np.where(r2[crown] < 3.0, top[crown] - rng.uniform(0.0, 1.5, crown.sum()) ** 2, rng.uniform(0.0, 0.2, crown.sum()))
    lab = np.where((z > 0.2) | stem, tree, 0).astype(np.int64)
    x[:2], y[:2], z[:2] = (0.0, 11.999), (0.0, 8.999), (0.0, 9.999)                   # the grid is 48 x 36 x 40 whatever the rounding to f32 does
    xyz = np.column_stack([np.clip(x, 0.0, 11.999), np.clip(y, 0.0, 8.999), np.clip(z, 0.0, 9.999)])
    order = np.lexsort((np.floor(xyz[:, 0] / 0.5), np.floor(xyz[:, 1] / 0.5)))        # spatially sorted, as tiles and results come
    xyz, lab = np.ascontiguousarray(xyz[order]), np.ascontiguousarray(lab[order])
    P = 200
    origins = np.column_stack([rng.uniform(0.0, 12.0, P), rng.uniform(0.0, 9.0, P), rng.uniform(0.3, 7.0, P)])
    origins[:20] = np.minimum(np.round(origins[:20] * 4.0) / 4.0, [11.75, 8.75, 9.75])   # on voxel faces, edges and corners, inside the grid
    origins[20:24] = [[-0.5, 1.0, 1.0], [3.0, 9.5, 1.0], [3.0, 3.0, 10.5], [12.0, 3.0, 1.0]]             # outside the grid
    skip = rng.integers(-1, 7, P).astype(np.int32)
    return xyz, lab, origins, skip


@pytest.fixture(scope="module")
def cloud():
    from treelearn_amd.util.light import sky_directions
    xyz, lab, origins, skip = _random_cloud()
    x32 = xyz.astype(np.float32)
    dirs, ring, lo, hi = sky_directions()
    out = dict(xyz=xyz, x32=x32, lab=lab, origins=origins, skip=skip, sky=(dirs, ring, lo, hi))
    for key, pts in (("64", xyz), ("32", x32)):
        vox = ref.light_voxels(pts, lab, VOXEL)
        m = ref.march(vox, origins, dirs, ring, 9, skip=skip, **MARCH)
        assert vox["n"] == [48, 36, 40] and vox["i0"] == [0, 0, 0]
        total = m["counts"].sum(0)                                                    # [R, 4]
        assert (total.sum(0) > 0).all(), "all four exit codes occur"
        assert ((total[:, 0] > 0) & (total[:, 1] + total[:, 2] > 0)).any(), "a ring is neither fully open nor fully blocked"
        assert m["status"].sum() == 4 and int(total.sum()) == 196 * 324
        out["vox" + key], out["march" + key] = vox, m
    return out


def _device_rows(xyz, stride):
    if stride == 4:
        wide = np.full((len(xyz), 4), 7.0, xyz.dtype)
        wide[:, :3] = xyz
        dev = torch.from_numpy(wide).cuda()[:, :3]
        assert dev.stride() == (4, 1)
        return dev
    return torch.from_numpy(np.ascontiguousarray(xyz)).cuda()


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_random_cloud(cloud, dtype, stride, order):
    from treelearn_amd.util.light import light_voxels
    key = "64" if dtype == "f64" else "32"
    xyz, lab = (cloud["xyz"] if dtype == "f64" else cloud["x32"]), cloud["lab"]
    if order == "shuffled":
        p = np.random.default_rng(4).permutation(len(lab))
        xyz, lab = xyz[p], lab[p]
    vox = light_voxels(_device_rows(xyz, stride), torch.from_numpy(lab).cuda(), VOXEL)
    assert_voxels(vox, cloud["vox" + key])
    dirs, ring, _, _ = cloud["sky"]
    assert_march(gpu_march(vox, cloud["origins"], dirs, ring, 9, skip=cloud["skip"], **MARCH), cloud["march" + key])
    if stride == 3 and order == "sorted":
        nolab = light_voxels(xyz, None, VOXEL)                                        # host arrays, no labels: the same bits, skip ignored
        assert nolab.owner is None and np.array_equal(_occ(nolab), _occ(vox))
        free = ref.march(dict(cloud["vox" + key], owner=None), cloud["origins"], dirs, ring, 9, **MARCH)
        assert_march(gpu_march(nolab, cloud["origins"], dirs, ring, 9, skip=cloud["skip"], **MARCH), free)


def test_row_order_does_not_change_a_bit(cloud):
    from treelearn_amd.util.light import light_voxels, march
    xyz, lab = cloud["xyz"], cloud["lab"]
    dirs, ring, _, _ = cloud["sky"]
    p = np.random.default_rng(9).permutation(len(lab))
    a, b = light_voxels(xyz, lab, VOXEL), light_voxels(xyz[p], lab[p], VOXEL)
    assert torch.equal(a.occ, b.occ) and torch.equal(a.owner, b.owner)
    ma = march(a, cloud["origins"], dirs, ring, 9, skip=cloud["skip"], **MARCH)
    mb = march(b, cloud["origins"][::-1].copy(), dirs, ring, 9, skip=cloud["skip"][::-1].copy(), **MARCH)
    assert torch.equal(ma["counts"], mb["counts"].flip(0)) and torch.equal(ma["status"], mb["status"].flip(0))


def test_sensor_grid_against_the_restatement(cloud):
    from treelearn_amd.util.light import light_model
    from treelearn_amd.util.terrain import terrain_model
    xyz, lab = cloud["xyz"], cloud["lab"]
    dirs, ring, lo, hi = cloud["sky"]
    t = terrain_model(xyz, lab)
    st = []
    light = light_model(xyz, t, lab, offset=[100.0, 200.0, 50.0], stages=st, sensor_cell=2.0, max_range=9.0)
    assert [k for k, _ in st] == ["voxels", "sensor grid", "derive"]
    assert (light.sensor_ix0, light.sensor_iy0, light.sensor_nx, light.sensor_ny) == (0, 0, 6, 5) and light.n_no_ground == 0
    gx, gy = np.meshgrid((np.arange(6) + 0.5) * 2.0, (np.arange(5) + 0.5) * 2.0)
    ground = t.sample(np.column_stack([gx.reshape(-1), gy.reshape(-1)])).cpu().numpy()
    _exact("sensor_z", light.sensor_z, (ground + 1.3).reshape(5, 6))
    origins = np.column_stack([gx.reshape(-1), gy.reshape(-1), ground + 1.3])
    want = ref.march(cloud["vox64"], origins, dirs, ring, 9, max_range=9.0)
    _exact("counts", light.counts, want["counts"].reshape(5, 6, 9, 4))
    assert light.n_outside == int(want["status"].sum()) == 6                          # the row of sensors at y = 9 lies beyond the last voxel
    rays = np.bincount(ring)
    for j in range(5):
        for i in range(6):
            k = j * 6 + i
            d = ref.derive(want["counts"][k], rays, lo, hi)
            for name in DERIVED:
                w = np.full_like(np.asarray(d[name], np.float64), np.nan) if want["status"][k] else d[name]
                _close(f"{name}[{j}, {i}]", getattr(light, name)[j, i], w)
    known = light.openness[:4]
    assert np.isfinite(known).all() and 0.0 < known.min() < known.max() < 1.0 and np.isfinite(light.lai_e[:4]).all() and (light.lai_e[:4] > 0).all()
    host = light.to_host()
    assert host["x0"] == 100.0 and host["y0"] == 200.0 and host["z0"] == 50.0 and host["sensor_x0"] == 100.0 and host["voxel"] == 0.25
    _exact("occ", host["occ"], cloud["vox64"]["occ"])
    assert "owner" not in host                                                        # the dense owner grid stays on the device
    _exact("owner", light.vox.owner.cpu().numpy(), cloud["vox64"]["owner"])
    assert host["openness"].shape == (5, 6) and host["gap"].shape == (5, 6, 9) and host["counts"].dtype == np.int32 and host["n_outside"] == 6
    assert np.array_equal(host["sensor_z"], light.sensor_z + 50.0)


def test_point_light_and_hemisphere(cloud):
    from treelearn_amd.util.light import hemi_directions, light_model, sky_directions, SKY_RGB
    from treelearn_amd.util.terrain import terrain_model
    sub = slice(None, None, 40)
    xyz, lab = np.ascontiguousarray(cloud["xyz"][sub]), np.ascontiguousarray(cloud["lab"][sub])
    light = light_model(xyz, terrain_model(cloud["xyz"], cloud["lab"]), lab, voxel=0.5, max_range=9.0)
    vox = ref.light_voxels(xyz, lab, 0.5)
    # openness per row: from the centre of the row's voxel, 2 rings x 8 azimuths
    got = light.point_light(n_rings=2, n_azimuth=8)
    assert got.shape == (len(xyz),) and got.dtype == np.float64
    dirs, ring, lo, hi = sky_directions(2, 8)
    idx = np.floor(xyz / 0.5).astype(np.int64) - np.array(vox["i0"])
    m = ref.march(vox, ((np.array(vox["i0"]) + idx).astype(np.float64) + 0.5) * 0.5, dirs, ring, 2, max_range=9.0)
    want = np.array([ref.derive(m["counts"][k], np.bincount(ring), lo, hi)["openness"] for k in range(len(xyz))])
    _close("point_light", got, want)
    assert np.isfinite(got).any() and got[np.isfinite(got)].min() < got[np.isfinite(got)].max()
    far = light.point_light(np.array([[50.0, 0.0, 0.0], xyz[7]]), n_rings=2, n_azimuth=8)
    assert np.isnan(far[0]) and (far[1] == got[7] or np.isnan(got[7]))
    # the hemispherical view from under the crowns
    hd, inside = hemi_directions(32)
    assert inside.shape == (32, 32) and inside.sum() == len(hd) and not inside[0, 0] and inside[16, 16]
    assert np.abs(np.sqrt((hd * hd).sum(1)) - 1.0).max() <= 1e-15 and (hd[:, 2] > 0).all()
    code, first = light.hemi_rays(6.0, 4.5, 32, z=1.0)
    w = ref.march(vox, [[6.0, 4.5, 1.0]], hd, np.zeros(len(hd), np.int32), 1, max_range=9.0)
    _exact("hemi code", code[inside], w["code"][0])
    _exact("hemi first", first[inside], w["first"][0])
    assert (code[~inside] == 254).all() and np.isnan(first[~inside]).all()
    img = light.hemi_picture(6.0, 4.5, 32, z=1.0)
    assert img.shape == (32, 32, 3) and img.dtype == np.uint8 and (img[~inside] == 0).all()
    sky = (code == 1) | (code == 2)
    assert sky.any() and (code == 0).any() and (img[sky] == SKY_RGB).all() and (img[code == 0][:, 1] >= 30).all() and (img[code == 0][:, 1] <= 160).all()


# ------------------------------------------------------------------ the tree columns
def _small_plot(labelled=False):
    from treelearn_amd.synth import make_tile
    t = make_tile(extent=12, voxel=0.1, n_trees=6, fill=0.10, seed=5)
    pts = t["points"].astype(np.float64) + np.array([1000.0, 2000.0, 50.0])
    return np.column_stack([pts, t["instance_label"].astype(np.float64)]) if labelled else pts


TREE_CFG = dict(voxel=0.5, n_rings=5, n_azimuth=12, max_range=30.0)


def _want_columns(xyz, lab, cfg):
    from treelearn_amd.util.light import sky_directions
    p = dict(ref.DEFAULTS, **cfg)
    vox = ref.light_voxels(xyz, lab, p["voxel"])
    vox["tree_voxels"] = ref.tree_voxels(xyz, lab, vox)
    return ref.tree_columns(vox, int(lab.max()), sky_directions(p["n_rings"], p["n_azimuth"], p["max_zenith"]), **cfg)


def assert_columns(got, want):
    from treelearn_amd.util.light import LIGHT_COLUMNS
    assert tuple(k for k in got if k.startswith("light_")) == LIGHT_COLUMNS
    _exact("light_columns", got["light_columns"], want["light_columns"])
    for k in LIGHT_COLUMNS[1:]:
        assert got[k].dtype == np.float64
        _close(k, got[k], want[k])


def test_tree_columns_on_the_synthetic_plot():
    from treelearn_amd.util.inventory import COLUMNS, tree_inventory
    from treelearn_amd.util.light import light_model
    from treelearn_amd.util.terrain import terrain_model
    data = _small_plot(labelled=True)
    xyz = data[:, :3] - data[:, :3].mean(0)
    lab = data[:, 3].astype(np.int64)
    want = _want_columns(xyz, lab, TREE_CFG)
    assert (want["light_columns"] > 0).all() and len(want["light_columns"]) == 6 and np.isfinite(want["light_openness"]).all()
    inv = tree_inventory(xyz, lab, light=True, light_cfg=TREE_CFG)
    assert tuple(inv)[:len(COLUMNS)] == COLUMNS and tuple(inv)[len(COLUMNS):] == tuple(k for k in inv if k.startswith("light_"))
    assert_columns(inv, want)
    plain = tree_inventory(xyz, lab)
    assert tuple(plain) == COLUMNS and all(np.array_equal(plain[k], inv[k], equal_nan=True) for k in COLUMNS)
    light = light_model(xyz, terrain_model(xyz, lab), lab, **TREE_CFG)
    assert_columns(light.tree_light(), want)
    more = light.tree_light(T=8)                                                      # trees without rows: 0 columns and NaN
    assert more["light_columns"].tolist()[6:] == [0, 0] and all(np.isnan(more[k][6:]).all() for k in ("light_openness", "light_gap_zenith",
                                                                                                       "light_lai_above", "light_edge_share"))


def test_a_lone_tall_tree_and_a_tree_under_a_crown():
    """Tree 1 stands alone and is the tallest: its zenith gap is exactly 1.  Tree 2 spreads a closed crown at 10 to 11 m over tree 3, whose
    top is at 5 m: tree 3's zenith gap is below 1, and exactly 1 once the rays skip nothing but tree 2 is taken away."""
    from treelearn_amd.util.inventory import tree_inventory
    rng = np.random.default_rng(2)
    g = np.column_stack([rng.uniform(0, 30, 4000), rng.uniform(0, 12, 4000), rng.uniform(0, 0.1, 4000)])
    t1 = np.column_stack([rng.normal(25.0, 0.6, 3000), rng.normal(6.0, 0.6, 3000), rng.uniform(0.1, 16.0, 3000)])
    t2 = np.column_stack([rng.uniform(2, 10, 20000), rng.uniform(2, 10, 20000), rng.uniform(10.0, 11.0, 20000)])
    t3 = np.column_stack([rng.normal(6.0, 0.4, 1500), rng.normal(6.0, 0.4, 1500), rng.uniform(0.1, 5.0, 1500)])
    xyz = np.concatenate([g, t1, t2, t3])
    lab = np.concatenate([np.zeros(4000), np.full(3000, 1), np.full(20000, 2), np.full(1500, 3)]).astype(np.int64)
    cfg = dict(voxel=0.5, n_rings=6, n_azimuth=12, max_range=40.0)
    inv = tree_inventory(xyz, lab, light=True, light_cfg=cfg)
    assert_columns(inv, _want_columns(xyz, lab, cfg))
    assert inv["light_gap_zenith"][0] == 1.0 and inv["light_gap_zenith"][2] < 0.5 and inv["light_openness"][2] < inv["light_openness"][0]
    assert inv["light_lai_above"][2] > inv["light_lai_above"][0] and inv["light_gap_zenith"][1] == 1.0
    keep = lab != 2
    alone = tree_inventory(xyz[keep], lab[keep], light=True, light_cfg=cfg)
    assert alone["light_gap_zenith"][2] == 1.0 and alone["light_columns"][1] == 0 and np.isnan(alone["light_openness"][1])


# ------------------------------------------------------------------ the C entry points
def test_c_entry_points_null_zero_size_and_out_of_range():
    from treelearn_amd import _hip
    L, P = _hip.lib(), _hip.ptr
    dev = "cuda"
    pts = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    lab = torch.zeros(4, dtype=torch.int64, device=dev)
    occ = torch.full((8,), 7, dtype=torch.int32, device=dev)
    owner = torch.full((8,), 7, dtype=torch.int32, device=dev)
    err = torch.full((2,), 7, dtype=torch.int32, device=dev)
    org = torch.zeros((2, 3), dtype=torch.float64, device=dev)
    dirs = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64, device=dev)
    ring = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.full((8,), 7, dtype=torch.int32, device=dev)
    status = torch.full((2,), 7, dtype=torch.int32, device=dev)
    code = torch.full((2,), 7, dtype=torch.uint8, device=dev)
    first = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    s, ERR = _hip.stream(), _hip.TL_ERR_ARG
    vx = lambda *a, **k: L.tl_light_voxels(*a)                                        # noqa: E731
    ok_v = [P(pts), 1, 3, 4, P(lab), 1.0, 0, 0, 0, 2, 2, 2, P(occ), P(owner), P(err), s]
    ok_m = [P(org), None, 2, P(dirs), P(ring), 1, 1, P(occ), P(owner), 1.0, 0, 0, 0, 2, 2, 2, 60.0, 1, P(counts), P(status), P(code), P(first), s]

    def with_(args, **at):
        a = list(args)
        for i, v in at.items():
            a[int(i[1:])] = v
        return a

    # tl_light_voxels: null pointers, labels without owner and the reverse, sizes and the grid's limits
    for bad in (dict(_0=None), dict(_12=None), dict(_14=None), dict(_4=None), dict(_13=None), dict(_1=2), dict(_2=2), dict(_3=-1), dict(_5=0.0),
                dict(_5=float("nan")), dict(_5=float("inf")), dict(_9=-1), dict(_9=8193), dict(_9=8192, _10=8192, _11=8), dict(_9=0),
                dict(_6=1 << 53), dict(_0=_hip._vp(pts.data_ptr() + 4))):
        assert vx(*with_(ok_v, **bad)) == ERR, bad
    assert vx(*with_(ok_v, _4=None, _13=None, _9=8192, _10=8192, _11=33)) == ERR       # 2^26 * 33 > 2^31 without an owner grid
    # tl_light_march
    for bad in (dict(_0=None), dict(_3=None), dict(_4=None), dict(_7=None), dict(_18=None), dict(_19=None), dict(_2=-1), dict(_5=-1), dict(_6=0),
                dict(_6=65537), dict(_9=0.0), dict(_9=float("nan")), dict(_13=8193), dict(_13=0), dict(_16=0.0), dict(_16=float("inf")),
                dict(_16=float("nan")), dict(_17=0), dict(_10=-(1 << 53)), dict(_21=_hip._vp(first.data_ptr() + 4))):
        assert L.tl_light_march(*with_(ok_m, **bad)) == ERR, bad
    torch.cuda.synchronize()
    assert occ.tolist() == [7] * 8 and owner.tolist() == [7] * 8 and err.tolist() == [7, 7] and counts.tolist() == [7] * 8
    assert status.tolist() == [7, 7] and code.tolist() == [7, 7] and first.tolist() == [7.0, 7.0]
    # zero sizes: TL_OK without a launch; tl_light_voxels still clears occ, owner and *err
    assert L.tl_light_march(*with_(ok_m, _2=0)) == 0
    assert L.tl_light_march(*with_(ok_m, _2=0, _13=0, _14=0, _15=0)) == 0
    assert vx(*with_(ok_v, _3=0, _9=0, _10=0, _11=0)) == 0
    torch.cuda.synchronize()
    assert occ.tolist() == [7] * 8 and owner.tolist() == [7] * 8 and err.tolist() == [0, 7] and counts.tolist() == [7] * 8 and status.tolist() == [7, 7]
    assert vx(*with_(ok_v, _3=0, _13=P(owner[:8]))) == 0
    torch.cuda.synchronize()
    assert occ.tolist() == [0] * 4 + [7] * 4 and owner.tolist() == [-1] * 8              # 2 x 2 rows of one word; 2 x 2 x 2 owners
    # an empty table: the origins' status and cleared counts, nothing else
    assert L.tl_light_march(*with_(ok_m, _5=0)) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0] * 8 and status.tolist() == [0, 0] and code.tolist() == [7, 7] and first.tolist() == [7.0, 7.0]


def test_row_kernel_skips_and_flags_what_it_refuses():
    """The device side of the refusals, which light_voxels' host checks come before: a row with a NaN coordinate or a voxel outside the
    grid, and a label beyond 32 bits, are skipped and set the flag; a label below 0 occupies its voxel and owns nothing."""
    from treelearn_amd import _hip
    L, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    nan = float("nan")
    pts = torch.tensor([[0.5, 0.5, 0.5], [nan, 0.5, 0.5], [1.5, 1.5, 1.5], [5.0, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 0.5, 0.5], [0.5, 0.5, -0.5],
                        [0.5, 0.5, 1.5]], dtype=torch.float32, device="cuda")
    lab = torch.tensor([3, 9, -4, 9, 1 << 40, 0, 9, 2], dtype=torch.int64, device="cuda")
    occ = torch.full((2, 2, 1), 7, dtype=torch.int32, device="cuda")
    owner = torch.full((2, 2, 2), 7, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.tl_light_voxels(P(pts), 0, 3, 8, P(lab), 1.0, 0, 0, 0, 2, 2, 2, P(occ), P(owner), P(err), s) == 0
    assert err.item() == 1 and occ.tolist() == [[[3], [1]], [[1], [2]]]                # the row with the label beyond 32 bits still set its bit
    assert owner.tolist() == [[[3, 0], [-1, -1]], [[2, -1], [-1, -1]]]
    clean = pts[[0, 2, 5, 7]].contiguous()
    assert L.tl_light_voxels(P(clean), 0, 3, 4, None, 1.0, 0, 0, 0, 2, 2, 2, P(occ), None, P(err), s) == 0
    assert err.item() == 0 and occ.tolist() == [[[3], [0]], [[1], [2]]]


# ------------------------------------------------------------------ segment_forest, save_results, the command line
SAMPLE = dict(stride=1.0)                                                 # tiles side by side: four cover the plot
LIGHT_CFG = dict(voxel=0.5, sensor_cell=3.0, n_rings=5, n_azimuth=12)
PREVIEW_CFG = dict(size=128)


@pytest.fixture(scope="module")
def segmented():
    """segment_forest on the 12 m plot of six trees of tests/test_gpu_crown.py with the pinned-head random model of
    tests/test_gpu_inventory.py: with light, inventory and preview; with terrain and preview only; without any flag."""
    from treelearn_amd.model import TreeLearn
    from treelearn_amd.synth import random_state_dict
    from treelearn_amd.util.segment import MODEL_CFG, segment_forest
    pts = _small_plot()
    sd = random_state_dict(7, channels=32, num_blocks=7)
    sd["offset_linear.3.weight"].zero_(); sd["offset_linear.3.bias"].zero_()
    sd["semantic_linear.3.weight"].zero_(); sd["semantic_linear.3.bias"][:] = torch.tensor([2.0, -2.0])
    m = TreeLearn(**MODEL_CFG).cuda().eval()
    m.load_state_dict(sd)
    cfg = dict(use_hdbscan=False, tau_vert=0.0, tau_off=1e9, tau_group=0.3, tau_min=20)
    kw = dict(sample_cfg=SAMPLE, grouping_cfg=cfg, return_type="original")
    with torch.no_grad():
        res = segment_forest(pts, m, inventory=True, light=True, light_cfg=LIGHT_CFG, preview=True, preview_cfg=PREVIEW_CFG, **kw)
        base = segment_forest(pts, m, inventory=True, terrain=True, preview=True, preview_cfg=PREVIEW_CFG, **kw)
        plain = segment_forest(pts, m, **kw)
    return pts, res, base, plain


def test_segment_forest_without_the_flag_is_unchanged(segmented):
    from treelearn_amd.util.light import LIGHT_COLUMNS
    _, res, base, plain = segmented
    assert set(plain) == {"coords", "labels", "categories"}
    assert set(base) == set(plain) | {"inventory", "terrain", "height_above_ground", "preview"} and set(res) == set(base) | {"light"}
    for k in plain:
        assert np.array_equal(plain[k], res[k]) and np.array_equal(plain[k], base[k]), k
    assert np.array_equal(base["height_above_ground"], res["height_above_ground"], equal_nan=True)
    assert all(np.array_equal(base["terrain"][k], res["terrain"][k], equal_nan=True) for k in base["terrain"])
    assert not any(k.startswith("light") for k in base["inventory"]) and tuple(res["inventory"])[-5:] == LIGHT_COLUMNS
    assert tuple(res["inventory"])[:-5] == tuple(base["inventory"])
    for k, v in base["inventory"].items():
        assert v.dtype == res["inventory"][k].dtype and v.tobytes() == res["inventory"][k].tobytes(), k
    assert set(res["preview"]) == set(base["preview"]) | {"light"} and "light" not in base["preview"]
    for k, v in base["preview"].items():
        assert v.tobytes() == res["preview"][k].tobytes(), k
    pic = res["preview"]["light"]
    assert pic.dtype == np.uint8 and pic.ndim == 3 and pic.shape[2] == 3 and pic.shape[0] >= 4


def test_segment_forest_light_files_and_cli(segmented, tmp_path):
    """The light model of segment_forest is light_model on the returned coords and labels in the frame segment_forest works in: the test
    centres the cloud as segment_forest does (the same torch expression on the same device)."""
    from treelearn_amd.util.light import cloud_light, light_model, SKY_RGB
    from treelearn_amd.util.segment import save_results
    from treelearn_amd.util.terrain import terrain_model
    pts, res, base, plain = segmented
    xyz = torch.from_numpy(pts).to("cuda", torch.float64)
    mean = xyz.mean(0)
    assert np.array_equal((xyz - mean + mean).cpu().numpy(), res["coords"])
    centred = xyz - mean
    t = terrain_model(centred, res["labels"], offset=mean)
    light = light_model(centred, t, res["labels"], offset=mean, **LIGHT_CFG)
    want, got = light.to_host(), res["light"]
    assert set(got) == set(want) and "owner" not in got and "occ" in got and got["voxel"] == 0.5 and got["sensor_cell"] == 3.0
    for k in want:
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.array_equal(got[k], want[k], equal_nan=np.asarray(want[k]).dtype.kind == "f"), k
    mean_h = mean.cpu().numpy()
    assert got["x0"] == light.vox.ix0 * 0.5 + mean_h[0] and got["sensor_y0"] == light.sensor_iy0 * 3.0 + mean_h[1]
    cols = light.tree_light(T=len(res["inventory"]["tree_id"]))
    for k, v in cols.items():
        assert np.array_equal(res["inventory"][k], v, equal_nan=True), k

    save_results(res, str(tmp_path / "api"), "plot", ["npy"], save_treewise=False)
    with np.load(tmp_path / "api" / "light.npz") as f:
        assert set(f.files) == set(got) and all(np.array_equal(f[k], got[k], equal_nan=f[k].dtype.kind == "f") and f[k].dtype == np.asarray(got[k]).dtype
                                                for k in got)
    assert (tmp_path / "api" / "preview" / "light.png").exists()
    header = open(tmp_path / "api" / "tree_inventory.csv").readline().strip().split(",")
    assert header[-6:-1] == list(cols) and header[-1] == "category"
    save_results(plain, str(tmp_path / "plain"), "plot", ["npy"], save_treewise=False)
    assert not (tmp_path / "plain" / "light.npz").exists()

    # the command line in a child process on the plot with its true labels (label 0 = ground), against the same call made here
    forest = tmp_path / "labelled.npy"
    data = _small_plot(labelled=True)
    np.save(forest, data)
    env = dict(os.environ, PYTHONPATH=REPO)
    # the picture from the middle of the plot with max_range = 6 m: a ray is sky when nothing lies within 6 m of the sensor, which holds
    # for the directions under the crowns (they begin higher up) and fails towards the stems and along the ground: both kinds of pixel
    hx, hy = (float(v) for v in np.round(data[:, :2].mean(0), 3))
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "treelearn_amd.util.light", "--forest", str(forest), "--out",
                        str(tmp_path / "cli.npz"), "--light-voxel", "0.5", "--sensor-cell", "3", "--rings", "5", "--azimuths", "12", "--max-range", "6", "--hemi", f"{hx},{hy}",
                        "--hemi-out", str(tmp_path / "sky.png"), "--hemi-size", "48"], capture_output=True, text=True, cwd=REPO, env=env)
    assert p.returncode == 0 and "mean openness" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    mine, _ = cloud_light(data, max_range=6.0, **LIGHT_CFG)
    h = mine.to_host()
    with np.load(tmp_path / "cli.npz") as f:
        assert set(f.files) == set(h) and all(np.array_equal(f[k], h[k], equal_nan=f[k].dtype.kind == "f") for k in h)
    assert np.isfinite(h["openness"]).any() and h["n_no_ground"] == 0
    img = _read_png(tmp_path / "sky.png")
    assert img.shape == (48, 48, 3)
    same = mine.hemi_picture(hx - mine.offset[0], hy - mine.offset[1], 48)
    assert np.array_equal(img, same)
    sky = (img == np.array(SKY_RGB, np.uint8)).all(2)
    blocked = (img[:, :, 1] > img[:, :, 0]) & (img[:, :, 1] > img[:, :, 2]) & ~sky
    assert sky.sum() >= 10 and blocked.sum() >= 10, (int(sky.sum()), int(blocked.sum()))


def _read_png(path):
    """An 8-bit RGB PNG whose rows all use filter 0, as util.render.write_png writes it, as u8 [H, W, 3]."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, w, h = 8, b"", 0, 0
    while at < len(raw):
        n, tag = struct.unpack(">I", raw[at:at + 4])[0], raw[at + 4:at + 8]
        body = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            assert (depth, colour) == (8, 2)
        elif tag == b"IDAT":
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3).copy()
