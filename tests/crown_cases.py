"""Crown-structure cases worked by hand, shared by tests/test_host_crown.py (through the numpy restatement) and
tests/test_gpu_crown.py (through tl_crown_voxel_keys / tl_crown_structure).  Each case is a dict: xyz f64 [N, 3], lab i64 [N], cfg (crown
parameters), check(res) asserting on the crown columns and res["crown_profile"], and optionally
  z_ref   a per-tree reference height in place of z_low (NaN: a tree over unfilled terrain), applied to the inventory's table.
Every coordinate is dyadic and every row of a voxel sits at the voxel's centre (cells of 0.25 m, layers of 0.5 m): cell (ix, iy), layer l
is ((ix + 0.5) / 4, (iy + 0.5) / 4, l / 2 + 0.25).  A tree stands on four rows at z = 0 in its anchor cell (z_low = 0: rank 3 of more than
11 rows) and ends in four rows at z_top in the same cell; its base rows (z <= 0.5) all lie at the anchor's centre, so the position is
exactly that centre and every implementation computes the same bits.  Cells then sit exactly on sector borders (u = 0, |u| = |v|): the
margin condition of the restatement does not apply to these cases (`exact`), the comparisons decide them the same way everywhere."""
import numpy as np

NAN = np.isnan
ANCHOR = (12, -8)                                  # centre (3.125, -1.875)
FLOATS = ("crown_base_h", "crown_length", "crown_ratio", "crown_widest_h", "crown_volume", "crown_proj_area", "crown_x", "crown_y",
          "crown_offset", "crown_radius_max", "crown_radius_mean")


def _centre(ix, iy):
    return (ix + 0.5) / 4, (iy + 0.5) / 4


def _voxels(vox):
    return np.array([[*_centre(ix, iy), l / 2 + 0.25] for ix, iy, l in vox], np.float64).reshape(-1, 3)


def _block(x0, x1, y0, y1, layers):
    """The voxels of the cells x0 .. x1 by y0 .. y1 (inclusive) in every layer of `layers`."""
    return [(ix, iy, l) for l in layers for ix in range(x0, x1 + 1) for iy in range(y0, y1 + 1)]


def _stem(layers, anchor=ANCHOR):
    return [(anchor[0], anchor[1], l) for l in layers]


def _tree(vox, z_top, anchor=ANCHOR, extra=()):
    ax, ay = _centre(*anchor)
    ends = [[ax, ay, 0.0]] * 4 + [[ax, ay, z_top]] * 4
    return np.concatenate([np.array(ends), _voxels(vox), np.array(list(extra), np.float64).reshape(-1, 3)])


def _shuffled(xyz, lab, seed):
    p = np.random.default_rng(seed).permutation(len(xyz))
    return np.ascontiguousarray(xyz[p]), np.ascontiguousarray(np.asarray(lab, np.int64)[p])


def _one(xyz, seed):
    return _shuffled(xyz, np.ones(len(xyz), np.int64), seed)


def _no_crown(res, t):
    assert all(NAN(res[k][t]) for k in FLOATS) and res["crown_voxels"][t] == 0 and res["crown_proj_cells"][t] == 0
    assert NAN(res["crown_profile"]["radii"][t]).all()


def _types(res):
    p = res["crown_profile"]
    assert all(res[k].dtype == np.int64 for k in ("crown_layers", "crown_voxels", "crown_proj_cells")) and all(res[k].dtype == np.float64 for k in FLOATS)
    assert p["h"].dtype == np.float64 and p["n"].dtype == np.int64 and p["cells"].dtype == np.int64 and p["radii"].dtype == np.float64
    assert p["h"].shape == p["n"].shape == p["cells"].shape and p["radii"].shape == (len(res["crown_layers"]), 8)


LOLLIPOP = _stem(range(8)) + _block(10, 13, -10, -7, range(8, 12))


def case_lollipop():
    """A one-cell stem in layers 0-7 under a crown of 4 x 4 cells in layers 8-11.  The stem layer under the crown is thin (1 * 100 <
    10 * 16): one gap is bridged, the second ends the walk, so the base stays at layer 8.  The anchor is cell (12, -8), the crown cells
    10 .. 13 by -10 .. -7: u, v in {-0.5, -0.25, 0, 0.25}."""
    xyz, lab = _one(_tree(LOLLIPOP, 5.75), 1)

    def check(res):
        _types(res)
        p = res["crown_profile"]
        assert p["h"].shape == (1, 12) and np.array_equal(p["h"][0], 0.5 * np.arange(12))
        assert p["n"][0].tolist() == [5] + [1] * 7 + [16] * 3 + [20] and p["cells"][0].tolist() == [1] * 8 + [16] * 4
        assert res["crown_layers"][0] == 12 and res["crown_base_h"][0] == 4.0 and res["crown_length"][0] == 1.75
        assert res["crown_ratio"][0] == 1.75 / 5.75 and res["crown_widest_h"][0] == 4.25
        assert res["crown_voxels"][0] == 64 and res["crown_volume"][0] == 2.0
        assert res["crown_proj_cells"][0] == 16 and res["crown_proj_area"][0] == 1.0
        assert res["crown_x"][0] == 3.0 and res["crown_y"][0] == -2.0 and res["crown_offset"][0] == np.sqrt(0.03125)
        want = np.sqrt(np.array([0.0625, 0.125, 0.0625, 0.3125, 0.3125, 0.5, 0.3125, 0.125]))
        assert np.array_equal(p["radii"][0], want)
        assert res["crown_radius_max"][0] == np.sqrt(0.5)
        s = np.float64(0.0)
        for r in want:
            s = s + r
        assert res["crown_radius_mean"][0] == s / 8.0
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


THIN = _stem(range(6)) + _block(10, 13, -9, -8, [6]) + _stem([7]) + _block(10, 13, -9, -8, [8]) + _block(10, 13, -10, -7, [9])


def case_thin_layer_bridged():
    """Layer 9 is the widest (16 cells), layers 8 and 6 hold 8, layer 7 only the stem: with max_gap = 1 the walk bridges it and the base is
    layer 6; layers 5 and 4 are thin, the second ends the walk."""
    xyz, lab = _one(_tree(THIN, 4.75), 2)

    def check(res):
        _types(res)
        assert res["crown_profile"]["cells"][0].tolist() == [1] * 6 + [8, 1, 8, 16] and res["crown_layers"][0] == 10
        assert res["crown_base_h"][0] == 3.0 and res["crown_widest_h"][0] == 4.75 and res["crown_voxels"][0] == 33
        assert res["crown_proj_cells"][0] == 16 and res["crown_length"][0] == 1.75
    return dict(xyz=xyz, lab=lab, cfg=dict(max_gap=1), check=check)


def case_thin_layer_not_bridged():
    xyz, lab = _one(_tree(THIN, 4.75), 3)

    def check(res):
        assert res["crown_base_h"][0] == 4.0 and res["crown_voxels"][0] == 24 and res["crown_proj_cells"][0] == 16
        assert res["crown_volume"][0] == 0.75
    return dict(xyz=xyz, lab=lab, cfg=dict(max_gap=0), check=check)


INCLUSIVE = _stem(range(8)) + [(12, -8, 8), (13, -8, 8)] + _block(10, 14, -10, -7, [9])


def case_threshold_inclusive():
    """cells[8] * 100 = 200 = base_percent * cells_max = 10 * 20 exactly: layer 8 is crown-like."""
    xyz, lab = _one(_tree(INCLUSIVE, 4.75), 4)

    def check(res):
        assert res["crown_profile"]["cells"][0].tolist() == [1] * 8 + [2, 20]
        assert res["crown_base_h"][0] == 4.0 and res["crown_voxels"][0] == 22 and res["crown_proj_cells"][0] == 20
    return dict(xyz=xyz, lab=lab, cfg=dict(base_percent=10), check=check)


def case_threshold_missed():
    """The same tree with base_percent = 11: 200 < 220, layer 8 is thin and the base is the widest layer itself."""
    xyz, lab = _one(_tree(INCLUSIVE, 4.75), 5)

    def check(res):
        assert res["crown_base_h"][0] == 4.5 and res["crown_voxels"][0] == 20 and res["crown_proj_cells"][0] == 20
        assert res["crown_length"][0] == 0.25
    return dict(xyz=xyz, lab=lab, cfg=dict(base_percent=11), check=check)


def case_wide_layer_below_min_height():
    """Layer 1 (bottom 0.5 m < min_height) holds 25 cells of low vegetation: it takes no part; the widest layer is 8 with 16."""
    vox = _stem([0]) + _block(10, 14, -10, -6, [1]) + _stem(range(2, 8)) + _block(10, 13, -10, -7, [8, 9])
    xyz, lab = _one(_tree(vox, 4.75), 6)

    def check(res):
        assert res["crown_profile"]["cells"][0].tolist() == [1, 25] + [1] * 6 + [16, 16]
        assert res["crown_widest_h"][0] == 4.25 and res["crown_base_h"][0] == 4.0 and res["crown_voxels"][0] == 32
        assert res["crown_proj_cells"][0] == 16
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_shorter_than_min_height():
    """H = 0.75: two layers, both below min_height = 1.0: no crown, but the layers are still counted."""
    xyz, lab = _one(_tree(_stem([0, 0, 0, 0]), 0.75), 7)

    def check(res):
        _types(res)
        p = res["crown_profile"]
        assert p["h"].shape == (1, 2) and p["h"][0].tolist() == [0.0, 0.5] and p["n"][0].tolist() == [8, 4] and p["cells"][0].tolist() == [1, 1]
        assert res["crown_layers"][0] == 2
        _no_crown(res, 0)
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_borders_at_negative_coordinates():
    """Anchor cell (-8, -8).  Rows exactly on layer bottoms (z = 4.0 is layer 8, z = 4.5 layer 9) and exactly on cell borders at negative
    coordinates (x = -2.5 is cell -10: floor, not truncation; y = -2.0 is cell -8)."""
    a = (-8, -8)
    border = [[x, -2.0, 4.0] for x in (-2.5, -2.25, -2.0, -1.75)] + [[-2.0, y, 4.5] for y in (-2.5, -2.25, -2.0, -1.75, -1.5)]
    xyz, lab = _one(_tree(_stem(range(8), a), 4.75, a, border), 8)

    def check(res):
        p = res["crown_profile"]
        assert p["cells"][0].tolist() == [1] * 8 + [4, 5] and p["n"][0].tolist() == [5] + [1] * 7 + [4, 5 + 4]
        assert res["crown_widest_h"][0] == 4.75 and res["crown_base_h"][0] == 4.0 and res["crown_voxels"][0] == 9
        assert res["crown_proj_cells"][0] == 8                         # x cells -10 .. -7 at y cell -8, y cells -10, -9, -7, -6 at x cell -8
        assert res["crown_x"][0] == ((-10 - 9 - 8 - 7 - 8 * 4) / 8 + 0.5) * 0.25 and res["crown_y"][0] == ((-8 * 4 - 10 - 9 - 7 - 6) / 8 + 0.5) * 0.25
    return dict(xyz=xyz, lab=lab, cfg=dict(base_percent=50), check=check)


def case_rows_outside_the_layers():
    """The lollipop with three rows below z_low (rank 3 keeps z_low = 0) and three above z_top in layer 12 and higher, in a cell of their
    own: they are in no layer, in no count and in no projection."""
    ax, ay = _centre(*ANCHOR)
    extra = [[ax, ay, -0.25], [ax, ay, -0.5], [ax, ay, -4.0]] + [[7.625, -1.875, z] for z in (6.0, 6.25, 40.0)]
    xyz, lab = _one(_tree(LOLLIPOP, 5.75, extra=extra), 9)

    def check(res):
        p = res["crown_profile"]
        assert p["h"].shape == (1, 12) and p["n"][0].tolist() == [5] + [1] * 7 + [16] * 3 + [20] and p["n"][0].sum() == len(xyz) - 6
        assert res["crown_voxels"][0] == 64 and res["crown_proj_cells"][0] == 16 and res["crown_x"][0] == 3.0
        assert res["crown_length"][0] == 1.75 and res["crown_profile"]["radii"][0][0] == 0.25
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_max_layers():
    """The lollipop cut at ten layers: the rows of layers 10 and 11 are in no layer; the height is still the tree's."""
    xyz, lab = _one(_tree(LOLLIPOP, 5.75), 10)

    def check(res):
        p = res["crown_profile"]
        assert p["h"].shape == (1, 10) and p["cells"][0].tolist() == [1] * 8 + [16] * 2 and res["crown_layers"][0] == 10
        assert res["crown_voxels"][0] == 32 and res["crown_volume"][0] == 1.0 and res["crown_base_h"][0] == 4.0 and res["crown_length"][0] == 1.75
    return dict(xyz=xyz, lab=lab, cfg=dict(max_layers=10), check=check)


def case_one_sided():
    """A crown of four cells east of the stem only (v = 0, u = 0.25 .. 1.0) plus the anchor cell itself (u = v = 0: sector 0): seven empty
    sectors of 0.0, the centroid two cells east of the position."""
    vox = _stem(range(8)) + [(ix, -8, 8) for ix in range(12, 17)]
    xyz, lab = _one(_tree(vox, 4.25), 11)

    def check(res):
        assert res["crown_profile"]["radii"][0].tolist() == [1.0] + [0.0] * 7
        assert res["crown_radius_max"][0] == 1.0 and res["crown_radius_mean"][0] == 0.125
        assert res["crown_proj_cells"][0] == 5 and res["crown_x"][0] == 3.625 and res["crown_y"][0] == -1.875 and res["crown_offset"][0] == 0.5
        assert res["crown_base_h"][0] == 4.0 and res["crown_voxels"][0] == 5
    return dict(xyz=xyz, lab=lab, cfg=dict(base_percent=50), check=check)


def _two_lollipops():
    t1 = _tree(LOLLIPOP, 5.75)
    t2 = _tree(_stem(range(8)) + _block(10, 13, -10, -7, range(8, 10)), 4.75) + np.array([10.0, 0.0, 0.0])
    return t1, t2


def case_nan_z_ref():
    """Two trees; the second stands where the terrain has no value: zero layers, NaN / 0 in every column, the profile as wide as the first's."""
    t1, t2 = _two_lollipops()
    xyz, lab = _shuffled(np.concatenate([t1, t2]), np.concatenate([np.full(len(t1), 1), np.full(len(t2), 2)]), 12)

    def check(res):
        _types(res)
        p = res["crown_profile"]
        assert p["h"].shape == (2, 12) and NAN(p["h"][1]).all() and (p["n"][1] == 0).all() and (p["cells"][1] == 0).all()
        assert res["crown_layers"].tolist() == [12, 0] and res["crown_voxels"].tolist() == [64, 0]
        _no_crown(res, 1)
    return dict(xyz=xyz, lab=lab, cfg={}, check=check, z_ref=np.array([0.0, np.nan]))


def case_label_gap():
    """Labels {1, 3} (and 0, -1, ignored, inside tree 1's crown layers): tree 2 has no rows, zero layers and NaN / 0 in every column."""
    t1, t3 = _two_lollipops()
    junk = _voxels(_block(20, 24, -10, -7, [8, 9]))
    xyz = np.concatenate([t1, t3, junk, junk])
    lab = np.concatenate([np.full(len(t1), 1), np.full(len(t3), 3), np.zeros(len(junk)), np.full(len(junk), -1)])
    xyz, lab = _shuffled(xyz, lab, 13)

    def check(res):
        p = res["crown_profile"]
        assert p["h"].shape == (3, 12) and NAN(p["h"][1]).all() and NAN(p["h"][2][10:]).all() and not NAN(p["h"][2][:10]).any()
        assert res["crown_layers"].tolist() == [12, 0, 10] and res["crown_voxels"].tolist() == [64, 0, 32]
        assert res["crown_proj_cells"].tolist() == [16, 0, 16] and res["crown_x"][2] == 13.0 and res["crown_y"][2] == -2.0
        _no_crown(res, 1)
        assert np.array_equal(p["radii"][0], p["radii"][2])
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_no_trees():
    def check(res):
        p = res["crown_profile"]
        assert all(p[k].shape == (0, 0) for k in ("h", "n", "cells")) and p["radii"].shape == (0, 8)
        assert all(len(res[k]) == 0 for k in FLOATS + ("crown_layers", "crown_voxels", "crown_proj_cells"))
        assert res["crown_voxels"].dtype == np.int64 and p["n"].dtype == np.int64
    return dict(xyz=np.zeros((3, 3)), lab=np.array([0, -1, 0], np.int64), cfg={}, check=check)


CASES = dict(lollipop=case_lollipop, thin_layer_bridged=case_thin_layer_bridged, thin_layer_not_bridged=case_thin_layer_not_bridged,
             threshold_inclusive=case_threshold_inclusive, threshold_missed=case_threshold_missed,
             wide_layer_below_min_height=case_wide_layer_below_min_height, shorter_than_min_height=case_shorter_than_min_height,
             borders_at_negative_coordinates=case_borders_at_negative_coordinates, rows_outside_the_layers=case_rows_outside_the_layers,
             max_layers=case_max_layers, one_sided=case_one_sided, nan_z_ref=case_nan_z_ref, label_gap=case_label_gap, no_trees=case_no_trees)
