"""Stem-profile cases worked by hand, shared by tests/test_host_stem.py (through the numpy restatement) and
tests/test_gpu_stem.py (through tl_stem_keys / tl_stem_profile).  Each case is a dict: xyz f64 [N, 3], lab i64 [N], cfg (stem parameters),
check(res) asserting on the stem columns and res["stem_profile"], and optionally
  exact   True where rows sit exactly on the corridor or the search radius by construction (dyadic coordinates, the position an exact
          mean): every implementation computes the same bits there, and the margin condition of the restatement does not apply;
  z_ref   a per-tree reference height in place of z_low (NaN: a tree over unfilled terrain), applied to the inventory's table.
Trees stand on four base rows at z = 0 (z_low = 0: rank 3 of more than 11 rows) and end in four rows at their top (z_top).  Stem rows
are rings of 64 rows exactly at slab centres, so the expected values are closed forms."""
import numpy as np

PI = 3.141592653589793
NAN = np.isnan
TOL = 1e-12


def _ring(cx, cy, r, z, n_ang=64, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n_ang) / n_ang
    return np.column_stack([cx + r * np.cos(a), cy + r * np.sin(a), np.full(n_ang, z)])


def _base(cx, cy, z=0.0):
    return np.array([[cx + 0.125, cy, z], [cx - 0.125, cy, z], [cx, cy + 0.125, z], [cx, cy - 0.125, z]])


def _top(cx, cy, z):
    """Four rows at height z, 1.75 m from the stem: outside every corridor used here; they fix z_top = z."""
    return np.array([[cx + 1.75, cy, z]] * 4)


def _tree(cx, cy, layers, z_top):
    """layers: (z, radius, centre offset x) per ring."""
    return np.concatenate([_base(cx, cy)] + [_ring(cx + dx, cy, r, z) for z, r, dx in layers] + [_top(cx, cy, z_top)])


def _shuffled(xyz, lab, seed):
    p = np.random.default_rng(seed).permutation(len(xyz))
    return np.ascontiguousarray(xyz[p]), np.ascontiguousarray(np.asarray(lab, np.int64)[p])


def _one(xyz, seed):
    return _shuffled(xyz, np.ones(len(xyz), np.int64), seed)


HS = 0.5 + 0.5 * np.arange(20)                     # the slab centres of a 10.2 m tree with the defaults: 0.5 .. 10.0


def _frustums(hs, rs):
    V = PI * rs[0] * rs[0] * hs[0]
    for i in range(len(hs) - 1):
        V += PI / 3.0 * (hs[i + 1] - hs[i]) * (rs[i] * rs[i] + rs[i] * rs[i + 1] + rs[i + 1] * rs[i + 1])
    return V


def _assert_states(res, t, states):
    p = res["stem_profile"]
    assert p["state"][t].tolist() == states, p["state"][t].tolist()
    acc = np.asarray(states) == 1
    for k in ("x", "y", "r", "rmse"):
        assert np.array_equal(NAN(p[k][t]), ~acc), k
    assert res["stem_slices"][t] == acc.sum() and p["state"].dtype == np.int64 and p["n"].dtype == np.int64 and res["stem_slices"].dtype == np.int64
    assert (p["n"][t][np.asarray(states) == 0] == 0).all()


def case_cylinder():
    xyz, lab = _one(_tree(3.0, -2.0, [(z, 0.15, 0.0) for z in HS], 10.2), 1)

    def check(res):
        p = res["stem_profile"]
        assert p["h"].shape == (1, 20) and np.array_equal(p["h"][0], HS)
        _assert_states(res, 0, [1] * 20)
        assert p["n"][0].tolist() == [64] * 20
        assert np.abs(p["r"][0] - 0.15).max() <= TOL and np.abs(p["x"][0] - 3.0).max() <= TOL and np.abs(p["y"][0] + 2.0).max() <= TOL
        assert (p["rmse"][0] >= 0).all() and p["rmse"][0].max() <= TOL
        assert res["stem_base_h"][0] == 0.5 and res["stem_top_h"][0] == 10.0
        assert abs(res["stem_volume"][0] - PI * 0.15 ** 2 * res["stem_top_h"][0]) <= TOL
        assert abs(res["stem_lean"][0]) <= TOL and abs(res["stem_taper"][0]) <= TOL and abs(res["dbh_stem"][0] - 0.30) <= TOL
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_cone():
    rs = 0.2 - 0.01 * HS
    xyz, lab = _one(_tree(3.0, -2.0, [(z, r, 0.0) for z, r in zip(HS, rs)], 10.2), 2)

    def check(res):
        _assert_states(res, 0, [1] * 20)
        assert np.abs(res["stem_profile"]["r"][0] - rs).max() <= TOL
        assert abs(res["stem_taper"][0] + 0.02) <= TOL
        assert abs(res["stem_volume"][0] - _frustums(HS, rs)) <= TOL
        assert abs(res["dbh_stem"][0] - 2 * (0.2 - 0.01 * 1.3)) <= TOL and abs(res["stem_lean"][0]) <= TOL
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_lean():
    xyz, lab = _one(_tree(3.0, -2.0, [(z, 0.15, 0.05 * z) for z in HS], 10.2), 3)

    def check(res):
        p = res["stem_profile"]
        _assert_states(res, 0, [1] * 20)
        assert np.abs(p["x"][0] - (3.0 + 0.05 * HS)).max() <= TOL and np.abs(p["y"][0] + 2.0).max() <= TOL
        assert abs(res["stem_lean"][0] - np.arctan(0.05) * 180.0 / PI) <= 1e-11      # degrees: 57 x the error of the centres
        assert abs(res["stem_taper"][0]) <= TOL and abs(res["stem_volume"][0] - PI * 0.15 ** 2 * 10.0) <= TOL
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_crown():
    """A stem up to 3 m under a scattered crown: 40 rows per slab spread over a disc of 0.3 m fit no circle (rmse several cm); three
    misses stop the walk and the slabs above are not visited."""
    rng = np.random.default_rng(4)
    rows = [_tree(3.0, -2.0, [(z, 0.15, 0.0) for z in HS[:6]], 10.2)]
    for z in HS[6:]:
        a, r = rng.uniform(0, 2 * np.pi, 40), 0.3 * np.sqrt(rng.uniform(0, 1, 40))
        rows.append(np.column_stack([3.0 + r * np.cos(a), -2.0 + r * np.sin(a), np.full(40, z)]))
    xyz, lab = _one(np.concatenate(rows), 4)

    def check(res):
        p = res["stem_profile"]
        _assert_states(res, 0, [1] * 6 + [2] * 3 + [0] * 11)
        assert p["n"][0][:9].tolist() == [64] * 6 + [40] * 3 and np.array_equal(p["h"][0], HS)
        assert res["stem_top_h"][0] == 3.0 and abs(res["stem_volume"][0] - PI * 0.15 ** 2 * 3.0) <= TOL
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_gap_in_stem():
    """No rows in the slab at 3 m: one miss, the walk resumes, the volume bridges it."""
    xyz, lab = _one(_tree(3.0, -2.0, [(z, 0.15, 0.0) for z in HS if z != 3.0], 10.2), 5)

    def check(res):
        _assert_states(res, 0, [1] * 5 + [2] + [1] * 14)
        assert res["stem_profile"]["n"][0][5] == 0
        assert abs(res["stem_volume"][0] - PI * 0.15 ** 2 * 10.0) <= TOL and res["stem_top_h"][0] == 10.0
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_whorl():
    """A ring of radius 0.25 at 3 m on a stem of 0.15: inside the search radius (0.325), a clean circle, but beyond max_growth (0.1875)."""
    xyz, lab = _one(_tree(3.0, -2.0, [(z, 0.25 if z == 3.0 else 0.15, 0.0) for z in HS], 10.2), 6)

    def check(res):
        _assert_states(res, 0, [1] * 5 + [2] + [1] * 14)
        assert res["stem_profile"]["n"][0][5] == 64
        assert abs(res["stem_volume"][0] - PI * 0.15 ** 2 * 10.0) <= TOL
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def _bounds(seed, cfg, extra, n0):
    """Dyadic geometry: position exactly (3, -2) (the base rows alone: first_height = 1), z_ref = 0, thickness 0.25; slab 0 is
    0.875 <= z < 1.125.  A ring of 8 rows at 1.0 plus one row on the lower bound (in), one on the upper (out), one just under it (in)."""
    lo, hi = (0.0 + 1.0) - 0.25 / 2, (0.0 + 1.0) + 0.25 / 2
    rows = np.array([[3.15, -2.0, lo], [2.85, -2.0, hi], [3.0, -1.85, np.nextafter(hi, -np.inf)]] + extra)
    xyz, lab = _one(np.concatenate([_base(3.0, -2.0), _ring(3.0, -2.0, 0.15, 1.0, 8), rows, _top(3.0, -2.0, 3.0)]), seed)

    def check(res):
        p = res["stem_profile"]
        assert p["h"][0].tolist() == [1.0, 1.5, 2.0, 2.5, 3.0]
        assert p["n"][0].tolist() == [n0, 0, 0, 0, 0] and p["state"][0][1:].tolist() == [2, 2, 0, 0]
    return dict(xyz=xyz, lab=lab, cfg=dict(dict(first_height=1.0, thickness=0.25), **cfg), check=check, exact=True)


def case_bounds_corridor():
    """A search radius of 2 m, so the corridor of 1.5 m decides: a row exactly 1.5 m away is out, one 2^-10 m closer is in."""
    return _bounds(7, dict(corridor=1.5, start_radius=2.0), [[4.5, -2.0, 1.0], [3.0, -2.0 + 1.4990234375, 1.0], [3.0, -2.0 - 1.75, 1.0]], 8 + 2 + 1)


def case_bounds_search():
    """The search radius of 0.5 m decides: a row exactly 0.5 m from the position is out, one 2^-10 m closer is in."""
    return _bounds(8, dict(corridor=1.5, start_radius=0.5), [[3.5, -2.0, 1.0], [3.0, -2.0 + 0.4990234375, 1.0], [3.0, -2.0 - 1.0, 1.0]], 8 + 2 + 1)


def case_step_equals_thickness():
    """Slabs that tile the height (step = thickness = 0.5): a row on the shared bound hi_k = lo_(k+1) belongs to slab k + 1 alone.  Every
    slab holds its centre ring and the ring on its lower bound; the ring at 10.25 lies on the last slab's upper bound and in no slab."""
    layers = [(z, 0.15, 0.0) for z in HS] + [(z - 0.25, 0.15, 0.0) for z in HS] + [(10.25, 0.15, 0.0)]
    xyz, lab = _one(_tree(3.0, -2.0, layers, 10.4), 9)

    def check(res):
        _assert_states(res, 0, [1] * 20)
        assert res["stem_profile"]["n"][0].tolist() == [128] * 20
        assert abs(res["stem_volume"][0] - PI * 0.15 ** 2 * 10.0) <= TOL
    return dict(xyz=xyz, lab=lab, cfg=dict(thickness=0.5), check=check)


def case_short_trees():
    """Tree 1 ends below the first slab (S_t = 0); tree 2 has exactly one slab: volume of the cylinder below it, no DBH, lean or taper."""
    t1 = np.concatenate([_base(3.0, -2.0), _ring(3.0, -2.0, 0.15, 0.3, 8), _top(3.0, -2.0, 0.4)])
    t2 = np.concatenate([_base(13.0, -2.0), _ring(13.0, -2.0, 0.15, 0.5), _top(13.0, -2.0, 0.75)])
    xyz, lab = _shuffled(np.concatenate([t1, t2]), np.concatenate([np.full(len(t1), 1), np.full(len(t2), 2)]), 10)

    def check(res):
        p = res["stem_profile"]
        assert p["h"].shape == (2, 1) and NAN(p["h"][0, 0]) and p["h"][1, 0] == 0.5
        _assert_states(res, 0, [0])
        _assert_states(res, 1, [1])
        assert res["stem_slices"].tolist() == [0, 1]
        assert all(NAN(res[k][0]) for k in ("stem_base_h", "stem_top_h", "stem_volume", "dbh_stem", "stem_lean", "stem_taper"))
        assert res["stem_base_h"][1] == 0.5 and res["stem_top_h"][1] == 0.5 and abs(res["stem_volume"][1] - PI * 0.15 ** 2 * 0.5) <= TOL
        assert NAN(res["dbh_stem"][1]) and NAN(res["stem_lean"][1]) and NAN(res["stem_taper"][1])
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_max_slices():
    xyz, lab = _one(_tree(3.0, -2.0, [(z, 0.15, 0.0) for z in HS], 10.2), 11)

    def check(res):
        assert res["stem_profile"]["h"].shape == (1, 4)
        _assert_states(res, 0, [1] * 4)
        assert res["stem_top_h"][0] == 2.0 and abs(res["stem_volume"][0] - PI * 0.15 ** 2 * 2.0) <= TOL and abs(res["dbh_stem"][0] - 0.30) <= TOL
    return dict(xyz=xyz, lab=lab, cfg=dict(max_slices=4), check=check)


def case_nan_z_ref():
    """Two cylinders; the second stands where the terrain has no value: zero slabs, NaN in every column, and the profile as wide as the first's."""
    t1 = _tree(3.0, -2.0, [(z, 0.15, 0.0) for z in HS[:6]], 3.2)
    t2 = _tree(13.0, -2.0, [(z, 0.15, 0.0) for z in HS], 10.2)
    xyz, lab = _shuffled(np.concatenate([t1, t2]), np.concatenate([np.full(len(t1), 1), np.full(len(t2), 2)]), 12)

    def check(res):
        p = res["stem_profile"]
        assert p["h"].shape == (2, 6) and NAN(p["h"][1]).all()
        _assert_states(res, 0, [1] * 6)
        _assert_states(res, 1, [0] * 6)
        assert res["stem_slices"].tolist() == [6, 0] and NAN(res["stem_volume"][1]) and NAN(res["stem_base_h"][1])
    return dict(xyz=xyz, lab=lab, cfg={}, check=check, z_ref=np.array([0.0, np.nan]))


def case_label_gap():
    """Labels {1, 3} (and 0, -1, ignored): tree 2 has no rows, zero slabs and NaN in every column."""
    t1 = _tree(3.0, -2.0, [(z, 0.15, 0.0) for z in HS[:6]], 3.2)
    t3 = _tree(13.0, -2.0, [(z, 0.1, 0.0) for z in HS[:4]], 2.2)
    junk = _ring(3.0, -2.0, 0.3, 1.0)                                     # other labels inside tree 1's first slabs: never candidates
    xyz = np.concatenate([t1, t3, junk, junk])
    lab = np.concatenate([np.full(len(t1), 1), np.full(len(t3), 3), np.zeros(len(junk)), np.full(len(junk), -1)])
    xyz, lab = _shuffled(xyz, lab, 13)

    def check(res):
        p = res["stem_profile"]
        assert p["h"].shape == (3, 6) and NAN(p["h"][1]).all() and NAN(p["h"][2][4:]).all()
        _assert_states(res, 0, [1] * 6)
        _assert_states(res, 1, [0] * 6)
        _assert_states(res, 2, [1] * 4 + [0] * 2)
        assert res["stem_slices"].tolist() == [6, 0, 4] and NAN(res["stem_volume"][1])
        assert abs(res["stem_volume"][2] - PI * 0.1 ** 2 * 2.0) <= TOL and abs(res["dbh_stem"][2] - 0.2) <= TOL
    return dict(xyz=xyz, lab=lab, cfg={}, check=check)


def case_no_trees():
    def check(res):
        p = res["stem_profile"]
        assert all(p[k].shape == (0, 0) for k in ("h", "x", "y", "r", "rmse", "n", "state"))
        assert all(len(res[k]) == 0 for k in ("stem_slices", "stem_base_h", "stem_top_h", "stem_volume", "dbh_stem", "stem_lean", "stem_taper"))
        assert res["stem_slices"].dtype == np.int64 and p["n"].dtype == np.int64
    return dict(xyz=np.zeros((3, 3)), lab=np.array([0, -1, 0], np.int64), cfg={}, check=check)


CASES = dict(cylinder=case_cylinder, cone=case_cone, lean=case_lean, crown=case_crown, gap_in_stem=case_gap_in_stem, whorl=case_whorl,
             bounds_corridor=case_bounds_corridor, bounds_search=case_bounds_search, step_equals_thickness=case_step_equals_thickness,
             short_trees=case_short_trees, max_slices=case_max_slices, nan_z_ref=case_nan_z_ref, label_gap=case_label_gap,
             no_trees=case_no_trees)
