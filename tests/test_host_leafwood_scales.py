"""Host tests of the leaf-wood seed over several scales (util/leafwood.py, csrc/tl_leafwood.hip: tl_leafwood_seed_scales; no GPU):
the count rule through the numpy restatement, check_scales on every constraint, the options of the five command lines, the entry point's
declaration, binding and argument checks on host memory, and the generated leaf-on tree through the restatement at the recommended scales:
recall and precision of the wood flag, both above the one-scale figures of §25."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

import leafwood_cases as cases
import leafwood_restatement as ref
import leafwood_scales_restatement as sref
from test_host_leafwood import PRECISION_MIN, RECALL_MIN                  # the one-scale figures of §25, rounded down

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES, SCALES_MIN = (0.1, 0.3, 0.4), 2                                   # the recommended point of DESIGN §26
# The generated leaf-on tree at these scales through the restatement's f64 features, on the host: recall 0.8966, precision 0.8222
# (one scale: 0.8193 / 0.7284).  Asserted: the measured figures rounded down to two decimals; the generator is seeded, they do not move.
RECALL_SCALES_MIN, PRECISION_SCALES_MIN = 0.89, 0.82


def test_the_restatement_shares_the_rules_it_does_not_change():
    assert sref.seed is ref.seed and sref.vote is ref.vote and sref.voxel_keys is ref.voxel_keys and sref.components is ref.components
    assert sref.LEAFWOOD_SCALE_DEFAULTS == dict(scales=None, scales_min=1)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_count_rule_through_the_restatement(S):
    feats, want = cases.seed_cases()
    p = dict(ref.LEAFWOOD_DEFAULTS, **cases.SEED_P)
    shifts = (0, 1, 6, 5)                                                 # scale k holds the rows shifted by shifts[k]: every count 0..S occurs
    f = np.stack([np.roll(feats, shifts[k], axis=0) for k in range(S)], 1)
    hold = np.stack([np.roll(want.astype(np.int64), shifts[k]) for k in range(S)], 1).sum(1)
    assert set(hold.tolist()) == set(range(S + 1))
    for k in range(1, S + 1):
        got, counted = sref.seed_scales(f, p, k)
        assert got.dtype == np.uint8 and np.array_equal(counted, hold) and np.array_equal(got, (hold >= k).astype(np.uint8))
    assert np.array_equal(sref.seed_scales(f[:, :1, :], p, 1)[0], want)                       # one scale: rule 2 itself
    # a scale with fewer than min_neighbours neighbours, or a NaN, does not count -- whatever the others say
    row = np.array([[[0.9, 0.0, 0.0, 4], [0.9, 0.0, 0.0, 50], [np.nan, 0.8, 0.9, 50], [0.1, 0.8, 0.9, 50]]], np.float32)[:, :S, :]
    assert sref.seed_scales(row, p, 1)[1].tolist() == [[0, 1, 1, 2][S - 1]]


def test_one_scale_at_the_radius_is_the_one_scale_restatement():
    c = cases.COMPONENT_CASES["threshold"]()
    a = ref.leafwood(c["xyz"], c["lab"], c["tree"], c["p"])
    b = sref.leafwood_scales(c["xyz"], c["lab"], c["tree"], c["p"], [c["p"]["radius"]], 1)
    for k in ("wood", "seed", "voted") + ref.LEAFWOOD_COLUMNS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(a["rows"], b["rows"]) and a["margins"] == b["margins"]


def test_check_scales():
    from treelearn_amd.util.leafwood import LEAFWOOD_DEFAULTS, LEAFWOOD_SCALE_DEFAULTS, check_params, check_scales
    assert LEAFWOOD_SCALE_DEFAULTS == sref.LEAFWOOD_SCALE_DEFAULTS == dict(scales=None, scales_min=1)
    assert not set(LEAFWOOD_SCALE_DEFAULTS) & set(LEAFWOOD_DEFAULTS) and check_params() == LEAFWOOD_DEFAULTS     # beside the eleven, not among them
    assert check_scales() == LEAFWOOD_SCALE_DEFAULTS and check_scales(dict(scales=None), scales_min=None) == LEAFWOOD_SCALE_DEFAULTS
    s = check_scales(scales=(0.2, 0.4), scales_min=2.0)
    assert s == dict(scales=[0.2, 0.4], scales_min=2) and isinstance(s["scales_min"], int) and isinstance(s["scales"], list)
    assert check_scales(dict(scales=[0.3]))["scales_min"] == 1 and check_scales(scales=np.array([0.1, 0.2, 0.3, 0.4]), scales_min=4)["scales_min"] == 4
    nan, inf = float("nan"), float("inf")
    for bad in (dict(scales=[]), dict(scales=[0.1, 0.2, 0.3, 0.4, 0.5]), dict(scales=[0.2, 0.2]), dict(scales=[0.4, 0.2]), dict(scales=[0.0, 0.2]),
                dict(scales=[-0.2]), dict(scales=[nan]), dict(scales=[0.2, inf]), dict(scales=["0.2"]), dict(scales=0.2), dict(scales="0.2"),
                dict(scales=[0.2, 0.4], scales_min=0), dict(scales=[0.2, 0.4], scales_min=3), dict(scales=[0.2, 0.4], scales_min=1.5),
                dict(scales=[0.2, 0.4], scales_min=nan), dict(scales=[0.2, 0.4], scales_min=True), dict(scales_min=2), dict(nothing=1)):
        with pytest.raises(ValueError):
            check_scales(bad)


def test_argument_parsers(tmp_path):
    from treelearn_amd.util import branches, inventory, leafwood, segment, wood
    ap = argparse.ArgumentParser()
    leafwood.add_arguments(ap)
    leafwood.add_arguments(ap)                                            # a second call adds nothing
    a = ap.parse_args([])
    assert leafwood.scales_of(a) == leafwood.LEAFWOOD_SCALE_DEFAULTS and leafwood.params_of(a) == leafwood.LEAFWOOD_DEFAULTS
    a = ap.parse_args(["--leafwood-scales", "0.1", "0.3", "0.4", "--leafwood-scales-min", "2", "--leafwood-vote-iters", "3"])
    assert leafwood.check_scales(leafwood.scales_of(a)) == dict(scales=[0.1, 0.3, 0.4], scales_min=2)
    assert leafwood.params_of(a) == dict(leafwood.LEAFWOOD_DEFAULTS, vote_iters=3)
    forest = tmp_path / "f.npy"
    np.save(forest, np.zeros((4, 4)))
    # scales outside their constraint end every command line before any GPU work, and nothing is written
    for bad in (["--leafwood-scales", "0.4", "0.2"], ["--leafwood-scales", "0.2", "0.4", "--leafwood-scales-min", "3"], ["--leafwood-scales-min", "2"],
                ["--leafwood-scales"], ["--leafwood-scales", "0.1", "0.2", "0.3", "0.4", "0.5"]):
        with pytest.raises(SystemExit):
            leafwood.main(["--forest", str(forest), "--out", str(tmp_path / "o.npy")] + bad)
        with pytest.raises(SystemExit):
            branches.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--leafwood"] + bad)
        with pytest.raises(SystemExit):
            wood.main(["--forest", str(forest), "--out", str(tmp_path / "o.npz"), "--leafwood"] + bad)
        with pytest.raises(SystemExit):
            inventory.main(["--forest", str(forest), "--out", str(tmp_path / "o.csv"), "--leafwood"] + bad)
    (tmp_path / "w.pth").write_bytes(b"")
    common = ["--forest", str(forest), "--weights", str(tmp_path / "w.pth"), "--out", str(tmp_path)]
    with pytest.raises(SystemExit):
        segment.parse_args(common + ["--leafwood", "--leafwood-scales", "0.4", "0.2"])
    a = segment.parse_args(common + ["--leafwood", "--leafwood-scales", "0.2", "0.4", "--leafwood-scales-min", "2"])
    assert a.leafwood and a.leafwood_scales == [0.2, 0.4] and a.leafwood_scales_min == 2
    a = segment.parse_args(common)
    assert a.leafwood_scales is None and a.leafwood_scales_min == 1 and leafwood.params_of(a) == leafwood.LEAFWOOD_DEFAULTS
    assert not (tmp_path / "o.npz").exists() and not (tmp_path / "o.csv").exists() and not (tmp_path / "o.npy").exists()
    with pytest.raises(ValueError):                                       # the API checks before any GPU work too
        segment.segment_forest(None, None, leafwood=True, leafwood_scales=(0.4, 0.2))
    with pytest.raises(ValueError):
        inventory.tree_inventory(None, None, leafwood=True, leafwood_scales=(0.2, 0.4), leafwood_scales_min=3)
    with pytest.raises(ValueError):
        inventory.cloud_inventory(np.zeros((1, 4)), leafwood=True, leafwood_scales_min=2)


def test_header_declares_and_library_exports_the_entry_point():
    from treelearn_amd import _hip, build as b
    from treelearn_amd.util.leafwood import check_params
    header = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    m = re.search(r"\bint tl_leafwood_seed_scales\(([^;]*)\);", header)
    res, args = _hip.PROTOTYPES["tl_leafwood_seed_scales"]
    assert m and len(m.group(1).split(",")) == 7 == len(args) and res is ctypes.c_int32
    assert args[2] is ctypes.c_int32 and args[4] is ctypes.c_int32 and args[1] is ctypes.c_int64
    assert hasattr(ctypes.CDLL(b.build(verbose=False)), "tl_leafwood_seed_scales")
    lib = _hip.lib()

    def params(**kw):
        return _hip.LeafwoodParams(**{**check_params(), "filter": 1, **kw})
    good = params()
    buf = (ctypes.c_char * 1024)()                                       # host memory: only its address and alignment are looked at
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    p, odd8, odd4 = (ctypes.c_void_p(base + k) for k in (0, 8, 4))
    seed = lambda *a: lib.tl_leafwood_seed_scales(*a, None)              # noqa: E731
    ok, bad = _hip.TL_OK, _hip.TL_ERR_ARG
    for S in (1, 2, 3, 4):                                                # nothing to do, found out after the argument checks and without a launch
        for k in range(1, S + 1):
            assert seed(p, 0, S, good, k, p) == ok
    assert seed(p, 0, 2, good, 1, odd4) == ok                             # the u8 flags anywhere
    assert seed(None, 0, 2, good, 1, p) == bad and seed(p, 0, 2, good, 1, None) == bad and seed(p, 0, 2, None, 1, p) == bad
    assert seed(odd8, 0, 2, good, 1, p) == bad and seed(odd4, 0, 2, good, 1, p) == bad          # the rows are read as float4
    assert seed(p, -1, 2, good, 1, p) == bad
    for S, k in ((0, 1), (5, 1), (-1, 1), (2, 0), (2, 3), (1, 2), (4, 5), (3, -1)):
        assert seed(p, 0, S, good, k, p) == bad, (S, k)
    nan = float("nan")
    for wrong in (dict(radius=0.0), dict(radius=nan), dict(voxel=0.0), dict(min_neighbours=2), dict(linearity_min=1.1), dict(planarity_min=nan),
                  dict(verticality_min=-0.1), dict(vote_iters=9), dict(vote_percent=0), dict(reach=3), dict(min_component=0), dict(filter=2)):
        assert seed(p, 0, 2, params(**wrong), 1, p) == bad, wrong


@pytest.fixture(scope="module")
def leaf_on():
    """The generated leaf-on tree through the restatement at the recommended scales (the three feature restatements computed once)."""
    import inventory_restatement as inv_ref
    xyz, lab, truth, length = cases.leaf_on_tree()
    base = inv_ref.tree_inventory(xyz, lab)
    tree = np.column_stack([base["x"], base["y"], base["z_low"], base["z_top"]])
    return dict(xyz=xyz, lab=lab, truth=truth, length=length, tree=tree, got=sref.leafwood_scales(xyz, lab, tree, {}, SCALES, SCALES_MIN))


def test_generated_leaf_on_tree_recall_and_precision(leaf_on):
    truth, wood, m = leaf_on["truth"], leaf_on["got"]["wood"], leaf_on["got"]["margins"]
    assert m["radius"] > ref.MIN_RADIUS_MARGIN and min(m["voxel"], m["anchor"]) > ref.MIN_FLOOR_MARGIN, m
    tp = int((wood & truth).sum())
    recall, precision = tp / int(truth.sum()), tp / int(wood.sum())
    print(f"scales {SCALES} min {SCALES_MIN}: rows {len(truth)}, wood {int(truth.sum())}, flagged {int(wood.sum())}, recall {recall:.4f}, "
          f"precision {precision:.4f}, components {leaf_on['got']['lw_components'][0]}, margins {m}")
    assert recall > RECALL_MIN and precision > PRECISION_MIN              # each strictly above the one-scale bound
    assert recall > 0.8193 and precision > 0.7284                         # ... and above the one-scale figures themselves (§25)
    assert recall >= RECALL_SCALES_MIN and precision >= PRECISION_SCALES_MIN


def test_generated_leaf_on_tree_skeleton_length(leaf_on):
    """skel_length of the branches restatement on the wood rows, printed: 257.6 m against 224.3 m of true limb length (one scale:
    239.1 m; no point of the grid of §26 comes closer than the one scale does, so none is asserted)."""
    import branches_restatement as br_ref
    xyz, lab, tree, rows = leaf_on["xyz"], leaf_on["lab"], leaf_on["tree"], leaf_on["got"]["rows"]
    wood = br_ref.branch_structure(xyz[rows], lab[rows], tree[:, 0], tree[:, 1], tree[:, 2])["skel_length"][0]
    print(f"true limb length {leaf_on['length']:.3f} m, skel_length on the wood rows at scales {SCALES} min {SCALES_MIN}: {wood:.3f} m")
    assert np.isfinite(wood) and wood > 0
