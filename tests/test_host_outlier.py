"""Outlier filters without a GPU: hand-worked cases of the restatement (tests/outlier_restatement.py, the specification of
csrc/tl_outlier.hip) and the config rules of util/outlier.py as crops.check_cfg and tiles.write_tiles apply them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlier_restatement as R  # noqa: E402

from treelearn_amd.util import crops as C  # noqa: E402
from treelearn_amd.util import outlier as O  # noqa: E402


# ============================================================================================ 1. the restatement, by hand
def test_collinear_points_statistical_filter_by_hand():
    # x = 0, 1, 2, 3, 10 with k = 2: every point's two smallest distances are 0 (itself) and the gap to its nearest neighbour, so
    # avg = (0.5, 0.5, 0.5, 0.5, 3.5); mean = 5.5 / 5 = 1.1; std = sqrt((4 * 0.6^2 + 2.4^2) / 4) = sqrt(1.8) = 1.3416...;
    # thr = 1.1 + 1 * 1.3416 = 2.4416: the four points at 0..3 stay, the one at 10 goes.
    xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], dtype=np.float64)
    avg = R.knn_mean_dist(xyz, 2)
    assert avg.tolist() == [0.5, 0.5, 0.5, 0.5, 3.5]
    assert abs(R.sor_threshold(avg, 1.0) - (1.1 + np.sqrt(1.8))) < 1e-12
    assert R.sor_mask(xyz, 2, 1.0).tolist() == [True, True, True, True, False]
    # the divisor of the mean is n also when some avg are 0, and k = 1 keeps nothing
    assert not R.sor_mask(xyz, 1, 1.0).any()
    # n < k: min(k, n) = 5 distances
    assert R.knn_mean_dist(xyz, 64)[0] == (0 + 1 + 2 + 3 + 10) / 5
    assert not R.sor_mask(xyz[:1], 2, 1.0).any() and R.sor_mask(xyz[:0], 2, 1.0).shape == (0,)


def test_integer_lattice_radius_filter_is_strict():
    g = np.arange(3, dtype=np.float64)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    assert (R.radius_count(xyz, 1.0) == 1).all()                      # the neighbours at exactly 1 are not inside
    assert R.rad_mask(xyz, 1.0, 0).all() and not R.rad_mask(xyz, 1.0, 1).any()
    cnt = R.radius_count(xyz, 1.0001)
    assert cnt[13] == 7 and cnt[0] == 4                               # centre: 6 face neighbours; corner: 3


def test_duplicated_points_have_zero_mean_distance_and_are_removed():
    xyz = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4.5, 0, 0]], dtype=np.float64)
    avg = R.knn_mean_dist(xyz, 2)
    assert avg[0] == 0 and avg[1] == 0 and (avg[2:] > 0).all()
    keep = R.sor_mask(xyz, 2, 10.0)
    assert keep.tolist() == [False, False, True, True, True, True]
    assert R.denoise(xyz, (2, 10.0), (1.25, 1)).tolist() == [False, False, True, True, True, False]


# ============================================================================================ 2. config rules
def test_a_complete_pair_is_accepted():
    cfg = dict(C.TRAIN_CFG, n_neigh_sor=20, multiplier_sor=1.5)
    assert C.check_cfg(cfg) == dict(sor=(20, 1.5), rad=None)
    assert C.check_cfg(dict(C.TRAIN_CFG, rad=0.25, npoints_rad=5)) == dict(sor=None, rad=(0.25, 5))
    both = O.active_filters(dict(n_neigh_sor=2, multiplier_sor=1, rad=1, npoints_rad=0))
    assert both == dict(sor=(2, 1.0), rad=(1.0, 0)) and O.active_filters(both) is both
    assert O.active_filters(dict()) == dict(sor=None, rad=None) and O.active_filters(None) == dict(sor=None, rad=None)
    assert C.check_cfg(C.TRAIN_CFG) == dict(sor=None, rad=None)

    class NS:
        n_neigh_sor, multiplier_sor, rad, npoints_rad = 6, 0.5, None, None
    assert O.active_filters(NS()) == dict(sor=(6, 0.5), rad=None)


@pytest.mark.parametrize("key,other", [("n_neigh_sor", "multiplier_sor"), ("multiplier_sor", "n_neigh_sor"), ("rad", "npoints_rad"),
                                       ("npoints_rad", "rad")])
def test_a_half_set_pair_is_refused_by_name(key, other, tmp_path):
    with pytest.raises(NotImplementedError, match=f"^{key} is set but {other} is not"):
        O.active_filters({key: 2})
    with pytest.raises(NotImplementedError, match=f"^{key} is set"):                  # also beside a complete other pair
        C.check_cfg(dict(C.TRAIN_CFG, **{key: 2}, **({"rad": 1, "npoints_rad": 1} if "sor" in key else {"n_neigh_sor": 2, "multiplier_sor": 1})))
    from treelearn_amd.util.tiles import write_tiles
    with pytest.raises(NotImplementedError, match=f"^{key} is set"):
        write_tiles(str(tmp_path / "forest" / "p.npy"), dict(sample_generator={key: 2}))
    assert not os.listdir(str(tmp_path))                                               # refused before anything is written


@pytest.mark.parametrize("pair", [dict(n_neigh_sor=0, multiplier_sor=1.0), dict(n_neigh_sor=-3, multiplier_sor=1.0),
                                  dict(n_neigh_sor=2, multiplier_sor=0.0), dict(n_neigh_sor=2, multiplier_sor=-1.0),
                                  dict(n_neigh_sor=65, multiplier_sor=1.0), dict(n_neigh_sor=2.5, multiplier_sor=1.0),
                                  dict(rad=0.0, npoints_rad=3), dict(rad=0.5, npoints_rad=-1)])
def test_values_out_of_range_raise_value_error(pair, tmp_path):
    with pytest.raises(ValueError):
        O.active_filters(pair)
    with pytest.raises(ValueError):
        C.generate_random_crops(str(tmp_path), pair)
    assert not os.listdir(str(tmp_path))


def test_command_lines_take_the_four_keys():
    from treelearn_amd.util import tiles as T
    a = T.parse_args(["--forest", "x.npy", "--n-neigh-sor", "20", "--multiplier-sor", "1.5"])
    assert (a.n_neigh_sor, a.multiplier_sor, a.rad, a.npoints_rad) == (20, 1.5, None, None)
    with pytest.raises(SystemExit):
        C.parse_args(["--base-dir", ".", "--rad", "0.3"])
