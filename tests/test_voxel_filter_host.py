"""The voxel filter tests' inputs under the reference alone (no GPU): the sweeps of tests/voxel_filter_common.py reach
the paths of the adaptive search they are meant to reach, the restatement of the search agrees with the oracle at every
threshold, the clustered clouds have the survivors they were built to have, and the library's host functions
(dliom_voxel_filter, dliom_adaptive_voxel_filter) equal the oracle on all of it, bit for bit.
tests/test_gpu_voxel_filter.py then runs the same inputs through the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_filter_common as vc  # noqa: E402
from voxel_filter_common import f32  # noqa: E402


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_search_path_on_hand_made_counts():
    """The restatement on count functions small enough to follow by hand (max_length 2: halvings 1, 0.5, ..., 2 / 128;
    the bisection between 1 and 2 tries 1.5, then 1.75 or 1.25, ...)."""
    def count(table, default):
        return lambda length: table.get(float(length), default)
    assert vc.search_path(count({}, 5), 10, 2.0, 10) == ("sparse", 10)     # size() <= min_num_points: a tie is sparse
    assert vc.search_path(count({2.0: 7}, 0), 10, 2.0, 7) == ("max", 7)      # size() >= min_num_points: a tie is dense
    assert vc.search_path(count({}, 3), 10, 2.0, 4) == ("none", 3)
    # 1.0 is dense enough; 1.5 is not (high = 1.5), 1.25 is (low = 1.25), 1.375 is not: (1.375 - 1.25) / 1.25 <= 0.1 ends
    c = count({2.0: 1, 1.0: 8, 1.5: 2, 1.25: 6, 1.375: 4}, 0)
    assert vc.search_path(c, 10, 2.0, 5) == ("2/fof", 6)
    # only 2 / 8 = 0.25 and below are dense enough; every mid length between 0.25 and 0.5 as well: 0.375, 0.4375, 0.46875
    c = lambda length: 9 if float(length) < 0.5 else 1  # noqa: E731
    assert vc.search_path(c, 10, 2.0, 5) == ("8/ooo", 9)
    # four steps: 1.5, 1.25, 1.125 fail, then 1.0625 (dense enough or not)
    c = count({1.0: 8, 1.0625: 7}, 1)
    assert vc.search_path(c, 10, 2.0, 5) == ("2/fffo", 7)
    assert vc.search_path(count({1.0: 8}, 1), 10, 2.0, 5) == ("2/ffff", 8)
    # the last halving is max_length / 128: high = max_length / 64 > 0.01 max_length > max_length / 128
    c = lambda length: 9 if float(length) <= 2.0 / 128 else 1  # noqa: E731
    assert vc.search_path(c, 10, 2.0, 5)[0].startswith("128/")
    c = lambda length: 9 if float(length) < 2.0 / 128 else 1  # noqa: E731
    assert vc.search_path(c, 10, 2.0, 5) == ("none", 1)


def test_oracle_crops_before_it_rounds(orc):
    """AdaptiveVoxelFilter is FilterByMaxRange, THEN the search (:147-150): non-finite points and points far outside any
    voxel key never reach the rounding, so the oracle may be given them, and its output is that of the clean cloud."""
    pts = vc.search_cloud()
    for max_range in vc.SEARCH_MAX_RANGES:
        cloud, added = vc.with_unroundable_points(pts, max_range)
        assert np.array_equal(bits(vc.crop(cloud, max_range)), bits(vc.crop(pts, max_range)))
        for t in (1, 150, 1000, 5000):
            want = orc.adaptive_voxel_filter(2.0, t, max_range, pts)
            assert np.array_equal(bits(orc.adaptive_voxel_filter(2.0, t, max_range, cloud)), bits(want)), (max_range, t)


@pytest.mark.parametrize("max_range", vc.SEARCH_MAX_RANGES)
@pytest.mark.parametrize("max_length", vc.SEARCH_MAX_LENGTHS)
def test_sweep_reaches_every_path_and_host_filter_equals_oracle(dl, orc, max_length, max_range):
    """The conditions the device test relies on, under the reference alone: the restatement's count is the oracle's at
    every threshold; the sweep reaches `sparse`, `max`, `none`, a halving of the second insert launch (max_length / 8 or
    below, for 2.0 and 3.1), four bisection steps, and at least 30 (2.0, 3.1) / 15 (0.7) distinct paths.  And the
    library's host function equals the oracle over the whole sweep."""
    sweep = vc.search_sweep(orc, max_length, max_range)
    paths = vc.check_sweep_conditions(sweep, max_length)
    print("max_length %.1f max_range %.1f: %d thresholds, %d distinct paths, halvings %s" % (
        max_length, max_range, len(sweep), len(paths), sorted({vc.path_divisor(p) for p in paths if "/" in p})))
    pts = vc.search_cloud()
    for t, path, _, want in sweep:
        got = dl.adaptive_voxel_filter(max_length, t, max_range, pts)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (t, path)


def test_pair_classes_and_cross_pairs_exist(orc):
    classes = vc.pair_classes(orc)
    sweep = {t: path for t, path, _, _ in vc.search_sweep(orc, 2.0, 50.0)}
    assert vc.path_divisor(sweep[classes["first"][1]]) in (2, 4)
    assert vc.path_divisor(sweep[classes["second"][1]]) >= 8
    assert len(vc.path_steps(sweep[classes["deepest"][1]])) >= 4
    assert len(vc.cross_pairs(orc)) >= 5
    assert any(a[0] != b[0] and a[2] != b[2] for a, b in vc.cross_pairs(orc))


@pytest.mark.parametrize("name", vc.cluster_cases(5000))
def test_clustered_clouds_have_their_survivors(dl, orc, name):
    """The clustered clouds at n = 5000: the oracle keeps exactly the indices the cloud was built to keep, and the host
    function returns those points, bit for bit and in order."""
    pts, keep = vc.cluster_cloud(name, 5000)
    assert np.array_equal(orc.voxel_filter(vc.CLUSTER_EDGE, pts), keep)
    got = dl.voxel_filter(vc.CLUSTER_EDGE, pts)
    assert got.shape == (len(keep), 3) and np.array_equal(bits(got), bits(pts[keep]))


def test_clustered_clouds_above_65536_have_their_survivors(orc):
    for name in vc.cluster_cases(70001):
        pts, keep = vc.cluster_cloud(name, 70001)
        assert np.array_equal(orc.voxel_filter(vc.CLUSTER_EDGE, pts), keep), name
    assert "b_first_at_65536" in vc.cluster_cases(70001) and "b_first_at_65536" not in vc.cluster_cases(5000)


def test_sizes_have_survivors_beyond_65536(orc):
    """What the device test asserts about the large clouds holds for the reference: survivors in the 257th compaction
    workgroup and beyond (indices from 65 536 on), behind thousands of earlier survivors.  At 0.05 m every large cloud has
    them.  At 2.0 m the +-20 m cube's voxels are nearly all taken within the first 65 536 points: the 1 and 257 points that
    n = 65 537 and 65 793 have behind them add no voxel (vc.has_late_survivors), the larger clouds add a few dozen."""
    for n in [n for n in vc.SIZES_N if n > 65536]:
        for size in vc.SIZES_EDGE:
            keep = vc.uniform_keep(orc, n, size)
            assert np.all(np.diff(keep) > 0)
            late = keep >= 65536
            assert (late.sum() >= 1) == vc.has_late_survivors(n, size), (n, size, late.sum())
            if late.any():
                assert np.argmax(late) > 9000, (n, size, np.argmax(late))
