"""The device voxel filters (csrc/voxel_filter.hip: VoxelFilter, AdaptiveVoxelFilter, the joint search of two adaptive
filters) where their kernels and their host search can break: above 65 536 points (the compaction's prefix loop takes a
second trip from workgroup 257 on), around the workgroup shapes, with one voxel's points in every workgroup, on both key
layouts and at the keys' limit, on every path of the adaptive search including ties of its comparisons, on every pairing
of those paths, and on one context whose scratch is carved for very different shapes in turn.  Every comparison is with
the CPU oracle and exact: the coordinates' bits, in order.  The inputs come from tests/voxel_filter_common.py;
tests/test_voxel_filter_host.py shows without a GPU that they reach what they are meant to reach."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import voxel_filter_common as vc  # noqa: E402
from voxel_filter_common import f32  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_same_points(got, want, what=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), what


def device_filter(dl, ctx, pts, size):
    cloud = dl.PointCloud(ctx, pts)
    try:
        out = cloud.voxel_filter(size)
        got = out.download()
        out.close()
        return got
    finally:
        cloud.close()


# ---------------------------------------------------------------------------------------------------------------------
# (a) sizes
@pytest.mark.parametrize("size", vc.SIZES_EDGE)
@pytest.mark.parametrize("n", vc.SIZES_N)
def test_sizes_around_the_workgroup_shapes_and_above_65536(dl, ctx, orc, n, size):
    """n on both sides of 256, 1024, 2048 (the LDS table), 32 768 and 65 536 (table_capacity's steps), and up to
    262 145; at 0.05 m nearly every point survives (large compaction offsets), at 2.0 m every workgroup meets every voxel.
    Above 65 536 points a compaction thread sums several preceding workgroups: there the survivors from index 65 536 on,
    and the positions they are written to, are checked on their own."""
    pts = vc.uniform_cloud(n, size)
    keep = vc.uniform_keep(orc, n, size)
    want = pts[keep]
    got = device_filter(dl, ctx, pts, size)
    assert_same_points(got, want)
    assert_same_points(dl.voxel_filter(size, pts), want, "host function")
    if n > 65536:
        late = np.flatnonzero(keep >= 65536)
        assert (len(late) >= 1) == vc.has_late_survivors(n, size)
        if len(late):
            # they exist, they sit behind the survivors of 256+ workgroups, and each is where the reference has it
            assert late[0] > 9000 and late[-1] == len(keep) - 1
            assert np.array_equal(bits(got[late]), bits(pts[keep[late]]))
            assert np.array_equal(bits(got[late[0] - 1]), bits(pts[keep[late[0] - 1]]))


# ---------------------------------------------------------------------------------------------------------------------
# (b) clustered clouds
@pytest.mark.parametrize("n,name", [(n, name) for n in vc.CLUSTER_N for name in vc.cluster_cases(n)])
def test_clustered_clouds(dl, ctx, orc, n, name):
    """One voxel's points in every workgroup: all points in one voxel; two voxels alternating; a voxel whose only member
    is the last point; a voxel whose FIRST member is the last point of an insert workgroup (1023), the first of the next
    (1024, 1025) or of compaction workgroup 257 (65 536, n = 70 001 only) with later members in every following workgroup
    -- the survivor is exactly that index; bit-identical copies; signed zeros and subnormals.  The survivors are the
    indices the cloud was built to keep: their coordinates by bits, in order, and equal to the oracle and the host."""
    pts, keep = vc.cluster_cloud(name, n)
    assert np.array_equal(orc.voxel_filter(vc.CLUSTER_EDGE, pts), keep)
    got = device_filter(dl, ctx, pts, vc.CLUSTER_EDGE)
    assert_same_points(got, pts[keep], (name, n))
    assert_same_points(dl.voxel_filter(vc.CLUSTER_EDGE, pts), pts[keep], "host function")
    if name.startswith("b_first_at_"):
        first = int(name[len("b_first_at_"):])
        assert len(got) == 2 and np.array_equal(bits(got[1]), bits(pts[first]))
        assert not np.array_equal(bits(pts[first]), bits(pts[first + 256]))  # (a later member would not pass for it)


# ---------------------------------------------------------------------------------------------------------------------
# (c) key layouts and limits
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_far_point_moves_the_launch_to_the_21_bit_keys(dl, ctx, orc, sign, axis):
    """Two clouds that differ in one point appended at the end, 4096 edges out: the first fits the packed words
    (13 bits per axis), the second does not and is filtered again with the 21-bit keys -- one rerun exactly, the same
    survivors in front of the far point, and both equal to the oracle."""
    size = 0.25
    near = vc.uniform_cloud(3001, size)
    far_point = np.array([0.1, -0.1, 0.2], f32)
    far_point[axis] = f32(sign * 4096 * size)
    far = np.concatenate([near, far_point[None]])
    before = ctx.voxel_filter_reruns()
    got_near = device_filter(dl, ctx, near, size)
    assert ctx.voxel_filter_reruns() == before
    got_far = device_filter(dl, ctx, far, size)
    assert ctx.voxel_filter_reruns() == before + 1
    assert_same_points(got_near, near[orc.voxel_filter(size, near)])
    assert_same_points(got_far, far[orc.voxel_filter(size, far)])
    assert len(got_far) == len(got_near) + 1
    assert np.array_equal(bits(got_far[:-1]), bits(got_near)) and np.array_equal(bits(got_far[-1]), bits(far_point))


def test_largest_accepted_voxel_index(dl, ctx, orc):
    """|p / size| = 1 048 574 (size 1.0: the coordinate is exact) on every axis and sign is inside the keys."""
    pts = vc.uniform_cloud(2049, 1.0).copy()
    for k, (axis, sign) in enumerate((a, s) for a in range(3) for s in (1.0, -1.0)):
        pts[100 + 300 * k, axis] = f32(sign * 1048574.0)
        pts[101 + 300 * k] = pts[100 + 300 * k]  # and a second point of that voxel
    keep = orc.voxel_filter(1.0, pts)
    assert all(100 + 300 * k in keep and 101 + 300 * k not in keep for k in range(6))
    assert_same_points(device_filter(dl, ctx, pts, 1.0), pts[keep])


REFUSED = [("index_1048575", axis, sign * 1048575.0) for axis in range(3) for sign in (1.0, -1.0)] + \
          [("nan", 0, np.nan), ("nan", 2, np.nan), ("+inf", 1, np.inf), ("-inf", 2, -np.inf)]


@pytest.mark.parametrize("what,axis,value", REFUSED)
def test_refused_points_and_the_call_after(dl, ctx, orc, what, axis, value):
    """A voxel index of 1 048 575 (on either sign and each axis) is outside the 21-bit keys, and a NaN or infinite
    coordinate has no voxel: DLIOM_ERR_INVALID_ARGUMENT.  The next call on the same context equals the oracle."""
    clean = vc.uniform_cloud(2047, 1.0)
    pts = clean.copy()
    pts[1500, axis] = f32(value)
    cloud = dl.PointCloud(ctx, pts)
    with pytest.raises(dl.DliomError) as e:
        cloud.voxel_filter(1.0)
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    cloud.close()
    assert_same_points(device_filter(dl, ctx, clean, 1.0), clean[orc.voxel_filter(1.0, clean)])
    small = vc.uniform_cloud(257, 2.0)
    assert_same_points(device_filter(dl, ctx, small, 2.0), small[orc.voxel_filter(2.0, small)])


@pytest.mark.parametrize("max_range", vc.SEARCH_MAX_RANGES)
def test_adaptive_filter_drops_what_it_cannot_round(dl, ctx, orc, max_range):
    """FilterByMaxRange comes first: non-finite points and points far outside any voxel key fail `norm <= max_range` and
    are dropped as the reference drops them, on every kind of path (the "already sparse" one keeps every in-range point).
    The oracle is given the same cloud: it crops before it rounds (tests/test_voxel_filter_host.py)."""
    pts, added = vc.with_unroundable_points(vc.search_cloud(), max_range)
    cloud = dl.PointCloud(ctx, pts)
    in_range = len(vc.crop(pts, max_range))
    for t in (1, 150, 1000, in_range - 1, in_range, in_range + 1, 5000):
        want = orc.adaptive_voxel_filter(2.0, t, max_range, pts)
        assert np.all(np.isfinite(want))
        out = cloud.adaptive_voxel_filter(2.0, t, max_range)
        got = out.download()
        out.close()
        assert_same_points(got, want, (max_range, t))
    a, b = cloud.adaptive_voxel_filter_pair((2.0, in_range, max_range), (0.7, 150, max_range))
    assert_same_points(a.download(), orc.adaptive_voxel_filter(2.0, in_range, max_range, pts))
    assert_same_points(b.download(), orc.adaptive_voxel_filter(0.7, 150, max_range, pts))
    for c in (a, b, cloud):
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# (d) the adaptive search, every path
@pytest.mark.parametrize("max_range", vc.SEARCH_MAX_RANGES)
@pytest.mark.parametrize("max_length", vc.SEARCH_MAX_LENGTHS)
def test_adaptive_search_every_path(dl, ctx, orc, max_length, max_range):
    """min_num_points swept over every survivor count c of a ladder of lengths (the tie that the search's `>=` turns on)
    and c + 1, plus 1, n and n + 1 (the `<=` of "already sparse"): the device result equals the oracle's at each.  The
    sweep is shown first to reach `sparse`, `max`, `none`, halvings of the second insert launch (a bisection that reads
    tables[2]), four bisection steps and at least 30 (15 for max_length 0.7) distinct paths
    (vc.check_sweep_conditions)."""
    sweep = vc.search_sweep(orc, max_length, max_range)
    vc.check_sweep_conditions(sweep, max_length)
    cloud = dl.PointCloud(ctx, vc.search_cloud())
    wrong = []
    for t, path, survivors, want in sweep:
        out = cloud.adaptive_voxel_filter(max_length, t, max_range)
        got = out.download()
        out.close()
        if got.shape != want.shape or not np.array_equal(bits(got), bits(want)):
            wrong.append((t, path, len(got), survivors))
    cloud.close()
    assert not wrong, wrong


# ---------------------------------------------------------------------------------------------------------------------
# (e) the joint search of two filters
@pytest.fixture(scope="module")
def window_of(dl, ctx, orc):
    """-> f(device cloud): the search window RealTimeCorrelativeScanMatcher3D builds for it.  The window's
    max_scan_range is the cloud's largest norm as the device computed it (dliom_cloud's bound, which has no export)."""
    from helpers import build_oracle_submap, to_device_grid
    grid = to_device_grid(dl, ctx, build_oracle_submap(orc, 0.5, num_scans=1))
    options = dict(linear_search_window=0.5, angular_search_window=0.02, translation_delta_cost_weight=0.1,
                   rotation_delta_cost_weight=0.1)
    matcher = dl.RealTimeCorrelativeScanMatcher3D(ctx, options)
    pose = np.array([0, 0, 0, 1.0, 0, 0, 0])

    def device_window(cloud):
        matcher.Match(pose, cloud, grid)
        return matcher.last_stats().window

    def host_window(points):
        return matcher.window(0.5, points)
    yield device_window, host_window
    grid.close()


def window_tuple(w):
    return (w.linear_window_size, w.angular_window_size, f32(w.angular_step_size).tobytes(), f32(w.max_scan_range).tobytes(),
            w.num_translations, w.num_rotations, w.num_candidates)


def check_pair(dl, orc, cloud, first, second, window_of):
    device_window, host_window = window_of
    a, b = cloud.adaptive_voxel_filter_pair(first, second)
    try:
        for out, options in ((a, first), (b, second)):
            want = vc.sweep_entry(orc, options)
            assert_same_points(out.download(), want, (first, second, options))
            if len(want):
                assert max(np.linalg.norm(want, axis=1)) > 1.5  # (above the window's floor of 3 cells: the norm shows)
                assert window_tuple(device_window(out)) == window_tuple(host_window(want)), (first, second, options)
    finally:
        a.close()
        b.close()


def test_adaptive_pair_every_pairing_of_paths(dl, ctx, orc, window_of):
    """One threshold per class of path (sparse, max, none, decided in the first launch and bisected, decided in the
    second launch and bisected, the deepest bisection), every ordered pair of them through the joint search, a class with
    itself included: each output equals its own single-filter oracle result, and the largest norm the device attached to
    it gives the matcher the window that the oracle's points give.  Two bisected filters put the second one's tree behind
    the first one's in one launch (tree_base > 0, the most lengths a launch carries)."""
    classes = vc.pair_classes(orc)
    cloud = dl.PointCloud(ctx, vc.search_cloud())
    try:
        for first_name, first in classes.items():
            for second_name, second in classes.items():
                check_pair(dl, orc, cloud, first, second, window_of)
    finally:
        cloud.close()


def test_adaptive_pair_across_lengths_and_ranges(dl, ctx, orc, window_of):
    """Pairs whose filters differ in max_length and max_range (their trees differ, their crops differ)."""
    cloud = dl.PointCloud(ctx, vc.search_cloud())
    try:
        for first, second in vc.cross_pairs(orc):
            check_pair(dl, orc, cloud, first, second, window_of)
    finally:
        cloud.close()


# ---------------------------------------------------------------------------------------------------------------------
# (f) one context, changing shapes
def run_sequence(dl, ctx, orc, steps):
    for kind, arguments in steps:
        if kind == "plain":
            n, size = arguments
            pts = vc.sequence_cloud(n, size)
            want = pts[vc.uniform_keep(orc, n, size)] if n else pts
            assert_same_points(device_filter(dl, ctx, pts, size), want, (kind, arguments))
        else:
            first, second = arguments
            cloud = dl.PointCloud(ctx, vc.search_cloud())
            assert len(cloud) == 4160
            a, b = cloud.adaptive_voxel_filter_pair(first, second)
            assert_same_points(a.download(), vc.sweep_entry(orc, first), (kind, first))
            assert_same_points(b.download(), vc.sweep_entry(orc, second), (kind, second))
            for c in (a, b, cloud):
                c.close()


@pytest.mark.parametrize("reverse_first", [False, True])
def test_one_context_changing_shapes(dl, orc, reverse_first):
    """The scratch is carved per call from n and the number of lengths: on ONE new context a plain filter at 262 145
    points, then 257, an adaptive pair at 4160 (32 tables), plain at 65 793, 1 and an empty cloud, then the same in
    reverse order (and, on another new context, reverse order first: the block grows call by call)."""
    steps = vc.sequence_steps(orc)
    own = dl.Context(0)
    try:
        for order in ((steps[::-1], steps) if reverse_first else (steps, steps[::-1])):
            run_sequence(dl, own, orc, order)
    finally:
        own.close()


# ---------------------------------------------------------------------------------------------------------------------
def test_randomised_slice(capsys):
    """Seeds 1-40 of tools/fuzz_voxel_filter.py with n capped at 70 000 (ten of them above 65 536): random sizes weighted
    to the boundaries, edge lengths, clusterings and adaptive triples, plain / adaptive / pair against the oracle."""
    from tools import fuzz_voxel_filter
    status = fuzz_voxel_filter.main(["--seeds"] + [str(s) for s in range(1, 41)] + ["--max-n", "70000", "--quiet"])
    out = capsys.readouterr().out
    assert status == 0 and "voxel filter fuzz ok: 40 cases equal" in out, out
