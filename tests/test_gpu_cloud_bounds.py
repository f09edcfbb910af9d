"""The bound a device-made cloud carries (dliom_cloud_bounds: max_norm, abs_max) against cloud_max_norm's arithmetic in
numpy float32 (tests/cloud_bounds_common.py ref_max_norm) on the cloud's own downloaded points, by bit pattern: sqrt is
correctly rounded and monotone and the order of operations is fixed, so equality is the tolerance -- and the reference's
matcher takes the maximum over the filtered cloud, so a larger "safe" bound is a difference as well.  No downloaded byte
depends on the bound; the matchers' windows and the grids' growth do.  The inputs are prescribed (sizes around 64 and 256,
the farthest kept or removed point at the first / last lane, thread and point); tests/test_cloud_bounds_host.py checks on
the CPU that every case keeps and removes what it claims."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_common as ac  # noqa: E402
import cloud_bounds_common as cb  # noqa: E402
from cloud_bounds_common import f32  # noqa: E402

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


def check(name, bounds, points, want_points=None):
    """bounds of a device-made cloud against its downloaded points (and those against what the stage must keep)."""
    max_norm, abs_max = bounds
    if want_points is not None:
        assert points.tobytes() == np.ascontiguousarray(want_points, f32).tobytes(), name
    want = cb.ref_max_norm(points)
    assert cb.bits(max_norm) == cb.bits(want), (name, max_norm, want)
    with np.errstate(all="ignore"):
        for a in range(3):  # negative: unknown; else at least the true maximum
            finite = np.abs(points[:, a])[~np.isnan(points[:, a])]
            assert abs_max[a] < 0 or len(finite) == 0 or abs_max[a] >= finite.max(), (name, a, abs_max)


@pytest.mark.parametrize("n", cb.SIZES)
def test_host_upload_equals_numpy_reference(dl, ctx, n):
    """Ties ref_max_norm to cloud_max_norm (core.hip), on the same clouds the stages below get; abs_max of finite points
    is the true maximum."""
    for kind in ("range", "remover", "voxel"):
        for case in cb.cases(kind, n):
            cloud = dl.PointCloud(ctx, case.points)
            max_norm, abs_max = cloud.bounds()
            assert cb.bits(max_norm) == cb.bits(cb.ref_max_norm(case.points)), case.name
            if len(case.points) and np.isfinite(case.points).all():
                assert cb.bits(abs_max) == cb.bits(np.abs(case.points).max(axis=0)), case.name
            cloud.close()
    for case in cb.sampler_cases()[-6:]:  # a NaN and an infinity among them
        cloud = dl.PointCloud(ctx, case.points)
        assert cb.bits(cloud.bounds()[0]) == cb.bits(cb.ref_max_norm(case.points)), case.name
        cloud.close()


@pytest.mark.parametrize("n", cb.SIZES)
def test_range_filter(dl, ctx, n):
    for case in cb.cases("range", n):
        cloud = dl.PointCloud(ctx, case.points)
        kept, index = cloud.min_max_range_filter((0, 0, 0), *case.params)
        assert np.array_equal(index, np.flatnonzero(case.keep)), case.name
        check(case.name, kept.bounds(), kept.download(), case.points[case.keep])
        kept.close()
        cloud.close()
        batch = dl.PointsBatch(ctx, case.points, (0, 0, 0))
        batch.min_max_range_filter(*case.params)
        check(case.name + " (batch)", batch.cloud().bounds(), batch.download()[0], case.points[case.keep])
        batch.close()


@pytest.mark.parametrize("n", cb.SIZES)
def test_outlier_remover(dl, ctx, n):
    for case in cb.cases("remover", n):
        for as_batch in (False, True):
            remover = dl.OutlierRemover(ctx, cb.EDGE)
            if case.keep.any():
                hits = dl.PointCloud(ctx, case.points[case.keep])
                remover.mark_hits(hits)
                hits.close()
            if as_batch:
                batch = dl.PointsBatch(ctx, case.points, (0, 0, 0))
                batch.remove_outliers(remover)
                check(case.name + " (batch)", batch.cloud().bounds(), batch.download()[0], case.points[case.keep])
                batch.close()
            else:
                cloud = dl.PointCloud(ctx, case.points)
                kept, index = remover.filter(cloud)
                assert np.array_equal(index, np.flatnonzero(case.keep)), case.name
                check(case.name, kept.bounds(), kept.download(), case.points[case.keep])
                kept.close()
                cloud.close()
            remover.close()


@pytest.mark.parametrize("n", cb.SIZES)
def test_voxel_filters(dl, ctx, orc, n):
    for case in cb.cases("voxel", n):
        cloud = dl.PointCloud(ctx, case.points)
        want = case.points[case.keep]
        out = cloud.voxel_filter(cb.EDGE)
        check(case.name + " (plain)", out.bounds(), out.download(), want)
        out.close()
        cropped = orc.adaptive_voxel_filter(*cb.ADAPTIVE_CROPPED, case.points) if len(case.points) else want
        for options, expect in ((cb.ADAPTIVE_ALL, want), (cb.ADAPTIVE_CROPPED, cropped)):
            out = cloud.adaptive_voxel_filter(*options)
            check(case.name + " (adaptive %s)" % (options,), out.bounds(), out.download(), expect)
            out.close()
        a, b = cloud.adaptive_voxel_filter_pair(cb.ADAPTIVE_ALL, cb.ADAPTIVE_CROPPED)
        check(case.name + " (pair, first)", a.bounds(), a.download(), want)
        check(case.name + " (pair, second)", b.bounds(), b.download(), cropped)
        if "kept_far" in case.name and n > 1:  # the farthest point lies beyond the second filter's max_range
            assert b.bounds()[0] < a.bounds()[0], case.name
        a.close()
        b.close()
        cloud.close()


def test_sampler(dl, ctx):
    for case in cb.sampler_cases():
        sampler = dl.FixedRatioSampler(case.params)
        batch = dl.PointsBatch(ctx, case.points, (0, 0, 0))
        batch.fixed_ratio_sample(sampler)
        check(case.name, batch.cloud().bounds(), batch.download()[0], case.points[case.keep])
        if "repaired" in case.name:
            assert sampler.stats()["repaired_chunks"] > 0, case.name
        elif case.params == 0.5:
            assert sampler.stats()["repaired_chunks"] == 0, case.name
        batch.close()
        sampler.close()


def test_sampler_carries_its_state_into_the_next_batch(dl, ctx):
    """The second batch starts from the first one's state (chunk 0 from the true counts, the others from a guess)."""
    sampler = dl.FixedRatioSampler(0.55)
    pulses = samples = 0
    for n in (4097, 257, 4097):
        keep = cb.sampler_keep(0.55, n, pulses, samples)
        kept = np.flatnonzero(keep)
        pts = cb.shell(n, keep, int(kept[-1]), int(np.flatnonzero(~keep)[-1]))
        batch = dl.PointsBatch(ctx, pts, (0, 0, 0))
        batch.fixed_ratio_sample(sampler)
        check("sampler state %d" % n, batch.cloud().bounds(), batch.download()[0], pts[keep])
        batch.close()
        pulses, samples = pulses + n, samples + int(keep.sum())
        assert sampler.state() == (pulses, samples)
    sampler.close()


@pytest.mark.parametrize("n", cb.SIZES)
def test_front_end_returns_cloud(dl, ctx, orc, n):
    """dliom_add_range_data hands its caller a device-made cloud (voxel filter, de-skew and gate, voxel filter, transform
    into the tracking frame): its bound comes from transform_kernel's per-workgroup maxima folded on the host, and it is
    the one producer that knows abs_max -- which must be the true maximum a coordinate.  A range beyond 4095 voxel edges
    takes both stages off their packed path (counted)."""
    prev, cur = cb.frontend_poses()
    for case in cb.frontend_cases(n):
        want, index = cb.frontend_oracle(orc, case)
        reruns = ctx.voxel_filter_reruns()
        cloud, _, _ = dl.add_range_data(ctx, prev, cur, cb.FRONTEND_PERIOD, case.points, (0, 0, 0), *case.params, cb.FRONTEND_VFS)
        got = cloud.download()
        assert len(got) == case.keep.sum() and np.array_equal(index, np.flatnonzero(case.keep)), case.name
        check(case.name, cloud.bounds(), got, want)
        max_norm, abs_max = cloud.bounds()
        if len(got):
            assert cb.bits(abs_max) == cb.bits(np.abs(got).max(axis=0)), (case.name, abs_max)
        else:
            assert cb.bits(max_norm) == cb.bits(0.0), case.name
        general = "general_path" in case.name
        assert (ctx.voxel_filter_reruns() - reruns >= 2) if general else (ctx.voxel_filter_reruns() == reruns), case.name
        cloud.close()


@pytest.fixture(scope="module")
def assemble_model(tmp_path_factory):
    return ac.build_model(tmp_path_factory.mktemp("assemble_model"))


def test_assembler(dl, ctx, assemble_model, tmp_path):
    times, poses, cloud_time = cb.assemble_trajectory()
    all_cases = cb.assemble_cases()
    pushed, results = ac.run_model(assemble_model, times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, c.points) for c in all_cases],
                                   tmp_path)
    assert pushed == 0
    trajectory = dl.Trajectory(ctx, times, poses)
    for case, want in zip(all_cases, results):
        cloud, origin, index = trajectory.assemble(cloud_time, case.points, ac.MOUNT)
        batch = dl.PointsBatch.from_sensor_points(trajectory, cloud_time, case.points, ac.MOUNT)
        if not case.keep.any():
            assert cloud is None and batch is None, case.name  # the reference returns nullptr: no cloud, no bound
            continue
        assert np.array_equal(index, want["index"]), case.name
        check(case.name, cloud.bounds(), cloud.download(), want["xyz"])
        check(case.name + " (batch)", batch.cloud().bounds(), batch.download()[0], want["xyz"])
        cloud.close()
        batch.close()
    trajectory.close()

