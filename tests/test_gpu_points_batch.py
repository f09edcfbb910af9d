"""Export batches in HBM (dliom_points_batch_*, dliom_fixed_ratio_sampler_*, dliom_points_xray_insert_batch) against the
CPU model of the reference's loops (tests/cpp/points_batch_model.cc).  Every comparison is exact equality of bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_common as ac  # noqa: E402
import points_batch_common as pb  # noqa: E402
import points_xray_common as pxc  # noqa: E402
from points_batch_common import PCD, PLY, f32  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 4097]
ATTRIBUTES = ["none", "intensities", "colors", "both", "single"]
PATTERNS = ["none", "all", "every_other", "first", "last"]
SINGLE = np.array([0.25, 0.5, 0.75], dtype=f32)


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return pb.build_model(tmp_path_factory.mktemp("points_batch_model"))


@pytest.fixture(scope="module")
def assemble_model(tmp_path_factory):
    return ac.build_model(tmp_path_factory.mktemp("assemble_model"))


def keep_pattern(n, pattern):
    keep = np.zeros(n, dtype=bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "every_other":
        keep[::2] = True
    elif pattern == "first":
        keep[:1] = True
    elif pattern == "last":
        keep[-1:] = True
    return keep


def cases():
    """(n, attributes, pattern, keep, points, intensities, colors as the model sees them)"""
    out = []
    for n in SIZES:
        for a, attributes in enumerate(ATTRIBUTES):
            for p, pattern in enumerate(PATTERNS):
                pts, it, col = pb.batch_arrays(n, 1000 * n + 10 * a + p, "none" if attributes == "single" else attributes)
                if attributes == "single" and n > 0:
                    col = np.tile(SINGLE, (n, 1))
                out.append((n, attributes, pattern, keep_pattern(n, pattern), pts, it, col))
    return out


def make_batch(dl, ctx, pts, it, col, attributes, origin=(0, 0, 0)):
    if attributes == "single":
        b = dl.PointsBatch(ctx, pts, origin, it, None)
        b.color(SINGLE)
        return b
    return dl.PointsBatch(ctx, pts, origin, it, col)


def counted(ctx, call):
    """-> (read-backs, synchronisations) the call took"""
    r0, s0 = ctx.read_backs(), ctx.synchronizations()
    call()
    return ctx.read_backs() - r0, ctx.synchronizations() - s0


def check_counters(records):
    """records: [(n, attributes, read-backs, synchronisations)] of compacting calls"""
    by_attributes = {}
    for n, attributes, reads, syncs in records:
        assert reads == (1 if n > 0 else 0), (n, attributes, reads)
        if n > 0:
            by_attributes.setdefault(attributes, set()).add(syncs)
    for attributes, syncs in by_attributes.items():
        assert len(syncs) == 1, (attributes, syncs)  # the same for 1 point and for 4097


def test_range_filter_gathers_attributes(dl, ctx, model, tmp_path):
    all_cases = cases()
    want = pb.run_model(model, [pb.remove_op(pts, it, col, keep) for (_, _, _, keep, pts, it, col) in all_cases], tmp_path)
    records = []
    for (n, attributes, pattern, keep, pts, it, col), w in zip(all_cases, want):
        # random directions; the kept points lie 10 m from the origin, the others 30 m
        d = np.random.RandomState(n).normal(size=(n, 3)) + 1e-3
        moved = (d / np.linalg.norm(d, axis=1)[:, None] * np.where(keep, 10.0, 30.0)[:, None]).astype(f32)
        b = make_batch(dl, ctx, moved, it, col, attributes)
        reads, syncs = counted(ctx, lambda: b.min_max_range_filter(5.0, 20.0))
        records.append((n, attributes, reads, syncs))
        pb.assert_batch_equals(b, (moved[keep], w[1], w[2]))
        assert w[0].tobytes() == pts[keep].tobytes()  # the model removed the same points
        b.close()
    check_counters(records)


def test_outlier_filter_batch_gathers_attributes(dl, ctx, model, tmp_path):
    all_cases = [c for c in cases() if c[1] in ("none", "both", "single")]
    want = pb.run_model(model, [pb.remove_op(pts, it, col, keep) for (_, _, _, keep, pts, it, col) in all_cases], tmp_path)
    records = []
    for (n, attributes, pattern, keep, _, it, col), w in zip(all_cases, want):
        # one point a voxel of 0.5 m; the voxels of the kept points have a hit, the others none: !(0 < 3 * 0) removes them
        pts = np.stack([0.5 * np.arange(n) + 0.25, np.full(n, 0.25), np.full(n, 0.25)], axis=1).astype(f32)
        remover = dl.OutlierRemover(ctx, 0.5)
        if keep.any():
            hits = dl.PointCloud(ctx, pts[keep])
            remover.mark_hits(hits)
            hits.close()
        b = make_batch(dl, ctx, pts, it, col, attributes)
        reads, syncs = counted(ctx, lambda: b.remove_outliers(remover))
        records.append((n, attributes, reads, syncs))
        pb.assert_batch_equals(b, (pts[keep], w[1], w[2]))
        b.close()
        remover.close()
    check_counters(records)


def test_from_sensor_points_gathers_intensities(dl, ctx, assemble_model, tmp_path):
    from dliom import synth
    times = ac.EPOCH + 100_000 * np.arange(5, dtype=np.int64)
    poses = np.array([synth.trajectory_pose(3.0 * k) for k in range(5)])
    trajectory = dl.Trajectory(ctx, times, poses)
    t_end = int(times[-1])
    batches, keeps = [], []
    for n in SIZES:
        for p, pattern in enumerate(PATTERNS):
            keep = keep_pattern(n, pattern)
            rng = np.random.RandomState(77 * n + p)
            xyzt = np.zeros((n, 4), dtype=f32)
            xyzt[:, :3] = rng.uniform(-20.0, 20.0, size=(n, 3))
            inside = -np.linspace(1000.0, 399_000.0, max(n, 1))[:n]
            xyzt[:, 3] = (np.where(keep, inside, inside - 500_000.0) / ac.TICKS).astype(f32)
            batches.append((t_end, ac.MOUNT, xyzt))
            keeps.append(keep)
    pushed, want = ac.run_model(assemble_model, times, poses, [ac.assemble_op(*b) for b in batches], tmp_path)
    assert pushed == 0
    records = []
    for (cloud_time, mount, xyzt), keep, w in zip(batches, keeps, want):
        n = len(xyzt)
        assert np.array_equal(w["index"], np.flatnonzero(keep))
        for with_intensities in (False, True):
            it = np.random.RandomState(n).uniform(0.0, 255.0, size=n).astype(f32) if with_intensities else None
            made = []
            reads, syncs = counted(ctx, lambda: made.append(dl.PointsBatch.from_sensor_points(trajectory, cloud_time, xyzt, mount, it)))
            records.append((n, with_intensities, reads, syncs))
            b = made[0]
            if not keep.any():
                assert b is None
                continue
            pb.assert_batch_equals(b, (w["xyz"], it[keep] if with_intensities else None, None))
            assert b.origin.tobytes() == w["origin"].tobytes()
            b.close()
    check_counters(records)
    trajectory.close()


RATIOS = [0.0, 1.0, 0.5, 0.1, 1.0 / 3.0, 0.55, 9.0 / 14.0, 9.0 / 11.0, 1e-4, 1.0 - 2.0 ** -53]
SEQUENCES = [[1] * 40, [63, 64, 65, 0, 4097], [7000, 7000, 7000, 7000]]


def run_sampler(dl, ctx, sampler, sizes):
    """-> per batch (kept input indices, state after it); the points carry their own index in x and an intensity"""
    out = []
    for n in sizes:
        index = np.arange(n, dtype=f32)
        pts = np.stack([index, np.zeros(n, dtype=f32), np.zeros(n, dtype=f32)], axis=1)
        b = dl.PointsBatch(ctx, pts, (0, 0, 0), index + f32(0.5), None)
        b.fixed_ratio_sample(sampler)
        got, it, _ = b.download()
        assert it is None or it.tobytes() == (got[:, 0] + f32(0.5)).tobytes()
        out.append((got[:, 0].astype(np.int64), sampler.state()))
        b.close()
    return out


@pytest.mark.parametrize("sequence", range(len(SEQUENCES)))
def test_sampler_equals_sequential_loop(dl, ctx, model, tmp_path, sequence):
    """The last sequence carries the state across batches and passes pulses at which the guessed chunk start is wrong
    (0.55: 1600, 2880, 3200, ...), so its repair passes run."""
    sizes = SEQUENCES[sequence]
    for ratio in RATIOS:
        # the model's loop over all the pulses, cut at the batches (tests/test_points_batch_host.py: the state carries over)
        keep, _, _ = pb.run_model(model, [pb.pulse_op(ratio, 0, 0, sum(sizes))], tmp_path)[0]
        want, at = [], 0
        for n in sizes:
            want.append((np.flatnonzero(keep[at:at + n]), (at + n, int(np.sum(keep[:at + n])))))
            at += n
        sampler = dl.FixedRatioSampler(ratio)
        for run in range(2):
            got = run_sampler(dl, ctx, sampler, sizes)
            for (gi, gs), (wi, ws) in zip(got, want):
                assert np.array_equal(gi, wi), (ratio, sizes)
                assert gs == ws, (ratio, gs, ws)
            sampler.reset()
            assert sampler.state() == (0, 0)
        sampler.close()


def test_sampler_repairs_wrong_guesses(dl, ctx, model, tmp_path):
    """Ratio 0.55 over 30 000 pulses from (0, 0): with chunks of 64 pulses the guess ceil(ratio * pulses) is wrong at 54
    chunk starts (the loop on the CPU, k = 1600 the first), so chunks are repaired; for 0.5 the guess is always right."""
    for ratio, repaired in ((0.55, True), (0.5, False)):
        keep, pulses, samples = pb.run_model(model, [pb.pulse_op(ratio, 0, 0, 30000)], tmp_path)[0]
        sampler = dl.FixedRatioSampler(ratio)
        (got, state), = run_sampler(dl, ctx, sampler, [30000])
        assert np.array_equal(got, np.flatnonzero(keep)) and state == (pulses, samples)
        stats = sampler.stats()
        assert stats["chunks"] == (30000 + 63) // 64
        if repaired:
            assert stats["repaired_chunks"] > 0 and stats["repair_passes"] > 0, stats
        else:
            assert stats["repaired_chunks"] == 0 and stats["repair_passes"] == 0, stats
        sampler.close()


def special_intensities():
    rng = np.random.RandomState(5)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 10.0, 255.0, 254.99998], dtype=f32)
    return np.concatenate([rng.uniform(-10.0, 300.0, size=1000).astype(f32), special])


@pytest.mark.parametrize("bounds", [(0.0, 255.0), (10.0, 10.0), (255.0, 0.0)])
def test_intensity_to_color_bits(dl, ctx, model, tmp_path, bounds):
    it = special_intensities()
    pts, _, _ = pb.batch_arrays(len(it), 9, "none")
    want = pb.run_model(model, [pb.intensity_to_color_op(pts, it, None, *bounds),
                                pb.intensity_to_color_op(pts, None, None, *bounds)], tmp_path)
    b = dl.PointsBatch(ctx, pts, (0, 0, 0), it, None)
    b.intensity_to_color(*bounds)
    _, _, col = b.download()
    assert col.view(np.uint32).tobytes() == want[0][2].view(np.uint32).tobytes()  # NaNs by bit pattern
    b.close()
    plain = dl.PointsBatch(ctx, pts)  # no intensities: left alone
    plain.intensity_to_color(*bounds)
    assert not plain.has_colors and want[1][2] is None
    plain.close()


def test_color_then_filter(dl, ctx, model, tmp_path):
    pts, it, col = pb.batch_arrays(600, 4, "both")
    rgb = np.array([0.125, 1.0, 0.0], dtype=f32)
    keep = np.linalg.norm(pts.astype(np.float64), axis=1)
    keep = (keep >= 5.0) & (keep <= 20.0)
    norms = np.sqrt(pts[:, 0] * pts[:, 0] + (pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2]))
    assert not np.any(np.abs(norms - 5.0) < 1e-3) and not np.any(np.abs(norms - 20.0) < 1e-3)  # no point near a bound
    colored = pb.run_model(model, [pb.color_op(pts, it, col, rgb)], tmp_path)[0]
    want = pb.run_model(model, [pb.remove_op(pts, it, colored[2], keep)], tmp_path)[0]
    b = dl.PointsBatch(ctx, pts, (0, 0, 0), it, col)
    b.color(rgb)
    b.min_max_range_filter(5.0, 20.0)
    pb.assert_batch_equals(b, want)
    assert 0 < len(b) < 600
    b.close()


TIE_COLORS = np.array([0.0, 1.0, 0.5, 1.0 / 510.0, 3.0 / 510.0, -0.0, 2.0, -1.0, np.inf, -np.inf, 0.3, 0.999], dtype=f32)
# (format, with_colors, with_intensities) -> record bytes
RECORDS = {(PLY, 0, 0): 12, (PLY, 1, 0): 15, (PLY, 0, 1): 16, (PLY, 1, 1): 19, (PCD, 0, 0): 12, (PCD, 1, 0): 16}


@pytest.mark.parametrize("layout", sorted(RECORDS))
def test_pack_equals_model(dl, ctx, model, tmp_path, layout):
    fmt, with_colors, with_intensities = layout
    sizes = [0, 1, 2, 3, 4, 5, 255, 256, 257, 1025]
    inputs = []
    for n in sizes:
        pts, it, _ = pb.batch_arrays(n, 31 + n, "intensities")
        col = np.resize(TIE_COLORS, 3 * n).reshape(n, 3) if with_colors else None
        inputs.append((pts, it if with_intensities else None, col))
    want = pb.run_model(model, [pb.pack_op(p, i, c, fmt, with_colors, with_intensities) for (p, i, c) in inputs], tmp_path)
    for n, (pts, it, col), w in zip(sizes, inputs, want):
        assert len(w) == n * RECORDS[layout]
        b = dl.PointsBatch(ctx, pts, (0, 0, 0), it, col)
        assert b.pack_size(fmt, with_colors, with_intensities) == len(w)
        out, written = b.pack(fmt, with_colors, with_intensities, capacity=len(w) + 8, fill=0xA5)
        assert written == len(w) and out[:written].tobytes() == w
        # The destination beyond num_bytes is untouched.  (This pins the copy to the host, which is exactly num_bytes long;
        # the kernel's own tail of 1 to 3 bytes lands in scratch and is covered by the equality above: records of 15 and
        # 19 bytes with n = 1, 2, 3, 5 leave tails of every length.)
        assert np.all(out[written:] == 0xA5)
        if n > 0:
            with pytest.raises(dl.DliomError) as e:
                b.pack(fmt, with_colors, with_intensities, capacity=len(w) - 1)
            assert e.value.status == dl.ERR_CAPACITY
        b.close()


def test_pack_single_color_and_refusals(dl, ctx, model, tmp_path):
    pts, it, _ = pb.batch_arrays(300, 8, "intensities")
    want = pb.run_model(model, [pb.pack_op(pts, it, np.tile(SINGLE, (300, 1)), PLY, 1, 1)], tmp_path)[0]
    b = dl.PointsBatch(ctx, pts, (0, 0, 0), it, None)
    before = b.download()
    for args in ((PLY, 1, 0), (PCD, 1, 0), (PCD, 0, 1), (7, 0, 0)):  # no colours yet; PCD has no intensities; no such format
        with pytest.raises(dl.DliomError) as e:
            b.pack(*args)
        assert e.value.status == dl.ERR_INVALID_ARGUMENT
    b.color(SINGLE)
    out, written = b.pack(PLY, 1, 1)
    assert out.tobytes() == want
    b.close()
    plain = dl.PointsBatch(ctx, pts)
    with pytest.raises(dl.DliomError) as e:
        plain.pack(PLY, 0, 1)  # the file has intensities, the batch has none
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    assert plain.download()[0].tobytes() == before[0].tobytes()
    plain.close()


@pytest.mark.parametrize("colors", ["none", "constant", "intensity"])
def test_xray_insert_batch_equals_host_colors(dl, ctx, colors):
    ops = pxc.drive_ops(3, 16, 128, colors)
    host, device = dl.PointsXray(ctx, 0.25, pxc.TRANSFORMS["yz"]), dl.PointsXray(ctx, 0.25, pxc.TRANSFORMS["yz"])
    for _, _, pts, col in ops:
        cloud = dl.PointCloud(ctx, pts)
        host.insert(cloud, None if len(col) == 0 else col)
        cloud.close()
        b = dl.PointsBatch(ctx, pts, (0, 0, 0), None, col if len(col) == len(pts) else None)
        if len(col) == 1:
            b.color(col[0])
        assert b.has_colors == (len(col) > 0)
        b.xray_insert(device)
        b.close()
    for a, b in zip(host.columns(), device.columns()):
        assert a.tobytes() == b.tobytes()
    assert len(host.columns()[0]) > 100
    assert host.voxels().tobytes() == device.voxels().tobytes()
    image = host.draw()
    assert image.size > 0 and image.tobytes() == device.draw().tobytes()
    host.close()
    device.close()


def test_refusals_leave_the_batch_unchanged(dl, ctx):
    L = dl.load_library()
    pts, it, col = pb.batch_arrays(300, 2, "both")
    origin = np.zeros(3, dtype=f32)
    h = C.c_void_p()

    def create(n, intensities, colors, num_colors, out=C.byref(h)):
        return L.dliom_points_batch_create(ctx.h, pts.ctypes.data_as(C.POINTER(C.c_float)), n, origin.ctypes.data_as(C.POINTER(C.c_float)),
                                           intensities, colors, num_colors, out)

    colp = col.ctypes.data_as(C.POINTER(C.c_float))
    for num_colors in (1, 299, 301, -1):  # RemovePoints indexes past the end of such a vector
        assert create(300, None, colp, num_colors) == dl.ERR_INVALID_ARGUMENT
    assert create(300, None, None, 300) == dl.ERR_INVALID_ARGUMENT
    assert create(-1, None, None, 0) == dl.ERR_INVALID_ARGUMENT
    assert create(300, None, None, 0, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_create(None, None, 0, origin.ctypes.data_as(C.POINTER(C.c_float)), None, None, 0, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    for f in (L.dliom_points_batch_destroy, L.dliom_fixed_ratio_sampler_destroy, L.dliom_fixed_ratio_sampler_reset):
        assert f(None) == dl.ERR_INVALID_ARGUMENT
    b = dl.PointsBatch(ctx, pts, (0, 0, 0), it, col)
    before = b.download()
    sampler, remover = dl.FixedRatioSampler(0.5), dl.OutlierRemover(ctx, 0.5)
    assert L.dliom_points_batch_fixed_ratio_sample(None, b.h) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_fixed_ratio_sample(sampler.h, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_outlier_remover_filter_batch(None, b.h) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_outlier_remover_filter_batch(remover.h, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_min_max_range_filter(None, 0.0, 1.0) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_min_max_range_filter(b.h, float("nan"), 1.0) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_color(b.h, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_xray_insert_batch(None, b.h) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_pack(b.h, PLY, 1, 1, None, 0, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_download(None, None, None, None) == dl.ERR_INVALID_ARGUMENT
    # objects of another context
    other = dl.Context(0)
    foreign_remover, foreign_xray = dl.OutlierRemover(other, 0.5), dl.PointsXray(other, 0.25)
    assert L.dliom_outlier_remover_filter_batch(foreign_remover.h, b.h) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_xray_insert_batch(foreign_xray.h, b.h) == dl.ERR_INVALID_ARGUMENT
    assert foreign_remover.stats()["phase"] == 1 and sampler.state() == (0, 0)
    # a non-finite point: phase three refuses it after its flags ran
    bad = pts.copy()
    bad[17, 1] = np.nan
    nb = dl.PointsBatch(ctx, bad, (0, 0, 0), it, col)
    assert L.dliom_outlier_remover_filter_batch(remover.h, nb.h) == dl.ERR_INVALID_ARGUMENT
    got = nb.download()
    assert got[0].view(np.uint32).tobytes() == bad.view(np.uint32).tobytes() and got[1].tobytes() == it.tobytes() and got[2].tobytes() == col.tobytes()
    after = b.download()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    for o in (nb, b, sampler, remover, foreign_remover, foreign_xray):
        o.close()
    other.close()


def test_adapter_pipeline_stays_on_the_device(dl, tmp_path):
    """tests/cpp/points_batch_adapter.cc: assemble -> min_max_range_filter -> fixed_ratio_sampler (0.55) -> outlier removal
    (three phases) -> intensity_to_color -> write_xray_image -> write_ply over four 16 x 256 scans, once on device batches
    and once on host vectors with the reference's sampler and PLY loops.  The files and the images are equal; the device
    run uploads no cloud from host points and downloads the packed records and nothing else of the batches."""
    exe = pb.build_adapter(tmp_path, dl.LIB_PATH)
    times, poses, mount, messages = pb.pipeline_messages(16, 256)
    out = pb.run_adapter(exe, tmp_path, times, poses, mount, messages)
    ply, image = out["device"]
    assert ply == out["host"][0]
    assert image.size > 1000 and image.tobytes() == out["host"][1].tobytes() and image.shape == out["host"][1].shape
    header = dl.ply_header(1, 1, out["records"] // 19)
    assert out["records"] % 19 == 0 and ply[:len(header)] == header
    sampled = sum(len(m[1]) for m in messages)
    assert 0.2 * sampled < out["records"] // 19 < 0.55 * sampled + 4  # sampled, and some points removed behind the sampler
    assert out["uploads"] == 0
    assert out["downloaded"] == out["records"]
