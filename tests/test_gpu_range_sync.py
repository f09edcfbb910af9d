"""Two range sensors' clouds merged on the device (dliom_timed_cloud_stamp, dliom_timed_clouds_merge,
dliom_range_accumulator_add_timed_cloud) against the model of tests/range_sync_common.py, whose order of equal times is
the real std::sort's.  Every comparison is exact equality of bits, the origin-index channel included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import range_sync_common as rs  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


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


def assert_cloud_equals(cloud, xyzt, origin_index=None, what=""):
    got, _ = cloud.download()
    assert len(cloud) == len(xyzt), what
    assert np.array_equal(bits(got), bits(xyzt)), what
    front, back = cloud.front_back_time()
    want = (xyzt[0, 3], xyzt[-1, 3]) if len(xyzt) else (f32(0), f32(0))
    assert bits([front, back]).tolist() == bits(want).tolist(), what
    assert cloud.has_origin_index == (origin_index is not None) and not cloud.has_intensities, what
    if origin_index is not None:
        assert np.array_equal(bits(cloud.download_origin_index()), bits(origin_index)), what


def device_merge(dl, ctx, primary, primary_time, secondary, secondary_time, stamped=None):
    """the device's merge of arrays -> dl.TimedCloud (the inputs are closed again)"""
    clouds = [rs.upload(dl, ctx, a) for a in (primary, secondary)] + ([rs.upload(dl, ctx, stamped)] if stamped is not None else [])
    try:
        return dl.merge_timed_clouds(ctx, clouds[0], primary_time, clouds[1], secondary_time,
                                     primary_for_times=clouds[2] if stamped is not None else None)
    finally:
        for c in clouds:
            c.close()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 256, 257, 4097])
def test_stamp_equals_model(dl, ctx, n):
    xyzt = rs.points(n, rs.times("runs of 64", n))
    for scan_period in (0.1, 0.05):
        cloud = rs.upload(dl, ctx, xyzt)
        stamped = cloud.stamp(scan_period)
        assert_cloud_equals(stamped, rs.stamp(xyzt, scan_period), what="n %d period %g" % (n, scan_period))
        assert_cloud_equals(cloud, xyzt)  # the input is untouched
        stamped.close()
        cloud.close()


# 16 | 17: the insertion-sort threshold; 4096 | 4097: the sort in LDS, the radix sort with the replay in HBM arrays;
# 15 391 | 15 392 and 65 535 | 65 537: where the replay's segments leave LDS
@pytest.mark.parametrize("pattern", rs.PATTERNS)
@pytest.mark.parametrize("m", [16, 17, 4096, 4097, 15391, 15392, 65535, 65537])
def test_merge_equals_model(dl, ctx, orc, m, pattern):
    primary, primary_time, secondary, secondary_time = rs.pair_of_merged_size(m, m, pattern)
    want_xyzt, want_origin = rs.merge(orc, primary, primary_time, secondary, secondary_time)
    assert len(want_xyzt) == m and 0 < want_origin.sum() < m
    if pattern != "distinct" and m > 200:
        t = want_xyzt[:, 3]
        assert np.max(np.bincount(np.unique(t, return_inverse=True)[1])) >= 64  # runs of equal times
    merged = device_merge(dl, ctx, primary, primary_time, secondary, secondary_time)
    assert_cloud_equals(merged, want_xyzt, want_origin, "m %d %s" % (m, pattern))
    merged.close()


def _window_case(secondary_t, secondary_offset_ticks, n_p=40):
    primary = rs.points(11, rs.times("distinct", n_p))
    secondary = rs.points(12, np.asarray(secondary_t, f32))
    return primary, rs.PRIMARY_TIME, secondary, rs.PRIMARY_TIME + secondary_offset_ticks


def test_overlap_edges(dl, ctx, orc):
    """The window is [current_end - 0.1f, current_end], both ends inclusive.  With the secondary stamped like the primary
    its times are offsets from current_end itself, so a point can sit exactly on either end; with another stamp the times
    below keep well away from the ends."""
    assert rs.seconds(rs.PRIMARY_TIME) == 1_790_000_000.0
    on_start = float(f32(-0.1))
    cases = {
        "a point exactly on current_start and one exactly on current_end": (_window_case([-0.5, on_start, -0.0625, -0.03125, 0.0], 0), (1, 5)),
        "i_start = 0": (_window_case([-0.09375, -0.0625, 0.0], 0), (0, 3)),
        "no point behind the window (i_end = last)": (_window_case([-0.25, -0.125, -0.0625, -0.03125, 0.0], 0), (2, 5)),
        "points behind the window": (_window_case([-0.25, -0.0625, -0.046875, 0.0], 312_500), (1, 3)),
        "a one-point overlap": (_window_case([-0.5, -0.125, -0.03125, 0.0], 625_000), (1, 2)),
        "an empty primary: the window is one instant": (_window_case([-0.0625, 0.0], 0, n_p=0), (1, 2)),
    }
    for what, ((primary, pt, secondary, st), want_bounds) in cases.items():
        found = rs.overlap(primary, pt, secondary, st)
        assert found is not None and found[:2] == want_bounds, (what, found)
        want_xyzt, want_origin = rs.merge(orc, primary, pt, secondary, st)
        assert int(want_origin.sum()) == want_bounds[1] - want_bounds[0], what
        merged = device_merge(dl, ctx, primary, pt, secondary, st)
        assert_cloud_equals(merged, want_xyzt, want_origin, what)
        merged.close()
    # the first case by hand: the point on current_start has the primary's first time, the one on current_end time 0
    (primary, pt, secondary, st), _ = cases["a point exactly on current_start and one exactly on current_end"]
    assert st == pt and secondary[1, 3] == primary[0, 3] and secondary[4, 3] == 0


def test_no_overlap_is_refused_and_leaves_the_context_usable(dl, ctx, orc):
    primary, pt, secondary, st = _window_case([-0.03125, 0.0], 10_000_000)  # a whole second later: nothing inside
    assert rs.merge(orc, primary, pt, secondary, st) is None
    with pytest.raises(dl.DliomError) as e:
        device_merge(dl, ctx, primary, pt, secondary, st)
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    with pytest.raises(dl.DliomError) as e:  # an empty secondary has no i_start either
        device_merge(dl, ctx, primary, pt, np.zeros((0, 4), f32), pt)
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    # ... and the same context merges the next pair
    primary, pt, secondary, st = rs.pair_of_merged_size(5, 300, "runs of 64")
    want_xyzt, want_origin = rs.merge(orc, primary, pt, secondary, st)
    merged = device_merge(dl, ctx, primary, pt, secondary, st)
    assert_cloud_equals(merged, want_xyzt, want_origin)
    merged.close()


def test_manual_deskew_keeps_the_unstamped_times(dl, ctx, orc):
    """the window comes from the stamped copy, the merged prior points keep the message's times (:94)"""
    n_p = 500
    primary = rs.points(21, rs.times("runs of 64", n_p) * f32(0.5))  # the message's sweep: 0.05 s
    stamped = rs.stamp(primary, 0.1)
    secondary = rs.points(22, rs.times("runs of 64", 700))
    st = rs.PRIMARY_TIME + 250_000  # its points between -0.1 s and -0.05 s lie inside the stamped window only
    want_xyzt, want_origin = rs.merge(orc, primary, rs.PRIMARY_TIME, secondary, st, primary_for_times=stamped)
    narrow_xyzt, _ = rs.merge(orc, primary, rs.PRIMARY_TIME, secondary, st)
    assert len(want_xyzt) > len(narrow_xyzt)  # the stamped window is the wider one
    assert np.array_equal(np.sort(bits(want_xyzt[want_origin == 0][:, 3])), np.sort(bits(primary[:, 3])))
    p, s = rs.upload(dl, ctx, primary), rs.upload(dl, ctx, secondary)
    d = p.stamp(0.1)
    assert_cloud_equals(d, stamped)
    merged = dl.merge_timed_clouds(ctx, p, rs.PRIMARY_TIME, s, st, primary_for_times=d)
    assert_cloud_equals(merged, want_xyzt, want_origin)
    for c in (merged, d, p, s):
        c.close()


def test_consumers_of_one_sensor_refuse_the_channel(dl, ctx):
    primary, pt, secondary, st = rs.pair_of_merged_size(6, 100, "distinct")
    merged = device_merge(dl, ctx, primary, pt, secondary, st)
    pose = [0, 0, 0, 1, 0, 0, 0]
    with pytest.raises(dl.DliomError) as e:
        merged.add_range_data(pose, pose, 0.1, [0, 0, 0], 1.0, 100.0, 0.15)
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    for call in (lambda: merged.stamp(0.1), lambda: dl.merge_timed_clouds(ctx, merged, pt, merged, pt)):
        with pytest.raises(dl.DliomError) as e:
            call()
        assert e.value.status == dl.ERR_INVALID_ARGUMENT
    merged.close()


POSES = [np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]),
         np.array([0.05, -0.02, 0.01, 0.9998000066665778, 0.0, 0.0, 0.01999866669333308]),
         np.array([0.11, -0.03, 0.02, 0.9992001066609779, 0.0, 0.0, 0.03998933418663416])]
OPTS = dict(scan_period=0.1, min_range=1.0, max_range=60.0, voxel_filter_size=0.15)


def _finished(cloud, origin):
    xyz = cloud.download()
    return bits(xyz), bits(origin)


@pytest.mark.parametrize("two_origins", [False, True])
def test_accumulator_device_input_equals_host_input_and_oracle(dl, ctx, orc, two_origins):
    origins = [[0.1, 0.0, 0.3], [-0.4, 0.2, 0.5]] if two_origins else [[0.1, 0.0, 0.3]]
    from_device, from_host = dl.RangeDataAccumulator(ctx), dl.RangeDataAccumulator(ctx)
    oracle = orc.RangeDataAccumulator(OPTS["scan_period"], OPTS["min_range"], OPTS["max_range"], OPTS["voxel_filter_size"])
    args = (OPTS["scan_period"],)
    tail = (OPTS["min_range"], OPTS["max_range"], OPTS["voxel_filter_size"])
    for k in range(2):
        prev, predicted = POSES[k], POSES[k + 1]
        if two_origins:
            primary, pt, secondary, st = rs.pair_of_merged_size(30 + k, 5000 + k, "runs of 64")
            cloud = device_merge(dl, ctx, primary, pt, secondary, st)
            index = cloud.download_origin_index()
            assert 0 < index.sum() < len(index)
        else:
            cloud = rs.upload(dl, ctx, rs.points(40 + k, rs.times("runs of 64", 3000 + k)))
            index = None
        xyzt, _ = cloud.download()
        cur_d, count_d = from_device.add_timed_cloud(prev, predicted, *args, cloud, *tail, origins=origins)
        cur_h, count_h = from_host.add(prev, predicted, *args, xyzt, *tail, origins=origins, origin_index=index)
        cur_o = oracle.add(prev, predicted, xyzt, origins=origins, origin_index=None if index is None else index.astype(np.int32))
        assert count_d == count_h == k + 1
        assert np.array_equal(bits(cur_d), bits(cur_h)) and np.array_equal(bits(cur_d), bits(cur_o)), k
        cloud.close()
    cloud_d, origin_d = from_device.finish(OPTS["voxel_filter_size"])
    cloud_h, origin_h = from_host.finish(OPTS["voxel_filter_size"])
    want_xyz, want_origin = oracle.finish()
    got_d, got_h = _finished(cloud_d, origin_d), _finished(cloud_h, origin_h)
    assert len(got_d[0]) > 100
    assert np.array_equal(got_d[0], got_h[0]) and np.array_equal(got_d[1], got_h[1])
    assert np.array_equal(got_d[0], bits(want_xyz)) and np.array_equal(got_d[1], bits(want_origin))
    for c in (from_device, from_host):
        c.close()


@pytest.fixture(scope="module")
def adapter(dl, tmp_path_factory):
    """tests/cpp/range_sync_adapter.cc and its stream file: four 16 x 256 scans with their IMU samples"""
    import struct
    import subprocess
    from dliom import synth
    from test_gpu_parity import FRONT_END_OPTS
    d = tmp_path_factory.mktemp("range_sync_adapter")
    exe, libdir = str(d / "range_sync_adapter"), os.path.join(rs.ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(rs.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(rs.ROOT, "tests", "cpp", "range_sync_adapter.cc"),
                           os.path.join(rs.ROOT, "tests", "cpp", "point_cloud2_model.cc"), "-DPOINT_CLOUD2_MODEL_NO_MAIN",
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    T, scans_n = 0.1, 4
    centers = synth.bubbles()
    st = synth.trajectory_state(0.0)
    scans = [synth.moving_scan(T * k, 16, 256, centers) for k in range(1, scans_n + 1)]
    imus = [synth.imu_samples(T * (k - 1), T * k, 200.0) for k in range(1, scans_n + 1)]
    n = min(len(sc) for sc in scans)
    path = str(d / "stream.bin")
    with open(path, "wb") as f:  # (the stream file of tests/cpp/ltb3d_adapter.cc)
        f.write(struct.pack("4i", scans_n, n, len(imus[0][1]) - 1, 1))
        f.write(np.asarray(st, dtype=np.float64).tobytes())
        f.write(bytes(dl.front_end_options_struct(FRONT_END_OPTS)))
        f.write(np.asarray([0.08, 0.004, 4e-5, 2e-6], dtype=np.float64).tobytes())
        for (dt, acc, gyr), sc in zip(imus, scans):
            rows = np.concatenate([np.full((len(acc) - 1, 1), dt), acc[:-1], gyr[:-1]], axis=1)
            f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(sc[len(sc) - n:], dtype=np.float32).tobytes())
    return exe, path, scans_n


@pytest.mark.parametrize("descrew", [0, 1])
@pytest.mark.parametrize("num_accumulated", [1, 2])
def test_adapter_device_path_equals_host_path(adapter, num_accumulated, descrew):
    """two lidars' messages through SensorBridge: the same MatchingResult poses from the device synchronizer as from the
    host one, every scan merged on the device, none handed to the host, nothing downloaded"""
    import subprocess
    exe, path, scans_n = adapter
    out = subprocess.run([exe, path, str(num_accumulated), str(descrew)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RANGE SYNC ADAPTER DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    device = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("DEVICE ")]
    host = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("HOST ")]
    assert len(device) == len(host) == scans_n // num_accumulated and device == host, out.stdout[-3000:]
    assert len({tuple(p) for p in device}) == len(device)  # the sensor moved
    counters = [line.split() for line in out.stdout.splitlines() if line.startswith("COUNTERS ")][0]
    assert counters[1:] == ["device_merges", str(scans_n), "merge_host_fallbacks", "0", "merges_left_to_host", "0", "downloads", "0"], counters
    assert scans_n >= 3


def test_adapter_leaves_merges_of_column_times_to_the_host(adapter):
    """clouds without point times (every t equal; an Ouster's column times are the same case): the device's replay of
    std::sort on runs of equal times is the slower path, so the adapter downloads both clouds and
    merges on the host -- counted, and with the same poses"""
    import subprocess
    exe, path, scans_n = adapter
    out = subprocess.run([exe, path, "1", "1", "other"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RANGE SYNC ADAPTER DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    device = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("DEVICE ")]
    host = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("HOST ")]
    assert len(device) == len(host) == scans_n and device == host, out.stdout[-3000:]
    counters = [line.split() for line in out.stdout.splitlines() if line.startswith("COUNTERS ")][0]
    assert counters[1:] == ["device_merges", "0", "merge_host_fallbacks", "0", "merges_left_to_host", str(scans_n), "downloads",
                            str(2 * scans_n)], counters
