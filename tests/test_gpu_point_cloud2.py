"""PointCloud2 messages decoded on the device (dliom_point_cloud2_decode and the two consumers of a dliom_timed_cloud)
against the models of tests/point_cloud2_common.py.  Every comparison is exact equality of bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_common as ac  # noqa: E402
import point_cloud2_common as pc  # noqa: E402

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


def decode(dl, ctx, m, mode, tf=None):
    """the device's result shaped like the model's; a refusal comes back as its status"""
    try:
        cloud, time, origin = m.to_library(dl).decode(ctx, mode, tf)
    except dl.DliomError as e:
        return {"status": e.status}
    xyzt, it = cloud.download()
    assert len(cloud) == len(xyzt) and cloud.has_intensities == (it is not None)
    front, back = cloud.front_back_time()
    cloud.close()
    return {"status": pc.OK, "xyzt": xyzt, "intensities": it, "time": time, "origin": origin, "front": front, "back": back}


def check(dl, ctx, m, mode, tf=None, what=""):
    want = pc.model_decode(m, mode, tf)
    pc.assert_equal_results(decode(dl, ctx, m, mode, tf), want, what)
    return want


def shapes_of(n):
    """(height, width, point_step, row_pad) a size is run in: one row in each record size (22 bytes among them), and
    where n allows rows of a padded row_step whose ends fall inside a workgroup's 256 points"""
    shapes = [(1, n, step, 0) for step in (None, 22, 26, 32, 48)]
    if n % 4 == 0:
        shapes += [(4, n // 4, 22, 7), (4, n // 4, 48, 40)]
    if n % 10 == 0:
        shapes.append((n // 10, 10, 26, 3))  # 26 rows to a workgroup
    if n == 4099:
        shapes.append((4099 // 7, 7, 32, 1))  # (4095 points: the odd width puts every row end at another lane)
    return shapes


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1000, 4099])
@pytest.mark.parametrize("mode", pc.MODES)
def test_every_mode_and_size_equals_model(dl, ctx, mode, n):
    kept_all = 0
    for k, (height, width, step, row_pad) in enumerate(shapes_of(n)):
        if step is not None and step < pc.smallest_step(mode):
            step = 32  # (Robosense's fields need 21 bytes, ...)
        m = pc.make_message(1000 * mode + 10 * n + k, mode, height, width, step, row_pad=row_pad, with_intensity=not (mode == pc.EXPORT and k == 1))
        want = check(dl, ctx, m, mode, pc.MOUNT if k % 2 else None, (mode, n, height, width, step, row_pad))
        assert len(want["xyzt"]) == height * width
        kept_all += 1
    assert kept_all >= 5


def test_long_records_take_the_words_from_global_memory(dl, ctx):
    """records of 200 bytes do not fit the LDS span of 256 points: the second kernel, same words, same result"""
    for mode in (pc.VELODYNE, pc.ROBOSENSE, pc.EXPORT_RSLIDAR):
        for height, width, row_pad in ((1, 700, 0), (3, 259, 5)):
            m = pc.make_message(77 + mode, mode, height, width, 200, row_pad=row_pad)
            pc.set_values(m, {"y": np.inf}, [0, 5, 699])
            want = check(dl, ctx, m, mode, pc.MOUNT if mode in pc.SLAM_MODES else None)  # (kept infinities are only copied)
            assert len(want["xyzt"]) == height * width - (3 if mode in pc.SLAM_MODES else 0)


@pytest.mark.parametrize("mode", pc.MODES)
def test_dropping(dl, ctx, mode):
    n = 700
    slam = mode in pc.SLAM_MODES

    def message(seed=mode):
        return pc.make_message(seed, mode, 1, n, 22 if mode != pc.ROBOSENSE else 32)

    # each value in each coordinate; the first point; the last one (rel_time_last still comes from it)
    m = message()
    k = 10
    for c in "xyz":
        for v in (np.nan, np.inf, -np.inf):
            pc.set_values(m, {c: v}, k)
            k += 37
    pc.set_values(m, {"x": np.nan}, 0)
    pc.set_values(m, {"z": -np.inf}, n - 1)
    want = check(dl, ctx, m, mode, None, "single points")
    assert len(want["xyzt"]) == (n - 11 if slam else n)
    if mode in pc.TIME_FIELD:
        assert want["back"] != 0 and want["rel_time_last"] != 0  # the last kept point is not the message's last
    # runs of dropped points across the 256 boundaries, and a kept point alone between two runs
    m = message(mode + 10)
    run = np.r_[250:262, 263:300, 505:520]
    pc.set_values(m, {"y": np.nan}, run)
    # (the export modes keep these points; they get no frame change here, as in use: arithmetic on a NaN or an infinity
    # gives a NaN whose sign and payload IEEE 754 leaves to the machine, and only copies of the message's bits are compared)
    mount = pc.MOUNT if slam else None
    want = check(dl, ctx, m, mode, mount, "runs")
    assert len(want["xyzt"]) == (n - len(run) if slam else n)
    # everything dropped: an empty object, not a refusal
    m = message(mode + 20)
    pc.set_values(m, {"x": np.inf})
    want = check(dl, ctx, m, mode, mount, "all")
    assert want["status"] == pc.OK and len(want["xyzt"]) == (0 if slam else n)
    if slam:
        cloud, time, origin = m.to_library(dl).decode(ctx, mode, pc.MOUNT)
        assert len(cloud) == 0 and cloud.front_back_time() == (0, 0) and time == want["time"]
        with pytest.raises(dl.DliomError) as e:
            cloud.add_range_data(ac.IDENTITY, ac.IDENTITY, 0.1, (0, 0, 0), 1.0, 50.0, 0.15)
        assert e.value.status == dl.ERR_EMPTY_CLOUD
        cloud.close()


def test_empty_message(dl, ctx):
    for mode in (pc.OTHER, pc.EXPORT, pc.EXPORT_RSLIDAR):
        m = pc.make_message(3, mode, 0, 5)
        want = check(dl, ctx, m, mode)
        assert want["status"] == pc.OK and len(want["xyzt"]) == 0
    assert decode(dl, ctx, pc.make_message(3, pc.VELODYNE, 0, 5), pc.VELODYNE)["status"] == dl.ERR_INVALID_ARGUMENT


def test_transform(dl, ctx):
    for mode in (pc.OUSTER, pc.EXPORT):
        m = pc.make_message(40 + mode, mode, 2, 333, 48)
        plain = check(dl, ctx, m, mode, None)
        moved = check(dl, ctx, m, mode, pc.MOUNT)
        q = pc.MOUNT[3:].astype(f32)
        assert abs(float(np.dot(q.astype(np.float64), q.astype(np.float64))) - 1.0) > 1e-6  # cast as it is, not normalised
        assert pc.same_bits(plain["origin"], np.zeros(3)) and pc.same_bits(moved["origin"], pc.MOUNT[:3].astype(f32))
        assert pc.same_bits(plain["xyzt"][:, 3], moved["xyzt"][:, 3]) and not pc.same_bits(plain["xyzt"][:, :3], moved["xyzt"][:, :3])
        # a rotation (nearly: |q| is 0.999) and the translation: lengths about the mount's origin stay within 0.5 %
        before = np.linalg.norm(plain["xyzt"][:, :3].astype(np.float64), axis=1)
        after = np.linalg.norm(moved["xyzt"][:, :3].astype(np.float64) - pc.MOUNT[:3], axis=1)
        assert np.abs(after / before - 1.0).max() < 5e-3
    with pytest.raises(dl.DliomError):
        m.to_library(dl).decode(ctx, pc.EXPORT, np.array([0, 0, np.nan, 1, 0, 0, 0.0]))


def test_bad_time(dl, ctx):
    import ctypes as C
    m = pc.make_message(50, pc.VELODYNE, 1, 600, 22)
    pc.set_values(m, {"time": np.nan}, 300)
    assert pc.model_decode(m, pc.VELODYNE)["status"] == pc.INVALID
    lib = m.to_library(dl)
    h, t, o = C.c_void_p(), C.c_int64(), np.zeros(3, f32)
    status = ctx._L.dliom_point_cloud2_decode(ctx.h, C.byref(lib.struct), pc.VELODYNE, None, C.byref(h), C.byref(t),
                                              o.ctypes.data_as(C.POINTER(C.c_float)))
    assert status == dl.ERR_INVALID_ARGUMENT and not h  # *out stays NULL
    pc.set_values(m, {"x": np.nan}, 300)  # the same time on a dropped point is nobody's
    want = check(dl, ctx, m, pc.VELODYNE)
    assert want["status"] == pc.OK and len(want["xyzt"]) == 599
    # a time whose ticks do not fit: Robosense stamps 1e12 s apart
    r = pc.make_message(51, pc.ROBOSENSE, 1, 300, 32)
    pc.set_values(r, {"timestamp": 1.6e9 - 1e12}, 17)
    assert check(dl, ctx, r, pc.ROBOSENSE)["status"] == pc.INVALID


def _scan_case(beams, azimuths, k):
    from dliom import synth
    prev, cur = synth.trajectory_pose(0.1 * (k - 1)), synth.trajectory_pose(0.1 * k)
    pts, rel_t = synth.scan(cur, beams, azimuths)
    return prev, cur, pts, rel_t


@pytest.mark.parametrize("mode,beams,azimuths,k", [(pc.VELODYNE, 16, 512, 7), (pc.OUSTER, 64, 1024, 11)])
def test_front_end_equals_host_array_path(dl, ctx, mode, beams, azimuths, k):
    prev, cur, pts, rel_t = _scan_case(beams, azimuths, k)
    height = len(pts) // azimuths
    assert height >= beams // 2
    m = pc.scan_message(mode, pts, rel_t, height, azimuths)
    cloud, time, origin = m.to_library(dl).decode(ctx, mode, pc.MOUNT)
    xyzt, _ = cloud.download()
    want = pc.model_decode(m, mode, pc.MOUNT)
    assert pc.same_bits(xyzt, want["xyzt"]) and len(xyzt) == height * azimuths and time == want["time"]
    assert xyzt[-1, 3] == 0 and xyzt[0, 3] < -0.05  # a scan's worth of de-skew
    vfs, min_r, max_r, T = 0.15, 1.0, 100.0, 0.1
    before = ctx.read_backs()
    host_cloud, host_origin, host_pose = dl.add_range_data(ctx, prev, cur, T, xyzt, origin, min_r, max_r, vfs)
    host_read_backs = ctx.read_backs() - before
    cloud.close()
    before = ctx.read_backs()
    cloud, _, origin2 = m.to_library(dl).decode(ctx, mode, pc.MOUNT)
    got_cloud, got_origin, got_pose = cloud.add_range_data(prev, cur, T, origin2, min_r, max_r, vfs)
    new_read_backs = ctx.read_backs() - before
    a, b = got_cloud.download(), host_cloud.download()
    assert len(b) > 1000 and pc.same_bits(a, b)
    assert pc.same_bits(got_origin, host_origin) and pc.same_bits(got_pose, host_pose)
    assert new_read_backs <= host_read_backs + 1, (new_read_backs, host_read_backs)
    for c in (cloud, got_cloud, host_cloud):
        c.close()


@pytest.mark.parametrize("nodes", [3, 37])
def test_export_equals_host_array_path(dl, ctx, nodes):
    times, poses, cloud_time, xyzt = ac.drive(16, 256, nodes)
    n = len(xyzt)
    trajectory = dl.Trajectory(ctx, times, poses)
    for mode, with_intensity in ((pc.VELODYNE, False), (pc.EXPORT, True), (pc.EXPORT_RSLIDAR, True)):
        if mode == pc.VELODYNE:  # times that select: the message carries the scan's own
            m = pc.scan_message(pc.VELODYNE, xyzt[:, :3], xyzt[:, 3], 1, n)
            shift = 0
        else:  # t = 0 for every point: all of them at cloud_time
            m = pc.make_message(60 + mode, mode, 1, n, 32)
            pc.set_values(m, {"x": xyzt[:, 0], "y": xyzt[:, 1], "z": xyzt[:, 2]})
            shift = -int(0.03 * ac.TICKS)
        cloud, _, _ = m.to_library(dl).decode(ctx, mode, None)
        pts, it = cloud.download()
        assert (it is not None) == with_intensity
        if mode == pc.VELODYNE:
            assert pc.same_bits(pts[:, :3], xyzt[:, :3]) and np.abs(pts[:, 3] - xyzt[:, 3]).max() < 1e-6
        want = dl.PointsBatch.from_sensor_points(trajectory, cloud_time + shift, pts, ac.MOUNT, it)
        got = cloud.to_points_batch(trajectory, cloud_time + shift, ac.MOUNT)
        assert want is not None and got is not None and 0 < len(want) <= n
        (wp, wi, _), (gp, gi, _) = want.download(), got.download()
        assert pc.same_bits(gp, wp) and pc.same_bits(got.origin, want.origin)
        assert (gi is None) == (wi is None) == (not with_intensity)
        if with_intensity:
            assert pc.same_bits(gi, wi)
        if mode == pc.VELODYNE and nodes == 3:
            assert len(want) < n  # the scan overhangs the short trajectory: the assembler drops, the intensities follow
        cloud.close()
    # nothing kept: NULL from both
    cloud, _, _ = m.to_library(dl).decode(ctx, pc.EXPORT_RSLIDAR, None)
    assert cloud.to_points_batch(trajectory, cloud_time + 100 * ac.TICKS, ac.MOUNT) is None
    assert dl.PointsBatch.from_sensor_points(trajectory, cloud_time + 100 * ac.TICKS, cloud.download()[0], ac.MOUNT) is None
    cloud.close()
    trajectory.close()


def test_adapter_equals_host_decoded_ranges(dl, tmp_path):
    """tests/cpp/point_cloud2_adapter.cc: three scans through SensorBridge::HandlePointCloud2Message into
    LocalTrajectoryBuilder3D, and the same scans decoded on the host into the existing AddRangeData: equal poses."""
    exe = str(tmp_path / "point_cloud2_adapter")
    libdir = os.path.join(pc.ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(pc.ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", exe, os.path.join(pc.ROOT, "tests", "cpp", "point_cloud2_adapter.cc"),
                           os.path.join(pc.ROOT, "tests", "cpp", "point_cloud2_model.cc"), "-DPOINT_CLOUD2_MODEL_NO_MAIN",
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    import struct
    from dliom import synth
    from test_gpu_parity import FRONT_END_OPTS
    T, scans_n = 0.1, 3
    centers = synth.bubbles()
    st = synth.trajectory_state(0.0)
    scans = [synth.moving_scan(T * k, 16, 256, centers) for k in range(1, scans_n + 1)]
    imus = [synth.imu_samples(T * (k - 1), T * k, 200.0) for k in range(1, scans_n + 1)]
    n = min(len(sc) for sc in scans)
    path = str(tmp_path / "stream.bin")
    with open(path, "wb") as f:  # (the stream file of tests/cpp/ltb3d_adapter.cc)
        f.write(struct.pack("4i", scans_n, n, len(imus[0][1]) - 1, 1))
        f.write(np.asarray(st, dtype=np.float64).tobytes())
        f.write(bytes(dl.front_end_options_struct(FRONT_END_OPTS)))
        f.write(np.asarray([0.08, 0.004, 4e-5, 2e-6], dtype=np.float64).tobytes())
        for (dt, acc, gyr), sc in zip(imus, scans):
            rows = np.concatenate([np.full((len(acc) - 1, 1), dt), acc[:-1], gyr[:-1]], axis=1)
            f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(sc[len(sc) - n:], dtype=np.float32).tobytes())
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "POINT CLOUD2 ADAPTER DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    device = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("DEVICE ")]
    host = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("HOST ")]
    assert len(device) == len(host) == 3 and device == host, out.stdout[-3000:]
    assert len({tuple(p) for p in device}) == 3  # the sensor moved
