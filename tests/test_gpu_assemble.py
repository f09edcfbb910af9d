"""The batch assembler on the device (dliom_trajectory_*, dliom_cloud_from_sensor_points) against the CPU model of
HandleMessage over a TransformInterpolationBuffer (tests/cpp/assemble_model.cc).  Every comparison is exact equality:
kept_index, the cloud's bytes and the origin's bits.  The drives assert the conditions under which they compare something
(tests/assemble_common.py honest()): the scan crosses at least three intervals of the trajectory -- for the trajectories
of 2 and 3 nodes, which have one and two, every interval -- and at least 90 % of the kept points take slerp's sin / acos
branch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_common as ac  # noqa: E402
from assemble_common import EPOCH, IDENTITY, MOUNT, MOUNT_NO_TRANSLATION, TICKS, f32  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = ac.ROOT


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
    return ac.build_model(tmp_path_factory.mktemp("assemble_model"))


def check(dl, ctx, model, directory, times, poses, batches):
    """batches: [(cloud_time, mount, xyzt)] against one trajectory; -> the model's results."""
    pushed, results = ac.run_model(model, times, poses, [ac.assemble_op(*b) for b in batches], directory)
    assert pushed == 0
    trajectory = dl.Trajectory(ctx, times, poses)
    for (cloud_time, mount, xyzt), want in zip(batches, results):
        assert want["status"] == 0
        cloud, origin, index = trajectory.assemble(cloud_time, xyzt, mount)
        ac.assert_equal_bits(cloud, origin, index, want)
        if cloud is not None:
            cloud.close()
    trajectory.close()
    return results


@pytest.mark.parametrize("nodes", [2, 3, 37, 200])
@pytest.mark.parametrize("beams,azimuths", [(16, 256), (32, 512)])
def test_drives_equal_model(dl, ctx, model, tmp_path, beams, azimuths, nodes):
    times, poses, cloud_time, xyzt = ac.drive(beams, azimuths, nodes)
    before = ctx.assemble_check_stats()
    results = check(dl, ctx, model, tmp_path, times, poses, [(cloud_time, MOUNT, xyzt), (cloud_time, MOUNT_NO_TRANSLATION, xyzt)])
    for r in results:
        ac.honest(r, nodes)
    after = ctx.assemble_check_stats()
    assert after[0] - before[0] == after[1] - before[1]  # every recorded point was recomputed on the host
    assert after[0] - before[0] < len(xyzt) // 10 and after[2] == before[2]  # a handful, none of them different


def small_trajectory():
    """Five nodes 10 ms apart with rotations a few degrees apart."""
    from dliom import synth
    times = EPOCH + 100_000 * np.arange(5, dtype=np.int64)
    poses = np.array([synth.trajectory_pose(3.0 * k) for k in range(5)])
    return times, poses


def points(n, rel_ticks, seed=3):
    """n points with the relative times rel_ticks / 1e7 (cycled)."""
    rng = np.random.RandomState(seed)
    xyzt = np.zeros((n, 4), dtype=f32)
    xyzt[:, :3] = rng.uniform(-20.0, 20.0, size=(n, 3))
    if n > 0:
        xyzt[:, 3] = (np.resize(np.asarray(rel_ticks, dtype=np.float64), n) / TICKS).astype(f32)
    return xyzt


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_batch_sizes(dl, ctx, model, tmp_path, n):
    times, poses = small_trajectory()
    xyzt = points(n, -np.linspace(0.0, 390_000.0, 97))
    results = check(dl, ctx, model, tmp_path, times, poses, [(int(times[-1]), MOUNT, xyzt)])
    assert len(results[0]["index"]) == n


def test_points_outside_the_trajectory(dl, ctx, model, tmp_path):
    """None, all, only the first and only the last points outside: the origin comes from the last KEPT point."""
    times, poses = small_trajectory()
    t_end = int(times[-1])
    inside = -np.linspace(1000.0, 399_000.0, 300)
    none_kept = points(300, inside - 500_000.0)
    first_out = points(300, np.concatenate([inside[:10] - 500_000.0, inside[10:]]))
    last_out = points(300, np.concatenate([inside[:-10], np.full(10, 77.0)]))
    mixed = points(300, np.where(np.arange(300) % 3 == 0, 5000.0, inside))
    results = check(dl, ctx, model, tmp_path, times, poses, [(t_end, MOUNT, x) for x in (points(300, inside), none_kept, first_out, last_out, mixed)])
    assert [len(r["index"]) for r in results] == [300, 0, 290, 290, 200]
    assert results[3]["index"][-1] == 289 and results[3]["origin"].tobytes() != results[0]["origin"].tobytes()
    # an empty buffer has no time at all
    check(dl, ctx, model, tmp_path, [], np.zeros((0, 7)), [(t_end, MOUNT, points(65, inside))])


def test_points_on_node_times(dl, ctx, model, tmp_path):
    """Exactly on the earliest time, on the latest time and on an inner node's time; one tick beside each.  (The halves
    keep the float's rounding of t, a few hundredths of a tick here, away from the truncation.)"""
    times, poses = small_trajectory()
    rel = np.array([-400_000.5, 0.5, -200_000.5, -400_001.5, 1.5, -199_999.5, -200_001.5, -399_999.5, -1.5])
    results = check(dl, ctx, model, tmp_path, times, poses, [(int(times[-1]), MOUNT, points(9, rel)), (int(times[-1]), IDENTITY, points(9, rel))])
    assert list(results[0]["index"]) == [0, 1, 2, 5, 6, 7, 8] and results[0]["libm"] == 4


def test_duplicated_node_times_and_single_node(dl, ctx, model, tmp_path):
    times, poses = small_trajectory()
    dup = times.copy()
    dup[2] = dup[1]
    dup[3] = dup[1]
    rel = -np.linspace(0.0, 400_000.0, 401)  # every 1000 ticks: lands on the duplicated time as well
    results = check(dl, ctx, model, tmp_path, dup, poses, [(int(dup[-1]), MOUNT, points(401, rel))])
    assert len(results[0]["index"]) == 401
    # a single node: only time == node is kept
    results = check(dl, ctx, model, tmp_path, times[:1], poses[:1], [(int(times[0]), MOUNT, points(64, [0.0, -1.0, 1.0, 0.0]))])
    assert list(results[0]["index"]) == [i for i in range(64) if i % 4 in (0, 3)] and results[0]["libm"] == 0


def test_negative_time_truncates_toward_zero(dl, ctx, model, tmp_path):
    """int64(-0.99999994 ticks) = 0 (duration_cast truncates): the point is ON the latest node, not before it."""
    times, poses = small_trajectory()
    xyzt = points(4, [0.0])
    xyzt[:, 3] = [f32(-0.99e-7), f32(-1.0e-7), f32(0.99e-7), f32(-1.5e-7)]
    assert [int(np.float64(t) * 1e7) for t in xyzt[:, 3]] == [0, -1, 0, -1]
    results = check(dl, ctx, model, tmp_path, times, poses, [(int(times[-1]), MOUNT, xyzt)])
    assert list(results[0]["index"]) == [0, 1, 2, 3] and results[0]["libm"] == 2


def test_sign_flip_and_identical_rotations(dl, ctx, model, tmp_path):
    times, poses = small_trajectory()
    poses[2, 3:] = -poses[2, 3:]  # d < 0 into and out of node 2
    poses[3, 3:] = poses[4, 3:] = [0.5, 0.5, -0.5, 0.5]  # d = 1 exactly: the absD >= one branch
    rel = -np.linspace(500.0, 399_500.0, 800)
    for mount in (MOUNT, MOUNT_NO_TRANSLATION, IDENTITY):
        results = check(dl, ctx, model, tmp_path, times, poses, [(int(times[-1]), mount, points(800, rel))])
        assert len(results[0]["index"]) == 800 and 500 < results[0]["libm"] < 700


def test_refusals(dl, ctx, model, tmp_path):
    times, poses = small_trajectory()
    trajectory = dl.Trajectory(ctx, times, poses)
    good = points(100, -np.linspace(0.0, 390_000.0, 100))
    for bad in (np.nan, np.inf, -np.inf, 1e12, -1e12, 9.3e11):  # |t * 1e7| >= 2^63 = 9.22e18
        xyzt = good.copy()
        xyzt[57, 3] = bad
        _, results = ac.run_model(model, times, poses, [ac.assemble_op(int(times[-1]), MOUNT, xyzt)], tmp_path)
        assert results[0]["status"] == -1
        with pytest.raises(dl.DliomError) as e:
            trajectory.assemble(int(times[-1]), xyzt, MOUNT)
        assert e.value.status == dl.ERR_INVALID_ARGUMENT
    xyzt = good.copy()
    xyzt[57, 3] = 9.2e11  # the largest magnitude that is still defined: far outside the trajectory, dropped
    check(dl, ctx, model, tmp_path, times, poses, [(int(times[-1]), MOUNT, xyzt)])
    # a capacity too small: the count comes back, no cloud
    L = dl.load_library()
    h, kept, origin, index = C.c_void_p(), C.c_int64(), np.zeros(3, dtype=f32), np.zeros(100, dtype=np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    mount = np.array(MOUNT)
    args = (int(times[-1]), good.ctypes.data_as(fp), 100, mount.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h),
            origin.ctypes.data_as(fp), index.ctypes.data_as(ip))
    assert L.dliom_cloud_from_sensor_points(ctx.h, trajectory.h, *args, 99, C.byref(kept)) == dl.ERR_CAPACITY
    assert kept.value == 100 and not h
    assert L.dliom_cloud_from_sensor_points(ctx.h, trajectory.h, *args, -1, C.byref(kept)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_cloud_from_sensor_points(ctx.h, trajectory.h, args[0], args[1], -1, *args[3:], 100, C.byref(kept)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_cloud_from_sensor_points(ctx.h, trajectory.h, args[0], None, *args[2:], 100, C.byref(kept)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_cloud_from_sensor_points(ctx.h, None, *args, 100, C.byref(kept)) == dl.ERR_INVALID_ARGUMENT
    # a trajectory of another context, and a host-only one
    other = dl.Context(0)
    for foreign in (dl.Trajectory(other, times, poses), dl.Trajectory(None, times, poses)):
        assert L.dliom_cloud_from_sensor_points(ctx.h, foreign.h, *args, 100, C.byref(kept)) == dl.ERR_INVALID_ARGUMENT
        foreign.close()
    other.close()
    assert L.dliom_cloud_from_sensor_points(ctx.h, trajectory.h, *args, 100, C.byref(kept)) == dl.OK and kept.value == 100
    dl.PointCloud(ctx, _handle=h).close()
    trajectory.close()


def test_stages_share_the_scratch_on_one_context(dl, ctx, model, tmp_path):
    """The assembler, the range filter and the sampler carve the same scratch of the context, each to its own size: 4097
    points, then a 65-point batch filtered and sampled (0.55), then 4097 again, then 63 -- across one wavefront, one
    workgroup and 4096.  Every result is the model's, and the two 4097-point results are equal."""
    import points_batch_common as pb
    times, poses = small_trajectory()
    t_end = int(times[-1])

    def message(n):  # every third point lies outside the trajectory
        inside = -np.linspace(1000.0, 399_000.0, n)
        return points(n, np.where(np.arange(n) % 3 == 0, 5000.0, inside), seed=n)

    big, small = message(4097), message(63)
    pushed, (want_big, want_small) = ac.run_model(model, times, poses, [ac.assemble_op(t_end, MOUNT, big), ac.assemble_op(t_end, MOUNT, small)], tmp_path)
    assert pushed == 0 and len(want_big["index"]) == 4097 - 1366 and len(want_small["index"]) == 42
    # the batch: the kept points lie 10 m from the origin, the others 30 m
    batch_model = pb.build_model(tmp_path)
    pts, it, col = pb.batch_arrays(65, 65, "both")
    keep = np.arange(65) % 2 == 0
    d = np.random.RandomState(65).normal(size=(65, 3)) + 1e-3
    pts = (d / np.linalg.norm(d, axis=1)[:, None] * np.where(keep, 10.0, 30.0)[:, None]).astype(f32)
    filtered, (pulses, _, _) = pb.run_model(batch_model, [pb.remove_op(pts, it, col, keep), pb.pulse_op(0.55, 0, 0, 33)], tmp_path)
    assert len(filtered[0]) == 33 and 0 < int(np.sum(pulses)) < 33
    sampled, = pb.run_model(batch_model, [pb.remove_op(*filtered, pulses)], tmp_path)

    trajectory = dl.Trajectory(ctx, times, poses)
    first = trajectory.assemble(t_end, big, MOUNT)
    ac.assert_equal_bits(*first, want_big)
    b = dl.PointsBatch(ctx, pts, (0, 0, 0), it, col)
    b.min_max_range_filter(5.0, 20.0)
    pb.assert_batch_equals(b, filtered)
    sampler = dl.FixedRatioSampler(0.55)
    b.fixed_ratio_sample(sampler)
    pb.assert_batch_equals(b, sampled)
    sampler.close()
    b.close()
    again = trajectory.assemble(t_end, big, MOUNT)
    ac.assert_equal_bits(*again, want_big)
    assert again[0].download().tobytes() == first[0].download().tobytes() and again[1].tobytes() == first[1].tobytes()
    assert np.array_equal(again[2], first[2])
    last = trajectory.assemble(t_end, small, MOUNT)
    ac.assert_equal_bits(*last, want_small)
    for cloud in (first[0], again[0], last[0]):
        cloud.close()
    trajectory.close()


def assembler_round_trips(dl, ctx):
    """-> (read-backs, synchronisations) of one warm 4097-point dliom_cloud_from_sensor_points without a kept_index buffer,
    and the same with one."""
    times, poses = small_trajectory()
    trajectory = dl.Trajectory(ctx, times, poses)
    xyzt = points(4097, -np.linspace(0.0, 390_000.0, 97))
    L = dl.load_library()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    mount, origin, index = np.array(MOUNT), np.zeros(3, dtype=f32), np.zeros(4097, dtype=np.int32)
    out = []
    for kept_index in (None, index.ctypes.data_as(ip), None, index.ctypes.data_as(ip)):  # (the first two calls warm up)
        h, kept = C.c_void_p(), C.c_int64()
        r0, s0 = ctx.read_backs(), ctx.synchronizations()
        status = L.dliom_cloud_from_sensor_points(ctx.h, trajectory.h, int(times[-1]), xyzt.ctypes.data_as(fp), 4097,
                                                  mount.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h),
                                                  origin.ctypes.data_as(fp), kept_index, 4097, C.byref(kept))
        out.append((ctx.read_backs() - r0, ctx.synchronizations() - s0))
        assert status == dl.OK and kept.value == 4097
        dl.PointCloud(ctx, _handle=h).close()
    trajectory.close()
    return out[2], out[3]


def test_round_trips_of_a_call(dl, ctx):
    """One polled read-back a call; the download of kept_index, when asked for, is one stream synchronisation more
    (DESIGN.md section 3.13), with the compaction shared among the export stages as before it was."""
    without_index, with_index = assembler_round_trips(dl, ctx)
    assert without_index == (1, 0)
    assert with_index == (1, 1)


def test_adapter_chain_equals_model(dl, model, tmp_path):
    """transform::TransformInterpolationBuffer and io::AssemblePointsBatch -> MinMaxRangeFiteringPointsProcessor ->
    OutlierRemovingPointsProcessor's marks (tests/cpp/assemble_adapter.cc): the assembled batch is the model's, the chain
    behind it marks the voxels that the same batch marks when it is uploaded from the host, and it uploads nothing."""
    exe = str(tmp_path / "assemble_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "assemble_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    times, poses, cloud_time, xyzt = ac.drive(16, 256, 3)
    _, results = ac.run_model(model, times, poses, [ac.assemble_op(cloud_time, MOUNT, xyzt), ac.lookup_op(times[:1])], tmp_path)
    want = results[0]
    kept = ac.honest(want, 3)
    assert kept < len(xyzt)
    src, dst = str(tmp_path / "message.bin"), str(tmp_path / "adapter_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(times)], dtype=np.int64).tobytes() + times.tobytes() + poses.tobytes())
        f.write(np.array([cloud_time], dtype=np.int64).tobytes() + np.array(MOUNT).tobytes())
        f.write(np.array([len(xyzt)], dtype=np.int64).tobytes() + xyzt.tobytes())
    out = subprocess.run([exe, src, dst, "0.1", "1.0", "18.0"], timeout=300)
    assert out.returncode == 0
    data = open(dst, "rb").read()
    n = int(np.frombuffer(data, dtype=np.int64, count=1)[0])
    assert n == kept
    at = 8
    assert data[at:at + 12 * n] == want["xyz"].tobytes()
    at += 12 * n
    assert np.array_equal(np.frombuffer(data, dtype=f32, count=n, offset=at), want["index"].astype(f32))  # intensity = index
    at += 4 * n
    assert data[at:at + 12] == want["origin"].tobytes()
    assert int(np.frombuffer(data, dtype=np.int64, count=1, offset=at + 12)[0]) == cloud_time
    at += 20
    chains = []
    for _ in range(2):
        uploads, voxels = (int(v) for v in np.frombuffer(data, dtype=np.int64, count=2, offset=at))
        chains.append((uploads, data[at + 16:at + 16 + 16 * voxels]))
        assert voxels > 100
        at += 16 + 16 * voxels
    assert chains[0][0] == 0 and chains[1][0] == 1  # the assembled batch is on the device; the copy is uploaded once
    assert chains[0][1] == chains[1][1]
    assert list(np.frombuffer(data, dtype=np.int32, count=4, offset=at)) == [0, 1, 1, 0]
    assert data[at + 16:at + 72] == results[1][1][0].tobytes()
    assert at + 72 == len(data)
    # the range filter did something: the voxels are those of the model's points within [1, 18] m of the origin
    r = np.linalg.norm(want["xyz"] - want["origin"], axis=1)
    assert 0.3 < np.mean((r >= 1.0) & (r <= 18.0)) < 0.9


def test_randomised_slice(dl, ctx, model, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_assemble
    for seed in range(1, 41):
        fuzz_assemble.run_case(dl, ctx, model, seed, str(tmp_path))


def test_check_paths_forced_by_the_hooks_build(dl):
    """The rare paths in a process of its own with libdliom_hooks.so (tests/hooks_assemble_check.py): every point recorded
    (the ring overflows), and the device's rotation perturbed so that recorded points are recomputed and redone."""
    assert os.path.exists(dl.HOOKS_LIB_PATH), "libdliom_hooks.so not built (make -C d-liom_amd hooks)"
    env = dict(os.environ, DLIOM_LIB=dl.HOOKS_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hooks_assemble_check.py")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hooks_assemble_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
