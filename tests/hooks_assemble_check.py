"""Body of tests/test_gpu_assemble.py::test_check_paths_forced_by_the_hooks_build: runs with DLIOM_LIB pointing at
libdliom_hooks.so.  Knob 2 of dliom_ctx_set_tuning = 4 makes the batch assembler record EVERY point of the sin branch (the
ring overflows: the records-only pass over all points and the full read-back run); = 5 additionally moves the device's
rotation by some float ulp for every point with an even time, so that the host's recomputation with glibc differs and
those points are redone by the fix kernel.  The result must equal the model's bit for bit in both modes."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "d-liom_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import assemble_common as ac  # noqa: E402
import dliom as dl  # noqa: E402


def fixed_point_index(times, poses, cloud_time, xyzt, kept_index):
    """A kept point that mode 5 moves on the device and the fix kernel redoes: its time is an even tick strictly inside an
    interval whose rotations differ (slerp's sin branch, |d| < 1 - epsilon), between a quarter and three quarters of the
    way -- there the hook's scale1 * (1 + 2^-20) moves the interpolated quaternion by 2^-22 of itself or more, several float
    ulp, so the device's floats differ from the host's and the point is among the fixes."""
    for i in kept_index[len(kept_index) // 3:]:
        tick = int(cloud_time) + int(np.float64(xyzt[i, 3]) * 1e7)
        j = int(np.searchsorted(times, tick, side="left"))
        if tick % 2 != 0 or j == 0 or j >= len(times) or times[j] == tick:
            continue
        factor = (tick - int(times[j - 1])) / float(int(times[j]) - int(times[j - 1]))
        d = abs(float(np.dot(poses[j - 1, 3:], poses[j, 3:])))
        if 0.25 <= factor <= 0.75 and d < 1.0 - 1e-9:
            return int(i)
    raise AssertionError("no kept point that mode 5 moves")


def check_bounds_after_forced_fixes(ctx, trajectory, times, poses, cloud_time, xyzt):
    """dliom_cloud_bounds after the forced paths (hook values 4 and 5): the records-only pass must leave the first pass's
    maximum alone, and after assemble_fix_kernel the maximum is taken again -- here the farthest point is one of the
    redone ones, so a bound left from the device's own floats would differ."""
    import cloud_bounds_common as cb
    with tempfile.TemporaryDirectory() as d:
        exe = ac.build_model(d)
        _, results = ac.run_model(exe, times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, xyzt)], d)
        far = fixed_point_index(times, poses, cloud_time, xyzt, results[0]["index"])
        moved = xyzt.copy()
        reach = np.sqrt((xyzt[:, :3].astype(np.float64) ** 2).sum(axis=1))
        moved[far, :3] *= np.float32(3.0 * reach.max() / reach[far])
        _, results = ac.run_model(exe, times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, moved)], d)
    want = results[0]
    norms = (want["xyz"].astype(np.float64) ** 2).sum(axis=1)
    assert want["index"][int(np.argmax(norms))] == far  # the farthest map-frame point is the fixed one
    for mode in (4, 5):
        ctx.set_tuning(dl.TUNE_RESERVED_TEST_HOOK, mode)
        f0 = ctx.assemble_check_stats()[2]
        cloud, origin, index = trajectory.assemble(cloud_time, moved, ac.MOUNT)
        assert (ctx.assemble_check_stats()[2] > f0) == (mode == 5)
        ac.assert_equal_bits(cloud, origin, index, want)
        max_norm, abs_max = cloud.bounds()
        ref = cb.ref_max_norm(cloud.download())
        assert cb.bits(max_norm) == cb.bits(ref), (mode, max_norm, ref)
        assert all(a < 0 or a >= np.abs(want["xyz"][:, k]).max() for k, a in enumerate(abs_max))
        cloud.close()


def main():
    assert os.environ.get("DLIOM_LIB", "").endswith("libdliom_hooks.so")
    dl.load_library()
    ctx = dl.Context(0)
    times, poses, cloud_time, xyzt = ac.drive(16, 256, 37)
    with tempfile.TemporaryDirectory() as d:
        _, results = ac.run_model(ac.build_model(d), times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, xyzt)], d)
    want = results[0]
    libm = ac.honest(want, 37) and want["libm"]
    trajectory = dl.Trajectory(ctx, times, poses)
    for mode in (4, 5):
        ctx.set_tuning(dl.TUNE_RESERVED_TEST_HOOK, mode)
        r0, c0, f0, o0 = ctx.assemble_check_stats()
        cloud, origin, index = trajectory.assemble(cloud_time, xyzt, ac.MOUNT)
        r1, c1, f1, o1 = ctx.assemble_check_stats()
        assert r1 - r0 == libm and c1 - c0 == libm and o1 == o0 + 1, (mode, r1 - r0, c1 - c0, libm, o1 - o0)
        assert (f1 - f0 > 0) if mode == 5 else (f1 == f0), (mode, f1 - f0, libm)  # mode 5: every other point was moved
        ac.assert_equal_bits(cloud, origin, index, want)
        cloud.close()
    # the last kept point among the redone ones: the origin comes from the host's floats too
    sub = xyzt[:len(xyzt) // 2]
    with tempfile.TemporaryDirectory() as d:
        _, results = ac.run_model(ac.build_model(d), times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, s) for s in (sub, sub[:-1])], d)
    for s, w in zip((sub, sub[:-1]), results):
        cloud, origin, index = trajectory.assemble(cloud_time, s, ac.MOUNT)
        ac.assert_equal_bits(cloud, origin, index, w)
        cloud.close()
    check_bounds_after_forced_fixes(ctx, trajectory, times, poses, cloud_time, xyzt)
    ctx.set_tuning(dl.TUNE_RESERVED_TEST_HOOK, 0)
    r0, c0, f0, o0 = ctx.assemble_check_stats()
    cloud, origin, index = trajectory.assemble(cloud_time, xyzt, ac.MOUNT)
    r1, c1, f1, o1 = ctx.assemble_check_stats()
    ac.assert_equal_bits(cloud, origin, index, want)
    assert o1 == o0 and f1 == f0 and r1 - r0 == c1 - c0 and r1 - r0 < len(xyzt) // 10  # the real bound: a handful, none different
    print("hooks_assemble_check ok (real bound: %d of %d points re-examined on the host)" % (r1 - r0, len(xyzt)))
    cloud.close()
    trajectory.close()
    ctx.close()


if __name__ == "__main__":
    main()
