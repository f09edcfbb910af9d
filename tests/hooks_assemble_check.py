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

import assemble_common as ac  # noqa: E402
import dliom as dl  # noqa: E402


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
