#!/usr/bin/env python3
"""Randomised differential test of the device batch assembler (dliom_trajectory_*, dliom_cloud_from_sensor_points)
against the CPU model (tests/cpp/assemble_model.cc).  Each case (tests/assemble_common.py random_case) draws a
trajectory of 1 to 60 nodes with duplicated times, large and small rotation steps, sign flips and identical rotations, a
mount with or without a translation, and 1 to 3000 points whose times overhang the trajectory and sometimes fall exactly
on a node; kept_index, the cloud's bytes and the origin's bits are compared, all exactly.
tests/test_gpu_assemble.py runs seeds 1-40; `--soak SECONDS` keeps drawing cases (one process, one GPU)."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import assemble_common as ac  # noqa: E402


def run_case(dl, ctx, model, seed, directory):
    times, poses, cloud_time, mount, xyzt = ac.random_case(seed)
    pushed, results = ac.run_model(model, times, poses, [ac.assemble_op(cloud_time, mount, xyzt)], directory)
    assert pushed == 0 and results[0]["status"] == 0
    trajectory = dl.Trajectory(ctx, times, poses)
    cloud, origin, index = trajectory.assemble(cloud_time, xyzt, mount)
    ac.assert_equal_bits(cloud, origin, index, results[0])
    if cloud is not None:
        cloud.close()
    trajectory.close()
    return "seed %d: %d nodes, %d points, %d kept, %d on the sin branch" % (seed, len(times), len(xyzt), len(index),
                                                                        results[0]["libm"])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--seeds", type=int, nargs="*", default=list(range(1, 101)))
    ap.add_argument("--soak", type=float, default=0.0, help="seconds to keep drawing cases after --seeds")
    args = ap.parse_args()
    import dliom as dl
    ctx = dl.Context(0)
    with tempfile.TemporaryDirectory() as d:
        model = ac.build_model(d)
        t0, seed, done = time.time(), 0, 0
        for seed in args.seeds:
            print(run_case(dl, ctx, model, seed, d), flush=True)
            done += 1
        while time.time() - t0 < args.soak:
            seed += 1
            print(run_case(dl, ctx, model, seed, d), flush=True)
            done += 1
    print("fuzz_assemble: %d cases equal; recorded / recomputed / fixed / ring overflows: %s" % (done, ctx.assemble_check_stats()))
    ctx.close()


if __name__ == "__main__":
    main()
