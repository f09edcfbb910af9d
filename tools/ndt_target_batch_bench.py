"""K NDT targets built by a serial loop of dliom_ndt_target_create against one dliom_ndt_target_create_batch, in one process.
The K distinct target clouds are those tools/ndt_batch_bench.py aligns to: the scans at trajectory_pose(0.30 + 0.01 k) of the
cube and the ground, 64 x 1024, raw (the ground-truth tool) and filtered by the approximate voxel grid at 0.2 m.  The two are
checked equal first (every cell's bytes, the counts, the device table's size).  Then one warm-up of each and --repeats
alternating repetitions; a host clock around calls that end in a stream synchronisation; medians.  A line of JSON a case: ms a
call and targets/s of both, read-backs, the batch's stage split from one more, profiled call, and the share of the tool's loop
(build the K targets, then one dliom_ndt_align_batch over K pairs, clamped steps) that the build takes, serial and batched.
usage: python tools/ndt_target_batch_bench.py [--scenes cube ground] [--targets 1 4 16 64] [--repeats 5] [--leaf 0.2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
import dliom as dl  # noqa: E402
from dliom import synth  # noqa: E402

STAGES = ("sort_ms", "sums_ms", "host_ms", "upload_ms")
HEADER = """# python tools/ndt_target_batch_bench.py
# one MI355X, one process; medians of alternating repetitions of a serial loop of dliom_ndt_target_create and one
# dliom_ndt_target_create_batch over the same K clouds, after the two were checked equal byte for byte; batch_over_serial < 1: the
# batch is faster; build_share: the build / (the build + one dliom_ndt_align_batch of K pairs on those targets, clamped steps)
"""


def scans(scene, beams, azimuths, count):
    out = []
    for k in range(count):
        with synth.scene(scene, trajectory=False):
            out.append((synth.scan(synth.trajectory_pose(0.30 + 0.01 * k), beams, azimuths)[0],
                        synth.scan(synth.trajectory_pose(0.35 + 0.01 * k), beams, azimuths)[0]))
    return out


def upload(ctx, points, leaf):
    cloud = dl.PointCloud(ctx, points)
    if leaf <= 0.0:
        return cloud
    filtered = dl.approximate_voxel_filter(ctx, cloud, leaf)
    cloud.close()
    return filtered


def close_all(things):
    for t in things:
        t.close()


def serial(ctx, clouds, options):
    return [dl.NdtTarget(ctx, c, options) for c in clouds]


def check_equal(single, batched):
    for i, (a, b) in enumerate(zip(single, batched)):
        ca, cb = a.cells(), b.cells()
        for k in ca:
            if ca[k].tobytes() != cb[k].tobytes():
                raise SystemExit("target %d: %s differs between the serial loop and the batch" % (i, k))
        ma, mb = a.memory_stats(), b.memory_stats()
        for k in ("points", "kept_points", "cells", "valid_cells", "target_bytes"):
            if ma[k] != mb[k]:
                raise SystemExit("target %d: %s differs: %r and %r" % (i, k, ma[k], mb[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "ground"])
    ap.add_argument("--size", default="64x1024")
    ap.add_argument("--targets", nargs="+", type=int, default=[1, 4, 16, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.2, help="leaf of the filtered case's approximate voxel grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_target_batch_bench.txt"))
    args = ap.parse_args()
    beams, azimuths = (int(v) for v in args.size.split("x"))
    ctx = dl.Context(0)
    options = dl.ndt_options()
    limits = dl.ndt_target_batch_default_limits(max_targets_in_flight=max(1, min(max(args.targets), dl.NDT_TARGET_BATCH_MAX_TARGETS)))
    align_limits = dl.ndt_batch_default_limits(max_pairs_in_flight=max(1, min(max(args.targets), dl.NDT_BATCH_MAX_PAIRS)))
    lines = []
    for scene in args.scenes:
        host = scans(scene, beams, azimuths, max(args.targets))
        for leaf in (0.0, args.leaf):
            targets = [upload(ctx, t, leaf) for t, _ in host]
            sources = [upload(ctx, s, leaf) for _, s in host]
            indices = [dl.NnIndex(ctx, c) for c in targets]
            for count in args.targets:
                clouds = targets[:count]
                single = serial(ctx, clouds, options)  # warm-ups
                batched, stats = dl.ndt_targets_batch(ctx, clouds, options, limits)
                check_equal(single, batched)
                close_all(single)
                serial_ms, batch_ms, align_ms = [], [], []
                pairs = [(batched[k], sources[k], None, indices[k]) for k in range(count)]
                dl.ndt_align_batch(ctx, pairs, options, align_limits)  # warm-up
                for _ in range(args.repeats):  # alternating: both see the same neighbours on the machine
                    t = time.perf_counter()
                    built = serial(ctx, clouds, options)
                    serial_ms.append((time.perf_counter() - t) * 1e3)
                    close_all(built)
                    t = time.perf_counter()
                    built, _ = dl.ndt_targets_batch(ctx, clouds, options, limits)
                    batch_ms.append((time.perf_counter() - t) * 1e3)
                    close_all(built)
                    t = time.perf_counter()
                    dl.ndt_align_batch(ctx, pairs, options, align_limits)
                    align_ms.append((time.perf_counter() - t) * 1e3)
                ctx.set_profiling(1)
                timed_single = serial(ctx, clouds, options)
                timed, staged = dl.ndt_targets_batch(ctx, clouds, options, limits)
                ctx.set_profiling(0)
                single_build_ms = sum(t.memory_stats()["build_ms"] for t in timed_single)
                single_read_backs = sum(t.memory_stats()["read_backs"] for t in timed_single)
                close_all(timed_single + timed + batched)
                s, b, a = statistics.median(serial_ms), statistics.median(batch_ms), statistics.median(align_ms)
                line = json.dumps(dict(
                    scene=scene, scan=args.size, leaf=leaf, targets=count, points=int(np.mean([c.n for c in clouds])),
                    cells=stats["cells"], valid_cells=stats["valid_cells"], results_equal=True, serial_ms=s, batch_ms=b,
                    batch_over_serial=b / s, serial_ms_calls=serial_ms, batch_ms_calls=batch_ms, serial_targets_per_s=count / s * 1e3,
                    batch_targets_per_s=count / b * 1e3, serial_ms_per_target=s / count, batch_ms_per_target=b / count,
                    serial_read_backs=single_read_backs, batch_read_backs=stats["read_backs"], batch_chunks=stats["chunks"],
                    batch_synchronizations=stats["synchronizations"], scratch_bytes=stats["scratch_bytes"],
                    serial_profiled_build_ms=single_build_ms, batch_stages_ms={k: staged[k] for k in STAGES}, align_batch_ms=a,
                    serial_build_share=s / (s + a), batch_build_share=b / (b + a)))
                print(line, flush=True)
                lines.append(line)
            close_all(indices + targets + sources)
    ctx.close()
    with open(args.out, "w") as f:
        f.write(HEADER + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
