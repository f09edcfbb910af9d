"""K scan pairs aligned by a serial loop of dliom_ndt_align against one dliom_ndt_align_batch, in one process.  Scenes and
sizes as in tools/ndt_bench.py (cube and ground, 64 x 1024), raw (the ground-truth tool) and filtered by the approximate
voxel grid at 0.2 m (a few thousand points, where launches and read-backs dominate), both step modes; pair k is the scan at
trajectory_pose(0.30 + 0.01 k) (target) and the one at trajectory_pose(0.35 + 0.01 k) (source), each pair with a target and
a fitness index of its own, as the ground-truth tool's constraints have; the tool's settings.  The two are checked equal,
bit for bit, before anything is timed.  Then one warm-up of each and --repeats alternating repetitions; a host clock around
calls that end in the read-back of their last round; medians.  A line of JSON a case: pairs/s and ms a pair of both, steps
and read-backs, the batch's evaluation launches by kind and mixed steps, its stage split from one more, profiled call (the
serial loop's split is the sum of its results'), and the share of the tool's loop (build the K distinct targets, then one
batched call) that dliom_ndt_target_create takes.
usage: python tools/ndt_batch_bench.py [--scenes cube ground] [--pairs 1 4 16 64] [--repeats 5] [--leaf 0.2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
import ndt_batch_common as bc  # noqa: E402
import dliom as dl  # noqa: E402
from dliom import synth  # noqa: E402

SERIAL_STAGES = ("evaluate_ms", "reduce_ms", "host_ms")
BATCH_STAGES = ("evaluate_ms", "reduce_ms", "fitness_ms", "host_ms")
HEADER = """# python tools/ndt_batch_bench.py
# one MI355X, one process; medians of alternating repetitions of a serial loop of dliom_ndt_align (with the fitness index) and one
# dliom_ndt_align_batch over the same pairs, after the two were checked equal bit for bit; batch_over_serial < 1: the batch is faster;
# target_build_share: dliom_ndt_target_create of the K targets / (that + the batched call)
"""


def make_pairs(ctx, scene, beams, azimuths, count, leaf, options):
    """-> (pairs for ndt_align_batch, the target clouds (kept for the build's timing), what to close)"""
    pairs, targets, owned = [], [], []
    for k in range(count):
        with synth.scene(scene, trajectory=False):
            target = synth.scan(synth.trajectory_pose(0.30 + 0.01 * k), beams, azimuths)[0]
            source = synth.scan(synth.trajectory_pose(0.35 + 0.01 * k), beams, azimuths)[0]
        clouds = [dl.PointCloud(ctx, target), dl.PointCloud(ctx, source)]
        if leaf > 0.0:
            filtered = [dl.approximate_voxel_filter(ctx, c, leaf) for c in clouds]
            for c in clouds:
                c.close()
            clouds = filtered
        ndt_target, index = dl.NdtTarget(ctx, clouds[0], options), dl.NnIndex(ctx, clouds[0])
        owned += [ndt_target, index, clouds[0], clouds[1]]
        targets.append(clouds[0])
        pairs.append((ndt_target, clouds[1], None, index))
    return pairs, targets, owned


def serial(pairs, options):
    return [dl.Ndt(target, options, fitness_index=index).align(source) for target, source, _, index in pairs]


def build_ms(ctx, clouds, options):
    t = time.perf_counter()
    built = [dl.NdtTarget(ctx, c, options) for c in clouds]
    took = (time.perf_counter() - t) * 1e3
    for b in built:
        b.close()
    return took


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "ground"])
    ap.add_argument("--size", default="64x1024")
    ap.add_argument("--pairs", nargs="+", type=int, default=[1, 4, 16, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.2, help="leaf of the filtered case's approximate voxel grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndt_batch_bench.txt"))
    args = ap.parse_args()
    beams, azimuths = (int(v) for v in args.size.split("x"))
    ctx = dl.Context(0)
    limits = dl.ndt_batch_default_limits(max_pairs_in_flight=max(1, min(max(args.pairs), dl.NDT_BATCH_MAX_PAIRS)))
    lines = []
    for scene in args.scenes:
        for leaf in (0.0, args.leaf):
            all_pairs, all_targets, owned = make_pairs(ctx, scene, beams, azimuths, max(args.pairs), leaf, dl.ndt_options())
            for mode, mode_name in ((dl.NDT_STEP_CLAMPED, "clamped"), (dl.NDT_STEP_MORE_THUENTE, "more_thuente")):
                options = dl.ndt_options(step_mode=mode)
                for count in args.pairs:
                    pairs = all_pairs[:count]
                    single = serial(pairs, options)  # warm-up of the loop: every target reserves its scratch
                    batched, stats = dl.ndt_align_batch(ctx, pairs, options, limits)  # warm-up of the batch
                    differing = [(i, bc.same_result(b, s, read_backs=False)) for i, (b, s) in enumerate(zip(batched, single))
                                 if bc.same_result(b, s, read_backs=False)]
                    if differing:
                        raise SystemExit("batch and serial loop differ: %r" % differing[:4])
                    serial_ms, batch_ms, builds = [], [], []
                    for _ in range(args.repeats):  # alternating: both see the same neighbours on the machine
                        t = time.perf_counter()
                        serial(pairs, options)
                        serial_ms.append((time.perf_counter() - t) * 1e3)
                        t = time.perf_counter()
                        dl.ndt_align_batch(ctx, pairs, options, limits)
                        batch_ms.append((time.perf_counter() - t) * 1e3)
                        builds.append(build_ms(ctx, all_targets[:count], options))
                    ctx.set_profiling(1)
                    staged_single = serial(pairs, options)
                    _, staged = dl.ndt_align_batch(ctx, pairs, options, limits)
                    ctx.set_profiling(0)
                    s, b, build = statistics.median(serial_ms), statistics.median(batch_ms), statistics.median(builds)
                    line = json.dumps(dict(
                        scene=scene, scan=args.size, leaf=leaf, step_mode=mode_name, pairs=count,
                        source_points=int(np.mean([p[1].n for p in pairs])), iterations=[r["iterations"] for r in single],
                        results_equal=True, serial_ms=s, batch_ms=b, batch_over_serial=b / s, serial_ms_calls=serial_ms,
                        batch_ms_calls=batch_ms, serial_pairs_per_s=count / s * 1e3, batch_pairs_per_s=count / b * 1e3,
                        serial_ms_per_pair=s / count, batch_ms_per_pair=b / count,
                        serial_read_backs=sum(r["read_backs"] for r in single), batch_steps=stats["steps"],
                        batch_read_backs=stats["read_backs"], batch_chunks=stats["chunks"],
                        pair_evaluations=stats["pair_evaluations"], evaluation_launches=stats["evaluation_launches"],
                        mixed_steps=stats["mixed_steps"],
                        serial_stages_ms={k: sum(r[k] for r in staged_single) for k in SERIAL_STAGES},
                        batch_stages_ms={k: staged[k] for k in BATCH_STAGES},
                        target_build_ms=build, target_build_share=build / (build + b)))
                    print(line, flush=True)
                    lines.append(line)
            for thing in owned:
                thing.close()
    ctx.close()
    with open(args.out, "w") as f:
        f.write(HEADER + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
