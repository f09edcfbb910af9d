"""K scan pairs aligned by a serial loop of dliom_icp_align against one dliom_icp_align_batch, in one process.  Scenes and
sizes as in tools/icp_bench.py (cube and ground, 64 x 1024), raw and filtered by dliom_cloud_voxel_filter to about 4 k points
(where launches and read-backs dominate); pair k is the scan at trajectory_pose(0.30 + 0.01 k) (target) and the one at
trajectory_pose(0.35 + 0.01 k) (source), each pair with an index of its own, as the ground-truth tool's constraints have;
the 30 m preset.  The two are checked equal, bit for bit, before anything is timed.  Then one warm-up of each and
--repeats alternating repetitions; a host clock around calls that end in the read-back of their last step; medians.  A line
of JSON a case: pairs/s and ms a pair of both, steps and read-backs, and the batch's stage split from one more, profiled call
(the serial loop's split is the sum of its results').
usage: python tools/icp_batch_bench.py [--scenes cube ground] [--pairs 1 4 16 64] [--repeats 5] [--voxel 0.6]"""
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
import icp_batch_common as bc  # noqa: E402
import dliom as dl  # noqa: E402
from dliom import synth  # noqa: E402

STAGES = ("search_ms", "reduce_ms", "solve_ms", "transform_ms")


def make_pairs(ctx, scene, beams, azimuths, count, voxel):
    """-> (pairs for icp_align_batch, what to close)"""
    pairs, owned = [], []
    for k in range(count):
        with synth.scene(scene, trajectory=False):
            target = synth.scan(synth.trajectory_pose(0.30 + 0.01 * k), beams, azimuths)[0]
            source = synth.scan(synth.trajectory_pose(0.35 + 0.01 * k), beams, azimuths)[0]
        clouds = [dl.PointCloud(ctx, target), dl.PointCloud(ctx, source)]
        if voxel > 0.0:
            filtered = [c.voxel_filter(voxel) for c in clouds]
            for c in clouds:
                c.close()
            clouds = filtered
        index = dl.NnIndex(ctx, clouds[0])
        clouds[0].close()
        owned += [index, clouds[1]]
        pairs.append((index, clouds[1], None))
    return pairs, owned


def serial(pairs, options):
    return [dl.Icp(index, options).align(source) for index, source, _ in pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "ground"])
    ap.add_argument("--size", default="64x1024")
    ap.add_argument("--pairs", nargs="+", type=int, default=[1, 4, 16, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.6, help="edge of the filtered case's voxel filter (0.6 m: about 4 k points of the cube scan)")
    args = ap.parse_args()
    beams, azimuths = (int(v) for v in args.size.split("x"))
    ctx = dl.Context(0)
    options = dl.ground_truth_icp_options()
    limits = dl.icp_batch_default_limits(max_pairs_in_flight=max(1, min(max(args.pairs), dl.ICP_BATCH_MAX_PAIRS)),
                                         max_scratch_bytes=8 << 30)
    for scene in args.scenes:
        for voxel in (0.0, args.voxel):
            all_pairs, owned = make_pairs(ctx, scene, beams, azimuths, max(args.pairs), voxel)
            for count in args.pairs:
                pairs = all_pairs[:count]
                single = serial(pairs, options)  # warm-up of the loop: every index reserves its scratch
                batched, stats = dl.icp_align_batch(ctx, pairs, options, limits)  # warm-up of the batch
                differing = [(i, bc.same_result(b, s)) for i, (b, s) in enumerate(zip(batched, single)) if bc.same_result(b, s)]
                if differing:
                    raise SystemExit("batch and serial loop differ: %r" % differing[:4])
                serial_ms, batch_ms = [], []
                for _ in range(args.repeats):  # alternating: both see the same neighbours on the machine
                    t = time.perf_counter()
                    serial(pairs, options)
                    serial_ms.append((time.perf_counter() - t) * 1e3)
                    t = time.perf_counter()
                    dl.icp_align_batch(ctx, pairs, options, limits)
                    batch_ms.append((time.perf_counter() - t) * 1e3)
                ctx.set_profiling(1)
                staged_single = serial(pairs, options)
                _, staged = dl.icp_align_batch(ctx, pairs, options, limits)
                ctx.set_profiling(0)
                s, b = statistics.median(serial_ms), statistics.median(batch_ms)
                print(json.dumps(dict(
                    scene=scene, scan=args.size, voxel_filter=voxel, pairs=count,
                    source_points=int(np.mean([len(src) for _, src, _ in pairs])),
                    iterations=[r["iterations"] for r in single], results_equal=True,
                    serial_ms=s, batch_ms=b, batch_over_serial=b / s, serial_ms_calls=serial_ms, batch_ms_calls=batch_ms,
                    serial_pairs_per_s=count / s * 1e3, batch_pairs_per_s=count / b * 1e3, serial_ms_per_pair=s / count,
                    batch_ms_per_pair=b / count, serial_read_backs=sum(r["read_backs"] for r in single),
                    batch_steps=stats["steps"], batch_read_backs=stats["read_backs"], batch_chunks=stats["chunks"],
                    serial_stages_ms={k: sum(r[k] for r in staged_single) for k in STAGES},
                    batch_stages_ms={k: staged[k] for k in STAGES})), flush=True)
            for thing in owned:
                thing.close()
    ctx.close()


if __name__ == "__main__":
    main()
