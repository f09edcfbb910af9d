#!/usr/bin/env python3
"""X-ray aggregation (dliom_points_xray_*): time per batch on the device against the CPU model
(tests/cpp/points_xray_model.cc, one thread) on the same batches, results checked equal in the same run.

Drives of 64 x 1024 and 128 x 2048 scans of the cube scene with moving spheres at a 5 cm voxel size through the xy
transform, once without colours, once with one colour a batch and once with a colour per point.  The clouds are on the
device before the clock starts (the adapters hand a filter's output over there).  An insert returns with its last kernels
still in flight, so each timed call is followed by a stream synchronise inside the clock.  The device times are medians of
the warm inserts: every scan of the drive is inserted `rounds` times into the same aggregator and the first round (tables
growing) is reported apart.  Writes one JSON object per case to stdout and all of them to --out."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import points_xray_common as xc  # noqa: E402


def bench(dl, ctx, model, directory, beams, azimuths, scans, voxel_size, colors, rounds):
    ops = xc.drive_ops(scans, beams, azimuths, colors)
    transform = xc.TRANSFORMS["xy"]
    clouds = [dl.PointCloud(ctx, o[2]) for o in ops]
    x = dl.PointsXray(ctx, voxel_size, transform)
    first, warm = [], []
    for r in range(rounds):
        for o, c in zip(ops, clouds):
            col = None if len(o[3]) == 0 else o[3]
            ctx.synchronize()
            t0 = time.perf_counter()
            x.insert(c, col)
            ctx.synchronize()
            (first if r == 0 else warm).append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    image = x.draw()
    draw_s = time.perf_counter() - t0
    stats = x.stats()
    # the model on the same stream of inserts (every round), timed in this run on this machine
    want = xc.run_model(model, voxel_size, transform, ops * rounds, directory, timing=True)
    xc.assert_equal([x], [0] * (len(ops) * rounds), want)
    x.close()
    for c in clouds:
        c.close()
    model_ms = 1e3 * want.insert_seconds / (len(ops) * rounds)
    med = 1e3 * statistics.median(warm)
    return dict(tool="points_xray_bench", beams=beams, azimuths=azimuths, scans=scans, rounds=rounds, voxel_size=voxel_size,
                colors=colors, points_per_batch=int(np.mean([len(o[2]) for o in ops])), voxels=stats["voxels"],
                columns=stats["columns"], leaves=stats["leaves"], table_bytes=stats["table_bytes"],
                probes_per_point=stats["probes"] / stats["points"], longest_segment=stats["longest_segment"],
                growths=stats["growths"], image=list(image.shape), equal_to_model=True,
                device_ms_per_batch=dict(warm_median=med, warm_min=1e3 * min(warm), warm_max=1e3 * max(warm),
                                         first_round_median=1e3 * statistics.median(first), timed_calls=len(warm)),
                device_draw_ms=1e3 * draw_s, model_ms_per_batch=model_ms, model_draw_ms=1e3 * want.draw_seconds,
                speedup_over_model=model_ms / med, device_faster_than_model=bool(med < model_ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--big-scans", type=int, default=3, help="scans of the 128 x 2048 drive (0: skip it)")
    ap.add_argument("--voxel-size", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--colors", default="none,constant,intensity", help="which colour modes to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_xray_bench.json"))
    args = ap.parse_args()
    import dliom as dl
    ctx = dl.Context(0)
    results = []
    with tempfile.TemporaryDirectory() as d:
        model = xc.build_model(d)
        for beams, azimuths, scans in ((64, 1024, args.scans), (128, 2048, args.big_scans)):
            for colors in args.colors.split(","):
                if scans > 0:
                    results.append(bench(dl, ctx, model, d, beams, azimuths, scans, args.voxel_size, colors, args.rounds))
                    print(json.dumps(results[-1]), flush=True)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    assert all(r["device_faster_than_model"] for r in results), "the device insert is not faster than the model on one thread"


if __name__ == "__main__":
    main()
