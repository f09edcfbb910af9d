#!/usr/bin/env python3
"""2D probability grid insertion (dliom_inserter2d_insert_cloud): time per batch on the device against the CPU oracle's
insert (oracle.ProbabilityGrid.insert, -O3, one thread) on the same batches in the same run, equality checked in the run.

Drives of 64 x 1024 scans and of 128 x 2048 scans of the cube scene at 5 cm, after the device range filter 1 .. 60 m.
Per drive: one pass over the scans on a fresh grid that is compared with the oracle after every batch (the oracle's
insert is timed there); then >= 24 warm inserts cycling over the scans into the same grid -- host wall clock round the
call (every call ends in its own read-back) and the hits / rays / clear split from dliom_ctx_kernel_time -- and draw; the
oracle then receives the same warm inserts and the timed grid is compared once more.
Prints one JSON line per drive; --out also writes them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import outlier_common as oc  # noqa: E402
import probability_grid_common as pc  # noqa: E402

HIT, MISS = 0.55, 0.49


def bench(dl, orc, ctx, beams, azimuths, scans, resolution, repeats, check_warm=True):
    batches = oc.drive(scans, beams, azimuths)
    clouds, kept_pts = [], []
    for o, p in batches:
        c = dl.PointCloud(ctx, p)
        kept, index = c.min_max_range_filter(o, 1.0, 60.0)
        c.close()
        clouds.append(kept)
        kept_pts.append(p[index])
    grid, ins = dl.ProbabilityGrid2D(ctx, resolution), dl.Inserter2D(ctx, HIT, MISS, True)
    ogrid = pc.new_oracle_grid(orc, resolution)
    first, oracle_s = [], []
    for (o, _), c, k in zip(batches, clouds, kept_pts):
        t0 = time.perf_counter()
        ins.insert(grid, o, c)
        first.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ogrid.insert(o, k, HIT, MISS, True)
        oracle_s.append(time.perf_counter() - t0)
        pc.assert_equal(grid, ogrid)
    visited = grid.stats()["cells_visited"]
    cycle = ([(o, c) for (o, _), c in zip(batches, clouds)] * ((repeats + scans - 1) // scans))[:max(repeats, scans)]
    points_of = {id(c): k for c, k in zip(clouds, kept_pts)}
    for o, c in cycle[:2]:
        ins.insert(grid, o, c)  # warm
    warm = []
    for o, c in cycle:
        t0 = time.perf_counter()
        ins.insert(grid, o, c)
        warm.append(time.perf_counter() - t0)
    ctx.set_profiling(1)
    ctx.reset_profiling()
    for o, c in cycle:
        ins.insert(grid, o, c)
    if check_warm:  # the oracle receives the warm and the profiled inserts too: the timed grid is compared at the end
        for o, c in cycle[:2] + cycle + cycle:
            ogrid.insert(o, points_of[id(c)], HIT, MISS, True)
        pc.assert_equal(grid, ogrid)
    split = {name: ctx.kernel_time(k)[0] / len(cycle) for name, k in
             (("hits", dl.KERNEL_PG_HITS), ("rays", dl.KERNEL_PG_RAYS), ("clear", dl.KERNEL_PG_CLEAR))}
    ctx.set_profiling(0)
    draws = []
    for _ in range(8):
        t0 = time.perf_counter()
        image, _ = grid.draw(True)
        draws.append(time.perf_counter() - t0)
    stats = grid.stats()
    med = lambda v: 1e3 * statistics.median(v)
    out = dict(tool="probability_grid_bench", beams=beams, azimuths=azimuths, scans=scans, resolution=resolution,
               points_per_scan=sum(len(k) for k in kept_pts) / scans, grid_side=grid.limits()[2][0], grid_bytes=stats["bytes"],
               growths=stats["growths"], cells_visited_per_scan=visited / scans, error_word=stats["error_word"],
               # assert_equal raises otherwise: after every batch of the first pass; after all timed inserts if checked
               equal_to_oracle_after_every_first_pass_batch=True, equal_to_oracle_after_the_timed_inserts=True if check_warm else None,
               first_pass_ms_per_scan=med(first), oracle_ms_per_scan=med(oracle_s),
               device_ms_per_scan=dict(insert=med(warm), insert_min=1e3 * min(warm), insert_max=1e3 * max(warm), timed_calls=len(warm),
                                       kernels_hits=split["hits"], kernels_rays=split["rays"], kernels_clear=split["clear"]),
               draw_rotated_ms=med(draws), image=list(image.shape))
    out["cells_visited_per_s"] = out["cells_visited_per_scan"] / (1e-3 * max(split["rays"], 1e-9))
    out["speedup_over_oracle"] = out["oracle_ms_per_scan"] / out["device_ms_per_scan"]["insert"]
    out["device_faster_than_oracle"] = out["speedup_over_oracle"] > 1.0
    for c in clouds:
        c.close()
    ins.close()
    grid.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--scans", type=int, default=4)
    ap.add_argument("--big-scans", type=int, default=2, help="scans of the 128 x 2048 drive (0: skip it)")
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-final-check", action="store_true", help="do not replay the timed inserts into the oracle")
    args = ap.parse_args()
    import dliom as dl
    from oracle import oracle as orc
    ctx = dl.Context(0)
    lines = []
    for beams, azimuths, scans in ((64, 1024, args.scans), (128, 2048, args.big_scans)):
        if scans > 0:
            lines.append(bench(dl, orc, ctx, beams, azimuths, scans, args.resolution, args.repeats, not args.no_final_check))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
