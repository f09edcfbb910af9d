#!/usr/bin/env python3
"""Moving-object removal (dliom_outlier_remover_*): time per pass and per scan on the device against the CPU model
(tests/cpp/outlier_model.cc, one thread) on the same batches, results checked equal in the same run.

A drive of 64 x 1024 scans (and config 5's 128 x 2048) of the cube scene with moving spheres at a 5 cm voxel size.  The
device times are medians over >= 20 warm calls, host wall clock around the call (every call ends in its own read-back,
so it has finished when it returns); pass 2 is timed on a table that holds every scan's hits, cycling over the scans.
The equality check runs the three passes once on a fresh remover and compares the whole table and every kept_index with
the model's.  Prints one JSON line per drive.  DLIOM_LIB=<path> measures another build of the library (the flat-hash
experiment: make -C d-liom_amd experiments EXP_FLAGS=-DDLIOM_OUTLIER_LEAF_BITS=0 EXP_NAME=flat)."""
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
import outlier_common as oc  # noqa: E402


def timed(fn, calls):
    out = []
    for c in calls:
        t0 = time.perf_counter()
        fn(*c)
        out.append(time.perf_counter() - t0)
    return out


def bench(dl, ctx, model, directory, beams, azimuths, scans, voxel_size, repeats, with_model):
    batches = oc.drive(scans, beams, azimuths)
    clouds = [dl.PointCloud(ctx, p) for _, p in batches]
    points = sum(len(p) for _, p in batches)
    # ---- equality, and the counters of exactly one three-pass run
    r = dl.OutlierRemover(ctx, voxel_size)
    t1 = timed(r.mark_hits, [(c,) for c in clouds])
    t2 = timed(r.count_rays, [(o, c) for (o, _), c in zip(batches, clouds)])
    kept = []
    t3 = []
    for c in clouds:
        t0 = time.perf_counter()
        k, index = r.filter(c)
        t3.append(time.perf_counter() - t0)
        kept.append(index)
        k.close()
    stats = r.stats()
    table = r.voxels()
    out = dict(tool="outlier_bench", lib=os.path.basename(os.environ.get("DLIOM_LIB", dl.LIB_PATH)), beams=beams,
               azimuths=azimuths, scans=scans, voxel_size=voxel_size, points=points,
               removed=points - sum(len(k) for k in kept), voxels=stats["voxels"], leaves=stats["leaves"],
               table_bytes=stats["table_bytes"], growths=stats["growths"],
               samples_per_scan=stats["samples_walked"] / scans, probes_per_scan=stats["probes"] / scans,
               first_run_ms_per_scan=dict(pass1=1e3 * statistics.median(t1), pass2=1e3 * statistics.median(t2),
                                          pass3=1e3 * statistics.median(t3)))
    if with_model:
        results, want, text = oc.run_model(model, voxel_size, oc.three_pass_ops(batches), directory, timing=True)
        equal = (all(np.array_equal(a, b) for a, b in zip(table, want)) and
                 all(np.array_equal(k, w[1]) for k, w in zip(kept, results[2 * scans:])))
        words = text.split()
        out["equal_to_model"] = bool(equal)
        out["model_ms_per_scan"] = dict(pass1=1e3 * float(words[1]) / scans, pass2=1e3 * float(words[3]) / scans,
                                        pass3=1e3 * float(words[5]) / scans)
        assert int(words[7]) == stats["samples_walked"], (words, stats)
        assert equal, "device and model differ"
    r.close()
    # ---- warm timings: pass 1 into fresh removers (the table grows as in a real run), passes 2 and 3 cycling over the scans
    p1, keep = [], None
    for _ in range(max(1, (repeats + scans - 1) // scans)):
        if keep is not None:
            keep.close()
        keep = dl.OutlierRemover(ctx, voxel_size)
        p1 += timed(keep.mark_hits, [(c,) for c in clouds])
    cycle = [(o, c) for (o, _), c in zip(batches, clouds)]
    timed(keep.count_rays, cycle[:2])  # warm
    p2 = timed(keep.count_rays, (cycle * ((repeats + scans - 1) // scans))[:max(repeats, scans)])
    before = keep.stats()["probes"]
    p3 = []
    for c in (clouds * ((repeats + scans - 1) // scans))[:max(repeats, scans)]:
        t0 = time.perf_counter()
        k, _ = keep.filter(c)
        p3.append(time.perf_counter() - t0)
        k.close()
    assert keep.stats()["probes"] == before
    keep.close()
    med = lambda v: 1e3 * statistics.median(v)
    out["device_ms_per_scan"] = dict(pass1=med(p1), pass2=med(p2), pass3=med(p3), pass2_min=1e3 * min(p2), pass2_max=1e3 * max(p2),
                                     timed_calls=len(p2))
    out["pass2_samples_per_s"] = out["samples_per_scan"] / (1e-3 * out["device_ms_per_scan"]["pass2"])
    out["pass2_probes_per_s"] = out["probes_per_scan"] / (1e-3 * out["device_ms_per_scan"]["pass2"])
    if with_model:
        out["pass2_speedup_over_model"] = out["model_ms_per_scan"]["pass2"] / out["device_ms_per_scan"]["pass2"]
        out["pass2_device_faster_than_model"] = out["pass2_speedup_over_model"] > 1.0
    for c in clouds:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--big-scans", type=int, default=2, help="scans of the 128 x 2048 drive (0: skip it)")
    ap.add_argument("--voxel-size", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--no-model", action="store_true", help="device times only (no equality check)")
    args = ap.parse_args()
    import dliom as dl
    ctx = dl.Context(0)
    with tempfile.TemporaryDirectory() as d:
        model = None if args.no_model else oc.build_model(d)
        for beams, azimuths, scans in ((64, 1024, args.scans), (128, 2048, args.big_scans)):
            if scans > 0:
                print(json.dumps(bench(dl, ctx, model, d, beams, azimuths, scans, args.voxel_size, args.repeats,
                                       not args.no_model)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
