"""What merging a second lidar's scan on the device costs and saves.

From two decoded messages in HBM (the prior lidar's scan and the secondary's, whose sweep ends half a sweep later, so half
of it overlaps) to returns_in_tracking.  Ouster-shaped times (one time a column: runs of 64 or 128 equal times) and
Velodyne-shaped distinct times, 64 x 1024 and 128 x 2048 rays on the synthetic cube.  For each shape, in ONE run and
alternating scan by scan:

  new     dliom_timed_clouds_merge, dliom_range_accumulator_add_timed_cloud, dliom_range_accumulator_finish
  parent  dliom_timed_cloud_download of both objects, the adapter's host RangeDataSynchronizer (copy, merge, std::sort of
          20-byte records, repack: tools/range_sync_host_merge.cc, -O2), dliom_range_accumulator_add with its upload,
          dliom_range_accumulator_finish

Host clock around calls that end in their read-back (every call here does).  Medians over --scans scans after --warmup;
the two paths' results are compared byte for byte before anything is timed.  merge_ms is the new path's first call alone.
sort_ms is dliom_diag_std_sort_order on the merge's keys (the prior cloud's times, then the re-based ones): the sort
stage's kernels plus an upload and a download of four bytes a key that the merge does not have, so
sort_share_upper = sort_ms / new_ms bounds the sort stage's share from above.  --sweep adds smaller Ouster-shaped scans.
Needs a GPU; prints a table and one JSON line, and writes the JSON to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "d-liom_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import range_sync_common as rs  # noqa: E402

SHAPES = [("ouster", "runs of 64", 64, 1024), ("ouster", "runs of 64", 128, 2048), ("velodyne", "distinct", 64, 1024),
          ("velodyne", "distinct", 128, 2048)]
# smaller Ouster-shaped scans: where the two paths cross when every time is shared by a column
SWEEP = [("ouster", "runs of 64", 16, 32), ("ouster", "runs of 64", 16, 64), ("ouster", "runs of 64", 16, 128),
         ("ouster", "runs of 64", 16, 256), ("ouster", "runs of 64", 32, 512), ("ouster", "runs of 64", 64, 512)]
VFS, MIN_RANGE, MAX_RANGE, PERIOD = 0.15, 1.0, 100.0, 0.1
ORIGINS = [[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]]
f32p = C.POINTER(C.c_float)


def build_host_merge(directory):
    lib = os.path.join(directory, "librange_sync_host_merge.so")
    libdir = os.path.join(ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(libdir, "cpp"), "-o", lib, os.path.join(ROOT, "tools", "range_sync_host_merge.cc"), "-L", libdir,
                           "-ldliom", "-Wl,-rpath," + libdir])
    f = C.CDLL(lib).range_sync_host_merge
    f.restype = C.c_longlong
    f.argtypes = [f32p, C.c_longlong, C.c_longlong, f32p, C.c_longlong, C.c_longlong, C.c_int, f32p, f32p]
    return f


def scans_of(pattern, height, width, distinct):
    """-> [(prev_pose, predicted_pose, primary xyzt, secondary xyzt)]: the cube seen from two mounts, times by `pattern`"""
    from dliom import synth
    out = []
    for k in range(distinct):
        prev, cur = synth.trajectory_pose(0.1 * (k + 4)), synth.trajectory_pose(0.1 * (k + 5))
        pts, _ = synth.scan(cur, height, width)
        t = rs.times(pattern, len(pts), run=height)
        primary = np.concatenate([pts.astype(np.float32), t[:, None]], axis=1)
        secondary = primary.copy()
        secondary[:, :3] += np.asarray(ORIGINS[1], np.float32)
        out.append((prev, cur, np.ascontiguousarray(primary), np.ascontiguousarray(secondary)))
    return out


def median_ms(samples):
    return float(np.median(samples) * 1e3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="also the smaller Ouster-shaped scans of SWEEP")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dliom as dl
    if dl.device_count() <= 0:
        raise SystemExit("range_sync_bench needs a GPU: nothing is measured without one")
    host_merge = build_host_merge(tempfile.mkdtemp(prefix="range_sync_bench_"))
    ctx = dl.Context(0)
    accumulator = dl.RangeDataAccumulator(ctx)
    pt, st = rs.PRIMARY_TIME, rs.PRIMARY_TIME + 500_000
    rows = []
    for name, pattern, height, width in SHAPES + (SWEEP if args.sweep else []):
        scans = [(prev, cur, rs.upload(dl, ctx, a), rs.upload(dl, ctx, b)) for prev, cur, a, b in scans_of(pattern, height, width, args.distinct)]
        cap = max(len(a) + len(b) for _, _, a, b in scans)
        merged_xyzt, merged_index = np.zeros((cap, 4), np.float32), np.zeros(cap, np.float32)

        def finish():
            cloud, origin = accumulator.finish(VFS)
            return cloud, origin

        def new_path(prev, cur, a, b, stamps):
            merged = dl.merge_timed_clouds(ctx, a, pt, b, st)
            stamps.append(time.perf_counter())
            pose, _ = accumulator.add_timed_cloud(prev, cur, PERIOD, merged, MIN_RANGE, MAX_RANGE, VFS, origins=ORIGINS)
            cloud, origin = finish()
            merged.close()
            return cloud, origin, pose

        def parent_path(prev, cur, a, b, stamps):
            pa, _ = a.download()
            pb, _ = b.download()
            stamps.append(time.perf_counter())
            m = host_merge(pa.ctypes.data_as(f32p), len(pa), pt, pb.ctypes.data_as(f32p), len(pb), st, 0, merged_xyzt.ctypes.data_as(f32p),
                           merged_index.ctypes.data_as(f32p))
            assert m > len(pa)
            stamps.append(time.perf_counter())
            pose, _ = accumulator.add(prev, cur, PERIOD, merged_xyzt[:m], MIN_RANGE, MAX_RANGE, VFS, origins=ORIGINS,
                                      origin_index=merged_index[:m])
            cloud, origin = finish()
            return cloud, origin, pose

        # ---- equal results, before anything is timed
        merged_points = returns = 0
        keys = None
        for prev, cur, a, b in scans:
            merged = dl.merge_timed_clouds(ctx, a, pt, b, st)
            got, _ = merged.download()
            got_index = merged.download_origin_index()
            merged.close()
            m = host_merge(a.download()[0].ctypes.data_as(f32p), len(a), pt, b.download()[0].ctypes.data_as(f32p), len(b), st, 0,
                           merged_xyzt.ctypes.data_as(f32p), merged_index.ctypes.data_as(f32p))
            assert m == len(got) and got.tobytes() == merged_xyzt[:m].tobytes() and got_index.tobytes() == merged_index[:m].tobytes(), \
                "the merge differs"
            new, parent = new_path(prev, cur, a, b, []), parent_path(prev, cur, a, b, [])
            pa, pb = new[0].download(), parent[0].download()
            assert pa.tobytes() == pb.tobytes() and new[1].tobytes() == parent[1].tobytes() and new[2].tobytes() == parent[2].tobytes(), \
                "returns differ"
            merged_points, returns = m, len(pa)
            # the sort's input: the prior cloud's times, then the overlapping part's re-based ones
            i_start, i_end1, current_end, seconds_st = rs.overlap(a.download()[0], pt, b.download()[0], st)
            part = ((b.download()[0][i_start:i_end1, 3].astype(np.float64) + seconds_st) - current_end).astype(np.float32)
            keys = np.concatenate([a.download()[0][:, 3], part])
            assert len(keys) == m
            new[0].close()
            parent[0].close()
        # ---- timed, alternating
        t = {"new": [], "merge": [], "parent": [], "download": [], "host_merge": [], "sort": []}
        for k in range(args.warmup + args.scans):
            prev, cur, a, b = scans[k % len(scans)]
            stamps = []
            t0 = time.perf_counter()
            r = new_path(prev, cur, a, b, stamps)
            t1 = time.perf_counter()
            r[0].close()
            parent_stamps = []
            t2 = time.perf_counter()
            r = parent_path(prev, cur, a, b, parent_stamps)
            t3 = time.perf_counter()
            r[0].close()
            t4 = time.perf_counter()
            dl.diag_std_sort_order(ctx, keys)
            t5 = time.perf_counter()
            if k >= args.warmup:
                t["new"].append(t1 - t0)
                t["merge"].append(stamps[0] - t0)
                t["parent"].append(t3 - t2)
                t["download"].append(parent_stamps[0] - t2)
                t["host_merge"].append(parent_stamps[1] - parent_stamps[0])
                t["sort"].append(t5 - t4)
        row = {"sensor": name, "times": pattern if name == "velodyne" else "runs of %d" % height, "height": height, "width": width,
               "primary_points": len(scans[0][2]), "secondary_points": len(scans[0][3]), "merged_points": merged_points, "returns": returns,
               "scans": args.scans, "new_ms": median_ms(t["new"]), "parent_ms": median_ms(t["parent"]), "merge_ms": median_ms(t["merge"]),
               "parent_download_ms": median_ms(t["download"]), "parent_host_merge_ms": median_ms(t["host_merge"]),
               "sort_ms": median_ms(t["sort"])}
        row["sort_share_upper"] = row["sort_ms"] / row["new_ms"]
        row["speedup"] = row["parent_ms"] / row["new_ms"]
        for key in ("new", "parent"):
            q = np.percentile(np.asarray(t[key]) * 1e3, [10, 90])
            row["%s_ms_p10_p90" % key] = [float(q[0]), float(q[1])]
        rows.append(row)
        for _, _, a, b in scans:
            a.close()
            b.close()
    print("%-9s %-10s %8s %8s | %9s %9s %7s | %9s %9s %9s | %9s %9s" % ("sensor", "shape", "merged", "returns", "new", "parent", "x", "merge",
                                                                          "sort", "share <=", "download", "host merge"))
    for r in rows:
        print("%-9s %4dx%-5d %8d %8d | %6.3f ms %6.3f ms %7.2f | %6.3f ms %6.3f ms %9.2f | %6.3f ms %7.3f ms" %
              (r["sensor"], r["height"], r["width"], r["merged_points"], r["returns"], r["new_ms"], r["parent_ms"], r["speedup"],
               r["merge_ms"], r["sort_ms"], r["sort_share_upper"], r["parent_download_ms"], r["parent_host_merge_ms"]))
    result = {"bench": "range_sync", "warmup": args.warmup, "rows": rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    accumulator.close()
    ctx.close()


if __name__ == "__main__":
    main()
