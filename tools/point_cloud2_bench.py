"""What decoding PointCloud2 messages on the device costs and saves.

Ouster-shaped (48-byte records) and Velodyne-shaped (22-byte records, the float time at offset 18) messages of 64 x 1024
and 128 x 2048 points, a few distinct scans of the synthetic cube in turn.  For each shape, in ONE run and alternating
message by message:

  decode        dliom_point_cloud2_decode (upload of the message's bytes, one pass, one read-back)
                against the one-thread C++ model of the same statement (tests/cpp/point_cloud2_model.cc, -O2): the loop a
                caller of the library writes today
  scan          message -> returns_in_tracking
                new:    dliom_point_cloud2_decode, dliom_add_range_data_timed_cloud, the object destroyed
                parent: the model's decode on the host, then dliom_add_range_data on its vector

Host clock around calls that end in their read-back (every call here does).  Medians over --messages messages after
--warmup; the results of both paths are compared byte for byte on every distinct message before anything is timed.
--pinned: the message buffers (new path) and the model's output vector (parent path) are registered with
dliom_host_register first.  Needs a GPU; prints a table and one JSON line, and writes the JSON to --out."""
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

import point_cloud2_common as pc  # noqa: E402

SHAPES = [("ouster", pc.OUSTER, 64, 1024), ("ouster", pc.OUSTER, 128, 2048), ("velodyne", pc.VELODYNE, 64, 1024),
          ("velodyne", pc.VELODYNE, 128, 2048)]
VFS, MIN_RANGE, MAX_RANGE, PERIOD = 0.15, 1.0, 100.0, 0.1
f32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)


def build_model(directory):
    lib = os.path.join(directory, "libpoint_cloud2_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-DPOINT_CLOUD2_MODEL_NO_MAIN", "-I",
                           os.path.join(ROOT, "include"), "-o", lib, os.path.join(ROOT, "tests", "cpp", "point_cloud2_model.cc")])
    return C.CDLL(lib).point_cloud2_model


def scan_messages(mode, height, width, distinct):
    """`distinct` scans of height x width rays along the corkscrew, framed as the driver would; rays without a return are
    NaN points, as drivers of organised clouds send them -> [(prev_pose, predicted_pose, Message)]"""
    from dliom import synth
    out = []
    for k in range(distinct):
        prev, cur = synth.trajectory_pose(0.1 * (k + 4)), synth.trajectory_pose(0.1 * (k + 5))
        pts, rel_t = synth.scan(cur, height, width)
        n = height * width
        points = np.full((n, 3), np.nan, np.float32)
        times = np.full(n, rel_t[-1] if len(rel_t) else 0.0)
        points[:len(pts)], times[:len(pts)] = pts, rel_t
        out.append((prev, cur, pc.scan_message(mode, points, times, height, width, seed=k)))
    return out


def median_ms(samples):
    return float(np.median(samples) * 1e3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--pinned", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dliom as dl
    if dl.device_count() <= 0:
        raise SystemExit("point_cloud2_bench needs a GPU: nothing is measured without one")
    model = build_model(tempfile.mkdtemp(prefix="point_cloud2_bench_"))
    ctx = dl.Context(0)
    mount = pc.MOUNT
    mount_p = np.ascontiguousarray(mount, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    rows = []
    for name, mode, height, width in SHAPES:
        scans = scan_messages(mode, height, width, args.distinct)
        n = height * width
        xyzt = np.zeros((n, 4), np.float32)  # the host vector of the parent's path
        if args.pinned:
            ctx.host_register(xyzt)
        kept, has, stamp, origin = C.c_int64(), C.c_int(), C.c_int64(), np.zeros(3, np.float32)
        messages = [(prev, cur, m, m.to_library(dl)) for prev, cur, m in scans]
        if args.pinned:
            for _, _, m, _ in messages:
                ctx.host_register(m.data)

        def host_decode(lib_msg):
            status = model(C.byref(lib_msg.struct), mode, mount_p, xyzt.ctypes.data_as(f32p), None, C.byref(kept), C.byref(has),
                           C.byref(stamp), origin.ctypes.data_as(f32p))
            assert status == 0
            return xyzt[:kept.value]

        def parent_path(prev, cur, lib_msg):
            ranges = host_decode(lib_msg)
            return dl.add_range_data(ctx, prev, cur, PERIOD, ranges, origin, MIN_RANGE, MAX_RANGE, VFS)

        def new_path(prev, cur, lib_msg):
            cloud, _, device_origin = lib_msg.decode(ctx, mode, mount)
            result = cloud.add_range_data(prev, cur, PERIOD, device_origin, MIN_RANGE, MAX_RANGE, VFS)
            cloud.close()
            return result

        # ---- equal results, before anything is timed
        kept_points = returns = 0
        for prev, cur, m, lib_msg in messages:
            want = host_decode(lib_msg).copy()
            cloud, device_time, device_origin = lib_msg.decode(ctx, mode, mount)
            got, _ = cloud.download()
            cloud.close()
            assert pc.same_bits(got, want) and device_time == stamp.value and pc.same_bits(device_origin, origin), "decode differs"
            a, b = parent_path(prev, cur, lib_msg), new_path(prev, cur, lib_msg)
            pa, pb = a[0].download(), b[0].download()
            assert pc.same_bits(pa, pb) and pc.same_bits(a[1], b[1]) and pc.same_bits(a[2], b[2]), "returns differ"
            kept_points, returns = len(want), len(pa)
            a[0].close()
            b[0].close()
        # ---- timed, alternating
        t = {"device_decode": [], "model_decode": [], "new": [], "parent": []}
        for k in range(args.warmup + args.messages):
            prev, cur, m, lib_msg = messages[k % len(messages)]
            t0 = time.perf_counter()
            cloud, _, _ = lib_msg.decode(ctx, mode, mount)
            t1 = time.perf_counter()
            cloud.close()
            t2 = time.perf_counter()
            host_decode(lib_msg)
            t3 = time.perf_counter()
            r = new_path(prev, cur, lib_msg)
            t4 = time.perf_counter()
            r[0].close()
            t5 = time.perf_counter()
            r = parent_path(prev, cur, lib_msg)
            t6 = time.perf_counter()
            r[0].close()
            if k >= args.warmup:
                t["device_decode"].append(t1 - t0)
                t["model_decode"].append(t3 - t2)
                t["new"].append(t4 - t3)
                t["parent"].append(t6 - t5)
        row = {"sensor": name, "height": height, "width": width, "point_step": scans[0][2].point_step, "message_bytes": len(scans[0][2].data),
               "kept_points": kept_points, "returns": returns, "messages": args.messages,
               "decode_ms_device": median_ms(t["device_decode"]), "decode_ms_model": median_ms(t["model_decode"]),
               "scan_ms_new": median_ms(t["new"]), "scan_ms_parent": median_ms(t["parent"])}
        row["scans_per_s_new"], row["scans_per_s_parent"] = 1e3 / row["scan_ms_new"], 1e3 / row["scan_ms_parent"]
        for key in ("new", "parent"):
            q = np.percentile(np.asarray(t[key]) * 1e3, [10, 90])
            row["scan_ms_%s_p10_p90" % key] = [float(q[0]), float(q[1])]
        rows.append(row)
        if args.pinned:
            ctx.host_unregister(xyzt)
            for _, _, m, _ in messages:
                ctx.host_unregister(m.data)
    print("%-9s %-10s %6s %10s | %9s %9s | %9s %9s | %9s %9s" % ("sensor", "shape", "step", "bytes", "dec dev", "dec model", "scan new",
                                                                   "scan par", "new /s", "parent /s"))
    for r in rows:
        print("%-9s %4dx%-5d %6d %10d | %7.3f ms %7.3f ms | %7.3f ms %7.3f ms | %9.1f %9.1f" %
              (r["sensor"], r["height"], r["width"], r["point_step"], r["message_bytes"], r["decode_ms_device"], r["decode_ms_model"],
               r["scan_ms_new"], r["scan_ms_parent"], r["scans_per_s_new"], r["scans_per_s_parent"]))
    result = {"bench": "point_cloud2", "pinned": bool(args.pinned), "warmup": args.warmup, "rows": rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
