#!/usr/bin/env python3
"""The batch assembler (dliom_cloud_from_sensor_points): time per scan on the device against the CPU model of
HandleMessage's loop (tests/cpp/assemble_model.cc, one thread) on the same message, results checked equal in the same run.

Two drives: a 64 x 1024 scan and config 5's 128 x 2048, in the sensor frame, swept over 0.1 s of the corkscrew, against
200 nodes at 200 Hz.  The device time is the median over >= 20 warm calls, host wall clock around the whole call -- upload
of the message, kernels, the read-back of the count and the check's records, the kept indices' download (every call ends
in its own read-back, so it has finished when it returns).  The model's time is the best of five runs of its loop.  The
check's counters (points recorded / recomputed with glibc / redone) are per scan.  Prints one JSON line per drive;
--out writes them to a file as well (profiles/assemble_bench.json).

The kernels' share comes from a run of its own: `rocprofv3 --kernel-trace --stats -d DIR -o assemble --output-format csv
-- python tools/assemble_bench.py` (that run's timings are not used), then `--kernel-stats DIR/.../assemble_kernel_stats.csv`
on the untraced run adds one more JSON line with every kernel's calls, total microseconds and percentage."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import assemble_common as ac  # noqa: E402


def bench(dl, ctx, model, directory, beams, azimuths, repeats):
    nodes = 200
    times, poses, cloud_time, xyzt = ac.drive(beams, azimuths, nodes)
    _, results, text = ac.run_model(model, times, poses, [ac.assemble_op(cloud_time, ac.MOUNT, xyzt)], directory, timing=True)
    want = results[0]
    kept = ac.honest(want, nodes)
    model_ms = float(text.split()[2])
    trajectory = dl.Trajectory(ctx, times, poses)
    cloud, origin, index = trajectory.assemble(cloud_time, xyzt, ac.MOUNT)  # (cold: uploads the trajectory, sizes the scratch)
    ac.assert_equal_bits(cloud, origin, index, want)
    cloud.close()
    before, backs = ctx.assemble_check_stats(), ctx.read_backs()
    calls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        cloud, origin, index = trajectory.assemble(cloud_time, xyzt, ac.MOUNT)
        calls.append(time.perf_counter() - t0)
        cloud.close()
    after = ctx.assemble_check_stats()
    trajectory.close()
    device_ms = 1e3 * statistics.median(calls)
    return dict(tool="assemble_bench", beams=beams, azimuths=azimuths, points=len(xyzt), kept=kept, nodes=nodes,
                intervals_used=want["intervals"], sin_branch_points=want["libm"], equal_to_model=True,
                device_ms_per_scan=device_ms, device_ms_min=1e3 * min(calls), model_one_thread_ms_per_scan=model_ms,
                speedup=model_ms / device_ms, read_backs_per_scan=(ctx.read_backs() - backs) / repeats,
                recorded_per_scan=(after[0] - before[0]) / repeats, recomputed_per_scan=(after[1] - before[1]) / repeats,
                fixed_per_scan=(after[2] - before[2]) / repeats, ring_overflows=after[3] - before[3], repeats=repeats)


def kernel_shares(path):
    """rocprofv3's kernel_stats.csv -> [{name, calls, total_us, percent}], template arguments cut from the names."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"].replace("(anonymous namespace)::", "")
            name = (name[5:] if name.startswith("void ") else name).split("(")[0].split("<")[0]
            rows.append(dict(name=name, calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3,
                             percent=float(r["Percentage"])))
    merged = {}
    for r in rows:  # (instantiations of one library kernel count together)
        m = merged.setdefault(r["name"], dict(name=r["name"], calls=0, total_us=0.0, percent=0.0))
        for k in ("calls", "total_us", "percent"):
            m[k] += r[k]
    return sorted(merged.values(), key=lambda m: -m["total_us"])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-stats", default="", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    args = ap.parse_args()
    import dliom as dl
    ctx = dl.Context(0)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        model = ac.build_model(d)
        for beams, azimuths in ((64, 1024), (128, 2048)):
            rows.append(bench(dl, ctx, model, d, beams, azimuths, max(args.repeats, 20)))
            print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if args.kernel_stats:
        shares = kernel_shares(args.kernel_stats)
        rows.append(dict(tool="assemble_bench", rocprofv3_kernel_trace_stats=shares,
                         assemble_kernel_percent=sum(k["percent"] for k in shares if k["name"] == "dliom::assemble_kernel")))
        print(json.dumps(rows[-1]), flush=True)
    for r in rows[:2]:  # the project's standing gate: the device call is faster than the model on one thread
        assert r["device_ms_per_scan"] < r["model_one_thread_ms_per_scan"], r
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
