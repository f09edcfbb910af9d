#!/usr/bin/env python3
"""The X-ray aggregator's kernels under rocprofv3: `rocprofv3 --kernel-trace --stats` round tools/points_xray_bench.py on
the 64 x 1024 drive, one child run per colour mode (none, constant, intensity), so that the kernels of an insert with
per-point colours -- the library sort among them -- are told apart from those of the other two.  Per mode and kernel:
calls, total / median / min / max duration, and the microseconds per insert (total / inserts of the run, first round
included).  Writes profiles/points_xray_rocprofv3_kernel_stats.csv.

This process never opens the GPU.  Every child is a fresh process under `timeout -k 10`, which ends its whole process
tree, and the first child that fails, is killed or leaves no result ends the tool: nothing more is started on the device
after a fault."""
import argparse
import csv
import glob
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "tools", "points_xray_bench.py")
SCANS, ROUNDS = 6, 3
CHILD_SECONDS = 200


def kernel_name(full):
    """xray_*_kernel and the context's small kernels by their own names; rocprim's by the stage of the sort they are."""
    found = re.search(r"(xray_[a-z_]+_kernel|fill_multi_kernel|gather_to_pinned_kernel|aos_to_soa_kernel)", full)
    if found:
        return found.group(1)
    if "rocprim" in full:
        stage = re.search(r"wrapped_([a-z_]+)_config", full)
        return "hipcub sort: " + (stage.group(1) if stage else "other")
    return full.split("(")[0][:60]  # the runtime's own fills and copies


def trace(colors, base):
    directory = os.path.join(base, colors)
    os.makedirs(directory, exist_ok=True)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory,
           "-o", "px", "--", sys.executable, BENCH, "--scans", str(SCANS), "--big-scans", "0", "--rounds", str(ROUNDS), "--colors",
           colors, "--out", os.path.join(directory, "bench.json")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 or not files:
        raise RuntimeError("kernel trace of %s: exit status %d, %d result files; stopping here. %s" %
                           (colors, r.returncode, len(files), (r.stderr or "")[-400:]))
    durations = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            durations.setdefault(kernel_name(row["Kernel_Name"]), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    inserts = SCANS * ROUNDS
    return [dict(colors=colors, kernel=k, calls=len(v), total_us=round(sum(v), 1), median_us=round(statistics.median(v), 1),
                 min_us=round(min(v), 1), max_us=round(max(v), 1), us_per_insert=round(sum(v) / inserts, 2))
            for k, v in sorted(durations.items(), key=lambda kv: -sum(kv[1]))]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    base = tempfile.mkdtemp(prefix="px_profile_")
    rows = []
    for colors in ("none", "constant", "intensity"):
        rows += trace(colors, base)
    with open(os.path.join(a.out_dir, "points_xray_rocprofv3_kernel_stats.csv"), "w") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows(rows)
    for r in rows:
        print(",".join(str(v) for v in r.values()))
    shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
