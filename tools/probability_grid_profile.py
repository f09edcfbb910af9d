#!/usr/bin/env python3
"""The 2D probability grid's kernels under rocprofv3, each collection in a child run of its own:

  * `rocprofv3 --kernel-trace --stats` round tools/probability_grid_bench.py, one child per drive: per kernel the calls,
    total / median / min / max duration (profiles/probability_grid_rocprofv3_kernel_stats.csv);
  * `rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum` on pg_cast_rays_kernel alone (tools/pmc_live.py measure): the L2 hit rate
    of the ray pass (profiles/probability_grid_pmc_l2.json).

This process never opens the GPU.  Every child is a fresh process under `timeout -k 10`, which ends its whole process
tree, and the first child that fails, is killed or leaves no result ends the tool: nothing more is started on the device
after a fault."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "tools", "probability_grid_bench.py")
DRIVES = {"64x1024": ["--scans", "4", "--big-scans", "0"], "128x2048": ["--scans", "0", "--big-scans", "2"]}


CHILD_SECONDS = 280


def child(what, rocprof_args, bench_args, directory, result_glob):
    """One rocprofv3 run of the bench -> its result files; raises (and so ends the tool) on any failure."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = (["timeout", "-k", "10", str(CHILD_SECONDS), rocprof] + rocprof_args +
           ["--output-format", "csv", "-d", directory, "-o", "pg", "--", sys.executable, BENCH] + bench_args)
    r = subprocess.run(cmd, capture_output=True, text=True)
    files = glob.glob(os.path.join(directory, "**", result_glob), recursive=True)
    if r.returncode != 0 or not files:
        raise RuntimeError("%s: exit status %d, %d result files; stopping here. %s" % (what, r.returncode, len(files), (r.stderr or "")[-400:]))
    return files


def kernel_trace(drive, args, base):
    files = child("kernel trace of " + drive, ["--kernel-trace", "--stats"], args, os.path.join(base, "trace_" + drive),
                  "*kernel_trace.csv")
    durations = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            found = re.search(r"pg_[a-z_]+_kernel", row["Kernel_Name"])  # dliom::(anonymous namespace)::pg_..._kernel(...)
            if found:
                durations.setdefault(found.group(0), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return [dict(drive=drive, kernel=k, calls=len(v), total_us=round(sum(v), 1), median_us=round(statistics.median(v), 1),
                 min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in sorted(durations.items())]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    base = tempfile.mkdtemp(prefix="pg_profile_")
    rows = []
    for drive, args in DRIVES.items():
        rows += kernel_trace(drive, args, base)
    with open(os.path.join(a.out_dir, "probability_grid_rocprofv3_kernel_stats.csv"), "w") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows(rows)
    for r in rows:
        print(r)
    l2 = {}
    for drive, args in DRIVES.items():
        files = child("L2 counters of " + drive, ["--pmc", "TCC_HIT_sum", "TCC_MISS_sum", "--kernel-include-regex", "pg_cast_rays"],
                      args + ["--repeats", "8"], os.path.join(base, "pmc_" + drive), "*counter_collection.csv")
        acc = {}
        for f in files:
            for row in csv.DictReader(open(f)):
                acc.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        counters = {k: {"mean": sum(v) / len(v), "launches": len(v)} for k, v in acc.items()}
        hit, miss = counters["TCC_HIT_sum"]["mean"], counters["TCC_MISS_sum"]["mean"]
        l2[drive] = dict(counters=counters, l2_hit_rate=hit / (hit + miss))
    with open(os.path.join(a.out_dir, "probability_grid_pmc_l2.json"), "w") as f:
        json.dump(dict(kernel="pg_cast_rays_kernel", per_dispatch_means=l2), f, indent=1)
        f.write("\n")
    print(json.dumps(l2))
    shutil.rmtree(base, ignore_errors=True)


if __name__ == "__main__":
    main()
