#!/usr/bin/env python3
"""The stretch between one scan's Ceres and the next scan's score kernel, from a rocprofv3 kernel trace of bench.py.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python bench.py --gpus 1 --steps 50 --warmup 5
    python tools/critical_path.py DIR [--host-prep-log FILE] > profiles/critical_path_<when>.json

Per step (medians over the steps of the trace, microseconds):
  a               end of the last csm_final_reduce_kernel of step k -> start of the score kernel of step k + 1
  b               inside a: end of the last insertion kernel -> start of the first kernel behind it (the extent pre-pass)
  reduce_to_insert  end of that reduce kernel -> start of the first insertion kernel (host: Ceres' return, the caller)
  insert          first insertion kernel's start -> last one's end, and the kernels' own durations
  extent, extent_to_score, clear (multi_insert_kernel<4>)
--host-prep-log: stderr of a run on an experiments build with DLIOM_HOST_PREP_TIMING=1 (rtcsm3d.hip: HostPrepClock).
"""
import csv
import glob
import json
import os
import re
import statistics
import sys


def rows_of(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def med(v):
    return round(statistics.median(v), 2) if v else None


def main():
    args = sys.argv[1:]
    host_log = None
    if "--host-prep-log" in args:
        i = args.index("--host-prep-log")
        host_log = args[i + 1]
        del args[i:i + 2]
    rows = rows_of(args[0])
    score = [i for i, r in enumerate(rows) if "rtcsm_score" in r[2]]
    out = {k: [] for k in ("a", "b", "reduce_to_insert", "insert", "insert_kernels", "clear", "extent", "extent_to_score",
                           "clear_end_to_score", "score")}
    for s_prev, s in zip(score, score[1:]):
        between = rows[s_prev + 1:s]
        red = [r for r in between if "csm_final_reduce" in r[2]]
        ins = [r for r in between if "multi_insert_kernel" in r[2]]
        ext = [r for r in between if "rtcsm_box_extent" in r[2] or "rtcsm_prep_kernel" in r[2]]
        if not red or not ins or not ext:
            continue
        t_red = max(r[1] for r in red)
        out["a"].append((rows[s][0] - t_red) / 1e3)
        ins_end = max(r[1] for r in ins)
        behind = [r for r in between if r[0] >= ins_end and "multi_insert_kernel" not in r[2]]
        nxt = min([r[0] for r in behind] + [rows[s][0]])
        out["b"].append((nxt - ins_end) / 1e3)
        out["reduce_to_insert"].append((min(r[0] for r in ins) - t_red) / 1e3)
        out["insert"].append((ins_end - min(r[0] for r in ins)) / 1e3)
        out["insert_kernels"].append(sum(r[1] - r[0] for r in ins) / 1e3)
        clear = [r for r in ins if "<4>" in r[2] or "4>" in r[2].split("(")[0]]
        if clear:
            out["clear"].append(sum(r[1] - r[0] for r in clear) / 1e3)
            out["clear_end_to_score"].append((rows[s][0] - max(r[1] for r in clear)) / 1e3)
        out["extent"].append(sum(r[1] - r[0] for r in ext) / 1e3)
        out["extent_to_score"].append((rows[s][0] - max(r[1] for r in ext)) / 1e3)
        out["score"].append((rows[s][1] - rows[s][0]) / 1e3)
    result = {"unit": "us", "steps": len(out["a"]), "median": {k: med(v) for k, v in out.items()},
              "min": {k: (round(min(v), 2) if v else None) for k, v in out.items()},
              "kernel_names_between": sorted({re.sub(r"\(.*", "", r[2]) for s_prev, s in zip(score[:3], score[1:4])
                                              for r in rows[s_prev + 1:s]})}
    if host_log and os.path.exists(host_log):
        m = re.search(r"rtcsm host prep: matches (\d+) mean_us ([\d.]+) median_us ([\d.]+) min_us ([\d.]+)(?: lap_medians_us([\d. ]+))?",
                      open(host_log).read())
        if m:
            result["host_prep_us"] = {"matches": int(m.group(1)), "mean": float(m.group(2)), "median": float(m.group(3)),
                                      "min": float(m.group(4))}
            if m.group(5):  # cumulative, from match_begin's entry (rtcsm3d.hip: HostPrepClock)
                names = ("candidates", "tables_staged", "mirror_and_morton", "box_tables", "span_opened", "first_launch")
                result["host_prep_us"]["lap_medians"] = dict(zip(names, (float(v) for v in m.group(5).split())))
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
