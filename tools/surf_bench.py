#!/usr/bin/env python3
"""Submap image features (dliom.h "submap image features") on the three grids of tools/xray_bench.py: a front end's
finished submap (0.10 m and its 0.45 m twin) and BASELINE config 5's 0.05 m grid.  Per grid: the projected image's size,
the key points, milliseconds a call of dliom_surf_detect_and_compute (host image in, features out; median of --reps
after a first call that reserves the scratch) and of dliom_feature_index_add_from_grid (projection included, nothing
leaves HBM), and of the CPU model (tests/cpp/surf_model.cc) on one thread, process start and file I/O included; checks
that device and model give the same bytes.  The CPU column is this repository's model and NOT OpenCV: there is no
parent path and no reference timing.  One JSON line per grid.

--profile: milliseconds a kernel as well.  The tool then opens no GPU itself: it starts itself once plainly and once
under `rocprofv3 --kernel-trace --stats` (--reps 5), each a fresh child under `timeout -k 10`, stops at the first child
that fails, and writes the plain run's lines and the per-kernel rows (per launch size: calls, mean, least, most
microseconds) to --out (profiles/surf_bench.txt)."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


HEADER = """# python tools/surf_bench.py --profile
# Median of --reps calls after a first call that reserves the scratch.  The CPU column is tests/cpp/surf_model.cc on one
# thread, process start and file I/O included: this repository's model, NOT OpenCV (no parent path, no reference timing).
"""


def kernel_name(full):
    found = re.search(r"(surf_[a-z_]+_kernel|feature_keypoints_xy_kernel|xray_[a-z_]+_kernel|fill_multi_kernel|gather_to_pinned_kernel)", full)
    if found:
        return found.group(1)
    if "rocprim" in full:
        stage = re.search(r"wrapped_([a-z_]+)_config", full)
        return "hipcub sort or scan: " + (stage.group(1) if stage else "other")
    return None  # the front end's and the scene's kernels: not this feature's


def profile(args):
    """Two children, neither started after a failure; this process never opens the GPU."""
    me = os.path.abspath(__file__)
    plain = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "--reps", str(args.reps)], capture_output=True, text=True)
    if plain.returncode != 0:
        raise RuntimeError("plain run: exit status %d; stopping here. %s" % (plain.returncode, plain.stderr[-400:]))
    directory = tempfile.mkdtemp(prefix="surf_profile_")
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    traced = subprocess.run(["timeout", "-k", "10", "400", rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory,
                             "-o", "surf", "--", sys.executable, me, "--reps", "5"], capture_output=True, text=True)
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if traced.returncode != 0 or not files:
        raise RuntimeError("kernel trace: exit status %d, %d result files; stopping here. %s" %
                           (traced.returncode, len(files), traced.stderr[-400:]))
    durations = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = kernel_name(row["Kernel_Name"])
            if name is None:
                continue
            size = (int(row.get("Grid_Size_X", 0)), int(row.get("Grid_Size_Y", 1))) if name.startswith("surf_") else (0, 0)
            durations.setdefault((name, size), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    lines = [HEADER.rstrip("\n")] + [l for l in plain.stdout.splitlines() if l.startswith("{")]
    lines += ["#", "# rocprofv3 --kernel-trace --stats -- python tools/surf_bench.py --reps 5: microseconds a launch, per kernel and (for",
              "# this feature's own kernels) launch size in lanes x blockIdx.y -- the three images in the order above give three",
              "# sizes a kernel.  The other rows are the projection's, the index's and the context's helpers in the same run."]
    for (name, size), v in sorted(durations.items()):
        where = "grid %7d x %2d" % size if size != (0, 0) else " " * 17
        lines.append("%-44s %s  calls %4d  mean %7.1f us  least %7.1f  most %7.1f" % (name, where, len(v), sum(v) / len(v), min(v), max(v)))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    shutil.rmtree(directory, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surf_bench.txt"))
    args = ap.parse_args()
    if args.profile:
        profile(args)
        return
    import dliom as dl
    from dliom import synth
    from benchlib.config5 import config5_scene
    import surf_common as sc
    from xray_bench import front_end_submap
    tmp = tempfile.mkdtemp(prefix="surf_bench_")
    model = sc.build_model(tmp)
    ctx = dl.Context(0)
    sub = front_end_submap(dl, ctx)
    _, c5_grids, scene, _ = config5_scene(dl, synth, ctx)
    pose = list(sub["local_pose"])
    grids = [("front_end_0.10", sub["hi"]), ("front_end_0.45", sub["lo"]), ("config5_0.05", c5_grids[0])]
    options, device_options = sc.Options(), sc.Options().device(dl)
    ok = True
    for name, g in grids:
        image, ox, oy, resolution = dl.grid_project_to_image(g, pose)
        kp, desc = dl.surf_detect_and_compute(ctx, image, device_options)  # reserves the scratch
        detect_ms = median_ms(lambda: dl.surf_detect_and_compute(ctx, image, device_options, capacity=len(kp)), args.reps)
        index = dl.FeatureIndex(ctx, 64)

        def from_grid():
            index.add_from_grid(1, g, pose, device_options)
            index.remove(1)
        from_grid()
        grid_ms = median_ms(from_grid, args.reps)
        project_ms = median_ms(lambda: dl.grid_project_to_image(g, pose), args.reps)
        index.close()
        seconds = []
        status, count, want_kp, want_desc = sc.model_detect_and_compute(model, tmp, image, options, timing=seconds)
        equal = bool(status == sc.OK and kp.tobytes() == want_kp.tobytes() and desc.tobytes() == want_desc.tobytes())
        ok &= equal
        print(json.dumps(dict(grid=name, image_width=int(image.shape[1]), image_height=int(image.shape[0]), keypoints=int(len(kp)),
                              octaves=sorted(set(int(v) for v in kp[:, 5])), detect_and_compute_ms=round(detect_ms, 3),
                              add_from_grid_and_remove_ms=round(grid_ms, 3), project_to_image_to_host_ms=round(project_ms, 3),
                              model_one_thread_ms=round(seconds[0] * 1e3, 2), equal=equal)), flush=True)
    for g in c5_grids:
        g.close()
    scene["cloud"].close()
    sub["hi"].close()
    sub["lo"].close()
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
