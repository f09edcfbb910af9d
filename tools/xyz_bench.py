#!/usr/bin/env python3
"""XYZ text of one export batch (the action "write_xyz"): the device call against the reference's loop.

Batches: the map-frame points of one 64 x 1024 and one 128 x 2048 scan, in the cube and the ground scene.  Per batch:
  device_ms      dliom_points_batch_pack_xyz into a buffer of 39 n bytes -- sizing, scan, read-back of the size, emit and the
                 download of the text -- median of --repeats warm calls
  size_only_ms   the same call with bytes = NULL: sizing, scan and the read-back
  reference_ms   tests/cpp/xyz_writer_model.cc: one std::ostringstream a point, one thread
  host_loop_ms   tools/xyz_host_loop.cc: one thread over dliom_float_text
The three texts are checked equal in the run.  There is no gate on any ratio.

--profile adds, per batch, the share of coordinates that take float_text.h's multiword path, and once the kernels' VGPRs,
scratch, LDS and occupancy as hipcc reports them for points_text.hip.  --kernel-stats CSV adds the sizing / scan / emit
split from the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool (a run of its own: its timings
are not used).  Lines go to stdout and, with --out, to a file (profiles/xyz_bench.txt)."""
import argparse
import csv
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import xyz_text_common as xt  # noqa: E402

f32 = np.float32


def batch_points(scene, beams, azimuths):
    from dliom import synth
    with synth.scene(scene, trajectory=False):
        pose = synth.trajectory_pose(0.30)
        pts, _ = synth.scan(pose, beams, azimuths)
        return np.ascontiguousarray(synth.transform_points(pose, pts), dtype=f32)


def build_host_loop(directory, lib_path):
    exe = os.path.join(directory, "xyz_host_loop")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tools", "xyz_host_loop.cc"), lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)])
    return exe


def median_ms(call, repeats):
    for _ in range(3):
        call()
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        samples.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(samples)


def multiword_share(pts):
    a = np.abs(pts.astype(np.float64).reshape(-1))
    wide = np.isfinite(a) & (a != 0) & ((a < 1e-8) | (a >= 1e19))  # outside -8 <= X0 <= 18, up to the estimate's slack
    return float(np.mean(wide))


def bench(dl, ctx, model, loop, directory, scene, beams, azimuths, repeats, profile):
    import ctypes as C
    pts = batch_points(scene, beams, azimuths)
    n = len(pts)
    batch = dl.PointsBatch(ctx, pts)
    L = dl.load_library()
    out = np.zeros(dl.XYZ_MAX_RECORD * n, dtype=np.uint8)
    num = C.c_int64()
    u8p = out.ctypes.data_as(C.POINTER(C.c_uint8))

    def full():
        assert L.dliom_points_batch_pack_xyz(batch.h, u8p, len(out), C.byref(num)) == dl.OK

    def size_only():
        assert L.dliom_points_batch_pack_xyz(batch.h, None, 0, C.byref(num)) == dl.OK

    device_ms, size_ms = median_ms(full, repeats), median_ms(size_only, repeats)
    full()
    text = out[:num.value].tobytes()
    want, reference_ms = xt.run_model(model, pts, directory, timing=True)
    src, dst = os.path.join(directory, "xyz_in.bin"), os.path.join(directory, "xyz_loop.txt")
    host_loop_ms = float(subprocess.check_output([loop, src, dst]).decode())
    assert text == want, "the device's text differs from the reference's"
    assert open(dst, "rb").read() == want, "dliom_float_text's text differs from the reference's"
    batch.close()
    line = ("scene=%s scan=%dx%d points=%d text_bytes=%d bytes_per_point=%.2f device_ms=%.4f size_only_ms=%.4f reference_ms=%.3f "
            "host_loop_ms=%.3f reference_over_device=%.1f equal=yes" %
            (scene, beams, azimuths, n, len(want), len(want) / max(n, 1), device_ms, size_ms, reference_ms, host_loop_ms,
             reference_ms / device_ms))
    if profile:
        line += " multiword_share=%.6f" % multiword_share(pts)
    return line


def compile_report():
    """VGPRs, scratch, LDS and occupancy of points_text.hip's kernels, from hipcc's resource remarks."""
    pkg = os.path.join(ROOT, "d-liom_amd")
    with tempfile.TemporaryDirectory() as d:
        done = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                               "-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage", "-c",
                               os.path.join(pkg, "csrc", "points_text.hip"), "-o", os.path.join(d, "points_text.o")],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if done.returncode != 0:
        return ["compile: not measured (hipcc failed)"]
    lines, name = [], None
    for row in done.stdout.decode().splitlines():
        m = re.search(r"Function Name: (\S+)", row)
        if m:
            name = "xyz_size_kernel" if "xyz_size_kernel" in m.group(1) else "xyz_emit_kernel" if "xyz_emit_kernel" in m.group(1) else None
            if name:
                lines.append("compile kernel=%s" % name)
        elif name:
            m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", row)
            if m:
                lines[-1] += " %s=%s" % (m.group(1).split(" ")[0], m.group(2))
    return lines


def kernel_split(path):
    """rocprofv3's kernel_stats.csv -> one line a kernel of the XYZ call: calls, total microseconds, share among them"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            kind = ("sizing" if "xyz_size_kernel" in name else "emit" if "xyz_emit_kernel" in name else
                    "scan" if "scan" in name.lower() else None)
            if kind:
                rows.append((kind, int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3))
    total = sum(r[2] for r in rows) or 1.0
    out = {}
    for kind, calls, us in rows:
        c, u = out.get(kind, (0, 0.0))
        out[kind] = (c + calls, u + us)
    return ["split kernel=%s calls=%d total_us=%.1f share=%.3f" % (k, c, u, u / total) for k, (c, u) in sorted(out.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kernel-stats", default="", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out")
    args = ap.parse_args()
    import dliom as dl
    ctx = dl.Context(0)
    lines = ["# python tools/xyz_bench.py%s: one MI355X, one process; medians of %d warm calls; host loops on one thread" %
             (" --profile" if args.profile else "", args.repeats)]
    print(lines[0], flush=True)
    with tempfile.TemporaryDirectory() as directory:
        model = xt.build_model(directory)
        loop = build_host_loop(directory, dl.LIB_PATH)
        for scene in ("cube", "ground"):
            for beams, azimuths in ((64, 1024), (128, 2048)):
                lines.append(bench(dl, ctx, model, loop, directory, scene, beams, azimuths, args.repeats, args.profile))
                print(lines[-1], flush=True)
    if args.profile:
        for line in compile_report():
            lines.append(line)
            print(line, flush=True)
    if args.kernel_stats:
        for line in kernel_split(args.kernel_stats):
            lines.append(line)
            print(line, flush=True)
    elif args.profile:
        lines.append("split: not measured in this run (needs --kernel-stats from a rocprofv3 --kernel-trace --stats run)")
        print(lines[-1], flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
