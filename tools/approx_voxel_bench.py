"""dliom_cloud_approximate_voxel_filter and dliom_ndt_scan_matcher against what the adapter did before them.  Both scene
families, 64 x 1024 and 128 x 2048 scans taken at trajectory_pose(0.30) (previous) and (0.35) (current).  A line of JSON a
case, from tools/approx_voxel_bench.cc (built here with g++ against libdliom.so):
  the filter on a cloud that lies in HBM, against download + registration::ApproximateVoxelGrid on one host thread + upload,
  checked equal;
  a MatchByNDT pair through registration::NdtScanMatcher (previous cells kept, one device filter) against
  registration::MatchByNDT (two host filters, two uploads, a target a pair), checked equal, in ms a pair, and the matcher's
  stages (filter, alignment, cells) one C call each.
Every list holds the repeated calls after the warm-up ones; median and the spread are added.
usage: python tools/approx_voxel_bench.py [--scenes cube ground] [--sizes 64x1024 128x2048] [--warmup 2] [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))
from dliom import synth  # noqa: E402

HEADER = """# python tools/approx_voxel_bench.py
# one MI355X, one run; host clock around calls that end in a device synchronise; *_ms lists: the repeated calls after the warm-up
# calls, in order; median / min / max beside them.  The host column is the adapter's one-thread loop with its download and upload.
"""


def summary(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "ground"])
    ap.add_argument("--sizes", nargs="+", default=["64x1024", "128x2048"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_voxel_bench.txt"))
    args = ap.parse_args()
    libdir = os.path.join(ROOT, "d-liom_amd")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "approx_voxel_bench")
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-DNDEBUG", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(libdir, "cpp"), "-o", exe, os.path.join(ROOT, "tools", "approx_voxel_bench.cc"),
                               "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
        for scene in args.scenes:
            for size in args.sizes:
                beams, azimuths = (int(v) for v in size.split("x"))
                with synth.scene(scene, trajectory=False):
                    previous = synth.scan(synth.trajectory_pose(0.30), beams, azimuths)[0]
                    current = synth.scan(synth.trajectory_pose(0.35), beams, azimuths)[0]
                paths = [os.path.join(tmp, "previous.bin"), os.path.join(tmp, "current.bin")]
                for path, cloud in zip(paths, (previous, current)):
                    with open(path, "wb") as f:
                        f.write(np.ascontiguousarray(cloud, np.float32).tobytes())
                run = subprocess.run([exe] + paths + [str(args.warmup), str(args.repeats)], stdout=subprocess.PIPE, universal_newlines=True)
                line = dict(scene=scene, scan=size, exit_status=run.returncode)
                line.update(json.loads(run.stdout))
                for key in [k for k in line if k.endswith("_ms")]:
                    line[key[:-3] + "_summary_ms"] = summary(line[key])
                print(json.dumps(line), flush=True)
                lines.append(json.dumps(line))
                if run.returncode != 0:
                    raise SystemExit("results differ: " + scene + " " + size)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(HEADER + "".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
