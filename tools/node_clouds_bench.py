#!/usr/bin/env python3
"""Kept scans in HBM (dliom_node_clouds_*): the map cloud and the range-data file of K nodes, device calls against the
reference's loops.

Nodes: K in {1, 64, 1024} copies of one filtered cloud of 30 000 returns (a 128 x 2048 scan of the cube and of the ground
scene through VoxelFilter(0.15), its first 30 000 points).  tools/node_clouds_bench.cc runs, in one process and in
alternating repetitions,
  pack_point_cloud2   cartographer_ros::NodeCloudCache::FullMapCloud (Node::PublishFullMapCloud's loop: one launch and one
                      download a chunk) against HostPointCloud2Data, the reference's stream.next() loop, one thread
  to_proto            NodeCloudCache::SerializeRangeData (sizing launch, scan, read-back, emit launch, download a chunk)
                      against HostNodeRangeData, sensor::ToProto and the serialisation, one thread
and reports medians: ms a call, points a second, and for to_proto the sizing half (launch, scan and read-back, measured as
the size query) beside the rest (emit launch and download).  page_locked_ms is the C call itself into one buffer the caller
keeps page-locked (dliom_host_register), sized by the bound that needs no size query: no vector made, the download one DMA.  The bytes are checked equal before anything is timed.  There
is no gate on any ratio.  --profile adds the kernels' VGPRs, scratch, LDS and occupancy as hipcc reports them.  Lines go to
stdout and, with --out, to a file (profiles/node_clouds_bench.txt)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

RETURNS = 30000


def filtered_cloud(dl, ctx, scene):
    from dliom import synth
    with synth.scene(scene, trajectory=False):
        pose = synth.trajectory_pose(0.30)
        pts, _ = synth.scan(pose, 128, 2048)
    cloud = dl.PointCloud(ctx, np.ascontiguousarray(pts, dtype=np.float32))
    kept = cloud.voxel_filter(0.15)
    out = kept.download()[:RETURNS]
    cloud.close()
    kept.close()
    return np.ascontiguousarray(out, dtype=np.float32)


def kernel_resources():
    """hipcc's -Rpass-analysis=kernel-resource-usage lines for node_clouds.hip's own kernels"""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(ROOT, "d-liom_amd", "csrc", "node_clouds.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    lines, name = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"\d+(node_\w+_kernel|cloud_pack_kernel|range_\w+_kernel)", m.group(1))
            if name:
                lines.append("kernel " + name.group(1))
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            lines[-1] += "  %s %s" % (m.group(1).split(" [")[0], m.group(2))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--repeats", type=int, default=0, help="0: 41 for K <= 64, 7 beyond")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import dliom as dl
    lib = os.path.join(ROOT, "d-liom_amd")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "node_clouds_bench")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "node_clouds_bench.cc"),
                               "-L", lib, "-ldliom", "-Wl,-rpath," + lib])
        ctx = dl.Context(0)
        clouds = {scene: filtered_cloud(dl, ctx, scene) for scene in ("cube", "ground")}
        ctx.close()
        for scene, pts in clouds.items():
            path = os.path.join(tmp, scene + ".bin")
            with open(path, "wb") as f:
                f.write(np.int32(len(pts)).tobytes() + pts.tobytes())
            for k in args.nodes:
                repeats = args.repeats or (41 if k <= 64 else 7)
                out = subprocess.run([exe, path, str(k), str(repeats)], capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    raise SystemExit("node_clouds_bench failed (%d): %s%s" % (out.returncode, out.stdout, out.stderr))
                lines.append("scene %s repeats %d %s" % (scene, repeats, out.stdout.strip()))
                print(lines[-1], flush=True)
    if args.profile:
        for line in kernel_resources():
            lines.append(line)
            print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
