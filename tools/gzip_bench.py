#!/usr/bin/env python3
"""Gzip on the device (dliom.h "gzip on the device") against zlib level 1 on one host thread, the reference's
common::FastGzipString.

1. textures  a grid of the cube and of the ground scene (the cells a 128 x 2048 scan hits, at the resolution that makes the
             X-ray texture about 600 x 600 and about 2000 x 2000): dliom_grid_xray_texture_gzip against
             dliom_grid_xray_texture followed by zlib.compress(cells, 1), each into pageable memory and into a buffer the
             caller keeps page-locked (dliom_host_register).  ms a texture, bytes downloaded, compressed bytes of both.
2. records   K kept scans of 30 000 returns (tools/node_clouds_bench.py's nodes): NodeClouds.to_pbstream against to_proto
             followed by zlib level 1 and the 8-byte size a message, the same two memory kinds.
Medians of alternating repetitions; before anything is timed the device's bytes are inflated with zlib and compared with
the host path's.  No gate on any ratio.  --profile adds the stored share and the kernels' VGPRs, scratch, LDS and occupancy
as hipcc reports them; the split between the chunk kernel (matches, parse, emit), the scan and the gather is the
kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool.  Lines go to stdout and, with --out, to a file
(profiles/gzip_bench.txt)."""
import argparse
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "d-liom_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

u8p = C.POINTER(C.c_uint8)
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def scene_points(scene):
    from dliom import synth
    with synth.scene(scene, trajectory=False):
        pts, _ = synth.scan(synth.trajectory_pose(0.30), 128, 2048)
    return np.ascontiguousarray(pts, dtype=np.float32)


def scene_grid(dl, ctx, pts, side):
    """the cells the scan hits, at the resolution that makes the larger side of the xy extent `side` cells"""
    extent = float(max(np.ptp(pts[:, 0]), np.ptp(pts[:, 1])))
    resolution = extent / side
    cells = np.unique(np.round(pts / np.float32(resolution)).astype(np.int64), axis=0)
    value = dl.load_library().dliom_probability_to_value(C.c_float(0.9))
    g = dl.HybridGrid(ctx, resolution)
    g.set_values(cells, np.full(len(cells), value, dtype=np.uint16))
    return g


def median_ms(calls, repeats):
    """[median ms] of the calls, run in alternation"""
    times = [[] for _ in calls]
    for _ in range(repeats):
        for k, call in enumerate(calls):
            t0 = time.perf_counter()
            call()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in times]


class Buffer:
    def __init__(self, L, ctx, n, page_locked):
        self.a = np.zeros(max(n, 1), dtype=np.uint8)
        self.p = self.a.ctypes.data_as(u8p)
        self.L, self.ctx, self.locked = L, ctx, page_locked
        if page_locked:
            assert L.dliom_host_register(ctx.h, self.a.ctypes.data, self.a.size) == 0

    def close(self):
        if self.locked:
            self.L.dliom_host_unregister(self.ctx.h, self.a.ctypes.data)


def bench_texture(dl, ctx, grid, repeats):
    L = ctx._L
    pp = IDENTITY.ctypes.data_as(C.POINTER(C.c_double))
    w, h, res, size = C.c_int32(), C.c_int32(), C.c_double(), C.c_int64()
    sl = (C.c_double * 7)()
    stats = dl.GzipStats()
    assert L.dliom_grid_xray_texture(grid.h, pp, None, 0, C.byref(w), C.byref(h), C.byref(res), sl) == 0
    n = 2 * w.value * h.value
    out = {}
    for kind in ("pageable", "page_locked"):
        plain, packed = Buffer(L, ctx, n, kind == "page_locked"), Buffer(L, ctx, dl.gzip_bound(n), kind == "page_locked")
        host = lambda: (L.dliom_grid_xray_texture(grid.h, pp, plain.p, n, C.byref(w), C.byref(h), C.byref(res), sl),
                        zlib.compress(plain.a[:n], 1, 31) if sys.version_info >= (3, 11) else zlib.compress(plain.a[:n], 1))
        device = lambda: L.dliom_grid_xray_texture_gzip(grid.h, pp, packed.p, packed.a.size, C.byref(size), C.byref(w), C.byref(h),
                                                        C.byref(res), sl, C.byref(stats))
        host_result = host()
        assert host_result[0] == 0 and device() == 0
        assert zlib.decompress(packed.a[:size.value].tobytes(), 31) == plain.a[:n].tobytes()
        for _ in range(3):
            host(), device()
        out[kind] = median_ms([host, device], repeats)
        zlib_bytes = len(host_result[1])
        plain.close()
        packed.close()
    return ("texture %d x %d bytes %d | device_gz_bytes %d zlib1_bytes %d stored_chunks %d of %d | pageable: texture+zlib1_ms %.3f "
            "texture_gzip_ms %.3f | page_locked: texture+zlib1_ms %.3f texture_gzip_ms %.3f | downloaded %d against %d"
            % (w.value, h.value, n, size.value, zlib_bytes, stats.chunks_stored, stats.chunks, out["pageable"][0], out["pageable"][1],
               out["page_locked"][0], out["page_locked"][1], size.value, n))


def bench_records(dl, ctx, pts, k, repeats):
    from node_clouds_bench import RETURNS
    L = ctx._L
    cache = dl.NodeClouds(ctx)
    cloud = dl.PointCloud(ctx, pts[:RETURNS])
    for i in range(k):
        cache.add(cloud, None, timestamp=1000 + i, trajectory_id=0, local_pose7=(0.1 * i, 0, 0, 1, 0, 0, 0))
    cloud.close()
    message_capacity = k * (192 + dl.NODE_RANGE_MAX_RECORD * RETURNS)
    record_capacity = k * (8 + dl.gzip_bound(192 + dl.NODE_RANGE_MAX_RECORD * RETURNS))
    offsets, record_offsets = np.zeros(k + 1, dtype=np.int64), np.zeros(k + 1, dtype=np.int64)
    op, rp = offsets.ctypes.data_as(C.POINTER(C.c_int64)), record_offsets.ctypes.data_as(C.POINTER(C.c_int64))
    stats = dl.GzipStats()
    out = {}
    for kind in ("pageable", "page_locked"):
        plain, packed = Buffer(L, ctx, message_capacity, kind == "page_locked"), Buffer(L, ctx, record_capacity, kind == "page_locked")

        def host():
            assert L.dliom_node_clouds_to_proto(cache.h, 0, k, None, plain.p, message_capacity, op, None) == 0
            records = []
            for i in range(k):
                member = zlib.compress(plain.a[offsets[i]:offsets[i + 1]], 1)
                records.append(struct.pack("<q", len(member)) + member)
            return records

        def device():
            assert L.dliom_node_clouds_to_pbstream(cache.h, 0, k, None, packed.p, record_capacity, rp, None, C.byref(stats)) == 0

        records = host()
        device()
        for i in range(k):
            record = packed.a[record_offsets[i]:record_offsets[i + 1]].tobytes()
            assert struct.unpack_from("<q", record)[0] == len(record) - 8
            assert zlib.decompress(record[8:], 31) == plain.a[offsets[i]:offsets[i + 1]].tobytes()
        out[kind] = median_ms([host, device], repeats)
        zlib_bytes = sum(len(r) for r in records)
        plain.close()
        packed.close()
    line = ("records K %d message_bytes %d | device_bytes %d zlib1_bytes %d stored_chunks %d of %d | pageable: to_proto+zlib1_ms %.3f "
            "to_pbstream_ms %.3f | page_locked: to_proto+zlib1_ms %.3f to_pbstream_ms %.3f"
            % (k, int(offsets[k]), int(record_offsets[k]), zlib_bytes, stats.chunks_stored, stats.chunks, out["pageable"][0], out["pageable"][1],
               out["page_locked"][0], out["page_locked"][1]))
    cache.close()
    return line


def kernel_resources():
    """hipcc's -Rpass-analysis=kernel-resource-usage lines for gzip.hip's kernels"""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(ROOT, "d-liom_amd", "csrc", "gzip.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    lines, name = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"\d+(gzip_\w+_kernel)", m.group(1))
            if name:
                lines.append("kernel " + name.group(1))
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            lines[-1] += "  %s %s" % (m.group(1).split(" [")[0], m.group(2))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="*", default=[600, 2000])
    ap.add_argument("--nodes", type=int, nargs="*", default=[1000])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--record-repeats", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_bench.txt"))
    args = ap.parse_args()
    import dliom as dl
    ctx = dl.Context(0)
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    points = {scene: scene_points(scene) for scene in ("cube", "ground")}
    for scene, pts in points.items():
        for side in args.sides:
            grid = scene_grid(dl, ctx, pts, side)
            say("scene %s repeats %d %s" % (scene, args.repeats, bench_texture(dl, ctx, grid, args.repeats)))
            grid.close()
    for k in args.nodes:
        say("scene cube repeats %d %s" % (args.record_repeats, bench_records(dl, ctx, points["cube"], k, args.record_repeats)))
    if args.profile:
        for line in kernel_resources():
            say(line)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
