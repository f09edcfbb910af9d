#!/usr/bin/env python3
"""Compression of trajectory node clouds on the device (dliom_clouds_compress, dliom_clouds_compress_to_proto) against the
one-thread C++ restatement of the statement (tests/cpp/compressed_cloud_model.cc) on the same clouds, checked equal
before anything is timed.

Two workloads: 2 000 nodes x 3 clouds of 100-400 points in ONE batch (the shape of SerializeState: adaptively filtered
scans of the cube scene, a node's clouds around its pose), and one cloud of 65 536 points.  The clouds are on the device
before the clock starts, as a node's are.  Times are medians of warm calls, host wall clock around the call (each ends
in its own read-back, so it has finished when it returns); the query-then-fill wrappers of the Python mirror are not
used, a call is ONE call of the C function with a buffer that is large enough.  Prints one JSON line per workload.

--profile: a plain run, then the same under `rocprofv3 --kernel-trace`, each a fresh child under `timeout -k 10` (no
child is started after a failure; this process never opens the GPU), and the kernel time of a proto call split into
keys / sort / emission / packing by the order of the launches; written to --out as well."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
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


def node_clouds(nodes, seed=1):
    """3 clouds a node, 100-400 points each: points of the walls of a 40 m room seen from a pose on a slow loop."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(nodes):
        centre = np.array([12 * np.cos(0.01 * i), 12 * np.sin(0.01 * i), 0.3 * np.sin(0.05 * i)])
        for _ in range(3):
            n = int(rng.randint(100, 401))
            d = rng.normal(size=(n, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            world = centre + d * rng.uniform(2.0, 20.0, size=(n, 1))
            out.append(np.clip(world, -20, 20).astype(np.float32) - centre.astype(np.float32))
    return out


def big_cloud(n=65536, seed=2):
    return np.random.RandomState(seed).uniform(-40, 40, size=(n, 3)).astype(np.float32)


def raw_call(fn, ctx, handles, k, out, offsets):
    refused = C.c_int(-1)
    pointer = out.ctypes.data_as(C.POINTER(C.c_int32 if out.dtype == np.int32 else C.c_uint8))
    status = fn(ctx.h, handles, k, pointer, out.size, offsets.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(refused))
    if status != 0:
        raise RuntimeError("status %d, first refused %d" % (status, refused.value))


def bench(dl, ctx, cc, model, directory, name, arrays, calls, with_model):
    L = ctx._L
    clouds = [dl.PointCloud(ctx, a) for a in arrays]
    k, points = len(clouds), sum(len(a) for a in arrays)
    handles = (C.c_void_p * k)(*[c.h for c in clouds])
    offsets = np.zeros(k + 1, dtype=np.int64)
    words = np.zeros(5 * points, dtype=np.int32)
    raw_call(L.dliom_clouds_compress, ctx, handles, k, words, offsets)
    word_offsets = offsets.copy()
    out = dict(tool="compressed_cloud_bench", workload=name, clouds=k, points=points, words=int(word_offsets[k]),
               blocks=int(word_offsets[k] - points) // 4)
    if with_model:
        want, model_ms = cc.run_cpp_model(model, directory, arrays, repeats=5)
        equal = all(w is not None and word_offsets[i + 1] - word_offsets[i] == len(w[1]) and
                    np.array_equal(words[word_offsets[i]:word_offsets[i + 1]], w[1]) for i, w in enumerate(want))
        out["equal_to_model"] = bool(equal)
        assert equal, "device and model differ"
        out["model_ms"] = model_ms
        out["model_clouds_per_s"] = 1e3 * k / model_ms
    # the bytes: sized by a query, equal to the Python mirror's framing of the words for a few clouds
    L.dliom_clouds_compress_to_proto(ctx.h, handles, k, None, 0, offsets.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(C.c_int()))
    data = np.zeros(int(offsets[k]), dtype=np.uint8)
    raw_call(L.dliom_clouds_compress_to_proto, ctx, handles, k, data, offsets)
    for i in sorted({0, k // 2, k - 1}):
        framed = dl.compressed_point_cloud_to_proto(len(arrays[i]), words[word_offsets[i]:word_offsets[i + 1]])
        assert data[offsets[i]:offsets[i + 1]].tobytes() == framed, "bytes and framed words differ"
    out["proto_bytes"] = int(offsets[k])

    def median_ms(fn, buffer):
        for _ in range(3):
            raw_call(fn, ctx, handles, k, buffer, offsets)
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            raw_call(fn, ctx, handles, k, buffer, offsets)
            t.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(t), min(t), max(t)
    for key, fn, buffer in (("words", L.dliom_clouds_compress, words), ("proto", L.dliom_clouds_compress_to_proto, data)):
        med, lo, hi = median_ms(fn, buffer)
        out[key + "_ms_per_call"] = med
        out[key + "_ms_least_most"] = [lo, hi]
        out[key + "_clouds_per_s"] = 1e3 * k / med
    for c in clouds:
        c.close()
    return out


STAGES = ("keys", "sort", "emission", "packing")


def split_by_launch_order(rows):
    """Microseconds a call in each stage: a call's launches are keys, the sort's kernels, heads .. emit (emission), then
    the byte scan, the byte offsets and the pack kernel (packing)."""
    rows = sorted(rows, key=lambda r: int(r["Start_Timestamp"]))
    calls, stage = [], None
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "compress_keys_kernel" in name:
            calls.append(dict.fromkeys(STAGES, 0.0))
            stage = "keys"
        elif stage is None:
            continue
        elif "compress_heads_kernel" in name:
            stage = "emission"
        elif "decompress_kernel" in name or "fill_multi" in name:
            stage = None
            continue
        elif stage == "keys":
            stage = "sort"
        calls[-1][stage] += us
        if "compress_emit_kernel" in name:
            stage = "packing"
        elif "compress_pack_kernel" in name:
            stage = None
    return calls


def profile(args):
    me = os.path.abspath(__file__)
    plain = subprocess.run(["timeout", "-k", "10", "500", sys.executable, me, "--calls", str(args.calls)], capture_output=True, text=True)
    if plain.returncode != 0:
        raise RuntimeError("plain run: exit status %d; stopping here. %s" % (plain.returncode, plain.stderr[-400:]))
    directory = tempfile.mkdtemp(prefix="compressed_cloud_profile_")
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    traced = subprocess.run(["timeout", "-k", "10", "500", rocprof, "--kernel-trace", "--output-format", "csv", "-d", directory, "-o", "cc",
                             "--", sys.executable, me, "--calls", "5", "--no-model", "--proto-only"], capture_output=True, text=True)
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if traced.returncode != 0 or not files:
        raise RuntimeError("kernel trace: exit status %d, %d result files; stopping here. %s" %
                           (traced.returncode, len(files), traced.stderr[-400:]))
    rows = [row for f in files for row in csv.DictReader(open(f))]
    calls = split_by_launch_order(rows)
    # --proto-only runs 8 proto calls a workload and nothing else that compresses: the nodes' calls, then the big cloud's
    lines = [l for l in plain.stdout.splitlines() if l.startswith("{")]
    half = len(calls) // 2
    for name, part in (("nodes", calls[:half]), ("big", calls[half:])):
        warm = part[3:]
        split = {s: statistics.median(c[s] for c in warm) for s in STAGES}
        lines.append(json.dumps(dict(tool="compressed_cloud_bench", workload=name, kernel_us_per_proto_call=split,
                                     kernel_us_total=sum(split.values()), traced_calls=len(warm))))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    shutil.rmtree(directory, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--proto-only", action="store_true", help="3 + --calls proto calls a workload and nothing else (for the kernel trace)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compressed_cloud_bench.txt"))
    args = ap.parse_args()
    if args.profile:
        profile(args)
        return
    import dliom as dl
    import compressed_cloud_common as cc
    ctx = dl.Context(0)
    workloads = (("nodes", node_clouds(args.nodes)), ("big", [big_cloud()]))
    if args.proto_only:
        for _, arrays in workloads:
            clouds = [dl.PointCloud(ctx, a) for a in arrays]
            handles = (C.c_void_p * len(clouds))(*[c.h for c in clouds])
            data, offsets = np.zeros(45 * sum(len(a) for a in arrays) + 16 * len(clouds), dtype=np.uint8), np.zeros(len(clouds) + 1, dtype=np.int64)
            for _ in range(3 + args.calls):
                raw_call(ctx._L.dliom_clouds_compress_to_proto, ctx, handles, len(clouds), data, offsets)
        ctx.close()
        return
    directory = tempfile.mkdtemp(prefix="compressed_cloud_bench_")
    model = None if args.no_model else cc.build_cpp_model(directory)
    for name, arrays in workloads:
        print(json.dumps(bench(dl, ctx, cc, model, directory, name, arrays, args.calls, not args.no_model)), flush=True)
    shutil.rmtree(directory, ignore_errors=True)
    ctx.close()


if __name__ == "__main__":
    main()
