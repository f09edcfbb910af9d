"""K nearest-neighbour indices built by a serial loop of dliom_nn_index_create against one dliom_nn_index_create_batch, in one
process.  Scenes and sizes as in tools/icp_batch_bench.py (cube and ground, 64 x 1024), raw and filtered by
dliom_cloud_voxel_filter at 0.6 m; target k is the scan at trajectory_pose(0.30 + 0.01 k), K distinct targets along the
trajectory, as the ground-truth tool's constraints have.  The two are checked equal before anything is timed: by the memory
statistics and by a query of each target cloud against its own index, bit for bit.  Then one warm-up of each and --repeats
alternating repetitions; a host clock around calls that end in a stream synchronisation; medians.  A line of JSON a case:
ms a call and indices/s of both, read-backs, the batch's box / sort / alloc split from one more, profiled call, and the
builds' share of build + dliom_icp_align_batch (the sources: the scans at trajectory_pose(0.35 + 0.01 k), the 30 m preset).

    python tools/nn_index_batch_bench.py [--scenes cube ground] [--indices 1 4 16 64] [--repeats 5] [--voxel 0.6]

--single N: instead, N calls of dliom_nn_index_create on the cube's raw 64 x 1024 scan through the library that --lib (or
DLIOM_LIB) names, bound with ctypes alone so that a library of an earlier commit loads too; one JSON line with the median.
Three alternating processes of 40 calls on each of two libraries are the A/B of DESIGN.md 3.28."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "d-liom_amd"))

MEMORY_FIELDS = ("points", "finite_points", "cells", "dims", "cell_edge", "index_bytes")
STAGES = ("box_ms", "sort_ms", "alloc_ms")


def single_build(lib_path, calls):
    from dliom import synth
    with synth.scene("cube", trajectory=False):
        scan = np.ascontiguousarray(synth.scan(synth.trajectory_pose(0.30), 64, 1024)[0], np.float32)
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.dliom_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.dliom_cloud_create.argtypes = [vp, C.c_void_p, C.c_int64, C.POINTER(vp)]
    L.dliom_nn_index_create.argtypes = [vp, vp, C.c_void_p, C.POINTER(vp)]
    for name in ("dliom_nn_index_destroy", "dliom_cloud_destroy", "dliom_ctx_destroy"):
        getattr(L, name).argtypes = [vp]
    ctx, cloud = vp(), vp()
    assert L.dliom_ctx_create(0, C.byref(ctx)) == 0
    assert L.dliom_cloud_create(ctx, scan.ctypes.data, len(scan), C.byref(cloud)) == 0
    ms = []
    for k in range(calls + 3):  # three warm-ups: code loading, the first allocations
        index = vp()
        t = time.perf_counter()
        status = L.dliom_nn_index_create(ctx, cloud, None, C.byref(index))
        elapsed = (time.perf_counter() - t) * 1e3
        assert status == 0
        L.dliom_nn_index_destroy(index)
        if k >= 3:
            ms.append(elapsed)
    L.dliom_cloud_destroy(cloud)
    L.dliom_ctx_destroy(ctx)
    print(json.dumps(dict(lib=lib_path, points=len(scan), calls=calls, median_ms=statistics.median(ms), min_ms=min(ms),
                          max_ms=max(ms))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cube", "ground"])
    ap.add_argument("--size", default="64x1024")
    ap.add_argument("--indices", nargs="+", type=int, default=[1, 4, 16, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxel", type=float, default=0.6)
    ap.add_argument("--single", type=int, default=0)
    ap.add_argument("--lib", default=os.environ.get("DLIOM_LIB") or os.path.join(ROOT, "d-liom_amd", "libdliom.so"))
    args = ap.parse_args()
    if args.single > 0:
        return single_build(args.lib, args.single)
    import icp_batch_common as bc
    import dliom as dl
    from dliom import synth

    beams, azimuths = (int(v) for v in args.size.split("x"))
    most = max(args.indices)
    ctx = dl.Context(0)
    options = dl.ground_truth_icp_options()
    limits = dl.nn_index_batch_default_limits(max_indices_in_flight=min(most, dl.NN_INDEX_BATCH_MAX_INDICES), max_points_in_flight=1 << 30)
    icp_limits = dl.icp_batch_default_limits(max_pairs_in_flight=min(most, dl.ICP_BATCH_MAX_PAIRS), max_scratch_bytes=8 << 30)

    def serial(clouds):
        return [dl.NnIndex(ctx, c) for c in clouds]

    def close(indices):
        for index in indices:
            index.close()

    for scene in args.scenes:
        with synth.scene(scene, trajectory=False):
            scans = [[synth.scan(synth.trajectory_pose(t0 + 0.01 * k), beams, azimuths)[0] for k in range(most)] for t0 in (0.30, 0.35)]
        for voxel in (0.0, args.voxel):
            targets, sources = [[dl.PointCloud(ctx, s) for s in group] for group in scans]
            if voxel > 0.0:
                for group in (targets, sources):
                    filtered = [c.voxel_filter(voxel) for c in group]
                    close(group)
                    group[:] = filtered
            for count in args.indices:
                clouds = targets[:count]
                single = serial(clouds)  # warm-up of the loop
                batched, stats = dl.nn_indices_batch(ctx, clouds, limits=limits)  # warm-up of the batch
                for k, (a, b, cloud) in enumerate(zip(batched, single, clouds)):
                    ma, mb = a.memory_stats(), b.memory_stats()
                    qa, qb = a.query(cloud), b.query(cloud)
                    if [ma[f] for f in MEMORY_FIELDS] != [mb[f] for f in MEMORY_FIELDS] or not np.array_equal(qa[0], qb[0]) or \
                            not bc.same_bits(qa[1], qb[1]) or any(qa[2][f] != qb[2][f] for f in ("non_finite", "settled_by_grid", "settled_by_brute_force")):
                        raise SystemExit("batch and serial loop differ at index %d" % k)
                close(single)
                serial_ms, batch_ms = [], []
                before = ctx.read_backs()
                for _ in range(args.repeats):  # alternating: both see the same neighbours on the machine
                    t = time.perf_counter()
                    built = serial(clouds)
                    serial_ms.append((time.perf_counter() - t) * 1e3)
                    close(built)
                    t = time.perf_counter()
                    built, _ = dl.nn_indices_batch(ctx, clouds, limits=limits)
                    batch_ms.append((time.perf_counter() - t) * 1e3)
                    close(built)
                read_backs = ctx.read_backs() - before
                ctx.set_profiling(1)
                built, staged = dl.nn_indices_batch(ctx, clouds, limits=limits)
                ctx.set_profiling(0)
                close(built)
                pairs = [(index, source, None) for index, source in zip(batched, sources[:count])]
                dl.icp_align_batch(ctx, pairs, options, icp_limits)  # warm-up
                align_ms = []
                for _ in range(3):
                    t = time.perf_counter()
                    dl.icp_align_batch(ctx, pairs, options, icp_limits)
                    align_ms.append((time.perf_counter() - t) * 1e3)
                close(batched)
                s, b, a = statistics.median(serial_ms), statistics.median(batch_ms), statistics.median(align_ms)
                print(json.dumps(dict(
                    scene=scene, scan=args.size, voxel_filter=voxel, indices=count, target_points=int(np.mean([c.n for c in clouds])),
                    cells=stats["cells"], builds_equal=True, serial_ms=s, batch_ms=b, batch_over_serial=b / s, serial_ms_calls=serial_ms,
                    batch_ms_calls=batch_ms, serial_indices_per_s=count / s * 1e3, batch_indices_per_s=count / b * 1e3,
                    serial_ms_per_index=s / count, batch_ms_per_index=b / count,
                    serial_read_backs=count, batch_read_backs=stats["read_backs"], read_backs_of_the_timed_loops=read_backs,
                    batch_chunks=stats["chunks"], batch_cell_runs=stats["cell_runs"], batch_scratch_bytes=stats["scratch_bytes"],
                    batch_stages_ms={k: staged[k] for k in STAGES}, icp_align_batch_ms=a,
                    serial_build_share=s / (s + a), batch_build_share=b / (b + a))), flush=True)
            close(targets)
            close(sources)
    ctx.close()


if __name__ == "__main__":
    main()
