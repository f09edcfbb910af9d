"""Shared by tests/test_outlier_host.py, tests/test_gpu_outlier.py, tools/fuzz_outlier.py and tools/outlier_bench.py:
builds and runs the CPU model (tests/cpp/outlier_model.cc), and makes the synthetic drives with moving obstacles."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "outlier_model.cc")
MARK, RAYS, FILTER, RANGE, TRACE = 1, 2, 3, 4, 5
f32 = np.float32


def build_model(directory):
    exe = os.path.join(str(directory), "outlier_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def op(kind, points, origin=(0.0, 0.0, 0.0), a=0.0, b=0.0):
    return (kind, np.asarray(origin, dtype=f32), float(a), float(b), np.ascontiguousarray(points, dtype=f32).reshape(-1, 3))


def run_model(exe, voxel_size, ops, directory, timing=False):
    """-> (per op: status | (status, kept indices) | list of (cells, product-form cells) per ray), (xyz, hits, rays)[, text]"""
    src, dst = os.path.join(str(directory), "ops.bin"), os.path.join(str(directory), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<d", voxel_size))
        for kind, origin, a, b, pts in ops:
            f.write(struct.pack("<i3fddi", kind, *[float(v) for v in origin], a, b, len(pts)))
            f.write(pts.tobytes())
    text = subprocess.check_output([exe, src, dst] + (["--time"] if timing else [])).decode()
    data = open(dst, "rb").read()
    at, results = 0, []
    for kind, _, _, _, pts in ops:
        if kind == TRACE:
            rays = []
            for _ in range(len(pts)):
                k = struct.unpack_from("<i", data, at)[0]
                cells = np.frombuffer(data, dtype=np.int32, count=6 * k, offset=at + 4).reshape(k, 2, 3)
                at += 4 + 24 * k
                rays.append((cells[:, 0].copy(), cells[:, 1].copy()))
            results.append(rays)
            continue
        status = struct.unpack_from("<i", data, at)[0]
        at += 4
        if kind in (FILTER, RANGE):
            k = struct.unpack_from("<i", data, at)[0]
            results.append((status, np.frombuffer(data, dtype=np.int32, count=k, offset=at + 4).copy()))
            at += 4 + 4 * k
        else:
            results.append(status)
    count = struct.unpack_from("<q", data, at)[0]
    rows = np.frombuffer(data, dtype=np.int32, count=5 * count, offset=at + 8).reshape(count, 5)
    assert at + 8 + 20 * count == len(data)
    table = (rows[:, :3].copy(), rows[:, 3].copy(), rows[:, 4].copy())
    return (results, table, text) if timing else (results, table)


def three_pass_ops(batches):
    """The reference's stream, restarted twice: every batch marked, then every batch's rays, then every batch filtered."""
    return ([op(MARK, p, o) for o, p in batches] + [op(RAYS, p, o) for o, p in batches] +
            [op(FILTER, p, o) for o, p in batches])


def drive(num_scans, beams, azimuths, movers=8, step=0.12, seed=5):
    """Map-frame batches [(origin float32[3], points float32 (n, 3))] of a sensor on the corkscrew in the closed cube
    scene: 30 static spheres, and `movers` spheres that move 0.7 m between scans across the space the sensor looks
    through, so that later rays pass through the voxels where they stood."""
    from dliom import synth
    rng = np.random.RandomState(seed)
    static = synth.bubbles()[:30]
    start = rng.uniform(-1.0, 1.0, size=(movers, 3))
    start = 4.0 * start / np.linalg.norm(start, axis=1, keepdims=True) + np.array([0.0, 1.0, 0.5])
    heading = rng.uniform(-1.0, 1.0, size=(movers, 3))
    heading = 0.7 * heading / np.linalg.norm(heading, axis=1, keepdims=True)
    batches = []
    for s in range(num_scans):
        pose = synth.trajectory_pose(step * s)
        centers = np.concatenate([static, start + s * heading])
        pts, _ = synth.scan(pose, beams, azimuths, centers=centers)
        batches.append((pose[:3].astype(f32), synth.transform_points(pose, pts)))
    return batches


def honest(batches, results, table):
    """The conditions under which a multi-scan comparison compares something (asserted by the tests that use a drive)."""
    total = sum(len(p) for _, p in batches)
    kept = sum(len(r[1]) for r in results[2 * len(batches):])
    removed = 1.0 - kept / total
    assert all((r if isinstance(r, int) else r[0]) == 0 for r in results), "a parity case may not contain a refusal"
    assert 0.01 <= removed <= 0.60, removed
    xyz, hits, rays = table
    assert np.any((rays > 0) & (rays < 3 * hits)), "no voxel with rays > 0 survives"
    return removed
