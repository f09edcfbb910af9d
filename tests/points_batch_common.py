"""Shared by tests/test_points_batch_host.py, tests/test_gpu_points_batch.py and tools/points_batch_bench.py: builds and
runs the CPU model of the batch stages (tests/cpp/points_batch_model.cc) and makes the inputs."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SRC = os.path.join(ROOT, "tests", "cpp", "points_batch_model.cc")
REMOVE, PULSE, COLOR, INTENSITY_TO_COLOR, PACK, HEADER = 1, 2, 3, 4, 5, 6
PLY, PCD = 0, 1
f32 = np.float32


def build_model(directory):
    exe = os.path.join(str(directory), "points_batch_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def _batch_bytes(points, intensities, colors):
    pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    out = struct.pack("<qiq", len(pts), 0 if intensities is None else 1, 0 if colors is None else len(colors)) + pts.tobytes()
    if intensities is not None:
        out += np.ascontiguousarray(intensities, dtype=f32).tobytes()
    if colors is not None:
        out += np.ascontiguousarray(colors, dtype=f32).tobytes()
    return out


def remove_op(points, intensities, colors, keep):
    return (REMOVE, _batch_bytes(points, intensities, colors) + np.ascontiguousarray(keep, dtype=np.uint8).tobytes())


def pulse_op(ratio, num_pulses, num_samples, n):
    return (PULSE, struct.pack("<dqqq", float(ratio), int(num_pulses), int(num_samples), int(n)), int(n))


def color_op(points, intensities, colors, rgb):
    return (COLOR, _batch_bytes(points, intensities, colors) + np.ascontiguousarray(rgb, dtype=f32).tobytes())


def intensity_to_color_op(points, intensities, colors, lo, hi):
    return (INTENSITY_TO_COLOR, _batch_bytes(points, intensities, colors) + struct.pack("<ff", lo, hi))


def pack_op(points, intensities, colors, fmt, with_colors, with_intensities):
    return (PACK, _batch_bytes(points, intensities, colors) + struct.pack("<iii", fmt, int(with_colors), int(with_intensities)))


def header_op(fmt, with_colors, with_intensities, count):
    return (HEADER, struct.pack("<iiiq", fmt, int(with_colors), int(with_intensities), int(count)))


def run_model(exe, ops, directory, timing=False):
    """-> one result an op: a batch (points (n, 3), intensities or None, colors (n, 3) or None) for REMOVE / COLOR /
    INTENSITY_TO_COLOR, (keep bool[n], num_pulses, num_samples) for PULSE, bytes for PACK and HEADER."""
    src, dst = os.path.join(str(directory), "points_batch_ops.bin"), os.path.join(str(directory), "points_batch_out.bin")
    with open(src, "wb") as f:
        for o in ops:
            f.write(struct.pack("<i", o[0]))
            f.write(o[1])
    text = subprocess.check_output([exe, src, dst] + (["--time"] if timing else [])).decode()
    data = open(dst, "rb").read()
    at, results = 0, []
    for o in ops:
        if o[0] == PULSE:
            n = o[2]
            keep = np.frombuffer(data, dtype=np.uint8, count=n, offset=at) != 0
            pulses, samples = struct.unpack_from("<qq", data, at + n)
            at += n + 16
            results.append((keep, pulses, samples))
        elif o[0] in (PACK, HEADER):
            (n,) = struct.unpack_from("<q", data, at)
            results.append(data[at + 8:at + 8 + n])
            at += 8 + n
        else:
            n, ni, nc = struct.unpack_from("<qqq", data, at)
            at += 24
            pts = np.frombuffer(data, dtype=f32, count=3 * n, offset=at).reshape(n, 3).copy()
            at += 12 * n
            it = np.frombuffer(data, dtype=f32, count=ni, offset=at).copy() if ni else None
            at += 4 * ni
            col = np.frombuffer(data, dtype=f32, count=3 * nc, offset=at).reshape(nc, 3).copy() if nc else None
            at += 12 * nc
            results.append((pts, it, col))
    assert at == len(data)
    return (results, float(text)) if timing else results


def closed_form(ratio, k):
    """min(k, ceil(ratio * k)): what a sampler that began at (0, 0) does NOT always hold after k pulses."""
    return min(k, int(np.ceil(np.float64(ratio) * np.float64(k))))


def batch_arrays(n, seed, attributes):
    """n points about the origin with ranges spread over 0..40 m -> (points, intensities or None, colors or None);
    attributes: "none", "intensities", "colors", "both"."""
    rng = np.random.RandomState(seed)
    pts = (rng.normal(size=(n, 3)) * rng.uniform(0.0, 25.0, size=(n, 1))).astype(f32)
    it = rng.uniform(0.0, 255.0, size=n).astype(f32) if attributes in ("intensities", "both") else None
    col = rng.uniform(0.0, 1.0, size=(n, 3)).astype(f32) if attributes in ("colors", "both") else None
    return pts, it, col


def assert_batch_equals(batch, want):
    """A device batch (dliom.PointsBatch) against a model result, by bytes."""
    pts, it, col = batch.download()
    wp, wi, wc = want
    assert len(batch) == len(wp)
    assert pts.tobytes() == wp.tobytes()
    assert (it is None) == (wi is None) and (col is None) == (wc is None), (batch.has_intensities, batch.has_colors)
    if wi is not None:
        assert it.tobytes() == wi.tobytes()
    if wc is not None:
        assert col.tobytes() == wc.tobytes()


ADAPTER_SRC = os.path.join(ROOT, "tests", "cpp", "points_batch_adapter.cc")


def build_adapter(directory, lib_path):
    exe = os.path.join(str(directory), "points_batch_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "d-liom_amd", "cpp"), "-o", exe, ADAPTER_SRC, lib_path,
                           "-Wl,-rpath," + os.path.dirname(lib_path)])
    return exe


def pipeline_messages(beams, azimuths, scans=4, seed=3):
    """`scans` messages of one sensor-frame scan shape against the 200-node corkscrew, each scaled a little differently,
    with random intensities over [-20, 300] -> (times, poses, mount, [(cloud_time, xyzt, intensities)])"""
    import assemble_common as ac
    times, poses, cloud_time, xyzt = ac.drive(beams, azimuths, 200)
    rng = np.random.RandomState(seed)
    messages = []
    for s in range(scans):
        moved = xyzt.copy()
        moved[:, :3] *= f32(1.0 + 0.01 * s)
        messages.append((cloud_time, moved, rng.uniform(-20.0, 300.0, size=len(xyzt)).astype(f32)))
    return times, poses, ac.MOUNT, messages


def run_adapter(exe, directory, times, poses, mount, messages, voxel_size=0.25, min_range=1.0, max_range=20.0, ratio=0.55,
                xray_voxel_size=0.1, repeats=0):
    """-> dict: device / host (ply bytes, image uint32 (h, w)), uploads, downloaded, records[, device_ms, host_ms]"""
    src, dst = os.path.join(str(directory), "pipeline_in.bin"), os.path.join(str(directory), "pipeline_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<q", len(times)) + np.ascontiguousarray(times, dtype=np.int64).tobytes())
        f.write(np.ascontiguousarray(poses, dtype=np.float64).tobytes() + np.ascontiguousarray(mount, dtype=np.float64).tobytes())
        f.write(struct.pack("<q", len(messages)))
        for cloud_time, xyzt, intensities in messages:
            f.write(struct.pack("<qq", int(cloud_time), len(xyzt)) + np.ascontiguousarray(xyzt, dtype=f32).tobytes())
            f.write(np.ascontiguousarray(intensities, dtype=f32).tobytes())
    text = subprocess.run([exe, src, dst] + [repr(float(v)) for v in (voxel_size, min_range, max_range, ratio, xray_voxel_size)] +
                          [str(int(repeats))], timeout=600, check=True, stdout=subprocess.PIPE).stdout.decode()
    data = open(dst, "rb").read()
    at, out = 0, {}
    for name in ("device", "host"):
        (n,) = struct.unpack_from("<q", data, at)
        ply = data[at + 8:at + 8 + n]
        w, h = struct.unpack_from("<qq", data, at + 8 + n)
        at += 24 + n
        out[name] = (ply, np.frombuffer(data, dtype=np.uint32, count=w * h, offset=at).reshape(h, w).copy())
        at += 4 * w * h
    out["uploads"], out["downloaded"], out["records"] = struct.unpack_from("<qqq", data, at)
    assert at + 24 == len(data)
    if repeats > 0:
        out["device_ms"], out["host_ms"] = (float(v) for v in text.split())
    return out
