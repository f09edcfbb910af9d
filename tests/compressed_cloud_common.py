"""numpy model of sensor::CompressedPointCloud and the TrajectoryNodeData message, written from the statement in
include/dliom.h ("compressed point clouds"), plus what the host and GPU tests share: the protobuf message classes built
from descriptors, and the known-answer inputs of the reference's compressed_point_cloud_test.cc restated as data."""
import os
import subprocess

import numpy as np

PRECISION = np.float32(0.001)
LIMIT = np.float32(8388608.0)
LARGEST_ACCEPTED = np.float32(8388.607421875)


def accepted(points):
    """Step 1 per point: every coordinate passes |p| / 0.001f < 8388608.f in float32 (NaN and inf fail)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.all(np.abs(p) / PRECISION < LIMIT, axis=1)


def lround(x):
    """std::lround of float32 values: round half away from zero (x - trunc(x) is exact)."""
    x = np.asarray(x, dtype=np.float32)
    t = np.trunc(x)
    d = x - t
    return t.astype(np.int64) + (d >= 0.5) - (d <= -0.5)


def quantize(points):
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    return lround(p / PRECISION)


def block_keys(blocks):
    """The 42-bit iterator-order key of block coordinates (n, 3) in [-8192, 8191]."""
    b = np.asarray(blocks, dtype=np.int64).reshape(-1, 3) + 8192
    X, Y, Z = b[:, 0], b[:, 1], b[:, 2]
    fields = (Z >> 6, Y >> 6, X >> 6, (Z >> 3) & 7, (Y >> 3) & 7, (X >> 3) & 7, Z & 7, Y & 7, X & 7)
    widths = (8, 8, 8, 3, 3, 3, 3, 3, 3)
    key = np.zeros(len(b), dtype=np.int64)
    for f, w in zip(fields, widths):
        key = (key << w) | f
    return key


def compress(points):
    """(num_points, int32 point_data) of a float32 cloud (n, 3); None if the bound check refuses it."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    if not np.all(accepted(p)):
        return None
    q = quantize(p)
    block, off = q >> 10, q & 1023
    key = block_keys(block)
    order = np.argsort(key, kind="stable")
    words = (((off[:, 2] << 10) + off[:, 1]) << 10) + off[:, 0]
    out = []
    starts = [i for i in range(len(order)) if i == 0 or key[order[i]] != key[order[i - 1]]] + [len(order)]
    for a, e in zip(starts[:-1], starts[1:]):
        out.append(np.concatenate(([e - a], block[order[a]], words[order[a:e]])))
    data = np.concatenate(out) if out else np.zeros(0, dtype=np.int64)
    return len(p), data.astype(np.int32)


def decompress(num_points, point_data):
    """float32 (num_points, 3) of a well-formed stream: float(int32((block << 10) + off)) * 0.001f."""
    d = np.asarray(point_data, dtype=np.int64)
    blocks, words, i, seen = [], [], 0, 0
    while seen < num_points:  # ReadNextPoint's walk
        count = int(d[i])
        blocks.append(np.broadcast_to(d[i + 1:i + 4], (count, 3)))
        words.append(d[i + 4:i + 4 + count])
        seen += count
        i += 4 + count
    if not words:
        return np.zeros((0, 3), dtype=np.float32)
    block, w = np.concatenate(blocks), np.concatenate(words)
    off = np.stack([w & 1023, (w >> 10) & 1023, w >> 20], axis=1)
    q = (((block << 10) + off) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return q.astype(np.float32) * PRECISION


# compressed_point_cloud_test.cc:59-69 (the eleven single points), :73-75 and :100-102, as data
KNOWN_SINGLE_POINTS = np.array([
    [8000.0, 7500.0, 5000.0], [1000.0, 2000.0, 3000.0], [100.0, 200.0, 300.0], [10.0, 20.0, 30.0],
    [-0.00049, -0.0005, -0.0015], [0.05119, 0.0512, 0.05121], [-0.05119, -0.0512, -0.05121], [0.8405, 0.84, 0.8396],
    [0.8395, 0.8394, 0.8393], [0.839, 0.8391, 0.8392], [0.8389, 0.8388, 0.83985]], dtype=np.float32)
KNOWN_THREE_POINTS = np.array([[0.838, 0, 0], [0.839, 0, 0], [0.840, 0, 0]], dtype=np.float32)


def known_no_gaps_cloud():
    x = PRECISION * np.arange(3000, dtype=np.float32) - np.float32(1.5)  # kPrecision * i - 1.5f, in float
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1).astype(np.float32)


# ---- the one-thread C++ restatement (tests/cpp/compressed_cloud_model.cc) ----
MODEL_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "compressed_cloud_model.cc")


def build_cpp_model(directory):
    exe = os.path.join(str(directory), "compressed_cloud_model")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, MODEL_SRC])
    return exe


def run_cpp_model(exe, directory, clouds, repeats=0):
    """[(num_points, int32 point_data) or None where refused] for float32 clouds, and the median milliseconds of a pass
    over all of them (None unless repeats > 0)."""
    src, dst = os.path.join(str(directory), "clouds.bin"), os.path.join(str(directory), "streams.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(clouds)).tobytes())
        for c in clouds:
            c = np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3)
            f.write(np.int32(len(c)).tobytes() + c.tobytes())
    printed = subprocess.check_output([exe, src, dst] + ([str(repeats)] if repeats > 0 else []))
    blob, at, out = open(dst, "rb").read(), 0, []
    for _ in clouds:
        n = int(np.frombuffer(blob, dtype=np.int32, count=1, offset=at)[0])
        words = int(np.frombuffer(blob, dtype=np.int64, count=1, offset=at + 4)[0])
        out.append(None if n < 0 else (n, np.frombuffer(blob, dtype=np.int32, count=words, offset=at + 12).copy()))
        at += 12 + 4 * words
    assert at == len(blob)
    return out, (float(printed.split()[0]) if repeats > 0 else None)


# ---- google.protobuf's own serialisation of the messages ----
_classes = None


def message_classes():
    """(CompressedPointCloud, TrajectoryNodeData) built from descriptors that restate sensor/proto/sensor.proto,
    transform/proto/transform.proto and mapping/proto/trajectory_node_data.proto."""
    global _classes
    if _classes is not None:
        return _classes
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    T = descriptor_pb2.FieldDescriptorProto
    f = descriptor_pb2.FileDescriptorProto()
    f.name, f.package, f.syntax = "dliom_test/node_data.proto", "dliom_test", "proto3"

    def message(name, fields):
        m = f.message_type.add()
        m.name = name
        for fname, number, typ, label, type_name in fields:
            fd = m.field.add()
            fd.name, fd.number, fd.type, fd.label = fname, number, typ, label
            if type_name:
                fd.type_name = ".dliom_test." + type_name
    O, R = T.LABEL_OPTIONAL, T.LABEL_REPEATED
    message("Vector3d", [(n, i + 1, T.TYPE_DOUBLE, O, None) for i, n in enumerate("xyz")])
    message("Quaterniond", [(n, i + 1, T.TYPE_DOUBLE, O, None) for i, n in enumerate("xyzw")])
    message("Rigid3d", [("translation", 1, T.TYPE_MESSAGE, O, "Vector3d"), ("rotation", 2, T.TYPE_MESSAGE, O, "Quaterniond")])
    message("CompressedPointCloud", [("num_points", 1, T.TYPE_INT32, O, None), ("point_data", 3, T.TYPE_INT32, R, None)])
    message("TrajectoryNodeData", [
        ("timestamp", 1, T.TYPE_INT64, O, None), ("gravity_alignment", 2, T.TYPE_MESSAGE, O, "Quaterniond"),
        ("filtered_gravity_aligned_point_cloud", 3, T.TYPE_MESSAGE, O, "CompressedPointCloud"),
        ("high_resolution_point_cloud", 4, T.TYPE_MESSAGE, O, "CompressedPointCloud"),
        ("low_resolution_point_cloud", 5, T.TYPE_MESSAGE, O, "CompressedPointCloud"),
        ("rotational_scan_matcher_histogram", 6, T.TYPE_FLOAT, R, None), ("local_pose", 7, T.TYPE_MESSAGE, O, "Rigid3d")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(f)
    _classes = tuple(message_factory.GetMessageClass(pool.FindMessageTypeByName("dliom_test." + n))
                     for n in ("CompressedPointCloud", "TrajectoryNodeData"))
    return _classes


def fill_cloud_message(msg, num_points, point_data):
    msg.num_points = int(num_points)
    msg.point_data.extend(int(w) for w in point_data)
    return msg


def cloud_message_bytes(num_points, point_data):
    return fill_cloud_message(message_classes()[0](), num_points, point_data).SerializeToString()


def node_message_bytes(timestamp, gravity_wxyz, streams, histogram, pose7):
    """mapping::ToProto(TrajectoryNode::Data): every sub-message is set (mutable_*), so present even when empty.
    streams: three (num_points, point_data)."""
    msg = message_classes()[1]()
    msg.timestamp = int(timestamp)
    g = msg.gravity_alignment
    g.SetInParent()
    g.w, g.x, g.y, g.z = (float(v) for v in gravity_wxyz)
    for sub, (n, d) in zip((msg.filtered_gravity_aligned_point_cloud, msg.high_resolution_point_cloud,
                            msg.low_resolution_point_cloud), streams):
        sub.SetInParent()
        fill_cloud_message(sub, n, d)
    msg.rotational_scan_matcher_histogram.extend(float(np.float32(h)) for h in histogram)
    lp = msg.local_pose
    lp.translation.SetInParent()
    lp.rotation.SetInParent()
    lp.translation.x, lp.translation.y, lp.translation.z = (float(v) for v in pose7[:3])
    lp.rotation.w, lp.rotation.x, lp.rotation.y, lp.rotation.z = (float(v) for v in pose7[3:])
    return msg.SerializeToString()
