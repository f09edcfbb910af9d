"""numpy float32 model of the node-cloud cache's two record kinds, written from the statement in include/dliom.h ("node
clouds kept in HBM"): the PointCloud2 record (x, y, z, 1.0f of a return moved by zero, one or two float poses) and the
mapping::proto::NodeRangeData message.  Plus what the host and GPU tests share: Rigid3f::inverse, the protobuf message
classes built from descriptors, and the scenes."""
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 256        # records a tile of the proto passes (csrc/node_clouds.hip kTile)
MAX_RECORD = 17   # DLIOM_NODE_RANGE_MAX_RECORD
IDENTITY7 = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float32)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- the float transform: sensor::TransformPointCloud in Eigen's operation order, every operation rounded to float ----
def transform(pose7, points):
    """rotation * p + translation for float32 points (n, 3) under the float pose [tx, ty, tz, qw, qx, qy, qz]:
    QuaternionBase::_transformVector (uv = u x v; uv += uv; (v + w uv) + u x uv), then the translation."""
    t = f32(pose7)
    p = f32(points).reshape(-1, 3)
    w, qx, qy, qz = t[3], t[4], t[5], t[6]
    vx, vy, vz = p[:, 0], p[:, 1], p[:, 2]
    uvx = qy * vz - qz * vy
    uvy = qz * vx - qx * vz
    uvz = qx * vy - qy * vx
    uvx, uvy, uvz = uvx + uvx, uvy + uvy, uvz + uvz
    cx = qy * uvz - qz * uvy
    cy = qz * uvx - qx * uvz
    cz = qx * uvy - qy * uvx
    out = np.stack([((vx + w * uvx) + cx) + t[0], ((vy + w * uvy) + cy) + t[1], ((vz + w * uvz) + cz) + t[2]], axis=1)
    assert out.dtype == np.float32
    return out


def transform_in_turn(poses, points):
    """second * (first * p): every pose applied to the rounded result of the one before"""
    p = f32(points).reshape(-1, 3)
    for pose in f32(poses).reshape(-1, 7):
        p = transform(pose, p)
    return p


def rigid3f_inverse(pose7):
    """Rigid3f::inverse (rigid_transform.h:167-171): the conjugate, and -(conjugate * translation)"""
    t = f32(pose7)
    conjugate = np.array([0, 0, 0, t[3], -t[4], -t[5], -t[6]], dtype=np.float32)
    moved = transform(conjugate, t[:3].reshape(1, 3))[0]
    return np.concatenate([-moved, conjugate[3:]]).astype(np.float32)


def pose_product(a, b):
    """a * b as ONE float pose (rigid_transform.h:206-212 with the SSE lane order of Eigen's quaternion product): what the reference does NOT
    do between local_pose.inverse() and global_pose -- the tests show that it differs"""
    a, b = f32(a), f32(b)
    aw, ax, ay, az = a[3:]
    bw, bx, by, bz = b[3:]
    q = np.array([(aw * bw - ax * bx) - (az * bz + ay * by), (ax * bw - az * by) + (ay * bz + aw * bx),
                  (ay * bw - ax * bz) + (az * bx + aw * by), (az * bw - ay * bx) + (ax * by + aw * bz)], dtype=np.float32)
    return np.concatenate([transform(a, b[:3].reshape(1, 3))[0], q]).astype(np.float32)


def point_cloud2_data(returns, poses=None):
    """msg.data of a node: x, y, z, 1.0f a return, the point moved by the poses in turn"""
    p = f32(returns).reshape(-1, 3)
    if poses is not None:
        p = transform_in_turn(poses, p)
    rec = np.ones((len(p), 4), dtype=np.float32)
    rec[:, :3] = p
    return rec.tobytes()


# ---- the wire format ----
def varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _scalar_fields(values, fmt, wire_type):
    out = b""
    for i, v in enumerate(values):
        if v != 0:  # -0.0 == 0: dropped; NaN != 0: written
            out += bytes([(i + 1) << 3 | wire_type]) + struct.pack(fmt, v)
    return out


def vector3f(field, xyz):
    payload = _scalar_fields([np.float32(v) for v in xyz], "<f", 5)
    return varint(field << 3 | 2) + varint(len(payload)) + payload


def message(field, payload):
    return varint(field << 3 | 2) + varint(len(payload)) + payload


def rigid3d(field, pose7):
    """transform::proto::Rigid3d of (x, y, z, qw, qx, qy, qz): both sub-messages always present"""
    pose = [float(v) for v in pose7]
    translation = _scalar_fields(pose[:3], "<d", 1)
    rotation = _scalar_fields([pose[4], pose[5], pose[6], pose[3]], "<d", 1)
    return message(field, message(1, translation) + message(2, rotation))


def record_lengths(points):
    p = f32(points).reshape(-1, 3)
    return 2 + 5 * np.sum(p != 0, axis=1)


def records(field, points):
    return b"".join(vector3f(field, p) for p in f32(points).reshape(-1, 3))


def node_message(info, returns, misses):
    """mapping::proto::NodeRangeData of a node; info: dict(timestamp, trajectory_id, node_index, local_pose7, origin_in_local)"""
    out = b""
    for field, key in ((1, "timestamp"), (2, "trajectory_id"), (3, "node_index")):
        if int(info.get(key, 0)) != 0:
            out += varint(field << 3) + varint(int(info[key]))
    out += rigid3d(4, info.get("local_pose7", (0, 0, 0, 1, 0, 0, 0)))
    range_data = vector3f(1, info.get("origin_in_local", (0, 0, 0))) + records(2, returns) + records(3, misses)
    return out + message(5, range_data)


def tile_start_residues(nodes):
    """{byte offset mod 4} of every tile's first record in the nodes' messages laid back to back.
    nodes: [(info, returns, misses)]"""
    residues, at = set(), 0
    for info, returns, misses in nodes:
        msg = node_message(info, returns, misses)
        lengths = np.concatenate([record_lengths(returns), record_lengths(misses)]).astype(np.int64)
        body = int(lengths.sum())
        first = at + len(msg) - body
        starts = first + np.concatenate([[0], np.cumsum(lengths)])[:-1][::TILE] if len(lengths) else []
        residues.update(int(s) % 4 for s in starts)
        at += len(msg)
    return residues


# ---- scenes ----
def random_pose(rng, translation=20.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.concatenate([rng.uniform(-translation, translation, 3), q]).astype(np.float32)


def random_pose_d(rng, translation=20.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.concatenate([rng.uniform(-translation, translation, 3), q])


def cloud(rng, n, zeros=False):
    """n float32 points; zeros: every fourth point has 1 to 3 coordinates that are 0, -0.0 or NaN"""
    p = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
    p[p == 0] = 1.0
    if zeros and n:
        special = np.array([0.0, -0.0, np.nan], dtype=np.float32)
        for i in range(0, n, 4):
            for a in rng.choice(3, size=1 + (i // 4) % 3, replace=False):
                p[i, a] = special[(i // 4 + a) % 3]
        if n > 2:
            p[1] = 0.0       # 0 coordinates written: a 2-byte record
            p[2] = -0.0
    return p


def info_of(rng, i, timestamp=None, trajectory_id=None):
    return {"timestamp": 636_000_000_000_000_000 + 1000 * i if timestamp is None else timestamp,
            "trajectory_id": i % 3 if trajectory_id is None else trajectory_id, "node_index": 0,
            "local_pose7": random_pose_d(rng), "origin_in_local": rng.uniform(-5, 5, 3).astype(np.float32)}


def residue_scene():
    """[(info, returns, misses)] whose tiles begin at all four byte offsets mod 4 (the tests assert it on the model)"""
    rng = np.random.default_rng(3)
    return [(info_of(rng, i), cloud(rng, n, zeros=True), cloud(rng, m, zeros=True)) for i, (n, m) in
            enumerate([(700, 0), (257, 300), (0, 0), (1025, 5), (513, 2), (300, 300)])]


# ---- google.protobuf's own serialisation of the messages ----
_classes = None


def message_classes():
    """dict of the classes Vector3f, Vector3d, Quaterniond, Rigid3d, RangeData, NodeRangeData, built from descriptors that restate
    transform/proto/transform.proto, sensor/proto/sensor.proto and mapping/proto/local_slam_range_data.proto"""
    global _classes
    if _classes is not None:
        return _classes
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    T = descriptor_pb2.FieldDescriptorProto
    f = descriptor_pb2.FileDescriptorProto()
    f.name, f.package, f.syntax = "dliom_test/node_range_data.proto", "dliom_test_nrd", "proto3"

    def add(name, fields):
        m = f.message_type.add()
        m.name = name
        for fname, number, typ, label, type_name in fields:
            fd = m.field.add()
            fd.name, fd.number, fd.type, fd.label = fname, number, typ, label
            if type_name:
                fd.type_name = ".dliom_test_nrd." + type_name
    O, R = T.LABEL_OPTIONAL, T.LABEL_REPEATED
    add("Vector3f", [(n, i + 1, T.TYPE_FLOAT, O, None) for i, n in enumerate("xyz")])
    add("Vector3d", [(n, i + 1, T.TYPE_DOUBLE, O, None) for i, n in enumerate("xyz")])
    add("Quaterniond", [(n, i + 1, T.TYPE_DOUBLE, O, None) for i, n in enumerate("xyzw")])
    add("Rigid3d", [("translation", 1, T.TYPE_MESSAGE, O, "Vector3d"), ("rotation", 2, T.TYPE_MESSAGE, O, "Quaterniond")])
    add("RangeData", [("origin", 1, T.TYPE_MESSAGE, O, "Vector3f"), ("returns", 2, T.TYPE_MESSAGE, R, "Vector3f"),
                      ("misses", 3, T.TYPE_MESSAGE, R, "Vector3f")])
    add("NodeRangeData", [("timestamp", 1, T.TYPE_INT64, O, None), ("trajectory_id", 2, T.TYPE_INT32, O, None),
                          ("node_index", 3, T.TYPE_INT32, O, None), ("local_pose", 4, T.TYPE_MESSAGE, O, "Rigid3d"),
                          ("range_data_in_local", 5, T.TYPE_MESSAGE, O, "RangeData")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(f)
    _classes = {n: message_factory.GetMessageClass(pool.FindMessageTypeByName("dliom_test_nrd." + n))
                for n in ("Vector3f", "Vector3d", "Quaterniond", "Rigid3d", "RangeData", "NodeRangeData")}
    return _classes


def protobuf_node_message(info, returns, misses):
    """SerializeRangeData's message as google.protobuf builds it: mutable_local_pose, mutable_range_data_in_local and
    mutable_origin are called, so the three sub-messages are present even when empty"""
    msg = message_classes()["NodeRangeData"]()
    msg.timestamp, msg.trajectory_id, msg.node_index = int(info["timestamp"]), int(info["trajectory_id"]), int(info["node_index"])
    pose = [float(v) for v in info["local_pose7"]]
    lp = msg.local_pose
    lp.translation.SetInParent()
    lp.rotation.SetInParent()
    lp.translation.x, lp.translation.y, lp.translation.z = pose[:3]
    lp.rotation.w, lp.rotation.x, lp.rotation.y, lp.rotation.z = pose[3:]
    rd = msg.range_data_in_local
    rd.SetInParent()
    rd.origin.SetInParent()
    rd.origin.x, rd.origin.y, rd.origin.z = (float(np.float32(v)) for v in info["origin_in_local"])
    for sub, pts in ((rd.returns, returns), (rd.misses, misses)):
        for p in f32(pts).reshape(-1, 3):
            v = sub.add()
            v.x, v.y, v.z = float(p[0]), float(p[1]), float(p[2])
    return msg


def has_negative_zero(*arrays):
    return any(bool(np.any((np.asarray(a, dtype=np.float64) == 0) & np.signbit(np.asarray(a, dtype=np.float64)))) for a in arrays)
