"""The node-cloud cache without a GPU: the numpy model (tests/node_clouds_common.py) against the oracle's transform and
against google.protobuf, the written rule for -0.0 and NaN, the host entry points (dliom_rigid3f_inverse,
dliom_node_range_data_check), symbols, struct layouts and refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import node_clouds_common as nc  # noqa: E402

NAMES = ["dliom_node_clouds_create", "dliom_node_clouds_create_sized", "dliom_node_clouds_destroy", "dliom_node_clouds_clear",
         "dliom_node_clouds_add", "dliom_node_clouds_size", "dliom_node_clouds_info", "dliom_node_clouds_memory_stats",
         "dliom_node_clouds_download", "dliom_node_clouds_pack_point_cloud2", "dliom_cloud_pack_point_cloud2", "dliom_rigid3f_inverse",
         "dliom_node_clouds_to_proto", "dliom_node_range_data_check", "dliom_node_range_data_from_proto"]


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


def scene(seed, n_r=40, n_m=9, zeros=False):
    rng = np.random.default_rng(seed)
    return nc.info_of(rng, seed), nc.cloud(rng, n_r, zeros), nc.cloud(rng, n_m, zeros)


# ---- the transform ----
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_transform_equals_oracle(orc, seed):
    rng = np.random.default_rng(seed)
    pts = nc.cloud(rng, 500)
    first, second = nc.random_pose(rng), nc.random_pose(rng)
    one = nc.transform(first, pts)
    assert np.array_equal(one.view(np.uint32), orc.transform_points(first, pts).view(np.uint32))
    two = nc.transform_in_turn([first, second], pts)
    assert np.array_equal(two.view(np.uint32), orc.transform_points(second, orc.transform_points(first, pts)).view(np.uint32))


def test_two_poses_in_turn_differ_from_their_product():
    """pb_range_data_to_ros_cloud rounds between local_pose.inverse() and global_pose: on this pair the product of the two
    poses, applied once, gives other bits, so a cache that multiplied the poses first would be found out."""
    rng = np.random.default_rng(11)
    pts = nc.cloud(rng, 500)
    local, global_pose = nc.random_pose(rng), nc.random_pose(rng)
    inverse = nc.rigid3f_inverse(local)
    in_turn = nc.transform_in_turn([inverse, global_pose], pts)
    at_once = nc.transform(nc.pose_product(global_pose, inverse), pts)
    assert np.allclose(in_turn, at_once, atol=1e-3)  # the same map, to float accuracy
    assert np.any(in_turn.view(np.uint32) != at_once.view(np.uint32))


def test_rigid3f_inverse(dl, orc):
    rng = np.random.default_rng(5)
    for _ in range(20):
        pose = nc.random_pose(rng)
        want = nc.rigid3f_inverse(pose)
        assert np.array_equal(dl.rigid3f_inverse(pose).view(np.uint32), want.view(np.uint32))
        # ... and it is the inverse: back to within float rounding of the points' size
        pts = nc.cloud(rng, 50)
        back = orc.transform_points(want, orc.transform_points(pose, pts))
        assert np.max(np.abs(back - pts)) < 1e-3
    assert dl.load_library().dliom_rigid3f_inverse(None, None) == dl.ERR_INVALID_ARGUMENT


# ---- the message ----
@pytest.mark.parametrize("seed,n_r,n_m", [(1, 40, 9), (2, 0, 0), (3, 1, 0), (4, 0, 3), (5, 964, 0)])
def test_model_message_equals_protobuf(seed, n_r, n_m):
    info, returns, misses = scene(seed, n_r, n_m)
    # the installed runtime writes -0.0, the reference's drops it: the generator must yield none for this comparison
    assert not nc.has_negative_zero(returns, misses, info["origin_in_local"], info["local_pose7"])
    assert nc.node_message(info, returns, misses) == nc.protobuf_node_message(info, returns, misses).SerializeToString()


def test_model_message_zero_scalars_and_negative_ids():
    rng = np.random.default_rng(8)
    for timestamp, trajectory_id in ((0, 0), (5, -1), (-7, 2 ** 31 - 1), (2 ** 62, -2 ** 31)):
        info = nc.info_of(rng, 1, timestamp=timestamp, trajectory_id=trajectory_id)
        info["node_index"] = trajectory_id
        returns = nc.cloud(rng, 5)
        returns[2] = 0.0  # (+0.0: dropped by both)
        got = nc.node_message(info, returns, returns[:0])
        assert got == nc.protobuf_node_message(info, returns, returns[:0]).SerializeToString()
        if trajectory_id < 0:
            assert bytes([2 << 3]) + nc.varint(trajectory_id) in got and len(nc.varint(trajectory_id)) == 10


def test_written_rule_for_negative_zero_and_nan():
    """-0.0 is dropped and NaN is written (v == 0 decides), whatever the installed runtime does with -0.0."""
    assert nc.vector3f(2, [-0.0, 0.0, -0.0]) == bytes([0x12, 0])
    nan = nc.vector3f(3, [np.nan, -0.0, 1.0])
    assert nan[:2] == bytes([0x1A, 10]) and nan[2] == 0x0D and nan[7] == 0x1D and len(nan) == 12
    assert np.isnan(np.frombuffer(nan[3:7], dtype="<f4")[0])
    full = nc.vector3f(2, [1.0, 2.0, 3.0])
    assert len(full) == nc.MAX_RECORD and full[1] == 15
    info, returns, misses = scene(9, 30, 8, zeros=True)
    assert nc.has_negative_zero(returns) and np.isnan(returns).any()
    lengths = nc.record_lengths(returns)
    assert set(int(v) for v in lengths) == {2, 7, 12, 17}
    msg = nc.node_message(info, returns, misses)
    parsed = nc.message_classes()["NodeRangeData"]()
    parsed.ParseFromString(msg)
    got = np.array([[p.x, p.y, p.z] for p in parsed.range_data_in_local.returns], dtype=np.float32)
    want = np.where(returns == 0, np.float32(0), returns)  # a dropped -0.0 comes back as +0.0
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want))


def test_round_trip_through_parse_from_string(dl):
    info, returns, misses = scene(21, 300, 40)
    msg = nc.node_message(info, returns, misses)
    parsed = nc.message_classes()["NodeRangeData"]()
    parsed.ParseFromString(msg)
    assert parsed.SerializeToString() == msg
    assert parsed.timestamp == info["timestamp"] and parsed.trajectory_id == info["trajectory_id"]
    assert len(parsed.range_data_in_local.returns) == 300 and len(parsed.range_data_in_local.misses) == 40
    got, n_r, n_m = dl.node_range_data_check(msg)
    assert (n_r, n_m) == (300, 40) and got["timestamp"] == info["timestamp"] and got["trajectory_id"] == info["trajectory_id"]
    assert np.array_equal(got["local_pose7"], np.asarray(info["local_pose7"], dtype=np.float64))
    assert np.array_equal(got["origin_in_local"], info["origin_in_local"])


def test_tile_starts_cover_all_residues():
    assert nc.tile_start_residues(nc.residue_scene()) == {0, 1, 2, 3}


# ---- the parser ----
def test_parser_accepts_what_protobuf_accepts(dl):
    info, returns, misses = scene(31, 6, 2)
    empty, n_r, n_m = dl.node_range_data_check(b"")
    assert (n_r, n_m, empty["timestamp"], empty["trajectory_id"]) == (0, 0, 0, 0) and not empty["local_pose7"].any()
    # any field order, unknown fields of every wire type in between, a second RangeData merged
    fields = [nc.varint(1 << 3) + nc.varint(info["timestamp"]), nc.varint(2 << 3) + nc.varint(info["trajectory_id"] or 7),
              nc.rigid3d(4, info["local_pose7"])]
    unknown = nc.varint(9 << 3) + nc.varint(300) + bytes([10 << 3 | 1]) + bytes(8) + bytes([11 << 3 | 5]) + bytes(4) + nc.message(12, b"xyz")
    first = nc.message(5, nc.records(2, returns[:4]) + unknown + nc.records(3, misses))
    second = nc.message(5, nc.vector3f(1, info["origin_in_local"]) + nc.records(2, returns[4:]))
    shuffled = second[:0] + first + unknown + fields[2] + fields[1] + second + fields[0]
    want = nc.message_classes()["NodeRangeData"]()
    want.ParseFromString(shuffled)
    got, n_r, n_m = dl.node_range_data_check(shuffled)
    assert (n_r, n_m) == (len(want.range_data_in_local.returns), len(want.range_data_in_local.misses)) == (6, 2)
    assert got["timestamp"] == want.timestamp and got["trajectory_id"] == want.trajectory_id
    assert np.array_equal(got["origin_in_local"], info["origin_in_local"])
    assert got["local_pose7"][3] == want.local_pose.rotation.w and got["local_pose7"][0] == want.local_pose.translation.x


def test_parser_refuses_malformed_streams(dl):
    info, returns, misses = scene(32, 6, 2)
    msg = nc.node_message(info, returns, misses)
    L = dl.load_library()

    def status(data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        return L.dliom_node_range_data_check(buf.ctypes.data_as(C.POINTER(C.c_uint8)) if len(buf) else None, len(buf), None, None, None)
    assert status(msg) == dl.OK
    for cut in range(1, len(msg)):
        # a cut that falls between two top-level fields leaves a shorter message that is well formed
        ok = cut in _top_level_boundaries(msg)
        assert (status(msg[:cut]) == dl.OK) == ok, cut
    assert status(bytes([0x80] * 11)) == dl.ERR_INVALID_ARGUMENT                      # a varint that never ends
    assert status(bytes([0])) == dl.ERR_INVALID_ARGUMENT                              # field number 0
    assert status(bytes([5 << 3 | 2, 5, 0x12, 9])) == dl.ERR_INVALID_ARGUMENT         # a length beyond the message
    assert status(nc.message(5, bytes([0x12, 3, 0x0D, 1, 2]))) == dl.ERR_INVALID_ARGUMENT   # a float cut short
    assert status(bytes([1 << 3 | 3])) == dl.ERR_INVALID_ARGUMENT                     # a group
    assert L.dliom_node_range_data_check(None, 4, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_node_range_data_check(None, -1, None, None, None) == dl.ERR_INVALID_ARGUMENT


def _top_level_boundaries(msg):
    at, out = 0, set()
    while at < len(msg):
        tag = msg[at]
        at += 1
        if tag & 7 == 0:
            while msg[at] & 0x80:
                at += 1
            at += 1
        else:
            length, shift = 0, 0
            while True:
                b = msg[at]
                at += 1
                length |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
            at += length
        out.add(at)
    return out


# ---- the interface ----
def test_names_are_bound_and_declared(dl):
    bound = {name for name, _, _ in dl.SYMBOLS}
    header = open(os.path.join(nc.ROOT, "include", "dliom.h")).read()
    lib = C.CDLL(dl.LIB_PATH)
    for name in NAMES:
        assert name in bound and name + "(" in header and hasattr(lib, name), name
    for name in ("NodeClouds", "node_range_data_from_proto", "node_range_data_check", "rigid3f_inverse"):
        assert hasattr(dl, name)
    assert hasattr(dl.PointCloud, "pack_point_cloud2")
    for method in ("add", "pack_point_cloud2", "to_proto", "download", "info", "memory_stats", "clear", "size"):
        assert hasattr(dl.NodeClouds, method)
    assert "#define DLIOM_NODE_RANGE_MAX_RECORD 17" in header and dl.NODE_RANGE_MAX_RECORD == nc.MAX_RECORD == 17


def test_struct_layouts_match_the_header(dl, tmp_path):
    structs = {"dliom_node_cloud_info": dl.NodeCloudInfo, "dliom_node_clouds_memory": dl.NodeCloudsMemory,
               "dliom_node_clouds_transform": dl.NodeCloudsTransform, "dliom_node_clouds_limits": dl.NodeCloudsLimits,
               "dliom_node_clouds_stats": dl.NodeCloudsStats}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "dliom.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(nc.ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for field, _ in cls._fields_:
            assert int(got[cname + "." + field]) == getattr(cls, field).offset, (cname, field)


def test_null_arguments_are_refused(dl):
    L = dl.load_library()
    E = dl.ERR_INVALID_ARGUMENT
    h, n = C.c_void_p(), C.c_int64()
    offsets = (C.c_int64 * 2)()
    assert L.dliom_node_clouds_create(None, C.byref(h)) == E and L.dliom_node_clouds_create_sized(None, 64, C.byref(h)) == E
    assert L.dliom_node_clouds_destroy(None) == E and L.dliom_node_clouds_clear(None) == E
    assert L.dliom_node_clouds_add(None, None, None, None, None, None) == E
    assert L.dliom_node_clouds_size(None, C.byref(n), None, None) == E
    assert L.dliom_node_clouds_info(None, 0, None, None, None) == E
    assert L.dliom_node_clouds_memory_stats(None, None) == E
    assert L.dliom_node_clouds_download(None, 0, None, None) == E
    assert L.dliom_node_clouds_pack_point_cloud2(None, 0, 0, None, None, None, 0, offsets, None) == E
    assert L.dliom_node_clouds_to_proto(None, 0, 0, None, None, 0, offsets, None) == E
    assert L.dliom_cloud_pack_point_cloud2(None, None, None, 0, C.byref(n)) == E
    assert L.dliom_node_range_data_from_proto(None, None, 0, None, None, None) == E
