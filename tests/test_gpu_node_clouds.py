"""The node-cloud cache on the device (dliom_node_clouds_*, dliom_cloud_pack_point_cloud2, dliom_node_range_data_from_proto,
cartographer_ros::NodeCloudCache) against the numpy model of tests/node_clouds_common.py: every result bit for bit, or
byte for byte."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import node_clouds_common as nc  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = nc.TILE  # the tile-boundary sizes below move with it
SIZES = [0, 1, TILE - 1, TILE, TILE + 1, 70001]


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


def add_nodes(dl, ctx, cache, nodes, pose_to_local=None):
    for info, returns, misses in nodes:
        r, m = dl.PointCloud(ctx, returns), (dl.PointCloud(ctx, misses) if misses is not None else None)
        cache.add(r, m, pose_to_local=pose_to_local, **info)
        r.close()
        if m is not None:
            m.close()


def make_nodes(seed, sizes, zeros=False):
    """[(info, returns, misses)] for sizes [(returns, misses)]"""
    rng = np.random.default_rng(seed)
    return [(nc.info_of(rng, i), nc.cloud(rng, n, zeros), nc.cloud(rng, m, zeros)) for i, (n, m) in enumerate(sizes)]


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), k, got[max(0, k - 20):k + 20], want[max(0, k - 20):k + 20]


def assert_bytes(got, want):
    assert got == want, first_difference(got, want)


def split(out, offsets):
    return [out[offsets[i]:offsets[i + 1]].tobytes() for i in range(len(offsets) - 1)]


def assert_messages(cache, nodes, first=0, **kw):
    out, offsets, stats, status = cache.to_proto(first, len(nodes), **kw)
    assert status == 0 and offsets[-1] == len(out)
    for got, (info, returns, misses) in zip(split(out, offsets), nodes):
        assert_bytes(got, nc.node_message(info, returns, misses))
    return out.tobytes(), stats


def assert_clouds(cache, nodes, first=0, poses=None, per_node=False, **kw):
    out, offsets, stats, status = cache.pack_point_cloud2(first, len(nodes), poses=poses, per_node=per_node, **kw)
    assert status == 0 and offsets[-1] == len(out)
    for i, (got, (_, returns, _)) in enumerate(zip(split(out, offsets), nodes)):
        p = None if poses is None else (np.asarray(poses, dtype=np.float32).reshape(len(nodes), -1, 7)[i] if per_node else poses)
        assert_bytes(got, nc.point_cloud2_data(returns, p))
    return out.tobytes(), stats


# ---- sizes ----
@pytest.mark.parametrize("n", SIZES)
def test_one_node_of_every_size(dl, ctx, n):
    nodes = make_nodes(100 + n, [(n, n // 3)], zeros=True)
    cache = dl.NodeClouds(ctx)
    add_nodes(dl, ctx, cache, nodes)
    assert cache.size() == (1, n, n // 3)
    r, m = cache.download(0)
    assert np.array_equal(r.view(np.uint32), nodes[0][1].view(np.uint32)) and np.array_equal(m.view(np.uint32), nodes[0][2].view(np.uint32))
    rng = np.random.default_rng(n)
    _, stats = assert_clouds(cache, nodes, poses=nc.random_pose(rng))
    assert stats["launches"] == (1 if n else 0) and stats["readbacks"] == 0 and stats["points"] == n
    _, stats = assert_messages(cache, nodes)
    assert (stats["chunks"], stats["launches"], stats["readbacks"]) == ((1, 4, 1) if n + n // 3 else (1, 1, 0))
    got = cache.info(0)
    assert got["timestamp"] == nodes[0][0]["timestamp"] and np.array_equal(got["local_pose7"], nodes[0][0]["local_pose7"])
    assert np.array_equal(got["origin_in_local"], nodes[0][0]["origin_in_local"])
    cache.close()


# ---- many nodes, chunks, transform modes ----
K70 = [(0, 0), (0, 0), (300, 7), (0, 0), (1, 0), (0, 5)] + [((37 * i) % 700, (11 * i) % 90) for i in range(61)] + [(TILE, TILE), (0, 0), (0, 0)]


@pytest.fixture(scope="module")
def seventy(dl, ctx):
    assert len(K70) == 70
    nodes = make_nodes(7, K70, zeros=True)
    cache = dl.NodeClouds(ctx)
    add_nodes(dl, ctx, cache, nodes)
    yield cache, nodes
    cache.close()


def test_seventy_nodes_with_empty_ones_and_every_chunking(seventy):
    cache, nodes = seventy
    assert {0, 1, 2, 3} == nc.tile_start_residues(nodes)
    clouds, messages = {}, {}
    for limit in (1, 300, 0):
        clouds[limit] = assert_clouds(cache, nodes, poses=nc.random_pose(np.random.default_rng(1)), max_points_per_chunk=limit)
        messages[limit] = assert_messages(cache, nodes, max_points_per_chunk=limit)
    for results, per_chunk in ((clouds, 1), (messages, 4)):
        assert results[1][0] == results[300][0] == results[0][0]
        chunks = [results[limit][1]["chunks"] for limit in (1, 300, 0)]
        assert chunks[0] > chunks[1] > chunks[2] == 1
        for limit in (1, 300, 0):
            assert results[limit][1]["launches"] == per_chunk * results[limit][1]["chunks"]
    assert [messages[limit][1]["readbacks"] for limit in (1, 300, 0)] == [messages[limit][1]["chunks"] for limit in (1, 300, 0)]
    # a range in the middle, and K = 1 on an empty node
    assert_clouds(cache, nodes[1:9], first=1)
    assert_messages(cache, nodes[3:4], first=3)
    assert_messages(cache, nodes[60:70], first=60)


@pytest.mark.parametrize("num_poses,per_node", [(0, False), (1, False), (1, True), (2, False), (2, True)])
def test_transform_modes(seventy, num_poses, per_node):
    cache, nodes = seventy
    rng = np.random.default_rng(10 * num_poses + per_node)
    poses = None if num_poses == 0 else np.stack([nc.random_pose(rng) for _ in range(num_poses * (len(nodes) if per_node else 1))])
    assert_clouds(cache, nodes, poses=poses, per_node=per_node, max_points_per_chunk=2000)


def test_two_poses_stay_separate(dl, ctx):
    """the pair of tests/test_node_clouds_host.py on which the product of the poses gives other bits"""
    rng = np.random.default_rng(11)
    pts = nc.cloud(rng, 500)
    local, global_pose = nc.random_pose(rng), nc.random_pose(rng)
    inverse = dl.rigid3f_inverse(local)
    cache = dl.NodeClouds(ctx)
    add_nodes(dl, ctx, cache, [(nc.info_of(rng, 0), pts, None)])
    out, _, _, _ = cache.pack_point_cloud2(poses=np.stack([inverse, global_pose]))
    assert_bytes(out.tobytes(), nc.point_cloud2_data(pts, [inverse, global_pose]))
    assert out.tobytes() != nc.point_cloud2_data(pts, [nc.pose_product(global_pose, inverse)])
    cache.close()


# ---- add ----
def test_add_with_pose_and_download(dl, ctx):
    rng = np.random.default_rng(5)
    returns, misses, pose = nc.cloud(rng, 1000), nc.cloud(rng, 77), nc.random_pose(rng)
    r, m = dl.PointCloud(ctx, returns), dl.PointCloud(ctx, misses)
    cache = dl.NodeClouds(ctx)
    info = nc.info_of(rng, 0)
    assert cache.add(r, m, **info) == 0 and cache.add(r, m, pose_to_local=pose, **info) == 1 and cache.add(r, None, pose_to_local=pose, **info) == 2
    plain, moved, alone = cache.download(0), cache.download(1), cache.download(2)
    assert np.array_equal(plain[0].view(np.uint32), returns.view(np.uint32)) and np.array_equal(plain[1].view(np.uint32), misses.view(np.uint32))
    assert np.array_equal(moved[0].view(np.uint32), r.download(pose).view(np.uint32))  # dliom_cloud_download_transformed
    assert np.array_equal(moved[1].view(np.uint32), m.download(pose).view(np.uint32))
    assert np.array_equal(moved[0].view(np.uint32), nc.transform(pose, returns).view(np.uint32))
    assert np.array_equal(alone[0].view(np.uint32), moved[0].view(np.uint32)) and len(alone[1]) == 0
    # the single cloud's records
    out, n = r.pack_point_cloud2(pose)
    assert n == 16 * len(returns)
    assert_bytes(out.tobytes(), nc.point_cloud2_data(returns, [pose]))
    assert_bytes(r.pack_point_cloud2()[0].tobytes(), nc.point_cloud2_data(returns))
    other = dl.Context(0)
    foreign = dl.PointCloud(other, returns[:3])
    with pytest.raises(dl.DliomError):
        cache.add(foreign)
    foreign.close()
    other.close()
    for c in (r, m, cache):
        c.close()


def test_growth_keeps_earlier_nodes(dl, ctx):
    """nodes added after a pack, then 3 000 tiny nodes in slabs of 4 096 floats: more slabs, a larger table, the same bytes"""
    rng = np.random.default_rng(9)
    early = make_nodes(1, [(500, 20), (0, 0), (TILE + 1, 3)], zeros=True)
    cache = dl.NodeClouds(ctx, slab_floats=4096)
    add_nodes(dl, ctx, cache, early)
    clouds_before, _ = assert_clouds(cache, early, poses=nc.random_pose(np.random.default_rng(2)))
    messages_before, _ = assert_messages(cache, early)
    before = cache.memory_stats()
    big = dl.PointCloud(ctx, nc.cloud(rng, 5000))  # more than a slab: one of its own
    tiny_points = nc.cloud(rng, 3 * 3000, zeros=True).reshape(3000, 3, 3)
    tiny = [(nc.info_of(rng, i), tiny_points[i][:1 + i % 3], tiny_points[i][:i % 2]) for i in range(3000)]
    cache.add(big, **nc.info_of(rng, 0))
    big.close()
    add_nodes(dl, ctx, cache, tiny)
    after = cache.memory_stats()
    assert after["slabs"] > before["slabs"] + 10 and after["bytes_used"] <= after["bytes_reserved"]
    assert cache.size()[0] == 3 + 1 + 3000
    assert assert_clouds(cache, early, poses=nc.random_pose(np.random.default_rng(2)))[0] == clouds_before
    assert assert_messages(cache, early)[0] == messages_before
    assert cache.memory_stats()["table_bytes"] > after["table_bytes"] >= before["table_bytes"] > 0  # mirrored lazily, and grown
    _, stats = assert_messages(cache, tiny, first=4)
    assert (stats["chunks"], stats["launches"], stats["readbacks"]) == (1, 4, 1)
    assert_clouds(cache, tiny, first=4)
    cache.clear()
    assert cache.size() == (0, 0, 0) and cache.memory_stats()["slabs"] == 1 and cache.memory_stats()["bytes_used"] == 0
    add_nodes(dl, ctx, cache, early[:1])
    assert assert_messages(cache, early[:1])[0] == messages_before[:len(nc.node_message(*early[0]))]
    cache.close()


# ---- the message's corners ----
@pytest.mark.parametrize("records", [7, 8, 963, 964])
def test_payload_sizes_around_the_varint_steps(dl, ctx, records):
    """full 17-byte records, no origin bytes: RangeData's length is 2 + 17 n -- 121 / 138 around 128, 16 373 / 16 390 around 16 384"""
    rng = np.random.default_rng(records)
    info = nc.info_of(rng, 1)
    info["origin_in_local"] = np.zeros(3, dtype=np.float32)
    nodes = [(info, nc.cloud(rng, records), nc.cloud(rng, 0))]
    assert len(nc.varint(2 + 17 * records)) == {7: 1, 8: 2, 963: 2, 964: 3}[records]
    cache = dl.NodeClouds(ctx)
    add_nodes(dl, ctx, cache, nodes)
    assert_messages(cache, nodes)
    cache.close()


@pytest.mark.parametrize("timestamp,trajectory_id,node_index", [(0, 0, 0), (5, -1, -7), (-3, 2 ** 31 - 1, 1)])
def test_omitted_and_negative_scalars(dl, ctx, timestamp, trajectory_id, node_index):
    rng = np.random.default_rng(3)
    info = nc.info_of(rng, 0, timestamp=timestamp, trajectory_id=trajectory_id)
    info["node_index"] = node_index
    info["origin_in_local"] = np.array([0.0, -0.0, np.nan], dtype=np.float32)
    info["local_pose7"] = np.array([0.0, -0.0, 1.5, 0.0, 1.0, 0.0, -0.0])
    for misses in (0, 6):
        nodes = [(info, nc.cloud(rng, 9, zeros=True), nc.cloud(rng, misses, zeros=True))]
        cache = dl.NodeClouds(ctx)
        add_nodes(dl, ctx, cache, nodes)
        msg, _ = assert_messages(cache, nodes)
        if trajectory_id < 0:
            assert bytes([2 << 3]) + nc.varint(trajectory_id) in msg
        cache.close()


def test_capacity_too_small_writes_nothing_past_it(seventy, dl):
    import ctypes as C
    cache, nodes = seventy
    u8p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int64)

    def raw(proto, limit, buffer, capacity, offsets):
        limits = dl.NodeCloudsLimits(limit)
        if proto:
            return cache._L.dliom_node_clouds_to_proto(cache.h, 0, len(nodes), C.byref(limits), buffer.ctypes.data_as(u8p), capacity,
                                                       offsets.ctypes.data_as(i64p), None)
        return cache._L.dliom_node_clouds_pack_point_cloud2(cache.h, 0, len(nodes), None, C.byref(limits), buffer.ctypes.data_as(u8p), capacity,
                                                            offsets.ctypes.data_as(i64p), None)
    for proto, limit in ((True, 300), (True, 0), (False, 300)):
        full, offsets, _, status = (cache.to_proto if proto else cache.pack_point_cloud2)(max_points_per_chunk=limit)
        assert status == 0
        for capacity in (0, 1, len(full) // 2, len(full) - 1):
            guarded = np.full(capacity + 64, 0xA5, dtype=np.uint8)  # the call is told of `capacity` bytes: 64 guard bytes behind
            got_offsets = np.zeros(len(nodes) + 1, dtype=np.int64)
            assert raw(proto, limit, guarded, capacity, got_offsets) == dl.ERR_CAPACITY
            assert np.array_equal(got_offsets, offsets) and got_offsets[-1] == len(full)  # the size is reported
            assert np.all(guarded[capacity:] == 0xA5)
            written = guarded[:capacity]
            assert np.all((written == full[:capacity]) | (written == 0xA5))  # whole chunks that fit, or nothing
        exact = np.full(len(full) + 64, 0xA5, dtype=np.uint8)
        assert raw(proto, limit, exact, len(full), np.zeros(len(nodes) + 1, dtype=np.int64)) == 0
        assert np.array_equal(exact[:len(full)], full) and np.all(exact[len(full):] == 0xA5)


# ---- from_proto ----
def test_from_proto_add_pack_is_pb_range_data_to_ros_cloud(dl, ctx):
    """a range-data file's messages -> from_proto -> add -> two poses per node: global_pose * (local_pose.inverse() * p)"""
    rng = np.random.default_rng(12)
    nodes = make_nodes(12, [(400, 30), (0, 0), (TILE + 3, 0), (5, 5)], zeros=False)
    cache = dl.NodeClouds(ctx)
    poses, want = [], []
    for info, returns, misses in nodes:
        parsed, r, m = dl.node_range_data_from_proto(ctx, nc.node_message(info, returns, misses))
        assert parsed["timestamp"] == info["timestamp"] and np.array_equal(parsed["local_pose7"], info["local_pose7"])
        assert np.array_equal(r.download().view(np.uint32), returns.view(np.uint32)) and len(m) == len(misses)
        cache.add(r, m, **parsed)
        r.close()
        m.close()
        local, global_pose = np.asarray(parsed["local_pose7"], dtype=np.float32), nc.random_pose(rng)
        poses.append(np.stack([dl.rigid3f_inverse(local), global_pose]))
        want.append(nc.point_cloud2_data(returns, [nc.rigid3f_inverse(local), global_pose]))
    out, offsets, _, status = cache.pack_point_cloud2(poses=np.stack(poses), per_node=True)
    assert status == 0
    for got, w in zip(split(out, offsets), want):
        assert_bytes(got, w)
    assert_messages(cache, nodes)  # and back to the same file
    with pytest.raises(dl.DliomError):
        dl.node_range_data_from_proto(ctx, nc.node_message(*nodes[0])[:-3])
    cache.close()


# ---- the C++ adapters ----
def build_adapter(tmp_path):
    exe = str(tmp_path / "node_clouds_adapter")
    libdir = os.path.join(nc.ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(nc.ROOT, "tests", "cpp", "node_clouds_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    return exe


def read_blob(blob, at):
    n_offsets, n_bytes = struct.unpack_from("<qq", blob, at)
    offsets = np.frombuffer(blob, dtype=np.int64, count=n_offsets, offset=at + 16)
    data = blob[at + 16 + 8 * n_offsets:at + 16 + 8 * n_offsets + n_bytes]
    return [data[offsets[i]:offsets[i + 1]] for i in range(n_offsets - 1)], at + 16 + 8 * n_offsets + n_bytes


def test_cpp_node_cloud_cache(dl, ctx, tmp_path):
    """SerializeRangeData, FullMapCloud and GlobalClouds of cartographer_ros::NodeCloudCache: equal to the adapter's host loops
    (checked in the program) and to the model; trajectories in map order, a scan without a node skipped"""
    rng = np.random.default_rng(21)
    sizes = [(300, 9), (0, 0), (TILE + 1, 0), (40, 40), (1000, 3), (7, 0)]
    trajectories = [2, 0, 2, 0, 0, 2]
    nodes = make_nodes(21, sizes, zeros=True)
    for (info, _, _), t in zip(nodes, trajectories):
        info["trajectory_id"] = t
    local_to_map = nc.random_pose_d(rng)
    table = {nodes[i][0]["timestamp"]: nc.random_pose_d(rng) for i in (0, 1, 3, 5)}
    src, dst = str(tmp_path / "nodes.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<2i", len(nodes), len(table)) + np.asarray(local_to_map, dtype=np.float64).tobytes())
        for time, pose in table.items():
            f.write(struct.pack("<q", time) + np.asarray(pose, dtype=np.float64).tobytes())
        for info, returns, misses in nodes:
            f.write(struct.pack("<3i", info["trajectory_id"], len(returns), len(misses)) + struct.pack("<q", info["timestamp"]))
            f.write(np.asarray(info["local_pose7"], dtype=np.float64).tobytes() + nc.f32(info["origin_in_local"]).tobytes())
            f.write(nc.f32(returns).tobytes() + nc.f32(misses).tobytes())
    out = subprocess.run([build_adapter(tmp_path), "nodes", src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "NODE CLOUDS ADAPTER DONE scans 6 kept 4" in out.stdout, out.stdout + out.stderr
    blob = open(dst, "rb").read()
    map_order = [i for t in sorted(set(trajectories)) for i in range(len(nodes)) if trajectories[i] == t]
    messages, at = read_blob(blob, 0)
    assert len(messages) == len(nodes)
    for got, i in zip(messages, map_order):
        assert_bytes(got, nc.node_message(*nodes[i]))
    full, at = read_blob(blob, at)
    to_map = np.asarray(local_to_map, dtype=np.float32)
    for got, i in zip(full, map_order):
        assert_bytes(got, nc.point_cloud2_data(nodes[i][1], [to_map]))
    global_clouds, at = read_blob(blob, at)
    assert at == len(blob) and len(global_clouds) == 4
    for got, i in zip(global_clouds, (0, 1, 3, 5)):
        info = nodes[i][0]
        local = np.asarray(info["local_pose7"], dtype=np.float32)
        assert_bytes(got, nc.point_cloud2_data(nodes[i][1], [nc.rigid3f_inverse(local), np.asarray(table[info["timestamp"]], dtype=np.float32)]))
    # ... and the Python side gives the same messages
    cache = dl.NodeClouds(ctx)
    add_nodes(dl, ctx, cache, [nodes[i] for i in map_order])
    python_messages, offsets, _, _ = cache.to_proto()
    assert split(python_messages, offsets) == messages
    cache.close()


def test_front_end_scan_handed_to_the_cache(dl, tmp_path):
    """LocalTrajectoryBuilder3D with SetNodeCloudCache: what the cache kept of every matched scan equals the host
    range_data_in_local of the same MatchingResult, bit for bit (compared in the program), with its time, pose and origin"""
    from dliom import synth
    from test_gpu_parity import FRONT_END_OPTS
    noise = [0.08, 0.004, 4e-5, 2e-6]
    T, scans_n, beams, az = 0.1, 4, 16, 256
    centers = synth.bubbles()
    st = synth.trajectory_state(0.0)
    scans = [synth.moving_scan(T * k, beams, az, centers) for k in range(1, scans_n + 1)]
    imus = [synth.imu_samples(T * (k - 1), T * k, 200.0) for k in range(1, scans_n + 1)]
    path = str(tmp_path / "stream.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("4i", scans_n, len(scans[0]), len(imus[0][1]) - 1, 1))
        f.write(np.asarray(st, dtype=np.float64).tobytes())
        f.write(bytes(dl.front_end_options_struct(FRONT_END_OPTS)))
        f.write(np.asarray(noise, dtype=np.float64).tobytes())
        for (dt, acc, gyr), sc in zip(imus, scans):
            rows = np.concatenate([np.full((len(acc) - 1, 1), dt), acc[:-1], gyr[:-1]], axis=1)
            f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(sc, dtype=np.float32).tobytes())
    out = subprocess.run([build_adapter(tmp_path), "frontend", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "NODE CLOUDS FRONT END DONE results" in out.stdout, out.stdout + out.stderr
    assert int(out.stdout.split("results")[1].split()[0]) >= 2
