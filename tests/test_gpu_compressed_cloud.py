"""sensor::CompressedPointCloud and TrajectoryNodeData on the device against the numpy model
(tests/compressed_cloud_common.py) and google.protobuf, bit for bit and byte for byte: single clouds at the sizes where
the kernels change workgroups, batches with empty clouds and shared blocks, refusals, decompression, node data."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compressed_cloud_common as cc
from test_compressed_cloud_host import MALFORMED_STREAMS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_BLOCKS = np.array([-1, 0, 7, 8, 63, 64, -8, -9, -64, -65, 3])  # the -1/0, 7/8 and 63/64 boundaries of the three levels


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


def raster_points(block, off):
    return ((np.asarray(block, dtype=np.int64) * 1024 + off).astype(np.float32) * cc.PRECISION).astype(np.float32)


def edge_cloud(seed, n):
    """n shuffled points of both signs in about n / 3 blocks on the level boundaries, raster cells repeated."""
    rng = np.random.RandomState(seed)
    blocks = rng.choice(EDGE_BLOCKS, size=(max(n // 3, 1), 3))
    offs = rng.choice([0, 1, 511, 1022, 1023], size=(max(n // 5, 1), 3))
    pts = raster_points(blocks[rng.randint(len(blocks), size=n)], offs[rng.randint(len(offs), size=n)])
    return pts[rng.permutation(n)]


def one_block_cloud(n):
    rng = np.random.RandomState(70)
    return raster_points(np.array([3, -2, 0]), rng.randint(1, 1023, size=(n, 3)))


def own_block_cloud(n):
    rng = np.random.RandomState(71)
    side = np.arange(-21, 22)
    grid = np.stack(np.meshgrid(side, side, side, indexing="ij"), axis=-1).reshape(-1, 3)
    return raster_points(grid[rng.permutation(len(grid))[:n]], 512)


def same_stream(got, want):
    return got[0] == want[0] and got[1].dtype == np.int32 and np.array_equal(got[1], want[1])


def check_cloud(dl, ctx, pts):
    want = cc.compress(pts)
    cloud = dl.PointCloud(ctx, pts)
    got = dl.compress_point_cloud(ctx, cloud)
    assert same_stream(got, want)
    assert dl.compress_point_clouds_to_proto(ctx, [cloud])[0] == cc.cloud_message_bytes(*want)
    cloud.close()
    return want


# ---- single clouds ----
def test_known_answers(dl, ctx):
    for i in range(len(cc.KNOWN_SINGLE_POINTS)):
        n, data = check_cloud(dl, ctx, cc.KNOWN_SINGLE_POINTS[i:i + 1])
        assert n == 1 and len(data) == 5
    assert list(check_cloud(dl, ctx, cc.KNOWN_THREE_POINTS)[1]) == [3, 0, 0, 0, 838, 839, 840]
    assert len(check_cloud(dl, ctx, cc.known_no_gaps_cloud())[1]) == 3016
    n, data = check_cloud(dl, ctx, np.zeros((0, 3), dtype=np.float32))
    assert n == 0 and len(data) == 0
    top = cc.LARGEST_ACCEPTED
    assert list(check_cloud(dl, ctx, np.array([[top, -top, 0]], dtype=np.float32))[1][:4]) == [1, 8191, -8192, 0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_on_the_block_boundaries(dl, ctx, n):
    n_points, data = check_cloud(dl, ctx, edge_cloud(n, n))
    assert n_points == n and (n < 63 or len(data) < 5 * n)  # blocks are shared: input order inside a block matters


def test_input_order_is_kept_inside_a_block(dl, ctx):
    pts = raster_points(np.array([-1, 7, 63]), np.array([[5, 5, 5], [9, 9, 9], [5, 5, 5], [1, 1, 1], [9, 9, 9], [5, 5, 5]]))
    n, data = check_cloud(dl, ctx, pts)
    word = lambda o: (((o << 10) + o) << 10) + o
    assert list(data) == [6, -1, 7, 63] + [word(o) for o in (5, 9, 5, 1, 9, 5)]


def test_70001_points_in_one_block(dl, ctx):
    n, data = check_cloud(dl, ctx, one_block_cloud(70001))
    assert n == 70001 and data[0] == 70001 and len(data) == 70005


def test_70001_points_each_in_a_block_of_its_own(dl, ctx):
    n, data = check_cloud(dl, ctx, own_block_cloud(70001))
    assert n == 70001 and len(data) == 5 * 70001


# ---- batches ----
def batch_clouds(k):
    empty = np.zeros((0, 3), dtype=np.float32)
    if k == 1:
        return [edge_cloud(1, 300)]
    if k == 2:
        shared = edge_cloud(2, 200)
        return [shared, shared[::-1].copy()]  # the same blocks in both: they must not merge
    rng = np.random.RandomState(67)
    clouds = [edge_cloud(100 + i, int(rng.randint(1, 400))) for i in range(k)]
    for i in (0, 1, 30, 31, k - 1):
        clouds[i] = empty
    clouds[10] = clouds[11] = clouds[12].copy()
    return clouds


@pytest.mark.parametrize("k", [1, 2, 67])
def test_batches_equal_the_single_calls(dl, ctx, k):
    arrays = batch_clouds(k)
    clouds = [dl.PointCloud(ctx, a) for a in arrays]
    want = [cc.compress(a) for a in arrays]
    got = dl.compress_point_clouds(ctx, clouds)
    got_bytes = dl.compress_point_clouds_to_proto(ctx, clouds)
    assert len(got) == len(got_bytes) == k
    for c in range(k):
        assert same_stream(got[c], want[c]), c
        assert same_stream(dl.compress_point_cloud(ctx, clouds[c]), want[c]), c
        assert got_bytes[c] == cc.cloud_message_bytes(*want[c]), c
        assert dl.compress_point_clouds_to_proto(ctx, [clouds[c]])[0] == got_bytes[c], c
    if k == 67:  # None is the empty cloud
        with_none = [None if len(c) == 0 else c for c in clouds]
        assert all(same_stream(g, w) for g, w in zip(dl.compress_point_clouds(ctx, with_none), want))
        assert dl.compress_point_clouds_to_proto(ctx, with_none) == got_bytes
    assert dl.compress_point_clouds(ctx, []) == [] and dl.compress_point_clouds_to_proto(ctx, []) == []
    for c in clouds:
        c.close()


def test_packed_bytes_of_negative_blocks_and_small_words(dl, ctx):
    negative = raster_points(np.array([[-3, -1, -8192], [-65, 5, -9]]), np.array([[1000, 1000, 1000], [7, 0, 1023]]))
    small = raster_points(np.array([[0, 0, 0], [1, 2, 3]]), np.array([[127, 0, 0], [0, 0, 0]]))  # every word < 128
    clouds = [dl.PointCloud(ctx, a) for a in (negative, small)]
    want = [cc.compress(a) for a in (negative, small)]
    assert max(want[1][1]) < 128 and min(want[0][1]) < 0
    got = dl.compress_point_clouds_to_proto(ctx, clouds)
    assert got == [cc.cloud_message_bytes(*w) for w in want]
    assert len(got[1]) == 2 + 2 + len(want[1][1])  # one byte a word
    for c in clouds:
        c.close()


# ---- refusal ----
def raw_batch(dl, ctx, clouds, capacity, as_bytes):
    L, k = ctx._L, len(clouds)
    handles = (C.c_void_p * k)(*[c.h for c in clouds])
    offsets = np.full(k + 1, -7, dtype=np.int64)
    out = np.full(max(capacity, 1), 0x5A, dtype=np.uint8 if as_bytes else np.int32)
    refused = C.c_int(-5)
    fn = L.dliom_clouds_compress_to_proto if as_bytes else L.dliom_clouds_compress
    ptr = out.ctypes.data_as(C.POINTER(C.c_uint8 if as_bytes else C.c_int32))
    status = fn(ctx.h, handles, k, ptr, capacity, offsets.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(refused))
    return status, refused.value, offsets, out


@pytest.mark.parametrize("as_bytes", [False, True])
def test_a_refused_cloud_refuses_the_batch(dl, ctx, as_bytes):
    arrays = [edge_cloud(200 + i, 50) for i in range(5)]
    arrays[3][17, 1] = np.nan
    clouds = [dl.PointCloud(ctx, a) for a in arrays]
    status, refused, offsets, out = raw_batch(dl, ctx, clouds, 4096, as_bytes)
    assert status == dl.ERR_GRID_EXTENT and refused == 3
    assert np.all(offsets == -7) and np.all(out == 0x5A)  # nothing written
    arrays[1][49, 2] = np.float32(-8388.608)
    clouds[1].close()
    clouds[1] = dl.PointCloud(ctx, arrays[1])
    status, refused, offsets, out = raw_batch(dl, ctx, clouds, 4096, as_bytes)
    assert status == dl.ERR_GRID_EXTENT and refused == 1
    assert np.all(offsets == -7) and np.all(out == 0x5A)
    with pytest.raises(dl.CloudRefused) as e:
        (dl.compress_point_clouds_to_proto if as_bytes else dl.compress_point_clouds)(ctx, clouds)
    assert e.value.status == dl.ERR_GRID_EXTENT and e.value.first_refused == 1
    with pytest.raises(dl.CloudRefused):
        dl.compress_point_cloud(ctx, clouds[3])
    for inf in (np.inf, -np.inf):
        bad = dl.PointCloud(ctx, np.array([[0, inf, 0]], dtype=np.float32))
        assert raw_batch(dl, ctx, [clouds[0], bad], 4096, as_bytes)[:2] == (dl.ERR_GRID_EXTENT, 1)
        bad.close()
    for c in clouds:
        c.close()


@pytest.mark.parametrize("as_bytes", [False, True])
def test_capacity_reports_the_needed_size(dl, ctx, as_bytes):
    arrays = [edge_cloud(300 + i, 40 + i) for i in range(3)]
    clouds = [dl.PointCloud(ctx, a) for a in arrays]
    want = [cc.compress(a) for a in arrays]
    sizes = [len(cc.cloud_message_bytes(*w)) if as_bytes else len(w[1]) for w in want]
    status, refused, offsets, out = raw_batch(dl, ctx, clouds, sum(sizes) - 1, as_bytes)
    assert status == dl.ERR_CAPACITY and refused == -1
    assert list(offsets) == [0] + list(np.cumsum(sizes)) and np.all(out == 0x5A)
    status, refused, offsets, out = raw_batch(dl, ctx, clouds, sum(sizes), as_bytes)
    assert status == dl.OK and list(offsets) == [0] + list(np.cumsum(sizes))
    for c in clouds:
        c.close()


# ---- decompression ----
@pytest.mark.parametrize("case", ["edges", "one block", "own blocks", "empty", "limit"])
def test_decompression_equals_the_model(dl, ctx, case):
    pts = {"edges": lambda: edge_cloud(9, 1025), "one block": lambda: one_block_cloud(70001),
           "own blocks": lambda: own_block_cloud(4097), "empty": lambda: np.zeros((0, 3), dtype=np.float32),
           "limit": lambda: np.array([[cc.LARGEST_ACCEPTED, -cc.LARGEST_ACCEPTED, 0.0005]], dtype=np.float32)}[case]()
    n, data = cc.compress(pts)
    want = cc.decompress(n, data)
    cloud = dl.decompress_point_cloud(ctx, n, data)
    assert len(cloud) == n
    got = cloud.download()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    from_bytes = dl.point_cloud_from_compressed_proto(ctx, cc.cloud_message_bytes(n, data))
    assert from_bytes.download().tobytes() == want.tobytes()
    # bounds as a cloud uploaded from the host has them
    uploaded = dl.PointCloud(ctx, want)
    for c in (cloud, from_bytes):
        max_norm, abs_max = c.bounds()
        assert max_norm == uploaded.bounds()[0] and np.array_equal(abs_max, uploaded.bounds()[1])
    # Compress(Decompress(s)) on the device
    assert same_stream(dl.compress_point_cloud(ctx, cloud), cc.compress(want))
    # ... and the loaded cloud goes where every cloud goes
    if n > 0:
        filtered = cloud.voxel_filter(0.5)
        assert 0 < len(filtered) <= n
        filtered.close()
    for c in (cloud, from_bytes, uploaded):
        c.close()


def test_decompression_wraps_block_coordinates_like_int32(dl, ctx):
    data = np.array([2, (1 << 21) + 3, -(1 << 21) - 1, 5, (7 << 20) + (8 << 10) + 9, 1], dtype=np.int32)
    cloud = dl.decompress_point_cloud(ctx, 2, data)
    assert cloud.download().tobytes() == cc.decompress(2, data).tobytes()
    cloud.close()


@pytest.mark.parametrize("name", sorted(MALFORMED_STREAMS))
def test_malformed_streams_are_refused_on_the_device_path(dl, ctx, name):
    num_points, words = MALFORMED_STREAMS[name]
    with pytest.raises(dl.DliomError) as e:
        dl.decompress_point_cloud(ctx, num_points, np.array(words, dtype=np.int32))
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    with pytest.raises(dl.DliomError) as e:
        dl.point_cloud_from_compressed_proto(ctx, cc.cloud_message_bytes(num_points, words))
    assert e.value.status == dl.ERR_INVALID_ARGUMENT


# ---- node data ----
def node_case(seed):
    rng = np.random.RandomState(seed)
    hist = rng.uniform(0, 1, 120).astype(np.float32)
    hist[::7] = 0.0
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return dict(timestamp=636727077537462912 + seed, gravity=(1.0, 0.0, 0.0, 0.0), high=edge_cloud(seed, 350),
                low=edge_cloud(seed + 1, 120), histogram=hist, pose=np.concatenate([rng.uniform(-50, 50, 3), q]))


def test_node_data_is_byte_identical_and_round_trips(dl, ctx):
    case = node_case(40)
    hi, lo = dl.PointCloud(ctx, case["high"]), dl.PointCloud(ctx, case["low"])
    streams = [(0, []), cc.compress(case["high"]), cc.compress(case["low"])]
    want = cc.node_message_bytes(case["timestamp"], case["gravity"], streams, case["histogram"], case["pose"])
    got = dl.trajectory_node_data_to_proto(ctx, case["timestamp"], case["gravity"], None, hi, lo, case["histogram"], case["pose"])
    assert got == want
    # a 2D node: the filtered cloud set, no histogram, a tilted gravity alignment, timestamp 0
    g = np.array([np.cos(0.1), np.sin(0.1), 0.0, 0.0])
    want2 = cc.node_message_bytes(0, g, [streams[2], (0, []), (0, [])], [], (0, 0, 0, 1, 0, 0, 0))
    assert dl.trajectory_node_data_to_proto(ctx, 0, g, lo, None, None, [], (0, 0, 0, 1, 0, 0, 0)) == want2
    back = dl.trajectory_node_data_from_proto(ctx, got)
    assert back["timestamp"] == case["timestamp"] and np.array_equal(back["gravity_alignment"], case["gravity"])
    assert np.array_equal(back["local_pose"], case["pose"]) and back["histogram"].tobytes() == case["histogram"].tobytes()
    assert len(back["filtered_gravity_aligned"]) == 0
    for name, s in (("high_resolution", streams[1]), ("low_resolution", streams[2])):
        assert back[name].download().tobytes() == cc.decompress(*s).tobytes()  # the 0.001 rounding the model predicts
    # what protobuf parses out of the bytes is the message itself; its own re-serialisation is read back the same
    msg = cc.message_classes()[1]()
    msg.ParseFromString(got)
    assert msg.high_resolution_point_cloud.num_points == 350 and len(msg.rotational_scan_matcher_histogram) == 120
    back2 = dl.trajectory_node_data_from_proto(ctx, want2, histogram_capacity=0)
    assert len(back2["histogram"]) == 0 and back2["timestamp"] == 0 and np.array_equal(back2["gravity_alignment"], g)
    assert back2["filtered_gravity_aligned"].download().tobytes() == cc.decompress(*streams[2]).tobytes()
    with pytest.raises(dl.DliomError) as e:
        dl.trajectory_node_data_from_proto(ctx, got[:-3])
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    for c in [hi, lo] + [b[k] for b in (back, back2) for k in ("filtered_gravity_aligned", "high_resolution", "low_resolution")]:
        c.close()


def download_borrowed(L, handle):
    n = C.c_int64()
    assert L.dliom_cloud_size(handle, C.byref(n)) == 0
    out = np.zeros((n.value, 3), dtype=np.float32)
    assert L.dliom_cloud_download(handle, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return out


def test_a_front_end_node_round_trips_and_still_matches(dl, ctx):
    from dliom import synth
    from test_gpu_parity import FRONT_END_OPTS
    L = ctx._L
    fe = dl.LocalTrajectoryBuilder3D(ctx, FRONT_END_OPTS)
    gravity = np.array([1.0, 0, 0, 0])
    for s in range(4):
        truth = synth.trajectory_pose(0.1 * s)
        pts, _ = synth.scan(truth, 16, 256)
        r = fe.match(synth.perturb_pose(truth, 0.03, 0.2, seed=300 + s), np.zeros(3, np.float32), pts)
        if s < 3:
            fe.insert(int(s * 1e6), r["pose_estimate"], gravity)
    hi, lo = C.c_void_p(), C.c_void_p()
    assert L.dliom_front_end_matched_clouds(fe.h, C.byref(hi), C.byref(lo)) == 0 and hi.value and lo.value
    hi_pts, lo_pts = download_borrowed(L, hi), download_borrowed(L, lo)
    assert len(hi_pts) > 50 and len(lo_pts) > 20
    clouds = [dl._BorrowedCloud(L, h, len(p)) for h, p in ((hi, hi_pts), (lo, lo_pts))]
    hist = dl.cloud_rotational_histogram(ctx, clouds[0], 120)
    data = dl.trajectory_node_data_to_proto(ctx, 3000000, gravity, None, clouds[0], clouds[1], hist, r["pose_estimate"])
    streams = [(0, []), cc.compress(hi_pts), cc.compress(lo_pts)]
    assert data == cc.node_message_bytes(3000000, gravity, streams, hist, r["pose_estimate"])
    node = dl.trajectory_node_data_from_proto(ctx, data)
    loaded_hi, loaded_lo = node["high_resolution"].download(), node["low_resolution"].download()
    assert loaded_hi.tobytes() == cc.decompress(*streams[1]).tobytes() and loaded_lo.tobytes() == cc.decompress(*streams[2]).tobytes()
    order = np.argsort(cc.block_keys(cc.quantize(hi_pts) >> 10), kind="stable")  # the loaded cloud is in block order
    assert np.max(np.abs(loaded_hi - hi_pts[order])) <= 0.00051
    # Loop closure against the submap the node was matched in, from the node as it was and from the loaded node.  The
    # test is about the node's data, not the matcher's gates: the three thresholds are set so that the best candidate is
    # always reported, and the two results are compared.  The loaded points moved by <= 0.5 mm an axis on a 0.1 m grid:
    # a point changes its cell with probability 3 * 2 * 0.0005 / 0.1 = 3 %, by at most 0.8 in probability, so the score
    # moves by 0.024 in expectation (bound: twice that); the winner may move to a neighbouring candidate, one 0.1 m step
    # an axis.
    sub = fe.active_submap(0)
    opts = dict(branch_and_bound_depth=5, full_resolution_depth=3, min_rotational_score=0.0, min_low_resolution_score=0.0,
                linear_xy_search_window=0.6, linear_z_search_window=0.3, angular_search_window=0.2)
    qs, qn = sub["local_pose"][3:], r["pose_estimate"][3:]
    w = qs[0] * qn[0] + qs[1] * qn[1] + qs[2] * qn[2] + qs[3] * qn[3]  # conj(q_submap) * q_node: w and z
    z = qs[0] * qn[3] - qs[3] * qn[0] - qs[1] * qn[2] + qs[2] * qn[1]
    x = qs[0] * qn[1] - qs[1] * qn[0] - qs[2] * qn[3] + qs[3] * qn[2]
    y = qs[0] * qn[2] - qs[2] * qn[0] - qs[3] * qn[1] + qs[1] * qn[3]
    node_yaw = float(np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z)))
    matcher = dl.FastCorrelativeScanMatcher3D(ctx, sub["hi"], sub["lo"], hist.reshape(1, -1), [node_yaw], opts)
    results = []
    for a, b, h in ((hi_pts, lo_pts, hist), (loaded_hi, loaded_lo, node["histogram"])):
        node_data = dict(gravity_alignment=node["gravity_alignment"], high_resolution_point_cloud=a, low_resolution_point_cloud=b,
                         rotational_scan_matcher_histogram=h)
        results.append(matcher.Match(r["pose_estimate"], sub["local_pose"], node_data, 0.0))
    assert results[0]["found"] and results[1]["found"]
    assert np.all(np.abs(results[1]["pose"][:3] - results[0]["pose"][:3]) <= 0.1 + 1e-6)
    assert abs(results[1]["score"] - results[0]["score"]) <= 0.048
    assert np.linalg.norm(results[1]["pose"][:3] - r["pose_estimate"][:3]) < 0.6  # it found the node where the front end put it
    matcher.close()
    for k in ("filtered_gravity_aligned", "high_resolution", "low_resolution"):
        node[k].close()
    fe.close()


# ---- the C++ adapters ----
def test_cpp_adapters_equal_the_python_side(dl, ctx, tmp_path):
    exe = str(tmp_path / "compressed_cloud_adapter")
    libdir = os.path.join(ROOT, "d-liom_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(libdir, "cpp"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "compressed_cloud_adapter.cc"), "-L", libdir, "-ldliom",
                           "-Wl,-rpath," + libdir])
    cases = [node_case(50 + i) for i in range(3)]
    cases[1]["high"] = np.zeros((0, 3), dtype=np.float32)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            f.write(np.int64(c["timestamp"]).tobytes() + np.asarray(c["gravity"], dtype=np.float64).tobytes())
            f.write(np.asarray(c["pose"], dtype=np.float64).tobytes())
            for a in (c["high"], c["low"], c["histogram"]):
                f.write(np.int32(len(a)).tobytes() + a.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=120)
    blob = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take():
        nonlocal at
        n = int(np.frombuffer(blob, dtype=np.int64, count=1, offset=at)[0])
        at += 8 + n
        return blob[at - n:at]
    for c in cases:
        hi, lo = dl.PointCloud(ctx, c["high"]), dl.PointCloud(ctx, c["low"])
        node = dl.trajectory_node_data_to_proto(ctx, c["timestamp"], c["gravity"], None, hi, lo, c["histogram"], c["pose"])
        assert take() == node                                                  # mapping::ToProto, one node
        assert take() == node                                                  # ... the batched form over all nodes
        assert take() == dl.compress_point_clouds_to_proto(ctx, [hi])[0]       # sensor::CompressedPointCloud(cloud).ToProto()
        assert take() == dl.compress_point_clouds_to_proto(ctx, [hi])[0]       # ... built from a sensor::PointCloud
        assert take() == cc.decompress(*cc.compress(c["high"])).tobytes()      # Decompress()
        rounded = [(0, [])] + [cc.compress(cc.decompress(*cc.compress(c[k]))) for k in ("high", "low")]
        assert take() == cc.node_message_bytes(c["timestamp"], c["gravity"], rounded, c["histogram"], c["pose"])  # ToProto(FromProto(node))
        hi.close()
        lo.close()
    assert at == len(blob)
