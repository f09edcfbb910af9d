"""sensor::CompressedPointCloud / TrajectoryNodeData without a GPU: the numpy model against the reference's known
answers, the model's block order against a nested-loop formulation and the oracle's HybridGrid iterator, the bound check
next to 2^23, and the library's host-only framing and parsers against google.protobuf."""
import ctypes as C

import numpy as np
import pytest

import compressed_cloud_common as cc


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


# ---- the model against compressed_point_cloud_test.cc ----
@pytest.mark.parametrize("i", range(len(cc.KNOWN_SINGLE_POINTS)))
def test_model_single_points(i):
    p = cc.KNOWN_SINGLE_POINTS[i:i + 1]
    n, data = cc.compress(p)
    assert n == 1 and len(data) == 5 and data[0] == 1  # one block plus one word
    back = cc.decompress(n, data)
    assert back.shape == (1, 3) and np.all(np.abs(back - p) <= cc.PRECISION)
    n2, data2 = cc.compress(back)
    again = cc.decompress(n2, data2)
    assert np.all(np.abs(again - p) <= cc.PRECISION)


def test_model_three_points_and_empty():
    n, data = cc.compress(cc.KNOWN_THREE_POINTS)
    back = cc.decompress(n, data)
    assert n == 3 and len(back) == 3
    for p in cc.KNOWN_THREE_POINTS:
        assert np.any(np.all(np.abs(back - p) <= cc.PRECISION, axis=1))
    assert list(data) == [3, 0, 0, 0, 838, 839, 840]
    n, data = cc.compress(np.zeros((0, 3), dtype=np.float32))
    assert n == 0 and len(data) == 0 and cc.decompress(0, data).shape == (0, 3)


def test_model_no_gaps():
    cloud = cc.known_no_gaps_cloud()
    n, data = cc.compress(cloud)
    assert n == 3000 and len(data) == 3000 + 4 * 4  # -1500 .. 1499 spans the blocks -2, -1, 0, 1 on x
    back = cc.decompress(n, data)
    n2, data2 = cc.compress(back)
    assert n2 == n and np.array_equal(data2, data)
    x = np.sort(back[:, 0])
    assert np.all(np.abs(np.abs(np.diff(x)) - cc.PRECISION) <= np.float32(1e-7))


def test_cpp_restatement_equals_the_model(tmp_path):
    rng = np.random.RandomState(8)
    blocks = rng.choice(np.array([-8192, 8191, -1, 0, 7, 8, 63, 64, -64, -65]), size=(40, 3))
    pts = ((blocks[rng.randint(40, size=900)] * 1024 + rng.choice([0, 1, 511, 1023], size=(900, 3))).astype(np.float32) * cc.PRECISION)
    pts = np.clip(pts, -cc.LARGEST_ACCEPTED, cc.LARGEST_ACCEPTED).astype(np.float32)
    refused = pts[:5].copy()
    refused[3, 2] = np.nan
    clouds = [pts, cc.known_no_gaps_cloud(), cc.KNOWN_SINGLE_POINTS, np.zeros((0, 3), np.float32), refused,
              rng.uniform(-30, 30, size=(2000, 3)).astype(np.float32)]
    got, _ = cc.run_cpp_model(cc.build_cpp_model(tmp_path), tmp_path, clouds)
    for g, c in zip(got, clouds):
        want = cc.compress(c)
        assert (g is None and want is None) or (g[0] == want[0] and np.array_equal(g[1], want[1]))
    assert got[4] is None and got[0][0] == 900


# ---- the block order ----
def edge_blocks(rng, count):
    edges = np.array([-8192, 8191, -1, 0, 7, 8, 63, 64, -64, -65])
    b = rng.choice(edges, size=(count, 3))
    b[count // 2:] = rng.randint(-8192, 8192, size=(count - count // 2, 3))
    return np.unique(b, axis=0)


def nested_loop_order(blocks):
    """The iterator's walk in literal nested z, y, x loops over the three levels (meta cells, leaves, cells) of the
    shifted coordinates, visiting only what is present."""
    s = np.asarray(blocks) + 8192
    present = {tuple(int(v) for v in c): i for i, c in enumerate(s)}
    order = []
    metas = sorted({(c[2] >> 6, c[1] >> 6, c[0] >> 6) for c in present})  # the outer z, y, x loops, empty ones skipped
    for mz, my, mx in metas:
        for lz in range(8):
            for ly in range(8):
                for lx in range(8):
                    for cz in range(8):
                        for cy in range(8):
                            for cx in range(8):
                                c = (mx << 6 | lx << 3 | cx, my << 6 | ly << 3 | cy, mz << 6 | lz << 3 | cz)
                                if c in present:
                                    order.append(present[c])
    return order


def test_block_order_equals_nested_loops():
    blocks = edge_blocks(np.random.RandomState(5), 120)
    assert len(blocks) > 60
    assert list(np.argsort(cc.block_keys(blocks), kind="stable")) == nested_loop_order(blocks)


def test_block_order_equals_the_oracles_iterator(orc):
    rng = np.random.RandomState(6)
    edges = np.array([-1, 0, 7, 8, 63, 64, -64, -65, -512, 511])
    blocks = np.unique(np.concatenate([rng.choice(edges, size=(80, 3)), rng.randint(-512, 512, size=(150, 3))]), axis=0)
    grid = orc.HybridGrid(1.0)
    grid.set_values(blocks.astype(np.int32), np.full(len(blocks), 100, dtype=np.uint16))  # a cell at every block
    xyz, _ = grid.export_cells()  # the reference iterator's order
    mine = blocks[np.argsort(cc.block_keys(blocks), kind="stable")]
    assert np.array_equal(np.asarray(xyz, dtype=np.int64), mine)


# ---- the bound check ----
def test_bound_check_next_to_the_limit():
    top = cc.LARGEST_ACCEPTED
    up = np.nextafter(top, np.float32(np.inf))
    assert cc.accepted([[top, -top, 0]])[0] and not cc.accepted([[up, 0, 0]])[0] and not cc.accepted([[0, 0, -up]])[0]
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = np.zeros((1, 3), dtype=np.float32)
            p[0, axis] = bad
            assert not cc.accepted(p)[0] and cc.compress(p) is None
    n, data = cc.compress([[top, -top, 0]])
    assert list(data[:4]) == [1, 8191, -8192, 0]
    # no accepted float rounds to 2^23: the floats next to the bound, both signs
    f = top
    for _ in range(4096):
        assert cc.accepted([[f, 0, 0]])[0]
        q = cc.quantize([[f, -f, 0]])[0]
        assert q[0] < (1 << 23) and q[1] > -(1 << 23) and -8192 <= (q[1] >> 10) and (q[0] >> 10) <= 8191
        f = np.nextafter(f, np.float32(0))
    f = up
    for _ in range(64):
        assert not cc.accepted([[f, 0, 0]])[0]
        f = np.nextafter(f, np.float32(np.inf))


# ---- wire format ----
WORD_STREAMS = [
    (0, []),
    (0, [5]),  # num_points = 0 with words: framing does not validate
    (1, [1, 0, 0, 0, 0]),
    (5, [5, -1, 2, -8192, 0, 127, 128, 16383, 16384]),                      # 1, 2, 3 varint bytes, negative blocks
    (4, [2, 8191, -8192, -1, 2097151, 2097152, 2, 0, 0, 0, 268435455, 268435456]),  # 3, 4, 5 varint bytes
    (3, [3, -3, -2, -1, (1 << 30) - 1, 1, 0]),
]


@pytest.mark.parametrize("num_points,words", WORD_STREAMS)
def test_framing_is_byte_identical_to_protobuf(dl, num_points, words):
    mine = dl.compressed_point_cloud_to_proto(num_points, words)
    assert mine == cc.cloud_message_bytes(num_points, words)
    n, back = dl.compressed_point_cloud_from_proto(mine)
    assert n == num_points and list(back) == list(words)
    msg = cc.message_classes()[0]()
    msg.ParseFromString(mine)
    assert msg.num_points == num_points and list(msg.point_data) == list(words)


def varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def test_parser_accepts_unpacked_and_unknown_fields(dl):
    words = [2, -1, 0, 5, 1000, 70000]
    unpacked = b"\x08" + varint(2) + b"".join(b"\x18" + varint(w) for w in words)
    unknown = varint(9 << 3 | 2) + varint(3) + b"abc" + varint(2 << 3 | 0) + varint(77) + varint(12 << 3 | 5) + b"\0\0\0\0"
    for data in (unpacked, unknown + unpacked, unpacked + unknown, unpacked[:2] + unknown + unpacked[2:]):
        n, back = dl.compressed_point_cloud_from_proto(data)
        assert n == 2 and list(back) == words
    # a mix of both forms keeps the order
    mixed = b"\x18" + varint(2) + b"\x1a" + varint(len(varint(-1)) + 1) + varint(-1) + varint(0) + b"\x18" + varint(5)
    assert list(dl.compressed_point_cloud_from_proto(mixed)[1]) == [2, -1, 0, 5]


@pytest.mark.parametrize("data", [b"\x08", b"\x08\x80", b"\x1a\x05\x01", b"\x1a\x02\x80\x80", b"\x18", b"\x0b", b"\x1a"])
def test_parser_refuses_truncated_bytes(dl, data):
    with pytest.raises(dl.DliomError) as e:
        dl.compressed_point_cloud_from_proto(data)
    assert e.value.status == dl.ERR_INVALID_ARGUMENT


# (num_points, words) that Decompress must refuse; shared with the GPU test
MALFORMED_STREAMS = {
    "count zero": (0, [0, 0, 0, 0]),
    "count negative": (1, [-1, 0, 0, 0, 5]),
    "ends inside a header": (1, [1, 0, 0, 0, 5, 1, 0]),
    "header only": (1, [1, 0, 0]),
    "ends inside a block": (3, [3, 0, 0, 0, 5, 6]),
    "counts sum too low": (3, [2, 0, 0, 0, 5, 6]),
    "counts sum too high": (1, [2, 0, 0, 0, 5, 6]),
    "trailing words": (1, [1, 0, 0, 0, 5, 9]),
    "trailing block": (1, [1, 0, 0, 0, 5, 1, 1, 1, 1, 7]),
    "words but no points": (0, [1, 0, 0, 0, 5]),
    "point word negative": (1, [1, 0, 0, 0, -1]),
    "point word 2^30": (2, [2, 0, 0, 0, 5, 1 << 30]),
    "huge count": (1, [2 ** 31 - 1, 0, 0, 0, 5]),
    "negative num_points": (-1, []),
}


@pytest.mark.parametrize("name", sorted(MALFORMED_STREAMS))
def test_malformed_streams_are_refused(dl, name):
    num_points, words = MALFORMED_STREAMS[name]
    # the words lie at the very end of their array: the check has nothing of its own behind them to stray into
    assert not dl.compressed_point_cloud_check(num_points, np.array(words, dtype=np.int32))
    data = cc.cloud_message_bytes(num_points, words)
    n, back = dl.compressed_point_cloud_from_proto(data)  # the bytes form: parsed, then checked
    assert (n, list(back)) == (num_points, words) and not dl.compressed_point_cloud_check(n, back)


def test_well_formed_streams_pass_the_check(dl):
    assert dl.compressed_point_cloud_check(0, [])
    for cloud in (cc.KNOWN_THREE_POINTS, cc.known_no_gaps_cloud(), cc.KNOWN_SINGLE_POINTS):
        assert dl.compressed_point_cloud_check(*cc.compress(cloud))
    assert dl.compressed_point_cloud_check(2, [1, 9, 9, 9, (1 << 30) - 1, 1, -9, -9, -9, 0])


def test_framing_capacity_and_arguments(dl):
    L = dl.load_library()
    w = np.array([1, 0, 0, 0, 300], dtype=np.int32)
    n = C.c_int64()
    wp = w.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.dliom_compressed_point_cloud_to_proto(1, wp, 5, None, 0, C.byref(n)) == dl.OK and n.value == 2 + 2 + 6
    small = (C.c_uint8 * 4)()
    assert L.dliom_compressed_point_cloud_to_proto(1, wp, 5, small, 4, C.byref(n)) == dl.ERR_CAPACITY and n.value == 10
    assert bytes(small) == b"\0\0\0\0"
    assert L.dliom_compressed_point_cloud_to_proto(1, None, 5, None, 0, C.byref(n)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_compressed_point_cloud_to_proto(1, wp, -1, None, 0, C.byref(n)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_compressed_point_cloud_to_proto(1, wp, 5, None, 0, None) == dl.ERR_INVALID_ARGUMENT


def test_node_message_model_matches_the_reference_layout():
    """The protobuf message the GPU test compares with: every sub-message present, zeros omitted."""
    data = cc.node_message_bytes(0, (1, 0, 0, 0), [(0, [])] * 3, [], (0, 0, 0, 1, 0, 0, 0))
    w = b"\x21" + np.float64(1.0).tobytes()  # Quaterniond.w = 1
    assert data == b"\x12\x09" + w + b"\x1a\x00\x22\x00\x2a\x00" + b"\x3a\x0d" + b"\x0a\x00" + b"\x12\x09" + w


# ---- no device ----
def test_gpu_entry_points_fail_loudly_without_a_device(dl):
    if dl.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(dl.DliomError) as e:
        dl.Context(0)
    assert e.value.status == dl.ERR_NO_DEVICE
    L = dl.load_library()
    h, n, r = C.c_void_p(), C.c_int64(), C.c_int()
    w = np.array([1, 0, 0, 0, 1], dtype=np.int32)
    wp = w.ctypes.data_as(C.POINTER(C.c_int32))
    off = (C.c_int64 * 2)()
    # without a context there is nothing to run on: refused, never computed on the host
    assert L.dliom_cloud_decompress(None, 1, wp, 5, C.byref(h)) == dl.ERR_INVALID_ARGUMENT and not h.value
    assert L.dliom_cloud_from_compressed_proto(None, None, 0, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_clouds_compress(None, None, 0, None, 0, off, C.byref(r)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_clouds_compress_to_proto(None, None, 0, None, 0, off, C.byref(r)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_cloud_compress(None, None, None, 0, C.byref(n)) == dl.ERR_INVALID_ARGUMENT
