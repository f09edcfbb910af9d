"""Gzip members made on the device (dliom_gzip, dliom_gzip_segments, dliom_grid_xray_texture_gzip,
dliom_node_clouds_to_pbstream) against the independent Python model of tests/gzip_common.py, byte for byte, and against
zlib as the decoder."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gzip_common as gz  # noqa: E402
import node_clouds_common as nc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """[(name, input, the model's member, the model's chunk counts)]: computed once, shared, never changed"""
    out = []
    for name, data in gz.cases():
        count = {}
        out.append((name, data, gz.model(data, count), count))
    return out


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), k, got[max(0, k - 12):k + 12], want[max(0, k - 12):k + 12]


def test_single_calls_equal_the_model(dl, ctx, cases):
    for name, data, want, count in cases:
        got, stats = dl.gzip(ctx, data, with_stats=True)
        assert got == want, (name,) + first_difference(got, want)
        assert zlib.decompress(got, 31) == data, name
        assert stats["chunks"] == count["chunks"] and stats["chunks_stored"] == count["chunks_stored"], (name, stats, count)
        assert stats["read_backs"] == 1 and stats["bytes_downloaded"] == len(got) <= dl.gzip_bound(len(data)), (name, stats)
    stored = {name: count["chunks_stored"] for name, _, _, count in cases}
    assert stored["10000 random bytes"] == 3 and stored["fixed ties with stored"] == 0 and stored["n=0"] == 1


def test_all_cases_as_segments_of_one_call(dl, ctx, cases):
    """every case a segment, at whatever alignment the ones in front leave it"""
    blob = b"".join(data for _, data, _, _ in cases)
    offsets = np.cumsum([0] + [len(data) for _, data, _, _ in cases])
    members, stats = dl.gzip_segments(ctx, blob, offsets, with_stats=True)
    assert len(members) == len(cases)
    for (name, data, want, _), got in zip(cases, members):
        assert got == want, (name,) + first_difference(got, want)
    assert stats["read_backs"] == 1 and stats["bytes_downloaded"] == sum(len(m) for m in members)
    assert stats["chunks"] == sum(count["chunks"] for _, _, _, count in cases)
    assert stats["chunks_stored"] == sum(count["chunks_stored"] for _, _, _, count in cases) > 0


@pytest.mark.parametrize("k", [1, 3, 17])
def test_segments_equal_single_calls(dl, ctx, k):
    rng = np.random.default_rng(k)
    sizes = [0, 5000, 1, 0, 4096, 12289, 3, 4097, 0, 70, 8192, 2, 4095, 0, 9000, 258, 0][:k] if k > 1 else [6001]
    parts = []
    for i, n in enumerate(sizes):
        symbols = (2, 256, 5)[i % 3]
        parts.append(rng.integers(0, symbols, size=n, dtype=np.uint8).tobytes())
    lead = b"not part of any segment"
    blob = lead + b"".join(parts)
    offsets = len(lead) + np.cumsum([0] + sizes)
    members = dl.gzip_segments(ctx, blob, offsets)
    assert len(members) == k
    for part, member in zip(parts, members):
        assert member == dl.gzip(ctx, part) == gz.model(part) and zlib.decompress(member, 31) == part


def test_two_calls_give_equal_bytes(dl, ctx, cases):
    data = b"".join(data for _, data, _, _ in cases[-12:])
    first = dl.gzip(ctx, data)
    assert first == dl.gzip(ctx, data) and zlib.decompress(first, 31) == data


def test_refusals(dl, ctx):
    L = ctx._L
    u8p = C.POINTER(C.c_uint8)
    data = np.frombuffer(bytes(range(200)) * 50, dtype=np.uint8)
    member = dl.gzip(ctx, data)
    out, size = np.full(len(member) + 16, 0xee, dtype=np.uint8), C.c_int64(-1)
    p, o = data.ctypes.data_as(u8p), out.ctypes.data_as(u8p)
    assert L.dliom_gzip(ctx.h, p, data.size, o, len(member) - 1, C.byref(size), None) == dl.ERR_CAPACITY
    assert size.value == len(member) and bytes(out) == b"\xee" * len(out)  # the size, and nothing written
    assert L.dliom_gzip(ctx.h, p, data.size, o, len(member), C.byref(size), None) == dl.OK
    assert bytes(out[:len(member)]) == member and bytes(out[len(member):]) == b"\xee" * 16
    E = dl.ERR_INVALID_ARGUMENT
    offsets, out_offsets = (C.c_int64 * 3)(0, 100, 50), (C.c_int64 * 3)()
    assert L.dliom_gzip(ctx.h, None, 5, o, 64, C.byref(size), None) == E
    assert L.dliom_gzip(ctx.h, p, 5, None, 64, C.byref(size), None) == E and L.dliom_gzip(ctx.h, p, 5, o, 64, None, None) == E
    assert L.dliom_gzip_segments(ctx.h, p, offsets, 2, o, 64, out_offsets, None) == E  # descending
    assert L.dliom_gzip_segments(ctx.h, p, None, 2, o, 64, out_offsets, None) == E
    assert L.dliom_gzip_segments(ctx.h, p, offsets, 1, o, 64, None, None) == E
    too_large = (C.c_int64 * 2)(0, 2 ** 31)  # refused before a byte is read
    assert L.dliom_gzip_segments(ctx.h, p, too_large, 1, o, 64, out_offsets, None) == dl.ERR_TOO_LARGE
    assert L.dliom_gzip(ctx.h, p, 2 ** 31, o, 64, C.byref(size), None) == dl.ERR_TOO_LARGE


def small_grid(dl, ctx, resolution, seed):
    L = dl.load_library()
    rng = np.random.default_rng(seed)
    cells = rng.integers(-40, 40, size=(3000, 3))
    probs = rng.uniform(0.3, 0.9, size=len(cells)).astype(np.float32)
    values = np.array([L.dliom_probability_to_value(C.c_float(p)) for p in probs], dtype=np.uint16)
    g = dl.HybridGrid(ctx, resolution)
    g.set_values(cells, values)
    return g


def test_gzipped_texture_inflates_to_the_texture(dl, ctx):
    g = small_grid(dl, ctx, 0.1, 7)
    for pose in ([0, 0, 0, 1, 0, 0, 0], [1.25, -3.5, 0.4, np.cos(0.35), 0.0, 0.0, np.sin(0.35)]):
        w, h, res, slice_pose, cells = dl.grid_xray_texture(g, pose)
        gw, gh, gres, gslice, cells_gz, stats = dl.grid_xray_texture_gzip(g, pose, with_stats=True)
        assert (gw, gh, gres) == (w, h, res) and gslice.tobytes() == slice_pose.tobytes() and w * h > 4096
        assert zlib.decompress(cells_gz, 31) == cells.tobytes() and cells_gz == gz.model(cells.tobytes())
        assert stats["read_backs"] == 1 and stats["bytes_downloaded"] == len(cells_gz) < cells.size
    g.close()


def test_gzipped_texture_of_an_empty_grid(dl, ctx):
    g = dl.HybridGrid(ctx, 0.1)
    w, h, res, slice_pose, cells = dl.grid_xray_texture(g, [0, 0, 1, 1, 0, 0, 0])
    gw, gh, gres, gslice, cells_gz = dl.grid_xray_texture_gzip(g, [0, 0, 1, 1, 0, 0, 0])
    assert (gw, gh, gres) == (w, h, res) == (0, 0, res) and gslice.tobytes() == slice_pose.tobytes()
    assert cells_gz == gz.model(b"") and zlib.decompress(cells_gz, 31) == b""
    g.close()


NODE_SIZES = [(300, 9), (0, 0), (nc.TILE + 1, 0), (40, 40), (5000, 3), (7, 0), (1, 1), (900, 900), (2, 0)]


def make_cache(dl, ctx, sizes):
    rng = np.random.default_rng(len(sizes))
    cache = dl.NodeClouds(ctx)
    for i, (n, m) in enumerate(sizes):
        r, mi = dl.PointCloud(ctx, nc.cloud(rng, n, zeros=True)), dl.PointCloud(ctx, nc.cloud(rng, m, zeros=True))
        cache.add(r, mi, **nc.info_of(rng, i))
        r.close()
        mi.close()
    return cache


def check_records(dl, cache, count, **kw):
    messages, offsets, _, status = cache.to_proto()
    assert status == dl.OK
    out, record_offsets, stats, gz_stats, status = cache.to_pbstream(fill=0xee, **kw)
    assert status == dl.OK and len(record_offsets) == count + 1 and record_offsets[0] == 0
    for i in range(count):
        message = messages[offsets[i]:offsets[i + 1]].tobytes()
        record = out[record_offsets[i]:record_offsets[i + 1]].tobytes()
        assert struct.unpack_from("<q", record)[0] == len(record) - 8, i
        assert zlib.decompress(record[8:], 31) == message, i
        assert record[8:] == gz.model(message), i
    assert bytes(out[record_offsets[count]:]) == b"\xee" * (len(out) - record_offsets[count])
    assert gz_stats["bytes_downloaded"] == record_offsets[count] and stats["bytes"] == record_offsets[count]
    return stats, gz_stats


@pytest.mark.parametrize("count", [1, 2, 9])
def test_pbstream_records(dl, ctx, count):
    """the zero-point node is the second"""
    cache = make_cache(dl, ctx, NODE_SIZES[:count])
    stats, gz_stats = check_records(dl, cache, count)
    assert stats["chunks"] == 1 and gz_stats["read_backs"] == 1
    cache.close()


def test_pbstream_records_across_a_chunk_limit(dl, ctx):
    cache = make_cache(dl, ctx, NODE_SIZES)
    stats, gz_stats = check_records(dl, cache, len(NODE_SIZES), max_points_per_chunk=1000)
    assert stats["chunks"] > 2 and gz_stats["read_backs"] == stats["chunks"]
    # a capacity short of the records: the offsets are owed, the bytes behind the capacity are not
    full, offsets, _, _, _ = cache.to_pbstream()
    short, short_offsets, _, _, status = cache.to_pbstream(capacity=int(offsets[-1]) - 1, fill=0xee, max_points_per_chunk=1000)
    assert status == dl.ERR_CAPACITY and np.array_equal(short_offsets, offsets)
    cache.close()
