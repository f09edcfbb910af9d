"""Gzip on the device beyond the sizes of tests/test_gpu_gzip.py, byte for byte against the Python model of
tests/gzip_common.py and against zlib as the decoder:
  * more segments in one call than one launch chain takes (dliom.h: "up to 8190 segments"), so that gzip_on_device's later
    chains run -- their offsets shifted, their bytes downloaded behind the earlier ones, capacities refused across chains --
    and the same from inside dliom_node_clouds_to_pbstream with more nodes than that in one chunk;
  * segments of up to 2^26 + 4133 bytes, whose chunks place their CRC share with pow2[12..26] of gzip_format.h's tables,
    alone and among short segments, and the context's scratch used again after it has grown;
  * a texture of more than 2^20 bytes.
A segment's chunks are drawn from six fixed ones (gzip_common.big_segment), so the model runs once a distinct chunk."""
import ctypes as C
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gzip_common as gz  # noqa: E402
import node_clouds_common as nc  # noqa: E402

pytestmark = pytest.mark.gpu

U8P, I64P, F64P = C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_double)
LEAD = b"not part of any segment"
LONG = (1 << 26) + 4096 + 37


def chain_segments():
    """the segments of one launch chain, from the header's text"""
    header = open(os.path.join(gz.ROOT, "include", "dliom.h")).read()
    found = re.findall(r"one launch chain for up to (\d+) segments", header)
    assert len(found) == 1
    return int(found[0])


G = chain_segments()
KS = [G, G + 1, 2 * G + 3]


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
def memo():
    return {}


def first_difference(got, want):
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    n = min(len(a), len(b))
    wrong = np.flatnonzero(a[:n] != b[:n])
    k = int(wrong[0]) if len(wrong) else n
    return len(got), len(want), k, bytes(got[max(0, k - 12):k + 12]), bytes(want[max(0, k - 12):k + 12])


# ---- segments across launch chains ----
@pytest.fixture(scope="module")
def pool():
    """about 40 payloads of the lengths 0, 1, 2, 3, 5, 70, 258, 259, 4095, 4096, 4097, 8193 -> [(payload, the model's
    member, its chunk counts)], and the indices of the short, the middle and the long ones"""
    rng = np.random.default_rng(8190)
    payloads = [b""]
    for n in (1, 2, 3, 5, 70):
        payloads += [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 2, n, dtype=np.uint8).tobytes(), b"z" * n,
                     bytes(range(140, 140 + n))]
    for n in (258, 259):
        payloads += [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 3, n, dtype=np.uint8).tobytes(), b"q" * n]
    for n in (4095, 4096, 4097, 8193):
        payloads += [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 3, n, dtype=np.uint8).tobytes(),
                     rng.integers(0, 2, n, dtype=np.uint8).tobytes()]
    out = []
    for p in payloads:
        count = {}
        out.append((p, gz.model(p, count), count))
    assert len(out) == 39 and sorted({len(p) for p in payloads}) == [0, 1, 2, 3, 5, 70, 258, 259, 4095, 4096, 4097, 8193]
    short = [i for i, p in enumerate(payloads) if 0 < len(p) <= 70]
    middle = [i for i, p in enumerate(payloads) if 70 < len(p) < 4095]
    long_ = [i for i, p in enumerate(payloads) if len(p) >= 4095]
    two_chunks = [i for i, p in enumerate(payloads) if len(p) == 4097]
    return out, short, middle, long_, two_chunks


_calls = {}


def call_of(pool, k):
    """the k segments of a call -> (blob, offsets, [pool index]): built once a k"""
    if k in _calls:
        return _calls[k]
    entries, short, middle, long_, two_chunks = pool
    rng = np.random.default_rng(k)
    kind = rng.random(k)
    pick = np.where(kind < 0.05, 0, np.where(kind < 0.93, rng.choice(short, k), np.where(kind < 0.985, rng.choice(middle, k), rng.choice(long_, k))))
    # empty segments at both ends of the call and of the first chain; the first chain's last non-empty segment, the second
    # chain's first non-empty one and the two on either side of the second and third chains' border have two chunks
    for n, at in enumerate((G - 2, G + 2, 2 * G - 1, 2 * G)):
        if at < k - 1:
            pick[at] = two_chunks[n % len(two_chunks)]
    for at in (0, G - 1, G, G + 1, k - 1):
        if at < k:
            pick[at] = 0
    sizes = np.array([len(entries[i][0]) for i in pick], dtype=np.int64)
    blob = LEAD + b"".join(entries[i][0] for i in pick)
    offsets = len(LEAD) + np.concatenate([[0], np.cumsum(sizes)])
    assert len(LEAD) == 23 and len(blob) < 3 << 20 and offsets[-1] == len(blob)
    _calls[k] = (blob, offsets, pick)
    return _calls[k]


def segments_raw(dl, ctx, blob, offsets, capacity, room):
    """dliom_gzip_segments into a buffer of `room` >= capacity bytes filled with 0xee -> (status, buffer, out_offsets, stats)"""
    data, off = np.frombuffer(blob, dtype=np.uint8), np.ascontiguousarray(offsets, dtype=np.int64)
    out, out_off, stats = np.full(room, 0xee, dtype=np.uint8), np.full(len(off), -1, dtype=np.int64), dl.GzipStats()
    status = ctx._L.dliom_gzip_segments(ctx.h, data.ctypes.data_as(U8P), off.ctypes.data_as(I64P), len(off) - 1, out.ctypes.data_as(U8P),
                                        int(capacity), out_off.ctypes.data_as(I64P), C.byref(stats))
    return status, out, out_off, stats.as_dict()


def wanted(pool, pick):
    entries = pool[0]
    members = [entries[i][1] for i in pick]
    return members, np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)


@pytest.mark.parametrize("k", KS)
def test_segments_across_launch_chains(dl, ctx, pool, k):
    entries = pool[0]
    blob, offsets, pick = call_of(pool, k)
    members, want_offsets = wanted(pool, pick)
    total = int(want_offsets[-1])
    status, out, out_off, stats = segments_raw(dl, ctx, blob, offsets, total + 64, total + 64)
    assert status == dl.OK
    # contiguous, in order, from 0: the members' offsets are the sums of the model's sizes
    wrong = np.flatnonzero(out_off != want_offsets)
    assert len(wrong) == 0, (k, len(wrong), wrong[:4], out_off[wrong[:4]], want_offsets[wrong[:4]])
    if out[:total].tobytes() != b"".join(members):
        for s in range(k):
            got = out[out_off[s]:out_off[s + 1]].tobytes()
            assert got == members[s], (k, s, len(entries[pick[s]][0])) + first_difference(got, members[s])
    assert bytes(out[total:]) == b"\xee" * 64
    for s in range(k):
        assert zlib.decompress(out[out_off[s]:out_off[s + 1]].tobytes(), 31) == entries[pick[s]][0], (k, s)
    assert stats["read_backs"] == -(-k // G), (k, stats)
    assert stats["chunks"] == sum(entries[i][2]["chunks"] for i in pick), (k, stats)
    assert stats["chunks_stored"] == sum(entries[i][2]["chunks_stored"] for i in pick) > 0, (k, stats)
    assert stats["bytes_downloaded"] == out_off[k] == total, (k, stats)
    # what the call was to hold
    lengths = np.diff(offsets)
    assert all(lengths[at] == 0 for at in (0, G - 1, G, G + 1, k - 1) if at < k)
    assert all(lengths[at] == 4097 for at in (G - 2, G + 2, 2 * G - 1, 2 * G) if at < k - 1)
    assert set(lengths.tolist()) == {0, 1, 2, 3, 5, 70, 258, 259, 4095, 4096, 4097, 8193}


def test_capacity_refusals_across_chains(dl, ctx, pool):
    k = 2 * G + 3
    blob, offsets, pick = call_of(pool, k)
    members, want_offsets = wanted(pool, pick)
    total = int(want_offsets[-1])
    room = total + 64
    status, full, full_off, _ = segments_raw(dl, ctx, blob, offsets, room, room)
    assert status == dl.OK and np.array_equal(full_off, want_offsets)
    # (a) one byte short of the total: the last chain does not fit
    status, out, out_off, stats = segments_raw(dl, ctx, blob, offsets, total - 1, room)
    assert status == dl.ERR_CAPACITY and np.array_equal(out_off, full_off)
    assert bytes(out[total - 1:]) == b"\xee" * (room - total + 1)
    assert stats["read_backs"] == 3
    # (b) the first chain does not fit: the later chains still owe their sizes, no byte is downloaded
    capacity = int(full_off[100])
    assert 0 < capacity < full_off[G]
    status, out, out_off, stats = segments_raw(dl, ctx, blob, offsets, capacity, room)
    assert status == dl.ERR_CAPACITY and np.array_equal(out_off, full_off)
    assert stats["read_backs"] == 3 and stats["bytes_downloaded"] == 0, stats
    assert bytes(out) == b"\xee" * room
    # (c) exact
    status, out, out_off, stats = segments_raw(dl, ctx, blob, offsets, total, room)
    assert status == dl.OK and np.array_equal(out_off, full_off)
    assert bytes(out[:total]) == bytes(full[:total]) and bytes(out[total:]) == b"\xee" * 64
    assert stats["read_backs"] == 3 and stats["bytes_downloaded"] == total


# ---- long segments ----
@pytest.fixture(scope="module")
def long_segment():
    return gz.big_segment(LONG, 26)


@pytest.fixture(scope="module")
def long_result(dl, ctx, long_segment):
    """(member, stats) of the long segment's first call on the module's context"""
    return dl.gzip(ctx, long_segment, with_stats=True)


def test_one_long_segment(dl, ctx, memo, long_segment, long_result):
    """chunk 0 has 2^26 + 37 bytes behind it, the chunks behind it every pattern of the bits 12..25"""
    got, stats = long_result
    count = {}
    want = gz.model_cached(long_segment, memo, count)
    assert got == want, first_difference(got, want)
    assert zlib.decompress(got, 31) == long_segment  # (zlib checks CRC-32 and ISIZE of what it has inflated)
    assert stats["chunks"] == 16386 == count["chunks"] and stats["read_backs"] == 1, stats
    assert stats["chunks_stored"] == count["chunks_stored"] > 1000 and stats["bytes_downloaded"] == len(got)


def test_long_segments_among_short_ones(dl, ctx, memo):
    sizes = [0, (1 << 20) + 1, 3, (1 << 22) + 4095, 4096, (1 << 24) + 4097, 1]
    parts = [gz.big_segment(n, 100 + i) for i, n in enumerate(sizes)]
    blob = LEAD + b"".join(parts)
    offsets = len(LEAD) + np.cumsum([0] + sizes)
    members, stats = dl.gzip_segments(ctx, blob, offsets, with_stats=True)
    assert len(members) == len(sizes) and stats["read_backs"] == 1
    count = {}
    for i, (part, member) in enumerate(zip(parts, members)):
        want = gz.model_cached(part, memo, count)
        assert member == want, (i,) + first_difference(member, want)
        alone = dl.gzip(ctx, part)
        assert member == alone, (i,) + first_difference(member, alone)
    assert stats["chunks"] == count["chunks"] and stats["chunks_stored"] == count["chunks_stored"]
    assert stats["bytes_downloaded"] == sum(len(m) for m in members)


def test_scratch_reuse_after_it_has_grown(dl, ctx, long_segment, long_result):
    cases = gz.cases()[:30]
    want = [gz.model(data) for _, data in cases]
    for (name, data), member in zip(cases, want):
        got = dl.gzip(ctx, data)
        assert got == member, (name,) + first_difference(got, member)
    blob = b"".join(data for _, data in cases)
    members = dl.gzip_segments(ctx, blob, np.cumsum([0] + [len(data) for _, data in cases]))
    for (name, _), got, member in zip(cases, members, want):
        assert got == member, (name,) + first_difference(got, member)
    again, stats = dl.gzip(ctx, long_segment, with_stats=True)
    assert again == long_result[0], first_difference(again, long_result[0])
    assert stats == long_result[1]


# ---- a texture of more than 2^20 bytes ----
@pytest.fixture
def wide_grid(dl, ctx):
    """4000 cells spread over 800 x 800 x 8; closed before the context is, whatever the test does"""
    L = dl.load_library()
    rng = np.random.default_rng(800)
    cells = np.concatenate([rng.integers(-400, 400, size=(4000, 2)), rng.integers(-4, 4, size=(4000, 1))], axis=1)
    probs = rng.uniform(0.55, 0.9, size=len(cells)).astype(np.float32)
    values = np.array([L.dliom_probability_to_value(C.c_float(p)) for p in probs], dtype=np.uint16)
    g = dl.HybridGrid(ctx, 0.1)
    g.set_values(cells, values)
    yield g
    g.close()


def test_texture_of_hundreds_of_chunks(dl, ctx, memo, wide_grid):
    L, g = dl.load_library(), wide_grid
    pose = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
    w, h, res, slice_pose, texture = dl.grid_xray_texture(g, pose)
    texture = texture.tobytes()
    assert 2 * w * h == len(texture) > 1 << 20
    gw, gh, gres, gslice, cells_gz, stats = dl.grid_xray_texture_gzip(g, pose, with_stats=True)
    assert (gw, gh, gres) == (w, h, res) and gslice.tobytes() == slice_pose.tobytes()
    count = {}
    want = gz.model_cached(texture, memo, count)
    assert cells_gz == want, first_difference(cells_gz, want)
    assert zlib.decompress(cells_gz, 31) == texture
    assert stats["chunks"] == count["chunks"] == -(-len(texture) // gz.CHUNK) and stats["chunks_stored"] == count["chunks_stored"]
    assert stats["read_backs"] == 1 and stats["bytes_downloaded"] == len(cells_gz)
    # the size query, and a capacity one byte short
    size, cw, ch, cres, cslice = C.c_int64(-1), C.c_int32(), C.c_int32(), C.c_double(), np.zeros(7)
    args = (C.byref(size), C.byref(cw), C.byref(ch), C.byref(cres), cslice.ctypes.data_as(F64P), None)
    assert L.dliom_grid_xray_texture_gzip(g.h, pose.ctypes.data_as(F64P), None, 0, *args) == dl.OK
    assert size.value == dl.gzip_bound(2 * w * h) == gz.bound(len(texture)) and (cw.value, ch.value) == (w, h)
    out = np.full(len(cells_gz) + 16, 0xee, dtype=np.uint8)
    size.value = -1
    assert L.dliom_grid_xray_texture_gzip(g.h, pose.ctypes.data_as(F64P), out.ctypes.data_as(U8P), len(cells_gz) - 1, *args) == dl.ERR_CAPACITY
    assert size.value == len(cells_gz) and bytes(out) == b"\xee" * len(out)
    assert L.dliom_grid_xray_texture_gzip(g.h, pose.ctypes.data_as(F64P), out.ctypes.data_as(U8P), len(cells_gz), *args) == dl.OK
    assert bytes(out[:len(cells_gz)]) == cells_gz and bytes(out[len(cells_gz):]) == b"\xee" * 16


# ---- more nodes in one chunk of to_pbstream than one launch chain takes ----
@pytest.fixture
def many_nodes(dl, ctx):
    """a cache of G + 7 nodes of 0 to 80 points, the nodes 0, G - 1, G and the last without any: four device clouds added
    again and again under differing infos.  Closed before the context is, whatever the test does."""
    count = G + 7
    rng = np.random.default_rng(count)
    clouds = {n: dl.PointCloud(ctx, nc.cloud(rng, n, zeros=True)) for n in (0, 1, 2, 40)}
    shapes = [(1, 0), (2, 1), (0, 0), (40, 0), (0, 2), (1, 1), (40, 40), (2, 2), (0, 1), (2, 40)]
    cache = dl.NodeClouds(ctx)
    try:
        for i in range(count):
            n, m = (0, 0) if i in (0, G - 1, G, count - 1) else shapes[int(rng.integers(len(shapes)))]
            cache.add(clouds[n], clouds[m], **nc.info_of(rng, i))
        for c in clouds.values():
            c.close()
        yield cache
    finally:
        cache.close()


def test_pbstream_of_more_nodes_than_a_chain(dl, ctx, many_nodes):
    cache, count = many_nodes, G + 7
    assert len(cache) == count
    messages, offsets, _, status = cache.to_proto()
    assert status == dl.OK
    out, record_offsets, stats, gz_stats, status = cache.to_pbstream(fill=0xee)
    assert status == dl.OK and stats["chunks"] == 1 and gz_stats["read_backs"] == 2, (stats, gz_stats)
    assert len(record_offsets) == count + 1 and record_offsets[0] == 0 and np.all(np.diff(record_offsets) > 8)
    modelled = set(np.linspace(1, count - 2, 59).astype(int).tolist()) | {0, G - 1, G, G + 1, count - 1}
    assert len(modelled) == 64
    for i in range(count):
        message = messages[offsets[i]:offsets[i + 1]].tobytes()
        record = out[record_offsets[i]:record_offsets[i + 1]].tobytes()
        assert struct.unpack_from("<q", record)[0] == len(record) - 8, i
        assert zlib.decompress(record[8:], 31) == message, i
        assert record[8:] == dl.gzip_host(message), i
        if i in modelled:
            assert record[8:] == gz.model(message), i
    end = int(record_offsets[count])
    assert gz_stats["bytes_downloaded"] == end == stats["bytes"]
    assert len(out) > end and bytes(out[end:]) == b"\xee" * (len(out) - end)
    # many chunks, each with one launch chain of gzip: the same bytes
    chunked, chunked_offsets, stats, gz_stats, status = cache.to_pbstream(fill=0xee, max_points_per_chunk=1000)
    assert status == dl.OK and stats["chunks"] > 2 and gz_stats["read_backs"] == stats["chunks"]
    assert np.array_equal(chunked_offsets, record_offsets) and bytes(chunked[:end]) == bytes(out[:end])
    # a capacity one byte short: the last chain of the chunk does not fit
    short, short_offsets, _, gz_stats, status = cache.to_pbstream(capacity=end - 1, fill=0xee)
    assert status == dl.ERR_CAPACITY and np.array_equal(short_offsets, record_offsets) and gz_stats["read_backs"] == 2
