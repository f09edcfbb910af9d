"""dliom_gzip_host and dliom_gzip_bound (dliom.h "gzip on the device") against the independent Python model of
tests/gzip_common.py, byte for byte, and against zlib as the decoder.  No GPU."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gzip_common as gz  # noqa: E402

NAMES = ["dliom_gzip_bound", "dliom_gzip_host", "dliom_gzip", "dliom_gzip_segments", "dliom_grid_xray_texture_gzip",
         "dliom_node_clouds_to_pbstream"]


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def cases():
    return gz.cases()


def test_host_equals_the_model_and_zlib_inflates_it(dl, cases):
    stored = 0
    for name, data in cases:
        count = {}
        want, got = gz.model(data, count), dl.gzip_host(data)
        assert got == want, (name, len(got), len(want))
        assert zlib.decompress(got, 31) == data, name
        assert len(got) <= dl.gzip_bound(len(data)), name
        assert got[:10] == gz.HEADER and got[-8:] == struct.pack("<II", zlib.crc32(data), len(data)), name
        stored += count["chunks_stored"]
    assert stored > 0


def test_the_cases_hold_what_they_name(cases):
    by_name = dict(cases)
    for name, data in cases:
        if name.startswith("length "):
            assert int(name.split()[1]) in gz.token_lengths(data), name
        if name.startswith("distance ") and name.split()[1].rstrip(",").isdigit():
            assert int(name.split()[1].rstrip(",")) in gz.token_distances(data), name
    assert {258} == gz.token_lengths(by_name["run 259"]) and {1} == gz.token_distances(by_name["run 259"])
    cut = by_name["distance 4093, cut at the chunk end"]
    assert (4093, 3, 4093) in gz.tokens_of(cut[:gz.CHUNK]) and cut[3:8] == cut[gz.CHUNK:gz.CHUNK + 5]
    straddle = by_name["a pattern across the chunk boundary"]
    assert straddle[gz.CHUNK - 4:gz.CHUNK] == straddle[gz.CHUNK:gz.CHUNK + 4] and gz.tokens_of(straddle[gz.CHUNK:])[0][2] == 0
    wins, ties = by_name["fixed wins by a byte"], by_name["fixed ties with stored"]
    assert len(gz.fixed_form(wins, True)) + 1 == len(gz.stored_form(wins, True))
    assert len(gz.fixed_form(ties, True)) == len(gz.stored_form(ties, True)) and not gz.chunk_form(ties, True)[1]
    count = {}
    gz.model(by_name["10000 random bytes"], count)
    assert count == {"chunks": 3, "chunks_stored": 3}
    nine_bit = gz.model(by_name["all byte values x 3"])
    assert zlib.decompress(nine_bit, 31) == by_name["all byte values x 3"]


def test_bound_formula(dl):
    assert [dl.gzip_bound(n) for n in (0, 1, 4096, 4097)] == [23, 24, 18 + 4096 + 5, 18 + 4097 + 10]
    for n in (0, 1, 4095, 4096, 4097, 8192, 8193, 720000, 2 ** 31 - 1):
        assert dl.gzip_bound(n) == gz.bound(n), n
    assert dl.load_library().dliom_gzip_bound(-1) == -1
    assert dl.GZIP_CHUNK == gz.CHUNK


def test_names_are_bound_declared_and_exported(dl):
    bound = {name for name, _, _ in dl.SYMBOLS}
    header = open(os.path.join(gz.ROOT, "include", "dliom.h")).read()
    lib = C.CDLL(dl.LIB_PATH)
    for name in NAMES:
        assert name in bound and name + "(" in header and hasattr(lib, name), name
    for name in ("gzip", "gzip_host", "gzip_segments", "gzip_bound", "grid_xray_texture_gzip"):
        assert hasattr(dl, name), name
    assert hasattr(dl.NodeClouds, "to_pbstream")
    assert "#define DLIOM_GZIP_CHUNK 4096" in header and "dliom_gzip_stats" in header
    assert [f for f, _ in dl.GzipStats._fields_] == ["chunks", "chunks_stored", "read_backs", "bytes_downloaded"]
    assert C.sizeof(dl.GzipStats) == 32


def test_refusals(dl):
    L = dl.load_library()
    E = dl.ERR_INVALID_ARGUMENT
    data = np.frombuffer(b"hello hello hello", dtype=np.uint8)
    out, size = np.zeros(64, dtype=np.uint8), C.c_int64(-5)
    p, o = data.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    offsets = (C.c_int64 * 2)(0, data.size)
    assert L.dliom_gzip_host(None, data.size, o, 64, C.byref(size)) == E
    assert L.dliom_gzip_host(p, data.size, None, 64, C.byref(size)) == E
    assert L.dliom_gzip_host(p, data.size, o, 64, None) == E
    assert L.dliom_gzip_host(p, -1, o, 64, C.byref(size)) == E and L.dliom_gzip_host(p, data.size, o, -1, C.byref(size)) == E
    assert L.dliom_gzip(None, p, data.size, o, 64, C.byref(size), None) == E
    assert L.dliom_gzip_segments(None, p, offsets, 1, o, 64, offsets, None) == E
    assert L.dliom_grid_xray_texture_gzip(None, None, o, 64, C.byref(size), None, None, None, None, None) == E
    assert L.dliom_node_clouds_to_pbstream(None, 0, 0, None, o, 64, offsets, None, None) == E
    # a capacity one byte short: the size, and nothing written
    member = dl.gzip_host(data.tobytes())
    out[:] = 0xee
    assert L.dliom_gzip_host(p, data.size, o, len(member) - 1, C.byref(size)) == dl.ERR_CAPACITY
    assert size.value == len(member) and bytes(out) == b"\xee" * 64
    assert L.dliom_gzip_host(p, data.size, o, len(member), C.byref(size)) == dl.OK and bytes(out[:len(member)]) == member
    with pytest.raises(dl.DliomError) as e:
        dl.gzip_host(data.tobytes(), capacity=len(member) - 1)
    assert e.value.status == dl.ERR_CAPACITY
    # empty input needs no pointer
    assert L.dliom_gzip_host(None, 0, o, 64, C.byref(size)) == dl.OK and zlib.decompress(bytes(out[:size.value]), 31) == b""
