"""The gzip adapters of the C++ header (Submap3D::ToResponseProto(pose, kGzipped), NodeCloudCache::SerializeRangeDataFramed,
common::FastGzipString) through tests/cpp/gzip_adapter.cc: what they return inflates with zlib to what the ungzipped
methods return."""
import ctypes as C
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gzip_common as gz  # noqa: E402

pytestmark = pytest.mark.gpu


def small_grid(dl, ctx, resolution, seed):
    L = dl.load_library()
    rng = np.random.default_rng(seed)
    cells = rng.integers(-40, 40, size=(3000, 3))
    probs = rng.uniform(0.3, 0.9, size=len(cells)).astype(np.float32)
    values = np.array([L.dliom_probability_to_value(C.c_float(p)) for p in probs], dtype=np.uint16)
    g = dl.HybridGrid(ctx, resolution)
    g.set_values(cells, values)
    return g


def blobs(data):
    at = 0
    while at < len(data):
        (n,) = struct.unpack_from("<q", data, at)
        yield data[at + 8:at + 8 + n]
        at += 8 + n


def test_adapters_inflate_to_the_ungzipped_methods(tmp_path):
    import dliom as dl
    ctx = dl.Context(0)
    paths = []
    for k, resolution in enumerate((0.1, 0.45)):
        g = small_grid(dl, ctx, resolution, 30 + k)
        paths.append(str(tmp_path / ("grid%d.pb" % k)))
        open(paths[-1], "wb").write(g.to_proto())
        g.close()
    ctx.close()
    exe, dst = str(tmp_path / "gzip_adapter"), str(tmp_path / "out.bin")
    libdir = os.path.dirname(dl.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(gz.ROOT, "tests", "cpp", "gzip_adapter.cc"),
                           "-L", libdir, "-ldliom", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe] + paths + [dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "GZIP ADAPTER DONE textures 2 records 5" in out.stdout, out.stdout + out.stderr
    data = open(dst, "rb").read()
    # the record count sits between the textures' blobs and the records': cut there
    parts, at = [], 0
    for _ in range(4):
        (n,) = struct.unpack_from("<q", data, at)
        parts.append(data[at + 8:at + 8 + n])
        at += 8 + n
    (count,) = struct.unpack_from("<q", data, at)
    assert count == 5
    parts += list(blobs(data[at + 8:]))
    assert len(parts) == 4 + 2 * 5 + 2
    for k in range(2):
        cells, cells_gz = parts[2 * k], parts[2 * k + 1]
        assert len(cells) > 1000 and cells_gz[:10] == gz.HEADER and zlib.decompress(cells_gz, 31) == cells
        assert cells_gz == gz.model(cells)
    for i in range(5):
        message, record = parts[4 + 2 * i], parts[5 + 2 * i]
        assert struct.unpack_from("<q", record)[0] == len(record) - 8
        assert zlib.decompress(record[8:], 31) == message and record[8:] == gz.model(message)
    text, text_gz = parts[-2], parts[-1]
    assert zlib.decompress(text_gz, 31) == text and text_gz == gz.model(text) and len(text_gz) < len(text)
