"""XYZ text of device batches (dliom_points_batch_pack_xyz, dliom_cloud_pack_xyz, the write_xyz / dump_num_points /
frame_id_filter adapters) against the CPU model tests/cpp/xyz_writer_model.cc -- the reference's std::ostringstream loop
-- byte for byte in every case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_batch_common as pb  # noqa: E402
import xyz_text_common as xt  # noqa: E402
from xyz_text_common import f32  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 4097]
_U8P = C.POINTER(C.c_uint8)


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
def model(tmp_path_factory):
    return xt.build_model(tmp_path_factory.mktemp("xyz_writer_model"))


def device_text(dl, ctx, pts):
    b = dl.PointsBatch(ctx, pts)
    out, n = b.pack_xyz()
    b.close()
    assert n == len(out)
    return out.tobytes()


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), k, got[max(0, k - 40):k + 40], want[max(0, k - 40):k + 40]


def assert_text(got, want):
    assert got == want, first_difference(got, want)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(dl, ctx, model, tmp_path, n):
    pts, _, _ = pb.batch_arrays(n, 77 + n, "none")
    want = xt.run_model(model, pts, tmp_path)
    assert_text(device_text(dl, ctx, pts), want)
    if n == 0:
        assert want == b""


def test_more_than_65536_points(dl, ctx, model, tmp_path):
    """257 workgroups' totals: more than one block of the scan over the workgroups, if the scan has more than one."""
    pts, _, _ = pb.batch_arrays(65537, 5, "none")
    assert_text(device_text(dl, ctx, pts), xt.run_model(model, pts, tmp_path))


@pytest.mark.parametrize("kind", ["short", "long", "by_point", "by_workgroup"])
def test_record_length_patterns(dl, ctx, model, tmp_path, kind):
    """6-byte and 39-byte records: every workgroup's range starts at another byte of a dword, and a wrong offset anywhere
    shifts everything behind it."""
    pts = xt.length_pattern(4097, kind)
    want = xt.run_model(model, pts, tmp_path)
    if kind != "long":
        assert want[:6] == b"0 0 0\n"
    if kind != "short":
        record = b"-1.17549e-38 -1.17549e-38 -1.17549e-38\n"
        assert len(record) == xt.MAX_RECORD and record in want
    # (by_workgroup: the eight odd workgroups of 256 are long, the nine even ones -- the last holds one point -- short)
    assert len(want) == {"short": 6 * 4097, "long": 39 * 4097, "by_point": 6 * 2049 + 39 * 2048,
                         "by_workgroup": 6 * 2049 + 39 * 2048}[kind]
    assert_text(device_text(dl, ctx, pts), want)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("group", ["special", "ties", "decades"])
def test_value_lists_on_every_axis(dl, ctx, model, tmp_path, group, axis):
    """Batch creation takes non-finite points as they are, so the special values run on the device too."""
    values = {"special": xt.special_values, "ties": xt.tie_values, "decades": xt.decade_values}[group]()
    pts = xt.as_axis(values, axis)
    want = xt.run_model(model, pts, tmp_path)
    assert_text(device_text(dl, ctx, pts), want)
    # and the host entry point gives the same characters
    line = want.split(b"\n")[0].split(b" ")
    assert line[axis] == dl.float_text(values[0])


def test_exponent_fields(dl, ctx, model, tmp_path):
    values = xt.exponent_field_values()
    pts = values[:len(values) // 3 * 3].reshape(-1, 3)
    assert_text(device_text(dl, ctx, pts), xt.run_model(model, pts, tmp_path))


def test_stride_sweep(dl, ctx, model, tmp_path):
    """2^20 points whose coordinates are the bit patterns at stride 1367 through all 2^32."""
    pts = xt.stride_points()
    assert_text(device_text(dl, ctx, pts), xt.run_model(model, pts, tmp_path))


def test_capacity(dl, ctx, model, tmp_path):
    pts = np.concatenate([pb.batch_arrays(1000, 3, "none")[0], xt.length_pattern(513, "by_point")])
    n = len(pts)
    want = xt.run_model(model, pts, tmp_path)
    size = len(want)
    b = dl.PointsBatch(ctx, pts)
    L = dl.load_library()
    assert b.pack_xyz_size() == size
    # exact capacity
    out, written = b.pack_xyz(capacity=size, fill=0xAB)
    assert written == size and out.tobytes() == want
    # one byte short: refused, the size reported, nothing written
    short = np.full(size - 1, 0xAB, dtype=np.uint8)
    num = C.c_int64(-1)
    assert L.dliom_points_batch_pack_xyz(b.h, short.ctypes.data_as(_U8P), size - 1, C.byref(num)) == dl.ERR_CAPACITY
    assert num.value == size and np.all(short == 0xAB)
    # room to spare: the tail keeps its fill
    out, written = b.pack_xyz(capacity=size + 64, fill=0xAB)
    assert written == size and out[:size].tobytes() == want and np.all(out[size:] == 0xAB)
    # the longest text a batch of n points can have: one call suffices
    out, written = b.pack_xyz(capacity=dl.XYZ_MAX_RECORD * n, fill=0xAB)
    assert written == size and out[:size].tobytes() == want and np.all(out[size:] == 0xAB)
    # a negative capacity is refused
    assert L.dliom_points_batch_pack_xyz(b.h, short.ctypes.data_as(_U8P), -1, C.byref(num)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_batch_pack_xyz(b.h, short.ctypes.data_as(_U8P), 10, None) == dl.ERR_INVALID_ARGUMENT
    b.close()


def test_attributes_ignored_and_batch_unchanged(dl, ctx, model, tmp_path):
    pts, it, col = pb.batch_arrays(1500, 9, "both")
    want = xt.run_model(model, pts, tmp_path)
    b = dl.PointsBatch(ctx, pts, (1.0, 2.0, 3.0), it, col)
    out, written = b.pack_xyz()
    assert out.tobytes() == want and written == len(want)
    pb.assert_batch_equals(b, (pts, it, col))
    assert b.has_intensities and b.has_colors and np.array_equal(b.origin, np.array([1, 2, 3], dtype=f32))
    b.close()


def test_synchronizations(dl, ctx):
    pts, _, _ = pb.batch_arrays(4097, 21, "none")
    b = dl.PointsBatch(ctx, pts)
    b.pack_xyz()  # warm: scratch grown
    L = dl.load_library()
    out = np.zeros(dl.XYZ_MAX_RECORD * len(pts), dtype=np.uint8)
    num = C.c_int64()
    s0 = ctx.synchronizations()
    assert L.dliom_points_batch_pack_xyz(b.h, out.ctypes.data_as(_U8P), len(out), C.byref(num)) == dl.OK
    s1 = ctx.synchronizations()
    assert L.dliom_points_batch_pack_xyz(b.h, None, 0, C.byref(num)) == dl.OK
    s2 = ctx.synchronizations()
    assert 0 <= s1 - s0 <= 2 and 0 <= s2 - s1 <= 1
    r0 = ctx.read_backs()
    assert L.dliom_points_batch_pack_xyz(b.h, out.ctypes.data_as(_U8P), len(out), C.byref(num)) == dl.OK
    assert ctx.read_backs() - r0 == 1  # the size; the text comes in the one download
    b.close()
    empty = dl.PointsBatch(ctx, np.zeros((0, 3), dtype=f32))
    s0, r0 = ctx.synchronizations(), ctx.read_backs()
    assert empty.pack_xyz_size() == 0 and empty.pack_xyz(capacity=8, fill=7)[1] == 0
    assert ctx.synchronizations() == s0 and ctx.read_backs() == r0
    empty.close()


def test_cloud_pack_equals_the_batch(dl, ctx, model, tmp_path):
    pts, _, _ = pb.batch_arrays(2049, 31, "none")
    want = xt.run_model(model, pts, tmp_path)
    cloud = dl.PointCloud(ctx, pts)
    out, written = cloud.pack_xyz()
    assert written == len(want) and out.tobytes() == want
    assert device_text(dl, ctx, pts) == want
    out, written = cloud.pack_xyz(capacity=len(want) + 5, fill=1)
    assert written == len(want) and np.all(out[len(want):] == 1)


def test_adapter_pipeline_stays_on_the_device(dl, tmp_path):
    """tests/cpp/xyz_writer_adapter.cc: assemble -> min_max_range_filter -> frame_id_filter -> dump_num_points -> write_xyz
    over four 16 x 256 scans, one of them of a dropped frame; once on device batches and once on host vectors with the
    reference's loops.  Equal files and counts; no cloud uploaded from host points; exactly the file's bytes downloaded
    (a SyncToHost anywhere would add 12 bytes a point and more)."""
    exe = xt.build_adapter(tmp_path, dl.LIB_PATH)
    times, poses, mount, messages = pb.pipeline_messages(16, 256)
    frames = ["lidar", "dropped", "lidar", "lidar"]
    messages = [(t, xyzt, it, frame) for (t, xyzt, it), frame in zip(messages, frames)]
    out = xt.run_adapter(exe, tmp_path, times, poses, mount, messages)
    text, counted = out["device"]
    assert (text, counted) == out["host"]
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 == counted
    kept = sum(len(m[1]) for m in messages if m[3] != "dropped")
    assert 0.2 * kept < counted <= kept
    assert all(len(line.split(b" ")) == 3 for line in lines[:-1])
    assert out["uploads"] == 0
    assert out["downloaded"] == len(text)
