"""X-ray images of point clouds without a GPU: the new names are bound and declared and their argument checks refuse
before anything runs; the CPU model (tests/cpp/points_xray_model.cc) on cases small enough to work out by hand, which are
written down here; dliom_points_xray_pixel (the expression the device paints with) against the model's pixels; and the
scenes of the GPU parity tests against honest()."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_xray_common as xc  # noqa: E402
from points_xray_common import IDENTITY, WHITE, f32, insert  # noqa: E402

NAMES = ("dliom_points_xray_create", "dliom_points_xray_destroy", "dliom_points_xray_insert", "dliom_points_xray_bounding_box",
         "dliom_points_xray_columns", "dliom_points_xray_voxels", "dliom_points_xray_draw", "dliom_points_xray_stats",
         "dliom_points_xray_pixel")


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return xc.build_model(tmp_path_factory.mktemp("points_xray_model"))


def test_names_are_bound_and_declared(dl):
    bound = {name for name, _, _ in dl.SYMBOLS}
    header = open(os.path.join(xc.ROOT, "include", "dliom.h")).read()
    lib = C.CDLL(dl.LIB_PATH)
    for name in NAMES:
        assert name in bound and name + "(" in header and hasattr(lib, name), name
    assert hasattr(dl, "PointsXray") and hasattr(dl, "points_xray_pixel")
    assert "points_xray_bytes" in dict(dl.MemoryStats._fields_)
    # the fields an existing caller reads keep their places: the new one is the last
    assert [n for n, _ in dl.MemoryStats._fields_][-3:] == ["outlier_table_bytes", "probability_grid_bytes", "points_xray_bytes"]


def test_argument_checks_refuse_before_anything_runs(dl):
    """No device is touched: the handles are never dereferenced (they point at zeroed host memory)."""
    L = dl.load_library()
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # stands for a context / aggregator / cloud
    out, n = C.c_void_p(), C.c_int64()
    t = (C.c_float * 7)(0, 0, 0, 1, 0, 0, 0)
    i32, u32, f3 = (C.c_int32 * 6)(), (C.c_uint32 * 4)(), (C.c_float * 6)()
    w, h, e = C.c_int32(), C.c_int32(), C.c_int()
    bad = dl.ERR_INVALID_ARGUMENT
    assert L.dliom_points_xray_create(None, 0.05, t, C.byref(out)) == bad
    assert L.dliom_points_xray_create(fake, 0.05, None, C.byref(out)) == bad
    assert L.dliom_points_xray_create(fake, 0.05, t, None) == bad
    for size in (0.0, -0.05, float("nan"), float("inf"), 1e-60, 1e60):
        assert L.dliom_points_xray_create(fake, size, t, C.byref(out)) == bad, size
    assert L.dliom_points_xray_create(fake, 0.05, (C.c_float * 7)(0, float("nan"), 0, 1, 0, 0, 0), C.byref(out)) == bad
    assert not out.value
    assert L.dliom_points_xray_destroy(None) == bad
    assert L.dliom_points_xray_insert(None, fake, None, 0) == bad and L.dliom_points_xray_insert(fake, None, None, 0) == bad
    # the zeroed cloud has 0 points: any colour count other than 0 or 1 is refused, and so is a count without colours
    assert L.dliom_points_xray_insert(fake, fake, f3, 2) == bad and L.dliom_points_xray_insert(fake, fake, f3, -1) == bad
    assert L.dliom_points_xray_insert(fake, fake, None, 1) == bad
    assert L.dliom_points_xray_bounding_box(None, i32, i32, C.byref(e)) == bad
    assert L.dliom_points_xray_bounding_box(fake, None, i32, C.byref(e)) == bad
    assert L.dliom_points_xray_bounding_box(fake, i32, i32, None) == bad
    assert L.dliom_points_xray_columns(None, i32, f3, u32, u32, 1, C.byref(n)) == bad
    assert L.dliom_points_xray_columns(fake, i32, f3, u32, u32, 1, None) == bad
    assert L.dliom_points_xray_columns(fake, i32, f3, u32, u32, -1, C.byref(n)) == bad
    assert L.dliom_points_xray_columns(fake, i32, None, u32, u32, 1, C.byref(n)) == bad  # some but not all outputs
    assert L.dliom_points_xray_voxels(None, i32, 1, C.byref(n)) == bad
    assert L.dliom_points_xray_voxels(fake, i32, 1, None) == bad
    assert L.dliom_points_xray_voxels(fake, i32, -1, C.byref(n)) == bad
    assert L.dliom_points_xray_draw(None, None, None, u32, 4, C.byref(w), C.byref(h)) == bad
    assert L.dliom_points_xray_draw(fake, None, None, u32, 4, None, C.byref(h)) == bad
    assert L.dliom_points_xray_draw(fake, None, None, u32, -1, C.byref(w), C.byref(h)) == bad
    assert L.dliom_points_xray_draw(fake, i32, None, u32, 4, C.byref(w), C.byref(h)) == bad  # half a box
    assert L.dliom_points_xray_stats(None, C.byref(dl.PointsXrayStats())) == bad
    assert L.dliom_points_xray_stats(fake, None) == bad
    assert L.dliom_points_xray_pixel(1, 1, None, u32) == bad and L.dliom_points_xray_pixel(1, 1, f3, None) == bad
    assert L.dliom_points_xray_pixel(2, 1, f3, u32) == bad  # more voxels than the fullest column


def test_pixel_mapping_flips_y_and_z(model, tmp_path):
    """voxel_size 1, identity.  Voxels (x, y, z) = (0, 0, 0), (0, 2, 0), (0, 0, 1): box y 0..2, z 0..1, so width 3, height
    2, and pixel (x, y) = (2 - y, 1 - z): (2, 1), (0, 1), (2, 0).  Every column holds one voxel, so IntoImage's max stays
    at FLT_MIN, log(1) / max = 0, and every pixel is white whatever its colour: the all-ones image."""
    pts = np.array([[0, 0, 0], [0, 2, 0], [0, 0, 1]], dtype=f32)
    r = xc.run_model(model, 1.0, IDENTITY, [insert(pts, (1.0, 0.0, 0.0))], tmp_path)
    a = r.aggregations[0]
    assert r.statuses == [0] and a["image"].shape == (2, 3) and np.all(a["image"] == WHITE)
    assert a["yz"].tolist() == [[0, 0], [0, 1], [2, 0]]  # the std::map's order
    assert a["voxels"].tolist() == [[0, 0, 0], [0, 2, 0], [0, 0, 1]]  # (z, y, x) order
    # a second voxel in column (y, z) = (2, 0) makes it the fullest: saturation 1 there, pure red; the others stay white
    r = xc.run_model(model, 1.0, IDENTITY, [insert(pts, (1.0, 0.0, 0.0)), insert([[5, 2, 0]], (1.0, 0.0, 0.0))], tmp_path)
    image = r.aggregations[0]["image"]
    assert image.tolist() == [[WHITE, WHITE, WHITE], [0xFFFF0000, WHITE, WHITE]]
    assert r.box[0].tolist() == [0, 0, 0] and r.box[1].tolist() == [5, 2, 1]
    # the xy transform looks down: a point at (x, y, z) = (1, 2, 3) lands in camera cell (-3, 2, 1)
    r = xc.run_model(model, 1.0, xc.TRANSFORMS["xy"], [insert([[1, 2, 3]])], tmp_path)
    assert r.aggregations[0]["voxels"].tolist() == [[-3, 2, 1]]
    r = xc.run_model(model, 1.0, xc.TRANSFORMS["xz"], [insert([[1, 2, 3]])], tmp_path)
    assert r.aggregations[0]["voxels"].tolist() == [[2, -1, 3]]
    r = xc.run_model(model, 1.0, xc.TRANSFORMS["yz"], [insert([[1, 2, 3]])], tmp_path)
    assert r.aggregations[0]["voxels"].tolist() == [[-1, -2, 3]]


def test_two_points_in_one_voxel_count_twice_but_occupy_once(model, tmp_path):
    """Both points add their colour and increment `count`; the voxel is one.  Three voxels along x in column (0, 0), one
    of them hit twice: count 4, occupied 3.  The other column holds one voxel: saturation log(1) / log(3) = 0, white.
    Column (0, 0): sums 0.25 * 4 = 1.0 in every channel, mean 0.25, saturation 1: Mix(1, 0.25, 1) = 0.25,
    lround(0.25 * 255 = 63.75) = 64 = 0x40."""
    pts = np.array([[0, 0, 0], [0.2, 0.1, -0.1], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=f32)
    r = xc.run_model(model, 1.0, IDENTITY, [insert(pts, np.full((5, 3), 0.25, dtype=f32))], tmp_path)
    a = r.aggregations[0]
    assert a["yz"].tolist() == [[0, 0], [1, 0]] and a["counts"].tolist() == [4, 1] and a["occupied"].tolist() == [3, 1]
    assert a["sums"].tolist() == [[1.0, 1.0, 1.0], [0.25, 0.25, 0.25]]
    assert a["image"].tolist() == [[WHITE, 0xFF404040]]
    # without colours the sums stay 0 and the column is black
    r = xc.run_model(model, 1.0, IDENTITY, [insert(pts)], tmp_path)
    assert r.aggregations[0]["image"].tolist() == [[WHITE, 0xFF000000]] and not r.aggregations[0]["sums"].any()
    # the sums carry over from one insert to the next, in call order: 2^24 + 1 + 1 = 2^24 in float (each 1 is half an ulp, ties to
    # even), 1 + 1 + 2^24 = 2^24 + 2
    big, one = (16777216.0, 0, 0), (1, 0, 0)
    p = [[0, 0, 0]]
    a = xc.run_model(model, 1.0, IDENTITY, [insert(p, big), insert(p, one), insert(p, one)], tmp_path).aggregations[0]
    b = xc.run_model(model, 1.0, IDENTITY, [insert(p, one), insert(p, one), insert(p, big)], tmp_path).aggregations[0]
    assert a["sums"][0, 0] == f32(16777216.0) and b["sums"][0, 0] == f32(16777218.0) and a["counts"].tolist() == [3]


def test_refusals_leave_the_model_unchanged(model, tmp_path):
    ok = np.array([[8191, 0, 0], [0, -8192, 0], [0, 0, 8191]], dtype=f32)
    ops = [insert(ok), insert([[1, 1, 1], [8192, 0, 0]]), insert([[0, 0, -8193]]), insert([[1, 1, 1], [np.nan, 0, 0]]),
           insert([[np.inf, 0, 0]])]
    r = xc.run_model(model, 1.0, IDENTITY, ops, tmp_path)
    assert r.statuses == [0, -6, -6, -1, -1]
    assert r.aggregations[0]["voxels"].tolist() == [[0, -8192, 0], [8191, 0, 0], [0, 0, 8191]]  # (1, 1, 1) is not there
    assert r.box[0].tolist() == [0, -8192, 0] and r.box[1].tolist() == [8191, 0, 8191]
    # nothing inserted: no image ("Not writing output")
    r = xc.run_model(model, 1.0, IDENTITY, [insert(np.zeros((0, 3), dtype=f32))], tmp_path)
    assert r.box is None and r.aggregations[0]["image"].shape == (0, 0)


def test_two_floors_share_the_box(model, tmp_path):
    ops = [insert([[0, 0, 0], [1, 0, 0]], aggregation=0), insert([[0, 3, 2]], aggregation=1)]
    r = xc.run_model(model, 1.0, IDENTITY, ops, tmp_path, floors=2)
    assert r.box[1].tolist() == [1, 3, 2] and r.aggregations[0]["box"][1].tolist() == [1, 0, 0]
    black = 0xFF000000
    assert r.aggregations[0]["image"].tolist() == [[WHITE] * 4, [WHITE] * 4, [WHITE, WHITE, WHITE, black]]
    assert r.aggregations[1]["image"].tolist() == [[WHITE] * 4, [WHITE] * 4, [WHITE] * 4]  # one voxel a column: white


def test_host_pixel_equals_model_for_every_count_pair(dl, model, tmp_path):
    """dliom_points_xray_pixel over all 1 <= n <= max <= 300 with random means (some outside [0, 1], which the clamp
    takes), against the model's IntoImage expression."""
    n, mx = np.meshgrid(np.arange(1, 301), np.arange(1, 301), indexing="ij")
    keep = n <= mx
    n, mx = n[keep].astype(np.uint32), mx[keep].astype(np.uint32)
    assert len(n) == 300 * 301 // 2
    means = np.random.RandomState(12).uniform(-0.1, 1.1, (len(n), 3)).astype(f32)
    want = xc.run_model(model, 1.0, IDENTITY, [xc.pixels(n, mx, means)], tmp_path).pixels[0]
    got = np.array([dl.points_xray_pixel(a, b, c) for a, b, c in zip(n, mx, means)], dtype=np.uint32)
    assert np.array_equal(got, want)
    assert len(np.unique(want)) > 10000 and np.all(want[mx == 1] == WHITE)
    assert dl.points_xray_pixel(0, 5, (0.0, 0.0, 0.0)) == WHITE


@pytest.mark.parametrize("colors", ["constant", "intensity"])
def test_the_parity_scenes_are_honest(model, tmp_path, colors):
    """What tests/test_gpu_points_xray.py relies on, checked where no GPU is needed: the smallest drive has images with
    empty and occupied pixels, a column of eight or more voxels, and coloured columns whose sums depend on the order."""
    for name in ("yz", "xy", "xz"):
        ops = xc.drive_ops(12, 16, 256, colors)
        r = xc.run_model(model, 0.05, xc.TRANSFORMS[name], ops, tmp_path)
        fraction = xc.honest(r, ops, 0.05, xc.TRANSFORMS[name], colored=True)
        print(name, colors, "order-sensitive share of the columns with >= 8 points: %.3f" % fraction)


def test_prescribed_runs_are_what_they_claim(model, tmp_path):
    """The premises of test_gpu_points_xray.py's prescribed runs: the batch's run lengths are the prescribed list; every run
    of 64 or more is order-sensitive (sequential != reversed, sequential != pairwise; the seed was chosen for this); the
    batch is interleaved (no run is contiguous in batch order); the three variants differ only in the one-point inserts."""
    pts, colors, column = xc.run_length_batch()
    assert xc.run_lengths_of(1.0, IDENTITY, pts) == xc.RUN_LENGTHS and len(pts) == sum(xc.RUN_LENGTHS) <= 65537
    sensitive = xc.order_sensitive_runs(colors, column)
    assert len(sensitive) == sum(k >= 64 for k in xc.RUN_LENGTHS) and all(sensitive), sensitive
    for k, length in enumerate(xc.RUN_LENGTHS):
        where = np.flatnonzero(column == k)
        assert len(where) == length and (length < 3 or where[-1] - where[0] + 1 > length)
    for colors_kind in ("point", "constant", "none"):
        variants = [xc.run_length_ops(last, colors_kind) for last in xc.RUN_LAST]
        for last, ops in zip(xc.RUN_LAST, variants):
            assert len(ops) == 12 and all(len(o[2]) == 1 for o in ops[:10])
            assert ops[-1][2].tobytes() == pts.tobytes() and ops[-2][2].tobytes() == variants[0][-1][2].tobytes()
            cells = xc.camera_cells(1.0, IDENTITY, np.concatenate([o[2] for o in ops[:10]]))
            assert len({tuple(c[1:]) for c in cells}) == 10  # ten columns, claimed one insert at a time
            last_cell = cells[9, 1:]
            main = xc.camera_cells(1.0, IDENTITY, pts)
            assert int(np.sum((main[:, 1] == last_cell[0]) & (main[:, 2] == last_cell[1]))) == last
            r = xc.run_model(model, 1.0, IDENTITY, ops, tmp_path)
            assert r.statuses == [0] * 12 and r.aggregations[0]["counts"].tolist() == [2 * k + 1 for k in xc.RUN_LENGTHS]


@pytest.mark.parametrize("count", xc.COLUMN_COUNTS)
def test_prescribed_column_counts_are_what_they_claim(model, tmp_path, count):
    ops = xc.column_count_ops(count)
    assert max(len(o[2]) for o in ops) <= 65537
    r = xc.run_model(model, 1.0, IDENTITY, ops, tmp_path)
    a = r.aggregations[0]
    assert r.statuses == [0] * len(ops) and len(a["yz"]) == count
    # the last batch brings exactly one new column, three times, with three different colours, between points of column 0
    before = xc.run_model(model, 1.0, IDENTITY, ops[:-1], tmp_path).aggregations[0]
    assert len(before["yz"]) == count - 1
    cells = xc.camera_cells(1.0, IDENTITY, ops[-1][2])[:, 1:]
    new = [i for i, c in enumerate(cells) if not np.any(np.all(before["yz"] == c, axis=1))]
    assert new == [0, 2, 4] and len({ops[-1][3][i].tobytes() for i in new}) == 3
    first = xc.camera_cells(1.0, IDENTITY, ops[0][2])[0, 1:]
    assert np.array_equal(cells[1], first) and np.array_equal(cells[3], first)
