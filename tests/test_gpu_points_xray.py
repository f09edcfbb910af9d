"""X-ray images of point clouds on the device (dliom_points_xray_*) against the CPU model of io::XRayPointsProcessor
(tests/cpp/points_xray_model.cc).  Every comparison is exact equality: the whole column table (the float sums as bits),
the voxel list, the bounding box and the image bytes.  The drives assert the conditions under which they compare
something (tests/points_xray_common.py honest()): images with empty and occupied pixels, a column of eight or more voxels,
and -- in the coloured cases -- columns whose sequential sums differ from the same sums in another order."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import points_xray_common as xc  # noqa: E402
from points_xray_common import IDENTITY, TRANSFORMS, WHITE, f32, insert  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = xc.ROOT


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
    return xc.build_model(tmp_path_factory.mktemp("points_xray_model"))


@pytest.mark.parametrize("colors", ["none", "constant", "intensity"])
@pytest.mark.parametrize("beams,azimuths,voxel_size,view", [(16, 256, 0.05, "yz"), (16, 256, 0.07, "xy"), (16, 256, 0.15, "xz"),
                                                            (32, 512, 0.05, "xy"), (32, 512, 0.07, "xz"), (32, 512, 0.15, "yz"),
                                                            (64, 1024, 0.05, "xz"), (64, 1024, 0.07, "yz"), (64, 1024, 0.15, "xy"),
                                                            (64, 1024, 0.05, "yz"), (64, 1024, 0.05, "xy")])
def test_drive_equals_model(dl, ctx, model, tmp_path, beams, azimuths, voxel_size, view, colors):
    """The 12-scan drive: every size with every voxel size, every view three times (a Latin square, not the full cross),
    and the largest drive at the stock 5 cm in all three views; each without colours, with one colour a batch and with per-point colours from random intensities.  The 32 x 512
    cases hand their colours over in page-locked memory."""
    ops = xc.drive_ops(12, beams, azimuths, colors)
    _, stats, fraction = xc.compare(dl, ctx, model, voxel_size, TRANSFORMS[view], ops, tmp_path, colored=colors != "none",
                                    registered=beams == 32)
    print("%s %s: %s; order-sensitive share %s" % (view, colors, stats[0], fraction))
    assert stats[0]["points"] == sum(len(o[2]) for o in ops) and stats[0]["probes"] >= 2 * stats[0]["points"]
    assert ctx.memory_stats()["points_xray_bytes"] == 0  # closed: its tables left the ledger


def test_growth_empty_single_and_one_voxel_batches(dl, ctx, model, tmp_path):
    rng = np.random.RandomState(3)
    big = xc.drive_ops(2, 32, 512, "intensity")
    one_voxel = (np.array([2.0, 1.0, 0.5]) + rng.uniform(-0.02, 0.02, (500, 3))).astype(f32)
    ops = [insert(big[0][2][:3], big[0][3][:3]),  # a tiny first batch, then large ones: tables and pools grow
           big[1],
           insert(np.zeros((0, 3), dtype=f32)),   # an empty batch
           insert([[1.0, 2.0, 3.0]], (0.5, 0.25, 0.125)),  # one point, one colour
           insert([[1.0, 2.0, 3.0]], [[0.1, 0.2, 0.3]]),
           insert(one_voxel, rng.uniform(0, 1, (500, 3))),  # all points in one voxel: one run of 500
           insert(one_voxel),
           insert(one_voxel, (0.3, 0.6, 0.9)),
           big[0]]
    result, stats, _ = xc.compare(dl, ctx, model, 0.05, IDENTITY, ops, tmp_path, need_honest=False)
    assert stats[0]["growths"] >= 2 and stats[0]["longest_segment"] >= 500 and stats[0]["inserts"] == len(ops) - 1
    column = result.aggregations[0]
    assert column["counts"].max() >= 1500


def test_one_column_of_65536_points(dl, ctx, model, tmp_path):
    """Every point of the batch in one column (y, z), spread over x: one sequential sum of 65 536 random colours, three
    times over (per point, constant, per point again on top of the stored sums)."""
    rng = np.random.RandomState(8)
    n = 65536
    pts = np.stack([rng.uniform(-20.0, 20.0, n), np.full(n, 0.26), np.full(n, -1.01)], axis=1).astype(f32)
    colors = rng.uniform(0.0, 1.0, (n, 3)).astype(f32)
    ops = [insert(pts, colors), insert(pts, (0.1, 0.7, 0.3)), insert(pts, colors[::-1])]
    result, stats, _ = xc.compare(dl, ctx, model, 0.05, IDENTITY, ops, tmp_path, need_honest=False)
    a = result.aggregations[0]
    assert len(a["yz"]) == 1 and a["counts"][0] == 3 * n and a["occupied"][0] > 500 and stats[0]["longest_segment"] == n
    # the sequential sum differs from the reversed one, so an unordered sum could not have matched
    rev = xc.run_model(model, 0.05, IDENTITY, [insert(pts[::-1], colors[::-1])], tmp_path).aggregations[0]
    first = xc.run_model(model, 0.05, IDENTITY, ops[:1], tmp_path).aggregations[0]
    assert rev["sums"].tobytes() != first["sums"].tobytes()


def test_two_floors_in_the_shared_box(dl, ctx, model, tmp_path):
    drive = xc.drive_ops(12, 16, 256, "intensity")
    ops = []
    for s, o in enumerate(drive):
        pts = o[2] + (np.array([0.0, 0.0, 0.0 if s < 6 else 3.0], dtype=f32))
        ops.append(insert(pts, o[3], aggregation=0 if s < 6 else 1))
    result, _, _ = xc.compare(dl, ctx, model, 0.07, TRANSFORMS["yz"], ops, tmp_path, floors=2, need_honest=False)
    a, b = result.aggregations
    assert a["image"].shape == b["image"].shape and a["image"].tobytes() != b["image"].tobytes()
    assert not np.array_equal(a["box"][1], b["box"][1])  # neither floor's own box is the shared one
    xc.honest(result)


def test_draw_before_any_insert_and_box_arguments(dl, ctx):
    x = dl.PointsXray(ctx, 0.05)
    assert x.bounding_box() is None and x.draw().shape == (0, 0)
    assert len(x.voxels()) == 0 and len(x.columns()[0]) == 0
    # an empty aggregator in a box someone else filled: all white
    image = x.draw((np.array([0, -2, -1]), np.array([5, 3, 1])))
    assert image.shape == (3, 6) and np.all(image == WHITE)
    cloud = dl.PointCloud(ctx, np.array([[0, 0, 0], [0.05, 0, 0], [0, 0.5, 0.25]], dtype=f32))
    x.insert(cloud, (0.0, 0.0, 1.0))
    lo, hi = x.bounding_box()
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [1, 10, 5]
    image = x.draw()
    assert image.shape == (6, 11) and image[5, 10] == 0xFF0000FF and image[0, 0] == WHITE and (image != WHITE).sum() == 1
    with pytest.raises(dl.DliomError) as e:
        x.draw((np.array([0, 0, 0]), np.array([1, 9, 5])))  # does not hold every voxel
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    L = dl.load_library()
    import ctypes as C
    w, h = C.c_int32(), C.c_int32()
    small = np.zeros(4, dtype=np.uint32)
    s = L.dliom_points_xray_draw(x.h, None, None, small.ctypes.data_as(C.POINTER(C.c_uint32)), 4, C.byref(w), C.byref(h))
    assert s == dl.ERR_CAPACITY and (w.value, h.value) == (11, 6)
    with pytest.raises(dl.DliomError) as e:
        x.insert(cloud, np.zeros((2, 3), dtype=f32))  # neither 0, 1 nor 3 colours
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    cloud.close()
    x.close()


def test_refusals_leave_tables_and_box_unchanged(dl, ctx, model, tmp_path):
    vs = 0.05
    res = float(f32(vs))
    inside = np.array([[8191 * res, 0, 0], [-8192 * res, 1, 2], [1, 2, 3], [1.01, 2, 3]], dtype=f32)
    bad = [np.array([[1, 2, 3], [0, 8192.6 * res, 0]], dtype=f32), np.array([[5, 5, 5], [np.nan, 0, 0]], dtype=f32),
           np.array([[5, 5, 5], [0, np.inf, 0]], dtype=f32), np.array([[0, 0, -8193 * res]], dtype=f32)]
    colors = np.random.RandomState(1).uniform(0, 1, (4, 3)).astype(f32)
    ops = [insert(inside, colors)] + [insert(b, c) for b in bad for c in (None, (0.5, 0.5, 0.5))] + [insert(bad[0], colors[:2])]
    result = xc.run_model(model, vs, IDENTITY, ops, tmp_path)
    assert result.statuses == [0] + [dl.ERR_GRID_EXTENT] * 2 + [dl.ERR_INVALID_ARGUMENT] * 4 + [dl.ERR_GRID_EXTENT] * 3
    assert 8191 in result.aggregations[0]["voxels"][:, 0] and -8192 in result.aggregations[0]["voxels"][:, 0]
    xs, statuses = xc.run_device(dl, ctx, vs, IDENTITY, ops)
    xc.assert_equal(xs, statuses, result)  # the in-range points of the refused batches are not there either
    stats = xs[0].stats()
    assert stats["inserts"] == 1 and stats["points"] == 4
    xs[0].close()


def test_memory_returns_to_the_ledger(dl, ctx):
    before = ctx.memory_stats()["points_xray_bytes"]
    x = dl.PointsXray(ctx, 0.1)
    created = ctx.memory_stats()["points_xray_bytes"]
    assert created > before
    pts = np.random.RandomState(0).uniform(-20, 20, (20000, 3)).astype(f32)
    c = dl.PointCloud(ctx, pts)
    x.insert(c, np.random.RandomState(1).uniform(0, 1, (20000, 3)).astype(f32))
    s = x.stats()
    assert ctx.memory_stats()["points_xray_bytes"] == before + s["table_bytes"] > created
    assert s["table_bytes"] >= s["leaves"] * 64 + s["columns"] * 24
    x.draw()
    assert ctx.memory_stats()["points_xray_bytes"] == before + x.stats()["table_bytes"]
    x.close()
    c.close()
    assert ctx.memory_stats()["points_xray_bytes"] == before


def test_adapter_pipeline_equals_model(dl, model, tmp_path):
    """io::XRayPointsProcessor, ColoringPointsProcessor and IntensityToColorPointsProcessor of dliom_cartographer.h
    (tests/cpp/points_xray_adapter.cc): range filter -> X-ray x3 -> intensity colours -> X-ray x3 -> one colour -> X-ray,
    the seven images equal to the model's, the batch uploaded once."""
    exe = str(tmp_path / "points_xray_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "points_xray_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import outlier_common as oc
    batches = oc.drive(12, 32, 512)  # (the 16 x 256 drive leaves at most 5 voxels a column in the xz view: not honest)
    lo, hi, vs = 1.0, 14.0, 0.05
    rng = np.random.RandomState(21)
    omodel = oc.build_model(tmp_path)
    kept, intensities = [], []
    for o, p in batches:
        (_, keep), = oc.run_model(omodel, vs, [oc.op(oc.RANGE, p, o, lo, hi)], tmp_path)[0]
        inten = rng.uniform(-20.0, 300.0, len(p)).astype(f32)
        intensities.append(inten)
        kept.append((p[keep], inten[keep]))
    src, dst = str(tmp_path / "batches.bin"), str(tmp_path / "adapter_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(batches)], dtype=np.int32).tobytes())
        for (o, p), inten in zip(batches, intensities):
            f.write(o.tobytes() + np.array([len(p)], dtype=np.int32).tobytes() + p.tobytes() + inten.tobytes())
    out = subprocess.run([exe, src, dst, repr(vs), repr(lo), repr(hi)], timeout=300)
    assert out.returncode == 0
    data = open(dst, "rb").read()
    at = 0
    constant = np.array([255, 100, 0], dtype=f32) / f32(255.0)  # ColoringPointsProcessor: c / 255.f in float
    stages = ([(v, None) for v in ("yz", "xy", "xz")] + [(v, "intensity") for v in ("yz", "xy", "xz")] + [("xy", "constant")])
    for view, colors in stages:
        if colors is None:
            ops = [insert(p) for p, _ in kept]
        elif colors == "intensity":
            ops = [insert(p, xc.intensity_colors(i, 0.0, 255.0)) for p, i in kept]
        else:
            ops = [insert(p, constant) for p, _ in kept]
        want = xc.run_model(model, vs, TRANSFORMS[view], ops, tmp_path)
        xc.honest(want, ops, vs, TRANSFORMS[view], colored=colors == "intensity")
        name_len = int(np.frombuffer(data, dtype=np.int32, count=1, offset=at)[0])
        name = data[at + 4:at + 4 + name_len].decode()
        at += 4 + name_len
        w, h = np.frombuffer(data, dtype=np.int32, count=2, offset=at)
        image = np.frombuffer(data, dtype=np.uint32, count=int(w) * int(h), offset=at + 8).reshape(h, w)
        at += 8 + 4 * int(w) * int(h)
        assert name == "xray_%s_%s.png" % (view, colors or "gray")
        assert image.shape == want.aggregations[0]["image"].shape and image.tobytes() == want.aggregations[0]["image"].tobytes(), name
    uploads, batches_seen = np.frombuffer(data, dtype=np.int64, count=2, offset=at)
    at += 16
    assert at == len(data)
    # one upload per batch, by the range filter; the seven X-ray stages behind it upload no points
    assert batches_seen == len(batches) and uploads == len(batches)


def test_randomised_slice(dl, ctx, model, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_points_xray
    for seed in (1, 2, 3, 4, 5, 6, 7, 8):
        fuzz_points_xray.run_case(dl, ctx, model, seed, str(tmp_path))


@pytest.mark.parametrize("colors", ["point", "constant", "none"])
@pytest.mark.parametrize("last", xc.RUN_LAST)
def test_prescribed_run_lengths(dl, ctx, model, tmp_path, last, colors):
    """Runs of exactly 1, 2, 63, 64, 65, 127, 128, 129, 192 and 193 points in one batch, interleaved in batch order, the run
    of `last` points at the very end of the sorted arrays (j + 64 == n for 64; a trip with count == 0 for 128); the batch a
    second time on top of the stored sums.  tests/test_points_xray_host.py asserts the run lengths and that every run of
    64 or more sums to different bits in another order."""
    ops = xc.run_length_ops(last, colors)
    assert xc.run_lengths_of(1.0, IDENTITY, ops[-1][2]) == xc.RUN_LENGTHS
    result, stats, _ = xc.compare(dl, ctx, model, 1.0, IDENTITY, ops, tmp_path, need_honest=False)
    a = result.aggregations[0]
    assert a["counts"].tolist() == [2 * k + 1 for k in xc.RUN_LENGTHS] and stats[0]["columns"] == len(xc.RUN_LENGTHS)
    assert stats[0]["longest_segment"] == max(xc.RUN_LENGTHS)


@pytest.mark.parametrize("colors", ["point", "constant", "none"])
@pytest.mark.parametrize("count", xc.COLUMN_COUNTS)
def test_prescribed_column_counts(dl, ctx, model, tmp_path, count, colors):
    """Exactly 2^k - 1, 2^k and 2^k + 1 columns (k = 8, 16): the radix sort's key width steps there.  The highest slot holds
    a run of 3 interleaved with points of slot 0: a sort that drops the top key bit breaks the run up."""
    ops = xc.column_count_ops(count, colors)
    result, stats, _ = xc.compare(dl, ctx, model, 1.0, IDENTITY, ops, tmp_path, need_honest=False)
    a = result.aggregations[0]
    assert stats[0]["columns"] == count == len(a["yz"])
    last = count - 1
    at = np.flatnonzero((a["yz"][:, 0] == last % 256 - 128) & (a["yz"][:, 1] == last // 256 - 128))
    assert len(at) == 1 and a["counts"][at[0]] == 3
