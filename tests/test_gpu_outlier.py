"""Moving-object removal on the device (dliom_outlier_remover_*, dliom_cloud_min_max_range_filter) against the CPU model
of the reference's two points processors (tests/cpp/outlier_model.cc).  Every comparison is exact equality: the whole
voxel table (keys, hits, rays), kept_index and the kept cloud's bytes per batch.  The multi-scan scenes assert the
conditions under which they compare something (tests/outlier_common.py honest(): 1 % .. 60 % of the points removed, a
surviving voxel with rays > 0, no refusal)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlier_common as oc  # noqa: E402
from outlier_common import FILTER, MARK, RANGE, RAYS, f32, op  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = oc.ROOT


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
    return oc.build_model(tmp_path_factory.mktemp("outlier_model"))


def assert_table_equal(remover, table):
    xyz, hits, rays = remover.voxels()
    assert np.array_equal(xyz, table[0]) and np.array_equal(hits, table[1]) and np.array_equal(rays, table[2])


def run_device(dl, ctx, voxel_size, batches, table_after_marks=None):
    """The three passes over `batches` -> (remover, [(kept points, kept_index)] per batch)."""
    r = dl.OutlierRemover(ctx, voxel_size)
    clouds = [dl.PointCloud(ctx, p) for _, p in batches]
    for c in clouds:
        r.mark_hits(c)
    if table_after_marks is not None:
        assert_table_equal(r, table_after_marks)
    for (o, _), c in zip(batches, clouds):
        r.count_rays(o, c)
    out = []
    for c in clouds:
        kept, index = r.filter(c)
        out.append((kept.download(), index))
        kept.close()
    for c in clouds:
        c.close()
    return r, out


def compare(dl, ctx, model, voxel_size, batches, tmp_path, need_honest=True):
    results, table = oc.run_model(model, voxel_size, oc.three_pass_ops(batches), tmp_path)
    assert all((s if isinstance(s, int) else s[0]) == 0 for s in results)
    removed = oc.honest(batches, results, table) if need_honest else None
    r, out = run_device(dl, ctx, voxel_size, batches)
    assert_table_equal(r, table)
    for (_, pts), (kept_pts, index), (_, want) in zip(batches, out, results[2 * len(batches):]):
        assert np.array_equal(index, want)
        assert kept_pts.tobytes() == pts[want].tobytes()
    stats = r.stats()
    assert stats["voxels"] == len(table[1]) and stats["phase"] == 3
    r.close()
    return removed, stats


@pytest.mark.parametrize("beams,azimuths,voxel_size", [(16, 256, 0.05), (16, 256, 0.15), (16, 256, 0.07), (32, 512, 0.15),
                                                       (64, 1024, 0.15)])
def test_drive_with_moving_obstacles_equals_model(dl, ctx, model, tmp_path, beams, azimuths, voxel_size):
    batches = oc.drive(12, beams, azimuths)
    removed, stats = compare(dl, ctx, model, voxel_size, batches, tmp_path)
    print("removed %.4f of %d points; %s" % (removed, sum(len(p) for _, p in batches), stats))
    assert stats["samples_walked"] > 0 and stats["probes"] > 0
    assert ctx.memory_stats()["outlier_table_bytes"] == 0  # the remover is closed: its table left the ledger


def test_memory_stats_count_the_table(dl, ctx):
    before = ctx.memory_stats()["outlier_table_bytes"]
    r = dl.OutlierRemover(ctx, 0.1)
    c = dl.PointCloud(ctx, np.random.RandomState(0).uniform(-20, 20, (20000, 3)).astype(f32))
    r.mark_hits(c)
    s = r.stats()
    assert ctx.memory_stats()["outlier_table_bytes"] == before + s["table_bytes"] and s["table_bytes"] >= s["leaves"] * 4096
    r.close()
    c.close()
    assert ctx.memory_stats()["outlier_table_bytes"] == before


def test_growth_empty_single_and_degenerate_batches(dl, ctx, model, tmp_path):
    rng = np.random.RandomState(3)
    big = oc.drive(2, 32, 512)
    o = np.array([0.3, -0.2, 0.1], dtype=f32)
    empty = np.zeros((0, 3), dtype=f32)
    one_voxel = (np.array([2.0, 1.0, 0.5]) + rng.uniform(-0.02, 0.02, (500, 3))).astype(f32)
    batches = [(o, big[0][1][:3]),                 # tiny first batch, then a large one: the table and the pool grow
               big[1],
               (o, empty),                          # an empty batch in every pass
               (o, np.array([[1.0, 2.0, 3.0]], dtype=f32)),  # one point
               (o, one_voxel),                      # all points in one voxel
               (one_voxel[0], one_voxel),           # the origin inside a hit voxel
               (o, np.tile(o, (7, 1))),             # points at the origin: length 0, no sample
               big[0]]
    results, table = oc.run_model(model, 0.05, oc.three_pass_ops(batches), tmp_path)
    marks = oc.run_model(model, 0.05, [op(MARK, p, o_) for o_, p in batches], tmp_path)[1]
    r, out = run_device(dl, ctx, 0.05, batches, table_after_marks=marks)
    assert_table_equal(r, table)
    assert r.stats()["growths"] >= 2
    for (_, pts), (kept_pts, index), (status, want) in zip(batches, out, results[2 * len(batches):]):
        assert status == 0 and np.array_equal(index, want) and kept_pts.tobytes() == pts[want].tobytes()
    r.close()


def test_extent_phase_order_non_finite_and_capacity(dl, ctx, model, tmp_path):
    L = dl.load_library()
    vs = 0.05
    res = f32(vs)
    inside = np.array([[8191 * float(res), 0, 0], [-8192 * float(res), 1, 2], [1, 2, 3], [1.01, 2, 3]], dtype=f32)
    outside = np.array([[1, 2, 3], [0, 8192.6 * float(res), 0]], dtype=f32)
    results, table = oc.run_model(model, vs, [op(MARK, inside), op(MARK, outside), op(MARK, [[np.nan, 0, 0]])], tmp_path)
    assert results == [0, dl.ERR_GRID_EXTENT, dl.ERR_INVALID_ARGUMENT] and 8191 in table[0][:, 0] and -8192 in table[0][:, 0]
    r = dl.OutlierRemover(ctx, vs)
    c_in, c_out = dl.PointCloud(ctx, inside), dl.PointCloud(ctx, outside)
    c_nan, c_inf = dl.PointCloud(ctx, [[np.nan, 0, 0]]), dl.PointCloud(ctx, [[1, 2, 3], [0, np.inf, 0]])
    r.mark_hits(c_in)
    assert_table_equal(r, table)
    for cloud, status in ((c_out, dl.ERR_GRID_EXTENT), (c_nan, dl.ERR_INVALID_ARGUMENT), (c_inf, dl.ERR_INVALID_ARGUMENT)):
        with pytest.raises(dl.DliomError) as e:
            r.mark_hits(cloud)
        assert e.value.status == status
        assert_table_equal(r, table)  # unchanged, the in-range hit of the refused batch included
    o = np.zeros(3, dtype=f32)
    for cloud, origin in ((c_nan, o), (c_inf, o), (c_in, np.array([0, np.nan, 0], dtype=f32))):
        with pytest.raises(dl.DliomError) as e:
            r.count_rays(origin, cloud)
        assert e.value.status == dl.ERR_INVALID_ARGUMENT
    assert r.stats()["phase"] == 1  # a refused call does not advance the phase
    # a pass-2 point outside the extent is no error: its samples outside read no hit
    r.count_rays(o, c_out)
    want = oc.run_model(model, vs, [op(MARK, inside), op(RAYS, outside), op(FILTER, outside), op(FILTER, inside)], tmp_path)
    assert_table_equal(r, want[1])
    with pytest.raises(dl.DliomError) as e:
        r.mark_hits(c_in)  # phase 1 is over
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    with pytest.raises(dl.DliomError) as e:
        r.filter(c_nan)
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    # capacity: the count is filled in, no cloud
    h, kept = C.c_void_p(), C.c_int64(-1)
    index = np.zeros(1, dtype=np.int32)
    s = L.dliom_outlier_remover_filter(r.h, c_in.h, C.byref(h), index.ctypes.data_as(C.POINTER(C.c_int32)), 1, C.byref(kept))
    assert s == dl.ERR_CAPACITY and kept.value == len(want[0][3][1]) > 1 and not h.value
    # a pass-3 point outside the extent is removed; without kept_index the capacity does not matter
    s = L.dliom_outlier_remover_filter(r.h, c_out.h, C.byref(h), None, 0, C.byref(kept))
    assert s == 0 and kept.value == len(want[0][2][1]) == 1
    L.dliom_cloud_destroy(h)
    kept_cloud, idx = r.filter(c_in)
    assert np.array_equal(idx, want[0][3][1])
    with pytest.raises(dl.DliomError) as e:
        r.count_rays(o, c_in)  # phase 2 is over
    assert e.value.status == dl.ERR_INVALID_ARGUMENT
    assert_table_equal(r, want[1])
    for c in (c_in, c_out, c_nan, c_inf, kept_cloud):
        c.close()
    r.close()


def test_min_max_range_filter_equals_model(dl, ctx, model, tmp_path):
    rng = np.random.RandomState(11)
    o = np.array([0.5, -1.5, 0.25], dtype=f32)
    pts = (o + rng.normal(size=(20000, 3)) * rng.uniform(0.1, 40.0, (20000, 1))).astype(f32)
    d = pts - o
    ranges = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    assert ranges.dtype == f32
    lo, hi = float(np.sort(ranges)[2000]), float(np.sort(ranges)[15000])  # two points' float ranges equal the bounds exactly
    cloud = dl.PointCloud(ctx, pts)
    empty = dl.PointCloud(ctx, np.zeros((0, 3), dtype=f32))
    for a, b in ((lo, hi), (1.0, 60.0), (np.nextafter(lo, 1e9), np.nextafter(hi, 0.0)), (0.0, np.inf), (5.0, 1.0)):
        (status, want), = oc.run_model(model, 0.1, [op(RANGE, pts, o, a, b)], tmp_path)[0]
        kept, index = cloud.min_max_range_filter(o, a, b)
        assert status == 0 and np.array_equal(index, want) and kept.download().tobytes() == pts[want].tobytes()
        kept.close()
    (_, want), = oc.run_model(model, 0.1, [op(RANGE, pts, o, lo, hi)], tmp_path)[0]
    assert np.argsort(ranges)[2000] in want and np.argsort(ranges)[15000] in want  # range == bound is kept
    assert 0 < len(want) < len(pts)
    kept, index = empty.min_max_range_filter(o, 1.0, 2.0)
    assert len(kept) == 0 and len(index) == 0
    for c in (kept, cloud, empty):
        c.close()


def test_export_chain_on_device_clouds(dl, ctx, model, orc, tmp_path):
    """min_max_range_filter -> remove moving objects -> voxel filter, the points never leaving the device in between."""
    batches = oc.drive(12, 16, 256)
    lo, hi, vs, vf = 1.0, 14.0, 0.1, 0.2
    ranged = []
    for o, p in batches:
        (_, keep), = oc.run_model(model, vs, [op(RANGE, p, o, lo, hi)], tmp_path)[0]
        ranged.append((o, p[keep]))
    results, table = oc.run_model(model, vs, oc.three_pass_ops(ranged), tmp_path)
    oc.honest(ranged, results, table)
    r = dl.OutlierRemover(ctx, vs)
    clouds = []
    for o, p in batches:
        raw = dl.PointCloud(ctx, p)
        clouds.append(raw.min_max_range_filter(o, lo, hi)[0])
        raw.close()
    for c in clouds:
        r.mark_hits(c)
    for (o, _), c in zip(batches, clouds):
        r.count_rays(o, c)
    assert_table_equal(r, table)
    for (o, p), c, (_, want) in zip(ranged, clouds, results[2 * len(ranged):]):
        kept, _ = r.filter(c)
        out = kept.voxel_filter(vf)
        survivors = p[want]
        assert out.download().tobytes() == survivors[orc.voxel_filter(vf, survivors)].tobytes()
        for x in (kept, out, c):
            x.close()
    r.close()


def test_adapter_classes_equal_model(dl, model, tmp_path):
    """io::OutlierRemovingPointsProcessor / MinMaxRangeFiteringPointsProcessor of dliom_cartographer.h through their three
    Flush() phases (tests/cpp/outlier_adapter.cc), intensities and colors filtered with the points."""
    exe = str(tmp_path / "outlier_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "outlier_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    batches = oc.drive(12, 16, 256)
    lo, hi, vs = 1.0, 14.0, 0.1
    ops = []
    ranged = []
    for o, p in batches:
        (_, keep), = oc.run_model(model, vs, [op(RANGE, p, o, lo, hi)], tmp_path)[0]
        ranged.append((o, p[keep], keep))
    results, table = oc.run_model(model, vs, oc.three_pass_ops([(o, p) for o, p, _ in ranged]), tmp_path)
    oc.honest([(o, p) for o, p, _ in ranged], results, table)
    src, dst = str(tmp_path / "batches.bin"), str(tmp_path / "adapter_out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(batches)], dtype=np.int32).tobytes())
        for o, p in batches:
            f.write(o.tobytes() + np.array([len(p)], dtype=np.int32).tobytes() + p.tobytes())
    out = subprocess.run([exe, src, dst, repr(vs), repr(lo), repr(hi)], timeout=300)
    assert out.returncode == 0
    data = open(dst, "rb").read()
    at = 0
    for (o, p, keep), (_, want) in zip(ranged, results[2 * len(ranged):]):
        n = int(np.frombuffer(data, dtype=np.int32, count=1, offset=at)[0])
        at += 4
        pts = np.frombuffer(data, dtype=f32, count=3 * n, offset=at).reshape(n, 3)
        at += 12 * n
        intensities = np.frombuffer(data, dtype=f32, count=n, offset=at)
        at += 4 * n
        colors = np.frombuffer(data, dtype=f32, count=3 * n, offset=at).reshape(n, 3)
        at += 12 * n
        source = keep[want]  # indices into the batch as it was streamed
        assert pts.tobytes() == p[want].tobytes()
        assert np.array_equal(intensities, source.astype(f32))  # the adapter test streams intensity = index
        assert np.array_equal(colors, np.stack([source, 2 * source, 3 * source], axis=1).astype(f32))
    assert at == len(data)


def test_randomised_slice(dl, ctx, model, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_outlier
    for seed in (1, 2, 3, 4, 5, 6):
        fuzz_outlier.run_case(dl, ctx, model, seed, str(tmp_path))
