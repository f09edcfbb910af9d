"""The 2D probability grid on the device (dliom_probability_grid_*, dliom_inserter2d_*) against the CPU oracle
(oracle.ProbabilityGrid, a restatement of mapping/2d + mapping/internal/2d/ray_casting.cc).  Every comparison of cells,
limits, boxes and pixels is exact equality (np.array_equal); the only tolerances are the reference's own, on the
probabilities of its known-answer test.  The drives assert the conditions under which they compare something."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import outlier_common as oc  # noqa: E402
import probability_grid_common as pc  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
HIT, MISS = 0.55, 0.49  # assets_writer_ros_map.lua


@pytest.fixture(scope="module")
def dl():
    import dliom
    return dliom


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


class Pair:
    """A device grid and an oracle grid that receive the same inserts."""

    def __init__(self, dl, orc, ctx, resolution, limits=None, hit=HIT, miss=MISS, free=True):
        self.grid = dl.ProbabilityGrid2D(ctx, resolution, limits)
        self.ins = dl.Inserter2D(ctx, hit, miss, free)
        self.ogrid = pc.new_oracle_grid(orc, resolution, limits)
        self.hit, self.miss, self.free = hit, miss, free

    def insert(self, origin, points):
        pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
        self.ins.insert(self.grid, origin, pts)
        self.ogrid.insert(origin, pts, self.hit, self.miss, self.free)
        return pc.assert_equal(self.grid, self.ogrid)

    def close(self):
        self.ins.close()
        self.grid.close()


def test_reference_known_answers(dl, orc, ctx):
    """mapping/2d/range_data_inserter_2d_test.cc:32-131, data only: the 5 x 5 fixture, one scan from (-0.5, 0.5)."""
    limits = (1.0, 5.0, 5, 5)  # MapLimits(1., Vector2d(1., 5.), CellLimits(5, 5))
    pair = Pair(dl, orc, ctx, 1.0, limits, hit=0.7, miss=0.4)
    returns = np.array([[-3.5, 0.5, 0], [-2.5, 1.5, 0], [-1.5, 2.5, 0], [-0.5, 3.5, 0]], dtype=f32)
    origin = np.array([-0.5, 0.5, 0], dtype=f32)
    cells = pair.insert(origin, returns)
    assert pair.grid.limits() == (1.0, (1.0, 5.0), (5, 5))  # :71-75 the limits are unchanged
    # :76-84 expected_states[column][row] is the cell (x = row, y = column): the rows below are rows of the cell array.
    # The cells hold correspondence costs: 8193 is the value of 1 - 0.7 (HIT), 20480 of 1 - 0.4 (MISS).
    U, H, M = 0, 8193, 20480
    want = np.array([[U, U, U, U, U], [U, H, M, M, M], [U, U, H, M, M], [U, U, U, H, M], [U, U, U, U, H]], dtype=np.uint16)
    assert np.array_equal(cells, want)
    xy = np.array([(x, y) for y in range(5) for x in range(5)], dtype=np.int32)
    p, known = pair.grid.get_probabilities(xy)
    for (x, y), pi, ki in zip(xy, p, known):
        state = want[y, x]
        assert ki == (state != U)
        assert pi == f32(pair.ogrid.get_probability(int(x), int(y)))
        if state == H:
            assert abs(pi - 0.7) <= 1e-4
        if state == M:
            assert abs(pi - 0.4) <= 1e-4
    p_out, k_out = pair.grid.get_probabilities([[-1, 0], [5, 5], [0, 7]])
    assert np.all(p_out == pc.K_MIN) and not k_out.any()
    cloud = dl.PointCloud(ctx, returns)
    for _ in range(1000):  # :113-131 the probabilities saturate
        pair.ins.insert(pair.grid, origin, cloud)
        pair.ogrid.insert(origin, returns, 0.7, 0.4)
    cloud.close()
    pc.assert_equal(pair.grid, pair.ogrid)
    p, _ = pair.grid.get_probabilities(xy)
    for (x, y), pi in zip(xy, p):
        state = want[y, x]
        if state == H:
            assert abs(pi - 0.9) <= 1e-3
        if state == M:
            assert abs(pi - 0.1) <= 1e-3
    pair.close()


def run_drive(dl, orc, ctx, batches, resolution=0.05):
    """-> what the honesty conditions need: sides of the grid per batch, final cells, cells changed after being set."""
    pair = Pair(dl, orc, ctx, resolution)
    sides, previous, rewritten = [100], None, 0
    for origin, pts in batches:
        cloud = dl.PointCloud(ctx, pts)
        kept, index = cloud.min_max_range_filter(origin, 1.0, 60.0)
        kept_pts = pts[index]
        pair.ins.insert(pair.grid, origin, kept)
        pair.ogrid.insert(origin, kept_pts, HIT, MISS, True)
        cells = pc.assert_equal(pair.grid, pair.ogrid)
        if previous is not None and previous.shape == cells.shape:
            rewritten += int(np.count_nonzero((previous != 0) & (previous != cells)))
        previous = cells
        sides.append(cells.shape[0])
        kept.close()
        cloud.close()
    stats = pair.grid.stats()
    pair.close()
    return sides, previous, rewritten, stats


@pytest.mark.parametrize("scans,beams,azimuths", [(4, 64, 1024), (2, 128, 2048)])
def test_drive_equals_oracle_after_every_batch(dl, orc, ctx, scans, beams, azimuths):
    batches = oc.drive(scans, beams, azimuths)
    sides, cells, rewritten, stats = run_drive(dl, orc, ctx, batches)
    print("grid sides %s, %d known cells, %d rewritten, %s" % (sides, np.count_nonzero(cells), rewritten, stats))
    assert stats["growths"] >= 2 and sides[-1] >= 400, "the grid did not grow twice"
    # correspondence cost below one half (value < 16384): more hits than misses; above: free space
    assert np.any((cells > 0) & (cells < 16384)) and np.any(cells > 16384), "hit-valued and miss-valued cells must both exist"
    assert rewritten > 0, "no cell changed in a later batch after being set in an earlier one"
    assert stats["cells_visited"] > 0 and stats["error_word"] == 0
    if (scans, beams, azimuths) == (4, 64, 1024):
        assert sides[-1] == 800 and np.count_nonzero(cells) == 361442  # what the oracle alone gives for this drive


def edge_batches(resolution):
    r = resolution
    rng = np.random.RandomState(2)
    corners = (np.round(rng.uniform(-40, 40, (300, 3))) * (r / 2)).astype(f32)  # coordinates on multiples of resolution / 2
    return [
        ("empty", (0.3, -0.2, 0.0), np.zeros((0, 3))),
        ("one point", (0.3, -0.2, 0.0), [[1.7, 2.2, 0.4]]),
        ("origin and point in one pixel", (0.51 * r, 0.52 * r, 0.0), [[0.53 * r, 0.57 * r, 0.0]]),
        ("vertical in full pixels, both ways", (0.26 * r, 0.3 * r, 0.0), [[0.31 * r, 17.2 * r, 0.0], [0.7 * r, -23.4 * r, 1.0]]),
        ("dy = 0", (0.3 * r, 0.4 * r, 0.0), [[25.3 * r, 0.4 * r, 0.0], [-31.6 * r, 0.4 * r, 0.0]]),
        ("rays that swap", (5.2 * r, 1.1 * r, 0.0), [[-20.5 * r, 9.3 * r, 0.0], [-3.2 * r, -14.8 * r, 0.0], [5.2 * r, -7.7 * r, 0.0]]),
        ("exact pixel corners", (0.0, 0.0, 0.0), corners),
        ("exact pixel corners from a corner", (2 * r, -3 * r, 0.0), corners),
        ("exact half pixels", (0.5 * r, 0.5 * r, 0.0), corners),
        ("diagonals through corners", (0.0, 0.0, 0.0), [[10 * r, 10 * r, 0], [-10 * r, 10 * r, 0], [10 * r, -10 * r, 0], [-7 * r, -7 * r, 0]]),
        ("duplicates of one end pixel", (0.3, -0.2, 0.0), np.array([1.234, -2.345, 0.0]) + rng.uniform(0, 0.2 * r, (400, 3)) * [1, 1, 0]),
        ("far point: several doublings", (0.0, 0.0, 0.0), [[2000 * r, -1700 * r, 0.0]]),
    ]


@pytest.mark.parametrize("resolution", [0.05, 0.1, 0.25, 1.0])
@pytest.mark.parametrize("free", [True, False])
def test_edge_batches_equal_oracle(dl, orc, ctx, resolution, free):
    pair = Pair(dl, orc, ctx, resolution, free=free)
    for name, origin, pts in edge_batches(resolution):
        before = pair.grid.stats()["growths"]
        pair.insert(np.array(origin, dtype=f32), pts)
        if name.startswith("far point"):
            assert pair.grid.stats()["growths"] - before >= 4
    assert pair.grid.stats()["inserts"] == len(edge_batches(resolution))
    pair.close()
    # each batch on a fresh grid as well: the first visit of every cell
    for name, origin, pts in edge_batches(resolution):
        pair = Pair(dl, orc, ctx, resolution, free=free)
        pair.insert(np.array(origin, dtype=f32), pts)
        pair.close()


def test_refusals_leave_the_grid_unchanged(dl, orc, ctx):
    pair = Pair(dl, orc, ctx, 0.05)
    rng = np.random.RandomState(4)
    good = rng.uniform(-8, 8, (2000, 3)).astype(f32)
    pair.insert(np.zeros(3, dtype=f32), good)
    snapshot = (pair.grid.limits(), pair.grid.cells()[0].copy(), pair.grid.stats())
    other = dl.Context(0)
    foreign = dl.PointCloud(other, good)
    L, o = dl.load_library(), np.zeros(3, dtype=f32)
    fp = C.POINTER(C.c_float)

    def status(origin, pts):
        pts = np.ascontiguousarray(pts, dtype=f32).reshape(-1, 3)
        origin = np.ascontiguousarray(origin, dtype=f32)
        return L.dliom_inserter2d_insert(pair.ins.h, pair.grid.h, origin.ctypes.data_as(fp), pts.ctypes.data_as(fp), len(pts))

    bad = good.copy()
    bad[1234, 1] = np.nan
    inf = good.copy()
    inf[7, 0] = np.inf
    cases = [(status(o, bad), dl.ERR_INVALID_ARGUMENT), (status(o, inf), dl.ERR_INVALID_ARGUMENT),
             (status([np.nan, 0, 0], good), dl.ERR_INVALID_ARGUMENT), (status([0, -np.inf, 0], good), dl.ERR_INVALID_ARGUMENT),
             (status(o, [[1e30, 0, 0]]), dl.ERR_GRID_EXTENT),       # the index leaves int
             (status(o, [[3e5, 0, 0]]), dl.ERR_GRID_EXTENT),        # beyond the budget (and num_cells * 1000 beyond int)
             (status([0, -4e6, 0], np.zeros((0, 3))), dl.ERR_GRID_EXTENT),
             (L.dliom_inserter2d_insert_cloud(pair.ins.h, pair.grid.h, o.ctypes.data_as(fp), foreign.h), dl.ERR_INVALID_ARGUMENT),
             (L.dliom_inserter2d_insert_cloud(pair.ins.h, pair.grid.h, o.ctypes.data_as(fp), None), dl.ERR_INVALID_ARGUMENT),
             (L.dliom_inserter2d_insert(pair.ins.h, pair.grid.h, o.ctypes.data_as(fp), None, -1), dl.ERR_INVALID_ARGUMENT),
             (L.dliom_inserter2d_insert(pair.ins.h, pair.grid.h, o.ctypes.data_as(fp), None, 5), dl.ERR_INVALID_ARGUMENT)]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
    small = dl.ProbabilityGrid2D(ctx, 0.05, budget_bytes=200 * 200 * 2)
    assert L.dliom_inserter2d_insert(pair.ins.h, small.h, o.ctypes.data_as(fp), good.ctypes.data_as(fp), len(good)) == dl.ERR_GRID_EXTENT
    assert small.limits()[2] == (100, 100) and not small.cells()[0].any()
    small.close()
    h = C.c_void_p()
    for hit, miss in ((0.5, 0.49), (0.55, 0.5), (0.3, 0.2), (float("nan"), 0.4)):
        assert L.dliom_inserter2d_create(ctx.h, hit, miss, 1, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert pair.grid.limits() == snapshot[0] and np.array_equal(pair.grid.cells()[0], snapshot[1]) and pair.grid.stats() == snapshot[2]
    pc.assert_equal(pair.grid, pair.ogrid)
    pair.insert(o, good * f32(1.5))  # and the grid still works
    pair.insert(np.array([0.0, 0.0, np.nan], dtype=f32), good[:100])  # the origin's z is never read (origin.head<2>())
    foreign.close()
    other.close()
    pair.close()


def test_tables_read_back_and_memory_is_counted(dl, orc, ctx):
    before = ctx.memory_stats()["probability_grid_bytes"]
    ins = dl.Inserter2D(ctx, HIT, MISS)
    hit, miss = ins.tables()
    assert np.array_equal(hit, dl.lookup_table_to_apply_correspondence_cost_odds(dl.odds(f32(HIT))))
    assert np.array_equal(miss, dl.lookup_table_to_apply_correspondence_cost_odds(dl.odds(f32(MISS))))
    grid = dl.ProbabilityGrid2D(ctx, 0.05)
    assert grid.memory_stats()["probability_grid_bytes"] == grid.stats()["bytes"] >= 100 * 100 * 2
    ins.insert(grid, (0, 0, 0), [[30.0, 1.0, 0.0]])
    assert grid.stats()["bytes"] >= 1600 * 1600 * 2
    assert ctx.memory_stats()["probability_grid_bytes"] == before + grid.stats()["bytes"] + 131072
    reads = ctx.read_backs()
    ins.insert(grid, (0, 0, 0), [[3.0, 1.0, 0.0], [2.0, 2.0, 0.0]])
    assert ctx.read_backs() - reads == 2  # the bounding box with the non-finite flag; the error words
    grid.close()
    ins.close()
    assert ctx.memory_stats()["probability_grid_bytes"] == before


def test_chain_range_filter_outlier_remover_insert(dl, orc, ctx, tmp_path):
    """range filter -> outlier remover (three phases) -> insert on the device, against the same chain through the CPU
    model of the two filters (tests/cpp/outlier_model.cc) and the oracle's insert."""
    model = oc.build_model(tmp_path)
    batches = oc.drive(6, 32, 512)
    ops = [oc.op(oc.RANGE, p, o, 1.0, 30.0) for o, p in batches]
    results, _ = oc.run_model(model, 0.15, ops, tmp_path)
    in_range = [(o, p[res[1]]) for (o, p), res in zip(batches, results)]
    results, _ = oc.run_model(model, 0.15, oc.three_pass_ops(in_range), tmp_path)
    kept_model = [p[res[1]] for (_, p), res in zip(in_range, results[2 * len(in_range):])]
    assert sum(len(k) for k in kept_model) < sum(len(p) for _, p in in_range)  # the remover removed something

    remover = dl.OutlierRemover(ctx, 0.15)
    clouds = []
    for o, p in batches:
        c = dl.PointCloud(ctx, p)
        kept, _ = c.min_max_range_filter(o, 1.0, 30.0)
        c.close()
        clouds.append(kept)
    for c in clouds:
        remover.mark_hits(c)
    for (o, _), c in zip(batches, clouds):
        remover.count_rays(o, c)
    pair = Pair(dl, orc, ctx, 0.05)
    for (o, _), c, want in zip(batches, clouds, kept_model):
        kept, _ = remover.filter(c)
        assert kept.download().tobytes() == want.tobytes()
        pair.ins.insert(pair.grid, o, kept)  # the points never left the device
        pair.ogrid.insert(o, want, HIT, MISS, True)
        pc.assert_equal(pair.grid, pair.ogrid)
        kept.close()
        c.close()
    remover.close()
    pair.close()


def test_draw_rotation_yaml_origin_and_fresh_grid(dl, orc, ctx):
    """A fresh grid: ComputeCroppedLimits gives offset 0 and 1 x 1 for an empty box (grid_2d.cc:103-107), so the
    reference draws one unknown pixel and never "no image"; so does the library."""
    pair = Pair(dl, orc, ctx, 0.05)
    image, offset = pair.grid.draw()
    assert image is not None and image.shape == (1, 1) and image[0, 0] == 128 and offset == (0, 0)
    L = dl.load_library()
    for o, p in oc.drive(2, 32, 512):
        cells = pair.insert(o, p)
    for rotate in (False, True):
        want, want_off = pc.draw(cells, rotate)
        got, off = pair.grid.draw(rotate)
        assert off == want_off and got.shape == want.shape and np.array_equal(got, want)
        assert len(np.unique(got)) > 3
    resolution, max_xy, _ = pair.grid.limits()
    pgm, yaml = pc.ros_map_files(cells, resolution, max_xy, "map.pgm")
    got, off = pair.grid.draw(True)
    h, w = got.shape
    origin = dl.ros_map_yaml_origin(resolution, max_xy, off, w, h)
    assert dl.ros_map_pgm_header(resolution, w, h) + got.tobytes() == pgm
    assert dl.ros_map_yaml(resolution, origin, "map.pgm") == yaml
    i32 = C.POINTER(C.c_int32)
    o2, s2 = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    buf = np.zeros(4, dtype=np.uint8)
    assert L.dliom_probability_grid_draw(pair.grid.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), 4, o2.ctypes.data_as(i32),
                                         s2.ctypes.data_as(i32), 1) == dl.ERR_CAPACITY and tuple(s2) == (w, h)
    pair.close()


def test_adapter_classes_write_the_oracles_ros_map(dl, orc, ctx, tmp_path):
    """io::ProbabilityGridPointsProcessor / RosMapWritingPointsProcessor of dliom_cartographer.h behind the range filter
    (tests/cpp/probability_grid_adapter.cc): the PGM and YAML bytes, the gray image and the forwarded batches against what
    is assembled here from the oracle."""
    import subprocess
    exe = str(tmp_path / "probability_grid_adapter")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(pc.ROOT, "include"), "-I",
                           os.path.join(pc.ROOT, "d-liom_amd", "cpp"), "-o", exe,
                           os.path.join(pc.ROOT, "tests", "cpp", "probability_grid_adapter.cc"), dl.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dl.LIB_PATH)])
    batches = oc.drive(5, 32, 512)
    batches.insert(2, (batches[0][0], np.zeros((0, 3), dtype=f32)))  # an empty batch in the stream
    lo, hi = 1.0, 12.0
    for resolution in (0.05, 0.1):
        out_dir = tmp_path / ("out_%g" % resolution)
        out_dir.mkdir()
        src = str(tmp_path / "batches.bin")
        with open(src, "wb") as f:
            f.write(np.array([len(batches)], dtype=np.int32).tobytes())
            for o, p in batches:
                f.write(o.tobytes() + np.array([len(p)], dtype=np.int32).tobytes() + p.tobytes())
        out = subprocess.run([exe, src, str(out_dir), repr(resolution), repr(lo), repr(hi)], timeout=300)
        assert out.returncode == 0
        ogrid = pc.new_oracle_grid(orc, resolution)
        forwarded = open(str(out_dir / "forwarded.bin"), "rb").read()
        at, removed = 0, 0
        for o, p in batches:
            cloud = dl.PointCloud(ctx, p)
            kept, index = cloud.min_max_range_filter(o, lo, hi)
            kept.close()
            cloud.close()
            removed += len(p) - len(index)
            ogrid.insert(o, p[index], HIT, MISS, True)
            n = int(np.frombuffer(forwarded, dtype=np.int32, count=1, offset=at)[0])
            assert n == len(index)
            assert forwarded[at + 4:at + 4 + 12 * n] == p[index].tobytes()  # forwarded untouched by the two map stages
            assert np.array_equal(np.frombuffer(forwarded, dtype=f32, count=n, offset=at + 4 + 12 * n), index.astype(f32))
            at += 4 + 16 * n
        assert at == len(forwarded) and removed > 0
        cells = ogrid.cells()
        pgm, yaml = pc.ros_map_files(cells, ogrid.resolution, ogrid.max_xy, "map.pgm")
        assert open(str(out_dir / "map.pgm"), "rb").read() == pgm
        assert open(str(out_dir / "map.yaml"), "rb").read() == yaml
        want, want_off = pc.draw(cells, False)
        data = open(str(out_dir / "grid.bin"), "rb").read()
        w, h, ox, oy = (int(v) for v in np.frombuffer(data, dtype=np.int32, count=4))
        assert (h, w) == want.shape and (ox, oy) == want_off and data[16:] == want.tobytes()
        assert len(np.unique(want)) > 3 and want.shape[0] > 100


def test_fuzz_slice(dl, orc, ctx):
    import fuzz_probability_grid as fz
    report = fz.run(dl, orc, ctx, seed=1, cases=12)
    print(report)
    assert report["skipped"] == 0 and report["cases"] == 12 and report["inserts"] > 12
