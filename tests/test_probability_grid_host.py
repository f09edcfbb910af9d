"""The host side of the 2D probability grid (include/dliom.h, "2D probability grid of the export pipeline") without a
GPU: the two lookup tables and the growth of the limits against the CPU oracle, the colour table and the ROS map texts
against restatements of the reference lines they replace, the refusals that must not touch a device, the ABI."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probability_grid_common as pc  # noqa: E402

f32 = np.float32


@pytest.fixture(scope="module")
def dl():
    import __graft_entry__
    __graft_entry__.build()
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def orc(dl):
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("p", [0.55, 0.49, 0.7, 0.4, 0.9, 0.1, 0.51, 0.62])
def test_correspondence_cost_tables_equal_oracle(dl, orc, p):
    odds = orc.odds(f32(p))
    want = np.zeros(32768, dtype=np.uint16)
    orc.lib().orc_lookup_table_to_apply_correspondence_cost_odds(C.c_float(odds), want.ctypes.data_as(C.POINTER(C.c_uint16)))
    got = dl.lookup_table_to_apply_correspondence_cost_odds(dl.odds(f32(p)))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, dl.compute_lookup_table_to_apply_odds(dl.odds(f32(p))))  # not the 3D inserter's table


def oracle_grow(orc, resolution, max_xy, num_cells, point):
    """Limits of an oracle grid after GrowLimits(point): an insert of no returns with the origin at `point` pads it by
    1e-6, so the test feeds the library the same two padded corners."""
    g = orc.ProbabilityGrid(resolution, max_xy, num_cells[0], num_cells[1])
    g.insert(np.array([point[0], point[1], 0.0], dtype=f32), np.zeros((0, 3), dtype=f32), 0.55, 0.49)
    g.cells()
    return g.max_xy, (g.num_x_cells, g.num_y_cells)


def library_grow(dl, resolution, max_xy, num_cells, point):
    """GrowAsNeeded on one point: min corner, then max corner, as two calls."""
    pad = f32(1e-6) * f32(1.0)
    lo = (f32(point[0]) - pad, f32(point[1]) - pad)
    hi = (f32(point[0]) + pad, f32(point[1]) + pad)
    mx, nc, off1, t1 = dl.probability_grid_grow_limits(resolution, max_xy, num_cells, lo)
    mx, nc, off2, t2 = dl.probability_grid_grow_limits(resolution, mx, nc, hi)
    return (float(mx[0]), float(mx[1])), (int(nc[0]), int(nc[1])), off1 + off2, t1 + t2


def test_limits_growth_equals_oracle_on_random_far_points(dl, orc):
    rng = np.random.RandomState(11)
    most = 0
    for case in range(200):
        resolution = float(rng.choice([0.05, 0.1, 0.02, 0.37, 1.0]))
        max_xy = (0.5 * 100 * resolution, 0.5 * 100 * resolution) if case % 2 else tuple(rng.uniform(-3, 3, 2))
        num = (100, 100) if case % 2 else (int(rng.randint(1, 40)), int(rng.randint(1, 40)))
        point = rng.uniform(-1, 1, 2) * 10.0 ** rng.uniform(-1, 1.8)  # at most 63 m: inside the default budget at 2 cm
        want_max, want_num = oracle_grow(orc, resolution, max_xy, num, point)
        got_max, got_num, offset, turns = library_grow(dl, resolution, max_xy, num, point)
        assert got_num == want_num and got_max == tuple(want_max), (case, resolution, point)
        assert got_num[0] == num[0] << turns and got_num[1] == num[1] << turns
        assert offset[0] == sum((num[0] << k) // 2 for k in range(turns)) and offset[1] == sum((num[1] << k) // 2 for k in range(turns))
        most = max(most, turns)
    assert most >= 4  # several doublings in one call were among the cases


def test_limits_growth_min_corner_before_max_corner(dl, orc):
    """A batch whose min and max corners both lie outside: the order of the two GrowLimits calls decides where the
    grid ends up, and it is the reference's (ray_casting.cc:158-161)."""
    resolution, max_xy, num = 0.5, (2.0, 2.0), (8, 8)
    g = orc.ProbabilityGrid(resolution, max_xy, *num)
    pts = np.array([[-9.0, -7.5, 0], [11.0, 6.25, 0]], dtype=f32)
    g.insert(np.zeros(3, dtype=f32), pts, 0.55, 0.49, insert_free_space=False)
    g.cells()
    pad = f32(1e-6)
    mx, nc, _, _ = dl.probability_grid_grow_limits(resolution, max_xy, num, (f32(-9.0) - pad, f32(-7.5) - pad))
    mx, nc, _, _ = dl.probability_grid_grow_limits(resolution, mx, nc, (f32(11.0) + pad, f32(6.25) + pad))
    assert (float(mx[0]), float(mx[1])) == tuple(g.max_xy) and (int(nc[0]), int(nc[1])) == (g.num_x_cells, g.num_y_cells)


def test_limits_growth_refusals_leave_the_limits(dl):
    mx, nc = np.array([2.5, 2.5]), np.array([100, 100], dtype=np.int32)
    off, turns = np.zeros(2, dtype=np.int32), C.c_int32()
    L = dl.load_library()

    def grow(px, py, budget=0):
        return L.dliom_probability_grid_grow_limits(0.05, mx.ctypes.data_as(C.POINTER(C.c_double)), nc.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    C.c_float(px), C.c_float(py), budget, off.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    C.byref(turns))
    assert grow(1e30, 0.0) == dl.ERR_GRID_EXTENT       # the index leaves int
    assert grow(1e6, 0.0) == dl.ERR_GRID_EXTENT        # num_cells * 1000 would leave int, or the budget
    assert grow(30.0, 0.0, budget=100000) == dl.ERR_GRID_EXTENT  # budget
    assert grow(float("nan"), 0.0) == dl.ERR_INVALID_ARGUMENT
    assert grow(float("inf"), 0.0) == dl.ERR_INVALID_ARGUMENT
    assert tuple(mx) == (2.5, 2.5) and tuple(nc) == (100, 100)
    assert grow(30.0, 0.0) == dl.OK and tuple(nc) == (1600, 1600)


def test_color_table_equals_restatement(dl):
    assert np.array_equal(dl.probability_grid_color_table(), pc.color_table())


@pytest.mark.parametrize("resolution,text", [(0.05, "0.050000"), (0.1, "0.100000")])
def test_pgm_header_and_yaml_text(dl, resolution, text):
    assert dl.ros_map_pgm_header(resolution, 640, 481) == ("P5\n# Cartographer map; %s m/pixel\n640 481\n255\n" % text).encode()
    origin = dl.ros_map_yaml_origin(resolution, (40.0, 38.5), (17, 3), 481, 640)
    want = (40.0 - (3 + 481) * resolution, 38.5 - (17 + 640) * resolution)
    assert tuple(origin) == want
    got = dl.ros_map_yaml(resolution, origin, "map.pgm")
    assert got == ("image: map.pgm\nresolution: %s\norigin: [%.6f, %.6f, 0.0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
                   % (text, want[0], want[1])).encode()
    n = C.c_int64()
    assert dl.load_library().dliom_ros_map_pgm_header(resolution, 1, 1, None, 0, C.byref(n)) == dl.ERR_CAPACITY and n.value > 0


def test_refusals_that_touch_no_device(dl):
    L = dl.load_library()
    h = C.c_void_p()
    origin = (C.c_float * 3)(0, 0, 0)
    fake = C.c_void_p(1)  # never dereferenced: every call below refuses on a NULL argument first
    assert L.dliom_probability_grid_create(None, 0.05, 0, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_create_with_limits(None, 1.0, 1.0, 5.0, 5, 5, 0, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_destroy(None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_inserter2d_create(None, 0.55, 0.49, 1, C.byref(h)) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_inserter2d_destroy(None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_inserter2d_insert_cloud(None, None, origin, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_inserter2d_insert_cloud(fake, None, origin, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_inserter2d_insert(None, None, origin, None, 0) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_inserter2d_insert(fake, None, origin, None, -1) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_inserter2d_tables(None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_cells(None, None, 0, None, None, 0) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_draw(None, None, 0, None, None, 0) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_get_probabilities(None, None, 0, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_limits(None, None, None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_get_stats(None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_memory_stats(None, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_probability_grid_color_table(None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_compute_lookup_table_to_apply_correspondence_cost_odds(1.0, None) == dl.ERR_INVALID_ARGUMENT
    assert L.dliom_ros_map_yaml_origin(0.05, None, None, 1, 1, None) == dl.ERR_INVALID_ARGUMENT


def test_abi_symbols_present(dl):
    header = open(os.path.join(ROOT, "include", "dliom.h")).read()
    declared = set(re.findall(r"\b(dliom_[a-z0-9_]+)\s*\(", header))
    bound = {name for name, _, _ in dl.SYMBOLS}
    ours = {n for n in declared if "probability_grid" in n or "inserter2d" in n or "ros_map" in n or "correspondence_cost" in n}
    assert len(ours) == 20 and ours <= bound
    lib = C.CDLL(dl.LIB_PATH)
    for name in ours:
        assert hasattr(lib, name), name
    assert "probability_grid_bytes" in dict(dl.MemoryStats._fields_)
    assert (dl.KERNEL_PG_HITS, dl.KERNEL_PG_RAYS, dl.KERNEL_PG_CLEAR) == (6, 7, 8) and "DLIOM_KERNEL_COUNT = 9" in header
