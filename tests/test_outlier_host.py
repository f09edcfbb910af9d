"""Moving-object removal without a GPU: the new names are bound in the library and their argument checks refuse before
anything runs; and the CPU model (tests/cpp/outlier_model.cc) on cases small enough to work out by hand, which are
written down here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlier_common as oc  # noqa: E402
from outlier_common import FILTER, MARK, RANGE, RAYS, TRACE, f32, op  # noqa: E402

NAMES = ("dliom_outlier_remover_create", "dliom_outlier_remover_destroy", "dliom_outlier_remover_mark_hits",
         "dliom_outlier_remover_count_rays", "dliom_outlier_remover_filter", "dliom_outlier_remover_voxels",
         "dliom_outlier_remover_stats", "dliom_cloud_min_max_range_filter")


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return oc.build_model(tmp_path_factory.mktemp("outlier_model"))


def table_dict(table):
    return {tuple(int(v) for v in c): (int(h), int(r)) for c, h, r in zip(*table)}


def test_names_are_bound_and_declared(dl):
    bound = {name for name, _, _ in dl.SYMBOLS}
    header = open(os.path.join(oc.ROOT, "include", "dliom.h")).read()
    lib = C.CDLL(dl.LIB_PATH)
    for name in NAMES:
        assert name in bound and name + "(" in header and hasattr(lib, name), name
    assert hasattr(dl, "OutlierRemover") and hasattr(dl.PointCloud, "min_max_range_filter")
    assert "outlier_table_bytes" in dict(dl.MemoryStats._fields_)


def test_argument_checks_refuse_before_anything_runs(dl):
    """No device is touched: the handles are never dereferenced (they point at zeroed host memory)."""
    L = dl.load_library()
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # stands for a context / remover / cloud
    out, n = C.c_void_p(), C.c_int64()
    o = (C.c_float * 3)(0, 0, 0)
    i32 = (C.c_int32 * 4)()
    bad = dl.ERR_INVALID_ARGUMENT
    assert L.dliom_outlier_remover_create(None, 0.05, C.byref(out)) == bad
    assert L.dliom_outlier_remover_create(fake, 0.05, None) == bad
    for size in (0.0, -0.05, float("nan"), float("inf"), 1e-60, 1e60):  # the last two: 0 and inf as the grid's float
        assert L.dliom_outlier_remover_create(fake, size, C.byref(out)) == bad, size
    assert L.dliom_outlier_remover_destroy(None) == bad
    assert L.dliom_outlier_remover_mark_hits(None, fake) == bad and L.dliom_outlier_remover_mark_hits(fake, None) == bad
    assert L.dliom_outlier_remover_count_rays(None, o, fake) == bad
    assert L.dliom_outlier_remover_count_rays(fake, None, fake) == bad
    assert L.dliom_outlier_remover_count_rays(fake, o, None) == bad
    assert L.dliom_outlier_remover_filter(None, fake, C.byref(out), i32, 4, C.byref(n)) == bad
    assert L.dliom_outlier_remover_filter(fake, None, C.byref(out), i32, 4, C.byref(n)) == bad
    assert L.dliom_outlier_remover_filter(fake, fake, None, i32, 4, C.byref(n)) == bad
    assert L.dliom_outlier_remover_filter(fake, fake, C.byref(out), i32, 4, None) == bad
    assert L.dliom_outlier_remover_filter(fake, fake, C.byref(out), i32, -1, C.byref(n)) == bad
    assert L.dliom_outlier_remover_voxels(None, i32, i32, i32, 1, C.byref(n)) == bad
    assert L.dliom_outlier_remover_voxels(fake, i32, i32, i32, 1, None) == bad
    assert L.dliom_outlier_remover_voxels(fake, i32, i32, i32, -1, C.byref(n)) == bad
    assert L.dliom_outlier_remover_stats(None, C.byref(dl.OutlierStats())) == bad
    assert L.dliom_outlier_remover_stats(fake, None) == bad
    for args in ((None, fake, o, 1.0, 2.0, C.byref(out), i32, 4, C.byref(n)),
                 (fake, None, o, 1.0, 2.0, C.byref(out), i32, 4, C.byref(n)),
                 (fake, fake, None, 1.0, 2.0, C.byref(out), i32, 4, C.byref(n)),
                 (fake, fake, o, 1.0, 2.0, None, i32, 4, C.byref(n)),
                 (fake, fake, o, 1.0, 2.0, C.byref(out), i32, 4, None),
                 (fake, fake, o, 1.0, 2.0, C.byref(out), i32, -1, C.byref(n))):
        assert L.dliom_cloud_min_max_range_filter(*args) == bad
    assert not out.value


def test_one_ray_through_two_hit_voxels_and_the_length_boundary(model, tmp_path):
    """voxel_size 1 keeps everything exact.  Hits at x = 2, 4 and 4.5 (cells 2, 4 and lround(4.5) = 5).
    Ray 0 -> 2: x = 0, 1        (x < 2): cells 0, 1           -- its own voxel is not sampled
    Ray 0 -> 4: x = 0, 1, 2, 3  (x < 4, the length is an exact multiple of the step): cell 2 counted, cell 4 is not
    Ray 0 -> 4.5: x = 0 .. 4: cells 0, 1, 2, 3, 4: cells 2 and 4 counted, cell 5 is not
    A point at the origin has length 0 and makes no sample, not even in its own voxel."""
    pts = np.array([[2, 0, 0], [4, 0, 0], [4.5, 0, 0], [0, 0, 0]], dtype=f32)
    results, table = oc.run_model(model, 1.0, [op(MARK, pts), op(RAYS, pts), op(FILTER, pts), op(TRACE, pts)], tmp_path)
    assert table_dict(table) == {(0, 0, 0): (1, 3), (2, 0, 0): (1, 2), (4, 0, 0): (1, 1), (5, 0, 0): (1, 0)}
    # rays < 3 * hits: (0,0,0) has 3 rays on 1 hit -> removed; the others stay
    assert results[0] == 0 and results[1] == 0 and results[2][0] == 0 and results[2][1].tolist() == [0, 1, 2]
    assert [len(r[0]) for r in results[3]] == [2, 4, 5, 0]
    assert results[3][2][0][:, 0].tolist() == [0, 1, 2, 3, 4]
    # two samples of one ray in the same voxel count twice: step 0.5 in a grid of 0.5 would not do it, a diagonal does
    diag = np.array([[1.0, 1.0, 0.0]], dtype=f32)  # length sqrt(2): x = 0, 1 -> samples (0,0,0), (0.7071, 0.7071, 0)
    results, table = oc.run_model(model, 1.0, [op(MARK, [[1, 1, 0]]), op(RAYS, diag), op(RAYS, diag)], tmp_path)
    assert table_dict(table) == {(1, 1, 0): (1, 2)}  # lround(0.7071) = 1 on both axes, once per RAYS op


def test_three_hits_boundary_on_both_sides(model, tmp_path):
    """One hit in cell 2; every ray 0 -> (3, 0, 0) samples x = 0, 1, 2 and counts once in it.  rays = 2 < 3 * 1 keeps the
    point, rays = 3 removes it; with two hits the limit is 6."""
    hit = np.array([[2, 0, 0]], dtype=f32)
    for hits, rays, kept in ((1, 2, True), (1, 3, False), (2, 5, True), (2, 6, False), (1, 0, True)):
        through = np.tile(np.array([[3, 0, 0]], dtype=f32), (rays, 1))
        results, table = oc.run_model(model, 1.0, [op(MARK, hit)] * hits + [op(RAYS, through), op(FILTER, hit)], tmp_path)
        assert table_dict(table) == {(2, 0, 0): (hits, rays)}
        assert results[-1][1].tolist() == ([0] if kept else [])
    # a point whose voxel was never marked: VoxelData(), !(0 < 0): removed
    results, _ = oc.run_model(model, 1.0, [op(MARK, hit), op(FILTER, [[7, 7, 7], [2, 0, 0]])], tmp_path)
    assert results[-1][1].tolist() == [1]


def test_recurrence_is_not_the_product_form(model, tmp_path):
    """x += voxel_size_ is a float recurrence, x = float(double(x) + 0.05); over a 60 m ray it departs from k * 0.05f and
    some samples land in other cells.  The test of the device against this model guards that only if such samples exist
    on the ray used: asserted here."""
    ray = np.array([[41.3, 37.9, 21.7]], dtype=f32)  # 60.1 m
    (trace,), _ = oc.run_model(model, 0.05, [op(TRACE, ray)], tmp_path)
    recurrence, product = trace[0]
    x, xs = f32(0), []
    while x < np.sqrt(ray[0, 0] * ray[0, 0] + (ray[0, 1] * ray[0, 1] + ray[0, 2] * ray[0, 2])):
        xs.append(x)
        x = f32(np.float64(x) + 0.05)
    assert len(recurrence) == len(xs) and 1195 <= len(xs) <= 1210
    assert any(xs[k] != f32(k) * f32(0.05) for k in range(len(xs)))
    differing = int(np.any(recurrence != product, axis=1).sum())
    print("samples %d, cells that differ from the product form: %d" % (len(xs), differing))
    assert differing >= 1


def test_extent_rule(model, tmp_path):
    """Indices [-8192, 8191] per axis: 8191 and -8192 are accepted, 8192 and -8193 refused with the table unchanged (the
    accepted point of the refused batch included)."""
    ok = np.array([[8191, 0, 0], [0, -8192, 0], [0, 0, 8191]], dtype=f32)
    ops = [op(MARK, ok), op(MARK, [[1, 1, 1], [8192, 0, 0]]), op(MARK, [[0, 0, -8193]]), op(MARK, [[np.inf, 0, 0]]),
           op(RAYS, [[9000, 0, 0]]), op(FILTER, [[8191, 0, 0], [8192, 0, 0]])]
    results, table = oc.run_model(model, 1.0, ops, tmp_path)
    assert results[:5] == [0, -6, -6, -1, 0]
    # the ray 0 -> 9000 samples cells 0 .. 8999: 8191 is counted once, the samples beyond read no voxel
    assert table_dict(table) == {(8191, 0, 0): (1, 1), (0, -8192, 0): (1, 0), (0, 0, 8191): (1, 0)}
    assert results[5][1].tolist() == [0]  # the pass-3 point outside the grid is removed
    # the loop of a ray of voxel_size * 2^24 does not end in the reference: refused
    results, _ = oc.run_model(model, 1.0, [op(RAYS, [[16777216.0, 0, 0]]), op(RAYS, [[16777215.0, 0, 0]][:0])], tmp_path)
    assert results == [-7, 0]


def test_min_max_range_model(model, tmp_path):
    pts = np.array([[3, 4, 0], [0.6, 0.8, 0], [6, 8, 0], [0, 0, 0], [3, 4, 0.01]], dtype=f32)
    (status, kept), = oc.run_model(model, 1.0, [op(RANGE, pts, (0, 0, 0), 1.0, 5.0)], tmp_path)[0]
    assert status == 0 and kept.tolist() == [0, 1]  # range == bound on both sides is kept; 5.00001 is not
    (_, kept), = oc.run_model(model, 1.0, [op(RANGE, pts, (3, 4, 0), 0.0, 0.0)], tmp_path)[0]
    assert kept.tolist() == [0]


def test_kept_set_does_not_depend_on_batch_order(model, tmp_path):
    rng = np.random.RandomState(4)
    centre = np.array([1.0, -2.0, 0.5])
    batches = []
    for _ in range(5):
        o = (centre + rng.uniform(-3, 3, 3)).astype(f32)
        d = rng.normal(size=(400, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        batches.append((o, (centre + d * rng.choice([2.0, 4.0], 400)[:, None]).astype(f32)))
    def kept_sets(p1, p2, p3):
        ops = ([op(MARK, batches[i][1]) for i in p1] + [op(RAYS, batches[i][1], batches[i][0]) for i in p2] +
               [op(FILTER, batches[i][1]) for i in p3])
        results, table = oc.run_model(model, 0.2, ops, tmp_path)
        return {i: r[1].tolist() for i, r in zip(p3, results[10:])}, table
    base, table = kept_sets(range(5), range(5), range(5))
    removed = sum(400 - len(v) for v in base.values())
    assert 0 < removed < 2000 and np.any(table[2] > 0)
    for seed in range(4):
        r = np.random.RandomState(seed)
        other, other_table = kept_sets(r.permutation(5), r.permutation(5), r.permutation(5))
        assert other == base and all(np.array_equal(a, b) for a, b in zip(table, other_table))
