"""NDT on the device against the CPU model of tests/ndt_common.py: bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_common as ic  # noqa: E402
import ndt_common as nd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dl():
    import dliom
    dliom.load_library()
    return dliom


@pytest.fixture(scope="module")
def ctx(dl):
    c = dl.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit for bit, any NaN standing for any other"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def device_options(dl, o):
    return dl.ndt_options(**o)


def check_cells(dl, ctx, points, **overrides):
    """The target's cells equal the model's: indices, counts, validity, and the bits of mean and icov -> the model's cells"""
    o = nd.options(**overrides)
    want = nd.build_cells(points, o)
    target = dl.NdtTarget(ctx, points, device_options(dl, o))
    try:
        got, stats = target.cells(), target.memory_stats()
    finally:
        target.close()
    assert np.array_equal(got["index"], want["index"])
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["valid"], want["valid"])
    assert same_bits(got["mean"], want["mean"]), np.flatnonzero((bits(got["mean"]) != bits(want["mean"])).any(axis=1))[:8]
    assert same_bits(got["icov"], want["icov"]), np.flatnonzero((bits(got["icov"]) != bits(want["icov"])).any(axis=1))[:8]
    assert (stats["points"], stats["kept_points"], stats["cells"], stats["valid_cells"]) == \
        (len(points), want["kept_points"], len(want["n"]), int(want["valid"].sum()))
    return want


def blob(rng, centre, n, spread=0.15):
    return (np.asarray(centre) + spread * rng.standard_normal((n, 3))).astype(np.float32)


# ---- cells ---------------------------------------------------------------------------------------------------------------------
def test_cells_of_every_length(dl, ctx):
    """Cells of 1 .. 4097 points, one beside the other: below and at the minimum, one wave, one workgroup's chunk and its
    neighbours, and 17 chunks (32 with the padding) through the binary counter"""
    rng = np.random.RandomState(1)
    sizes = [1, 2, 3, 5, 6, 255, 256, 257, 4097]
    parts = [blob(rng, [2.0 * k + 0.5, 0.5, 0.5], n, 0.1) for k, n in enumerate(sizes)]
    points = np.concatenate(parts)
    points = points[rng.permutation(len(points))]  # a cell's points are not adjacent in the cloud
    want = check_cells(dl, ctx, points)
    main = {tuple(i): n for i, n in zip(want["index"], want["n"])}
    assert all(main[(2 * k, 0, 0)] >= n - 3 for k, n in enumerate(sizes))  # (a 0.1 m blob may lose a point to a neighbour)
    assert want["valid"].sum() >= 5


def test_cells_on_faces_negative_and_rounding(dl, ctx):
    """Points exactly on cell faces and an ulp from them, negative coordinates, and resolution 0.3, where x * inv rounds"""
    rng = np.random.RandomState(2)
    faces = np.array([-2.0, -1.0, 0.0, 1.0, 2.0, 3.0], np.float32)
    near = np.concatenate([faces, np.nextafter(faces, np.float32(-9)), np.nextafter(faces, np.float32(9))])
    grid = np.stack(np.meshgrid(near, near[:6], [0.25, -0.25]), axis=-1).reshape(-1, 3).astype(np.float32)
    cloud = np.concatenate([grid, blob(rng, [-3.5, -2.5, -1.5], 40), blob(rng, [-0.5, 0.5, -0.5], 40)])
    check_cells(dl, ctx, cloud)
    thirds = (0.3 * rng.randint(-20, 20, (600, 3)) + rng.choice([0.0, 1e-7, -1e-7], (600, 3))).astype(np.float32)
    want = check_cells(dl, ctx, np.concatenate([thirds, blob(rng, [0.1, 0.1, 0.1], 200, 0.2)]), resolution=0.3)
    assert want["valid"].sum() >= 1


def test_degenerate_cells(dl, ctx):
    """All z equal (the floor or the refusal, whichever the statement yields on these sums), identical points (invalid),
    non-finite points (skipped), points beyond the key range (skipped)"""
    rng = np.random.RandomState(3)
    flat = np.c_[rng.uniform(0.1, 0.9, (20, 2)), np.full(20, 0.5)].astype(np.float32)
    same = np.tile(np.array([[1.5, 0.5, 0.5]], np.float32), (9, 1))
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [3e6, 0.5, 0.5], [0.5, -1.2e6, 0.5]], np.float32)
    edge = np.array([[1048575.5, 0.5, 0.5], [-1048576.0, 0.5, 0.5]], np.float32)
    want = check_cells(dl, ctx, np.concatenate([flat, bad, same, edge, blob(rng, [4.5, 0.5, 0.5], 30)]))
    by_index = {tuple(i): (n, v) for i, n, v in zip(want["index"], want["n"], want["valid"])}
    assert by_index[(1, 0, 0)] == (9, False) and by_index[(0, 0, 0)][0] == 20
    assert (1048575, 0, 0) in by_index and (-1048576, 0, 0) in by_index and want["kept_points"] == 20 + 9 + 2 + 30


def test_sparse_box(dl, ctx):
    """Two clusters 3000 m apart: six thousand cells an axis between them, none of them stored"""
    rng = np.random.RandomState(4)
    a = np.concatenate([blob(rng, [0.5 + k, 0.5, 0.5], 12) for k in range(6)])
    b = a + np.array([3000.0, -3000.0, 3000.0], np.float32)
    want = check_cells(dl, ctx, np.concatenate([a, b]))
    assert len(want["n"]) < 200 and want["valid"].sum() >= 8


# ---- evaluation ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """About 300 cells: blobs on a 10 x 10 x 3 lattice of cell centres, and the model's cells"""
    rng = np.random.RandomState(5)
    centres = np.stack(np.meshgrid(np.arange(-5, 5), np.arange(-5, 5), np.arange(-1, 2)), axis=-1).reshape(-1, 3) + 0.5
    target = np.concatenate([blob(rng, c + rng.uniform(-0.2, 0.2, 3), rng.randint(4, 20)) for c in centres])
    target.setflags(write=False)
    cells = nd.build_cells(target)
    assert 250 <= cells["valid"].sum() <= 300
    return target, cells


@pytest.fixture(scope="module")
def scene_target(dl, ctx, scene):
    t = dl.NdtTarget(ctx, scene[0])
    yield t
    t.close()


def source_points(n, seed=6):
    """Inside the lattice, in the empty cells beside it, outside the box, and a few that are not finite"""
    rng = np.random.RandomState(seed)
    p = rng.uniform([-6.5, -6.5, -2.5], [6.5, 6.5, 3.5], (n, 3)).astype(np.float32)
    if n >= 16:
        p[3] = [40.0, 40.0, 40.0]
        p[5] = [-1e30, 0.0, 0.0]
        p[7] = [np.nan, 0.0, 0.0]
        p[9] = [0.0, np.inf, 0.0]
        p[11] = [2.2e6, 0.5, 0.5]
    return p


GENERIC_P = [0.4, -0.3, 0.2, 0.05, -0.08, 0.11]


def check_evaluation(dl, target, cells, source, p, what, o=None):
    got = dl.Ndt(target).evaluate(source, p, what)
    want = nd.evaluate(cells, source, p, o, what)
    assert got["pairs"] == want["pairs"]
    assert same_bits([got["score"]], [want["score"]]), (got["score"], want["score"])
    assert same_bits(got["gradient"], want["gradient"]), (got["gradient"], want["gradient"])
    assert same_bits(got["hessian"], want["hessian"]), np.argwhere(bits(got["hessian"]) != bits(want["hessian"]))[:6]
    return want


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 5000])
@pytest.mark.parametrize("p", [[0.0] * 6, GENERIC_P], ids=["zero", "generic"])
def test_evaluation_equals_model(dl, scene, scene_target, n, p):
    source = source_points(n)
    full = check_evaluation(dl, scene_target, scene[1], source, p, nd.EVAL_ALL)
    grad = check_evaluation(dl, scene_target, scene[1], source, p, nd.EVAL_GRADIENT)
    hess = check_evaluation(dl, scene_target, scene[1], source, p, nd.EVAL_HESSIAN)
    assert same_bits(grad["gradient"], full["gradient"]) and same_bits(hess["hessian"], full["hessian"])
    if n > 1:
        assert full["pairs"] > n // 2 and full["score"] > 0.0


def test_evaluation_at_the_radius_and_without_cells(dl, ctx):
    """A query at exactly r from a centroid (a pair), two ulps beyond (none); a target without a valid cell (zeros)"""
    rng = np.random.RandomState(6)
    cell = (np.array([0.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (16, 3))).astype(np.float32)
    cells = nd.build_cells(cell)
    m = cells["valid_mean"][0].astype(np.float32)
    at_r = np.array([m[0] + np.float32(1.0), m[1], m[2]], np.float32)
    beyond = at_r.copy()
    beyond[0] = np.nextafter(np.nextafter(at_r[0], np.float32(9)), np.float32(9))
    target = dl.NdtTarget(ctx, cell)
    try:
        assert check_evaluation(dl, target, cells, np.array([at_r]), [0.0] * 6, nd.EVAL_ALL)["pairs"] == 1
        assert check_evaluation(dl, target, cells, np.array([beyond]), [0.0] * 6, nd.EVAL_ALL)["pairs"] == 0
        assert check_evaluation(dl, target, cells, np.array([at_r, beyond, m]), [0.0] * 6, nd.EVAL_ALL)["pairs"] == 2
    finally:
        target.close()
    few = cell[:5]
    target = dl.NdtTarget(ctx, few)
    try:
        want = check_evaluation(dl, target, nd.build_cells(few), source_points(100), GENERIC_P, nd.EVAL_ALL)
        assert want["pairs"] == 0 and want["score"] == 0.0 and not want["hessian"].any()
        r = dl.Ndt(target).align(source_points(100))
        assert (r["converged"], r["reason"], r["iterations"], r["score"]) == (1, dl.NDT_ZERO_STEP, 0, 0.0)
        assert np.array_equal(r["transform"], np.eye(4)) and r["evaluations_with_hessian"] == 1
    finally:
        target.close()


# ---- alignment -----------------------------------------------------------------------------------------------------------------
def filtered(points):
    return nd.approximate_voxel_grid(points, 0.2)


def alignment_pairs():
    """(source, target) of the issue's cases: a moved copy and two different scans, every 8th point of the ground scan,
    raw and filtered at 0.2 m"""
    moved_source, target, _ = ic.moved_copy()
    other = ic.ground_scan(0.35)
    return {"moved": (moved_source[::4], target), "moved-filtered": (filtered(moved_source[::4]), filtered(target)),
            "scans": (other[::8], target), "scans-filtered": (filtered(other[::8]), filtered(target))}


_MODEL = {}


def model_alignment(name, mode, **overrides):
    """The model's alignment, computed once for the tests that share it, and left unchanged"""
    key = (name, mode, tuple(sorted((k, v.tobytes() if k == "guess" else v) for k, v in overrides.items())))
    if key not in _MODEL:
        source, target = alignment_pairs()[name]
        o = nd.options(step_mode=mode, **{k: v for k, v in overrides.items() if k != "guess"})
        _MODEL[key] = (nd.align(nd.build_cells(target, o), source, target, overrides.get("guess"), o), o)
    return _MODEL[key]


def compare_alignment(got, want, with_fitness=True):
    for k in ("converged", "reason", "iterations", "evaluations_with_hessian", "evaluations_without_hessian", "pairs"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert same_bits(got["p"], want["p"]), (got["p"], want["p"])
    assert same_bits(got["transform"], want["transform"])
    assert same_bits([got["score"], got["transformation_probability"]], [want["score"], want["transformation_probability"]])
    if with_fitness:
        assert got["fitness_count"] == want["fitness_count"] and same_bits([got["fitness_score"]], [want["fitness_score"]])
    else:
        assert got["fitness_count"] == 0 and np.isnan(got["fitness_score"])


@pytest.mark.parametrize("mode", [nd.STEP_CLAMPED, nd.STEP_MORE_THUENTE], ids=["clamped", "more-thuente"])
@pytest.mark.parametrize("name", ["moved", "moved-filtered", "scans", "scans-filtered"])
def test_alignment_equals_model(dl, ctx, name, mode):
    source, target_points = alignment_pairs()[name]
    want, o = model_alignment(name, mode)
    target, index = dl.NdtTarget(ctx, target_points, device_options(dl, o)), dl.NnIndex(ctx, target_points)
    try:
        got, aligned = dl.Ndt(target, fitness_index=index).align(source, want_aligned=True)
        compare_alignment(got, want)
        assert np.array_equal(aligned.view(np.uint32), want["aligned"].view(np.uint32))
        evaluations = got["evaluations_with_hessian"] + got["evaluations_without_hessian"]
        assert got["read_backs"] == evaluations + 2  # the fitness score's and the aligned cloud's norm
        if mode == nd.STEP_CLAMPED:
            assert got["evaluations_without_hessian"] == 0
        again = dl.Ndt(target, fitness_index=index).align(source)  # twice, same bytes
        for k in ("p", "transform"):
            assert got[k].tobytes() == again[k].tobytes()
        assert all(got[k] == again[k] for k in ("score", "fitness_score", "iterations", "pairs", "reason"))
        compare_alignment(dl.Ndt(target).align(source), want, with_fitness=False)  # without the fitness index
    finally:
        index.close()
        target.close()


@pytest.mark.parametrize("most", [0, 1])
def test_alignment_iteration_limits_and_guess(dl, ctx, most):
    guess = nd.transform_of([0.1, -0.05, 0.02, 0.01, 0.02, -0.03])
    source, target_points = alignment_pairs()["moved"]
    want, o = model_alignment("moved", nd.STEP_CLAMPED, maximum_iterations=most, transformation_epsilon=0.0)
    want_guess, _ = model_alignment("moved", nd.STEP_MORE_THUENTE, maximum_iterations=most + 2, guess=guess)
    assert (want["reason"], want["iterations"]) == (nd.ITERATIONS, most + 2)
    target = dl.NdtTarget(ctx, target_points, device_options(dl, o))
    try:
        compare_alignment(dl.Ndt(target).align(source), want, with_fitness=False)
        o2 = device_options(dl, nd.options(step_mode=nd.STEP_MORE_THUENTE, maximum_iterations=most + 2))
        compare_alignment(dl.Ndt(target, o2).align(source, guess=guess), want_guess, with_fitness=False)
    finally:
        target.close()


def test_profiled_alignment_reports_stage_times(dl, ctx):
    source, target_points = alignment_pairs()["moved"]
    want, o = model_alignment("moved", nd.STEP_CLAMPED)
    ctx.set_profiling(1)
    try:
        target = dl.NdtTarget(ctx, target_points)
        try:
            got = dl.Ndt(target).align(source)
            stats = target.memory_stats()
        finally:
            target.close()
    finally:
        ctx.set_profiling(0)
    compare_alignment(got, want, with_fitness=False)
    assert got["evaluate_ms"] > 0.0 and got["reduce_ms"] > 0.0 and got["host_ms"] >= 0.0 and stats["build_ms"] > 0.0
    assert stats["read_backs"] == 2


def test_argument_checks_on_the_device(dl, ctx):
    L = dl.load_library()
    points = ic.ground_scan()
    cloud = dl.PointCloud(ctx, points)
    other = dl.Context(0)
    h, r = C.c_void_p(), dl.NdtResult()
    eye = np.eye(4).reshape(16)
    g = eye.ctypes.data_as(C.POINTER(C.c_double))
    try:
        bad = [dict(resolution=0.0), dict(resolution=float("nan")), dict(resolution=-1.0), dict(step_size=0.0),
               dict(step_size=float("inf")), dict(outlier_ratio=0.0), dict(outlier_ratio=1.0), dict(transformation_epsilon=-1e-9),
               dict(maximum_iterations=-1), dict(min_points_per_voxel=2), dict(step_mode=2), dict(reserved=1)]
        for b in bad:
            o = dl.ndt_options(**b)
            assert L.dliom_ndt_target_create(ctx.h, cloud.h, C.byref(o), C.byref(h)) == dl.ERR_INVALID_ARGUMENT, b
        o = dl.ndt_options()
        assert L.dliom_ndt_target_create(other.h, cloud.h, C.byref(o), C.byref(h)) == dl.ERR_INVALID_ARGUMENT  # another context
        assert L.dliom_ndt_target_create(ctx.h, None, C.byref(o), C.byref(h)) == dl.ERR_INVALID_ARGUMENT
        target = dl.NdtTarget(ctx, cloud)
        foreign = dl.PointCloud(other, points[:50])
        foreign_index = dl.NnIndex(other, points[:50])
        try:
            for b in bad:
                o = dl.ndt_options(**b)
                assert L.dliom_ndt_align(target.h, cloud.h, g, C.byref(o), None, C.byref(r), None) == dl.ERR_INVALID_ARGUMENT, b
            o = dl.ndt_options()
            assert L.dliom_ndt_align(target.h, foreign.h, g, C.byref(o), None, C.byref(r), None) == dl.ERR_INVALID_ARGUMENT
            assert L.dliom_ndt_align(target.h, cloud.h, g, C.byref(o), foreign_index.h, C.byref(r), None) == dl.ERR_INVALID_ARGUMENT
            assert L.dliom_ndt_align(target.h, cloud.h, None, C.byref(o), None, C.byref(r), None) == dl.ERR_INVALID_ARGUMENT
            assert L.dliom_ndt_align(target.h, cloud.h, g, C.byref(o), None, None, None) == dl.ERR_INVALID_ARGUMENT
            o2 = dl.ndt_options(resolution=2.0)  # not the target's
            assert L.dliom_ndt_align(target.h, cloud.h, g, C.byref(o2), None, C.byref(r), None) == dl.ERR_INVALID_ARGUMENT
            for k, v in ((0, 2.0), (5, float("nan")), (12, 1e-3), (15, 2.0)):  # not rigid, not finite, a bad last row
                guess = eye.copy()
                guess[k] = v
                assert L.dliom_ndt_align(target.h, cloud.h, guess.ctypes.data_as(C.POINTER(C.c_double)), C.byref(o), None, C.byref(r),
                                         None) == dl.ERR_INVALID_ARGUMENT, k
            score, pairs, six, many = C.c_double(), C.c_int64(), np.zeros(6), np.zeros(36)
            p6, p36 = six.ctypes.data_as(C.POINTER(C.c_double)), many.ctypes.data_as(C.POINTER(C.c_double))
            assert L.dliom_ndt_evaluate(target.h, cloud.h, p6, C.byref(o), 3, C.byref(score), p6, p36, C.byref(pairs)) == \
                dl.ERR_INVALID_ARGUMENT
            assert L.dliom_ndt_evaluate(target.h, cloud.h, None, C.byref(o), 1, C.byref(score), p6, p36, C.byref(pairs)) == \
                dl.ERR_INVALID_ARGUMENT
            count = C.c_int64()
            cell = dl.NdtCell()
            assert L.dliom_ndt_target_cells(target.h, C.byref(cell), 1, C.byref(count)) == dl.ERR_CAPACITY and count.value > 1
        finally:
            foreign_index.close()
            foreign.close()
            target.close()
    finally:
        cloud.close()
        other.close()
